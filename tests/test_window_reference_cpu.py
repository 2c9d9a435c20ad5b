"""The reference and the launch geometry of the windowed key-split decode attention, without a GPU.

  * the float64 reference of tests/attn_reference.py with the window ANDed into ``visible`` (tests/window_cases.py) equals a direct softmax over
    the last ``window`` slots of each row;
  * the geometry of include/llamole_hip.h -- nrw = min(ceil(maxlen/512), ceil((window + S - 2)/512) + 1) ranges starting at the absolute range
    first = max(0, *pos - window + 1) / 512 -- covers every slot a window shows, for every position of a 1544-slot cache, every window up to
    past the cache and 1 / 9 / 16 new rows, and is never larger than the split entries' ceil(maxlen/512)."""
import numpy as np
import pytest
import torch

from tests import attn_reference as R
from tests import window_cases as W


@pytest.mark.parametrize("D,nh,nkv", [(64, 4, 2), (128, 7, 1)])
@pytest.mark.parametrize("pos,window", [(W.SMALL - 1, 600), (W.RANGE, 1), (W.RANGE + 1, W.RANGE), (40, 5000), (2 * W.RANGE, 2)])
def test_windowed_reference_is_a_softmax_over_the_last_window_slots(D, nh, nkv, pos, window):
    c = W.decode_window(R.decode_case(D, nh, nkv, W.SMALL, pos, "plain"), window)
    (q_rot, K, V, mask), _ = R.decode_expected(c)
    ref, _ = R.reference(c)
    G = nh // nkv
    lo = max(0, pos - window + 1)
    for b in range(c.B):
        start = max(lo, c.pads[b])
        if b % 3 == 2 or start > pos:                              # a fully masked row, or padding that reaches past the window
            assert float(ref[b].abs().max()) == 0.0
            continue
        assert bool(mask[b, 0, start:pos + 1].all()) and int(mask[b, 0].sum()) == pos + 1 - start
        for h in range(nh):
            k, v = K[b, h // G, start:pos + 1].double(), V[b, h // G, start:pos + 1].double()
            p = torch.softmax(c.scale * (k @ q_rot[b, h, 0].double()), dim=0)
            torch.testing.assert_close(ref[b, h, 0], p @ v, rtol=1e-12, atol=1e-12)


def test_a_window_hides_the_dominant_first_key_and_long_padding_empties_a_row():
    pos = W.SMALL - 1
    c = W.SC.decode_case(128, 4, 4, W.SMALL, pos, "dom_first")
    assert c.dominant
    w = W.decode_window(c, 600)
    assert not w.dominant and len(w.hidden) == len(c.dominant)      # every dominant key sits at the left edge: outside the window
    R.reference(w)
    full, _ = R.reference(c)
    cut, _ = R.reference(w)
    b = c.dominant[0][0]
    assert float((full[b] - cut[b]).abs().max()) > 1.0              # the value row of the dominant key (4 .. 11.5) has left the result
    # left padding longer than the window that reaches up to the position: the row sees nothing, its neighbour the last 50 slots
    lp = W.decode_window(W.SC.decode_case(64, 4, 2, W.SMALL, W.RANGE + 1, "longpad"), 50)
    ref, _ = R.reference(lp)
    assert W.SC.LONG_PAD > W.RANGE + 1 and not lp.visible[1].any() and int(lp.visible[0].sum()) == 50
    assert float(ref[1].abs().max()) == 0.0 and float(ref[0].abs().max()) > 0.0


@pytest.mark.parametrize("S", [1, 9, 16])
def test_geometry_covers_every_visible_slot_exhaustively_at_1544_slots(S):
    L = W.SMALL
    pos = np.arange(0, L - S + 1, dtype=np.int64)[:, None]         # every position at which the S new rows fit
    window = np.arange(1, L + 600, dtype=np.int64)[None, :]
    nr = -(-L // W.RANGE)
    nrw = np.minimum(nr, -(-(window + S - 2) // W.RANGE) + 1)
    first = np.maximum(0, pos - window + 1) // W.RANGE
    low = np.maximum(0, pos - window + 1)                          # the lowest slot row s = 0 sees
    high = pos + S - 1                                             # the highest slot row s = S - 1 sees: its own
    assert (first <= low // W.RANGE).all()
    assert (high // W.RANGE < first + nrw).all()
    assert (nrw >= 1).all() and (nrw <= nr).all()
    # the scalar statement the tests use agrees with the vectorised one
    for p, w in ((0, 1), (511, 1), (512, 2), (1543 - S + 1, 600), (1000, 2000), (1543 - S + 1, 513)):
        assert W.ranges(S, L, w) == int(nrw[0, w - 1]) and W.first_range(p, w) == int(first[p, w - 1])


def test_geometry_covers_the_case_list():
    for L, positions, windows in ((W.SMALL, W.POSITIONS, W.WINDOWS), (W.LONG, [W.LONG - 1], [W.LONG_WINDOW]),
                                  (W.HUGE, W.HUGE_POSITIONS, [W.LONG_WINDOW])):
        for S, _ in W.SUFFIX_ROWS:
            for pos in positions:
                for window in windows:
                    if pos + S > L:
                        continue
                    seen = W.in_window(pos, S, L, window) & (torch.arange(L)[None, :] <= (pos + torch.arange(S))[:, None])
                    idx = seen.any(0).nonzero().flatten()
                    first, nrw = W.first_range(pos, window), W.ranges(S, L, window)
                    assert first <= int(idx.min()) // W.RANGE and int(idx.max()) // W.RANGE < first + nrw, (L, S, pos, window)


def test_the_window_saves_ranges_at_long_caches():
    assert W.ranges(1, 32768, 4096) == 9 and W.ranges(16, 32768, 4096) == 10 and W.ranges(1, 131072, 4096) == 9
    assert W.ranges(1, 600, 4096) == 2 and W.ranges(1, 1, 1) == 1 and W.ranges(1, W.SMALL, 1) == 1 and W.ranges(1, W.SMALL, 2) == 2
