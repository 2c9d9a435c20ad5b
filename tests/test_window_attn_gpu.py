"""The windowed key-split decode attention (ll_decode_attn_rope_win_bf16, ll_suffix_attn_rope_win_bf16, ll_attn_win_workspace_bytes) through the
C ABI, on the cases of tests/window_cases.py: windows 1 .. 5000 on a 1544-slot cache with *pos on either side of the edges of the 512-key
ranges, suffix rows across an edge and in the last slot, a dominant key the window hides, left padding that leaves a row without a visible
key, NaN in every slot the call may not read (the slots below the window included), and 16904 / 131072 slots with a window of 4096.

Every call is checked four ways: (1) every output element within attn_reference's bound (2^-8 |ref| + 2^-11 sum_j p_j |v_j|, unchanged) of the
float64 reference with the window ANDed into what a row sees; (2) output and caches bit for bit those of ll_*_attn_rope_split_bf16 called with
the window cut out of its mask on the host; (3) with window >= *pos + S, bit for bit the split entry on the plain mask; the cache compared bit
for bit with the expected rows.  The windowed entries are given the PLAIN mask: the window is theirs to apply.

Largest err / bound measured on an MI355X (-s prints them): ll_decode_attn_rope_win_bf16 0.885, with norm weights 0.673,
ll_suffix_attn_rope_win_bf16 0.885, with norm weights 0.877."""
import gc

import pytest
import torch

from tests import attn_reference as R
from tests import qknorm_reference as Q
from tests import window_cases as W

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(autouse=True)
def _release_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def lib():
    from llamole_amd import _lib
    yield _lib.load()
    for entry, r in sorted(WORST.items()):
        print(f"\nlargest err / bound, {entry}: {r:.3f}")


def _check(rc, what):
    from llamole_amd import _lib
    _lib.check(rc, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _nan(*shape):
    return torch.full(shape, R.NAN, dtype=R.BF, device="cuda")


def _within(entry, c, out, ref, absref):
    assert torch.isfinite(out.float()).all(), (entry, c.variant, c.window, "the output holds NaN / inf")
    r = R.err_over_bound(out, ref, absref)
    WORST[entry] = max(WORST.get(entry, 0.0), r)
    assert r <= 1.0, (entry, c.variant, c.window, c.pos, r)


def _workspace(lib, B, S, c, window=None):
    """a NaN-filled workspace of exactly the size the query names: nothing may be read that was not written"""
    if window is None:
        n = int(lib.ll_attn_split_workspace_bytes(B, S, c.nh, c.nkv, c.maxlen, c.D))
    else:
        n = int(lib.ll_attn_win_workspace_bytes(B, S, c.nh, c.nkv, c.maxlen, c.D, window))
        assert n == B * S * c.nh * W.ranges(S, c.maxlen, window) * (c.D + 2) * 4
    return torch.full((n // 2,), R.NAN, dtype=R.BF, device="cuda"), n


def _norm_args(c):
    if hasattr(c, "qw"):
        c._qw, c._kw = c.qw.cuda(), c.kw.cuda()
        return c._qw.data_ptr(), c._kw.data_ptr(), c.eps
    return None, None, 0.0


# ------------------------------------------------------------------------------------------------------------------ decode
def run_decode(lib, c, dev, Kc, Vc, mask, window=None):
    """the windowed entry (``window``) or the split entry (None) on the device inputs ``dev`` and the mask ``mask``"""
    qkv, cos, sin, pos = dev
    ws, n = _workspace(lib, c.B, 1, c, window)
    out = _nan(c.B, c.nh * c.D)
    head = (qkv.data_ptr(), c.ld_qkv, cos.data_ptr(), sin.data_ptr(), c.cs_stride, Kc.data_ptr(), Vc.data_ptr(), pos.data_ptr(), mask.data_ptr(),
            c.mask_stride, out.data_ptr(), c.B, c.nh, c.nkv, c.maxlen, c.D, c.scale, *_norm_args(c))
    if window is None:
        _check(lib.ll_decode_attn_rope_split_bf16(*head, ws.data_ptr(), n, _stream()), "ll_decode_attn_rope_split_bf16")
    else:
        _check(lib.ll_decode_attn_rope_win_bf16(*head, window, ws.data_ptr(), n, _stream()), "ll_decode_attn_rope_win_bf16")
    torch.cuda.synchronize()
    return out.cpu().view(c.B, c.nh, 1, c.D)


def check_decode(lib, c, entry="ll_decode_attn_rope_win_bf16", expected=R.decode_expected):
    """``c``: a case of window_cases.decode_window"""
    keep = c.visible.clone()
    keep[:, c.pos] = False                                       # the stale row at *pos; everything below the window is NaN as well
    Kp, Vp = R.poison(c, c.K0, c.V0, keep)
    dev = (c.qkv.cuda(), c.cos.cuda(), c.sin.cuda(), torch.tensor([c.pos], dtype=torch.long, device="cuda"))
    plain, cut = c.mask.cuda(), c.mask_w.cuda()
    Kw, Vw = Kp.cuda(), Vp.cuda()
    out = run_decode(lib, c, dev, Kw, Vw, plain, c.window)
    inputs, (k_rot, v_new) = expected(c)
    ref, absref = R.reference(c, inputs)
    Kp[:, :, c.pos], Vp[:, :, c.pos] = k_rot, v_new              # the appended row, every other slot as it was
    assert torch.equal(_bits(Kw), _bits(Kp)), (entry, c.variant, c.window, "key cache")
    assert torch.equal(_bits(Vw), _bits(Vp)), (entry, c.variant, c.window, "value cache")
    _within(entry, c, out, ref, absref)
    for b in range(c.B):
        if not c.visible[b].any():
            assert float(out[b].float().abs().max()) == 0.0, (entry, c.variant, c.window, "a row without a visible key is not zero")
    # the split entry with the window cut out of its mask on the host: bit for bit
    Kp2, Vp2 = R.poison(c, c.K0, c.V0, keep)
    Ks, Vs = Kp2.cuda(), Vp2.cuda()
    out_s = run_decode(lib, c, dev, Ks, Vs, cut)
    assert torch.equal(_bits(out), _bits(out_s)), (entry, c.variant, c.window, c.pos, "output differs from the split entry on the cut mask")
    assert torch.equal(_bits(Kw), _bits(Ks)) and torch.equal(_bits(Vw), _bits(Vs))
    if c.window >= c.pos + 1:                                     # the window cannot bind: the split entry on the plain mask
        Ks, Vs = Kp2.cuda(), Vp2.cuda()
        out_p = run_decode(lib, c, dev, Ks, Vs, plain)
        assert torch.equal(_bits(out), _bits(out_p)), (entry, c.variant, c.window, c.pos, "output differs from the split entry")
        assert torch.equal(_bits(Kw), _bits(Ks)) and torch.equal(_bits(Vw), _bits(Vs))
    return out


@pytest.mark.parametrize("pos", W.POSITIONS)
@pytest.mark.parametrize("D,nh,nkv", W.GEOMETRIES)
def test_window_decode_range_edges(lib, D, nh, nkv, pos):
    """four ranges (the last of eight keys); windows of 1 and 2 keys, on either side of one range, longer than the cache; a dominant first key
    that the window hides ("dom_first"), left padding of 700 slots ("longpad")"""
    hidden = 0
    for c in W.decode_cases(D, nh, nkv, W.SMALL, pos):
        check_decode(lib, c)
        hidden += len(c.hidden)
    assert hidden > 0                                             # some window did hide a dominant key


@pytest.mark.parametrize("D,nh,nkv", W.GEOMETRIES)
def test_window_decode_16904_slots(lib, D, nh, nkv):
    for c in W.decode_cases(D, nh, nkv, W.LONG, W.LONG - 1, ("plain", "dom_first"), (W.LONG_WINDOW,)):
        check_decode(lib, c)


@pytest.mark.parametrize("pos", W.HUGE_POSITIONS)
def test_window_decode_131072_slots(lib, pos):
    """*pos in the last slot: ranges 247 .. 255 of 256; *pos = 200: range 0 and eight empty partials"""
    for c in W.decode_cases(128, 2, 1, W.HUGE, pos, ("plain",), (W.LONG_WINDOW,), B=2):
        check_decode(lib, c)


def test_window_decode_20_sequences(lib):
    for c in W.decode_cases(64, 4, 2, W.SMALL, W.SMALL - 1, ("plain",), (600,), B=20):
        check_decode(lib, c)


@pytest.mark.parametrize("D,nh,nkv", [(128, 8, 2), (64, 7, 1)])
def test_window_decode_with_head_norms(lib, D, nh, nkv):
    """q_norm_w / k_norm_w given: the Qwen3 layout against tests/qknorm_reference.py"""
    for pos in (W.RANGE, W.SMALL - 1):
        for v in ("plain", "dom_pos"):
            base = Q.decode_case(D, nh, nkv, W.SMALL, pos, v)
            for window in (1, W.RANGE + 1, 5000):
                check_decode(lib, W.decode_window(base, window), "ll_decode_attn_rope_win_bf16 norms", Q.decode_expected)


# ------------------------------------------------------------------------------------------------------------------ suffix
def run_suffix(lib, c, qkv, pos, Kc, Vc, cos, sin, mask, window=None):
    ws, n = _workspace(lib, c.B, c.S, c, window)
    out = _nan(c.B * c.S, c.nh * c.D)
    head = (qkv.data_ptr(), c.ld_qkv, cos.data_ptr(), sin.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), pos.data_ptr(), mask.data_ptr(),
            out.data_ptr(), c.B, c.S, c.nh, c.nkv, c.maxlen, c.D, c.scale, *_norm_args(c))
    if window is None:
        _check(lib.ll_suffix_attn_rope_split_bf16(*head, ws.data_ptr(), n, _stream()), "ll_suffix_attn_rope_split_bf16")
    else:
        _check(lib.ll_suffix_attn_rope_win_bf16(*head, window, ws.data_ptr(), n, _stream()), "ll_suffix_attn_rope_win_bf16")
    torch.cuda.synchronize()
    return out


def check_suffix(lib, c, entry="ll_suffix_attn_rope_win_bf16", expected=W.suffix_expected_window):
    """``c``: a case of window_cases.suffix_window; cos / sin / mask come from ll_suffix_prologue, as in the model"""
    B, S, nh, D, L, rows = c.B, c.S, c.nh, c.D, c.maxlen, c.B * c.S
    inw = W.in_window(c.pos, S, L, c.window)                      # [S, L]
    keep = c.old & inw.any(0)[None, :]                            # old slots below every row's window are NaN too
    Kp, Vp = R.poison(c, c.K0, c.V0, keep)
    posid, freq, mask2d, qkv = c.position_ids.cuda(), c.inv_freq.cuda(), c.mask2d.cuda(), c.qkv.cuda()
    pos = torch.tensor([c.pos], dtype=torch.long, device="cuda")
    cos, sin = _nan(rows, D), _nan(rows, D)
    plain = torch.ones(rows, L, dtype=torch.bool, device="cuda")
    _check(lib.ll_suffix_prologue(posid.data_ptr(), freq.data_ptr(), 1.0, mask2d.data_ptr(), c.mask2d_stride, pos.data_ptr(), cos.data_ptr(),
                                  sin.data_ptr(), plain.data_ptr(), B, S, D, L, _stream()), "ll_suffix_prologue")
    cut = (plain.view(B, S, L) & inw.cuda()[None]).view(rows, L).contiguous()
    Kw, Vw = Kp.cuda(), Vp.cuda()
    out = run_suffix(lib, c, qkv, pos, Kw, Vw, cos, sin, plain, c.window)
    inputs, written = expected(c, cos.cpu().view(B, S, D), sin.cpu().view(B, S, D))
    ref, absref = R.reference(c, inputs)
    Kx, Vx = Kp.clone(), Vp.clone()
    Kx[:, :, written], Vx[:, :, written] = inputs[1][:, :, written], inputs[2][:, :, written]
    assert torch.equal(_bits(Kw), _bits(Kx)), (entry, c.variant, c.window, "key cache")
    assert torch.equal(_bits(Vw), _bits(Vx)), (entry, c.variant, c.window, "value cache")
    _within(entry, c, out.cpu().view(B, S, nh, D).transpose(1, 2), ref, absref)
    Ks, Vs = Kp.cuda(), Vp.cuda()
    out_s = run_suffix(lib, c, qkv, pos, Ks, Vs, cos, sin, cut)
    assert torch.equal(_bits(out), _bits(out_s)), (entry, c.variant, c.window, c.pos, "output differs from the split entry on the cut mask")
    assert torch.equal(_bits(Kw), _bits(Ks)) and torch.equal(_bits(Vw), _bits(Vs))
    if c.window >= c.pos + S:
        Ks, Vs = Kp.cuda(), Vp.cuda()
        out_p = run_suffix(lib, c, qkv, pos, Ks, Vs, cos, sin, plain)
        assert torch.equal(_bits(out), _bits(out_p)), (entry, c.variant, c.window, c.pos, "output differs from the split entry")
        assert torch.equal(_bits(Kw), _bits(Ks)) and torch.equal(_bits(Vw), _bits(Vs))


@pytest.mark.parametrize("S,B", W.SUFFIX_ROWS)
@pytest.mark.parametrize("D,nh,nkv", W.GEOMETRIES)
def test_window_suffix_across_a_range_edge(lib, D, nh, nkv, S, B):
    """S new rows per sequence whose slots cross the edge 511 | 512, start on it, or end in the last slot of the cache"""
    hidden = 0
    for pos in W.SC.suffix_positions(S):
        for v in R.SUFFIX_VARIANTS:
            base = R.suffix_case(D, nh, nkv, B, S, W.SMALL, pos, v)
            for window in W.WINDOWS:
                c = W.suffix_window(base, window)
                check_suffix(lib, c)
                hidden += len(c.hidden)
    assert hidden > 0


def test_window_suffix_16904_slots_and_past_the_end(lib):
    for S, pos in ((9, W.LONG - 9), (16, W.LONG - 5)):             # the second: eleven rows past the last slot are not stored
        for v in R.SUFFIX_VARIANTS:
            check_suffix(lib, W.suffix_window(R.suffix_case(128, 8, 2, 2, S, W.LONG, pos, v), W.LONG_WINDOW))


def test_window_suffix_with_head_norms(lib):
    for S, B in ((9, 1), (3, 5)):
        for pos in (W.RANGE - 1 - S // 2, W.SMALL - S):
            for v in ("plain", "dom_own"):
                base = Q.suffix_case(128, 8, 2, B, S, W.SMALL, pos, v)
                for window in (2, 600):
                    c = W.suffix_window(base, window)
                    check_suffix(lib, c, "ll_suffix_attn_rope_win_bf16 norms",
                                 lambda c, cos, sin: W.suffix_expected_window(Q.normed(c), cos, sin))


# ------------------------------------------------------------------------------------------------------------------ bounds
def test_workspace_query(lib):
    q = lib.ll_attn_win_workspace_bytes
    for B, S, nh, nkv, L, D, w in ((1, 1, 32, 8, 131072, 128, 4096), (3, 16, 4, 2, W.SMALL, 64, 1), (2, 9, 7, 1, W.LONG, 128, 600),
                                   (1, 1, 2, 1, 600, 128, 4096), (64, 1, 28, 4, 32768, 128, 2 ** 31 - 1)):
        assert int(q(B, S, nh, nkv, L, D, w)) == B * S * nh * W.ranges(S, L, w) * (D + 2) * 4
    # a window of 4096 on 131072 slots: 9 ranges instead of 256
    assert 0 < int(q(1, 1, 32, 8, 131072, 128, 4096)) < int(lib.ll_attn_split_workspace_bytes(1, 1, 32, 8, 131072, 128))
    assert int(q(1, 1, 32, 8, 131072, 128, 4096)) * 256 == int(lib.ll_attn_split_workspace_bytes(1, 1, 32, 8, 131072, 128)) * 9
    # a window the cache cannot fill: the split entries' size
    assert int(q(1, 1, 4, 2, 1024, 64, 5000)) == int(lib.ll_attn_split_workspace_bytes(1, 1, 4, 2, 1024, 64))


def test_arguments_out_of_bounds_are_refused(lib):
    """LL_EINVAL from both entry points and -1 from the workspace query, nothing launched: outputs, cache and workspace (all the same few
    zero bytes) stay as they were"""
    D = 128
    t = torch.zeros(4096, dtype=R.BF, device="cuda")
    pos = torch.zeros(1, dtype=torch.long, device="cuda")
    p, st, pp, sc = t.data_ptr(), _stream(), pos.data_ptr(), D ** -0.5
    dec, suf, q = lib.ll_decode_attn_rope_win_bf16, lib.ll_suffix_attn_rope_win_bf16, lib.ll_attn_win_workspace_bytes
    big = 1 << 40

    def d(B=1, nh=2, nkv=1, L=1024, D=D, qn=None, kn=None, eps=0.0, window=64, ws=p, n=big, ld=4 * D):
        return dec(p, ld, p, p, 0, p, p, pp, p, L, p, B, nh, nkv, L, D, sc, qn, kn, eps, window, ws, n, st)

    def s(B=1, S=2, nh=2, nkv=1, L=1024, D=D, window=64, ws=p, n=big, ld=4 * D):
        return suf(p, ld, p, p, p, p, pp, p, p, B, S, nh, nkv, L, D, sc, None, None, 0.0, window, ws, n, st)

    rc = [d(window=0), d(window=-1), d(window=-2 ** 31), s(window=0), s(window=-7),                  # the window
          d(L=W.HUGE + 1), s(L=W.HUGE + 1), d(L=0), d(B=65), d(B=0), s(S=17), s(S=0), d(D=96), s(D=96),   # the split entries' bounds
          d(nh=3, nkv=2), d(nkv=0), d(ld=4 * D + 4), s(ld=4 * D + 4),
          d(qn=p, eps=1e-6), d(kn=p, eps=1e-6), d(qn=p, kn=p, eps=0.0),                              # one norm weight only; eps
          d(n=64), s(n=64), d(ws=p + 2), d(ws=None),                                                 # a small / misaligned / missing workspace
          int(q(1, 1, 2, 1, 1024, D, 0)), int(q(1, 1, 2, 1, 1024, D, -1)), int(q(1, 1, 2, 1, W.HUGE + 1, D, 64)),
          int(q(1, 17, 2, 1, 1024, D, 64)), int(q(1, 1, 2, 1, 1024, 96, 64)), int(q(0, 1, 2, 1, 1024, D, 64))]
    torch.cuda.synchronize()
    assert rc == [-1] * len(rc)
    assert float(t.float().abs().max()) == 0.0 and int(pos) == 0
    # the same few bytes are a valid call once the arguments are in bounds (a 1-slot cache, one row): it is the arguments that were refused
    assert int(q(1, 1, 2, 1, 1, D, 1)) == 2 * (D + 2) * 4
