"""The cases both tests of the windowed key-split decode attention run on (tests/test_window_reference_cpu.py without a GPU,
tests/test_window_attn_gpu.py through the C ABI): the cases of tests/attn_reference.py / tests/attn_split_cases.py with a sliding window ANDed
into what a query row sees.  HF's sliding_window_causal_mask_function over cache slots: key j is visible to the query row at slot p iff the
case's own mask shows it and j > p - window.  The geometry of the two launches is stated here in Python (``ranges`` / ``first_range``) the way
include/llamole_hip.h documents it."""
import copy

import torch

from tests import attn_reference as R
from tests import attn_split_cases as SC

RANGE = SC.RANGE
SMALL = SC.SMALL                                                   # 1544 slots: four ranges, the last one of eight keys
WINDOWS = [1, 2, RANGE - 1, RANGE, RANGE + 1, 600, SMALL - 1, SMALL, 5000]
POSITIONS = [40, RANGE - 1, RANGE, RANGE + 1, 2 * RANGE - 1, 2 * RANGE, SMALL - 1]
GEOMETRIES = SC.GEOMETRIES
VARIANTS = ["plain", "qzero", "dom_pos", "dom_first", "longpad"]
SUFFIX_ROWS = [(1, 1), (9, 1), (16, 2)]                            # S, B
LONG, LONG_WINDOW = SC.LONG, 4096                                  # 16904 slots
HUGE = SC.SPLIT_LIMIT                                              # 131072 slots
HUGE_POSITIONS = [HUGE - 1, 200]


def ranges(S, maxlen, window):
    """nrw: ranges of 512 slots per (head group, row) of the partial launch -- a function of the shapes and the window only"""
    return min(-(-maxlen // RANGE), -(-(window + S - 2) // RANGE) + 1)


def first_range(pos, window):
    """the absolute range workgroup x = 0 takes, computed on the device from *pos"""
    return max(0, pos - window + 1) // RANGE


def in_window(pos, S, maxlen, window):
    """bool [S, maxlen]: slot j lies in the window of the query row at slot pos + s"""
    j = torch.arange(maxlen)[None, :]
    return j > (pos + torch.arange(S))[:, None] - window


def decode_window(c, window):
    """A decode case (attn_reference.decode_case / attn_split_cases.decode_case) seen through a window: ``visible`` is cut to the window, the
    dominant keys the window hides are dropped from ``dominant`` (they must vanish from the result: the reference no longer sees them) and kept
    in ``hidden``; ``mask`` stays the plain mask the windowed entry is given, ``mask_w`` is the one with the window cut out on the host."""
    w = copy.copy(c)
    inw = in_window(c.pos, 1, c.maxlen, window)                    # [1, L]
    w.window = window
    w.visible = c.visible & inw
    w.mask_w = c.mask.clone()
    w.mask_w[:, :c.maxlen] &= inw
    w.dominant = [d for d in c.dominant if bool(inw[0, d[2]])]
    w.hidden = [d for d in c.dominant if not bool(inw[0, d[2]])]
    return w


def suffix_window(c, window):
    """A suffix case seen through a window: ``suffix_expected_window`` cuts the mask, the dominant keys outside their row's window are dropped."""
    w = copy.copy(c)
    inw = in_window(c.pos, c.S, c.maxlen, window)                  # [S, L]
    w.window = window
    w.dominant = [d for d in c.dominant if bool(inw[d[1], d[2]])]
    w.hidden = [d for d in c.dominant if not bool(inw[d[1], d[2]])]
    return w


def suffix_expected_window(c, cos=None, sin=None):
    (q_rot, K, V, mask), written = R.suffix_expected(c, cos, sin)
    return (q_rot, K, V, mask & in_window(c.pos, c.S, c.maxlen, c.window)[None]), written


def decode_cases(D, nh, nkv, maxlen, pos, variants=VARIANTS, windows=WINDOWS, B=3):
    """every (variant, window) of one geometry and position: the inputs of a variant are built once and shared by its windows.  "longpad" runs at
    every position: where the padding (700 slots) reaches past *pos the padded row has no visible key at all, behind it the window cuts into it"""
    for v in variants:
        c = SC.decode_case(D, nh, nkv, maxlen, pos, v, B=B)
        for window in windows:
            yield decode_window(c, window)
