"""The cases both tests of the key-split decode attention run on (tests/test_attn_split_reference_cpu.py without a GPU,
tests/test_attn_split_gpu.py through the C ABI), built with tests/attn_reference.py unchanged.  RANGE is the kernel's range length: the keys of
a cache are cut into ranges of 512 slots, so the edges that matter are slots 511 | 512 and 1023 | 1024, and the entry points' own limit."""
from tests import attn_reference as R

RANGE = 512
SPLIT_LIMIT = 131072
SMALL = 3 * RANGE + 8            # 1544 slots: four ranges, the last one of eight keys
LONG = R.MAXLEN_LIMIT + RANGE + 8                                # 16904
GEOMETRIES = [(64, 4, 2), (128, 4, 4), (128, 8, 2), (128, 7, 1)]    # D, nh, nkv: groups of 2, 1, 4, 7
SMALL_POSITIONS = [SMALL - 1, RANGE - 1, RANGE, RANGE + 1, 40]     # at 40 every later range is fully masked
VARIANTS = ["plain", "qzero", "q8", "dom_first", "dom_pos", f"dom_{RANGE - 1}", f"dom_{RANGE}", f"dom_{2 * RANGE - 1}", "longpad"]
LONG_VARIANTS = ["plain", "dom_pos", "dom_first", f"dom_{RANGE}", "longpad"]
LONG_PAD = RANGE + 188           # left padding longer than one range
HUGE_CASES = [(128, 2, 1, SPLIT_LIMIT - 1, "plain"), (128, 2, 1, SPLIT_LIMIT - 1, "qzero"), (128, 2, 1, SPLIT_LIMIT - 1, "dom_pos"),
              (64, 4, 2, SPLIT_LIMIT - 1, "plain"), (64, 4, 2, SPLIT_LIMIT - 1, f"dom_{2 * RANGE - 1}"),
              (128, 2, 1, 200, "plain")]                         # D, nh, nkv, *pos, variant at 131072 slots; *pos = 200: 255 of 256 ranges masked

SUFFIX_GEOMETRIES = [(64, 4, 2), (128, 8, 2), (128, 7, 1)]
SUFFIX_ROWS = [(1, 1), (9, 1), (16, 1), (1, 2), (9, 2), (16, 2)]            # S, B


def suffix_positions(S):
    """the new rows cross the edge 511 | 512 (or sit on either side of it), and end in the last slot of the cache"""
    return sorted({RANGE - 1 - S // 2, RANGE - S, RANGE, SMALL - S})


def fits(variant, pos):
    if variant == "longpad":
        return pos > LONG_PAD + 8
    if variant.startswith("dom_") and variant[4:].isdigit():
        return int(variant[4:]) <= pos
    return True


def decode_case(D, nh, nkv, maxlen, pos, variant="plain", B=3, **kw):
    """attn_reference.decode_case; "longpad": the plain case with the left-padded rows padded by LONG_PAD slots (more than one range)."""
    if variant != "longpad":
        return R.decode_case(D, nh, nkv, maxlen, pos, variant, B=B, **kw)
    c = R.decode_case(D, nh, nkv, maxlen, pos, "plain", B=B, **kw)
    for b in range(B):
        if b % 3 == 1:
            c.pads[b] = LONG_PAD
            c.visible[b, :LONG_PAD] = False
            c.mask[b, :LONG_PAD] = False
    c.variant = variant
    return c

