"""The cases tests/test_kv8_kernels_gpu.py runs the MX8 attention entries on (ll_decode_attn_rope_kv8, ll_suffix_attn_rope_kv8), in the style of
tests/attn_split_cases.py, whose case builder and range constants they use unchanged, with tests/attn_reference.py and tests/qknorm_reference.py.

The kernels are the key-split ones: ranges of 512 keys, so the edges that matter are slots 511 | 512 and 1023 | 1024.  The issue sets the cache
lengths: 64 (one partial range), 576 (two: the second of 64 keys), 1088 (three) and one case at 16448; suffix rows S = 9 at *pos = 508 of 576
(straddling the edge) and S = 16; head groups of 1, 2, 4 and 7; both head sizes; norm weights on and off; 1, 3 and 20 sequences.  Rows cycle
through full / left-padded / fully masked (attn_reference.decode_case), "longpad" pads by more than one range."""
from tests import attn_split_cases as SC

RANGE = SC.RANGE
GEOMETRIES = [(64, 4, 2), (128, 4, 4), (128, 8, 2), (128, 7, 1), (64, 7, 1)]      # D, nh, nkv: groups of 2, 1, 4, 7, 7
# maxlen, *pos, variants
DECODE_SHAPES = [(64, 63, ("plain",)),
                 (576, RANGE - 1, ("plain", "dom_pos", "dom_first")),
                 (576, RANGE, (f"dom_{RANGE - 1}", f"dom_{RANGE}", "dom_pos", "qzero")),
                 (1088, 1087, ("plain", "longpad", f"dom_{2 * RANGE - 1}", f"dom_{2 * RANGE}", "q8")),
                 (1088, 40, ("plain",))]                       # at 40 the two later ranges are fully masked
DECODE_CASES = [(D, nh, nkv, L, pos, v, 3) for D, nh, nkv in GEOMETRIES for L, pos, vs in DECODE_SHAPES for v in vs]
DECODE_CASES += [(64, 4, 2, 576, 575, "plain", 20), (128, 7, 1, 576, RANGE, "dom_pos", 20), (128, 8, 2, 1088, 1087, "dom_pos", 1),
                 (64, 7, 1, 64, 0, "plain", 1)]
LONG_CASE = (128, 8, 2, 16448, 16447, "plain", 3)
NORM_GEOMETRIES = [(128, 8, 2), (64, 7, 1), (64, 4, 2)]
NORM_SHAPES = [(576, RANGE - 1), (576, RANGE), (1088, 1087)]
NORM_VARIANTS = ("plain", "dom_pos")

SUFFIX_GEOMETRIES = [(64, 4, 2), (128, 8, 2), (128, 7, 1), (128, 4, 4)]
SUFFIX_SHAPES = [(9, 508), (16, 504), (16, 560)]             # S, *pos at 576 slots: across the edge 511 | 512 twice, and ending in the last slot
SUFFIX_BATCHES = (1, 2)
SUFFIX_NORM_GEOMETRIES = [(128, 8, 2), (64, 7, 1)]
SUFFIX_MAXLEN = 576


def decode_case(D, nh, nkv, maxlen, pos, variant, B):
    return SC.decode_case(D, nh, nkv, maxlen, pos, variant, B=B)
