"""The cases whose output and cache bits tests/golden/attn_bits.npz pins (tests/golden/make_attn_bits.py records them,
tests/test_attn_bits_gpu.py compares): every decode attention entry point at the smallest shapes that reach each kernel instance and each tile
or range edge, variant "plain".  The inputs are the seeded cases of attn_reference / qknorm_reference / attn_split_cases, the calls the run_*
helpers of the three GPU test files; nothing here generates data of its own."""
import hashlib

import torch

from tests import attn_reference as R
from tests import attn_split_cases as SC
from tests import qknorm_reference as Q

GROUPED = [(64, 4, 2), (128, 8, 2), (128, 7, 1), (64, 7, 1)]         # D, nh, nkv: groups of 2, 4 and 7, both wave counts, both D
SUFFIX = [(64, 4, 2, 2, 5, 300, 254), (128, 7, 1, 1, 9, 300, 250)]   # D, nh, nkv, B, S, maxlen, pos: the rows straddle key 256
SPLIT_POS, SPLIT_SUFFIX_POS = SC.RANGE, SC.RANGE - 4                 # 512; 508: nine rows cross the range edge 511 | 512


def _cases():
    """name -> (entry, builder of the case)"""
    out = {}
    for D, nh, nkv in [(64, 4, 2), (128, 6, 2)]:
        out[f"decode-{D}-{nh}-{nkv}"] = ("decode", lambda a=(D, nh, nkv): R.decode_case(*a, 300, 256, B=3))
        out[f"decode_qkn-{D}-{nh}-{nkv}"] = ("decode_qkn", lambda a=(D, nh, nkv): Q.decode_case(*a, 300, 256, B=3))
    for D, nh, nkv in GROUPED:
        out[f"grouped-{D}-{nh}-{nkv}"] = ("decode", lambda a=(D, nh, nkv): R.decode_case(*a, 300, 256, B=17))
        out[f"grouped_qkn-{D}-{nh}-{nkv}"] = ("decode_qkn", lambda a=(D, nh, nkv): Q.decode_case(*a, 300, 256, B=17))
    for a in SUFFIX:
        tag = "-".join(map(str, a))
        out[f"suffix-{tag}"] = ("suffix", lambda a=a: R.suffix_case(*a))
        out[f"suffix_qkn-{tag}"] = ("suffix_qkn", lambda a=a: Q.suffix_case(*a))
    out["attn-128-7-1"] = ("attn", lambda: R.attn_case(128, 7, 1, 5, 300, 254))
    for D, nh, nkv in SC.GEOMETRIES:
        out[f"split-{D}-{nh}-{nkv}"] = ("split", lambda a=(D, nh, nkv): SC.decode_case(*a, SC.SMALL, SPLIT_POS, B=3))
    for D, nh, nkv in [(128, 8, 2), (64, 4, 2)]:
        out[f"split_norms-{D}-{nh}-{nkv}"] = ("split", lambda a=(D, nh, nkv): Q.decode_case(*a, SC.SMALL, SPLIT_POS, B=3))
    for D, nh, nkv in [(64, 4, 2), (128, 7, 1)]:
        out[f"split_suffix-{D}-{nh}-{nkv}"] = ("split_suffix", lambda a=(D, nh, nkv): R.suffix_case(*a, 2, 9, SC.SMALL, SPLIT_SUFFIX_POS))
    out["split_suffix_norms-128-7-1"] = ("split_suffix", lambda: Q.suffix_case(128, 7, 1, 2, 9, SC.SMALL, SPLIT_SUFFIX_POS))
    return out


CASES = _cases()


def input_digest(c):
    """sha256 over every field of the case (names, scalars, the dtype, shape and bytes of every tensor)"""
    h = hashlib.sha256()
    for name, v in sorted(vars(c).items()):
        if name.startswith("_"):
            continue
        h.update(name.encode())
        if torch.is_tensor(v):
            h.update(f"{v.dtype}{tuple(v.shape)}".encode())
            h.update(v.contiguous().view(torch.uint8).numpy().tobytes())
        else:
            h.update(repr(v).encode())
    return h.hexdigest()


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def run(lib, name):
    """the case's input digest and the int16 bits of its output and of the K / V rows at the slots pos .. pos + S - 1 after the call"""
    from tests import test_attn_split_gpu as split_t
    from tests import test_decode_attention_reference_gpu as plain_t
    from tests import test_qknorm_attention_gpu as qkn_t
    entry, build = CASES[name]
    c = build()
    Kc, Vc = c.K0.cuda(), c.V0.cuda()
    if entry == "decode":
        out = plain_t.run_decode(lib, c, Kc, Vc)
    elif entry == "decode_qkn":
        rc, out = qkn_t.run_decode(lib, c, Kc, Vc)
        qkn_t._check(rc, name)
    elif entry == "attn":
        out = plain_t.run_attn(lib, c, Kc, Vc)
    elif entry == "split":
        out = split_t.run_decode(lib, c, Kc, Vc)
    else:
        cos, sin, mask = plain_t.run_prologue(lib, c)
        if entry == "suffix":
            out = plain_t.run_suffix(lib, c, Kc, Vc, cos, sin, mask)
        elif entry == "suffix_qkn":
            rc, out = qkn_t.run_suffix(lib, c, Kc, Vc, cos, sin, mask)
            qkn_t._check(rc, name)
        else:
            out = split_t.run_suffix(lib, c, Kc, Vc, cos, sin, mask)
    rows = slice(c.pos, c.pos + c.S)
    return {"in": input_digest(c), "out": _bits(out), "k": _bits(Kc[:, :, rows]), "v": _bits(Vc[:, :, rows])}
