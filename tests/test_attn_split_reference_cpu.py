"""The contract of the key-split decode attention (ll_decode_attn_rope_split_bf16, ll_suffix_attn_rope_split_bf16; include/llamole_hip.h),
emulated in torch without a GPU on the inputs tests/test_attn_split_gpu.py hands to the kernels: per range of keys the maximum m, the sum of
exponentials l and the un-normalised output in f32, then the combine with exp(m_r - M) and ONE rounding to bf16.  The correct emulation stays
inside the bound of tests/attn_reference.py (2^-8 |ref| + 2^-11 sum_j p_j |v_jd|, unchanged) on every case; each mistake such a kernel can make
leaves it on the case built to catch it (one dominant key on a range edge: random data cannot show one lost key among thousands).
Of the GPU test's inputs this file evaluates every four-range decode case, two geometries at 16385 / 16904 slots, two of the six 131072-slot
cases (the float64 reference of the others takes seconds each) and the suffix rows of one geometry; the cases with norm weights are not
emulated here (tests/test_qknorm_reference_cpu.py covers the norm; the split changes nothing in front of the rotation).

How many f32 terms one accumulator of the kernel sums at 131072 keys (the bound's f32 term allows roughly 2^13 sequential additions):
  P.V, D = 128: a lane sees 512 / (8 waves x 4 rows per load) = 16 rows of its range, 4 row groups are added across lanes, 8 waves through LDS,
       then the combine adds 256 / 4 = 64 ranges per slice and 4 slices:                          16 + 4 + 8 + 64 + 4 =  96 terms
  P.V, D = 64:  8 rows, 8 row groups, 8 waves, 256 / 8 = 32 ranges per slice, 8 slices:          8 + 8 + 8 + 32 + 8 =  64 terms
  l:   one exponential per thread, a wave sum (6 levels), 8 waves, then a wave sum and 8 waves over the 256 ranges:  about 28 levels
So at most 96 additions stand where 2^13 = 8192 are allowed (and a dot product of D <= 128 terms per score, as in the one-workgroup kernels)."""
import math

import pytest
import torch

from tests import attn_reference as R
from tests import attn_split_cases as SC


def emulate_split(q_rot, K, V, mask, scale, nh, nkv, rng=SC.RANGE, mistake=None):
    """f32 throughout.  mistake: no_rescale | den_no_rescale | empty_nan | empty_weighs | drop_last | drop_first"""
    idx = torch.arange(nh) // (nh // nkv)
    out = torch.empty(q_rot.shape, dtype=R.BF)
    sc = torch.tensor(scale, dtype=torch.float32)
    L = K.shape[2]
    for b in range(q_rot.shape[0]):
        Kh, Vh = torch.nan_to_num(K[b].float())[idx], torch.nan_to_num(V[b].float())[idx]
        ms, ls, accs = [], [], []
        for j0 in range(0, L, rng):
            j1 = min(j0 + rng, L)
            mk = mask[b][None, :, j0:j1].clone()                         # [1,S,n]
            if mistake == "drop_last":
                mk[..., -1] = False
            if mistake == "drop_first" and j0 > 0:
                mk[..., 0] = False
            s = (q_rot[b].float() @ Kh[:, j0:j1].transpose(-1, -2)) * sc
            s = s.masked_fill(~mk, -math.inf)
            m = s.amax(-1, keepdim=True)
            empty = ~torch.isfinite(m)
            if mistake == "empty_nan":
                e = torch.exp(s - m)                                       # -inf - -inf
            elif mistake == "empty_weighs":
                e = torch.where(empty, torch.ones_like(s), torch.exp(s - torch.where(empty, torch.zeros_like(m), m)))
                m = torch.where(empty, torch.zeros_like(m), m)            # a maximum that starts at 0
            else:
                e = torch.exp(s - torch.where(empty, torch.zeros_like(m), m))
            ms.append(m)
            ls.append(e.sum(-1, keepdim=True))
            accs.append(e @ Vh[:, j0:j1])
        m, l, acc = torch.stack(ms), torch.stack(ls), torch.stack(accs)    # [nr,nh,S,1|D]
        M = m.amax(0, keepdim=True)
        if mistake == "empty_nan":
            w = torch.exp(m - M)
        else:
            w = torch.where(torch.isfinite(m), torch.exp(m - torch.where(torch.isfinite(M), M, torch.zeros_like(M))), torch.zeros_like(m))
        wn = wd = w
        if mistake == "no_rescale":
            wn = wd = torch.isfinite(m).float()
        if mistake == "den_no_rescale":
            wd = torch.isfinite(m).float()
        num = (wn * torch.where(wn != 0, acc, torch.zeros_like(acc))).sum(0) if mistake != "empty_nan" else (wn * acc).sum(0)
        den = (wd * l).sum(0)
        inv = torch.where(den > 0, 1.0 / den, torch.zeros_like(den)) if mistake != "empty_nan" else 1.0 / den
        out[b] = (num * inv).to(R.BF)
    return out


def ratio(c, inputs, ref, **kw):
    return R.err_over_bound(emulate_split(*inputs, c.scale, c.nh, c.nkv, **kw), *ref)


def case_ref(c):
    inputs = R.expected(c)[0]
    return inputs, R.reference(c, inputs)


# ------------------------------------------------------------------------------------------------------------------ the correct emulation passes
@pytest.mark.parametrize("pos", SC.SMALL_POSITIONS)
@pytest.mark.parametrize("D,nh,nkv", SC.GEOMETRIES)
def test_split_emulation_is_inside_the_bound(D, nh, nkv, pos):
    for v in SC.VARIANTS:
        if not SC.fits(v, pos):
            continue
        c = SC.decode_case(D, nh, nkv, SC.SMALL, pos, v)
        inputs, ref = case_ref(c)
        for rng in (SC.RANGE, 2 * SC.RANGE):
            r = ratio(c, inputs, ref, rng=rng)
            assert r <= 1.0, (v, rng, r)
        got = emulate_split(*inputs, c.scale, c.nh, c.nkv)
        assert float(got[2].float().abs().max()) == 0.0            # the fully masked row: exact zeros


@pytest.mark.parametrize("maxlen", [R.MAXLEN_LIMIT + 1, SC.LONG])
@pytest.mark.parametrize("D,nh,nkv", [(64, 4, 2), (128, 7, 1)])
def test_split_emulation_beyond_16384_keys(D, nh, nkv, maxlen):
    for v in ("plain", f"dom_{SC.RANGE}", "longpad"):
        c = SC.decode_case(D, nh, nkv, maxlen, maxlen - 1, v)
        inputs, ref = case_ref(c)
        assert ratio(c, inputs, ref) <= 1.0, v


@pytest.mark.parametrize("D,nh,nkv,pos,variant", [SC.HUGE_CASES[0], SC.HUGE_CASES[-1]])
def test_split_emulation_at_131072_slots(D, nh, nkv, pos, variant):
    c = SC.decode_case(D, nh, nkv, SC.SPLIT_LIMIT, pos, variant)
    inputs, ref = case_ref(c)
    for rng in (SC.RANGE, 8192):
        assert ratio(c, inputs, ref, rng=rng) <= 1.0, rng


@pytest.mark.parametrize("S,B", [(9, 1), (16, 2)])
def test_split_emulation_on_suffix_rows(S, B):
    for pos in SC.suffix_positions(S):
        for v in R.SUFFIX_VARIANTS:
            c = R.suffix_case(128, 8, 2, B, S, SC.SMALL, pos, v)
            inputs, ref = case_ref(c)
            assert ratio(c, inputs, ref) <= 1.0, (pos, v)


# ------------------------------------------------------------------------------------------------------------------ the mistakes do not
@pytest.mark.parametrize("D,nh,nkv", SC.GEOMETRIES)
def test_combining_without_the_rescale_fails(D, nh, nkv):
    for v, pos in (("q8", SC.SMALL - 1), ("dom_pos", SC.SMALL - 1), (f"dom_{SC.RANGE}", SC.SMALL - 1), ("dom_first", SC.RANGE + 1)):
        c = SC.decode_case(D, nh, nkv, SC.SMALL, pos, v)
        inputs, ref = case_ref(c)
        assert ratio(c, inputs, ref) <= 1.0
        assert ratio(c, inputs, ref, mistake="no_rescale") > 1.0, (v, "numerator and denominator without exp(m_r - M)")
        assert ratio(c, inputs, ref, mistake="den_no_rescale") > 1.0, (v, "the denominators summed without the rescale")


@pytest.mark.parametrize("D,nh,nkv", SC.GEOMETRIES)
def test_a_range_without_a_visible_key_must_not_contribute(D, nh, nkv):
    """*pos = 40 in a cache of four ranges: three of them are fully masked (and hold NaN on the GPU)"""
    for v in ("plain", "dom_pos", "qzero"):
        c = SC.decode_case(D, nh, nkv, SC.SMALL, 40, v)
        inputs, ref = case_ref(c)
        assert ratio(c, inputs, ref) <= 1.0
        assert ratio(c, inputs, ref, mistake="empty_nan") == math.inf, (v, "-inf - -inf")
        assert ratio(c, inputs, ref, mistake="empty_weighs") > 1.0, (v, "an empty range with weight 1")


@pytest.mark.parametrize("D,nh,nkv", SC.GEOMETRIES)
def test_a_key_lost_on_a_range_edge_fails(D, nh, nkv):
    for j, mistake in ((SC.RANGE - 1, "drop_last"), (2 * SC.RANGE - 1, "drop_last"), (SC.RANGE, "drop_first")):
        c = SC.decode_case(D, nh, nkv, SC.SMALL, SC.SMALL - 1, f"dom_{j}")
        inputs, ref = case_ref(c)
        assert ratio(c, inputs, ref) <= 1.0
        assert ratio(c, inputs, ref, mistake=mistake) > 1.0, (j, mistake)
    # the new key itself on either side of an edge
    for pos, mistake in ((SC.RANGE - 1, "drop_last"), (SC.RANGE, "drop_first")):
        c = SC.decode_case(D, nh, nkv, SC.SMALL, pos, "dom_pos")
        inputs, ref = case_ref(c)
        assert ratio(c, inputs, ref, mistake=mistake) > 1.0, (pos, mistake)


@pytest.mark.parametrize("pos", [SC.RANGE, SC.RANGE + 1, SC.SMALL - 1])
@pytest.mark.parametrize("D,nh,nkv", SC.GEOMETRIES)
def test_a_stale_new_key_in_a_later_range_fails(D, nh, nkv, pos):
    """the workgroup whose range holds *pos -- not the first range here -- must take the new key / value from its own rotated copy"""
    c = SC.decode_case(D, nh, nkv, SC.SMALL, pos, "dom_pos")
    inputs, ref = case_ref(c)
    assert ratio(c, inputs, ref) <= 1.0
    for kw in (dict(stale_key=True), dict(stale_value=True)):
        stale = R.decode_expected(c, **kw)[0]
        assert ratio(c, stale, ref) > 1.0, kw
