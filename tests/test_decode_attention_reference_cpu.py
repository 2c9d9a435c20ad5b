"""The float64 reference of tests/attn_reference.py, checked without a GPU on the very inputs tests/test_decode_attention_reference_gpu.py hands
to the kernels: a plain f32 evaluation (f32 scores, f32 softmax, f32 P.V, one bf16 rounding) stays inside the derived bound on every case, and
each mistake a decode attention kernel can make leaves it on the case built to catch it."""
import math

import pytest
import torch

from tests import attn_reference as R


def emulate_f32(q_rot, K, V, mask, scale, nh, nkv, head_map="div"):
    """what a correct kernel computes: f32 throughout, one rounding to bf16.  head_map "mod" is the wrong GQA map h % nkv."""
    idx = torch.arange(nh) // (nh // nkv) if head_map == "div" else torch.arange(nh) % nkv
    out = torch.empty(q_rot.shape, dtype=R.BF)
    sc = torch.tensor(scale, dtype=torch.float32)
    for b in range(q_rot.shape[0]):
        Kh, Vh = torch.nan_to_num(K[b].float())[idx], torch.nan_to_num(V[b].float())[idx]
        s = (q_rot[b].float() @ Kh.transpose(-1, -2)) * sc
        s = s.masked_fill(~mask[b][None], -math.inf)
        m = s.amax(-1, keepdim=True)
        e = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
        den = e.sum(-1, keepdim=True)
        inv = torch.where(den > 0, 1.0 / den, torch.zeros_like(den))
        out[b] = ((e @ Vh) * inv).to(R.BF)
    return out


def ratio(c, inputs, ref=None, **kw):
    ref, absref = ref if ref is not None else R.reference(c)
    return R.err_over_bound(emulate_f32(*inputs, c.scale, c.nh, c.nkv, **kw), ref, absref)


def drop_keys(inputs, keys):
    q, K, V, mask = inputs
    mask = mask.clone()
    for b, s, j in keys:
        mask[b, s, j] = False
    return q, K, V, mask


def check_case(c):
    """the f32 evaluation passes; with the dominant keys of the case dropped it does not"""
    inputs = R.expected(c)[0]
    ref = R.reference(c, inputs)
    r = ratio(c, inputs, ref)
    assert r <= 1.0, (c.kind, c.variant, r)
    if c.dominant:
        assert ratio(c, drop_keys(inputs, c.dominant), ref) > 1.0, (c.kind, c.variant, "a lost dominant key passes")
    return r


# ------------------------------------------------------------------------------------------------------------------ the reference on its own
def test_rotary_is_hf_apply_rotary_pos_emb():
    from transformers.models.qwen2.modeling_qwen2 import apply_rotary_pos_emb
    g = torch.Generator().manual_seed(0)
    q, k = torch.randn(2, 4, 3, 64, generator=g).to(R.BF), torch.randn(2, 2, 3, 64, generator=g).to(R.BF)
    cos, sin = R.rope_tables(R.inv_freq(64), torch.tensor([[5, 6, 7], [40, 41, 42]]))
    qe, ke = apply_rotary_pos_emb(q, k, cos, sin)
    assert torch.equal(qe, R.rotary_bf16(q, cos[:, None], sin[:, None])) and torch.equal(ke, R.rotary_bf16(k, cos[:, None], sin[:, None]))


def test_attention_f64_is_sdpa_with_repeated_kv_heads():
    g = torch.Generator().manual_seed(1)
    B, nh, nkv, S, L, D = 2, 6, 2, 3, 37, 64
    q, K, V = (torch.randn(B, h, n, D, generator=g).to(R.BF) for h, n in ((nh, S), (nkv, L), (nkv, L)))
    mask = torch.rand(B, S, L, generator=g) > 0.3
    mask[1, 2] = False                                           # a row with no visible key gives zeros
    K[0, :, ~mask[0].any(0)] = R.NAN                           # slots nobody sees may hold anything
    ref, absref = R.attention_f64(q, K, V, mask, D ** -0.5, nh, nkv)
    Kr, Vr = (torch.nan_to_num(t.double()).repeat_interleave(nh // nkv, dim=1) for t in (K, V))
    want = torch.nn.functional.scaled_dot_product_attention(q.double(), Kr, Vr, attn_mask=mask[:, None], scale=D ** -0.5)
    want[1, :, 2] = 0                                            # sdpa gives NaN there
    torch.testing.assert_close(ref, want, rtol=1e-12, atol=1e-12)
    assert float(ref[1, :, 2].abs().max()) == 0 and float(absref[1, :, 2].abs().max()) == 0
    assert (absref >= ref.abs() - 1e-15).all()
    # the bound: exact zero demanded where it is zero, NaN never passes
    got = ref.to(R.BF)
    assert R.err_over_bound(got, ref, absref) <= 1.0
    bad = got.clone()
    bad[1, 0, 2, 0] = 1e-30
    assert R.err_over_bound(bad, ref, absref) == math.inf
    bad = got.clone()
    bad[0, 0, 0, 0] = R.NAN
    assert R.err_over_bound(bad, ref, absref) == math.inf


# ------------------------------------------------------------------------------------------------------------------ every GPU case passes
@pytest.mark.parametrize("maxlen,pos", R.POSITIONS)
@pytest.mark.parametrize("D,nh,nkv", R.GEOMETRIES)
def test_f32_evaluation_is_within_the_bound_decode(D, nh, nkv, maxlen, pos):
    for variant in R.decode_variants(maxlen, pos):
        for bcast in ((True, False) if variant == "plain" else (False,)):
            c = R.decode_case(D, nh, nkv, maxlen, pos, variant, bcast=bcast)
            check_case(c)
            inputs, (k_rot, v_new) = R.decode_expected(c)
            ref, _ = R.reference(c, inputs)
            if maxlen == 1:                                      # one key: the output is the new value row
                want = v_new.double().repeat_interleave(nh // nkv, dim=1) * c.visible[:, :1, None]
                assert torch.equal(ref[:, :, 0], want)
            if variant == "qzero":                               # uniform weights: the mean of the visible value rows
                for b in range(c.B):
                    n = int(c.visible[b].sum())
                    if n:
                        mean = inputs[2][b].double()[:, c.visible[b]].mean(1).repeat_interleave(nh // nkv, dim=0)
                        torch.testing.assert_close(ref[b, :, 0], mean, rtol=1e-12, atol=1e-12)
            assert float(ref[2].abs().max()) == 0.0              # the fully masked row


@pytest.mark.parametrize("maxlen,pos,variant", [(m, p, v) for m, p in R.GROUPED_POSITIONS for v in R.decode_variants(m, p)])
@pytest.mark.parametrize("D,nh,nkv", R.GROUPED_GEOMETRIES + [(64, 6, 2), (128, 6, 2)])
def test_f32_evaluation_is_within_the_bound_17_sequences(D, nh, nkv, maxlen, pos, variant):
    check_case(R.decode_case(D, nh, nkv, maxlen, pos, variant, B=17))


@pytest.mark.parametrize("variant", ["plain", "dom_pos"])
@pytest.mark.parametrize("maxlen", R.LDS_SWITCH)
def test_f32_evaluation_is_within_the_bound_lds_switch(maxlen, variant):
    check_case(R.decode_case(128, 7, 1, maxlen, maxlen - 1, variant, B=17))


@pytest.mark.parametrize("D,nh,nkv,S,maxlen,p0", R.ATTN_CASES)
def test_f32_evaluation_is_within_the_bound_attn(D, nh, nkv, S, maxlen, p0):
    for variant in R.ATTN_VARIANTS:
        check_case(R.attn_case(D, nh, nkv, S, maxlen, p0, variant))


@pytest.mark.parametrize("D,nh,nkv,B,S,maxlen,pos", R.SUFFIX_CASES)
def test_f32_evaluation_is_within_the_bound_suffix(D, nh, nkv, B, S, maxlen, pos):
    for variant in R.SUFFIX_VARIANTS:
        check_case(R.suffix_case(D, nh, nkv, B, S, maxlen, pos, variant))


@pytest.mark.parametrize("D,maxlen,variants", R.LONG_CASES)
@pytest.mark.parametrize("entry", ["decode", "suffix", "attn"])
def test_f32_evaluation_is_within_the_bound_long(entry, D, maxlen, variants):
    for variant in variants:
        check_case(R.long_case(entry, D, maxlen, variant))


# ------------------------------------------------------------------------------------------------------------------ every mistake is caught
def rotary_interleaved(x, cos, sin):
    """pairs (2i, 2i+1) instead of (i, i + D/2)"""
    h = x.shape[-1] // 2
    c, s = cos[..., :h].repeat_interleave(2, dim=-1), sin[..., :h].repeat_interleave(2, dim=-1)
    rot = torch.stack((-x[..., 1::2], x[..., 0::2]), dim=-1).flatten(-2)
    return x * c + rot * s


def shift_mask(inputs, by):
    q, K, V, mask = inputs
    out = torch.zeros_like(mask)
    if by > 0:
        out[..., by:] = mask[..., :-by]
    else:
        out[..., :by] = mask[..., -by:]
    return q, K, V, out


CATCH_GEOMETRIES = [(64, 6, 2), (128, 4, 2), (128, 7, 1)]


@pytest.mark.parametrize("D,nh,nkv", CATCH_GEOMETRIES)
@pytest.mark.parametrize("maxlen,pos,which", [(300, 256, "first"), (300, 256, "255"), (300, 256, "256"), (300, 256, "prev"), (300, 256, "pos"),
                                              (600, 300, "255"), (600, 300, "256"), (257, 256, "pos"), (256, 255, "pos"), (300, 255, "prev"),
                                              (40, 0, "pos"), (40, 39, "first")])
def test_a_key_dropped_at_a_boundary_is_caught(D, nh, nkv, maxlen, pos, which):
    c = R.decode_case(D, nh, nkv, maxlen, pos, "dom_" + which)
    inputs = R.expected(c)[0]
    assert c.dominant and ratio(c, inputs) <= 1.0
    for key in c.dominant:                                       # one key of one row is enough
        assert ratio(c, drop_keys(inputs, [key])) > 1.0


@pytest.mark.parametrize("D,nh,nkv", CATCH_GEOMETRIES)
@pytest.mark.parametrize("maxlen,pos", [(40, 0), (300, 255), (300, 256), (600, 300)])
def test_a_mask_shifted_by_one_slot_is_caught(D, nh, nkv, maxlen, pos):
    c = R.decode_case(D, nh, nkv, maxlen, pos, "dom_first")     # shifted up: the first visible key is lost
    assert ratio(c, shift_mask(R.expected(c)[0], 1)) > 1.0
    c = R.decode_case(D, nh, nkv, maxlen, pos, "dom_pos")       # shifted down: the new key is lost
    assert ratio(c, shift_mask(R.expected(c)[0], -1)) > 1.0


@pytest.mark.parametrize("D,nh,nkv", R.GEOMETRIES)
@pytest.mark.parametrize("maxlen,pos", [(40, 39), (300, 256), (600, 300)])
def test_the_scale_of_the_other_head_dim_is_caught(D, nh, nkv, maxlen, pos):
    for variant in ("plain", "q8"):
        c = R.decode_case(D, nh, nkv, maxlen, pos, variant)
        got = emulate_f32(*R.expected(c)[0], (192 - D) ** -0.5, c.nh, c.nkv)
        assert R.err_over_bound(got, *R.reference(c)) > 1.0


@pytest.mark.parametrize("D,nh,nkv", R.GEOMETRIES)
@pytest.mark.parametrize("maxlen,pos", [(40, 39), (300, 256), (600, 300)])
def test_interleaved_rotary_pairs_are_caught(D, nh, nkv, maxlen, pos):
    c = R.decode_case(D, nh, nkv, maxlen, pos, "plain")
    assert ratio(c, R.decode_expected(c, rotary=rotary_interleaved)[0]) > 1.0


@pytest.mark.parametrize("D,nh,nkv", [g for g in R.GEOMETRIES if 1 < g[2] < g[1]])
@pytest.mark.parametrize("maxlen,pos", [(40, 39), (300, 256), (600, 300)])
def test_the_head_map_h_mod_nkv_is_caught(D, nh, nkv, maxlen, pos):
    c = R.decode_case(D, nh, nkv, maxlen, pos, "plain")
    assert ratio(c, R.expected(c)[0], head_map="mod") > 1.0


@pytest.mark.parametrize("D,nh,nkv", CATCH_GEOMETRIES)
@pytest.mark.parametrize("maxlen,pos", [(1, 0), (40, 0), (40, 39), (300, 255), (300, 256), (600, 300)])
def test_the_stale_cache_row_is_caught(D, nh, nkv, maxlen, pos):
    c = R.decode_case(D, nh, nkv, maxlen, pos, "dom_pos")
    assert ratio(c, R.decode_expected(c, stale_key=True)[0]) > 1.0 or pos == 0         # one visible key: its weight is 1 whatever it holds
    assert ratio(c, R.decode_expected(c, stale_value=True)[0]) > 1.0


@pytest.mark.parametrize("D,nh,nkv", CATCH_GEOMETRIES)
@pytest.mark.parametrize("maxlen,pos", [(40, 39), (300, 255), (300, 256)])
def test_an_unrotated_new_key_is_caught(D, nh, nkv, maxlen, pos):
    """plain data at a short context: the new key's weight is a few percent and moves with its score.  (A dominant new key stays dominant
    unrotated -- the low frequencies barely turn -- so that case cannot tell.)"""
    c = R.decode_case(D, nh, nkv, maxlen, pos, "plain")
    assert not torch.equal(R.decode_expected(c)[1][0], c.k)
    assert ratio(c, R.decode_expected(c, rotate_new_key=False)[0]) > 1.0
