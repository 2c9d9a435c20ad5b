"""The float64 reference of tests/qknorm_reference.py, checked without a GPU on the inputs tests/test_qknorm_attention_gpu.py hands to the
kernels: (a) HuggingFace's Qwen3RMSNorm module in bf16 gives the reference's bits on tie-safe vectors, (b) a plain f32 evaluation of norm + rotary +
attention stays inside attn_reference's bound and stores the reference's key bits, (c) each mistake a kernel with the norm inside can make leaves
the bound or changes the stored key / value row."""
import pytest
import torch

from tests import attn_reference as R
from tests import qknorm_reference as Q
from tests.test_decode_attention_reference_cpu import emulate_f32


def norm_f32(x, w, eps=Q.EPS):
    """Qwen3RMSNorm.forward written out: f32 mean / rsqrt / product, cast, weight * that in bf16"""
    xf = x.float()
    xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return w * xf.to(Q.BF)


def ratio(c, inputs, ref):
    return R.err_over_bound(emulate_f32(*inputs, c.scale, c.nh, c.nkv), *ref)


# ------------------------------------------------------------------------------------------------------------------ the reference on its own
@pytest.mark.parametrize("D", [64, 128])
def test_hf_qwen3_rmsnorm_gives_the_reference_bits_on_tie_safe_vectors(D):
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RMSNorm
    g = torch.Generator().manual_seed(D)
    x, w = Q.tie_safe(g, (2, 5, 3, D)), Q.norm_weight(g, D)
    assert not Q.in_window(x).any()
    mod = Qwen3RMSNorm(D, eps=Q.EPS).to(Q.BF)
    with torch.no_grad():
        mod.weight.copy_(w)
        got = mod(x)
    assert got.dtype == Q.BF and torch.equal(got, Q.head_norm(x, w))
    assert torch.equal(norm_f32(x, w), Q.head_norm(x, w))
    assert not torch.equal(Q.head_norm(x, w), Q.head_norm(x, torch.ones_like(w)))        # the weights are not ones


@pytest.mark.parametrize("D", [64, 128])
def test_the_window_holds_about_one_percent_of_the_elements(D):
    g = torch.Generator().manual_seed(7 + D)
    x = torch.randn(4000, D, generator=g).to(Q.BF)
    flag = Q.in_window(x)
    assert 0.005 < float(flag.float().mean()) < 0.02
    share = float((~flag.any(-1)).float().mean())                # vectors the rejection keeps
    assert (0.3 < share < 0.5) if D == 128 else (0.45 < share < 0.65)
    # outside the window an f32 evaluation rounds as float64 does; the candidates cover the rest
    w = Q.norm_weight(g, D)
    differs = norm_f32(x, w) != Q.head_norm(x, w)
    assert not (differs & ~flag).any()
    cos, sin = R.rope_tables(R.inv_freq(D), torch.tensor([37]))
    cands, flag2 = Q.key_candidates(x, w, cos, sin)
    assert torch.equal(flag, flag2)
    got = R.rotary_bf16(norm_f32(x, w), cos, sin)
    hit = torch.stack([got == cand for cand in cands]).any(0)
    assert hit.all()
    pair = flag | flag.roll(D // 2, -1)                          # a rotated element depends on both elements of its pair
    assert all(torch.equal(cand[~pair], cands[0][~pair]) for cand in cands)


# ------------------------------------------------------------------------------------------------------------------ every GPU case passes in f32
@pytest.mark.parametrize("maxlen", Q.MAXLENS)
@pytest.mark.parametrize("nh,nkv", Q.GEOMETRIES)
@pytest.mark.parametrize("D", [64, 128])
def test_f32_evaluation_is_within_the_bound_decode(D, nh, nkv, maxlen):
    for pos in Q.positions(maxlen):
        for B in (3, 17):
            for variant in ("plain", "dom_pos", "tiny"):
                c = Q.decode_case(D, nh, nkv, maxlen, pos, variant, B=B)
                inputs, (k_rot, _) = Q.decode_expected(c)
                ref = R.reference(c, inputs)
                got, (k32, _) = Q.decode_expected(c, q=norm_f32(c.q, c.qw), k=norm_f32(c.k, c.kw))
                assert torch.equal(k32, k_rot)
                assert ratio(c, got, ref) <= 1.0, (variant, pos, B)
                if variant == "dom_pos":                         # the new key is exactly twice the rotated query of its group
                    assert torch.equal(k_rot.float(), 2 * inputs[0][:, ::nh // nkv, 0].float())


@pytest.mark.parametrize("maxlen", Q.MAXLENS)
@pytest.mark.parametrize("nh,nkv", Q.GEOMETRIES)
@pytest.mark.parametrize("D", [64, 128])
def test_f32_evaluation_is_within_the_bound_suffix(D, nh, nkv, maxlen):
    for S, B in Q.SUFFIX_ROWS:
        for pos in Q.suffix_positions(S, maxlen):
            for variant in ("plain", "dom_own"):
                c = Q.suffix_case(D, nh, nkv, B, S, maxlen, pos, variant)
                inputs, written = Q.suffix_expected(c)
                ref = R.reference(c, inputs)
                got, _ = Q.suffix_expected(c, q=norm_f32(c.q, c.qw), k=norm_f32(c.k, c.kw))
                assert torch.equal(got[1], inputs[1]) and int(written.sum()) == S
                assert ratio(c, got, ref) <= 1.0, (variant, pos, S, B)


# ------------------------------------------------------------------------------------------------------------------ every mistake is caught
def rotate_then_norm(c):
    """the norm applied after the rotation: hand attn_reference an identity rotation on rows that are already rotated and then normalised"""
    cos, sin = c.cos[:, None, :], c.sin[:, None, :]
    return Q.head_norm(R.rotary_bf16(c.q, cos, sin), c.qw), Q.head_norm(R.rotary_bf16(c.k, cos, sin), c.kw)


def mistakes(c):
    """name -> (inputs, (k_row, v_row)) of a wrong evaluation of the decode case c"""
    D = c.D
    out = {
        "no norm": Q.decode_expected(c, q=c.q, k=c.k),
        "q normalised with k's weight": Q.decode_expected(c, q=Q.head_norm(c.q, c.kw)),
        "weight before the first rounding": Q.decode_expected(c, q=Q.head_norm(c.q, c.qw, weight_first=True),
                                                              k=Q.head_norm(c.k, c.kw, weight_first=True)),
        "mean over D/2 elements": Q.decode_expected(c, q=Q.head_norm(c.q, c.qw, mean_over=D // 2), k=Q.head_norm(c.k, c.kw, mean_over=D // 2)),
        "v normalised": Q.decode_expected(c, v=Q.head_norm(c.v, c.kw)),
    }
    qr, kr = rotate_then_norm(c)
    ident = Q.normed(c, q=qr, k=kr)
    ident.cos, ident.sin = torch.ones_like(c.cos), torch.zeros_like(c.sin)
    out["norm after the rotation"] = R.decode_expected(ident)
    return out


@pytest.mark.parametrize("maxlen,pos", [(64, 37), (320, 256)])
@pytest.mark.parametrize("D,nh,nkv", [(64, 4, 2), (128, 4, 1), (128, 7, 1), (64, 3, 3)])
def test_each_mistake_leaves_the_bound_or_changes_the_stored_row(D, nh, nkv, maxlen, pos):
    for variant in ("plain", "dom_pos"):
        c = Q.decode_case(D, nh, nkv, maxlen, pos, variant)
        inputs, (k_rot, v_new) = Q.decode_expected(c)
        ref = R.reference(c, inputs)
        assert ratio(c, inputs, ref) <= 1.0
        for name, (wrong, (k_w, v_w)) in mistakes(c).items():
            if name == "q normalised with k's weight" and variant == "dom_pos":
                continue                                         # k_norm_w = 2 q_norm_w there: the query doubles and its key dominates all the more
            left = ratio(c, wrong, ref) > 1.0
            stored = not torch.equal(k_w, k_rot) or not torch.equal(v_w, v_new)
            assert left or stored, (name, variant)
            if name == "q normalised with k's weight":           # the stored rows cannot tell: the output must
                assert left and not stored, (name, variant)
            if name in ("no norm", "mean over D/2 elements", "norm after the rotation") and variant == "plain":
                assert left and stored, (name, variant)


@pytest.mark.parametrize("D,nh,nkv", [(64, 4, 2), (128, 4, 1)])
def test_dropped_eps_is_caught_on_tiny_rows(D, nh, nkv):
    """head rows scaled by 2^-12: mean(x^2) is about 2^-24 = 6e-8 against eps = 1e-6, so eps carries the norm"""
    c = Q.decode_case(D, nh, nkv, 64, 37, "tiny")
    inputs, (k_rot, _) = Q.decode_expected(c)
    ref = R.reference(c, inputs)
    assert ratio(c, inputs, ref) <= 1.0
    wrong, (k_w, _) = Q.decode_expected(c, q=Q.head_norm(c.q, c.qw, eps=0.0), k=Q.head_norm(c.k, c.kw, eps=0.0))
    assert ratio(c, wrong, ref) > 1.0 and not torch.equal(k_w, k_rot)
    assert float(k_w.float().abs().mean()) > 3 * float(k_rot.float().abs().mean())
