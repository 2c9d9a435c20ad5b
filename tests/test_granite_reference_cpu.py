"""The Granite layout on the CPU: the float64 reference of the scaled residual epilogue (LL_GEMV_RESIDUAL_SCALED, include/llamole_hip.h), built
by composition on tests/linear_reference.py, and what ``accelerate_llm``'s structural checks answer for Granite-family models.

The chain is  bf16r(res + bf16r(bf16r(v) * f32(m)))  on the exact pre-rounding value v = lin of linear_reference.linear64.  Every step is
monotone in v, increasing for m > 0 and decreasing for m < 0, so the accepted interval is the min / max of the chain at lin - e and lin + e with
the same e = 2^-14 absref: the summation that e bounds is the Linear's and has not changed.  m == 1 gives linear_reference's RESIDUAL interval.

Shown here on gemv-K2048, gemv-K4104, rows16-K160 and rows64-K32 for m in {0.22, 1.0, -0.5, 3.0}:
  * HF's own line ``residual + hidden_states * m`` on bf16 tensors of an f32-accumulated Linear (torch's CPU kernel: product in f32 with m
    rounded to f32, three bf16 roundings) lies inside every interval, and is bit for bit ``llm_accel.hf_scaled_residual``;
  * five mistakes leave the intervals at m = 0.22, -0.5 and 3.0: the multiplier dropped; applied to residual + y; applied before the bias; the
    rounding of acc + bias skipped (the CPU data shows it: 1 to 20 % of the elements of a set tell it apart at m = 0.22 and 3.0, so it is
    asserted there; at -0.5 the product with a power of two is exact and the two orders are the same arithmetic, which is asserted too); m
    taken in bf16 (0.22 only: -0.5 and 3.0 are bf16 numbers).
The structural part: tiny-granite builds, its layers are declined for device / dtype reasons alone, the multipliers are read as 0.22 / 12.0,
a non-finite or zero multiplier and a MoE layer with a multiplier are declined with their own strings, the GraniteMoe families are declined
structurally (their layers have a ``block_sparse_moe``, no ``mlp``), and models without the attributes answer what they answered."""
import pytest
import torch

from llamole_amd import e2e, llm_accel
from tests import linear_reference as R

MULTIPLIERS = (0.22, 1.0, -0.5, 3.0)
SETS = ("gemv-K2048", "gemv-K4104", "rows16-K160", "rows64-K32")


def f32(m):
    """the multiplier a kernel sees: the C ABI takes a float, and torch multiplies a bf16 tensor by a Python float rounded to f32"""
    return float(torch.tensor(m, dtype=torch.float32))


def scaled_chain(v, res, m):
    return R.bf16r(res.to(R.F64) + R.bf16r(R.bf16r(v) * f32(m)))


def scaled_interval(lin, e, res, m):
    """lo, hi, mid (float32 holding bf16 values): the chain is monotone in v for either sign of m, so the two ends bound it"""
    a, b = scaled_chain(lin - e, res, m), scaled_chain(lin + e, res, m)
    lo, hi, mid = (t.to(torch.float32) for t in (torch.minimum(a, b), torch.maximum(a, b), scaled_chain(lin, res, m)))
    assert bool(((lo <= mid) & (mid <= hi)).all())
    return lo, hi, mid


def scaled_bounds(o, use_bias, m):
    """the intervals of a whole operand set [M, N] (form NONE: o_proj and down_proj have no norm prologue)"""
    lin, e = o.linear(R.NONE, use_bias)
    return scaled_interval(lin[:, :o.N], e[:, :o.N], o.res, m)


def _acc32(o, use_bias):
    """an f32 evaluation of the Linear, as torch's CPU matmul gives it: acc [M, N] and bias (zeros without)"""
    acc = o.x.float() @ o.w[:o.N].float().t()
    b = o.bias[:o.N] if use_bias else torch.zeros(o.N)
    return acc, b


def _bf(t):
    return t.to(R.BF)


@pytest.mark.parametrize("name", SETS)
def test_hf_line_lies_inside_every_interval(name):
    o = R.operands(name)
    for use_bias in (False, True):
        acc, b = _acc32(o, use_bias)
        y = _bf(acc + b)
        for m in MULTIPLIERS:
            hf = o.res + y * m                                  # GraniteDecoderLayer.forward's line on bf16 tensors
            assert hf.dtype == R.BF
            assert torch.equal(hf, llm_accel.hf_scaled_residual(o.res, y, m)), (name, m, "the product's restatement is not HF's line")
            outside, pos = R.check(hf, *scaled_bounds(o, use_bias, m))
            assert outside == 0, (name, use_bias, m, outside, pos)
            if m == 1.0:                                        # the plain residual epilogue, interval for interval
                for got, want in zip(scaled_bounds(o, use_bias, m), o.bounds(R.NONE, use_bias, R.RESIDUAL)):
                    assert torch.equal(got, want)


def _mistakes(o, use_bias, m):
    acc, b = _acc32(o, use_bias)
    res = o.res.float()
    m32 = torch.tensor(m, dtype=torch.float32)
    y = _bf(acc + b).float()
    out = {"multiplier dropped": _bf(res + y),
           "applied to residual + y": _bf(_bf(res + y).float() * m32),
           "rounding of acc + bias skipped": _bf(res + _bf((acc + b) * m32).float()),
           "m in bf16": _bf(res + _bf(y * _bf(m32).float()).float())}
    if use_bias:
        out["applied before the bias"] = _bf(res + _bf(_bf(acc * m32 + b).float()).float())
    return out


@pytest.mark.parametrize("name", SETS)
def test_mistakes_leave_the_intervals(name):
    o = R.operands(name)
    for use_bias in (False, True):
        for m in (0.22, -0.5, 3.0):
            bounds = scaled_bounds(o, use_bias, m)
            for what, got in _mistakes(o, use_bias, m).items():
                outside, _ = R.check(got, *bounds)
                if (what == "m in bf16" and m != 0.22) or (what == "rounding of acc + bias skipped" and m == -0.5):
                    # -0.5 and 3.0 are bf16 numbers, and a product with a power of two is exact: the same arithmetic, not a mistake
                    assert outside == 0
                    continue
                print(f"{name} bias={use_bias} m={m}: {what}: {outside} of {got.numel()} elements outside")
                assert outside > 0, (name, use_bias, m, what)


# ------------------------------------------------------------------------------------------------------------------ structure
def _reasons(model):
    return [llm_accel.decoder_layer_declined(l) for l in model.model.layers]


def test_tiny_granite_builds_and_is_declined_for_device_and_dtype_alone():
    cfg = e2e.LLM_CONFIGS["tiny-granite"]
    assert cfg["cls"] == "Granite" and (cfg["embedding_multiplier"], cfg["attention_multiplier"], cfg["residual_multiplier"],
                                        cfg["logits_scaling"]) == (12.0, 0.0078125, 0.22, 8.0)
    for k in ("hidden_size", "num_hidden_layers", "num_attention_heads", "num_key_value_heads", "intermediate_size", "vocab_size"):
        assert cfg[k] == e2e.LLM_CONFIGS["tiny-llama"][k]
    big = e2e.LLM_CONFIGS["granite-3.3-8b"]
    assert (big["hidden_size"], big["num_hidden_layers"], big["num_attention_heads"], big["num_key_value_heads"], big["intermediate_size"],
            big["rope_theta"], big["rms_norm_eps"], big["tie_word_embeddings"]) == (4096, 40, 32, 8, 12800, 1e7, 1e-5, True)
    assert (big["embedding_multiplier"], big["attention_multiplier"], big["residual_multiplier"], big["logits_scaling"]) == (12.0, 0.0078125, 0.22, 16.0)
    llm = e2e.build_llm("tiny-granite", "cpu", torch.bfloat16)
    assert type(llm).__name__ == "GraniteForCausalLM"
    assert _reasons(llm) == ["weights are not on the device"] * 2
    assert _reasons(e2e.build_llm("tiny-granite", "cpu", torch.float32)) == ["weights are not bf16"] * 2
    assert llm_accel._multiplier(llm.model.layers[0], "residual_multiplier") == (0.22, True)
    assert llm_accel._multiplier(llm.model, "embedding_multiplier") == (12.0, True)
    assert float(llm.model.layers[0].self_attn.scaling) == 0.0078125        # the fused layer reads attention_multiplier here
    # accelerate_llm on a CPU model changes nothing and reports nothing declined
    assert llm_accel.accelerate_llm(llm) == {"linears": 0}


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), 0.0, 1e-60, 1e60, "0.22x", None])
def test_a_multiplier_that_is_not_a_finite_nonzero_float_declines_the_layer(bad):
    llm = e2e.build_llm("tiny-granite", "cpu", torch.bfloat16)
    llm.model.layers[1].residual_multiplier = bad
    assert _reasons(llm) == ["weights are not on the device", llm_accel.RESIDUAL_MULTIPLIER_DECLINED]
    assert llm_accel._multiplier(llm.model.layers[1], "residual_multiplier")[1] is False
    llm.model.embedding_multiplier = bad
    assert llm_accel._multiplier(llm.model, "embedding_multiplier")[1] is False


def test_a_moe_layer_with_a_multiplier_is_declined():
    llm = e2e.build_llm("tiny-qwen3-moe", "cpu", torch.bfloat16)
    before = _reasons(llm)
    assert before == ["weights are not on the device"] * 2
    llm.model.layers[0].residual_multiplier = 0.22
    llm.model.layers[1].residual_multiplier = 1.0           # the neutral value is the plain residual add
    assert _reasons(llm) == [llm_accel.MOE_RESIDUAL_MULTIPLIER_DECLINED, "weights are not on the device"]


@pytest.mark.parametrize("kind,extra", [("GraniteMoe", {}), ("GraniteMoeShared", dict(shared_intermediate_size=128)),
                                        ("GraniteMoeHybrid", dict(shared_intermediate_size=128, layer_types=["attention", "attention"]))])
def test_granitemoe_families_are_declined_structurally(kind, extra):
    """their decoder layers carry residual_multiplier like the dense ones; they have a ``block_sparse_moe`` (and ``shared_mlp``) instead of an
    ``mlp``, so no layer is fused -- with or without the multiplier -- and the base model's prologue is not installed either"""
    import transformers
    cfg = getattr(transformers, kind + "Config")(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                                 intermediate_size=128, vocab_size=512, num_local_experts=4, num_experts_per_tok=2,
                                                 residual_multiplier=0.22, embedding_multiplier=12.0, **extra)
    llm = getattr(transformers, kind + "ForCausalLM")(cfg).to(torch.bfloat16)
    assert all(not hasattr(l, "mlp") and hasattr(l, "block_sparse_moe") for l in llm.model.layers)
    assert _reasons(llm) == ["no self_attn / mlp"] * 2
    assert llm_accel.fuse_decoder_layers(llm) == 0
    assert llm_accel.model_decode_declined(llm) in ("not every decoder layer is fused", "not a Llama-layout base model")


@pytest.mark.parametrize("name", ["tiny-llama", "tiny", "tiny-qwen3", "tiny-qwen3-moe"])
def test_models_without_the_attributes_answer_what_they_answered(name):
    llm = e2e.build_llm(name, "cpu", torch.bfloat16)
    assert not hasattr(llm.model.layers[0], "residual_multiplier") and not hasattr(llm.model, "embedding_multiplier")
    assert _reasons(llm) == ["weights are not on the device"] * 2
    assert llm_accel._multiplier(llm.model.layers[0], "residual_multiplier") == (1.0, True)
    assert llm_accel._multiplier(llm.model, "embedding_multiplier") == (1.0, True)


def test_embedding_restatement_is_hf_line():
    g = torch.Generator().manual_seed(4)
    table = torch.randn(64, 40, generator=g).to(R.BF)
    ids = torch.tensor([[0, 63, 7], [7, 1, 62]])
    for m in (12.0, 0.22, -3.5):
        assert torch.equal(torch.nn.functional.embedding(ids, table) * m, llm_accel.hf_scaled_embedding(table, ids, m))
