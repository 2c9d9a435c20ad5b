"""The float64 reference of the Mixtral and shared-expert contracts (tests/moe2_reference.py) judged on the CPU, before any kernel is measured
against it: HuggingFace's own MixtralSparseMoeBlock and Qwen2MoeSparseMoeBlock (default experts implementation) + the decoder layer's
residual add stay inside every interval at 1 and 6 rows; three deliberate mistakes leave them (the Qwen3 contract on the Mixtral operands, the
shared gate dropped, sigmoid replaced by identity); and decoder_layer_declined answers for both families on the CPU."""
import pytest
import torch
import torch.nn as nn

from tests import moe2_reference as M2
from tests import moe_reference as MR

BF, F64 = torch.bfloat16, torch.float64
H = 256


def _spread(layer, seed):
    """HF draws norm weights as ones and the router at std 0.02 (logits that are all but equal): draw every operand of the block afresh"""
    g = torch.Generator().manual_seed(seed)
    mlp = layer.mlp
    with torch.no_grad():
        layer.post_attention_layernorm.weight.copy_((1 + 0.25 * torch.randn(H, generator=g)).to(BF))
        mlp.gate.weight.copy_((torch.randn(mlp.gate.weight.shape, generator=g) * 0.2).to(BF))
        ex = mlp.experts
        ex.gate_up_proj.copy_((torch.randn(ex.gate_up_proj.shape, generator=g) / 16).to(BF))
        ex.down_proj.copy_((torch.randn(ex.down_proj.shape, generator=g) * 0.35).to(BF))
        if hasattr(mlp, "shared_expert"):
            sh = mlp.shared_expert
            sh.gate_proj.weight.copy_((torch.randn(sh.gate_proj.weight.shape, generator=g) / 16).to(BF))
            sh.up_proj.weight.copy_((torch.randn(sh.up_proj.weight.shape, generator=g) / 16).to(BF))
            sh.down_proj.weight.copy_((torch.randn(sh.down_proj.weight.shape, generator=g) * 0.2).to(BF))
            mlp.shared_expert_gate.weight.copy_((torch.randn(1, H, generator=g) * 0.15).to(BF))


def _hf_case(name, rows, seed, **overrides):
    """(out [rows, H] of HF's block + residual add, what the reference needs to bound it)"""
    from llamole_amd.e2e import build_llm
    model = build_llm(name, "cpu", seed=seed, num_hidden_layers=1, **overrides)
    assert model.config._experts_implementation == "grouped_mm"          # HF's default, the contract's path
    layer = model.model.layers[0]
    _spread(layer, 5 + seed)
    h1 = torch.randn(1, rows, H, generator=torch.Generator().manual_seed(11 + seed)).to(BF)
    with torch.no_grad():
        xn = layer.post_attention_layernorm(h1)
        logits, w, idx = layer.mlp.gate(xn.reshape(-1, H))
        out = (h1 + layer.mlp(xn)).reshape(-1, H)
    x, n2, ex = h1.reshape(-1, H), layer.post_attention_layernorm, layer.mlp.experts
    _, _, _, ylo, yhi, ymid = MR.experts_ay(x, n2.weight.detach(), n2.variance_epsilon, idx.to(torch.int32), ex.gate_up_proj.detach(),
                                            ex.down_proj.detach())
    return layer, x, logits, w, idx, out, (ylo, yhi, ymid)


@pytest.mark.parametrize("rows", (1, 6))
def test_hf_mixtral_block_inside_and_the_qwen3_contract_outside(rows):
    # intermediate_size 64: the summation-order allowance of y grows with sqrt(I) and at 512 it spans a bf16 step on most outputs, which would
    # hide the one bf16 rounding this control is about; seed 0 is the first at which the control leaves an interval at both row counts
    layer, x, logits, w, idx, out, y = _hf_case("tiny-mixtral", rows, seed=0, intermediate_size=64)
    assert w.dtype == torch.float32                                       # MixtralTopKRouter keeps f32 weights
    ridx, w64, delta = M2.route64_f32(logits, 2)
    assert torch.equal(idx.to(torch.int32), ridx)
    assert M2.route_f32_ok(w, w64, delta) == 0
    bounds = M2.finish2(*y, w, x, w_f32=True)
    bad, _ = M2.check(out, *bounds)
    assert bad == 0
    # control: the Qwen3 contract on the same operands -- the weight rounded to bf16, every slot's product rounded to bf16
    qwen3 = MR.finish(*y, w.to(BF).float(), x)[2]
    bad_q, _ = M2.check(qwen3, *bounds)
    print(f"\nMixtral, {rows} rows: the Qwen3 contract leaves {bad_q} of {out.numel()} intervals")
    assert bad_q > 0


@pytest.mark.parametrize("rows", (1, 6))
def test_hf_qwen2_moe_block_inside_and_gate_mistakes_outside(rows):
    layer, x, logits, w, idx, out, y = _hf_case("tiny-qwen2-moe", rows, seed=0)
    assert w.dtype == BF and layer.mlp.gate.norm_topk_prob is False
    ridx, mid, lo, hi, _ = MR.route64(logits, 2, False)
    assert torch.equal(idx.to(torch.int32), ridx)
    assert bool(((w.float() >= lo) & (w.float() <= hi)).all())
    n2, sh = layer.post_attention_layernorm, layer.mlp.shared_expert
    shared = M2.shared64(x, n2.weight.detach(), n2.variance_epsilon, sh.gate_proj.weight.detach(), sh.up_proj.weight.detach(),
                         sh.down_proj.weight.detach(), layer.mlp.shared_expert_gate.weight.detach())
    bounds = M2.finish2(*y, w.float(), x, w_f32=False, shared=shared)
    bad, _ = M2.check(out, *bounds)
    assert bad == 0
    # HF's own s and g lie inside their intervals too
    with torch.no_grad():
        xn = n2(x)
        s, g = sh(xn), layer.mlp.shared_expert_gate(xn)[:, 0]
    assert bool(((s.to(F64) >= shared[0]) & (s.to(F64) <= shared[1])).all()) and bool(((g.to(F64) >= shared[3]) & (g.to(F64) <= shared[4])).all())
    # controls: the shared expert added ungated, and gated by the logit itself
    for gate in ("dropped", "identity"):
        wrong = M2.finish2(*y, w.float(), x, w_f32=False, shared=shared, gate=gate)[2]
        bad_w, _ = M2.check(wrong, *bounds)
        print(f"Qwen2-MoE, {rows} rows: gate {gate} leaves {bad_w} of {out.numel()} intervals")
        assert bad_w > 0, gate
    # ... and no shared expert at all (the Qwen3 block)
    bad_n, _ = M2.check(MR.finish(*y, w.float(), x)[2], *bounds)
    assert bad_n > 0


def test_gpu_cases_are_self_consistent():
    """the mid value of every GPU case lies inside its own interval, the f32 weights of an f32 PyTorch evaluation pass, and the two contracts
    differ on the GPU test's operands (so a kernel that computed the other one would be caught there)"""
    for name in ("same-M5-k2", "ends-M17-k4", "distinct-M4-k2"):
        c = M2.case2(name)
        l = c.logits.float()
        p = torch.softmax(l, dim=-1).gather(1, c.idx.long())
        w32 = p / p.sum(-1, keepdim=True)
        assert M2.route_f32_ok(w32, c.w64, c.delta) == 0
        assert M2.route_f32_ok(w32.to(BF).float(), c.w64, c.delta) > 0            # a weight rounded to bf16 is not an f32 weight
        for w, w_f32 in ((w32, True), (c.w, False)):
            for shared in (False, True):
                lo, hi, mid = c.bounds2(w, w_f32, shared)
                assert M2.check(mid, lo, hi, mid)[0] == 0
        mixtral = c.bounds2(w32, True, False)
        assert M2.check(MR.finish(*c.ay()[3:], w32.to(BF).float(), c.res)[2], *mixtral)[0] > 0


# ------------------------------------------------------------------------------------------------------------------ eligibility
def test_moe2_eligibility_cpu():
    from llamole_amd.e2e import build_llm
    from llamole_amd.llm_accel import decoder_layer_declined
    for name in ("tiny-mixtral", "tiny-qwen2-moe"):
        llm = build_llm(name, "cpu")
        assert [decoder_layer_declined(l) for l in llm.model.layers] == ["weights are not on the device"] * 2, name     # nothing structural
        assert decoder_layer_declined(build_llm(name, "cpu", dtype=torch.float32).model.layers[1]) == "weights are not bf16", name
    mixed = build_llm("tiny-qwen2-moe", "cpu", mlp_only_layers=[0])
    assert type(mixed.model.layers[0].mlp).__name__ == "Qwen2MoeMLP" and type(mixed.model.layers[1].mlp).__name__ == "Qwen2MoeSparseMoeBlock"
    assert [decoder_layer_declined(l) for l in mixed.model.layers] == ["weights are not on the device"] * 2
    # a Mixtral block is taken by its parts: a foreign router class is declined under the block's name
    foreign = build_llm("tiny-mixtral", "cpu").model.layers[0]
    foreign.mlp.gate.__class__ = type("OtherRouter", (type(foreign.mlp.gate),), {})
    assert decoder_layer_declined(foreign) == "MoE block of an unsupported kind (MixtralSparseMoeBlock)"
    foreign = build_llm("tiny-mixtral", "cpu").model.layers[0]
    foreign.mlp.experts.__class__ = type("OtherExperts", (type(foreign.mlp.experts),), {})
    assert decoder_layer_declined(foreign) == "MoE block of an unsupported kind (MixtralSparseMoeBlock)"
    # the shared expert of a Qwen2-MoE block
    biased = build_llm("tiny-qwen2-moe", "cpu").model.layers[0]
    biased.mlp.shared_expert.up_proj = nn.Linear(H, 384, bias=True, dtype=BF)
    assert decoder_layer_declined(biased) == "shared expert bias"
    biased = build_llm("tiny-qwen2-moe", "cpu").model.layers[0]
    biased.mlp.shared_expert_gate = nn.Linear(H, 1, bias=True, dtype=BF)
    assert decoder_layer_declined(biased) == "shared expert bias"
    odd = build_llm("tiny-qwen2-moe", "cpu", shared_expert_intermediate_size=12).model.layers[0]
    assert decoder_layer_declined(odd) == "shared_expert_intermediate_size is not a multiple of 8"
    two = build_llm("tiny-qwen2-moe", "cpu").model.layers[0]
    two.mlp.shared_expert_gate = nn.Linear(H, 2, bias=False, dtype=BF)
    assert decoder_layer_declined(two) == "shared expert is not gate_proj / up_proj [I_s, H], down_proj [H, I_s] with a shared_expert_gate [1, H]"
    gelu = build_llm("tiny-qwen2-moe", "cpu", hidden_act="gelu").model.layers[0]
    assert decoder_layer_declined(gelu) in ("shared expert activation is not SiLU", "activation is not SiLU")
    # the answers tests/test_moe_reference_cpu.py pins, again: a Qwen3 block with a shared expert, and one merely renamed
    shared = build_llm("tiny-qwen3-moe", "cpu").model.layers[0]
    shared.mlp.shared_expert = nn.Linear(8, 8)
    assert decoder_layer_declined(shared) == "MoE block of an unsupported kind (shared expert)"
    other = build_llm("tiny-qwen3-moe", "cpu").model.layers[0]
    other.mlp.__class__ = type("MixtralSparseMoeBlock", (type(other.mlp),), {})
    assert decoder_layer_declined(other) == "MoE block of an unsupported kind (MixtralSparseMoeBlock)"
    assert [decoder_layer_declined(l) for l in build_llm("tiny-qwen3-moe", "cpu").model.layers] == ["weights are not on the device"] * 2


def test_the_config_entries():
    from llamole_amd import e2e
    big = e2e.LLM_CONFIGS["mixtral-8x7b"]
    assert (big["cls"], big["hidden_size"], big["num_hidden_layers"], big["num_attention_heads"], big["num_key_value_heads"],
            big["intermediate_size"], big["num_local_experts"], big["num_experts_per_tok"], big["vocab_size"]) == ("Mixtral", 4096, 32, 32, 8, 14336, 8, 2, 32000)
    q = e2e.LLM_CONFIGS["qwen1.5-moe-a2.7b"]
    assert (q["cls"], q["hidden_size"], q["num_hidden_layers"], q["num_attention_heads"], q["num_key_value_heads"], q["num_experts"],
            q["num_experts_per_tok"], q["moe_intermediate_size"], q["shared_expert_intermediate_size"], q["vocab_size"]) == \
        ("Qwen2Moe", 2048, 24, 16, 16, 60, 4, 1408, 5632, 151936)
    t = e2e.build_llm("tiny-qwen2-moe", "cpu")
    assert t.model.layers[0].self_attn.q_proj.bias is not None and t.model.layers[0].mlp.gate.norm_topk_prob is False
    assert t.model.layers[0].mlp.shared_expert.gate_proj.out_features == 384 and t.model.layers[0].mlp.experts.down_proj.shape == (8, 256, 128)
    m = e2e.build_llm("tiny-mixtral", "cpu")
    assert m.model.layers[0].mlp.experts.down_proj.shape == (8, 256, 512) and m.model.layers[0].mlp.gate.top_k == 2
