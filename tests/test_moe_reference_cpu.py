"""The float64 MoE reference (tests/moe_reference.py) judged on the CPU, before any kernel is measured against it: an f32 PyTorch evaluation
of the contract stays inside every interval on every input set the GPU test uses; HuggingFace's own Qwen3MoeSparseMoeBlock (default experts
implementation) + residual add stays inside, and its `eager` implementation differs only by its bf16 running sum; fourteen mistakes a kernel
of this kind can make leave the interval or change idx; and decoder_layer_declined answers for MoE layers on the CPU."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import moe_reference as MR

BF = torch.bfloat16


def bf(t):
    return t.to(BF).float()


# ------------------------------------------------------------------------------------------------------------------ f32 evaluations
def route_f32(logits, top_k, norm_topk):
    l = logits.float()
    p = torch.softmax(l, dim=-1)
    idx = torch.sort(-l, dim=-1, stable=True).indices[:, :top_k]
    w = p.gather(1, idx)
    if norm_topk:
        w = w / w.sum(-1, keepdim=True)
    return idx.to(torch.int32), bf(w)


def experts_f32(c, idx, w, mistake=None):
    """the contract of ll_moe_experts_bf16 in f32 PyTorch, op by op; ``mistake`` names one deliberate deviation"""
    M, k, I, H = c.M, c.top_k, c.I, c.H
    x = c.x.float()
    denom = I if mistake == "norm-over-I" else H
    rstd = torch.rsqrt((x * x).sum(-1, keepdim=True) / denom + c.eps)
    nw = torch.ones(H) if mistake == "no-norm-weight" else c.norm_w.float()
    xn = bf(nw * bf(x * rstd))
    z = torch.zeros(M, k, H)
    for m in range(M):
        for j in range(k):
            e = int(idx[m, j])
            if mistake == "expert+1":
                e = (e + 1) % c.E
            gu = bf(xn[m] @ c.wgu[e].float().t())
            g, u = gu[:I], gu[I:]
            if mistake in ("up-before-gate", "silu-wrong-half"):      # both read silu off the up half; they are one value, reached two ways
                g, u = u, g
            a = bf(bf(F.silu(g)) * u)
            y = a @ c.wd[e].float().t()
            if mistake == "weight-before-rounding":
                z[m, j] = bf(w[m, j] * y)
            else:
                z[m, j] = bf(w[m, j] * bf(y))
    if mistake == "slot-dropped":
        z[:, -1] = 0
    if mistake == "slot-twice":
        z[:, 0] *= 2
    s = bf(z.sum(1))
    out = bf(c.res.float() + s)
    if mistake == "residual-twice":
        out = bf(c.res.float() + out)
    return out


def test_f32_router_stays_inside_on_every_gpu_set():
    total = free_total = 0
    for norm in (True, False):
        for E in MR.ROUTE_E:
            for k in MR.ROUTE_K:
                for M in MR.ROUTE_M:
                    logits, idx, mid, lo, hi, free = MR.route_case(E, k, M, norm)
                    gi, gw = route_f32(logits, k, norm)
                    assert torch.equal(gi, idx), (E, k, M)
                    assert bool(((gw >= lo) & (gw <= hi)).all()), (E, k, M, norm)
                    total += idx.numel()
                    free_total += free
    print(f"router weights with two accepted values: {free_total} of {total}")
    assert free_total < 0.05 * total      # the window is a rare exception, not a tolerance


@pytest.mark.parametrize("name", sorted(MR.EXPERT_SETS))
def test_f32_experts_stay_inside(name):
    c = MR.experts_case(name)
    bad, ratio = MR.check(experts_f32(c, c.idx, c.w), *c.bounds(c.w))
    assert bad == 0, (name, bad, ratio)


# ------------------------------------------------------------------------------------------------------------------ mistakes
EXPERT_MISTAKES = ("up-before-gate", "silu-wrong-half", "weight-before-rounding", "expert+1", "slot-dropped", "slot-twice", "residual-twice",
                   "no-norm-weight", "norm-over-I")


@pytest.mark.parametrize("mistake", EXPERT_MISTAKES)
def test_expert_mistakes_leave_the_interval(mistake):
    c = MR.experts_case("random-M64-k8-E128" if mistake == "weight-before-rounding" else "ends-M5-k2")
    bad, _ = MR.check(experts_f32(c, c.idx, c.w, mistake), *c.bounds(c.w))
    assert bad > 0, mistake


def test_router_mistakes_change_idx_or_leave_the_window():
    logits, idx, mid, lo, hi, _ = MR.route_case(60, 2, 16, True)
    outside = lambda w: int((~((w >= lo) & (w <= hi))).sum())
    # weights not renormalised / "renormalised" over all experts (the same numbers: the probabilities already sum to one over all experts)
    assert outside(MR.route64(logits, 2, False)[1]) > 0
    assert outside(MR.route64(logits, 2, True, renorm="all")[1]) > 0
    # softmax over the selected logits only: identical to the contract when norm_topk is set, so it is judged where it is not
    l2, i2, m2, lo2, hi2, _ = MR.route_case(60, 2, 16, False)
    wrong = MR.route64(l2, 2, False, softmax_over="selected")[1]
    assert int((~((wrong >= lo2) & (wrong <= hi2))).sum()) > 0
    # top-k by ascending value
    assert not torch.equal(MR.route64(logits, 2, True, select="asc")[0], idx)
    # a tie across the k-th boundary broken toward the higher index
    tie = torch.tensor([[0.0, 1.0, 3.0, 1.0, 1.0, -2.0, 0.5, 1.0]]).to(BF)
    good, high = MR.route64(tie, 2, True)[0], MR.route64(tie, 2, True, select="desc-high")[0]
    assert good.tolist() == [[2, 1]] and high.tolist() == [[2, 7]]


# ------------------------------------------------------------------------------------------------------------------ HF's own block
def _hf_layer(top_k, seed=0):
    from llamole_amd.e2e import build_llm
    model = build_llm("tiny-qwen3-moe", "cpu", seed=seed, num_experts_per_tok=top_k, num_hidden_layers=1)
    layer = model.model.layers[0]
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        layer.post_attention_layernorm.weight.copy_((1 + 0.25 * torch.randn(256, generator=g)).to(BF))
        layer.mlp.gate.weight.copy_((torch.randn(8, 256, generator=g) * 0.2).to(BF))
        layer.mlp.experts.gate_up_proj.copy_((torch.randn(8, 256, 256, generator=g) / 16).to(BF))
        layer.mlp.experts.down_proj.copy_((torch.randn(8, 256, 128, generator=g) * 0.35).to(BF))
    return model, layer


def _hf_out(model, layer, h1, impl):
    model.config._experts_implementation = impl
    with torch.no_grad():
        xn = layer.post_attention_layernorm(h1)
        logits, w, idx = layer.mlp.gate(xn.reshape(-1, 256))
        out = h1 + layer.mlp(xn)
    return logits, w, idx, out.reshape(-1, 256)


def test_hf_block_is_the_reference_and_eager_differs_by_its_bf16_running_sum():
    model, layer = _hf_layer(top_k=4)
    assert model.config._experts_implementation == "grouped_mm"          # HF's default, the contract's path
    g = torch.Generator().manual_seed(11)
    h1 = torch.randn(1, 24, 256, generator=g).to(BF)
    logits, w, idx, out = _hf_out(model, layer, h1, "grouped_mm")
    ridx, mid, lo, hi, _ = MR.route64(logits, 4, True)
    assert torch.equal(idx.to(torch.int32), ridx)
    assert bool(((w.float() >= lo) & (w.float() <= hi)).all())
    x = h1.reshape(-1, 256)
    ex = layer.mlp.experts
    _, _, _, ylo, yhi, ymid = MR.experts_ay(x, layer.post_attention_layernorm.weight.detach(), layer.post_attention_layernorm.variance_epsilon, ridx,
                                            ex.gate_up_proj.detach(), ex.down_proj.detach())
    bounds = MR.finish(ylo, yhi, ymid, w.float(), x)
    bad, _ = MR.check(out, *bounds)
    assert bad == 0
    # eager: index_add_ in ascending expert order keeps the running sum in bf16
    _, w_e, idx_e, out_e = _hf_out(model, layer, h1, "eager")
    assert torch.equal(idx_e, idx) and torch.equal(w_e, w)
    order = torch.sort(ridx, dim=1, stable=True).indices
    bad_eager_form, _ = MR.check(out_e, *MR.finish(ylo, yhi, ymid, w.float(), x, eager_order=order))
    bad_contract, _ = MR.check(out_e, *bounds)
    print(f"HF eager experts: {bad_contract} of {out_e.numel()} outputs outside the contract's interval, {bad_eager_form} outside the bf16-running-sum form")
    assert bad_eager_form == 0 and bad_contract > 0


# ------------------------------------------------------------------------------------------------------------------ eligibility
def test_moe_eligibility_cpu():
    from llamole_amd.e2e import build_llm
    from llamole_amd.llm_accel import decoder_layer_declined
    moe = build_llm("tiny-qwen3-moe", "cpu")
    assert [decoder_layer_declined(l) for l in moe.model.layers] == ["weights are not on the device"] * 2        # nothing structural in the way
    mixed = build_llm("tiny-qwen3-moe", "cpu", mlp_only_layers=[0])
    assert type(mixed.model.layers[0].mlp).__name__ == "Qwen3MoeMLP" and type(mixed.model.layers[1].mlp).__name__ == "Qwen3MoeSparseMoeBlock"
    assert [decoder_layer_declined(l) for l in mixed.model.layers] == ["weights are not on the device"] * 2
    assert decoder_layer_declined(build_llm("tiny-qwen3-moe", "cpu", dtype=torch.float32).model.layers[1]) == "weights are not bf16"
    shared = build_llm("tiny-qwen3-moe", "cpu").model.layers[0]
    shared.mlp.shared_expert = nn.Linear(8, 8)
    assert decoder_layer_declined(shared) == "MoE block of an unsupported kind (shared expert)"
    assert decoder_layer_declined(build_llm("tiny-qwen3-moe", "cpu", num_experts=16, num_experts_per_tok=9).model.layers[0]) == "top_k is not in 1..min(E, 8)"
    assert decoder_layer_declined(build_llm("tiny-qwen3-moe", "cpu", num_experts=257, moe_intermediate_size=8).model.layers[0]) == "more than 256 experts"
    assert decoder_layer_declined(build_llm("tiny-qwen3-moe", "cpu", hidden_act="gelu").model.layers[0]) == "activation is not SiLU"
    assert decoder_layer_declined(build_llm("tiny-qwen3-moe", "cpu", moe_intermediate_size=12).model.layers[0]) == "moe_intermediate_size is not a multiple of 8"
    wide = build_llm("tiny-qwen3-moe", "cpu", hidden_size=8, num_attention_heads=1, num_key_value_heads=1, head_dim=64, num_experts=2,
                     moe_intermediate_size=32776, vocab_size=64).model.layers[0]
    assert decoder_layer_declined(wide) == "moe_intermediate_size above 32768"          # the limit ll_moe_experts_bf16 checks
    other = build_llm("tiny-qwen3-moe", "cpu").model.layers[0]
    other.mlp.__class__ = type("MixtralSparseMoeBlock", (type(other.mlp),), {})
    assert decoder_layer_declined(other) == "MoE block of an unsupported kind (MixtralSparseMoeBlock)"
    # every layout fused before answers what it answered
    for name in ("tiny", "tiny-llama", "tiny-mistral", "tiny-qwen3"):
        assert [decoder_layer_declined(l) for l in build_llm(name, "cpu").model.layers] == ["weights are not on the device"] * 2, name
        assert decoder_layer_declined(build_llm(name, "cpu", dtype=torch.float32).model.layers[0]) == "weights are not bf16", name
    gelu = build_llm("tiny", "cpu", hidden_act="gelu").model.layers[0]
    assert decoder_layer_declined(gelu) == "activation is not SiLU"
