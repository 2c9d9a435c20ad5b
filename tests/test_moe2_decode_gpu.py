"""The fused decode on the Mixtral and shared-expert (Qwen2-MoE) layouts (`tiny-mixtral`, `tiny-qwen2-moe`, and the mixed `tiny-qwen2-moe`
whose layer 0 is dense): the stack installs and every layer is fused, a MoE layer is eight (Mixtral) / ten (Qwen2-MoE) launches at 1 and 6 rows
and HF's experts code runs in the prefill only, the captured step gives the tokens of the eager fused step at 1 / 6 / 20 rows, the fused
query-token forward agrees with the op-by-op one, one fused decode step agrees with the untouched HF model as well as HF's own bf16 does, and
beams and the MX8 cache give the tokens of the same model with its layers left to HF.

E, Y and the controls of the step test, and the query-token difference, are printed with -s."""
import copy
import warnings

import pytest
import torch

from llamole_amd import e2e
from llamole_amd.llm_decode import GraphedDecoder

pytestmark = pytest.mark.gpu

MARGIN = 1.5            # a bf16 engine against the reference's own bf16: the project's margin of record
KW = dict(do_sample=False, pad_token_id=0, eos_token_id=[])
# launches behind one call of the C ABI (include/llamole_hip.h): gate|up, down, slot sum + residual
LAUNCHES = {"ll_moe_experts_bf16": 3, "ll_moe_experts_ex_bf16": 3}
MODELS = {"mixtral": ("tiny-mixtral", {}), "qwen2": ("tiny-qwen2-moe", {}), "qwen2-mixed": ("tiny-qwen2-moe", {"mlp_only_layers": [0]})}


def _restore(llm):
    from llamole_amd.llm_accel import restore_decoder_layers, restore_elementwise, restore_linears, restore_model_decode
    restore_model_decode(llm)
    restore_decoder_layers(llm)
    restore_elementwise(llm)
    restore_linears(llm)


def _build(kind, seed=0):
    name, overrides = MODELS[kind]
    llm = e2e.build_llm(name, "cuda", torch.bfloat16, seed=seed, **overrides)
    g = torch.Generator().manual_seed(3 + seed)
    with torch.no_grad():                  # HF draws the router and the shared gate at std 0.02: logits that are all but equal; spread them
        for layer in llm.model.layers:
            if hasattr(layer.mlp, "gate"):
                layer.mlp.gate.weight.copy_((torch.randn(layer.mlp.gate.weight.shape, generator=g) * 0.2).to(torch.bfloat16))
            if hasattr(layer.mlp, "shared_expert_gate"):
                layer.mlp.shared_expert_gate.weight.copy_((torch.randn(1, 256, generator=g) * 0.2).to(torch.bfloat16))
    return llm


class _Spy:
    """stands in for the library handle of one fused layer and records the entry points it calls"""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self._calls.append(name)
            return fn(*a)
        return call


def _prompts(B, P=12, seed=21):
    g = torch.Generator().manual_seed(seed + B)
    p = torch.randint(5, 2000, (B, P), generator=g).cuda()
    m = torch.ones_like(p)
    if B > 1:
        m[0, :3] = 0                      # left padding
    return p, m


@pytest.mark.parametrize("kind", sorted(MODELS))
def test_installation_launch_count_and_no_hf_experts(kind):
    from llamole_amd.llm_accel import _FusedLayer, _FusedMoeLayer, accelerate_llm
    llm = _build(kind)
    try:
        info = accelerate_llm(llm)
        assert info["decoder_layers_5_launches"] == 2 and info["decode_prologue_1_launch"] is True
        assert not [k for k in info if k.endswith("_declined")]
        assert info["moe_layers_fused"] == (1 if kind == "qwen2-mixed" else 2)
        states = [l._ll_fused for l in llm.model.layers]
        assert type(states[1]) is _FusedMoeLayer and type(states[0]) is (_FusedLayer if kind == "qwen2-mixed" else _FusedMoeLayer)
        st = states[1]
        assert st.w_f32 == (kind == "mixtral") and (st.shared is not None) == (kind != "mixtral")
        assert st.w.dtype == (torch.float32 if kind == "mixtral" else torch.bfloat16)
        hf_calls = []
        for layer in llm.model.layers:
            if hasattr(layer.mlp, "experts"):
                layer.mlp.experts.forward = lambda *a, _f=layer.mlp.experts.forward, **k: (hf_calls.append(1), _f(*a, **k))[1]
        for B, gemv in ((1, "ll_gemv_fused_bf16"), (6, "ll_linear_rows16_bf16")):
            calls = []
            st.lib = _Spy(st.lib, calls)
            p, m = _prompts(B)
            dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
            hf_calls.clear()
            dec.generate(p, m, max_new_tokens=2, **KW)         # prefill (HF modules) + ONE fused decode step
            st.lib = st.lib._lib
            if kind == "mixtral":
                want, n = [gemv, "ll_decode_attn_rope_bf16", gemv, gemv, "ll_moe_route_f32", "ll_moe_experts_ex_bf16"], 8
            else:       # q|k|v, attention, o_proj, router + gate logits, route, shared gate|up, shared down, experts (3)
                want, n = [gemv, "ll_decode_attn_rope_bf16", gemv, gemv, "ll_moe_route_bf16", gemv, gemv, "ll_moe_experts_ex_bf16"], 10
            assert calls == want, (B, calls)
            assert sum(LAUNCHES.get(c, 1) for c in calls) == n
            # HF's experts ran in the prefill only: once per MoE layer
            assert len(hf_calls) == info["moe_layers_fused"], (B, len(hf_calls))
        if kind != "mixtral":
            # the stacked [E + 1, H] copy of the router and the shared gate follows its sources, in place
            from llamole_amd.llm_accel import refresh_weight_copies
            mlp = llm.model.layers[1].mlp
            assert st.router_w.shape == (9, 256) and torch.equal(st.router_w[8:], mlp.shared_expert_gate.weight)
            assert refresh_weight_copies(llm) == 0
            ptr = st.router_w.data_ptr()
            with torch.no_grad():
                mlp.shared_expert_gate.weight.mul_(2)
                mlp.shared_expert.up_proj.weight.mul_(2)
            assert refresh_weight_copies(llm) == 2
            assert st.router_w.data_ptr() == ptr and torch.equal(st.router_w[8:], mlp.shared_expert_gate.weight)
            assert torch.equal(st.wgu_s[384:], mlp.shared_expert.up_proj.weight)
    finally:
        _restore(llm)


@pytest.mark.parametrize("kind", sorted(MODELS))
def test_graphed_decode_equals_the_eager_fused_decode(kind, monkeypatch):
    from llamole_amd.llm_accel import _FusedLayer, _FusedMoeLayer, accelerate_llm
    llm = _build(kind)
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            accelerate_llm(llm)
            seen = []
            orig64, orig_sfx = _FusedMoeLayer.run64, _FusedLayer.run_suffix
            _FusedMoeLayer.run64 = lambda self, *a, **k: (seen.append("run64"), orig64(self, *a, **k))[1]
            _FusedLayer.run_suffix = lambda self, *a, **k: (seen.append("suffix"), orig_sfx(self, *a, **k))[1]
            try:
                for B in (1, 6, 20):
                    p, m = _prompts(B)
                    dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
                    eager = GraphedDecoder(llm, use_graph=False, fused_cache=True)
                    got = dec.generate(p, m, max_new_tokens=8, **KW)
                    assert dec._graph is not None, B
                    assert torch.equal(got, eager.generate(p, m, max_new_tokens=8, **KW)), B
                    skw = dict(max_new_tokens=8, do_sample=True, temperature=0.6, top_p=0.9, top_k=50, pad_token_id=0, eos_token_id=[])
                    a = dec.generate(p, m, generator=torch.Generator(device="cuda").manual_seed(5), **skw)
                    b = eager.generate(p, m, generator=torch.Generator(device="cuda").manual_seed(5), **skw)
                    assert torch.equal(a, b), B
                assert "run64" in seen
                # the query-token forward (9 positions): the fused path against the op-by-op path on the same cache (LLAMOLE_FUSED_SUFFIX=0), at
                # the bound tests/test_moe_decode_gpu.py uses.  Routing is discrete: the two paths compute the router logits with different kernels
                # (one bf16 step apart at most), and where a row's k-th and (k+1)-th logits tie one of them takes another expert -- a different
                # model output, not a rounding.  As in the step test below the input is therefore the first seed in 9..16 at which both paths
                # select the same experts in every MoE layer at every position (chosen on the routing alone, before any difference is looked at)
                routed = {"0": [], "1": []}
                orig_mlp = _FusedMoeLayer._mlp
                # (only the 9-row calls of the query-token forward are recorded: the decode steps and the prompt pass have other row counts)
                _FusedMoeLayer._mlp = lambda self, h1, *a, **k: (orig_mlp(self, h1, *a, **k),
                                                                  routed["1"].append(self.idx[:9].clone()) if h1.shape[0] == 9 else None)[0]
                hooks = [l.mlp.gate.register_forward_hook(lambda mod, a, out: routed["0"].append(out[2].to(torch.int32)) if out[2].shape[0] == 9 else None)
                         for l in llm.model.layers if hasattr(l.mlp, "gate")]
                try:
                    chosen = None
                    for seed in range(9, 17):
                        g = torch.Generator().manual_seed(seed)
                        p1 = torch.randint(5, 2000, (1, 20), generator=g).cuda()
                        tail = torch.randint(5, 2000, (1, 9), generator=g).cuda()
                        hid = {}
                        for mode in ("0", "1"):
                            monkeypatch.setenv("LLAMOLE_FUSED_SUFFIX", mode)
                            dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
                            dec.generate(p1, torch.ones_like(p1), max_new_tokens=16, **KW)
                            seen.clear()
                            routed[mode].clear()
                            hid[mode] = dec.continue_hidden(tail, 20 + 16 - 9).float().clone()
                            assert ("suffix" in seen) == (mode == "1")
                        assert len(routed["0"]) == len(routed["1"]) == len(hooks), (len(routed["0"]), len(routed["1"]))
                        if all(torch.equal(a.sort(-1).values, b.sort(-1).values) for a, b in zip(routed["0"], routed["1"])):
                            chosen = seed
                            break
                        # a seed passed over must not hide a real difference: attention is causal, so every position in front of the first one
                        # that is routed differently (in any layer) saw equal routings only, and is held to the same bound
                        differs = torch.stack([(a.sort(-1).values != b.sort(-1).values).any(-1) for a, b in zip(routed["0"], routed["1"])]).any(0)
                        first = int(differs.nonzero()[0])
                        per_pos = (hid["0"] - hid["1"]).abs().amax(-1).flatten() / hid["0"].abs().max()
                        print(f"\n{kind}: seed {seed} passed over, positions routed differently {differs.nonzero().flatten().tolist()}; "
                              f"max |diff| / max |h| per position {[round(float(v), 4) for v in per_pos]}")
                        assert float(per_pos[:first].max()) <= 3e-2 if first else True, (seed, first, per_pos)
                finally:
                    _FusedMoeLayer._mlp = orig_mlp
                    for h in hooks:
                        h.remove()
                assert chosen is not None, "no seed in 9..16 at which the fused and the op-by-op query-token forward route alike"
                err = float((hid["0"] - hid["1"]).abs().max() / hid["0"].abs().max())
                print(f"\n{kind}: seed {chosen}; query-token forward, fused against op-by-op: max |diff| / max |h| = {err:.5f}")
                assert err <= 3e-2
            finally:
                _FusedMoeLayer.run64, _FusedLayer.run_suffix = orig64, orig_sfx
        assert not rec, [str(w.message) for w in rec]
    finally:
        _restore(llm)


def _step_logits(llm, prompt, mask):
    dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
    toks = dec.generate(prompt, mask, max_new_tokens=2, **KW)
    return toks, dec.last_logits.float().clone()


def _hf_logits_and_routing(model, ids, mask):
    """logits of the last position and the experts every MoE layer selects for it, per row"""
    pos = (mask.long().cumsum(dim=1) - 1).clamp_min(0)
    picked = []
    hooks = [l.mlp.gate.register_forward_hook(lambda mod, a, out: picked.append(out[2].view(ids.shape[0], -1, out[2].shape[-1])[:, -1].sort(-1).values))
             for l in model.model.layers if hasattr(l.mlp, "gate")]
    try:
        with torch.no_grad():
            logits = model(input_ids=ids, attention_mask=mask, position_ids=pos, use_cache=False).logits[:, -1, :].float()
    finally:
        for h in hooks:
            h.remove()
    return logits, torch.stack(picked)


@pytest.mark.parametrize("kind", sorted(MODELS))
def test_one_fused_decode_step_against_hf(kind):
    """3 left-padded rows of 13 tokens, greedy, max_new_tokens = 2: last_logits are those of one fused decode step.  E = max |fused - HF f32|,
    Y = max |HF bf16 - HF f32|, E <= 1.5 Y.  Routing is discrete, so the input is the first seed in 0..15 for which HF bf16 and HF f32 select the
    same experts in every MoE layer for every row of that step.  Controls, inside the fused layers only (the prefill still runs HF's modules):
    the shared gate's row of the stacked router copy zeroed (sigmoid(0) = 0.5 on every row), and the Mixtral weights rounded to bf16 (the Qwen3
    contract: ll_moe_route_bf16 + ll_moe_experts_bf16); both must move E."""
    from llamole_amd.llm_accel import accelerate_llm
    llm = _build(kind)
    hf16, hf32 = copy.deepcopy(llm), copy.deepcopy(llm).float()
    mask = torch.ones(3, 13, dtype=torch.long, device="cuda")
    mask[1, :4] = 0
    mask[2, :7] = 0
    full = torch.cat([mask, torch.ones_like(mask[:, :1])], dim=1)
    try:
        info = accelerate_llm(llm)
        assert info["decoder_layers_5_launches"] == 2 and info["decode_prologue_1_launch"]
        chosen = None
        for seed in range(16):
            prompt = torch.randint(5, 2000, (3, 13), generator=torch.Generator().manual_seed(100 + seed)).cuda()
            toks, fused = _step_logits(llm, prompt, mask)
            ids = toks[:, :14]
            ref, r32 = _hf_logits_and_routing(hf32, ids, full)
            l16, r16 = _hf_logits_and_routing(hf16, ids, full)
            if torch.equal(r32, r16):
                chosen = seed
                break
        assert chosen is not None, "no seed in 0..15 on which HF bf16 and HF f32 route alike"
        Y = float((l16 - ref).abs().max())
        E = float((fused - ref).abs().max())
        print(f"\n{kind}: seed {chosen}; one decode step, max |logit error| against HF f32: fused E = {E:.5f}, HF bf16 Y = {Y:.5f}, E / Y = {E / Y:.3f}")
        assert Y > 0 and E <= MARGIN * Y, (E, Y)
        moe_states = [l._ll_fused for l in llm.model.layers if hasattr(l.mlp, "gate")]
        if kind == "mixtral":
            for st in moe_states:
                st.w_f32, st.w = False, torch.zeros_like(st.w, dtype=torch.bfloat16)
            what = "weights rounded to bf16"
        else:
            for st in moe_states:
                st.router_w[st.E].zero_()
            what = "shared gate weight zeroed"
        toks1, wrong = _step_logits(llm, prompt, mask)
        assert torch.equal(toks1[:, :14], ids)
        E1 = float((wrong - ref).abs().max())
        print(f"control: {what}: E = {E1:.5f}, E / Y = {E1 / Y:.3f}, max |logit change| = {float((wrong - fused).abs().max()):.5f}")
        assert E1 != E and not torch.equal(wrong, fused)
    finally:
        _restore(llm)


@pytest.mark.parametrize("kind", ["mixtral", "qwen2"])
def test_beams_and_the_mx8_cache_give_the_tokens_of_the_unfused_layers(kind):
    """num_beams = 2 and kv_cache = "mxfp8": the tokens of the same model with accelerate_llm(layers=False) on the same cache format."""
    from llamole_amd.llm_accel import accelerate_llm
    llm, plain = _build(kind), _build(kind)
    p, m = _prompts(2)
    try:
        info = accelerate_llm(llm)
        assert info["moe_layers_fused"] == 2 and "decoder_layers_5_launches" not in accelerate_llm(plain, layers=False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")         # the unfused MoE step may run eagerly with one warning (tests/test_moe_decode_gpu.py)
            for dec_kw, gen_kw in (({}, dict(num_beams=2)), (dict(kv_cache="mxfp8"), {})):
                got = GraphedDecoder(llm, use_graph=True, fused_cache=True, **dec_kw).generate(p, m, max_new_tokens=6, **KW, **gen_kw)
                want = GraphedDecoder(plain, use_graph=True, fused_cache=True, **dec_kw).generate(p, m, max_new_tokens=6, **KW, **gen_kw)
                assert torch.equal(got, want), (dec_kw, gen_kw, got, want)
    finally:
        _restore(llm)
        _restore(plain)


def test_quantised_qwen2_moe_rounds_the_shared_expert_and_packs_the_attention(monkeypatch):
    from llamole_amd import llm_accel
    from llamole_amd.llm_accel import accelerate_llm, set_packed_route
    monkeypatch.setattr(llm_accel, "WQ_ROUTES", llm_accel.all_packed_routes())
    llm = _build("qwen2")
    mlp = llm.model.layers[1].mlp
    before = [t.clone() for t in (mlp.experts.gate_up_proj, mlp.experts.down_proj, mlp.gate.weight, mlp.shared_expert_gate.weight)]
    shared_before = mlp.shared_expert.down_proj.weight.clone()
    p, m = _prompts(2)
    try:
        info = accelerate_llm(llm, quantization_bit=4)
        q = info["quantization"]
        assert q["bits"] == 4 and q["modules"] == 2 * (4 + 3) and q["packed_layers"] == 2 and q["experts"] == "bf16" and q["shared_expert"] == "bf16"
        assert info["decoder_layers_5_launches"] == 2 and info["moe_layers_fused"] == 2 and "decoder_layers_declined" not in info
        assert all(torch.equal(a, b) for a, b in zip(before, (mlp.experts.gate_up_proj, mlp.experts.down_proj, mlp.gate.weight,
                                                              mlp.shared_expert_gate.weight)))
        assert not torch.equal(shared_before, mlp.shared_expert.down_proj.weight)          # rounded like any nn.Linear
        st = llm.model.layers[1]._ll_fused
        assert len(st.pq) == 2 and torch.equal(st.wdown_s, mlp.shared_expert.down_proj.weight)
        dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
        packed = dec.generate(p, m, max_new_tokens=6, **KW)
        assert dec._graph is not None
        assert set_packed_route(llm, False) == 2
        plain = GraphedDecoder(llm, use_graph=True, fused_cache=True).generate(p, m, max_new_tokens=6, **KW)
        assert torch.equal(packed, plain)
    finally:
        _restore(llm)
