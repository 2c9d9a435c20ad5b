"""The fused decode on sparse-MoE models (`tiny-qwen3-moe`, and the mixed model whose layer 0 is dense): the stack installs, a MoE layer is
eight launches at 1..16 rows and HF's experts code is not called, the captured step gives the tokens of the eager fused step at 1 / 6 / 20 rows,
the fused query-token forward agrees with the op-by-op one on the same cache, one fused decode step agrees with the untouched HF model as well as HF's own bf16
does, `quantization_bit` packs the attention Linears and leaves the experts alone, and a MoE model whose layers are not fused still generates.

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
# launches behind one call of the C ABI (include/llamole_hip.h): ll_moe_experts_bf16 is gate|up, down, slot sum + residual
LAUNCHES = {"ll_moe_experts_bf16": 3}
MODELS = {"moe": {}, "mixed": {"mlp_only_layers": [0]}}


def _restore(llm):
    from llamole_amd.llm_accel import restore_decoder_layers, restore_elementwise, restore_linears, restore_model_decode
    restore_model_decode(llm)
    restore_decoder_layers(llm)
    restore_elementwise(llm)
    restore_linears(llm)


def _build(kind, seed=0):
    llm = e2e.build_llm("tiny-qwen3-moe", "cuda", torch.bfloat16, seed=seed, **MODELS[kind])
    e2e.randomize_head_norms(llm)
    g = torch.Generator().manual_seed(3 + seed)
    with torch.no_grad():                  # HF draws the router at std 0.02: logits that are all but equal; spread them
        for layer in llm.model.layers:
            if hasattr(layer.mlp, "gate"):
                layer.mlp.gate.weight.copy_((torch.randn(layer.mlp.gate.weight.shape, generator=g) * 0.2).to(torch.bfloat16))
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
        assert info["moe_layers_fused"] == (2 if kind == "moe" else 1)
        states = [l._ll_fused for l in llm.model.layers]
        assert isinstance(states[1], _FusedMoeLayer) and (isinstance(states[0], _FusedMoeLayer) == (kind == "moe"))
        assert type(states[0]) is (_FusedMoeLayer if kind == "moe" else _FusedLayer)
        # the expert and router parameters are read in place
        ex = llm.model.layers[1].mlp.experts
        assert states[1].experts is ex and states[1].router is llm.model.layers[1].mlp.gate
        hf_calls = []
        for layer in llm.model.layers:
            if hasattr(layer.mlp, "experts"):
                layer.mlp.experts.forward = lambda *a, _f=layer.mlp.experts.forward, **k: (hf_calls.append(1), _f(*a, **k))[1]
        for B, gemv in ((1, "ll_gemv_fused_bf16"), (6, "ll_linear_rows16_bf16")):
            calls = []
            states[1].lib = _Spy(states[1].lib, calls)
            p, m = _prompts(B)
            dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
            hf_calls.clear()
            dec.generate(p, m, max_new_tokens=2, **KW)         # prefill (HF modules) + ONE fused decode step
            states[1].lib = states[1].lib._lib
            want = [gemv, "ll_decode_attn_rope_qkn_bf16", gemv, gemv, "ll_moe_route_bf16", "ll_moe_experts_bf16"]
            assert calls == want, (B, calls)
            assert sum(LAUNCHES.get(c, 1) for c in calls) == 8
            # HF's experts ran in the prefill only: once per MoE layer
            assert len(hf_calls) == info["moe_layers_fused"], (B, len(hf_calls))
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
                # the query-token forward (9 positions): the fused path against the op-by-op path on the same cache (LLAMOLE_FUSED_SUFFIX=0), at the
                # tolerance tests/test_llm_decode.py holds the dense layouts to
                g = torch.Generator().manual_seed(9)
                p1 = torch.randint(5, 2000, (1, 20), generator=g).cuda()
                tail = torch.randint(5, 2000, (1, 9), generator=g).cuda()
                hid = {}
                for mode in ("0", "1"):
                    monkeypatch.setenv("LLAMOLE_FUSED_SUFFIX", mode)
                    dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
                    dec.generate(p1, torch.ones_like(p1), max_new_tokens=16, **KW)
                    seen.clear()
                    hid[mode] = dec.continue_hidden(tail, 20 + 16 - 9).float().clone()
                    assert ("suffix" in seen) == (mode == "1")
                err = float((hid["0"] - hid["1"]).abs().max() / hid["0"].abs().max())
                print(f"\n{kind}: query-token forward, fused against op-by-op: max |diff| / max |h| = {err:.5f}")
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
    same experts in every MoE layer for every row of that step: Y is then a rounding yardstick, not a routing flip.  Controls: the fused layers
    with the router's rows permuted, or with norm_topk inverted, miss the bound by far."""
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
        # controls, inside the fused layers only (the prefill still runs HF's modules, so the same step is compared)
        moe_states = [l._ll_fused for l in llm.model.layers if hasattr(l.mlp, "gate")]
        for st in moe_states:
            st.norm_topk = not st.norm_topk
        toks1, wrong = _step_logits(llm, prompt, mask)
        assert torch.equal(toks1[:, :14], ids)
        E1 = float((wrong - ref).abs().max())
        for st in moe_states:
            st.norm_topk = not st.norm_topk
            st.router = type("Permuted", (), {"weight": st.router.weight.detach().roll(1, 0).contiguous()})()
        toks2, wrong = _step_logits(llm, prompt, mask)
        assert torch.equal(toks2[:, :14], ids)
        E2 = float((wrong - ref).abs().max())
        print(f"controls: norm_topk inverted E = {E1:.5f}, router rows permuted E = {E2:.5f}")
        assert E1 > MARGIN * Y and E2 > MARGIN * Y
    finally:
        _restore(llm)


def test_quantised_mixed_model_packs_attention_and_leaves_the_experts(monkeypatch):
    from llamole_amd import llm_accel
    from llamole_amd.llm_accel import accelerate_llm, set_packed_route
    monkeypatch.setattr(llm_accel, "WQ_ROUTES", llm_accel.all_packed_routes())
    llm = _build("mixed")
    ex = llm.model.layers[1].mlp
    before = [t.clone() for t in (ex.experts.gate_up_proj, ex.experts.down_proj, ex.gate.weight)]
    p, m = _prompts(2)
    try:
        info = accelerate_llm(llm, quantization_bit=4)
        q = info["quantization"]
        assert q["bits"] == 4 and q["modules"] == 7 + 4 and q["packed_layers"] == 2 and q["experts"] == "bf16"
        assert info["decoder_layers_5_launches"] == 2 and info["moe_layers_fused"] == 1 and "decoder_layers_declined" not in info
        assert all(torch.equal(a, b) for a, b in zip(before, (ex.experts.gate_up_proj, ex.experts.down_proj, ex.gate.weight)))
        assert len(llm.model.layers[1]._ll_fused.pq) == 2 and len(llm.model.layers[0]._ll_fused.pq) == 4
        dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
        packed = dec.generate(p, m, max_new_tokens=6, **KW)
        assert dec._graph is not None
        assert set_packed_route(llm, False) == 2
        plain = GraphedDecoder(llm, use_graph=True, fused_cache=True).generate(p, m, max_new_tokens=6, **KW)
        assert torch.equal(packed, plain)
    finally:
        _restore(llm)


def test_a_moe_model_whose_layers_are_not_fused_still_generates():
    """accelerate_llm(layers=False): HF's own MoE block under the graphed decoder -- captured, or eager with one warning where the installed
    transformers / torch cannot capture its step; either way the tokens of the decoder built with use_graph=False."""
    from llamole_amd.llm_accel import accelerate_llm
    llm = _build("moe")
    p, m = _prompts(2)
    try:
        info = accelerate_llm(llm, layers=False)
        assert "decoder_layers_5_launches" not in info
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
            got = dec.generate(p, m, max_new_tokens=6, **KW)
        assert len(rec) <= 1, [str(w.message) for w in rec]
        print(f"\nunfused MoE model under GraphedDecoder: step captured = {dec._graph is not None}, experts implementation "
              f"{llm.config._experts_implementation}, warnings {[str(w.message)[:80] for w in rec]}")
        eager = GraphedDecoder(llm, use_graph=False, fused_cache=True).generate(p, m, max_new_tokens=6, **KW)
        assert torch.equal(got, eager)
    finally:
        _restore(llm)
