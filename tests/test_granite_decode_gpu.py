"""The fused decode on a Granite-layout model (`tiny-granite`: the Llama layout plus embedding_multiplier 12.0, attention_multiplier 2^-7,
residual_multiplier 0.22, logits_scaling 8.0): every layer is fused and the prologue installed, the residual adds go through the scaled
entries and the embedding through ll_embed_rows_bf16 at 1, 6 and 20 rows; one decode step agrees with the untouched HF model in f32 as well
as HF's own bf16 does (E <= 1.5 Y), while the same fused step WITHOUT the two multipliers -- what ran before the layout
was served -- misses that by far; greedy tokens equal HF's over 16 tokens on a prompt whose top-2 logit gap stays above 8 bf16 ulps; the
captured step gives the tokens of the eager step; the fused query-token forward agrees with the op-by-op one; `quantization_bit` keeps these
layers on the bf16 kernels and says why; `tiny-llama` calls the entries it called.

E, Y and E / Y are printed with -s; the figures measured on an MI355X are in DESIGN.md 4w."""
import copy
import math
import warnings

import pytest
import torch

from llamole_amd import e2e
from llamole_amd.llm_decode import GraphedDecoder
from tests.test_kv8_decode_gpu import KW, _prompts, _restore, _Spy

pytestmark = pytest.mark.gpu

MARGIN = 1.5            # a bf16 engine against the reference's own bf16: the project's margin of record
# test_greedy_tokens_equal_hf: weight seed, prompt generator seed and row, picked on the CPU (the gap is asserted, not assumed)
GREEDY_WEIGHT_SEED, GREEDY_PROMPT_SEED, GREEDY_PROMPT_ROW = 3, 100, 632
MIN_GAP_ULPS = 8.0
HOST_QUERIES = ("workspace", "ssq_chunks", "packed_elems", "rows64_pack")     # host code and the one-off weight packing, not launches of a step


def _build(name="tiny-granite"):
    llm = e2e.build_llm(name, "cuda", torch.bfloat16)
    if name == "tiny-granite":
        assert type(llm).__name__ == "GraniteForCausalLM" and llm.model.layers[0].residual_multiplier == 0.22
        assert llm.model.embedding_multiplier == 12.0 and llm.config.logits_scaling == 8.0
    return llm


def _step_calls(llm, B):
    """(per-layer entry points, model-level entry points) of ONE decode step: a two-token generate whose prefill runs HF's modules"""
    states = [l._ll_fused for l in llm.model.layers]
    per_layer = [[] for _ in states]
    top = []
    st = llm.model._ll_decode
    for s, calls in zip(states, per_layer):
        s.lib = _Spy(s.lib, calls)
    st["lib"] = _Spy(st["lib"], top)
    try:
        p, m = _prompts(B)
        GraphedDecoder(llm, use_graph=False, fused_cache=True).generate(p, m, max_new_tokens=2, **KW)
    finally:
        for s in states:
            s.lib = s.lib._lib
        st["lib"] = st["lib"]._lib
    return [[c for c in calls if not any(h in c for h in HOST_QUERIES)] for calls in per_layer], top


def _launches(calls, last):
    """launches behind a layer's entry calls, DERIVED from the entry names and the launcher's rule, not observed: a rows64 call that takes
    the K-split path is two launches (main + slab sum).  At these widths (K <= 512: one x stage) the launcher takes it only when a pre-norm
    is handed on, which the last layer's down_proj does not do: 7 launches per layer at 20 rows, 6 for the last layer."""
    n = 0
    for i, c in enumerate(calls):
        split = c in ("ll_linear_rows64_rs_bf16", "ll_linear_rows64_bf16") and i in (2, 4) and not (last and i == 4)
        n += 2 if split else 1
    return n


def _expected(B, scaled, first):
    if B > 16:
        lin, res = "ll_linear_rows64_bf16", "ll_linear_rows64_rs_bf16" if scaled else "ll_linear_rows64_bf16"
    elif B > 2:
        lin, res = "ll_linear_rows16_bf16", "ll_linear_rows16_rs_bf16" if scaled else "ll_linear_rows16_bf16"
    else:
        lin, res = "ll_gemv_fused_bf16", "ll_gemv_fused_rs_bf16" if scaled else "ll_gemv_fused_bf16"
    pre = ["ll_rows64_prenorm_bf16"] if (B > 16 and first) else []
    return pre + [lin, "ll_decode_attn_rope_bf16", res, lin, res]


def test_every_layer_fused_and_the_scaled_entries_are_the_ones_called():
    from llamole_amd.llm_accel import accelerate_llm
    llm = _build()
    try:
        info = accelerate_llm(llm)
        L = llm.config.num_hidden_layers
        assert info["decoder_layers_5_launches"] == L == 2 and info["decode_prologue_1_launch"] is True
        assert not [k for k in info if k.endswith("_declined")], info
        assert all(l._ll_fused.rscale == 0.22 and l._ll_fused.scaling == 0.0078125 for l in llm.model.layers)
        assert llm.model._ll_decode["embed_scale"] == 12.0
        for B in (1, 6, 20):
            layers, top = _step_calls(llm, B)
            for i, calls in enumerate(layers):
                assert calls == _expected(B, True, i == 0), (B, i, calls)
                body = calls[1:] if calls[0] == "ll_rows64_prenorm_bf16" else calls
                assert _launches(body, i == L - 1) == (5 if B <= 16 else (7 if i < L - 1 else 6)), (B, i, calls)
            assert top == ["ll_embed_rows_bf16", "ll_decode_prologue"], (B, top)       # one embedding launch, one prologue launch
    finally:
        _restore(llm)


def test_tiny_llama_calls_the_entries_it_called():
    from llamole_amd.llm_accel import accelerate_llm
    llm = _build("tiny-llama")
    try:
        info = accelerate_llm(llm)
        assert info["decoder_layers_5_launches"] == 2 and info["decode_prologue_1_launch"] is True
        assert all(l._ll_fused.rscale is None for l in llm.model.layers) and "embed_scale" not in llm.model._ll_decode
        for B in (1, 6, 20):
            layers, top = _step_calls(llm, B)
            for i, calls in enumerate(layers):
                assert calls == _expected(B, False, i == 0), (B, i, calls)
            assert top == ["ll_decode_prologue"], (B, top)
    finally:
        _restore(llm)


def _step_logits(llm, prompt):
    dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
    toks = dec.generate(prompt, torch.ones_like(prompt), max_new_tokens=2, **KW)
    return toks, dec.last_logits.float().clone()


def _hf_logits(model, ids):
    with torch.no_grad():
        return model(input_ids=ids, use_cache=False).logits[:, -1, :].float()


def test_one_decode_step_against_hf():
    """1 row of 13 tokens, greedy, max_new_tokens = 2: last_logits are those of one fused decode step.  Reference: the untouched HF model in
    f32 on prompt + first token; Y = max |HF bf16 - reference|; E = max |fused - reference| <= 1.5 Y.  Control: the same fused step with the
    residual and embedding multipliers dropped (the arithmetic of the Llama layout, which is what these layers ran before) misses it by far."""
    from llamole_amd.llm_accel import accelerate_llm
    llm = _build()
    hf16, hf32 = copy.deepcopy(llm), copy.deepcopy(llm).float()
    prompt = torch.randint(5, 2000, (1, 13), generator=torch.Generator().manual_seed(13)).cuda()
    try:
        info = accelerate_llm(llm)
        assert info["decoder_layers_5_launches"] == 2 and info["decode_prologue_1_launch"]
        toks, fused = _step_logits(llm, prompt)
        ids = toks[:, :14]
        ref = _hf_logits(hf32, ids)
        Y = float((_hf_logits(hf16, ids) - ref).abs().max())
        E = float((fused - ref).abs().max())
        print(f"\ntiny-granite one decode step, max |logit error| against HF f32: fused E = {E:.5f}, HF bf16 Y = {Y:.5f}, E / Y = {E / Y:.3f}")
        assert Y > 0 and E <= MARGIN * Y, (E, Y)
        for layer in llm.model.layers:
            layer._ll_fused.rscale = None
        del llm.model._ll_decode["embed_scale"]
        toks0, wrong = _step_logits(llm, prompt)
        assert torch.equal(toks0[:, :14], ids)                      # the same prefill (HF's modules) and first token: the same step is compared
        E0 = float((wrong - ref).abs().max())
        print(f"control, multipliers dropped in the fused step: E = {E0:.5f}, E / Y = {E0 / Y:.1f}")
        assert E0 > MARGIN * Y
    finally:
        _restore(llm)


def _bf16_ulp(x):
    return 2.0 ** (math.floor(math.log2(abs(x))) - 7)


def test_greedy_tokens_equal_hf():
    """16 greedy tokens against HF's own generate (the untouched bf16 model).  The comparison means something only where the argmax is not a
    matter of rounding: at every step the float64 gap between the two largest logits of HF f32 is asserted to exceed 8 bf16 ulps.
    Random-init logits are near-ties, so the case was searched on the CPU: weights of build_llm(seed = 3) drawn on the CPU (the device
    generator draws other weights), row 632 of 4096 prompts of generator seed 100 -- smallest gap 10.5 ulps over the 16 steps, seven
    distinct tokens.  Control: the fused layers with the residual multiplier dropped decode other tokens (as HF f32 with
    residual_multiplier = 1 does on the CPU), so the equality is owed to the scaled epilogue."""
    from llamole_amd.llm_accel import accelerate_llm
    llm = e2e.build_llm("tiny-granite", "cpu", torch.bfloat16, seed=GREEDY_WEIGHT_SEED).cuda()
    assert llm.lm_head.weight.data_ptr() != llm.model.embed_tokens.weight.data_ptr() and llm.model.layers[0].residual_multiplier == 0.22
    hf16, hf32 = copy.deepcopy(llm), copy.deepcopy(llm).float()
    prompts = torch.randint(5, 2000, (4096, 12), generator=torch.Generator().manual_seed(GREEDY_PROMPT_SEED))
    prompt = prompts[GREEDY_PROMPT_ROW:GREEDY_PROMPT_ROW + 1].cuda()
    ids, worst = prompt, math.inf
    for _ in range(16):
        top = _hf_logits(hf32, ids)[0].double().topk(2)
        a, b = float(top.values[0]), float(top.values[1])
        worst = min(worst, (a - b) / _bf16_ulp(max(abs(a), abs(b))))
        ids = torch.cat([ids, top.indices[:1][None]], dim=1)
    print(f"\nsmallest top-2 gap over 16 steps: {worst:.2f} bf16 ulps; tokens {ids[0, 12:].tolist()}")
    assert worst > MIN_GAP_ULPS, worst
    with torch.no_grad():
        want = hf16.generate(prompt, attention_mask=torch.ones_like(prompt), max_new_tokens=16, do_sample=False, pad_token_id=0, eos_token_id=None)
    assert torch.equal(want, ids)
    try:
        accelerate_llm(llm)
        for use_graph in (False, True):
            got = GraphedDecoder(llm, use_graph=use_graph, fused_cache=True).generate(prompt, torch.ones_like(prompt), max_new_tokens=16, **KW)
            assert torch.equal(got, want), (use_graph, got, want)
        for layer in llm.model.layers:
            layer._ll_fused.rscale = None
        wrong = GraphedDecoder(llm, use_graph=False, fused_cache=True).generate(prompt, torch.ones_like(prompt), max_new_tokens=16, **KW)
        assert not torch.equal(wrong, want), "the residual multiplier dropped from the fused layers decodes the same 16 tokens"
    finally:
        _restore(llm)


def test_captured_step_equals_the_eager_step_and_query_forward_agrees(monkeypatch):
    from llamole_amd.llm_accel import _FusedLayer, accelerate_llm
    llm = _build()
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            accelerate_llm(llm)
            seen = []
            orig_sfx = _FusedLayer.run_suffix
            monkeypatch.setattr(_FusedLayer, "run_suffix", lambda self, *a, **k: (seen.append("suffix"), orig_sfx(self, *a, **k))[1])
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
            # the query-token forward (9 positions): the fused path (ll_embed_rows_bf16, ll_linear_rows16_rs_bf16) against HF's modules
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
            print(f"\ntiny-granite: query-token forward, fused against op-by-op: max |diff| / max |h| = {err:.5f}")
            assert err <= 3e-2
        assert not rec, [str(w.message) for w in rec]
    finally:
        _restore(llm)


def test_quantization_bit_keeps_the_bf16_kernels_and_says_why():
    """quantization_bit = 8: the seven Linears of each layer are rounded onto the MX grid (module.weight overwritten: every path computes the
    same model), no packed codes are kept, the info names the reason, and the captured step still gives the tokens of its own eager step."""
    from llamole_amd.llm_accel import WQ_RESIDUAL_MULTIPLIER_REASON, accelerate_llm
    from llamole_amd.llm_quant import mx_round
    llm = _build()
    w0 = llm.model.layers[0].mlp.down_proj.weight.detach().clone()
    try:
        info = accelerate_llm(llm, quantization_bit=8)
        q = info["quantization"]
        assert q["bits"] == 8 and q["modules"] == 14 and q["packed_layers"] == 0 and q["bf16_layers"] == 2
        assert q["bf16_reason"] == WQ_RESIDUAL_MULTIPLIER_REASON
        assert info["decoder_layers_5_launches"] == 2 and not [k for k in info if k.endswith("_declined")]
        assert all(l._ll_fused.pq is None and l._ll_fused.wq_bits == 8 for l in llm.model.layers)
        w1 = llm.model.layers[0].mlp.down_proj.weight
        assert not torch.equal(w1, w0) and torch.equal(w1, mx_round(w0, 8)[0].to(w1.dtype))
        layers, _ = _step_calls(llm, 2)
        assert layers[0] == _expected(2, True, True), layers[0]       # no *_wq entry
        for B in (1, 6):
            p, m = _prompts(B)
            dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
            eager = GraphedDecoder(llm, use_graph=False, fused_cache=True)
            assert torch.equal(dec.generate(p, m, max_new_tokens=8, **KW), eager.generate(p, m, max_new_tokens=8, **KW)), B
    finally:
        _restore(llm)
