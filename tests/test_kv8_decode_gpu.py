"""The fused decode on the MX8 KV cache (`GraphedDecoder(..., kv_cache="mxfp8")`) on `tiny-llama`, `tiny-qwen3` and `tiny-qwen3-moe`: every
layer stays fused and `ll_decode_attn_rope_kv8` is the only attention call of a decode step; the captured step gives the tokens of the eager
step at 1, 6 and 20 rows; the fused query-token forward agrees with the op-by-op one, which runs HF's attention on the dequantised staging pair;
one decode step agrees with HF f32 on an `mx_round` DynamicCache as well as HF's own bf16 on that cache does (E <= 1.5 Y); the cache takes
(D + D/32) / 2D of the bf16 cache's bytes; with the option off the launches are the ones they were.

E, Y, E / Y and the distance of the MX8 step from the bf16-cache step (the price of the format, not gated) are printed with -s.
Measured on an MI355X: tiny-llama E = 0.01651, Y = 0.01696 (E / Y = 0.974), distance 0.0352 = 2.07 Y; tiny-qwen3 E = 0.03544, Y = 0.03660 (0.968),
distance 0.0488 = 1.33 Y; query-token forward, fused against op-by-op: 0.0081 / 0.0136 / 0.0124 of max |h| (llama / qwen3 / qwen3-moe)."""
import copy
import warnings

import pytest
import torch

from llamole_amd import e2e
from llamole_amd.kv_cache import MX8StaticCache
from llamole_amd.llm_decode import GraphedDecoder
from llamole_amd.llm_quant import mx_round

pytestmark = pytest.mark.gpu

MARGIN = 1.5            # a bf16 engine against the reference's own bf16: the project's margin of record
KW = dict(do_sample=False, pad_token_id=0, eos_token_id=[])
MODELS = ("tiny-llama", "tiny-qwen3", "tiny-qwen3-moe")
DENSE = ("tiny-llama", "tiny-qwen3")


def _restore(llm):
    from llamole_amd.llm_accel import restore_decoder_layers, restore_elementwise, restore_linears, restore_model_decode
    restore_model_decode(llm)
    restore_decoder_layers(llm)
    restore_elementwise(llm)
    restore_linears(llm)


def _build(name):
    llm = e2e.build_llm(name, "cuda", torch.bfloat16)
    if name != "tiny-llama":
        e2e.randomize_head_norms(llm)
    if name == "tiny-qwen3-moe":
        g = torch.Generator().manual_seed(3)
        with torch.no_grad():                  # HF draws the router at std 0.02: logits that are all but equal; spread them
            for layer in llm.model.layers:
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


def _attention_calls(llm, B, **dec_kw):
    """the attention entry points the fused layers call during a two-token generate (the prefill runs HF's modules, then ONE decode step)"""
    states = [l._ll_fused for l in llm.model.layers]
    calls = []
    for st in states:
        st.lib = _Spy(st.lib, calls)
    try:
        p, m = _prompts(B)
        dec = GraphedDecoder(llm, use_graph=False, fused_cache=True, **dec_kw)
        dec.generate(p, m, max_new_tokens=2, **KW)
    finally:
        for st in states:
            st.lib = st.lib._lib
    return [c for c in calls if "attn" in c and "workspace" not in c], dec      # the workspace query is host code


@pytest.mark.parametrize("name", MODELS)
def test_every_layer_fused_and_kv8_is_the_only_attention_call(name):
    from llamole_amd.llm_accel import accelerate_llm
    llm = _build(name)
    try:
        info = accelerate_llm(llm)
        L = llm.config.num_hidden_layers
        assert info["decoder_layers_5_launches"] == L and info["decode_prologue_1_launch"] is True
        for B in (1, 6, 20):
            calls, dec = _attention_calls(llm, B, kv_cache="mxfp8")
            assert calls == ["ll_decode_attn_rope_kv8"] * L, (B, calls)
            cache = dec.cache
            assert isinstance(cache, MX8StaticCache) and cache.shared_counter and dec._cache_fused
            l0 = cache.layers[0]
            Bc, nkv, maxlen, D = l0.keys.shape
            assert l0.keys.dtype == torch.uint8 and l0.key_scales.shape == (Bc, nkv, maxlen, D // 32) and maxlen == 64
            # (D + D/32) / 2D of the bf16 cache's bytes, and no bf16 cache beside it: one staging pair for all layers
            assert cache.nbytes() * 2 * D == (D + D // 32) * (L * 2 * Bc * nkv * maxlen * D * 2)
            assert len(cache.staging) == 2 and all(t.shape == l0.keys.shape and t.dtype == torch.bfloat16 for t in cache.staging)
            assert int(l0.cumulative_length) == 13
            # every slot written so far holds codes, nothing behind them
            assert not bool(l0.keys[:, :, 13:].any()) and bool(l0.key_scales[:, :, :13].all())
        # the option off: the launches of a bf16 static cache, as they were
        want = "ll_decode_attn_rope_bf16" if name == "tiny-llama" else "ll_decode_attn_rope_qkn_bf16"
        for kw in ({}, {"kv_cache": None}):
            calls, dec = _attention_calls(llm, 1, **kw)
            assert calls == [want] * L and type(dec.cache).__name__ == "StaticCache" and dec.cache.layers[0].keys.dtype == torch.bfloat16
    finally:
        _restore(llm)


@pytest.mark.parametrize("name", MODELS)
def test_captured_step_equals_the_eager_step_and_query_forward_agrees(name, monkeypatch):
    from llamole_amd.llm_accel import _FusedLayer, accelerate_llm
    llm = _build(name)
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            accelerate_llm(llm)
            seen = []
            orig_sfx = _FusedLayer.run_suffix
            monkeypatch.setattr(_FusedLayer, "run_suffix", lambda self, *a, **k: (seen.append("suffix"), orig_sfx(self, *a, **k))[1])
            for B in (1, 6, 20):
                p, m = _prompts(B)
                dec = GraphedDecoder(llm, use_graph=True, fused_cache=True, kv_cache="mxfp8")
                eager = GraphedDecoder(llm, use_graph=False, fused_cache=True, kv_cache="mxfp8")
                got = dec.generate(p, m, max_new_tokens=8, **KW)
                assert dec._graph is not None, B
                assert torch.equal(got, eager.generate(p, m, max_new_tokens=8, **KW)), B
                skw = dict(max_new_tokens=8, do_sample=True, temperature=0.6, top_p=0.9, top_k=50, pad_token_id=0, eos_token_id=[])
                a = dec.generate(p, m, generator=torch.Generator(device="cuda").manual_seed(5), **skw)
                b = eager.generate(p, m, generator=torch.Generator(device="cuda").manual_seed(5), **skw)
                assert torch.equal(a, b), B
            # the query-token forward (9 positions): the fused path (ll_suffix_attn_rope_kv8) against the op-by-op path on the same cache
            # (LLAMOLE_FUSED_SUFFIX=0: HF's modules, cache.update stores quantised and hands back the dequantised staging pair)
            g = torch.Generator().manual_seed(9)
            p1 = torch.randint(5, 2000, (1, 20), generator=g).cuda()
            tail = torch.randint(5, 2000, (1, 9), generator=g).cuda()
            hid, codes = {}, {}
            for mode in ("0", "1"):
                monkeypatch.setenv("LLAMOLE_FUSED_SUFFIX", mode)
                dec = GraphedDecoder(llm, use_graph=True, fused_cache=True, kv_cache="mxfp8")
                dec.generate(p1, torch.ones_like(p1), max_new_tokens=16, **KW)
                seen.clear()
                hid[mode] = dec.continue_hidden(tail, 20 + 16 - 9).float().clone()
                assert ("suffix" in seen) == (mode == "1")
                assert int(dec.cache.layers[0].cumulative_length) == 36
                codes[mode] = dec.cache.layers[0].keys[:, :, :36].clone()
            err = float((hid["0"] - hid["1"]).abs().max() / hid["0"].abs().max())
            print(f"\n{name}: query-token forward on the MX8 cache, fused against op-by-op: max |diff| / max |h| = {err:.5f}")
            assert err <= 3e-2
            assert torch.equal(codes["0"][:, :, :27], codes["1"][:, :, :27])       # the same prompt pass and decode steps in front of the tail
        assert not rec, [str(w.message) for w in rec]
    finally:
        _restore(llm)


def _mx_dynamic_cache(config):
    from transformers import DynamicCache

    class MXDynamicCache(DynamicCache):
        """HF's own growing cache holding mx_round of every new row"""

        def update(self, key_states, value_states, layer_idx, *a, **k):
            D = key_states.shape[-1]
            kq = mx_round(key_states.reshape(-1, D), 8)[0].view(key_states.shape).to(key_states.dtype)
            vq = mx_round(value_states.reshape(-1, D), 8)[0].view(value_states.shape).to(value_states.dtype)
            return super().update(kq, vq, layer_idx, *a, **k)

    return MXDynamicCache(config=config)


def _hf_logits_on_mx_cache(model, ids):
    mask = torch.ones_like(ids)
    pos = torch.arange(ids.shape[1], device=ids.device)[None]
    with torch.no_grad():
        return model(input_ids=ids, attention_mask=mask, position_ids=pos, past_key_values=_mx_dynamic_cache(model.config),
                     use_cache=True).logits[:, -1, :].float()


def _step_logits(llm, prompt, **dec_kw):
    dec = GraphedDecoder(llm, use_graph=False, fused_cache=True, **dec_kw)
    toks = dec.generate(prompt, torch.ones_like(prompt), max_new_tokens=2, **KW)
    return toks, dec.last_logits.float().clone()


@pytest.mark.parametrize("name", DENSE)
def test_one_decode_step_against_hf_on_an_mx_rounding_cache(name):
    """1 row of 13 tokens, greedy, max_new_tokens = 2: last_logits are those of one fused decode step on the MX8 cache.  Reference: the
    untouched HF model in f32 on a DynamicCache that applies mx_round to every new K / V row; Y = max |HF bf16 on that cache - reference|;
    E = max |fused - reference| <= 1.5 Y.  The distance of the step from the bf16-cache fused step is printed in units of Y, not gated."""
    from llamole_amd.llm_accel import accelerate_llm
    llm = _build(name)
    hf16, hf32 = copy.deepcopy(llm), copy.deepcopy(llm).float()
    prompt = torch.randint(5, 2000, (1, 13), generator=torch.Generator().manual_seed(13)).cuda()
    try:
        info = accelerate_llm(llm)
        assert info["decoder_layers_5_launches"] == 2 and info["decode_prologue_1_launch"]
        toks, fused = _step_logits(llm, prompt, kv_cache="mxfp8")
        ids = toks[:, :14]
        ref = _hf_logits_on_mx_cache(hf32, ids)
        Y = float((_hf_logits_on_mx_cache(hf16, ids) - ref).abs().max())
        E = float((fused - ref).abs().max())
        toks_bf, fused_bf = _step_logits(llm, prompt)
        price = float((fused - fused_bf).abs().max()) if torch.equal(toks_bf[:, :14], ids) else float("nan")
        print(f"\n{name}: one decode step on the MX8 cache, max |logit error| against HF f32 on the mx_round cache: fused E = {E:.5f}, "
              f"HF bf16 Y = {Y:.5f}, E / Y = {E / Y:.3f}; distance from the bf16-cache fused step = {price:.5f} = {price / Y:.2f} Y")
        assert Y > 0 and E <= MARGIN * Y, (E, Y)
    finally:
        _restore(llm)
