"""The fused decode on sliding-window models: `tiny-mistral-sw` (every layer, window 24) and `tiny-qwen2-sw` (layer 0 full, layer 1 sliding).
The whole stack installs (before the windowed attention entries a sliding layer was declined, and a Mistral layer -- whose module keeps no
``sliding_window`` attribute -- was fused as a full-attention layer), the sliding layers call ll_decode_attn_rope_win_bf16 /
ll_suffix_attn_rope_win_bf16 wherever the window can bind and exactly a Llama's entries where it cannot, one decode step beyond the window
agrees with the untouched HF model as well as HF's own bf16 does (also on a 16448-slot cache), the captured step decodes the tokens of the
op-by-op stack, beams and prompt lookup run, and an MX8 cache is refused.

E and Y of the step test are printed with -s.  Measured on an MI355X: tiny-mistral-sw E / Y = 1.05 at slot 40 and 0.89 at slot 16400,
tiny-qwen2-sw 1.12 and 0.94 (bound 1.5)."""
import copy
import gc
import warnings

import pytest
import torch

from llamole_amd import e2e
from llamole_amd.llm_decode import GraphedDecoder
from tests.test_kv8_decode_gpu import _Spy
from tests.test_longctx_decode_gpu import KW, MARGIN, P_LONG, _restore

pytestmark = pytest.mark.gpu

MODELS = ["tiny-mistral-sw", "tiny-qwen2-sw"]
WINDOWS = {"tiny-mistral-sw": [24, 24], "tiny-qwen2-sw": [None, 24]}
WIN, SUFFIX_WIN = "ll_decode_attn_rope_win_bf16", "ll_suffix_attn_rope_win_bf16"
TIE = 0.02              # the near-tie rule of tests/test_full_size_gpu.py: a token may differ where the top-2 margin is below 2 % of max |logit|


@pytest.fixture(autouse=True)
def _release_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _build(name, **over):
    return e2e.build_llm(name, "cuda", torch.bfloat16, seed=0, **over)


def _prompts(B, P=40, seed=21):
    g = torch.Generator().manual_seed(seed + B)
    p = torch.randint(5, 2000, (B, P), generator=g).cuda()
    m = torch.ones_like(p)
    if B > 1:
        m[1, :min(30, P - 8)] = 0             # left padding longer than the window
    if B > 2:
        m[2, :5] = 0
    return p, m


def _attention_calls(llm, p, m, new=2, tail=None):
    """the attention entry points the fused layers call, per layer: a prefill (HF modules), ``new - 1`` decode steps, then optionally the
    query-token forward of ``tail``"""
    states = [l._ll_fused for l in llm.model.layers]
    calls = [[] for _ in states]
    for st, c in zip(states, calls):
        st.lib = _Spy(st.lib, c)
    try:
        dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
        dec.generate(p, m, max_new_tokens=new, **KW)
        if tail is not None:
            dec.continue_hidden(tail, p.shape[1] + new - tail.shape[1])
    finally:
        for st in states:
            st.lib = st.lib._lib
    return [[c for c in cs if "attn" in c and "workspace" not in c] for cs in calls], dec


@pytest.mark.parametrize("name", MODELS)
def test_the_stack_installs_and_sliding_layers_call_the_windowed_entries(name):
    from llamole_amd.llm_accel import accelerate_llm
    llm = _build(name)
    try:
        info = accelerate_llm(llm)
        assert info["decoder_layers_5_launches"] == llm.config.num_hidden_layers == 2 and info["decode_prologue_1_launch"] is True
        assert not [k for k in info if k.endswith("_declined")], info
        assert [l._ll_fused.window for l in llm.model.layers] == WINDOWS[name]
        assert info["sliding_window_layers_fused"] == sum(w is not None for w in WINDOWS[name])
        p, m = _prompts(3)
        tail = torch.randint(5, 2000, (3, 4), generator=torch.Generator().manual_seed(9)).cuda()
        calls, dec = _attention_calls(llm, p, m, new=6, tail=tail)
        assert llm.model._ll_decode["served"] is True and llm.model._ll_decode["declined"] is None
        assert type(dec.cache).__name__ == "FullLengthStaticCache" and dec.cache.layers[0].keys.shape[2] == 64
        for w, cs in zip(WINDOWS[name], calls):                    # 5 decode steps, then 3 x 4 query-token rows
            assert cs == ([WIN] * 5 + [SUFFIX_WIN] if w else ["ll_decode_attn_rope_bf16"] * 5 + ["ll_suffix_attn_rope_bf16"]), (w, cs)
        with pytest.raises(ValueError, match="mxfp8"):
            GraphedDecoder(llm, use_graph=False, fused_cache=True, kv_cache="mxfp8").generate(p, m, max_new_tokens=2, **KW)
    finally:
        _restore(llm)


def test_launch_listing_of_full_attention_and_of_a_window_that_cannot_bind():
    """a `tiny-llama` step lists the entries it always listed; `tiny-mistral-sw` with a window of 512 on a 64-slot cache lists the same, and the
    windowed entry once the cache (576 slots) is longer than the window"""
    from llamole_amd.llm_accel import accelerate_llm
    listed = {}
    for name, over, P in (("tiny-llama", {}, 40), ("tiny-mistral-sw", dict(sliding_window=512), 40), ("tiny-mistral-sw", dict(sliding_window=512), 530)):
        llm = _build(name, **over)
        try:
            assert accelerate_llm(llm)["decode_prologue_1_launch"] is True
            p, m = _prompts(2, P)
            tail = torch.randint(5, 2000, (2, 4), generator=torch.Generator().manual_seed(9)).cuda()
            calls, dec = _attention_calls(llm, p, m, new=5, tail=tail)
            listed[(name, P)] = (calls, dec.cache.layers[0].keys.shape[2])
        finally:
            _restore(llm)
    old = [["ll_decode_attn_rope_bf16"] * 4 + ["ll_suffix_attn_rope_bf16"]] * 2
    assert listed[("tiny-llama", 40)] == (old, 64)
    assert listed[("tiny-mistral-sw", 40)] == (old, 64)
    assert listed[("tiny-mistral-sw", 530)] == ([[WIN] * 4 + [SUFFIX_WIN]] * 2, 576)


def _hf_logits(model, ids, mask):
    pos = (mask.long().cumsum(dim=1) - 1).clamp_min(0)
    with torch.no_grad():
        return model(input_ids=ids, attention_mask=mask, position_ids=pos, use_cache=False, logits_to_keep=1).logits[:, -1, :].float()


@pytest.mark.parametrize("P", [40, P_LONG])
@pytest.mark.parametrize("name", MODELS)
def test_one_fused_decode_step_beyond_the_window_against_hf(name, P):
    """2 rows of P tokens (the second left-padded), greedy, max_new_tokens = 2: last_logits are those of one fused decode step at cache slot P,
    beyond the window of 24, on a cache of 64 / 16448 slots.  E = max |fused - HF f32|, Y = max |HF bf16 - HF f32| on the same P + 1 tokens
    (HF's own sliding mask, no cache), E <= 1.5 Y."""
    from llamole_amd.llm_accel import accelerate_llm
    llm = _build(name)
    hf16, hf32 = copy.deepcopy(llm), copy.deepcopy(llm).float()
    try:
        accelerate_llm(llm)
        p, m = _prompts(2, P)
        dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
        toks = dec.generate(p, m, max_new_tokens=2, **KW)
        assert llm.model._ll_decode["served"] is True and dec.cache.layers[0].keys.shape[2] == (64 if P == 40 else 16448)
        fused = dec.last_logits.float().clone()
        ids = toks[:, :P + 1]
        full = torch.cat([m, torch.ones_like(m[:, :1])], dim=1)
        ref = _hf_logits(hf32, ids, full)
        Y = float((_hf_logits(hf16, ids, full) - ref).abs().max())
        E = float((fused - ref).abs().max())
        print(f"\n{name}: one decode step at slot {P}, max |logit error| against HF f32: fused E = {E:.5f}, HF bf16 Y = {Y:.5f}, E / Y = {E / Y:.3f}")
        assert Y > 0 and E <= MARGIN * Y, (E, Y)
    finally:
        _restore(llm)


def _same_or_near_tie(hf16, got, want, m, P):
    """token-equal; where a row differs, its first differing token must be a near-tie of the untouched model's logits over the tokens before it
    (TIE of max |logit|), and nothing behind that token is compared in that row"""
    for b in range(got.shape[0]):
        diff = (got[b] != want[b]).nonzero().flatten()
        if diff.numel() == 0:
            continue
        t = int(diff[0])
        assert t >= P
        mask = torch.cat([m[b:b + 1], torch.ones(1, t - P, dtype=m.dtype, device=m.device)], dim=1)
        logits = _hf_logits(hf16, want[b:b + 1, :t], mask)[0]
        for tok in (int(got[b, t]), int(want[b, t])):
            assert float(logits[tok]) >= float(logits.max()) - TIE * float(logits.abs().max()), (b, t, tok)


@pytest.mark.parametrize("name", MODELS)
def test_captured_generate_decodes_the_tokens_of_the_op_by_op_stack(name):
    """greedy, 24 new tokens behind 40 (64 slots, window 24), at batch 1, batch 3 left-padded and 17 rows (the seven-launch layers)"""
    from llamole_amd.llm_accel import accelerate_llm
    llm, plain = _build(name), _build(name)
    hf16 = copy.deepcopy(llm)
    try:
        assert accelerate_llm(llm)["decode_prologue_1_launch"] is True
        info = accelerate_llm(plain, layers=False)
        assert info["decode_attention"] and "decoder_layers_5_launches" not in info
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            for B in (1, 3, 17):
                p, m = _prompts(B)
                dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
                got = dec.generate(p, m, max_new_tokens=24, **KW)
                assert dec._graph is not None and dec._served_by_fused_prologue(), B
                assert torch.equal(got, dec.generate(p, m, max_new_tokens=24, **KW)), B                     # replayed
                assert torch.equal(got, GraphedDecoder(llm, use_graph=False, fused_cache=True).generate(p, m, max_new_tokens=24, **KW)), B
                ref = GraphedDecoder(plain, use_graph=False, fused_cache=True)
                want = ref.generate(p, m, max_new_tokens=24, **KW)
                assert type(ref.cache).__name__ == "FullLengthStaticCache" and not plain.model.__dict__.get("_ll_decode")
                _same_or_near_tie(hf16, got, want, m, p.shape[1])
        assert not [w for w in rec if "hipGraph" in str(w.message) or "eager" in str(w.message)], [str(w.message) for w in rec]
    finally:
        _restore(llm)
        _restore(plain)


@pytest.mark.parametrize("name", MODELS)
def test_beams_and_prompt_lookup(name, monkeypatch):
    """num_beams = 2: graphed, eager and the torch beam step give the same tokens; prompt_lookup_num_tokens = 4: the checks of
    tests/test_prompt_lookup_gpu.py (graphed, eager and torch sampler token-equal, the accepted counts those of the torch replay)"""
    from llamole_amd.llm_accel import accelerate_llm
    from tests.test_prompt_lookup_gpu import _run_e2e
    llm = _build(name)
    try:
        assert accelerate_llm(llm)["decode_prologue_1_launch"] is True
        p, m = _prompts(2)
        kw = dict(do_sample=False, num_beams=2, max_new_tokens=20, pad_token_id=0, eos_token_id=[2047, 7, 11])
        g = GraphedDecoder(llm, use_graph=True, fused_cache=True)
        a = g.generate(p, m, **kw)
        assert g._beam_graph is not None and g._served_by_fused_prologue()
        b = GraphedDecoder(llm, use_graph=False, fused_cache=True).generate(p, m, **kw)
        c = GraphedDecoder(llm, use_graph=True, fused_cache=True, sampler="torch").generate(p, m, **kw)
        assert torch.equal(a, b) and torch.equal(a, c), (a, b, c)
        _run_e2e(llm, monkeypatch, ks=(4,))
    finally:
        _restore(llm)
