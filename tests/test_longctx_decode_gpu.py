"""The fused decode on static caches beyond the 16384 slots of the one-workgroup attention kernels (`tiny-llama`, and `tiny-qwen3` for the
per-head norms): `generate` returns -- before the key-split entries it raised out of the attention call -- with the layers fused and
ll_decode_attn_rope_split_bf16 the entry that is called (the old one at a 512-slot cache), the captured step gives the tokens of the eager fused
step, one decode step at a position beyond 16384 agrees with the untouched HF model as well as HF's own bf16 does, the fused query-token forward
agrees with the op-by-op one on the same cache, the op-by-op stack (layers=False) runs there too, and a cache beyond 131072 slots decodes on
HF's layers instead of raising.

E and Y of the step test and the query-token difference are printed with -s."""
import copy
import gc
import warnings

import pytest
import torch

from llamole_amd import e2e
from llamole_amd.llm_decode import GraphedDecoder

pytestmark = pytest.mark.gpu

MARGIN = 1.5            # a bf16 engine against the reference's own bf16: the project's margin of record
KW = dict(do_sample=False, pad_token_id=0, eos_token_id=[])
P_LONG = 16400          # prompt tokens: with max_new_tokens <= 48 the static cache has 16448 slots, every decode position lies beyond 16384
PAD = 600               # left padding of the second row: longer than one 512-key range
MODELS = ["tiny-llama", "tiny-qwen3"]
SPLIT, OLD = "ll_decode_attn_rope_split_bf16", {"tiny-llama": "ll_decode_attn_rope_bf16", "tiny-qwen3": "ll_decode_attn_rope_qkn_bf16"}


@pytest.fixture(autouse=True)
def _release_device_memory():
    """these tests hold caches of up to 131080 slots and HF's f32 forward over 16401 tokens in torch's allocator, which keeps freed blocks: hand
    them back after every test, so that the engines of later tests, which allocate from the device directly, find the memory"""
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _restore(llm):
    from llamole_amd.llm_accel import restore_decoder_layers, restore_elementwise, restore_linears, restore_model_decode
    restore_model_decode(llm)
    restore_decoder_layers(llm)
    restore_elementwise(llm)
    restore_linears(llm)


def _build(name):
    llm = e2e.build_llm(name, "cuda", torch.bfloat16, seed=0)
    if name == "tiny-qwen3":
        e2e.randomize_head_norms(llm)
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


def _prompts(B, P=P_LONG, seed=21):
    g = torch.Generator().manual_seed(seed + B)
    p = torch.randint(5, 2000, (B, P), generator=g).cuda()
    m = torch.ones_like(p)
    if B > 1:
        m[1, :min(PAD, P // 2)] = 0           # left padding
    return p, m


@pytest.mark.parametrize("name", MODELS)
def test_generate_on_a_long_cache_is_fused_and_captured(name):
    from llamole_amd.llm_accel import ATTN_SPLIT_MAXLEN, accelerate_llm
    llm = _build(name)
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            info = accelerate_llm(llm)
            assert info["decoder_layers_5_launches"] == 2 and info["decode_prologue_1_launch"] is True
            assert info["long_cache_attention_max_slots"] == ATTN_SPLIT_MAXLEN == 131072
            st = llm.model.layers[1]._ll_fused
            for B in (1, 2):
                # which attention entry a decode step calls: the key-split one on 16448 slots, the one-workgroup one on 512
                for P, want in ((P_LONG, SPLIT), (500, OLD[name])):
                    calls = []
                    st.lib = _Spy(st.lib, calls)
                    p, m = _prompts(B, P)
                    dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
                    dec.generate(p, m, max_new_tokens=2, **KW)         # prefill (HF modules) + ONE decode step
                    st.lib = st.lib._lib
                    assert dec.cache.layers[0].keys.shape[2] == (16448 if P == P_LONG else 512)
                    assert llm.model._ll_decode["served"] is True and llm.model._ll_decode["declined"] is None
                    assert [c for c in calls if "attn" in c and "workspace" not in c] == [want], (B, P, calls)
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
            # one workspace per model and shape, not per layer or call
            ws = {id(v) for l in llm.model.layers for v in l._ll_fused._split_ws.values()}
            assert len(ws) == 2 and llm.model.layers[0]._ll_fused._split_ws is llm.model.layers[1]._ll_fused._split_ws
        # no shape was turned eager, no capture failed
        assert not [w for w in rec if "hipGraph" in str(w.message) or "eager" in str(w.message)], [str(w.message) for w in rec]
    finally:
        _restore(llm)


@pytest.mark.parametrize("name", MODELS)
def test_one_fused_decode_step_beyond_16384_against_hf(name):
    """2 rows of 16400 tokens (the second left-padded by 600), greedy, max_new_tokens = 2: last_logits are those of one fused decode step at cache
    slot 16400.  E = max |fused - HF f32|, Y = max |HF bf16 - HF f32| on the same 16401 tokens, E <= 1.5 Y."""
    from llamole_amd.llm_accel import accelerate_llm
    llm = _build(name)
    hf16, hf32 = copy.deepcopy(llm), copy.deepcopy(llm).float()
    try:
        accelerate_llm(llm)
        p, m = _prompts(2)
        dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
        toks = dec.generate(p, m, max_new_tokens=2, **KW)
        assert llm.model._ll_decode["served"] is True
        fused = dec.last_logits.float().clone()
        ids = toks[:, :P_LONG + 1]
        full = torch.cat([m, torch.ones_like(m[:, :1])], dim=1)
        pos = (full.long().cumsum(dim=1) - 1).clamp_min(0)
        with torch.no_grad():
            ref = hf32(input_ids=ids, attention_mask=full, position_ids=pos, use_cache=False, logits_to_keep=1).logits[:, -1, :].float()
            l16 = hf16(input_ids=ids, attention_mask=full, position_ids=pos, use_cache=False, logits_to_keep=1).logits[:, -1, :].float()
        Y = float((l16 - ref).abs().max())
        E = float((fused - ref).abs().max())
        print(f"\n{name}: one decode step at slot {P_LONG}, max |logit error| against HF f32: fused E = {E:.5f}, HF bf16 Y = {Y:.5f}, E / Y = {E / Y:.3f}")
        assert Y > 0 and E <= MARGIN * Y, (E, Y)
    finally:
        _restore(llm)


@pytest.mark.parametrize("name", MODELS)
def test_query_token_forward_on_a_long_cache(name, monkeypatch):
    """9 new positions on top of a 16448-slot cache: the fused path (ll_suffix_attn_rope_split_bf16) against the op-by-op path, whose attention
    declines to HF's own beyond 16384 slots, at the tolerance tests/test_llm_decode.py holds the dense layouts to"""
    from llamole_amd.llm_accel import _FusedLayer, accelerate_llm
    llm = _build(name)
    try:
        accelerate_llm(llm)
        seen = []
        orig = _FusedLayer.run_suffix
        _FusedLayer.run_suffix = lambda self, *a, **k: (seen.append("suffix"), orig(self, *a, **k))[1]
        try:
            p, m = _prompts(1)
            tail = torch.randint(5, 2000, (1, 9), generator=torch.Generator().manual_seed(9)).cuda()
            hid = {}
            for mode in ("0", "1"):
                monkeypatch.setenv("LLAMOLE_FUSED_SUFFIX", mode)
                dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
                dec.generate(p, m, max_new_tokens=16, **KW)
                seen.clear()
                calls = []
                st = llm.model.layers[1]._ll_fused
                st.lib = _Spy(st.lib, calls)
                hid[mode] = dec.continue_hidden(tail, P_LONG + 16 - 9).float().clone()
                st.lib = st.lib._lib
                assert ("suffix" in seen) == (mode == "1")
                assert ("ll_suffix_attn_rope_split_bf16" in calls) == (mode == "1")
            err = float((hid["0"] - hid["1"]).abs().max() / hid["0"].abs().max())
            print(f"\n{name}: query-token forward on 16448 slots, fused against op-by-op: max |diff| / max |h| = {err:.5f}")
            assert err <= 3e-2
        finally:
            _FusedLayer.run_suffix = orig
    finally:
        _restore(llm)


def test_op_by_op_stack_runs_beyond_16384_slots():
    """accelerate_llm(layers=False): the registered decode attention declines to HF's sdpa where ll_decode_attn_bf16 would refuse the cache"""
    from llamole_amd.llm_accel import accelerate_llm
    llm = _build("tiny-llama")
    try:
        info = accelerate_llm(llm, layers=False)
        assert info["decode_attention"] and "decoder_layers_5_launches" not in info
        p, m = _prompts(2)
        dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
        out = dec.generate(p, m, max_new_tokens=3, **KW)
        assert out.shape == (2, P_LONG + 3) and dec.cache.layers[0].keys.shape[2] == 16448
    finally:
        _restore(llm)


def test_a_cache_beyond_131072_slots_decodes_on_hf_layers():
    """131080 slots (a short prompt in a long bucket): no exception, the call is reported as declined by the decoder layers"""
    from llamole_amd.llm_accel import accelerate_llm
    llm = _build("tiny-llama")
    try:
        accelerate_llm(llm)
        p, m = _prompts(2, P=12)
        dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
        dec.len_bucket = 131072 + 8
        out = dec.generate(p, m, max_new_tokens=3, **KW)
        assert out.shape == (2, 15) and dec.cache.layers[0].keys.shape[2] == 131080
        st = llm.model._ll_decode
        assert st["served"] is False and "decoder_layers" in st["declined"] and "131080" in st["declined"]
        # the same prompt in a 64-slot cache runs fused again, and says so
        short = GraphedDecoder(llm, use_graph=False, fused_cache=True)
        short.generate(p, m, max_new_tokens=3, **KW)
        assert st["served"] is True and st["declined"] is None
    finally:
        _restore(llm)
