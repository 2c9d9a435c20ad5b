"""Sliding-window models on the graphed decode, without a GPU: what is eligible for the fused path, the full-length static cache that stands in
for transformers' sliding cache layer, and token / hidden-state parity of ``GraphedDecoder`` with HF's own ``generate`` (dynamic cache) well
past the window -- the static cache keeps slot j = position j and leaves the window to HF's sliding mask over (max_len, 0)."""
import pytest
import torch
from transformers.cache_utils import StaticCache, StaticLayer

from llamole_amd import e2e
from llamole_amd.kv_cache import FullLengthStaticCache, MX8StaticCache, cache_layer_types, static_cache_for
from llamole_amd.llm_accel import attn_window, decoder_layer_declined, model_decode_declined
from llamole_amd.llm_decode import GraphedDecoder

SW_MODELS = ["tiny-mistral-sw", "tiny-qwen2-sw"]


def test_the_config_entries():
    big = e2e.LLM_CONFIGS["mistral-7b-v0.1"]
    assert (big["cls"], big["hidden_size"], big["num_hidden_layers"], big["num_attention_heads"], big["num_key_value_heads"],
            big["intermediate_size"], big["vocab_size"], big["sliding_window"]) == ("Mistral", 4096, 32, 32, 8, 14336, 32000, 4096)
    assert e2e.LLM_CONFIGS["mistral-7b"]["sliding_window"] is None and e2e.LLM_CONFIGS["tiny-mistral"]["sliding_window"] is None
    m = e2e.build_llm("tiny-mistral-sw", "cpu", torch.bfloat16)
    assert [attn_window(l.self_attn) for l in m.model.layers] == [24, 24] and cache_layer_types(m.config) == ["sliding_attention"] * 2
    q = e2e.build_llm("tiny-qwen2-sw", "cpu", torch.bfloat16)
    assert [attn_window(l.self_attn) for l in q.model.layers] == [None, 24]
    assert cache_layer_types(q.config) == ["full_attention", "sliding_attention"] and q.model.has_sliding_layers


def _pretend_fused(llm, D):
    """what model_decode_declined reads off an installed layer"""
    for l in llm.model.layers:
        l._ll_fused = type("F", (), {"D": D})()


@pytest.mark.parametrize("name", SW_MODELS)
def test_sliding_window_layers_are_eligible(name):
    llm = e2e.build_llm(name, "cpu", torch.bfloat16)
    for layer in llm.model.layers:
        assert decoder_layer_declined(layer) == "weights are not on the device"      # nothing structural: on the device it is fused
    # the model decode: with every layer fused, a CPU model is declined for where its inv_freq lives, no longer for its sliding layers
    _pretend_fused(llm, llm.model.layers[0].self_attn.head_dim)
    assert model_decode_declined(llm) == "inv_freq is not an f32 device tensor"


def test_what_is_still_declined():
    llm = e2e.build_llm("tiny-mistral-sw", "cpu", torch.bfloat16)
    layer = llm.model.layers[0]
    for bad in (0, -4, 24.0, True, "24"):
        layer.self_attn.sliding_window = bad
        assert decoder_layer_declined(layer) == f"sliding_window={bad!r} is not a positive int"
    layer.self_attn.sliding_window = 24
    assert decoder_layer_declined(layer) == "weights are not on the device"
    # a window on the module that its config does not state: HF's masks (prompt pass, op-by-op decode) come from the config, the windowed
    # kernels would read the module -- two models; declined for its structure, on a sliding model, a mixed one and one without a window
    layer.self_attn.sliding_window = 16
    assert decoder_layer_declined(layer) == "sliding-window layer"
    layer.self_attn.sliding_window = 24
    mixed = e2e.build_llm("tiny-qwen2-sw", "cpu", torch.bfloat16).model.layers
    mixed[0].self_attn.sliding_window = 24                         # layer_types names layer 0 "full_attention"
    mixed[1].self_attn.sliding_window = None                       # ... and layer 1 "sliding_attention"
    assert [decoder_layer_declined(l) for l in mixed] == ["sliding-window layer"] * 2
    plain = e2e.build_llm("tiny-llama", "cpu", torch.bfloat16).model.layers[0]
    plain.self_attn.sliding_window = 24
    assert decoder_layer_declined(plain) == "sliding-window layer"
    # a rotary module with one rope type per layer type (Gemma-3 style)
    _pretend_fused(llm, 128)
    llm.model.rotary_emb.rope_type = {"full_attention": "default", "sliding_attention": "default"}
    assert model_decode_declined(llm) == "rope_type per layer type"


@pytest.mark.parametrize("name", SW_MODELS)
def test_the_static_cache_of_a_sliding_config_is_full_length_layers_only(name):
    cfg = e2e.build_llm(name, "cpu", torch.float32).config
    hf = StaticCache(config=cfg, max_cache_len=100)
    assert any(type(l) is not StaticLayer for l in hf.layers)      # what transformers would build: a sliding layer with a host-side counter
    cache = static_cache_for(cfg, 100)
    assert isinstance(cache, FullLengthStaticCache) and len(cache.layers) == cfg.num_hidden_layers
    assert all(type(l) is StaticLayer and l.max_cache_len == 100 for l in cache.layers)
    assert all(cache.get_mask_sizes(1, i) == (100, 0) for i in range(len(cache.layers)))
    assert not any(cache.is_sliding)
    # a config without sliding layers keeps transformers' own cache
    plain = static_cache_for(e2e.build_llm("tiny-mistral", "cpu", torch.float32).config, 100)
    assert type(plain) is StaticCache and all(type(l) is StaticLayer for l in plain.layers)
    # the MX8 cache has no windowed kernels: refused, with both options named
    with pytest.raises(ValueError, match="mxfp8.*sliding_window=24"):
        MX8StaticCache(cfg, 1, 100, "cpu", torch.float32)
    with pytest.raises(ValueError, match="mxfp8.*sliding_window=24"):
        GraphedDecoder(e2e.build_llm(name, "cpu", torch.float32), use_graph=False, kv_cache="mxfp8")._prepare(1, 100, "cpu", False)


def _prompt():
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(5, 1000, (2, 12), generator=g)
    mask = torch.ones_like(prompt)
    mask[1, :4] = 0                                                # left padding
    return prompt, mask


@pytest.mark.parametrize("name,over", [("tiny-mistral-sw", dict(sliding_window=8)), ("tiny-qwen2-sw", {})])
def test_generate_and_query_forward_equal_hf_past_the_window(name, over):
    """greedy decode of 40 tokens behind a 12-token prompt (window 8 / 24): token-identical to HF generate on its dynamic cache; then the
    query-token forward on the decode's cache against HF's forward of the whole sequence"""
    llm = e2e.build_llm(name, "cpu", torch.float32, **over)
    window = llm.config.sliding_window
    prompt, mask = _prompt()
    kw = dict(max_new_tokens=40, do_sample=False, pad_token_id=0, eos_token_id=[])
    assert prompt.shape[1] + kw["max_new_tokens"] > 2 * window
    ref = llm.generate(inputs=prompt, attention_mask=mask, **kw)
    dec = GraphedDecoder(llm, use_graph=False)
    got = dec.generate(prompt, mask, **kw)
    assert torch.equal(ref, got)
    assert isinstance(dec.cache, FullLengthStaticCache) and all(type(l) is StaticLayer for l in dec.cache.layers)
    # a second call on the prepared cache (reset, same shape)
    assert torch.equal(dec.generate(prompt, mask, **kw), ref)
    # the query-token forward: 5 new tokens behind the first 30 generated ones, against HF's forward of the full sequence
    P, keep, S = prompt.shape[1], 30, 5
    g = torch.Generator().manual_seed(3)
    tail = torch.randint(5, 1000, (2, S), generator=g)
    hidden = dec.continue_hidden(tail, P + keep)
    full = torch.cat([ref[:, :P + keep], tail], dim=1)
    fmask = torch.cat([mask, torch.ones(2, keep + S, dtype=mask.dtype)], dim=1)
    posid = (fmask.cumsum(1) - 1).clamp(min=0)                     # positions count real tokens, as generate's do
    want = llm.model(input_ids=full, attention_mask=fmask, position_ids=posid).last_hidden_state[:, -S:]
    torch.testing.assert_close(hidden, want, rtol=1e-4, atol=1e-5)
