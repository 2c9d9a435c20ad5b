"""The MX8 KV cache without a GPU: `kv_cache.MX8StaticCache` on a CPU model runs on `llm_quant.mx_round` in torch, so the host logic -- the
storage format, the position counters, the staging pair, the decoder option and its refusals -- is checked here; the kernels are checked in
tests/test_kv8_kernels_gpu.py and the fused decode in tests/test_kv8_decode_gpu.py."""
import types

import pytest
import torch

from llamole_amd import e2e
from llamole_amd.kv_cache import MX8StaticCache, check_kv_cache, mx8_cache_bytes, mx8_dequantize, mx8_quantize_rows
from llamole_amd.llm_decode import GraphedDecoder
from llamole_amd.llm_quant import decode_codes, encode_codes8, mx_round

KW = dict(do_sample=False, pad_token_id=0, eos_token_id=[])


def _rows(seed=0, n=24, D=64):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, D, generator=g)
    x[0] = 0                                   # an all-zero row
    x[1, :32] = 0                              # an all-zero block beside a live one
    x[2] *= 400                                # Qwen2's K range
    x[3] *= 1e-30
    x[4, 5] = -0.0
    x[5, :32] = torch.linspace(-448, 448, 32)  # a block whose maximum is the largest E4M3 value
    return x


def test_codes_round_trip_to_mx_round_and_are_exactly_bf16():
    x = _rows()
    dq, sb = mx_round(x, 8)
    codes = encode_codes8(dq, sb)
    assert codes.dtype == torch.uint8 and codes.shape == x.shape and sb.shape == (x.shape[0], 2)
    back = mx8_dequantize(codes, sb)
    assert torch.equal(back.view(torch.int32), dq.view(torch.int32))            # bit for bit, the sign of a zero included
    assert torch.equal(back.to(torch.bfloat16).float(), back)                    # every dequantised value is a bf16 number
    assert not ((codes & 0x7f) == 0x7f).any()                                    # the quantiser never emits a NaN code
    # every code byte means what decode_codes says
    allc = torch.arange(256, dtype=torch.uint8).view(8, 32)
    one = torch.full((8, 1), 127, dtype=torch.uint8)
    vals = decode_codes(allc, 8)
    ok = ~torch.isnan(vals)
    assert int((~ok).sum()) == 2
    assert torch.equal(encode_codes8(torch.where(ok, vals, 0.0), one)[ok], allc[ok])
    c2, s2 = mx8_quantize_rows(x.view(2, 3, 4, 64))
    assert torch.equal(c2.view(-1, 64), codes) and torch.equal(s2.view(-1, 2), sb)


def test_cache_class_stores_mx_round_and_returns_the_staging_pair():
    llm = e2e.build_llm("tiny", "cpu", torch.float32)
    cfg = llm.config
    B, L, nkv, D = 2, 40, cfg.num_key_value_heads, cfg.hidden_size // cfg.num_attention_heads
    cache = MX8StaticCache(cfg, B, L, "cpu", torch.float32)
    assert len(cache.layers) == cfg.num_hidden_layers and not cache.shared_counter
    l0 = cache.layers[0]
    assert l0.keys.dtype == torch.uint8 and l0.keys.shape == (B, nkv, L, D) and l0.key_scales.shape == (B, nkv, L, D // 32)
    assert l0._ll_fused_update and l0.is_initialized and l0.keys.shape[2] == L
    assert cache.nbytes() == mx8_cache_bytes(B, nkv, L, D, cfg.num_hidden_layers)
    assert cache.nbytes() * 2 * D == (D + D // 32) * (cfg.num_hidden_layers * 2 * B * nkv * L * D * 2)      # (D + D/32) / 2D of a bf16 cache
    g = torch.Generator().manual_seed(1)
    k1, v1 = torch.randn(B, nkv, 9, D, generator=g) * 30, torch.randn(B, nkv, 9, D, generator=g)
    k2, v2 = torch.randn(B, nkv, 1, D, generator=g), torch.randn(B, nkv, 1, D, generator=g)
    K, V = cache.update(k1, v1, 0)
    assert K is cache.staging[0] and V is cache.staging[1] and K.shape == (B, nkv, L, D)
    assert torch.equal(K[:, :, :9], mx_round(k1.reshape(-1, D), 8)[0].view(B, nkv, 9, D))
    assert torch.equal(V[:, :, :9], mx_round(v1.reshape(-1, D), 8)[0].view(B, nkv, 9, D))
    assert int(l0.cumulative_length) == 9 and int(cache.layers[1].cumulative_length) == 0
    K1, _ = cache.update(k2, v2, 1)                       # another layer: the same staging pair, now holding that layer
    assert K1 is K and torch.equal(K[:, :, :1], mx_round(k2.reshape(-1, D), 8)[0].view(B, nkv, 1, D))
    K, V = cache.update(k2, v2, 0)
    assert int(l0.cumulative_length) == 10
    assert torch.equal(K[:, :, :9], mx_round(k1.reshape(-1, D), 8)[0].view(B, nkv, 9, D))                  # dequantised again from the codes
    assert torch.equal(K[:, :, 9:10], mx_round(k2.reshape(-1, D), 8)[0].view(B, nkv, 1, D))
    codes, scales = mx8_quantize_rows(k1)
    assert torch.equal(l0.keys[:, :, :9], codes) and torch.equal(l0.key_scales[:, :, :9], scales)
    assert not l0.keys[:, :, 10:].any() and not l0.values[:, :, 10:].any()
    cache.reset()
    assert int(l0.cumulative_length) == 0 and not l0.keys.any() and not l0.key_scales.any() and not l0.value_scales.any()


def _mx_dynamic_cache(config):
    from transformers import DynamicCache

    class MXDynamicCache(DynamicCache):
        """HF's own growing cache holding mx_round of every new row: the reference of the MX8 decode"""

        def update(self, key_states, value_states, layer_idx, *a, **k):
            D = key_states.shape[-1]
            kq = mx_round(key_states.reshape(-1, D), 8)[0].view(key_states.shape).to(key_states.dtype)
            vq = mx_round(value_states.reshape(-1, D), 8)[0].view(value_states.shape).to(value_states.dtype)
            return super().update(kq, vq, layer_idx, *a, **k)

    return MXDynamicCache(config=config)


def test_mxfp8_decoder_decodes_what_hf_generates_on_an_mx_rounding_dynamic_cache():
    llm = e2e.build_llm("tiny", "cpu", torch.float32)
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(5, 1000, (2, 12), generator=g)
    mask = torch.ones_like(prompt)
    mask[1, :4] = 0
    ref = llm.generate(inputs=prompt, attention_mask=mask, max_new_tokens=10, past_key_values=_mx_dynamic_cache(llm.config), **KW)
    dec = GraphedDecoder(llm, use_graph=False, kv_cache="mxfp8")
    got = dec.generate(prompt, mask, max_new_tokens=10, **KW)
    assert torch.equal(ref, got)
    assert isinstance(dec.cache, MX8StaticCache) and dec.cache.layers[0].keys.dtype == torch.uint8
    assert int(dec.cache.layers[0].cumulative_length) == int(dec.cache.layers[1].cumulative_length) == 12 + 9
    assert torch.equal(got, dec.generate(prompt, mask, max_new_tokens=10, **KW))            # the cache is reset and re-used
    plain = llm.generate(inputs=prompt, attention_mask=mask, max_new_tokens=10, **KW)
    assert torch.equal(plain, GraphedDecoder(llm, use_graph=False).generate(prompt, mask, max_new_tokens=10, **KW))     # the default: unchanged


def test_option_values_beams_and_environment(monkeypatch):
    llm = e2e.build_llm("tiny", "cpu", torch.float32)
    assert check_kv_cache(None) is None and check_kv_cache("mxfp8") == "mxfp8"
    for bad in ("fp8", "bf16", "", 8, True):
        with pytest.raises(ValueError, match="kv_cache"):
            GraphedDecoder(llm, use_graph=False, kv_cache=bad)
    prompt = torch.randint(5, 1000, (1, 6), generator=torch.Generator().manual_seed(3))
    dec = GraphedDecoder(llm, use_graph=False, kv_cache="mxfp8")
    with pytest.raises(NotImplementedError, match="num_beams.*kv_cache|kv_cache.*num_beams"):
        dec.generate(prompt, torch.ones_like(prompt), max_new_tokens=4, num_beams=2, **KW)
    from transformers import StaticCache
    plain = GraphedDecoder(llm, use_graph=False)
    assert plain.kv_cache is None
    plain.generate(prompt, torch.ones_like(prompt), max_new_tokens=3, **KW)
    assert type(plain.cache) is StaticCache and plain.cache.layers[0].keys.dtype == torch.float32
    monkeypatch.setenv("LLAMOLE_KV_CACHE", "mxfp8")
    assert GraphedDecoder(llm, use_graph=False).kv_cache == "mxfp8"
    monkeypatch.setenv("LLAMOLE_KV_CACHE", "int4")
    with pytest.raises(ValueError, match="kv_cache"):
        GraphedDecoder(llm, use_graph=False)


def test_report_names_the_cache_only_when_it_is_on(monkeypatch):
    monkeypatch.delenv("LLAMOLE_KV_CACHE", raising=False)
    llm = e2e.build_llm("tiny", "cpu", torch.float32)
    gd = types.SimpleNamespace(text_input_size=768, max_n_nodes=8)
    orch, _ = e2e.build_orchestrator(llm, gd, "cpu", torch.float32)
    assert orch.enable_mi355x_decode() == {"linears": 0} and orch.decoder.kv_cache is None
    assert orch.enable_mi355x_decode(kv_cache="mxfp8") == {"linears": 0, "kv_cache": "mxfp8"} and orch.decoder.kv_cache == "mxfp8"
    orch.enable_graphed_decode(use_graph=False, kv_cache="mxfp8")
    assert orch.decoder.kv_cache == "mxfp8"
    with pytest.raises(ValueError, match="kv_cache"):
        orch.enable_mi355x_decode(kv_cache="e5m2")


def test_load_yaml_args_keeps_the_key(tmp_path):
    from llamole_amd.eval import load_yaml_args
    p = tmp_path / "cfg.yaml"
    p.write_text("model_name_or_path: x\nkv_cache_dtype: mxfp8\n")
    assert load_yaml_args(str(p))[0].kv_cache_dtype == "mxfp8"
    p.write_text("model_name_or_path: x\n")
    assert load_yaml_args(str(p))[0].kv_cache_dtype is None
    assert load_yaml_args(str(p), {"kv_cache_dtype": "mxfp8"})[0].kv_cache_dtype == "mxfp8"
