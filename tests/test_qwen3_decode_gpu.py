"""The fused decode on a Qwen3-layout model (per-head q / k RMSNorm inside the attention launches): the whole stack installs on `tiny-qwen3` and
serves every path (five-launch layers, seven-launch layers, fused query-token forward, beams, all captured), one fused decode step agrees with
the untouched HF model as well as HF's own bf16 does, and `quantization_bit` packs the layers as for Qwen2.  The norm weights are drawn at random
(e2e.randomize_head_norms): HF's ones would hide a missing or swapped weight.

Measured on an MI355X (printed with -s; the first line of profiles/decode_qwen3_time.txt): one fused decode step E = 0.0103 against HF's own
bf16 Y = 0.0107 (E / Y = 0.97, bound 1.5); with all-ones norm weights in the fused layers E = 0.56.  The packed 4-bit route and the bf16 kernels
on the dequantised weights gave logits less than 5e-6 apart at 2 rows (max |logit| 1.17)."""
import copy
import warnings

import pytest
import torch

from llamole_amd import e2e
from llamole_amd.llm_decode import GraphedDecoder
from tests.test_rope_scaling_gpu import _cases, _decode_all

pytestmark = pytest.mark.gpu

MARGIN = 1.5            # a bf16 engine against the reference's own bf16: the project's margin of record


def _restore(llm):
    from llamole_amd.llm_accel import restore_decoder_layers, restore_elementwise, restore_linears, restore_model_decode
    restore_model_decode(llm)
    restore_decoder_layers(llm)
    restore_elementwise(llm)
    restore_linears(llm)


def _build():
    llm = e2e.build_llm("tiny-qwen3", "cuda", torch.bfloat16)
    assert e2e.randomize_head_norms(llm) == 4
    att = llm.model.layers[0].self_attn
    assert att.head_dim == 128 and att.q_proj.out_features == 512 != llm.config.hidden_size
    assert not torch.equal(att.q_norm.weight, att.k_norm.weight) and not torch.equal(att.q_norm.weight, torch.ones_like(att.q_norm.weight))
    return llm


def test_the_stack_installs_and_serves_every_path(monkeypatch):
    from llamole_amd.llm_accel import _FusedLayer, accelerate_llm
    llm = _build()
    calls = []
    for name in ("run64", "run_suffix"):
        orig = getattr(_FusedLayer, name)
        monkeypatch.setattr(_FusedLayer, name, lambda self, *a, _o=orig, _n=name, **k: (calls.append(_n), _o(self, *a, **k))[1])
    side = []                                                    # state of a side graph's shape after each call that went through it
    captured = GraphedDecoder._captured

    def watch(self, key, statics, fn):
        out = captured(self, key, statics, fn)
        side.append((key, type(self._side_graphs.get(key)).__name__))
        return out
    monkeypatch.setattr(GraphedDecoder, "_captured", watch)
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            info = accelerate_llm(llm)
            assert info["decoder_layers_5_launches"] == llm.config.num_hidden_layers == 2
            assert info["decode_prologue_1_launch"] is True and not [k for k in info if k.endswith("_declined")]
            assert all(l._ll_fused.qn is l.self_attn.q_norm and l._ll_fused.kn is l.self_attn.k_norm for l in llm.model.layers)
            out = _decode_all(llm)        # asserts: the second continue_hidden equals the first bitwise, step and beam step captured
        assert not rec, [str(w.message) for w in rec]
        assert "run64" in calls and "run_suffix" in calls
        # the query-token forward: eager when its shape is first seen, captured (graph, static buffers, output) and replayed the second time;
        # the step graph and the beam step graph are asserted inside _decode_all
        assert side == [(("suffix", 1, 9), "str"), (("suffix", 1, 9), "tuple")], side
        for case in ("pad2", "rows24", "beams"):
            assert torch.isfinite(out[case][1].float()).all()
        assert torch.isfinite(out["suffix"][1].float()).all()
    finally:
        _restore(llm)


def _step_logits(llm, prompt, mask):
    """(tokens [B, P + 2], logits of the ONE fused decode step behind the first new token) of a greedy two-token generate"""
    dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
    toks = dec.generate(prompt, mask, max_new_tokens=2, do_sample=False, pad_token_id=0, eos_token_id=[])
    return toks, dec.last_logits.float().clone()


def _hf_logits(model, ids, mask):
    pos = (mask.long().cumsum(dim=1) - 1).clamp_min(0)
    with torch.no_grad():
        return model(input_ids=ids, attention_mask=mask, position_ids=pos, use_cache=False).logits[:, -1, :].float()


def test_one_fused_decode_step_against_hf():
    """3 left-padded rows of 13 tokens, greedy, max_new_tokens = 2: last_logits are those of one fused decode step.  On the same device the
    untouched HF model in f32 and in bf16 on prompt + first token: Y = max |bf16 - f32| is the yardstick, E = max |fused - f32| the engine's
    error, E <= 1.5 Y.  Control: the fused layers handed all-ones norm weights miss that by far."""
    from llamole_amd.llm_accel import _FusedLayer, accelerate_llm
    llm = _build()
    hf16, hf32 = copy.deepcopy(llm), copy.deepcopy(llm).float()
    g = torch.Generator().manual_seed(13)
    prompt = torch.randint(5, 2000, (3, 13), generator=g).cuda()
    mask = torch.ones_like(prompt)
    mask[1, :4] = 0
    mask[2, :7] = 0
    try:
        info = accelerate_llm(llm)
        assert info["decoder_layers_5_launches"] == 2 and info["decode_prologue_1_launch"]
        calls = []
        orig = _FusedLayer.run
        _FusedLayer.run = lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1]
        try:
            toks, fused = _step_logits(llm, prompt, mask)
        finally:
            _FusedLayer.run = orig
        assert len(calls) == 2                                     # one decode step through both fused layers
        ids = toks[:, :14]
        full = torch.cat([mask, torch.ones_like(mask[:, :1])], dim=1)
        ref = _hf_logits(hf32, ids, full)
        Y = float((_hf_logits(hf16, ids, full) - ref).abs().max())
        E = float((fused - ref).abs().max())
        print(f"\ntiny-qwen3 one decode step, max |logit error| against HF f32: fused E = {E:.5f}, HF bf16 Y = {Y:.5f}, E / Y = {E / Y:.3f}")
        assert Y > 0 and E <= MARGIN * Y, (E, Y)
        # control: ones in place of the norm weights inside the fused layers only (the prefill still runs HF's modules)
        ones = torch.ones_like(llm.model.layers[0].self_attn.q_norm.weight)
        for layer in llm.model.layers:
            layer._ll_fused.qn = layer._ll_fused.kn = type("Ones", (), {"weight": ones})()
        toks1, wrong = _step_logits(llm, prompt, mask)
        assert torch.equal(toks1[:, :14], ids)                     # the same prefill and first token: the same step is compared
        E1 = float((wrong - ref).abs().max())
        print(f"control, all-ones norm weights in the fused layers: E = {E1:.5f}")
        assert E1 > MARGIN * Y
    finally:
        _restore(llm)


def test_quantised_qwen3_packs_both_layers_and_both_routes_decode_the_same_tokens(monkeypatch):
    """quantization_bit = 4: only the seven Linears are rounded, the norm weights stay; the packed route and the bf16 kernels on the dequantised
    weights decode the same tokens (the logits within 0.03 max |logit|, the limit tests/test_quant_gpu.py holds Qwen2 to)."""
    from llamole_amd import llm_accel
    from llamole_amd.llm_accel import accelerate_llm, set_packed_route
    monkeypatch.setattr(llm_accel, "WQ_ROUTES", llm_accel.all_packed_routes())
    llm = _build()
    norms = [l.self_attn.q_norm.weight.clone() for l in llm.model.layers]
    p2, m2, _, _, _ = _cases()
    kw = dict(max_new_tokens=2, do_sample=False, pad_token_id=0, eos_token_id=[])
    try:
        info = accelerate_llm(llm, quantization_bit=4)
        q = info["quantization"]
        assert q["bits"] == 4 and q["modules"] == 14 and q["packed_layers"] == 2 and q["bf16_layers"] == 0
        assert info["decoder_layers_5_launches"] == 2 and "decoder_layers_declined" not in info
        assert all(torch.equal(l.self_attn.q_norm.weight, w) for l, w in zip(llm.model.layers, norms))
        calls = []
        st0 = llm.model.layers[0]._ll_fused
        orig = st0._gemv_wq
        st0._gemv_wq = lambda x, *a, **k: (calls.append(x.shape[0]), orig(x, *a, **k))[1]
        dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
        packed = dec.generate(p2, m2, **kw)
        packed_logits = dec.last_logits.float().clone()
        assert calls == [2] * 4
        assert set_packed_route(llm, False) == 2
        dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
        plain = dec.generate(p2, m2, **kw)
        assert calls == [2] * 4                                    # the packed kernels did not run this time
        scale = float(dec.last_logits.float().abs().max())
        diff = float((dec.last_logits.float() - packed_logits).abs().max())
        print(f"\npacked against bf16 route: max |logit difference| {diff:.5f} of max |logit| {scale:.4f}")
        assert diff <= 0.03 * scale
        assert torch.equal(packed, plain)
    finally:
        _restore(llm)
