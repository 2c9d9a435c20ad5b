"""quantization_bit without a GPU: the MX quantiser in torch (known answers, properties), quantised tiny models on CPU, the option surface."""
import pytest
import torch

from llamole_amd import e2e
from llamole_amd.llm_decode import GraphedDecoder
from llamole_amd.llm_quant import (E2M1_VALUES, FORMATS, LAYER_LINEARS, check_quantization_bit, decode_codes, mx_round, quantize_llm)


def _scales(sb):
    return torch.ldexp(torch.ones(()), sb.to(torch.int32) - 127).repeat_interleave(32, dim=1)


# ------------------------------------------------------------------------------------------------ known answers
def test_e4m3_codes_decode_like_torch_float8():
    codes = torch.arange(256, dtype=torch.uint8)
    want = codes.view(torch.float8_e4m3fn).float()
    got = decode_codes(codes, 8)
    ok = ~torch.isnan(want)
    assert int((~ok).sum()) == 2 and torch.isnan(got[~ok]).all()       # 0x7f, 0xff
    assert torch.equal(got[ok], want[ok])
    # every finite code value is a fixed point of the quantiser at scale 1 (448 in the block pins e = 0)
    vals = got[ok]
    for i in range(0, len(vals), 31):
        blk = torch.zeros(1, 32)
        blk[0, :len(vals[i:i + 31])] = vals[i:i + 31]
        blk[0, 31] = 448.0
        dq, sb = mx_round(blk, 8)
        assert torch.equal(dq, blk) and int(sb) == 127


def test_e2m1_codes_and_ties_to_even():
    want = torch.tensor(list(E2M1_VALUES) + [-v for v in E2M1_VALUES])
    assert E2M1_VALUES == (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
    assert torch.equal(decode_codes(torch.arange(16, dtype=torch.uint8), 4), want)
    blk = torch.zeros(1, 32)
    blk[0, :16] = want
    dq, sb = mx_round(blk, 4)
    assert torch.equal(dq, blk) and int(sb) == 127
    # ties round to even at scale 1 (a 6 in the block pins e = 0): 2.5 -> 2, 5.0 -> 4, 3.5 -> 4, 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2
    t = torch.zeros(1, 32)
    t[0, :9] = torch.tensor([6.0, 2.5, 5.0, -3.5, 0.25, 0.75, 1.25, 1.75, -2.5])
    dq, sb = mx_round(t, 4)
    assert int(sb) == 127
    assert dq[0, :9].tolist() == [6.0, 2.0, 4.0, -4.0, 0.0, 1.0, 1.0, 2.0, -2.0]
    # E4M3 at scale 1: the step is 32 in [256, 448], 1/8 in [1, 2)
    t = torch.zeros(1, 32)
    t[0, :5] = torch.tensor([448.0, 272.0, 304.0, 1.0625, 1.1875])
    dq, sb = mx_round(t, 8)
    assert int(sb) == 127 and dq[0, :5].tolist() == [448.0, 256.0, 320.0, 1.0, 1.25]


# ------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("K", [3584, 18944])
def test_quantiser_properties(bits, K):
    f = FORMATS[bits]
    g = torch.Generator().manual_seed(K + bits)
    w = 0.02 * torch.randn(24, K, generator=g)
    w[2, 70] = 1.5                        # blocks with one outlier
    w[5, 1000] = -0.9
    w[7, 32:64] = 0                       # an all-zero block
    wb = w.bfloat16().float()
    dq, sb = mx_round(w, bits)
    assert dq.shape == w.shape and sb.shape == (24, K // 32) and sb.dtype == torch.uint8
    assert torch.equal(dq.bfloat16().float(), dq)                      # every dequantised weight is exactly a bf16 number
    dq2, _ = mx_round(dq, bits)
    assert torch.equal(dq2, dq)                                        # idempotent on values
    sc = _scales(sb)
    assert (wb.abs() / sc <= f["vmax"]).all()                          # no element saturates
    err = (wb - dq).abs()
    if bits == 8:
        assert (err <= torch.maximum(wb.abs() * 2.0 ** -4, sc * 2.0 ** -10)).all()
        assert torch.equal((wb / sc).to(torch.float8_e4m3fn).float() * sc, dq)      # the element rounding is torch's own E4M3 conversion
    else:
        assert (err <= sc).all()
    assert (dq[7, 32:64] == 0).all() and int(sb[7, 1]) == 127
    # the scale is the smallest power of two that fits the block maximum
    amax = wb.reshape(24, K // 32, 32).abs().amax(-1)
    nz = amax > 0
    s1 = torch.ldexp(torch.ones(()), sb.to(torch.int32) - 127)
    assert (amax[nz] / s1[nz] <= f["vmax"]).all() and (amax[nz] / (s1[nz] / 2) > f["vmax"]).all()


@pytest.mark.parametrize("bits", [8, 4])
def test_quantiser_refuses_partial_blocks(bits):
    with pytest.raises(ValueError, match="multiple of 32"):
        mx_round(torch.zeros(4, 48), bits)
    with pytest.raises(ValueError, match="4-bit or 8-bit"):
        mx_round(torch.zeros(4, 64), 5)


# ------------------------------------------------------------------------------------------------ quantised tiny models
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("arch", ["tiny", "tiny-llama", "tiny-mistral"])
def test_quantised_tiny_model_on_cpu(arch, bits):
    llm = e2e.build_llm(arch, "cpu", torch.float32)
    before = {k: v.clone() for k, v in llm.state_dict().items()}
    rep = quantize_llm(llm, bits)
    L = llm.config.num_hidden_layers
    assert rep["bits"] == bits and rep["format"] == FORMATS[bits]["name"] and rep["modules"] == 7 * L and rep["skipped"] == []
    assert rep["packed_bytes"] * 64 == rep["bf16_bytes"] * (4 * bits + 1)      # bits / 8 + 1 / 32 bytes per weight against 2
    assert rep["byte_ratio"] == round((bits / 8 + 1 / 32) / 2, 5)
    names = {f"{p}.{n}.weight" for p, n in LAYER_LINEARS}
    for k, v in llm.state_dict().items():
        is_layer_linear = any(k.endswith(n) for n in names) and ".layers." in k
        if is_layer_linear:
            assert not torch.equal(v, before[k]), k
            assert torch.equal(v, mx_round(before[k], bits)[0]), k
        else:
            assert torch.equal(v, before[k]), k                        # lm_head, the embeddings, the norms and the biases are untouched
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(5, 1000, (2, 12), generator=g)
    mask = torch.ones_like(prompt)
    mask[1, :4] = 0
    kw = dict(max_new_tokens=10, do_sample=False, pad_token_id=0, eos_token_id=[2047])
    ref = llm.generate(inputs=prompt, attention_mask=mask, **kw)
    got = GraphedDecoder(llm, use_graph=False).generate(prompt, mask, **kw)
    assert torch.equal(ref, got)


def test_enable_mi355x_decode_rounds_a_cpu_model():
    import types
    llm = e2e.build_llm("tiny", "cpu", torch.float32)
    w0 = llm.model.layers[0].mlp.down_proj.weight.clone()
    gd = types.SimpleNamespace(text_input_size=768, max_n_nodes=8)
    orch, tok = e2e.build_orchestrator(llm, gd, "cpu", torch.float32)
    info = orch.enable_mi355x_decode(quantization_bit=4)
    assert info["linears"] == 0 and info["quantization"]["bits"] == 4 and info["quantization"]["modules"] == 14
    assert torch.equal(llm.model.layers[0].mlp.down_proj.weight, mx_round(w0, 4)[0])
    assert orch.decoder is not None and not orch.decoder.use_graph


# ------------------------------------------------------------------------------------------------ options
def test_check_quantization_bit():
    assert check_quantization_bit(None) is None and check_quantization_bit(4) == 4 and check_quantization_bit(8) == 8
    for bad in (3, 16, 0, "8", 8.0, True):
        with pytest.raises(ValueError, match="4-bit or 8-bit"):
            check_quantization_bit(bad)


def test_yaml_surface_carries_the_key_and_training_refuses_it(tmp_path):
    import yaml
    from llamole_amd import eval as ev
    from llamole_amd import train as tr
    cfg = tmp_path / "c.yaml"
    cfg.write_text(yaml.safe_dump({"model_name_or_path": "x", "quantization_bit": 8}))
    assert ev.load_yaml_args(str(cfg))[0].quantization_bit == 8
    assert ev.load_yaml_args(str(cfg), overrides={"quantization_bit": 4})[0].quantization_bit == 4
    plain = tmp_path / "p.yaml"
    plain.write_text(yaml.safe_dump({"model_name_or_path": "x"}))
    assert ev.load_yaml_args(str(plain))[0].quantization_bit is None
    with pytest.raises(ValueError, match="QLoRA"):
        tr.run_train(str(cfg))
    with pytest.raises(ValueError, match="4-bit or 8-bit"):
        ev.run_eval(str(plain), overrides={"quantization_bit": 3})
