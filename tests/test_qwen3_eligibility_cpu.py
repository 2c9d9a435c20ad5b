"""`llm_accel.decoder_layer_declined` on CPU models: the Qwen3 layout (an RMSNorm over head_dim on q and k) is accepted up to the dtype / device
reasons, which come last; a whole-width norm (the OLMo2 layout), a single norm, unequal eps, a norm class without variance_epsilon and a
sliding-window layer are declined for their structure; for the layouts fused so far the answer is the one `fuse_decoder_layers` gave before."""
import pytest
import torch
import torch.nn as nn

from llamole_amd import e2e
from llamole_amd.llm_accel import _is_silu, accelerate_llm, decoder_layer_declined

DEVICE_REASONS = ("weights are not bf16", "weights are not on the device")


@pytest.fixture()
def qwen3():
    return e2e.build_llm("tiny-qwen3", "cpu", torch.bfloat16)


def test_the_config_entries():
    tiny, big = e2e.LLM_CONFIGS["tiny-qwen3"], e2e.LLM_CONFIGS["qwen3-8b"]
    assert tiny["cls"] == big["cls"] == "Qwen3"
    assert tiny["num_attention_heads"] * tiny["head_dim"] == 512 != tiny["hidden_size"]
    assert (big["hidden_size"], big["num_hidden_layers"], big["num_attention_heads"], big["num_key_value_heads"], big["head_dim"],
            big["intermediate_size"], big["vocab_size"], big["max_position_embeddings"]) == (4096, 36, 32, 8, 128, 12288, 151936, 40960)


def test_a_cpu_qwen3_model_is_declined_for_its_device_only(qwen3):
    for layer in qwen3.model.layers:
        att = layer.self_attn
        assert type(att.q_norm).__name__ == "Qwen3RMSNorm" and att.q_norm.weight.numel() == att.head_dim == 128
        assert decoder_layer_declined(layer) == "weights are not on the device"
    assert decoder_layer_declined(e2e.build_llm("tiny-qwen3", "cpu", torch.float32).model.layers[0]) == "weights are not bf16"
    assert accelerate_llm(qwen3) == {"linears": 0}               # a CPU model: nothing is installed, nothing is reported


def test_randomize_head_norms_draws_q_and_k_apart(qwen3):
    assert e2e.randomize_head_norms(qwen3) == 4
    att = qwen3.model.layers[0].self_attn
    assert att.q_norm.weight.dtype == torch.bfloat16 and not torch.equal(att.q_norm.weight, att.k_norm.weight)
    assert 0.3 < float(att.q_norm.weight.float().std()) < 0.7 and abs(float(att.q_norm.weight.float().mean()) - 1) < 0.2
    assert decoder_layer_declined(qwen3.model.layers[0]) in DEVICE_REASONS
    assert e2e.randomize_head_norms(e2e.build_llm("tiny", "cpu", torch.bfloat16)) == 0


def test_structural_reasons_come_before_the_device(qwen3):
    layer = qwen3.model.layers[0]
    att = layer.self_attn
    Norm = type(att.q_norm)
    q_norm, k_norm = att.q_norm, att.k_norm
    # a norm over the whole projection width (OLMo2)
    att.q_norm = Norm(att.q_proj.out_features, eps=1e-6).to(torch.bfloat16)
    assert decoder_layer_declined(layer) == "q_norm is not a norm over head_dim"
    att.q_norm = q_norm
    att.k_norm = Norm(att.k_proj.out_features, eps=1e-6).to(torch.bfloat16)
    assert decoder_layer_declined(layer) == "k_norm is not a norm over head_dim"
    # only one of the two
    del att.k_norm
    assert decoder_layer_declined(layer) == "only one of q_norm / k_norm"
    att.k_norm = k_norm
    del att.q_norm
    assert decoder_layer_declined(layer) == "only one of q_norm / k_norm"
    # unequal eps
    att.q_norm = Norm(att.head_dim, eps=1e-5).to(torch.bfloat16)
    assert decoder_layer_declined(layer) == "q_norm and k_norm differ in variance_epsilon"
    # a norm class without variance_epsilon
    att.q_norm = nn.RMSNorm(att.head_dim, eps=1e-6).to(torch.bfloat16)
    assert decoder_layer_declined(layer) == "q_norm is not an RMSNorm with variance_epsilon"
    att.q_norm = nn.LayerNorm(att.head_dim).to(torch.bfloat16)
    assert decoder_layer_declined(layer) == "q_norm is not an RMSNorm with variance_epsilon"
    # an f32 norm weight on an otherwise bf16 layer: a dtype reason, after the structure
    att.q_norm = Norm(att.head_dim, eps=1e-6)
    assert decoder_layer_declined(layer) == "weights are not bf16"
    att.q_norm = q_norm
    assert decoder_layer_declined(layer) in DEVICE_REASONS
    # a sliding-window layer
    att.sliding_window = 128
    assert decoder_layer_declined(layer) == "sliding-window layer"
    att.sliding_window = None
    assert decoder_layer_declined(layer) in DEVICE_REASONS
    assert decoder_layer_declined(nn.Linear(4, 4)) == "no self_attn / mlp"


def _fused_before(layer):
    """the condition of fuse_decoder_layers before the per-head norms were accepted, word for word"""
    att, mlp = getattr(layer, "self_attn", None), getattr(layer, "mlp", None)
    if att is None or mlp is None or hasattr(layer, "_ll_fused"):
        return False
    return (all(type(getattr(att, a, None)) is nn.Linear for a in ("q_proj", "k_proj", "v_proj", "o_proj"))
            and all(type(getattr(mlp, a, None)) is nn.Linear for a in ("gate_proj", "up_proj", "down_proj"))
            and _is_silu(getattr(mlp, "act_fn", None)) and hasattr(layer, "input_layernorm")
            and hasattr(layer, "post_attention_layernorm") and hasattr(layer.input_layernorm, "variance_epsilon")
            and att.q_proj.weight.dtype == torch.bfloat16 and att.q_proj.weight.is_cuda
            and getattr(att, "head_dim", 0) in (64, 128) and att.q_proj.in_features % 8 == 0
            and att.q_proj.in_features <= 8192 and mlp.gate_proj.bias is None and mlp.up_proj.bias is None
            and mlp.down_proj.bias is None and getattr(att, "sliding_window", None) is None
            and not hasattr(att, "q_norm"))


@pytest.mark.parametrize("name", ["tiny", "tiny-llama", "tiny-mistral"])
def test_the_layouts_fused_so_far_get_the_answer_they_got(name):
    llm = e2e.build_llm(name, "cpu", torch.bfloat16)
    for layer in llm.model.layers:
        why = decoder_layer_declined(layer)
        assert (why is None) == _fused_before(layer)
        assert why == "weights are not on the device"            # nothing structural stands in the way: on the device it is fused, as before
    # and the structural part alone agrees too: the same layer with the device condition taken out of both
    for layer in llm.model.layers:
        layer.self_attn.sliding_window = 64
        assert decoder_layer_declined(layer) == "sliding-window layer" and not _fused_before(layer)
