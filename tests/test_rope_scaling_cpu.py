"""Scaled rotary embeddings, host side: the ``rope_scaling`` YAML key (rope.configure_rope, the reference's model_utils/rope.py:34-62 on
transformers' ``rope_parameters``), the definition of dynamic NTK that the device-side prologue implements, and the reset of a dynamic
module before each prefill of GraphedDecoder."""
import warnings

import pytest
import torch

DYNAMIC = dict(rope_parameters=dict(rope_type="dynamic", rope_theta=1e4, factor=2.0), max_position_embeddings=16)


def _llama_config(max_pos=2048):
    from transformers import LlamaConfig
    return LlamaConfig(hidden_size=64, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1, intermediate_size=64, vocab_size=64,
                       max_position_embeddings=max_pos, rope_theta=50000.0)


@pytest.mark.parametrize("kind,cutoff,want_factor,want_max", [("linear", 128, 1.0, 2048), ("dynamic", 4096, 2.0, 4096),
                                                              ("dynamic", 5000, 3.0, 5000), ("linear", None, 2.0, 2048)])
def test_configure_rope_table(kind, cutoff, want_factor, want_max):
    from llamole_amd.rope import configure_rope
    cfg = _llama_config()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        configure_rope(cfg, kind, cutoff)
    assert cfg.rope_parameters == {"rope_type": kind, "factor": want_factor, "rope_theta": 50000.0}      # rope_theta is kept
    assert isinstance(cfg.rope_parameters["factor"], float) and cfg.max_position_embeddings == want_max
    # the reference's warning when the input length does not exceed the model's
    assert any("smaller than max length" in str(x.message) for x in w) == (cutoff is not None and cutoff <= 2048)


def test_configure_rope_none_invalid_and_unsupported():
    from transformers import GPT2Config
    from llamole_amd.rope import configure_rope
    cfg = _llama_config()
    before = cfg.to_dict()
    configure_rope(cfg, None, 4096)
    assert cfg.to_dict() == before
    with pytest.raises(ValueError, match="'linear' and 'dynamic'"):
        configure_rope(cfg, "yarn", 4096)
    assert cfg.to_dict() == before
    gpt = GPT2Config(n_layer=1, n_head=1, n_embd=8)
    before = gpt.to_dict()
    with pytest.warns(UserWarning, match="does not support RoPE scaling"):
        configure_rope(gpt, "linear", 4096)
    assert gpt.to_dict() == before and not hasattr(gpt, "rope_parameters")
    # training with dynamic scaling: the reference's warning
    with pytest.warns(UserWarning, match="may not work well with fine-tuning"):
        configure_rope(_llama_config(), "dynamic", 4096, is_trainable=True)


def test_yaml_carries_rope_scaling_into_the_loaded_model(tmp_path):
    """load_yaml_args keeps the key, and the LLM loader of GraphLLMForCausalMLM.from_pretrained applies it to the config of a local checkpoint
    before the weights are loaded, with model_max_length = cutoff_len."""
    import yaml
    from transformers import LlamaForCausalLM
    from llamole_amd.eval import load_yaml_args
    from llamole_amd.modeling_llamole import GraphLLMForCausalMLM
    torch.manual_seed(0)
    src = LlamaForCausalLM(_llama_config(max_pos=32))
    src.save_pretrained(str(tmp_path / "llm"))
    ycfg = tmp_path / "gen.yaml"
    base = dict(model_name_or_path=str(tmp_path / "llm"), cutoff_len=80)
    yaml.safe_dump(dict(base, rope_scaling="dynamic"), open(ycfg, "w"))
    margs, dargs, targs, _, _ = load_yaml_args(str(ycfg))
    assert margs.rope_scaling == "dynamic"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        llm = GraphLLMForCausalMLM.load_language_model(margs, dargs, targs)
    assert llm.config.rope_parameters == {"rope_type": "dynamic", "factor": 3.0, "rope_theta": 50000.0}
    assert llm.config.max_position_embeddings == 80 and llm.model.rotary_emb.rope_type == "dynamic"
    assert torch.equal(llm.model.layers[0].self_attn.q_proj.weight, src.model.layers[0].self_attn.q_proj.weight)
    # without the key the checkpoint's own config stands
    yaml.safe_dump(base, open(ycfg, "w"))
    margs, dargs, targs, _, _ = load_yaml_args(str(ycfg))
    assert margs.rope_scaling is None
    llm = GraphLLMForCausalMLM.load_language_model(margs, dargs, targs)
    assert llm.config.rope_parameters["rope_type"] == "default" and llm.config.max_position_embeddings == 32
    # a value the reference does not know is refused before anything is loaded
    margs.rope_scaling = "ntk"
    with pytest.raises(ValueError, match="'linear' and 'dynamic'"):
        GraphLLMForCausalMLM.load_language_model(margs, dargs, targs)


def test_dynamic_semantics_are_hfs_module_from_its_constructed_state():
    """What ll_decode_prologue_dyn implements: with L = max(position ids) + 1, inv_freq = original_inv_freq while L <= max_position_embeddings and
    transformers' own init function at L beyond -- equal to what HF's stateful module holds at every call of a sequence of non-decreasing
    lengths from its constructed state (a generate call).  The function is called as the module calls it, with the length as a 0-dim int64
    tensor; rows of the table are those values."""
    from llamole_amd.e2e import build_llm
    from llamole_amd.rope import dynamic_inv_freq, dynamic_inv_freq_table, reset_dynamic_rope
    m = build_llm("tiny-llama", "cpu", dtype=torch.float32, **DYNAMIC)
    rot = m.model.rotary_emb
    table = dynamic_inv_freq_table(m.config, "cpu", 64)
    assert table.shape == (48, 32) and table.dtype == torch.float32
    assert dynamic_inv_freq_table(m.config, "cpu", 16) is None
    x = torch.zeros(1, 1, 4)
    for L in range(8, 30):
        cos, sin = rot(x, torch.arange(L)[None])
        want = rot.original_inv_freq if L <= 16 else dynamic_inv_freq(m.config, "cpu", torch.tensor(L))
        assert torch.equal(rot.inv_freq, want), L
        assert torch.equal(rot.inv_freq, rot.original_inv_freq if L <= 16 else table[L - 17]), L
        assert rot.attention_scaling == 1.0
    assert torch.equal(dynamic_inv_freq(m.config, "cpu", torch.tensor(12)), dynamic_inv_freq(m.config, "cpu", torch.tensor(16)))
    # HF differs only when a shorter call that is still above max_position_embeddings follows a longer one: it keeps the longer call's
    # frequencies; from the constructed state it holds the call's own
    rot(x, torch.arange(20)[None])
    assert torch.equal(rot.inv_freq, table[28 - 16])
    assert reset_dynamic_rope(m) and rot.max_seq_len_cached == 16 and torch.equal(rot.inv_freq, rot.original_inv_freq)
    rot(x, torch.arange(20)[None])
    assert torch.equal(rot.inv_freq, table[20 - 17])
    assert not reset_dynamic_rope(build_llm("tiny-llama", "cpu", dtype=torch.float32))


def test_decoder_resets_a_dynamic_module_before_each_prefill(monkeypatch):
    """After a 22-token call (8 new tokens: HF's module ends at F(29)), an 18-token call on the same decoder -- above
    max_position_embeddings = 16, so transformers' own reset branch does not fire, and below the first call's length, so HF's module alone
    would keep F(29) through the prefill and the steps up to 25 positions -- equals a fresh model's, plain and beam."""
    from llamole_amd import rope
    from llamole_amd.e2e import build_llm
    from llamole_amd.llm_decode import GraphedDecoder
    g = torch.Generator().manual_seed(0)
    ids22, ids18 = torch.randint(5, 2000, (1, 22), generator=g), torch.randint(5, 2000, (1, 18), generator=g)
    kw = dict(max_new_tokens=8, do_sample=False)

    def fresh(**extra):
        d = GraphedDecoder(build_llm("tiny-llama", "cpu", dtype=torch.float32, **DYNAMIC), use_graph=False)
        return d.generate(ids18, **kw, **extra), d.last_logits.clone()

    m = build_llm("tiny-llama", "cpu", dtype=torch.float32, **DYNAMIC)
    dec = GraphedDecoder(m, use_graph=False)
    for extra in ({}, dict(num_beams=2)):
        dec.generate(ids22, **kw)
        assert int(m.model.rotary_emb.max_seq_len_cached) == 29
        out = dec.generate(ids18, **kw, **extra)
        want, want_logits = fresh(**extra)
        assert torch.equal(out, want) and torch.equal(dec.last_logits, want_logits), extra
    # the comparison sees the reset: without it HF's module keeps the longer call's frequencies and the logits differ
    monkeypatch.setattr(rope, "reset_dynamic_rope", lambda model: False)
    dec.generate(ids22, **kw)
    dec.generate(ids18, **kw)
    assert not torch.equal(dec.last_logits, fresh()[1])


def test_from_pretrained_loads_the_llm_through_the_rope_aware_loader(tmp_path, monkeypatch):
    """GraphLLMForCausalMLM.from_pretrained hands the YAML's namespaces to load_language_model when no language model is passed, and a
    training YAML (do_train) with rope_scaling: dynamic gets the reference's fine-tuning warning from there."""
    import yaml
    from transformers import LlamaForCausalLM
    from llamole_amd.eval import load_yaml_args
    from llamole_amd.modeling_llamole import GraphLLMForCausalMLM
    torch.manual_seed(0)
    LlamaForCausalLM(_llama_config(max_pos=32)).save_pretrained(str(tmp_path / "llm"))
    ycfg = tmp_path / "train.yaml"
    yaml.safe_dump(dict(model_name_or_path=str(tmp_path / "llm"), cutoff_len=64, rope_scaling="dynamic", do_train=True), open(ycfg, "w"))
    margs, dargs, targs, fargs, _ = load_yaml_args(str(ycfg))
    seen = []

    class Loaded(Exception):
        pass

    orig = GraphLLMForCausalMLM.load_language_model

    def spy(model_args, data_args=None, training_args=None):
        seen.append((model_args, data_args, training_args))
        with pytest.warns(UserWarning, match="may not work well with fine-tuning"):
            llm = orig(model_args, data_args, training_args)
        assert llm.config.rope_parameters == {"rope_type": "dynamic", "factor": 2.0, "rope_theta": 50000.0}
        assert llm.config.max_position_embeddings == 64
        raise Loaded            # what follows in from_pretrained (device move, graph modules) is not this test's subject

    monkeypatch.setattr(GraphLLMForCausalMLM, "load_language_model", staticmethod(spy))
    with pytest.raises(Loaded):
        GraphLLMForCausalMLM.from_pretrained(None, margs, dargs, targs, fargs)
    assert len(seen) == 1 and seen[0][0] is margs and seen[0][1] is dargs and seen[0][2] is targs


def test_llama31_rope_parameters_build_the_published_rotary_module():
    from llamole_amd.e2e import LLAMA31_ROPE, LLM_CONFIGS, build_llm
    assert LLAMA31_ROPE == dict(rope_type="llama3", rope_theta=500000.0, factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0,
                                original_max_position_embeddings=8192)
    assert "rope_parameters" not in LLM_CONFIGS["llama-3.1-8b"]          # the measured entry keeps default rope
    m = build_llm("tiny-llama", "cpu", dtype=torch.float32, rope_parameters=LLAMA31_ROPE, max_position_embeddings=131072)
    rot = m.model.rotary_emb
    assert rot.rope_type == "llama3" and rot.attention_scaling == 1.0
    ratio = rot.inv_freq / build_llm("tiny-llama", "cpu", dtype=torch.float32, rope_theta=500000.0).model.rotary_emb.inv_freq
    assert float(ratio.max()) == 1.0 and abs(float(ratio.min()) - 0.125) < 1e-6       # high frequencies stay, low ones are divided by 8
