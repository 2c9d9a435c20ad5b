"""Beam search / beam sample on the eager static-cache decoder and the torch beam step (CPU): HF GenerationMixin._beam_search."""
import pytest
import torch

from llamole_amd import e2e
from llamole_amd.llm_decode import GraphedDecoder

EOS10 = [2047, 7, 11, 13, 17, 19, 23, 29, 31, 37]


def _case(name):
    llm = e2e.build_llm(name, "cpu", torch.float32)
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(5, 1000, (2, 12), generator=g)
    mask = torch.ones_like(prompt)
    mask[1, :4] = 0
    prompt[1, :4] = 0                     # left pads
    return llm, prompt, mask


def _both(llm, prompt, mask, sync_every=16, **kw):
    ref = llm.generate(inputs=prompt, attention_mask=mask, **kw)
    got = GraphedDecoder(llm, use_graph=False, sync_every=sync_every).generate(prompt, mask, **kw)
    return ref, got


@pytest.mark.parametrize("name", ["tiny", "tiny-llama"])
@pytest.mark.parametrize("nb", [2, 4])
@pytest.mark.parametrize("lp", [1.0, 0.6, -1.0])
@pytest.mark.parametrize("es", [False, True, "never"])
def test_beam_equals_hf_generate(name, nb, lp, es):
    llm, prompt, mask = _case(name)
    kw = dict(max_new_tokens=10, do_sample=False, pad_token_id=0, eos_token_id=[2047], num_beams=nb, length_penalty=lp,
              early_stopping=es)
    ref, got = _both(llm, prompt, mask, **kw)
    assert torch.equal(ref, got)


def _early_eos(llm, prompt, mask, nb):
    """EOS ids that the beams of a plain run emit early: the second generated token of each item's best sequence."""
    kw = dict(max_new_tokens=10, do_sample=False, pad_token_id=0, eos_token_id=[2047], num_beams=nb)
    ref = llm.generate(inputs=prompt, attention_mask=mask, **kw)
    return sorted(set(int(x) for x in ref[:, 13]))


@pytest.mark.parametrize("name", ["tiny", "tiny-llama"])
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("es", [False, True, "never"])
@pytest.mark.parametrize("lp", [1.0, -1.0])
def test_early_hypotheses_and_fill(name, pad, es, lp):
    llm, prompt, mask = _case(name)
    for nb in (2, 4):
        eos = _early_eos(llm, prompt, mask, nb)
        kw = dict(max_new_tokens=16, do_sample=False, pad_token_id=pad, eos_token_id=eos + [2047], num_beams=nb, length_penalty=lp,
                  early_stopping=es)
        ref, got = _both(llm, prompt, mask, sync_every=1, **kw)
        assert torch.equal(ref, got), (nb, ref, got)
        ref16, got16 = _both(llm, prompt, mask, sync_every=16, **kw)
        assert torch.equal(got, got16)


def test_a_best_hypothesis_ends_early_and_pads_with_the_first_eos():
    llm, prompt, mask = _case("tiny")
    eos = _early_eos(llm, prompt, mask, 2)
    seen = False
    for pad in (0, 5):
        kw = dict(max_new_tokens=16, do_sample=False, pad_token_id=pad, eos_token_id=eos + [2047], num_beams=2)
        ref, got = _both(llm, prompt, mask, sync_every=1, **kw)
        assert torch.equal(ref, got)
        new = got[:, 12:]
        short = [b for b in range(2) if int(new[b, -1]) == (pad or eos[0]) and new.shape[1] > 1]
        seen = seen or bool(short)
    assert seen


def test_stops_globally_before_max_new_tokens():
    llm, prompt, mask = _case("tiny")
    eos = _early_eos(llm, prompt, mask, 2)
    kw = dict(max_new_tokens=40, do_sample=False, pad_token_id=0, eos_token_id=eos + [2047], num_beams=2, early_stopping=True)
    dec = GraphedDecoder(llm, use_graph=False, sync_every=1)
    got = dec.generate(prompt, mask, **kw)
    ref = llm.generate(inputs=prompt, attention_mask=mask, **kw)
    assert torch.equal(ref, got) and got.shape[1] < 12 + 40
    assert dec._last["n_new"] == got.shape[1] - 12


@pytest.mark.parametrize("name", ["tiny", "tiny-llama"])
@pytest.mark.parametrize("eos", [[2047], EOS10])
def test_eos_lists_and_inputs_embeds(name, eos):
    llm, prompt, mask = _case(name)
    kw = dict(max_new_tokens=8, do_sample=False, pad_token_id=0, eos_token_id=eos, num_beams=3, length_penalty=0.8)
    ref, got = _both(llm, prompt, mask, **kw)
    assert torch.equal(ref, got)
    emb = llm.get_input_embeddings()(prompt)
    ref_e = llm.generate(inputs_embeds=emb, attention_mask=mask, **kw)
    got_e = GraphedDecoder(llm, use_graph=False).generate(None, mask, inputs_embeds=emb, **kw)
    assert torch.equal(ref_e, got_e)


def test_sync_every_does_not_change_the_output():
    llm, prompt, mask = _case("tiny-llama")
    eos = _early_eos(llm, prompt, mask, 4)
    for es in (False, True):
        kw = dict(max_new_tokens=24, do_sample=False, pad_token_id=0, eos_token_id=eos, num_beams=4, early_stopping=es)
        a = GraphedDecoder(llm, use_graph=False, sync_every=1).generate(prompt, mask, **kw)
        b = GraphedDecoder(llm, use_graph=False, sync_every=16).generate(prompt, mask, **kw)
        assert torch.equal(a, b)
        kw_s = dict(kw, do_sample=True, temperature=0.6, top_p=0.9, top_k=50)
        a = GraphedDecoder(llm, use_graph=False, sync_every=1).generate(prompt, mask, generator=torch.Generator().manual_seed(3), **kw_s)
        b = GraphedDecoder(llm, use_graph=False, sync_every=16).generate(prompt, mask, generator=torch.Generator().manual_seed(3), **kw_s)
        assert torch.equal(a, b)


def test_validation():
    llm, prompt, mask = _case("tiny")
    dec = GraphedDecoder(llm, use_graph=False)
    with pytest.raises(ValueError):
        dec.generate(prompt, mask, max_new_tokens=2, do_sample=False, num_beams=2, early_stopping="sometimes")
    with pytest.raises(ValueError):
        dec.generate(prompt, mask, max_new_tokens=2, do_sample=False, num_beams=0)
    with pytest.raises(NotImplementedError):
        dec.generate(prompt, mask, max_new_tokens=2, do_sample=False, num_beams=1, length_penalty=0.8)
    with pytest.raises(NotImplementedError):
        dec.generate(prompt, mask, max_new_tokens=2, do_sample=False, num_beams=2, repetition_penalty=1.2)
    with pytest.raises(NotImplementedError):
        dec.generate(prompt, mask, max_new_tokens=2, do_sample=False, num_beams=2, output_scores=True)
    # num_beams 1 / None with neutral options: the plain decode, unchanged
    kw = dict(max_new_tokens=6, do_sample=False, pad_token_id=0, eos_token_id=[2047])
    plain = GraphedDecoder(llm, use_graph=False).generate(prompt, mask, **kw)
    assert torch.equal(plain, GraphedDecoder(llm, use_graph=False).generate(prompt, mask, num_beams=1, length_penalty=1.0, **kw))


def _hf_processed(lp, temperature, top_k, top_p, min_keep):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = lp.clone()
    if temperature != 1.0:
        s = TemperatureLogitsWarper(temperature)(None, s)
    if top_k:
        s = TopKLogitsWarper(top_k, min_tokens_to_keep=min_keep)(None, s)
    if top_p < 1.0:
        s = TopPLogitsWarper(top_p, min_tokens_to_keep=min_keep)(None, s)
    return s


@pytest.mark.parametrize("temperature,top_k,top_p,n_eos", [(0.6, 50, 0.9, 10), (1.0, 7, 0.5, 1), (0.8, 0, 0.95, 3)])
def test_torch_beam_sample_step_stays_in_hf_kept_set(temperature, top_k, top_p, n_eos):
    from llamole_amd.llm_beam import BeamParams, BeamState, beam_step_torch, beams_to_keep, state_layout
    B, nb, V, T = 3, 4, 300, 8
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(B * nb, V, generator=g) * 3).to(torch.bfloat16).float()
    eos = torch.arange(V - n_eos, V)
    K = beams_to_keep(nb, n_eos)
    p = BeamParams(B, nb, K, T, 8, eos, 1.0, False, True, temperature, top_k, top_p)

    def run(seed, t):
        st = BeamState(torch.zeros(state_layout(B, nb, K, T)[1], dtype=torch.uint8), B, nb, K, T)
        st.reset()
        st.run.copy_(torch.randn(B * nb, generator=torch.Generator().manual_seed(9)) - 3)     # a middle step: every beam live
        tok = beam_step_torch(logits, st, t, p, torch.Generator().manual_seed(seed))
        return tok, st

    tok, st = run(1, 2)
    tok2, st2 = run(1, 2)
    assert torch.equal(tok, tok2) and torch.equal(st.buf, st2.buf)
    kept = torch.isfinite(_hf_processed(torch.log_softmax(logits, -1), temperature, top_k, top_p, n_eos + 1))
    par = st.par.long()
    assert bool(kept[par, tok].all())
    draws = set()
    for seed in range(40):
        tok, st = run(seed, 2)
        par = st.par.long()
        assert bool(kept[par, tok].all())
        draws.add(tuple(tok.tolist()))
    assert len(draws) > 1


def test_graph_llm_generate_with_beams_and_design_hidden():
    from llamole_amd.modeling_llamole import GraphLLMForCausalMLM
    llm, prompt, mask = _case("tiny")
    m = GraphLLMForCausalMLM.__new__(GraphLLMForCausalMLM)
    torch.nn.Module.__init__(m)
    m.language_model = llm
    m.decoder = GraphedDecoder(llm, use_graph=False)
    kw = dict(max_new_tokens=6, do_sample=False, pad_token_id=0, eos_token_id=[2047], num_beams=3, length_penalty=0.8)
    got = m._llm_generate(inputs=prompt, attention_mask=mask, **kw)
    assert torch.equal(got, llm.generate(inputs=prompt, attention_mask=mask, **kw))
    # after a beam decode the cache holds running beams: no KV reuse, continue_hidden refuses
    with pytest.raises(RuntimeError):
        m.decoder.continue_hidden(got[:, -3:], 12 + 3)


def test_design_hidden_after_beams_takes_the_full_query_forward():
    """After a beam decode the cache holds running beams, not the returned sequence: design_hidden with reuse_query_kv gives the same
    condition as without it, and never runs the query tokens on top of the decode cache."""
    import types
    llm = e2e.build_llm("tiny", "cpu", torch.float32)
    orch, _ = e2e.build_orchestrator(llm, types.SimpleNamespace(text_input_size=768, max_n_nodes=8), "cpu", torch.float32)
    g = torch.Generator().manual_seed(1)
    prompt = torch.randint(5, 1000, (2, 12), generator=g)
    mask = torch.ones_like(prompt)
    kw = dict(do_sample=False, max_new_tokens=14, eos_token_id=[], pad_token_id=0, num_beams=3, length_penalty=0.8)
    orch.enable_graphed_decode(use_graph=False, reuse_query_kv=False)
    a0, ids0, c0 = orch.design_hidden(prompt, mask, None, **kw)
    orch.enable_graphed_decode(use_graph=False, reuse_query_kv=True)
    calls = []
    orig = orch.decoder.continue_hidden
    orch.decoder.continue_hidden = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    a1, ids1, c1 = orch.design_hidden(prompt, mask, None, **kw)
    assert calls == [] and a0.shape[1] == 14
    assert torch.equal(a0, a1) and torch.equal(ids0, ids1) and torch.equal(c0, c1)
