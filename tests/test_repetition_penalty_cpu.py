"""repetition_penalty on the eager static-cache decoder and the torch sampler (CPU): HF RepetitionPenaltyLogitsProcessor semantics."""
import pytest
import torch

from llamole_amd import e2e
from llamole_amd.llm_decode import GraphedDecoder, apply_repetition_penalty, sample_top_p


def _case(name):
    llm = e2e.build_llm(name, "cpu", torch.float32)
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(5, 1000, (2, 12), generator=g)
    mask = torch.ones_like(prompt)
    mask[1, :4] = 0
    prompt[1, :4] = 0                     # left pads (pad id 0): penalised too, as HF does
    return llm, prompt, mask


@pytest.mark.parametrize("name", ["tiny", "tiny-llama"])
@pytest.mark.parametrize("p", [1.3, 0.7])
def test_greedy_equals_hf_generate_with_penalty(name, p):
    llm, prompt, mask = _case(name)
    kw = dict(max_new_tokens=12, do_sample=False, pad_token_id=0, eos_token_id=[2047], repetition_penalty=p)
    ref = llm.generate(inputs=prompt, attention_mask=mask, **kw)
    got = GraphedDecoder(llm, use_graph=False).generate(prompt, mask, **kw)
    assert torch.equal(ref, got)
    # inputs_embeds: only the tokens generated in the call are penalised
    emb = llm.get_input_embeddings()(prompt)
    ref_e = llm.generate(inputs_embeds=emb, attention_mask=mask, **kw)
    got_e = GraphedDecoder(llm, use_graph=False).generate(None, mask, inputs_embeds=emb, **kw)
    assert torch.equal(ref_e, got_e)
    # the first token is an EOS for row 0: the rest of the row is padding, in both
    first = int(ref[0, 12])
    kw2 = dict(kw, eos_token_id=[first])
    ref2 = llm.generate(inputs=prompt, attention_mask=mask, **kw2)
    got2 = GraphedDecoder(llm, use_graph=False, sync_every=1).generate(prompt, mask, **kw2)
    assert torch.equal(ref2[:, :got2.shape[1]], got2) and (got2[0, 13:] == 0).all()


def test_penalty_changes_a_looping_greedy_decode():
    llm, prompt, mask = _case("tiny")
    kw = dict(max_new_tokens=12, do_sample=False, pad_token_id=0, eos_token_id=[2047])
    plain = GraphedDecoder(llm, use_graph=False).generate(prompt, mask, **kw)
    pen = GraphedDecoder(llm, use_graph=False).generate(prompt, mask, repetition_penalty=1.3, **kw)
    assert not torch.equal(plain, pen)
    same = GraphedDecoder(llm, use_graph=False).generate(prompt, mask, repetition_penalty=1.0, **kw)
    assert torch.equal(plain, same)


def _hf_kept(logits, ids, p, temperature, top_k, top_p):
    from transformers.generation.logits_process import (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper,
                                                        TopKLogitsWarper, TopPLogitsWarper)
    s = logits.clone()
    for proc in (RepetitionPenaltyLogitsProcessor(p), TemperatureLogitsWarper(temperature), TopKLogitsWarper(top_k),
                 TopPLogitsWarper(top_p)):
        s = proc(ids, s)
    return torch.isfinite(s)


@pytest.mark.parametrize("p,temperature,top_k,top_p", [(1.3, 0.6, 50, 0.9), (0.7, 1.0, 7, 0.5), (2.0, 0.8, 0, 0.95)])
def test_torch_sampler_keeps_hf_set(p, temperature, top_k, top_p):
    g = torch.Generator().manual_seed(1)
    B, V = 6, 500
    logits = (torch.randn(B, V, generator=g) * 3).to(torch.bfloat16).float()
    ids = torch.randint(0, V, (B, 40), generator=g)
    kept = _hf_kept(logits, ids, p, temperature, top_k if top_k else V, top_p)
    draws = torch.stack([sample_top_p(logits, temperature, top_p, g, top_k or None, repetition_penalty=p, penalty_ids=ids)
                         for _ in range(300)], dim=1)
    assert bool(kept.gather(1, draws).all())
    # every kept token is reachable: the penalised row is HF's processed row
    ref = logits.clone()
    s = ref.gather(1, ids)
    ref.scatter_(1, ids, torch.where(s < 0, s * p, s / p))
    assert torch.equal(apply_repetition_penalty(logits, ids, p), ref)


@pytest.mark.parametrize("bad", [0.0, -1.2, float("nan"), "x", 2])
def test_non_positive_penalty_raises(bad):
    llm, prompt, mask = _case("tiny")
    with pytest.raises(ValueError):
        GraphedDecoder(llm, use_graph=False).generate(prompt, mask, max_new_tokens=2, do_sample=False, repetition_penalty=bad)


def test_beam_search_stays_rejected():
    llm, prompt, mask = _case("tiny")
    with pytest.raises(NotImplementedError):
        GraphedDecoder(llm, use_graph=False).generate(prompt, mask, max_new_tokens=2, do_sample=False, repetition_penalty=1.2,
                                                      num_beams=2)


def test_graph_llm_generate_accepts_the_option():
    from llamole_amd.modeling_llamole import GraphLLMForCausalMLM
    llm, prompt, mask = _case("tiny")
    m = GraphLLMForCausalMLM.__new__(GraphLLMForCausalMLM)
    torch.nn.Module.__init__(m)
    m.language_model = llm
    m.decoder = GraphedDecoder(llm, use_graph=False)
    kw = dict(max_new_tokens=6, do_sample=False, pad_token_id=0, eos_token_id=[2047], repetition_penalty=1.3)
    got = m._llm_generate(inputs=prompt, attention_mask=mask, **kw)
    assert torch.equal(got, llm.generate(inputs=prompt, attention_mask=mask, **kw))


def test_validation_follows_hf():
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    from llamole_amd.llm_decode import check_repetition_penalty
    for bad in (2, 0.0, -1.5, float("nan")):
        with pytest.raises(ValueError):
            RepetitionPenaltyLogitsProcessor(bad)
        with pytest.raises(ValueError):
            check_repetition_penalty(bad)
    assert check_repetition_penalty(None) is None and check_repetition_penalty(1) is None and check_repetition_penalty(1.0) is None
    assert check_repetition_penalty(1.3) == 1.3
