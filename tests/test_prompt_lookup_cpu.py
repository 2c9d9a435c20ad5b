"""Prompt-lookup speculative decoding on the eager static-cache decoder and the torch step (CPU, f32): the drafting rule is HF's
PromptLookupCandidateGenerator.get_candidates, greedy tokens are HF generate's (plain and with prompt_lookup_num_tokens), the statistics
are those of a replay of HF's candidate generator over the returned sequence, an EOS inside an accepted run ends the output there,
sampled tokens lie in HF's kept set, continue_hidden works as after a plain generate, and the options are validated and plumbed."""
import pytest
import torch

from llamole_amd import e2e, llm_spec
from llamole_amd.llm_decode import GraphedDecoder

MODELS = ["tiny", "tiny-llama", "tiny-qwen3"]
KN = [(2, 1), (4, 2), (7, 3), (15, 2)]
MAX_NEW = 48
KW = dict(max_new_tokens=MAX_NEW, do_sample=False, eos_token_id=[2047], pad_token_id=0)
_llms, _plain = {}, {}


def _case(name):
    if name not in _llms:
        _llms[name] = e2e.build_llm(name, "cpu", torch.float32)
    prompt = torch.randint(5, 1000, (1, 12), generator=torch.Generator().manual_seed(0))
    return _llms[name], prompt, torch.ones_like(prompt)


def _hf_plain(name):
    """HF generate greedy, computed once per model and left unchanged."""
    if name not in _plain:
        llm, prompt, mask = _case(name)
        _plain[name] = llm.generate(inputs=prompt, attention_mask=mask, **KW)
    return _plain[name]


def _hf_drafts(history, k, n):
    """HF's candidates for a history (max_length out of reach, no EOS trimming)."""
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    gen = PromptLookupCandidateGenerator(eos_token_id=None, num_output_tokens=k, max_matching_ngram_size=n, max_length=10 ** 9)
    ids = torch.tensor([list(history)], dtype=torch.long)
    return gen.get_candidates(ids)[0][0, len(history):].tolist()


def replay(prompt_row, new_tokens, k, n, eos=(), drafts=_hf_drafts):
    """(forwards, accepted, steps) needed to reproduce ``new_tokens`` with HF's candidate generator as the drafter and the step of
    llm_spec.py: per step the forwarded rows are [last, drafts.., last..], the emitted tokens the longest agreeing run plus one, cut at
    EOS and at the end.  steps = [(index of the first token the step emits, number emitted)]."""
    history = list(prompt_row) + [new_tokens[0]]
    i, forwards, accepted, steps = 1, 0, 0, []
    while i < len(new_tokens) and new_tokens[i - 1] not in eos:
        d = drafts(history, k, n)
        rows = [new_tokens[i - 1]] + d + [new_tokens[i - 1]] * (k - len(d))
        e = 0
        while True:
            t = new_tokens[i + e]
            e += 1
            if t in eos or i + e >= len(new_tokens) or e > k or rows[e] != t:
                break
        steps.append((i, e))
        history += new_tokens[i:i + e]
        i += e
        forwards += 1
        accepted += e - 1
    return forwards, accepted, steps


@pytest.mark.parametrize("k,n", KN)
def test_draft_rule_equals_hf_get_candidates(k, n):
    g = torch.Generator().manual_seed(100 * k + n)
    seen = {"none": 0, "short": 0, "full": 0, "n_larger": 0}
    for L in range(2, 41):
        for _ in range(6):
            h = torch.randint(0, 4, (L,), generator=g).tolist()
            want = _hf_drafts(h, k, n)
            assert llm_spec.draft(h, k, n) == want, (h, k, n)
            rows = llm_spec.draft_rows(h, h[-1], k, n)
            assert rows == [h[-1]] + want + [h[-1]] * (k - len(want))
            seen["none" if not want else ("short" if len(want) < k else "full")] += 1
            seen["n_larger"] += n > L - 1
    # no match at all: distinct tokens; n larger than the history: a two-token history under n = 3
    assert llm_spec.draft(list(range(20)), k, n) == _hf_drafts(list(range(20)), k, n) == []
    assert llm_spec.draft([3, 3], k, 3) == _hf_drafts([3, 3], k, 3) == [3]
    assert llm_spec.draft([3], k, n) == [] and llm_spec.draft([], k, n) == []
    assert seen["short"] and seen["full"] and (seen["none"] or k > 2), seen
    assert seen["n_larger"] or n == 1, seen


@pytest.mark.parametrize("name", MODELS)
def test_hf_own_two_paths_agree(name):
    llm, prompt, mask = _case(name)
    assert torch.equal(llm.generate(inputs=prompt, attention_mask=mask, prompt_lookup_num_tokens=4, max_matching_ngram_size=2, **KW),
                       _hf_plain(name))


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("k,n", KN)
def test_greedy_tokens_and_statistics(name, k, n):
    llm, prompt, mask = _case(name)
    want = _hf_plain(name)
    dec = GraphedDecoder(llm, use_graph=False)
    got = dec.generate(prompt, mask, prompt_lookup_num_tokens=k, max_matching_ngram_size=n, **KW)
    assert torch.equal(got, want)
    new = got[0, 12:].tolist()
    forwards, accepted, _ = replay(prompt[0].tolist(), new, k, n, eos=(2047,))
    assert dec.spec_stats == {"forwards": forwards, "accepted": accepted, "tokens": len(new)} and dec._last["n_new"] == len(new)
    if 2047 not in new:
        assert len(new) == MAX_NEW == forwards + accepted + 1
    if (k, n) == (4, 2):
        hf_accepted = {"tiny": 19, "tiny-llama": 16, "tiny-qwen3": 9}[name]       # HF's generator at k = 4, n = 2 on this prompt
        assert accepted >= hf_accepted > 0, (accepted, hf_accepted)                 # (the repeated last token may be accepted on top)
    assert accepted > 0


@pytest.mark.parametrize("name", MODELS)
def test_eos_inside_an_accepted_run(name):
    """An EOS ends generation at its FIRST occurrence among the new tokens, and a draft is a copy of the history: an accepted draft can
    be that first occurrence only if it copies the prompt.  A random prompt never gets its bigrams repeated by these models, so the call's
    prompt is the 12 tokens plus the first m tokens of the model's own greedy continuation (the smallest m that gives such a case), whose
    repetitions the rest of the continuation then copies."""
    llm, prompt, mask = _case(name)
    all_new = _hf_plain(name)[0, 12:].tolist()
    found = None
    for m in range(1, MAX_NEW - 4):
        head, new = prompt[0].tolist() + all_new[:m], all_new[m:]
        _, _, steps = replay(head, new, 4, 2)
        # an accepted draft in the middle of a step (neither the step's first nor its last token) whose value did not occur earlier
        picks = [(i, e, i + j) for i, e in steps if e >= 3 for j in range(1, e - 1) if new[i + j] not in new[:i + j]]
        if picks:
            found = (m, new, picks[0])
            break
    assert found, "no accepted draft that is the first occurrence of its token"
    m, new, (i, e, at) = found
    p2 = torch.tensor([prompt[0].tolist() + all_new[:m]])
    kw = dict(KW, eos_token_id=[new[at]], max_new_tokens=MAX_NEW - m)
    want = llm.generate(inputs=p2, attention_mask=torch.ones_like(p2), **kw)
    dec = GraphedDecoder(llm, use_graph=False)
    got = dec.generate(p2, torch.ones_like(p2), prompt_lookup_num_tokens=4, max_matching_ngram_size=2, **kw)
    assert torch.equal(got, want) and got.shape[1] == 12 + m + at + 1 and int(got[0, -1]) == new[at]
    assert got[0, 12 + m:].tolist() == new[:at + 1]
    f, a, cut = replay(p2[0].tolist(), new[:at + 1], 4, 2, eos=(new[at],))
    assert cut[-1] == (i, at - i + 1) and at - i + 1 < e            # the step that would have emitted e tokens ends at the EOS
    assert dec.spec_stats == {"forwards": f, "accepted": a, "tokens": at + 1}


def test_max_new_tokens_cuts_a_run():
    llm, prompt, mask = _case("tiny")
    want = _hf_plain("tiny")
    for m in (1, 2, 7, 20):
        dec = GraphedDecoder(llm, use_graph=False)
        got = dec.generate(prompt, mask, prompt_lookup_num_tokens=7, **dict(KW, max_new_tokens=m))
        assert torch.equal(got, want[:, :12 + m]) and dec.spec_stats["tokens"] == m == dec._last["n_new"]


def _hf_kept(logits, temperature, top_k, top_p):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = logits.clone()
    for proc in (TemperatureLogitsWarper(temperature), TopKLogitsWarper(top_k), TopPLogitsWarper(top_p)):
        s = proc(None, s)
    return torch.isfinite(s)


@pytest.mark.parametrize("temperature,top_k,top_p", [(0.6, 50, 0.9), (1.0, 0, 0.8)])
def test_sampling_stays_in_hf_kept_set_and_reproduces(temperature, top_k, top_p):
    llm, prompt, mask = _case("tiny")
    kw = dict(max_new_tokens=24, do_sample=True, temperature=temperature, top_k=top_k, top_p=top_p, eos_token_id=[2047], pad_token_id=0,
              prompt_lookup_num_tokens=4)
    dec = GraphedDecoder(llm, use_graph=False)
    a = dec.generate(prompt, mask, generator=torch.Generator().manual_seed(7), **kw)
    b = dec.generate(prompt, mask, generator=torch.Generator().manual_seed(7), **kw)
    assert torch.equal(a, b)
    with torch.no_grad():
        logits = llm(input_ids=a, use_cache=False).logits[0].float()
    V = logits.shape[1]
    for t in range(12, a.shape[1]):
        kept = _hf_kept(logits[t - 1:t], temperature, top_k if top_k else V, top_p)
        assert bool(kept[0, a[0, t]]), t


@pytest.mark.parametrize("name", MODELS)
def test_continue_hidden_after_a_speculative_call(name):
    llm, prompt, mask = _case(name)
    tail = torch.randint(5, 1000, (1, 4), generator=torch.Generator().manual_seed(3))
    hid = {}
    for k in (None, 4):
        dec = GraphedDecoder(llm, use_graph=False)
        out = dec.generate(prompt, mask, prompt_lookup_num_tokens=k, **KW)
        assert dec._last["n_new"] == MAX_NEW and out.shape[1] == 12 + MAX_NEW
        hid[k] = dec.continue_hidden(tail, 12 + MAX_NEW - 1).float().clone()
    err = float((hid[None] - hid[4]).abs().max() / hid[None].abs().max())
    assert err <= 3e-2, err


def test_inputs_embeds_call_starts_from_an_empty_history():
    llm, prompt, mask = _case("tiny")
    emb = llm.get_input_embeddings()(prompt)
    want = llm.generate(inputs_embeds=emb, attention_mask=mask, **KW)
    dec = GraphedDecoder(llm, use_graph=False)
    got = dec.generate(None, mask, inputs_embeds=emb, prompt_lookup_num_tokens=4, **KW)
    assert torch.equal(got, want)
    new = got[0].tolist()
    f, a, _ = replay([], new, 4, 2, eos=(2047,))
    assert dec.spec_stats == {"forwards": f, "accepted": a, "tokens": len(new)}


def test_validation():
    llm, prompt, mask = _case("tiny")
    dec = GraphedDecoder(llm, use_graph=False)
    kw = dict(max_new_tokens=4, do_sample=False, pad_token_id=0)
    two = torch.cat([prompt, prompt])
    with pytest.raises(ValueError, match="batch of 1"):
        dec.generate(two, torch.ones_like(two), prompt_lookup_num_tokens=4, **kw)
    with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens together with num_beams"):
        dec.generate(prompt, mask, prompt_lookup_num_tokens=4, num_beams=2, **kw)
    with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens together with repetition_penalty"):
        dec.generate(prompt, mask, prompt_lookup_num_tokens=4, repetition_penalty=1.2, **kw)
    for bad in (1, 16, -3, 2.0, "4", True):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
            dec.generate(prompt, mask, prompt_lookup_num_tokens=bad, **kw)
    for bad in (0, -1, 1.5, "2", False):
        with pytest.raises(ValueError, match="max_matching_ngram_size"):
            dec.generate(prompt, mask, prompt_lookup_num_tokens=4, max_matching_ngram_size=bad, **kw)
    for off in (None, 0):
        with pytest.raises(ValueError, match="without `prompt_lookup_num_tokens`"):
            dec.generate(prompt, mask, prompt_lookup_num_tokens=off, max_matching_ngram_size=2, **kw)
    assert llm_spec.check_prompt_lookup(None, None) is None and llm_spec.check_prompt_lookup(0, None) is None
    assert llm_spec.check_prompt_lookup(2, None) == (2, 2) and llm_spec.check_prompt_lookup(15, 5) == (15, 5)


def test_option_off_is_the_plain_path(monkeypatch):
    """absent, None and 0: no function of the speculative path is entered."""
    llm, prompt, mask = _case("tiny")
    want = _hf_plain("tiny")

    def boom(*a, **k):
        raise AssertionError("speculative path entered with the option off")
    monkeypatch.setattr(GraphedDecoder, "_generate_spec_torch", boom)
    monkeypatch.setattr(GraphedDecoder, "_generate_spec", boom)
    monkeypatch.setattr(GraphedDecoder, "_spec_forward", boom)
    for extra in ({}, {"prompt_lookup_num_tokens": None}, {"prompt_lookup_num_tokens": 0}):
        dec = GraphedDecoder(llm, use_graph=False)
        assert torch.equal(dec.generate(prompt, mask, **KW, **extra), want) and dec.spec_stats is None
        assert dec.mask.shape[1] == 64          # no slack slots either: the bucket of 12 + 48


def test_environment_switch(monkeypatch):
    llm, prompt, mask = _case("tiny")
    monkeypatch.setenv("LLAMOLE_PROMPT_LOOKUP", "4")
    dec = GraphedDecoder(llm, use_graph=False)
    assert torch.equal(dec.generate(prompt, mask, **KW), _hf_plain("tiny")) and dec.spec_stats["accepted"] > 0
    two = torch.cat([prompt, prompt])           # a call that cannot take it runs the plain path
    dec2 = GraphedDecoder(llm, use_graph=False)
    dec2.generate(two, torch.ones_like(two), **dict(KW, max_new_tokens=4))
    assert dec2.spec_stats is None


def test_yaml_keys_survive_load_yaml_args(tmp_path):
    from llamole_amd.eval import load_yaml_args
    p = tmp_path / "gen.yaml"
    p.write_text("model_name_or_path: x\nprompt_lookup_num_tokens: 5\nmax_matching_ngram_size: 3\n")
    gen = load_yaml_args(str(p))[4].to_dict()
    assert gen["prompt_lookup_num_tokens"] == 5 and gen["max_matching_ngram_size"] == 3
    q = tmp_path / "plain.yaml"
    q.write_text("model_name_or_path: x\n")
    gen = load_yaml_args(str(q))[4].to_dict()
    assert "prompt_lookup_num_tokens" not in gen and "max_matching_ngram_size" not in gen


def test_graph_llm_generate_accepts_the_option():
    from llamole_amd.modeling_llamole import GraphLLMForCausalMLM
    llm, prompt, mask = _case("tiny")
    m = GraphLLMForCausalMLM.__new__(GraphLLMForCausalMLM)
    torch.nn.Module.__init__(m)
    m.language_model = llm
    m.decoder = GraphedDecoder(llm, use_graph=False)
    kw = dict(KW, prompt_lookup_num_tokens=4, max_matching_ngram_size=2)
    assert torch.equal(m._llm_generate(inputs=prompt, attention_mask=mask, **kw), _hf_plain("tiny"))
    assert m.decoder.spec_stats["accepted"] > 0
    m.decoder = None                            # the llm_decode='hf' path: HF takes the same options unchanged
    assert torch.equal(m._llm_generate(inputs=prompt, attention_mask=mask, **kw), _hf_plain("tiny"))
