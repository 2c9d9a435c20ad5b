"""Beam search on the device: the KV reorder (ll_beam_kv_reorder_bf16) against index_select, the beam step (ll_beam_step_bf16)
against the torch step of llm_beam.py, the beam-sample distribution, and the graphed decoder end to end."""
import itertools
import math

import numpy as np
import pytest
import torch

from llamole_amd.llm_beam import BeamParams, BeamState, beam_step_torch, beams_to_keep, state_layout

pytestmark = pytest.mark.gpu


def _lib():
    from llamole_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("D,nkv,maxlen,B,nb", [(64, 1, 64, 1, 2), (128, 2, 256, 3, 4), (128, 8, 1024, 2, 8), (64, 4, 128, 6, 3),
                                               (128, 4, 512, 1, 16)])
def test_kv_reorder_matches_index_select(D, nkv, maxlen, B, nb):
    lib = _lib()
    g = torch.Generator(device="cuda").manual_seed(D + nkv + B)
    R = B * nb
    ts = [torch.randn(R, nkv, maxlen, D, device="cuda", generator=g).to(torch.bfloat16) for _ in range(3)]
    ptrs = torch.tensor([x.data_ptr() for x in ts], dtype=torch.int64, device="cuda")
    par = []
    for b in range(B):
        kind = b % 3
        p = list(range(nb)) if kind == 0 else ([nb - 1] * nb if kind == 1 else torch.randint(0, nb, (nb,), generator=torch.Generator().manual_seed(b)).tolist())
        par += [b * nb + j for j in p]
    par = torch.tensor(par, dtype=torch.int32, device="cuda")
    for first, hi, from0 in ((0, maxlen // 3, 1), (maxlen // 4, maxlen - 5, 0), (5, maxlen, 0)):
        ref = [x.clone() for x in ts]
        for r, x in zip(ref, ts):
            idx = (torch.arange(R, device="cuda") // nb * nb) if from0 else par.long()
            r[:, :, first:hi] = x.index_select(0, idx)[:, :, first:hi]
        pos = torch.tensor([hi], dtype=torch.int64, device="cuda")
        first_dev = torch.tensor([first], dtype=torch.int64, device="cuda")
        assert lib.ll_beam_kv_reorder_bf16(ptrs.data_ptr(), len(ts), B, nb, nkv, maxlen, D, par.data_ptr(), first_dev.data_ptr(), from0,
                                           pos.data_ptr(), None) == 0
        torch.cuda.synchronize()
        for r, x in zip(ref, ts):
            assert torch.equal(r.view(torch.int16), x.view(torch.int16))      # slots outside [first, hi) and identity items untouched


def _state(B, nb, K, T, dev):
    st = BeamState(torch.zeros(state_layout(B, nb, K, T)[1], dtype=torch.uint8, device=dev), B, nb, K, T)
    st.reset()
    return st


def _hip_step(lib, logits, st, p, tok, seed):
    es = 2 if p.early_stopping == "never" else int(p.early_stopping is True)
    eos = p.eos.cuda().contiguous()
    inv = float(np.float32(1.0) / np.float32(p.temperature))
    rc = lib.ll_beam_step_bf16(logits.data_ptr(), logits.stride(0), p.B, p.nb, logits.shape[1], p.K, p.T, st.buf.data_ptr(), st.buf.numel(),
                               eos.data_ptr(), eos.numel(), p.max_new, p.length_penalty, es, int(p.do_sample), inv, p.top_k, p.top_p,
                               seed.data_ptr(), tok.data_ptr(), None, None, 0, None)
    assert rc == 0


@pytest.mark.parametrize("V", [2048, 32768, 128256, 152064])
@pytest.mark.parametrize("nb", [2, 4, 8])
@pytest.mark.parametrize("n_eos", [1, 10])
def test_beam_step_matches_torch_step(V, nb, n_eos):
    lib = _lib()
    B, T, max_new = 3, 16, 12
    K = beams_to_keep(nb, n_eos)
    g = torch.Generator(device="cuda").manual_seed(V + nb + n_eos)
    logits = (torch.randn(B * nb, V, device="cuda", generator=g) * 4).to(torch.bfloat16)
    # EOS ids among the strongest tokens, so that hits and finished hypotheses occur
    top = logits.float().topk(3, dim=-1).indices
    eos = torch.unique(top[:, 1].flatten())[:n_eos].cpu()
    eos = torch.cat([eos, torch.arange(V - (n_eos - eos.numel()), V)])[:n_eos]
    seed = torch.zeros(1, dtype=torch.long, device="cuda")
    for lp, es in ((1.0, False), (0.6, True), (-1.0, "never")):
        p = BeamParams(B, nb, K, T, max_new, eos, lp, es, False, 1.0, 0, 1.0)
        for t in (0, 5, max_new - 1):
            st = _state(B, nb, K, T, "cuda")
            if t:
                gg = torch.Generator(device="cuda").manual_seed(t)
                st.run.copy_(-torch.rand(B * nb, device="cuda", generator=gg) * 10)
                st.hyp.copy_(-torch.rand(B * nb, device="cuda", generator=gg) * 3 - 1)
                st.hyp.view(B, nb)[0] = -1e9
                st.fin.view(B, nb)[1:] = 1
                st.hyp_t.view(B, nb)[1:] = 2
                f = st.flags.view(B, 8)
                f[:, 3] = t
                f[:, 4 * (t & 1)] = 1
            a, b = BeamState(st.buf.clone(), B, nb, K, T), BeamState(st.buf.clone(), B, nb, K, T)
            ref_tok = beam_step_torch(logits, a, t, p)
            tok = torch.zeros(B * nb, dtype=torch.long, device="cuda")
            _hip_step(lib, logits, b, p, tok, seed)
            torch.cuda.synchronize()
            assert torch.equal(tok, ref_tok), (lp, es, t)
            for name in ("fin", "hyp_t", "hyp_beam", "hyp_tok", "flags", "par", "rtok", "rpar"):
                assert torch.equal(getattr(a, name), getattr(b, name)), (name, lp, es, t)
            # scores: 1e-6 relative, or 1e-6 absolute where a score is small next to the log-sum-exp its rounding comes from
            for name in ("run", "hyp"):
                torch.testing.assert_close(getattr(b, name), getattr(a, name), rtol=1e-6, atol=1e-6)


def test_beam_sample_distribution():
    """4000 items with the same logits at step 0 (beam 1 at -1e9): the K = 4 continuations of beam 0 are K draws without replacement
    from the kept set -- the frequency of each set within 4.5 sigma of its Plackett-Luce probability; removed tokens never drawn."""
    lib = _lib()
    B, nb, V, T = 4000, 2, 8, 4
    n_eos, K = 1, 4
    x = torch.tensor([2.0, 1.5, 1.0, 0.75, 0.5, 0.0, -3.0, -4.0])
    logits = x.to(torch.bfloat16).cuda().repeat(B * nb, 1).contiguous()
    p = BeamParams(B, nb, K, T, 4, torch.tensor([7]), 1.0, False, True, 0.8, 6, 1.0)
    st = _state(B, nb, K, T, "cuda")
    seed = torch.tensor([12345], dtype=torch.long, device="cuda")
    tok = torch.zeros(B * nb, dtype=torch.long, device="cuda")
    _hip_step(lib, logits, st, p, tok, seed)
    torch.cuda.synchronize()
    cand = st.cand.view(B, nb, K, 3)[:, 0, :, 2].cpu().long() % V              # row 0 of each item: its K draws
    assert int(cand.max()) < 6                                                # top-k 6: tokens 6 and 7 removed
    sets = [tuple(sorted(r)) for r in cand.tolist()]
    assert all(len(set(s)) == K for s in sets)
    w = np.exp(x.double().numpy()[:6] / 0.8)
    w = w / w.sum()
    for S in itertools.combinations(range(6), K):
        prob = 0.0
        for order in itertools.permutations(S):
            pr, left = 1.0, 1.0
            for i in order:
                pr *= w[i] / left
                left -= w[i]
            prob += pr
        n = sum(1 for s in sets if s == S)
        sigma = math.sqrt(B * prob * (1 - prob))
        assert abs(n - B * prob) <= 4.5 * sigma + 1e-9, (S, n, B * prob)


def _accel_case(name, B=2, P=12):
    from llamole_amd import e2e
    from llamole_amd.llm_accel import accelerate_llm
    llm = e2e.build_llm(name, "cuda", torch.bfloat16)
    accelerate_llm(llm)
    g = torch.Generator().manual_seed(B)
    prompt = torch.randint(5, 1000, (B, P), generator=g)
    mask = torch.ones_like(prompt)
    mask[1, :4] = 0
    prompt[1, :4] = 0
    return llm, prompt.cuda(), mask.cuda()


def _spy(monkeypatch):
    from llamole_amd.llm_decode import GraphedDecoder
    calls = []
    orig = GraphedDecoder._hip_beam

    def spy(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)
    monkeypatch.setattr(GraphedDecoder, "_hip_beam", spy)
    return calls


@pytest.mark.parametrize("name", ["tiny", "tiny-llama"])
def test_graphed_eager_torch_identical(name, monkeypatch):
    from llamole_amd.llm_decode import GraphedDecoder
    calls = _spy(monkeypatch)
    llm, prompt, mask = _accel_case(name)
    for kw in (dict(do_sample=False, num_beams=4, length_penalty=0.8), dict(do_sample=False, num_beams=2, early_stopping=True),
               dict(do_sample=False, num_beams=3, early_stopping="never", length_penalty=-1.0)):
        kw.update(max_new_tokens=20, pad_token_id=0, eos_token_id=[2047, 7, 11])
        a = GraphedDecoder(llm, use_graph=True).generate(prompt, mask, **kw)
        b = GraphedDecoder(llm, use_graph=False).generate(prompt, mask, **kw)
        c = GraphedDecoder(llm, use_graph=True, sampler="torch").generate(prompt, mask, **kw)
        assert torch.equal(a, b) and torch.equal(a, c), (kw, a, b, c)
    assert calls
    # beam sample: graphed and eager give the same tokens for one seed, and a reseeded call reproduces them
    kw = dict(do_sample=True, temperature=0.6, top_p=0.9, top_k=50, num_beams=4, max_new_tokens=20, pad_token_id=0, eos_token_id=[2047])
    dec = GraphedDecoder(llm, use_graph=True)
    a = dec.generate(prompt, mask, generator=torch.Generator(device="cuda").manual_seed(1), **kw)
    a2 = dec.generate(prompt, mask, generator=torch.Generator(device="cuda").manual_seed(1), **kw)
    b = GraphedDecoder(llm, use_graph=False).generate(prompt, mask, generator=torch.Generator(device="cuda").manual_seed(1), **kw)
    assert torch.equal(a, a2) and torch.equal(a, b)


def _hf_kept(logits, temperature, top_k, top_p, min_keep):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = torch.log_softmax(logits.float(), dim=-1)
    s = TemperatureLogitsWarper(temperature)(None, s)
    s = TopKLogitsWarper(top_k, min_tokens_to_keep=min_keep)(None, s)
    s = TopPLogitsWarper(top_p, min_tokens_to_keep=min_keep)(None, s)
    return torch.isfinite(s)


@pytest.mark.parametrize("temperature,top_k,top_p,n_eos", [(0.6, 50, 0.9, 10), (1.0, 20, 0.5, 10), (0.8, 30, 0.3, 1), (0.6, 50, 0.9, 3)])
def test_beam_sample_top_p_keeps_hf_set(temperature, top_k, top_p, n_eos):
    """HIP beam sample with top_p < 1: every row's drawn candidates lie in HF's Temperature -> TopK -> TopP kept set (min_tokens_to_keep
    = n_eos + 1), as many as it holds (up to K), and so do the running beams the merge picks."""
    lib = _lib()
    B, nb, V, T, t = 3, 4, 2048, 16, 3
    K = beams_to_keep(nb, n_eos)
    g = torch.Generator(device="cuda").manual_seed(top_k + n_eos)
    logits = (torch.randn(B * nb, V, device="cuda", generator=g) * 3).to(torch.bfloat16)
    kept = _hf_kept(logits.cpu(), temperature, top_k, top_p, n_eos + 1)
    p = BeamParams(B, nb, K, T, 12, torch.arange(V - n_eos, V), 1.0, False, True, temperature, top_k, top_p)
    for seed in range(5):
        st = _state(B, nb, K, T, "cuda")
        st.run.copy_(-torch.rand(B * nb, device="cuda", generator=g))          # a middle step: every beam live
        f = st.flags.view(B, 8)
        f[:, 3] = t
        f[:, 4 * (t & 1)] = 1
        tok = torch.zeros(B * nb, dtype=torch.long, device="cuda")
        _hip_step(lib, logits, st, p, tok, torch.tensor([seed], dtype=torch.long, device="cuda"))
        torch.cuda.synchronize()
        cand = st.cand.view(B * nb, K, 3).cpu()
        for r in range(B * nb):
            finite = torch.isfinite(cand[r, :, 1].view(torch.float32))
            toks = cand[r, :, 2].long()[finite] - (r % nb) * V
            # HF's sort leaves the order of equal values open: a token outside its kept set is admissible only when tied with the
            # kept set's lowest value (the kernel removes the lower-indexed of equal tokens first, as a stable ascending sort does)
            edge = logits[r].cpu()[kept[r]].float().min()
            assert bool((kept[r, toks] | (logits[r].cpu()[toks].float() == edge)).all()), r
            assert int(finite.sum()) == min(K, int(kept[r].sum())), r
            assert len(set(toks.tolist())) == toks.numel()
        par, tk = st.par.long().cpu(), tok.cpu()
        edge = torch.stack([logits[r].cpu()[kept[r]].float().min() for r in range(B * nb)])
        assert bool((kept[par, tk] | (logits.cpu()[par, tk].float() == edge[par])).all())


@pytest.mark.parametrize("name", ["tiny", "tiny-llama"])
def test_greedy_beam_equals_hf_generate(name):
    """Greedy beam search on the accelerated model against HF generate(num_beams) on the same model, B = 2.  Where a row differs, the
    two best hypotheses must be a near-tie: their scores within 1e-5 relative."""
    from llamole_amd.llm_decode import GraphedDecoder
    llm, prompt, mask = _accel_case(name)
    for nb, lp, es in ((2, 1.0, False), (4, 0.8, True), (3, -1.0, "never")):
        kw = dict(do_sample=False, num_beams=nb, length_penalty=lp, early_stopping=es, max_new_tokens=16, pad_token_id=0,
                  eos_token_id=[2047, 7, 11])
        ref = llm.generate(inputs=prompt, attention_mask=mask, return_dict_in_generate=True, output_scores=True, **kw)
        dec = GraphedDecoder(llm, use_graph=True)
        got = dec.generate(prompt, mask, **kw)
        ours = dec._beam_state.hyp.view(2, nb)[:, 0].cpu()
        hf = ref.sequences_scores.float().cpu()
        w = max(ref.sequences.shape[1], got.shape[1])
        pad = lambda x: torch.nn.functional.pad(x, (0, w - x.shape[1]), value=-7)       # noqa: E731
        for b in range(2):
            if not torch.equal(pad(ref.sequences)[b], pad(got)[b]):
                assert abs(float(ours[b]) - float(hf[b])) <= 1e-5 * abs(float(hf[b])), (name, nb, b, float(ours[b]), float(hf[b]))


def test_decoder_reused_across_prompt_lengths(monkeypatch):
    """One graphed decoder, calls of different prompt lengths (and EOS counts) in one cache bucket: the captured step reads the call's
    prompt length from the device, so every call equals a fresh decoder's."""
    from llamole_amd.llm_decode import GraphedDecoder
    calls = _spy(monkeypatch)
    llm, prompt, mask = _accel_case("tiny", P=20)
    dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
    cases = [(prompt, mask, [2047]), (prompt[:, 8:], mask[:, 8:], [2047]), (prompt[:, 3:], mask[:, 3:], []), (prompt[:, 8:], mask[:, 8:], [7])]
    for pr, ms, eos in cases:
        kw = dict(do_sample=False, num_beams=4, max_new_tokens=20, pad_token_id=0, eos_token_id=eos)
        a = dec.generate(pr, ms, **kw)
        b = GraphedDecoder(llm, use_graph=True, fused_cache=True).generate(pr, ms, **kw)
        c = GraphedDecoder(llm, use_graph=False, fused_cache=True).generate(pr, ms, **kw)
        assert torch.equal(a, b) and torch.equal(a, c), (pr.shape, eos)
    assert calls


@pytest.mark.parametrize("B", [6, 16])
def test_rows_17_to_64(B, monkeypatch):
    """B * nb = 24 / 64 rows: the seven-launch layers (ll_linear_rows64_bf16) and the HIP beam step in the captured step."""
    from llamole_amd import e2e
    from llamole_amd.llm_accel import (accelerate_elementwise, accelerate_linears, fuse_decoder_layers, fuse_model_decode,
                                       restore_decoder_layers, restore_elementwise, restore_linears, restore_model_decode,
                                       use_decode_attention)
    from llamole_amd.llm_decode import GraphedDecoder
    calls = _spy(monkeypatch)
    llm = e2e.build_llm("tiny", "cuda", torch.bfloat16)
    g = torch.Generator().manual_seed(B)
    prompt = torch.randint(5, 1000, (B, 10), generator=g).cuda()
    mask = torch.ones_like(prompt)
    mask[1, :4] = 0
    prompt[1, :4] = 0
    kw = dict(do_sample=False, num_beams=4, max_new_tokens=12, pad_token_id=0, eos_token_id=[2047, 7])
    try:
        assert accelerate_linears(llm, min_weight_elems=1) > 0
        accelerate_elementwise(llm)
        assert use_decode_attention(llm)
        assert fuse_decoder_layers(llm) == llm.config.num_hidden_layers and fuse_model_decode(llm)
        rows = []
        st0 = llm.model.layers[0]._ll_fused
        orig = st0.run64
        st0.run64 = lambda *a, **k: (rows.append(a[0].shape[0]), orig(*a, **k))[1]
        a = GraphedDecoder(llm, use_graph=True, fused_cache=True).generate(prompt, mask, **kw)
        n_hip = len(calls)
        b = GraphedDecoder(llm, use_graph=False, fused_cache=True).generate(prompt, mask, **kw)
        c = GraphedDecoder(llm, use_graph=True, fused_cache=True, sampler="torch").generate(prompt, mask, **kw)
    finally:
        restore_model_decode(llm)
        restore_decoder_layers(llm)
        restore_elementwise(llm)
        restore_linears(llm)
    assert 4 * B in rows                                                  # the 17-64-row decode path ran
    assert n_hip >= 2 and len(calls) > n_hip                              # graphed and eager decodes took the HIP beam step
    assert torch.equal(a, b) and torch.equal(a, c)


def test_single_beam_makes_no_beam_launch(monkeypatch):
    """num_beams absent or 1: no beam launch and the sampler is called with the same parameter tuples."""
    from llamole_amd.llm_decode import GraphedDecoder
    calls = _spy(monkeypatch)
    sp = []
    orig = GraphedDecoder._hip_sample

    def spy_sample(self, logits, p, advance):
        sp.append(p)
        return orig(self, logits, p, advance)
    monkeypatch.setattr(GraphedDecoder, "_hip_sample", spy_sample)
    llm, prompt, mask = _accel_case("tiny")
    for kw in (dict(do_sample=False, max_new_tokens=8, pad_token_id=0, eos_token_id=[2047]),
               dict(do_sample=True, temperature=0.6, top_k=50, top_p=0.9, max_new_tokens=8, pad_token_id=0, eos_token_id=[2047])):
        sp.clear()
        a = GraphedDecoder(llm).generate(prompt, mask, generator=torch.Generator(device="cuda").manual_seed(2), **kw)
        first = list(sp)
        sp.clear()
        b = GraphedDecoder(llm).generate(prompt, mask, num_beams=1, length_penalty=1.0,
                                         generator=torch.Generator(device="cuda").manual_seed(2), **kw)
        assert torch.equal(a, b) and sp == first and first
    assert not calls


@pytest.mark.parametrize("gen", [dict(num_beams=2), dict(do_sample=False, num_beams=3, length_penalty=0.8)])
def test_main_eval_with_beams(tmp_path, monkeypatch, gen):
    """`main.py eval` on the synthetic fixture with a beam-search YAML: every prompt comes back and every decode of the run (design,
    rollback, retro) went through the HIP beam step."""
    from llamole_amd import eval as ev
    from llamole_amd import synth
    from llamole_amd.llm_decode import GraphedDecoder
    from llamole_amd.modeling_llamole import SPECIAL_TOKENS
    from tests.test_eval_gpu import _script_chemistry
    _script_chemistry(monkeypatch)
    n_gen, n_beam = [], []
    orig_gen, orig_beam = GraphedDecoder.generate, GraphedDecoder._generate_beam
    monkeypatch.setattr(GraphedDecoder, "generate", lambda self, *a, **k: (n_gen.append(1), orig_gen(self, *a, **k))[1])
    monkeypatch.setattr(GraphedDecoder, "_generate_beam", lambda self, *a, **k: (n_beam.append(1), orig_beam(self, *a, **k))[1])
    hip = _spy(monkeypatch)
    cfg = synth.write_eval_fixture(str(tmp_path), SPECIAL_TOKENS)
    torch.manual_seed(0)
    try:
        out = ev.run_eval(cfg, overrides=dict(retro_iterations=3, retro_max_planning_time=20, **gen))
    finally:
        from transformers.models.qwen2 import modeling_qwen2 as mq
        if hasattr(mq.apply_rotary_pos_emb, "_ll_orig"):
            mq.apply_rotary_pos_emb = mq.apply_rotary_pos_emb._ll_orig
    assert [r["qa_idx"] for r in out["results"]] == [0, 1, 2, 3, 4]
    assert n_gen and len(n_beam) == len(n_gen) and len(hip) >= len(n_gen)
