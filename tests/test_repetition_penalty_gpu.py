"""repetition_penalty on the device: the seen-token set (ll_seen_set_init) and the penalised sampler (ll_sample_token_penalty_bf16)
through ctypes against HF's RepetitionPenalty -> Temperature -> TopK -> TopP chain, then the graphed decoder end to end."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CAP = 1024


class Pen:
    """Buffers of one sampler call for B rows of V logits, with a seen set of CAP tokens per row."""

    def __init__(self, B, V, max_new=64):
        from llamole_amd import _lib
        self.lib, self._lib, self.B, self.V = _lib.load(), _lib, B, V
        d = "cuda"
        self.seen = torch.zeros(int(self.lib.ll_seen_set_bytes(B, V, CAP)), dtype=torch.uint8, device=d)
        self.seed = torch.zeros(1, dtype=torch.long, device=d)
        self.eos = torch.full((4,), -1, dtype=torch.long, device=d)
        self.done = torch.zeros(B, dtype=torch.uint8, device=d)
        self.tok = torch.zeros(B, dtype=torch.long, device=d)
        self.out = torch.zeros(B, max_new, dtype=torch.long, device=d)
        self.step = torch.zeros(B, dtype=torch.long, device=d)
        self.ws = torch.zeros(int(self.lib.ll_sample_workspace_bytes(B)), dtype=torch.uint8, device=d)

    def init(self, ids):
        ids = ids.to("cuda").long().contiguous()
        rc = self.lib.ll_seen_set_init(self.seen.data_ptr(), self.seen.numel(), self.B, self.V, CAP, ids.data_ptr() if ids.numel() else None,
                                       max(1, ids.shape[1]), ids.shape[1], None)
        assert rc == 0

    def reset(self, seed):
        self.seed.fill_(seed)
        self.done.zero_()
        self.step.zero_()

    def _tail(self):
        return (self.seed.data_ptr(), self.eos.data_ptr(), 4, 0, self.done.data_ptr(), self.tok.data_ptr(), self.out.data_ptr(),
                self.out.stride(0), self.out.shape[1], self.step.data_ptr(), None, None, 0)

    def sample(self, logits, p, temperature=1.0, top_p=1.0, top_k=0, greedy=False):
        inv = float(np.float32(1.0) / np.float32(temperature))
        rc = self.lib.ll_sample_token_penalty_bf16(logits.data_ptr(), logits.stride(0), self.B, self.V, inv, top_p, int(top_k), int(greedy),
                                                   *self._tail(), self.seen.data_ptr(), self.seen.numel(), CAP, p, None)
        assert rc == 0
        return self.tok.clone()

    def sample_plain(self, logits, temperature=1.0, top_p=1.0, top_k=0, greedy=False):
        inv = float(np.float32(1.0) / np.float32(temperature))
        rc = self.lib.ll_sample_token_topk_ws_bf16(logits.data_ptr(), logits.stride(0), self.B, self.V, inv, top_p, int(top_k), int(greedy),
                                                   *self._tail(), None, self.ws.data_ptr(), self.ws.numel(), None)
        assert rc == 0
        return self.tok.clone()

    def set_of(self, b):
        """(count, sorted list, bitmap as a bool row) of row b."""
        rb = self.seen.numel() // self.B
        row = self.seen[b * rb:(b + 1) * rb].cpu()
        u32 = row[:(16 + 4 * CAP + 4 * ((self.V + 31) // 32))].view(torch.int32)
        n = int(u32[0])
        lst = sorted(int(x) for x in u32[4:4 + min(n, CAP)])
        words = u32[4 + CAP:4 + CAP + (self.V + 31) // 32].numpy().view(np.uint32)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:self.V].astype(bool)
        return n, lst, bits


def _hf_scores(logits, ids, p, temperature=1.0, top_k=0, top_p=1.0):
    """HF's processed f32 scores on the CPU (-inf = removed)."""
    from transformers.generation.logits_process import (InfNanRemoveLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                                                        TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper)
    s = logits.float().cpu().clone()
    ids = ids.cpu()
    procs = [RepetitionPenaltyLogitsProcessor(p), InfNanRemoveLogitsProcessor()]
    if temperature != 1.0:
        procs.append(TemperatureLogitsWarper(temperature))
    if top_k:
        procs.append(TopKLogitsWarper(top_k))
    if top_p < 1.0:
        procs.append(TopPLogitsWarper(top_p))
    for proc in procs:
        s = proc(ids, s)
    return s


def _rows(B, V, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, V, generator=g) * scale).to(torch.bfloat16)


def _seen_ids(B, V, n, seed):
    g = torch.Generator().manual_seed(seed + 1)
    if n == 0:
        return torch.zeros(B, 0, dtype=torch.long)
    return torch.stack([torch.randperm(V, generator=g)[:min(n, V)] for _ in range(B)])


def test_seen_set_init_matches_reference():
    V, B = 2048, 3
    pen = Pen(B, V)
    ids = torch.tensor([[0, 0, 0, 5, 7, 5, 2047], [3, 3, 3, 3, 3, 3, 3], [0, 1, 2, 3, 4, 5, 6]])       # pads (0), duplicates
    pen.init(ids)
    for b in range(B):
        n, lst, bits = pen.set_of(b)
        ref = sorted(set(ids[b].tolist()))
        assert n == len(ref) and lst == ref
        assert bits.nonzero()[0].tolist() == ref
    pen.init(torch.zeros(B, 0, dtype=torch.long))
    for b in range(B):
        n, lst, bits = pen.set_of(b)
        assert n == 0 and lst == [] and not bits.any()


@pytest.mark.parametrize("V", [2048, 32000, 128256, 152064])
def test_greedy_is_argmax_of_hf_scores(V):
    for B in (1, 3, 6, 24, 64):
        pen = Pen(B, V)
        logits = _rows(B, V, V + B).cuda()
        for p in (0.7, 1.3, 2.0):
            for n in (0, 1, 640, CAP):
                ids = _seen_ids(B, V, n, n + B)
                pen.init(ids)
                pen.reset(0)
                got = pen.sample(logits, p, greedy=True).cpu()
                ref = _hf_scores(logits, ids, p).argmax(dim=-1)
                assert torch.equal(got, ref), (V, B, p, n)


def _crafted(V):
    """p = 2: the seen 2.0 becomes 1.0 and ties with unseen 1.0s; the seen -0.5 becomes -1.0 and ties with unseen -1.0s."""
    x = torch.full((1, V), -8.0)
    x[0, 100] = 2.0       # seen -> 1.0
    x[0, 50] = 1.0
    x[0, 300] = 1.0
    x[0, 20] = 0.5
    x[0, 400] = -0.5      # seen -> -1.0
    x[0, 10] = -1.0
    x[0, 700] = 3.0       # seen -> 1.5
    return x.to(torch.bfloat16).cuda(), torch.tensor([[100, 400, 700]])


def test_crafted_ties_with_bf16_values():
    V = 2048
    logits, ids = _crafted(V)
    pen = Pen(1, V)
    pen.init(ids)
    pen.reset(0)
    assert int(pen.sample(logits, 2.0, greedy=True)) == 700
    logits[0, 700] = -8.0
    pen.init(ids)
    pen.reset(0)
    assert int(pen.sample(logits, 2.0, greedy=True)) == 50          # lowest index of the three 1.0s (one penalised)
    # top_k = 2 keeps every 1.0 (ties with the k-th value); top_k = 3 too; the nucleus boundary ties keep all of them
    for top_k, top_p in ((2, 1.0), (3, 1.0), (0, 0.5), (4, 0.9)):
        kept = torch.isfinite(_hf_scores(logits, ids, 2.0, 1.0, top_k, top_p))[0]
        drawn = set()
        for s in range(300):
            pen.init(ids)
            pen.reset(s)
            t = int(pen.sample(logits, 2.0, top_k=top_k, top_p=top_p))
            assert bool(kept[t]), (top_k, top_p, t)
            drawn.add(t)
        assert drawn == set(kept.nonzero()[:, 0].tolist()), (top_k, top_p)


@pytest.mark.parametrize("B", [2, 8])
@pytest.mark.parametrize("V,p,temperature,top_k,top_p", [(32000, 1.3, 0.6, 50, 0.9), (152064, 0.7, 1.0, 0, 0.8),
                                                           (152064, 2.0, 0.8, 5000, 0.95), (2048, 1.3, 1.2, 7, 1.0)])
def test_draws_lie_in_hf_kept_set(B, V, p, temperature, top_k, top_p):
    pen = Pen(B, V)
    logits = _rows(B, V, 7, scale=3.0).cuda()
    # the seen tokens include the row's largest logits, so the penalty moves the top of the distribution
    g = torch.Generator().manual_seed(3)
    top = logits.float().topk(8, dim=-1).indices.cpu()
    rows = []
    for r in range(B):
        perm = torch.randperm(V, generator=g)
        rows.append(torch.cat([top[r], perm[~torch.isin(perm, top[r])][:632]]))
    ids = torch.stack(rows)
    # HF's set, plus the rest of the tie group of HF's lowest kept value (torch.sort splits such a group at the nucleus boundary, the
    # sampler keeps all of it)
    pre = _hf_scores(logits, ids, p, temperature, top_k, 1.0)
    hf = torch.isfinite(_hf_scores(logits, ids, p, temperature, top_k, top_p))
    low = torch.where(hf, pre, torch.full_like(pre, float("inf"))).min(dim=1, keepdim=True).values
    kept = (hf | (torch.isfinite(pre) & (pre >= low))).cuda()
    bad = 0
    for s in range(2000):
        pen.init(ids)
        pen.reset(s)
        t = pen.sample(logits, p, temperature, top_p, top_k)
        bad += int((~kept.gather(1, t.view(B, 1))).sum())
    assert bad == 0


def test_frequencies_match_hf_probabilities():
    from scipy.stats import chisquare
    V = 2048
    logits = torch.full((1, V), -30.0)
    vals = [2.0, 1.5, 1.0, 0.5, 0.25, -0.5]
    for i, v in enumerate(vals):
        logits[0, 10 * (i + 1)] = v
    logits = logits.to(torch.bfloat16).cuda()
    ids = torch.tensor([[10, 30, 60]])
    s = _hf_scores(logits, ids, 1.7, 0.8, 5, 1.0)[0]
    probs = torch.softmax(s, dim=-1)
    keep = probs.nonzero()[:, 0]
    pen = Pen(1, V)
    counts = {int(k): 0 for k in keep}
    N = 6000
    for sd in range(N):
        pen.init(ids)
        pen.reset(sd)
        t = int(pen.sample(logits, 1.7, 0.8, 1.0, 5))
        assert t in counts
        counts[t] += 1
    obs = np.array([counts[int(k)] for k in keep], dtype=np.float64)
    exp = probs[keep].double().numpy()
    exp = exp / exp.sum() * obs.sum()
    assert chisquare(obs, exp).pvalue > 1e-4


@pytest.mark.parametrize("B,V", [(1, 152064), (3, 32000), (8, 152064)])
def test_neutral_penalty_or_empty_set_is_the_plain_sampler(B, V):
    logits = _rows(B, V, 11).cuda()
    pen = Pen(B, V)
    ids = _seen_ids(B, V, 640, 5)
    for p, seen in ((1.0, ids), (1.3, torch.zeros(B, 0, dtype=torch.long))):
        for s in range(100):
            pen.reset(s)
            ref = pen.sample_plain(logits, 0.6, 0.9, 50)
            ref_b = (pen.done.clone(), pen.step.clone(), pen.out.clone())
            pen.init(seen)
            pen.reset(s)
            got = pen.sample(logits, p, 0.6, 0.9, 50)
            assert torch.equal(got, ref), (p, s)
            assert torch.equal(pen.done, ref_b[0]) and torch.equal(pen.step, ref_b[1]) and torch.equal(pen.out, ref_b[2])


def test_set_tracks_prompt_and_emitted_tokens():
    B, V = 3, 32000
    pen = Pen(B, V)
    ids = _seen_ids(B, V, 20, 9)
    pen.init(ids)
    pen.reset(1)
    emitted = [[] for _ in range(B)]
    for i in range(12):
        t = pen.sample(_rows(B, V, 100 + i).cuda(), 1.3, 1.0, 1.0, 0).cpu()
        for b in range(B):
            emitted[b].append(int(t[b]))
    for b in range(B):
        n, lst, bits = pen.set_of(b)
        ref = sorted(set(ids[b].tolist()) | set(emitted[b]))
        assert lst == ref and n == len(ref) and bits.nonzero()[0].tolist() == ref


def test_nan_and_inf_on_seen_tokens():
    """A seen NaN is sanitised to 0.0 and a seen +-inf to +-max before nothing else (HF: the penalty keeps them NaN / inf, then
    InfNanRemoveLogitsProcessor maps them to 0 / +-finfo.max), as the unpenalised sampler treats the raw logit."""
    V = 2048
    x = torch.full((1, V), -4.0)
    x[0, 5] = float("nan")       # seen NaN -> 0.0: the row maximum, tied with the unseen 0.0 at 9
    x[0, 9] = 0.0
    x[0, 11] = -0.5               # seen -> -1.0
    x[0, 13] = float("-inf")      # seen
    logits = x.to(torch.bfloat16).cuda()
    ids = torch.tensor([[5, 11, 13]])
    pen = Pen(1, V)
    pen.init(ids)
    pen.reset(0)
    assert int(pen.sample(logits, 1.3, greedy=True)) == int(_hf_scores(logits, ids, 1.3).argmax()) == 5
    kept = torch.isfinite(_hf_scores(logits, ids, 1.3, 1.0, 2, 1.0))[0]
    for s in range(200):
        pen.init(ids)
        pen.reset(s)
        t = int(pen.sample(logits, 1.3, top_k=2))
        assert bool(kept[t]) and t in (5, 9)
    x[0, 700] = float("inf")      # seen +inf -> the maximum
    logits = x.to(torch.bfloat16).cuda()
    ids = torch.tensor([[5, 11, 13, 700]])
    pen.init(ids)
    pen.reset(0)
    assert int(pen.sample(logits, 1.3, greedy=True)) == int(_hf_scores(logits, ids, 1.3).argmax()) == 700
    pen.init(ids)
    pen.reset(0)
    assert int(pen.sample(logits, 1.3, 0.7, 0.9, 50)) == 700


# ---------------------------------------------------------------- decoder
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


def _spy_sampler(monkeypatch):
    from llamole_amd.llm_decode import GraphedDecoder
    calls = []
    orig = GraphedDecoder._hip_sample

    def spy(self, logits, sp, advance):
        calls.append(sp)
        return orig(self, logits, sp, advance)
    monkeypatch.setattr(GraphedDecoder, "_hip_sample", spy)
    return calls


@pytest.mark.parametrize("name", ["tiny", "tiny-llama"])
def test_graphed_decode_with_penalty(name, monkeypatch):
    from llamole_amd.llm_decode import GraphedDecoder
    llm, prompt, mask = _accel_case(name)
    kw = dict(max_new_tokens=8, do_sample=False, pad_token_id=0, eos_token_id=[2047], repetition_penalty=1.3)
    calls = _spy_sampler(monkeypatch)
    eager = GraphedDecoder(llm, use_graph=False).generate(prompt, mask, **kw)
    dec = GraphedDecoder(llm, use_graph=True)
    got = dec.generate(prompt, mask, **kw)
    assert calls and all(sp[5] == np.float32(1.3) for sp in calls)         # the HIP sampler ran, with the penalty
    assert torch.equal(eager, got)
    ref = llm.generate(inputs=prompt, attention_mask=mask, **kw)
    assert torch.equal(ref, got)                                           # all 8 new tokens
    # inputs_embeds (the form of the design and retro calls): only generated tokens are penalised
    emb = llm.get_input_embeddings()(prompt)
    got_e = GraphedDecoder(llm, use_graph=True).generate(None, mask, inputs_embeds=emb, **kw)
    assert torch.equal(got_e, GraphedDecoder(llm, use_graph=False).generate(None, mask, inputs_embeds=emb, **kw))
    assert torch.equal(got_e, llm.generate(inputs_embeds=emb, attention_mask=mask, **kw))
    # p switched 1.3 -> 1.0 -> 1.3 on one decoder: the tokens of fresh decoders
    plain = dict(kw, repetition_penalty=1.0)
    assert torch.equal(dec.generate(prompt, mask, **plain), GraphedDecoder(llm, use_graph=True).generate(prompt, mask, **plain))
    assert torch.equal(dec.generate(prompt, mask, **kw), got)
    # seeded sampling is reproducible
    gen = torch.Generator(device="cuda").manual_seed(5)
    skw = dict(max_new_tokens=12, do_sample=True, temperature=0.6, top_p=0.9, top_k=50, pad_token_id=0, repetition_penalty=1.3)
    s1 = dec.generate(prompt, mask, generator=gen, **skw)
    gen.manual_seed(5)
    assert torch.equal(s1, dec.generate(prompt, mask, generator=gen, **skw))


@pytest.mark.parametrize("B", [24, 64])
def test_wide_batches_with_penalty(B, monkeypatch):
    """17-64 rows decode on the seven-launch layers (ll_linear_rows64_bf16) and sample with the penalty in the captured step."""
    from llamole_amd import e2e
    from llamole_amd.llm_accel import (accelerate_elementwise, accelerate_linears, fuse_decoder_layers, fuse_model_decode,
                                       restore_decoder_layers, restore_elementwise, restore_linears, restore_model_decode,
                                       use_decode_attention)
    from llamole_amd.llm_decode import GraphedDecoder
    llm = e2e.build_llm("tiny", "cuda", torch.bfloat16)
    g = torch.Generator().manual_seed(B)
    prompt = torch.randint(5, 1000, (B, 10), generator=g).cuda()
    mask = torch.ones_like(prompt)
    mask[1, :4] = 0
    prompt[1, :4] = 0
    kw = dict(max_new_tokens=6, do_sample=False, pad_token_id=0, eos_token_id=[2047], repetition_penalty=1.3)
    ref = llm.generate(inputs=prompt, attention_mask=mask, **kw)          # HF on the stock modules
    calls = _spy_sampler(monkeypatch)
    try:
        assert accelerate_linears(llm, min_weight_elems=1) > 0
        accelerate_elementwise(llm)
        assert use_decode_attention(llm)
        assert fuse_decoder_layers(llm) == llm.config.num_hidden_layers and fuse_model_decode(llm)
        rows = []
        st0 = llm.model.layers[0]._ll_fused
        orig = st0.run64
        st0.run64 = lambda *a, **k: (rows.append(a[0].shape[0]), orig(*a, **k))[1]
        got = GraphedDecoder(llm, use_graph=True, fused_cache=True).generate(prompt, mask, **kw)
        eager = GraphedDecoder(llm, use_graph=False, fused_cache=True).generate(prompt, mask, **kw)
        # the same fused forward with the torch sampler: HF's formula over the same tokens, then argmax of the f32 row
        torch_ref = GraphedDecoder(llm, use_graph=False, fused_cache=True, sampler="torch").generate(prompt, mask, **kw)
    finally:
        restore_model_decode(llm)
        restore_decoder_layers(llm)
        restore_elementwise(llm)
        restore_linears(llm)
    assert B in rows                                                      # the 17-64-row decode path ran
    assert calls and all(sp[5] == np.float32(1.3) for sp in calls)     # with the penalised HIP sampler
    assert torch.equal(got, eager) and got.shape == (B, 16)
    assert torch.equal(got, torch_ref)
    # against HF on the stock modules: the fused bf16 layers round differently and a random tiny model has near ties, so only most
    # rows agree token for token; the penalty itself is pinned by the torch-sampler comparison above
    assert (ref == got).all(dim=1).float().mean() >= 0.5


def test_main_eval_with_repetition_penalty(tmp_path, monkeypatch):
    from llamole_amd import eval as ev
    from llamole_amd import synth
    from llamole_amd.modeling_llamole import SPECIAL_TOKENS
    from tests.test_eval_gpu import _script_chemistry
    _script_chemistry(monkeypatch)
    calls = _spy_sampler(monkeypatch)
    cfg = synth.write_eval_fixture(str(tmp_path), SPECIAL_TOKENS)
    with open(cfg, "a") as f:
        f.write("\nrepetition_penalty: 1.2\n")                 # the YAML key, as a generate config sets it
    torch.manual_seed(0)
    try:
        out = ev.run_eval(cfg, overrides={"retro_iterations": 3, "retro_max_planning_time": 20})
    finally:
        from transformers.models.qwen2 import modeling_qwen2 as mq
        if hasattr(mq.apply_rotary_pos_emb, "_ll_orig"):
            mq.apply_rotary_pos_emb = mq.apply_rotary_pos_emb._ll_orig
    assert [r["qa_idx"] for r in out["results"]] == [0, 1, 2, 3, 4]
    assert calls and all(sp[5] == np.float32(1.2) for sp in calls)          # every decode of the run sampled with the penalty
