"""Prompt-lookup speculative decoding on the device: ll_spec_draft against the torch drafting rule, ll_spec_verify_bf16 against the
existing token sampler as oracle (row i alone, B = 1, step preset to t + i), the documented refusals, and the decode end to end --
graphed == eager == sampler="torch" tokens on the fused S-row forward, statistics equal to a replay, one speculative step against HF f32
(E <= 1.5 Y as tests/test_granite_decode_gpu.py defines it), and the option off leaving the decode's launch list alone.

Figures are printed with -s; the ones measured on an MI355X are in DESIGN.md 4x."""
import copy
import warnings

import pytest
import torch

from llamole_amd import _lib, e2e, llm_spec
from llamole_amd.llm_decode import GraphedDecoder
from tests.test_kv8_decode_gpu import _restore, _Spy
from tests.test_prompt_lookup_cpu import KN, replay

pytestmark = pytest.mark.gpu

MARGIN = 1.5            # a bf16 engine against the reference's own bf16
CAP = 96                # history / output capacity of the kernel tests
MODES = [(1, 1.0, 1.0, 0), (0, 0.6, 0.9, 50), (0, 1.0, 0.8, 0)]        # (greedy, temperature, top_p, top_k)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _long(*v):
    return torch.tensor(list(v), dtype=torch.long, device="cuda")


# ------------------------------------------------------------------------------------------------------------------ draft kernel
def _draft(lib, history, last, k, n, append, pos=37, posid=29, cap=None):
    """(ids, position_ids, cache_position, history length, history) after one ll_spec_draft; ``history`` excludes ``last`` when append"""
    cap = cap or len(history) + 4
    hist = torch.full((cap,), -5, dtype=torch.long, device="cuda")
    hist[:len(history)] = torch.tensor(history, dtype=torch.long)
    hl, tok, p, q = _long(len(history)), _long(last), _long(pos), _long(posid)
    ids, pids, cpos = (torch.full((k + 1,), -9, dtype=torch.long, device="cuda") for _ in range(3))
    rc = lib.ll_spec_draft(hist.data_ptr(), cap, hl.data_ptr(), tok.data_ptr(), append, k, n, p.data_ptr(), q.data_ptr(), ids.data_ptr(),
                           pids.data_ptr(), cpos.data_ptr(), _stream())
    assert rc == 0, lib.ll_last_error()
    return ids.tolist(), pids.tolist(), cpos.tolist(), int(hl), hist.tolist()


@pytest.mark.parametrize("k,n", KN)
def test_draft_kernel_equals_the_torch_rule(lib, k, n):
    g = torch.Generator().manual_seed(100 * k + n)
    cases = [torch.randint(0, 4, (L,), generator=g).tolist() for L in range(2, 41)]
    cases += [list(range(20)), [3, 3], [3]]                 # no match, a continuation shorter than k, n larger than the history
    for h in cases:
        want = llm_spec.draft_rows(h, h[-1], k, n)
        for append in (0, 1):
            ids, pids, cpos, L, hist = _draft(lib, h[:len(h) - append], h[-1], k, n, append)
            assert ids == want, (h, k, n, append)
            assert pids == [29 + i for i in range(k + 1)] and cpos == [37 + i for i in range(k + 1)]
            assert L == len(h) and hist[:L] == h and all(t == -5 for t in hist[L:])
    # the empty history of an inputs_embeds call: the first token is appended, nothing can match
    ids, _, _, L, hist = _draft(lib, [], 11, k, n, 1)
    assert ids == [11] * (k + 1) and L == 1 and hist[0] == 11
    # a full history is not appended to
    ids, _, _, L, hist = _draft(lib, [1, 2, 1], 2, k, n, 1, cap=3)
    assert L == 3 and hist == [1, 2, 1] and ids == llm_spec.draft_rows([1, 2, 1], 2, k, n)


def test_draft_kernel_long_history_match_in_the_last_tokens(lib):
    """4096 tokens, all distinct but for the last 8: the only match of the last bigram starts 6 tokens before the end"""
    h = list(range(100, 100 + 4088)) + [5000, 5001, 7, 8, 9, 10, 5000, 5001]
    for k, n in KN:
        want = llm_spec.draft_rows(h, h[-1], k, n)
        assert want[1:1 + min(k, 6)] == [7, 8, 9, 10, 5000, 5001][:k] or n == 1
        ids, pids, cpos, L, _ = _draft(lib, h[:-1], h[-1], k, n, 1)
        assert ids == want and L == 4096 and pids[-1] == 29 + k and cpos[-1] == 37 + k, (k, n)


# ------------------------------------------------------------------------------------------------------------------ verify kernel
class _State:
    """device state of one verify call, poisoned where the kernel must not write"""

    def __init__(self, S, t, rows, history, eos=(), max_new=CAP, done=0):
        self.S = S
        self.seed, self.step, self.pos, self.posid, self.cum = _long(1234567), _long(t), _long(40), _long(33), _long(-1)
        self.done = torch.tensor([done], dtype=torch.uint8, device="cuda")
        self.tok, self.max_new, self.stats = _long(rows[0]), _long(max_new), _long(3, 4)
        self.out = torch.full((CAP,), -7, dtype=torch.long, device="cuda")
        self.eos = torch.full((32,), -1, dtype=torch.long, device="cuda")
        if eos:
            self.eos[:len(eos)] = torch.tensor(list(eos), dtype=torch.long)
        self.ids, self.pids, self.cpos = _long(*rows), _long(*range(33, 33 + S)), _long(*range(40, 40 + S))
        self.hist = torch.full((CAP,), -5, dtype=torch.long, device="cuda")
        self.hist[:len(history)] = torch.tensor(history, dtype=torch.long)
        self.hl = _long(len(history))
        self.xs = torch.full((16,), -3, dtype=torch.long, device="cuda")

    def tensors(self):
        return [self.step, self.pos, self.posid, self.cum, self.done, self.tok, self.stats, self.out, self.ids, self.pids, self.cpos, self.hist,
                self.hl]

    def snapshot(self):
        return [t.clone() for t in self.tensors()]


def _verify(lib, logits, st, mode, n=2, draft_next=1, S=None, V=None, ld=None, null=None):
    greedy, temp, top_p, top_k = mode
    import numpy as np
    args = [logits.data_ptr(), logits.stride(0) if ld is None else ld, st.S if S is None else S, logits.shape[1] if V is None else V,
            float(np.float32(1.0) / np.float32(temp)), top_p, top_k, greedy, st.seed.data_ptr(), st.eos.data_ptr(), 32, st.done.data_ptr(),
            st.tok.data_ptr(), st.out.data_ptr(), CAP, st.max_new.data_ptr(), st.step.data_ptr(), st.posid.data_ptr(), st.pos.data_ptr(),
            st.cum.data_ptr(), st.ids.data_ptr(), st.pids.data_ptr(), st.cpos.data_ptr(), st.hist.data_ptr(), CAP, st.hl.data_ptr(), n, draft_next,
            st.stats.data_ptr(), st.xs.data_ptr(), _stream()]
    if null is not None:
        args[null] = None
    return lib.ll_spec_verify_bf16(*args)


def _oracle(lib, logits, t, mode, seed=1234567):
    """x_i of every row: ll_sample_token_topk_bf16 on row i alone, B = 1, step preset to t + i"""
    import numpy as np
    greedy, temp, top_p, top_k = mode
    sd, done, tok, out = _long(seed), torch.zeros(1, dtype=torch.uint8, device="cuda"), _long(0), torch.zeros(CAP, dtype=torch.long, device="cuda")
    xs = []
    for i in range(logits.shape[0]):
        step = _long(t + i)
        row = logits[i:i + 1]
        rc = lib.ll_sample_token_topk_bf16(row.data_ptr(), row.stride(0), 1, row.shape[1], float(np.float32(1.0) / np.float32(temp)), top_p, top_k,
                                           greedy, sd.data_ptr(), None, 0, 0, done.data_ptr(), tok.data_ptr(), out.data_ptr(), CAP, CAP,
                                           step.data_ptr(), None, None, 0, None, _stream())
        assert rc == 0, lib.ll_last_error()
        xs.append(int(tok))
    return xs


def _check_step(lib, logits, rows, x, mode, t=5, eos=(), max_new=CAP, n=2, draft_next=1):
    """one verify call from a fresh state against llm_spec.accept on the oracle's tokens; returns the number emitted"""
    S, k = len(rows), len(rows) - 1
    history = [9, 8, 9, 8, 7, rows[0]]
    st = _State(S, t, rows, history, eos, max_new)
    assert _verify(lib, logits, st, mode, n=n, draft_next=draft_next) == 0, lib.ll_last_error()
    emitted, stop = llm_spec.accept(rows, x, set(eos), max_new - t)
    e = len(emitted)
    assert st.xs[:S].tolist() == x and st.xs[S:].tolist() == [-3] * (16 - S)
    assert int(st.step) == t + e and int(st.pos) == 40 + e and int(st.posid) == 33 + e and int(st.cum) == 40 + e
    assert int(st.done) == int(stop) and int(st.tok) == emitted[-1]
    assert st.out.tolist() == [-7] * t + emitted + [-7] * (CAP - t - e)
    h2 = history + emitted
    assert int(st.hl) == len(h2) and st.hist.tolist() == h2 + [-5] * (CAP - len(h2))
    assert st.stats.tolist() == [4, 4 + e - 1]
    if draft_next:
        assert st.ids.tolist() == llm_spec.draft_rows(h2, emitted[-1], k, n)
        assert st.pids.tolist() == [33 + e + i for i in range(S)] and st.cpos.tolist() == [40 + e + i for i in range(S)]
    else:
        assert st.ids.tolist() == rows and st.pids.tolist() == list(range(33, 33 + S)) and st.cpos.tolist() == list(range(40, 40 + S))
    return e


def _rows_accepting(x, a, V):
    """[last, d_1..d_k] whose first a drafts are the oracle's own tokens and whose draft a + 1 (and every later one) is not"""
    k = len(x) - 1
    return [17] + [x[i] if i < a else (x[i] + 1) % V for i in range(k)]


@pytest.mark.parametrize("V", [2048, 32000, 152064])
@pytest.mark.parametrize("S", [3, 6, 16])
def test_verify_emits_the_samplers_tokens(lib, V, S):
    g = torch.Generator().manual_seed(V + S)
    ld = V + 8                                              # a row stride that is not the width
    buf = torch.zeros(S, ld, dtype=torch.bfloat16, device="cuda")
    buf[:, :V] = (torch.randn(S, V, generator=g) * 3).to(torch.bfloat16).cuda()
    logits = buf[:, :V]
    k = S - 1
    for mode in MODES:
        x = _oracle(lib, logits, 5, mode)
        if mode[0]:
            assert x == logits.float().argmax(dim=-1).tolist()
        for a in range(k + 1):                              # every accepted length 0..k
            assert _check_step(lib, logits, _rows_accepting(x, a, V), x, mode) == a + 1, (mode, a)
        full = _rows_accepting(x, k, V)
        # an EOS at emitted index 0, in the middle and last; max_new reached mid-run; no next draft
        for j in (0, k // 2, k):
            first = x.index(x[j])                           # (a repeated token stops the run at its first occurrence)
            assert _check_step(lib, logits, full, x, mode, eos=(x[j], V + 5)) == first + 1, (mode, j)
        assert _check_step(lib, logits, full, x, mode, max_new=5 + 2) == 2
        assert _check_step(lib, logits, full, x, mode, max_new=5 + 1) == 1
        assert _check_step(lib, logits, full, x, mode, draft_next=0) == S
        # a call on a done state, or at step == max_new, changes nothing
        for kw in (dict(done=1), dict(max_new=5)):
            st = _State(S, 5, full, [9, 8, 17], **kw)
            before = st.snapshot()
            assert _verify(lib, logits, st, mode) == 0
            assert all(torch.equal(p, q) for p, q in zip(before, st.tensors())), kw


def test_seed_and_step_select_the_draw(lib):
    """sampling: another seed or another step value gives the oracle's other tokens (the counter is (t + i, 0) under *seed)"""
    V, S, mode = 32000, 6, MODES[2]
    logits = (torch.randn(S, V, generator=torch.Generator().manual_seed(1)) * 2).to(torch.bfloat16).cuda()
    base = _oracle(lib, logits, 5, mode)
    for t, seed in ((6, 1234567), (5, 99)):
        x = _oracle(lib, logits, t, mode, seed)
        assert x != base
        st = _State(S, t, _rows_accepting(x, S - 1, V), [1, 2, 17])
        st.seed.fill_(seed)
        assert _verify(lib, logits, st, mode) == 0
        assert st.out[t:t + S].tolist() == x


def test_documented_refusals_return_an_error_and_write_nothing(lib):
    V, S = 2048, 6
    logits = torch.zeros(S, V, dtype=torch.bfloat16, device="cuda")
    rows = [17, 1, 2, 3, 4, 5]
    bad = [dict(S=2), dict(S=17), dict(V=2044), dict(V=163848, ld=163848), dict(ld=V + 4), dict(ld=V - 8), dict(n=0), dict(null=0), dict(null=8),
           dict(null=15), dict(null=20), dict(null=23), dict(null=28), dict(null=29)]
    for kw in bad:
        st = _State(S, 5, rows, [9, 8, 17])
        before, xs = st.snapshot(), st.xs.clone()
        assert _verify(lib, logits, st, MODES[0], **kw) == -1, kw
        torch.cuda.synchronize()
        assert all(torch.equal(p, q) for p, q in zip(before, st.tensors())) and torch.equal(xs, st.xs), kw
    st = _State(S, 5, rows, [9, 8, 17])
    assert _verify(lib, logits, st, (0, -1.0, 0.9, 0)) == -1 and b"temperature" in lib.ll_last_error()
    # the draft entry: k outside 2..15, n < 1, no capacity, a null pointer
    hist, hl, tok = torch.full((8,), -5, dtype=torch.long, device="cuda"), _long(3), _long(17)
    out = [torch.full((16,), -9, dtype=torch.long, device="cuda") for _ in range(3)]
    for k, n, cap, null in ((1, 2, 8, None), (16, 2, 8, None), (4, 0, 8, None), (4, 2, 0, None), (4, 2, 8, 0), (4, 2, 8, 9)):
        args = [hist.data_ptr(), cap, hl.data_ptr(), tok.data_ptr(), 1, k, n, tok.data_ptr(), tok.data_ptr(), out[0].data_ptr(),
                out[1].data_ptr(), out[2].data_ptr(), _stream()]
        if null is not None:
            args[null] = None
        assert lib.ll_spec_draft(*args) == -1, (k, n, cap, null)
        torch.cuda.synchronize()
        assert int(hl) == 3 and bool((hist == -5).all()) and all(bool((o == -9).all()) for o in out)


# ------------------------------------------------------------------------------------------------------------------ end to end
SPEC_KW = dict(max_new_tokens=24, do_sample=False, pad_token_id=0, eos_token_id=[])


def _prompt(seed=21, P=12):
    p = torch.randint(5, 2000, (1, P), generator=torch.Generator().manual_seed(seed)).cuda()
    return p, torch.ones_like(p)


def _run_e2e(llm, monkeypatch, ks=(4, 7), **dec_kw):
    from llamole_amd.llm_accel import _FusedLayer
    seen = []
    orig = _FusedLayer.run_suffix
    monkeypatch.setattr(_FusedLayer, "run_suffix", lambda self, *a, **k: (seen.append("suffix"), orig(self, *a, **k))[1])
    p, m = _prompt()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        for k in ks:
            graphed = GraphedDecoder(llm, use_graph=True, fused_cache=True, **dec_kw)
            eager = GraphedDecoder(llm, use_graph=False, fused_cache=True, **dec_kw)
            by_torch = GraphedDecoder(llm, use_graph=False, fused_cache=True, sampler="torch", **dec_kw)
            kw = dict(SPEC_KW, prompt_lookup_num_tokens=k)
            seen.clear()
            got = graphed.generate(p, m, **kw)
            assert graphed._spec_graph is not None and graphed._graph is None and "suffix" in seen, k
            assert got.shape == (1, 12 + 24) and torch.equal(got[:, :12], p)
            assert torch.equal(got, eager.generate(p, m, **kw)), k
            assert torch.equal(got, by_torch.generate(p, m, **kw)), k
            new = got[0, 12:].tolist()
            f, a, _ = replay(p[0].tolist(), new, k, 2)
            want = {"forwards": f, "accepted": a, "tokens": 24}
            assert graphed.spec_stats == want and eager.spec_stats == want and by_torch.spec_stats == want, (k, graphed.spec_stats, want)
            assert graphed._last["n_new"] == 24
            graph = graphed._spec_graph
            assert torch.equal(graphed.generate(p, m, **kw), got) and graphed._spec_graph is graph          # replayed, not captured again
            skw = dict(kw, do_sample=True, temperature=0.6, top_p=0.9, top_k=50)
            s1 = graphed.generate(p, m, generator=torch.Generator(device="cuda").manual_seed(5), **skw)
            s2 = graphed.generate(p, m, generator=torch.Generator(device="cuda").manual_seed(5), **skw)
            s3 = eager.generate(p, m, generator=torch.Generator(device="cuda").manual_seed(5), **skw)
            assert torch.equal(s1, s2) and torch.equal(s1, s3), k
            print(f"\nk = {k}: greedy {want}, tokens per forward {24 / (f + 1):.2f}")
    assert not rec, [str(w.message) for w in rec]


@pytest.mark.parametrize("name", ["tiny", "tiny-llama", "tiny-qwen3"])
def test_graphed_eager_and_torch_sampler_give_the_same_tokens(name, monkeypatch):
    from llamole_amd.llm_accel import accelerate_llm
    llm = e2e.build_llm(name, "cuda", torch.bfloat16)
    try:
        info = accelerate_llm(llm)
        assert info["decoder_layers_5_launches"] == llm.config.num_hidden_layers and info["decode_prologue_1_launch"] is True
        _run_e2e(llm, monkeypatch)
    finally:
        _restore(llm)


def test_mxfp8_kv_cache(monkeypatch):
    from llamole_amd.llm_accel import accelerate_llm
    llm = e2e.build_llm("tiny-llama", "cuda", torch.bfloat16)
    try:
        accelerate_llm(llm)
        _run_e2e(llm, monkeypatch, ks=(4,), kv_cache="mxfp8")
    finally:
        _restore(llm)


def test_quantization_bit_4(monkeypatch):
    from llamole_amd.llm_accel import accelerate_llm
    llm = e2e.build_llm("tiny-llama", "cuda", torch.bfloat16)
    try:
        info = accelerate_llm(llm, quantization_bit=4)
        assert info["quantization"]["bits"] == 4
        _run_e2e(llm, monkeypatch, ks=(4,))
    finally:
        _restore(llm)


def test_hf_layers_run_the_same_step(monkeypatch):
    """layers=False: no fused query-token forward, HF's own forward serves the S rows under the same captured step"""
    from llamole_amd.llm_accel import accelerate_llm
    llm = e2e.build_llm("tiny-llama", "cuda", torch.bfloat16)
    try:
        accelerate_llm(llm, layers=False)
        p, m = _prompt()
        kw = dict(SPEC_KW, prompt_lookup_num_tokens=4)
        for fused_cache in (False, True):
            graphed = GraphedDecoder(llm, use_graph=True, fused_cache=fused_cache)
            eager = GraphedDecoder(llm, use_graph=False, fused_cache=fused_cache)
            got = graphed.generate(p, m, **kw)
            assert torch.equal(got, eager.generate(p, m, **kw)) and graphed._spec_graph is not None
            f, a, _ = replay(p[0].tolist(), got[0, 12:].tolist(), 4, 2)
            assert graphed.spec_stats == {"forwards": f, "accepted": a, "tokens": 24}
    finally:
        _restore(llm)


def test_continue_hidden_after_a_speculative_call():
    from llamole_amd.llm_accel import accelerate_llm
    llm = e2e.build_llm("tiny-llama", "cuda", torch.bfloat16)
    try:
        accelerate_llm(llm)
        p, m = _prompt()
        tail = torch.randint(5, 2000, (1, 4), generator=torch.Generator().manual_seed(9)).cuda()
        hid, toks = {}, {}
        for k in (None, 4):
            dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
            toks[k] = dec.generate(p, m, prompt_lookup_num_tokens=k, **SPEC_KW)
            assert dec._last["n_new"] == 24
            hid[k] = dec.continue_hidden(tail, 12 + 24 - 1).float().clone()
        if torch.equal(toks[None], toks[4]):
            err = float((hid[None] - hid[4]).abs().max() / hid[None].abs().max())
            print(f"\ncontinue_hidden after a speculative against a plain generate: max |diff| / max |h| = {err:.5f}")
            assert err <= 3e-2
        else:
            print("\nplain and speculative greedy tokens differ on this prompt: the hidden states are of different sequences")
    finally:
        _restore(llm)


def _hf_rows(model, ids, S):
    with torch.no_grad():
        return model(input_ids=ids, use_cache=False).logits[0, -S:, :].float()


@pytest.mark.parametrize("name", ["tiny", "tiny-llama", "tiny-qwen3"])
def test_one_speculative_step_against_hf(name):
    """1 row of 13 tokens, greedy, max_new_tokens = 2, k = 4: last_logits are the S = 5 logits rows of ONE speculative step.  Reference:
    the untouched HF model in f32 over prompt + the step's rows; Y = max |HF bf16 - reference|; E = max |fused - reference| <= 1.5 Y."""
    from llamole_amd.llm_accel import accelerate_llm
    llm = e2e.build_llm(name, "cuda", torch.bfloat16)
    hf16, hf32 = copy.deepcopy(llm), copy.deepcopy(llm).float()
    # a prompt that repeats itself, so that whatever comes first has a continuation to draft from under n = 1 when it is a prompt token
    base = torch.randint(5, 2000, (1, 6), generator=torch.Generator().manual_seed(13))
    prompt = torch.cat([base, base, base[:, :1]], dim=1).cuda()
    try:
        accelerate_llm(llm)
        dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
        toks = dec.generate(prompt, torch.ones_like(prompt), max_new_tokens=2, do_sample=False, pad_token_id=0, eos_token_id=[],
                            prompt_lookup_num_tokens=4, max_matching_ngram_size=1)
        assert dec.spec_stats["forwards"] == 1 and dec.last_logits.shape[0] == 5 and llm.model._ll_decode["served"]
        fused = dec.last_logits.float().clone()
        first = int(toks[0, 13])
        rows = llm_spec.draft_rows(prompt[0].tolist() + [first], first, 4, 1)
        ids = torch.cat([prompt, torch.tensor([rows], device="cuda")], dim=1)
        ref = _hf_rows(hf32, ids, 5)
        Y = float((_hf_rows(hf16, ids, 5) - ref).abs().max())
        E = float((fused - ref).abs().max())
        print(f"\n{name} one speculative step (rows {rows}), max |logit error| against HF f32 over 5 rows: fused E = {E:.5f}, "
              f"HF bf16 Y = {Y:.5f}, E / Y = {E / Y:.3f}")
        assert Y > 0 and E <= MARGIN * Y, (E, Y)
    finally:
        _restore(llm)


@pytest.mark.parametrize("name", ["tiny", "tiny-llama", "tiny-qwen3"])
def test_plain_against_speculative_greedy_tokens_reported(name):
    """Not asserted equal: the 1-row GEMV and the S-row MFMA Linear round differently, and a near-tie of these random-weight logits may flip
    (DESIGN.md 4x).  The prompt and the first token are the same computation."""
    from llamole_amd.llm_accel import accelerate_llm
    llm = e2e.build_llm(name, "cuda", torch.bfloat16)
    try:
        accelerate_llm(llm)
        p, m = _prompt()
        plain = GraphedDecoder(llm, use_graph=True, fused_cache=True).generate(p, m, **SPEC_KW)
        spec = GraphedDecoder(llm, use_graph=True, fused_cache=True).generate(p, m, prompt_lookup_num_tokens=4, **SPEC_KW)
        diff = (plain != spec)[0].nonzero()
        print(f"\n{name}: plain against speculative greedy tokens, first differing index: {int(diff[0]) - 12 if diff.numel() else None} of 24")
        assert torch.equal(plain[:, :13], spec[:, :13])
    finally:
        _restore(llm)


def test_option_off_calls_no_spec_entry_and_keeps_the_launch_list(monkeypatch):
    from llamole_amd.llm_accel import accelerate_llm
    llm = e2e.build_llm("tiny-llama", "cuda", torch.bfloat16)
    try:
        accelerate_llm(llm)
        real = _lib.load()
        top, per_layer, model_level = [], [[] for _ in llm.model.layers], []
        monkeypatch.setattr(_lib, "_lib", _Spy(real, top))
        states = [l._ll_fused for l in llm.model.layers]
        st = llm.model._ll_decode
        for s, calls in zip(states, per_layer):
            s.lib = _Spy(s.lib, calls)
        st["lib"] = _Spy(st["lib"], model_level)
        try:
            p, m = _prompt()
            for extra in ({}, {"prompt_lookup_num_tokens": None}, {"prompt_lookup_num_tokens": 0}):
                for c in [top, model_level] + per_layer:
                    c.clear()
                dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
                dec.generate(p, m, **dict(SPEC_KW, max_new_tokens=3), **extra)
                assert not [c for c in top + model_level + sum(per_layer, []) if c.startswith("ll_spec")]
                assert [c for c in top if c.startswith("ll_sample_token")] == ["ll_sample_token_topk_ws_bf16"] * 3, top
                assert model_level == ["ll_decode_prologue"] * 2, model_level
                for calls in per_layer:                     # two decode steps of the five-launch layer
                    assert calls == ["ll_gemv_fused_bf16", "ll_decode_attn_rope_bf16", "ll_gemv_fused_bf16", "ll_gemv_fused_bf16",
                                     "ll_gemv_fused_bf16"] * 2, calls
                assert dec.spec_stats is None and dec._spec_bufs is None and dec.mask.shape[1] == 64
            # and with it on the same spies see the two entries
            for c in [top, model_level] + per_layer:
                c.clear()
            GraphedDecoder(llm, use_graph=False, fused_cache=True).generate(p, m, prompt_lookup_num_tokens=4, **dict(SPEC_KW, max_new_tokens=3))
            assert "ll_spec_draft" in top and "ll_spec_verify_bf16" in top and "ll_suffix_prologue" in model_level
        finally:
            for s in states:
                s.lib = s.lib._lib
            st["lib"] = st["lib"]._lib
    finally:
        _restore(llm)
