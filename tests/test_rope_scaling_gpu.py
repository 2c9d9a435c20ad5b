"""Scaled rotary embeddings in the fused decode: llama3 / linear / yarn run the one-launch prologue with their own constants (a
default-rope twin holding the same three constants must decode bit-identically), dynamic NTK picks its frequencies on the device
(ll_decode_prologue_dyn / ll_suffix_prologue_dyn against the plain entry points and against HF's module), and a rotary module that reads
the device on the host is never captured without the fused prologue."""
import warnings

import pytest
import torch

from llamole_amd import e2e
from llamole_amd.llm_decode import GraphedDecoder

pytestmark = pytest.mark.gpu

SCALED = {
    # of the 32 frequencies 4 stay, 23 are divided by 8, the rest are interpolated: all three regimes of llama3
    "llama3": dict(rope_parameters=dict(rope_type="llama3", rope_theta=1e4, factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0,
                                        original_max_position_embeddings=64)),
    "linear": dict(rope_parameters=dict(rope_type="linear", rope_theta=1e4, factor=2.0)),
    # attention_scaling 1.1386: that argument of the prologue
    "yarn": dict(rope_parameters=dict(rope_type="yarn", rope_theta=1e4, factor=4.0, original_max_position_embeddings=64),
                 max_position_embeddings=256),
}
DYNAMIC = dict(rope_parameters=dict(rope_type="dynamic", rope_theta=1e4, factor=2.0), max_position_embeddings=16)
KW = dict(do_sample=False, pad_token_id=0, eos_token_id=[])


def _cases():
    g = torch.Generator().manual_seed(21)
    p2 = torch.randint(5, 2000, (2, 11), generator=g).cuda()
    m2 = torch.ones_like(p2)
    m2[0, :3] = 0                                                     # left padding
    p24 = torch.randint(5, 2000, (24, 12), generator=g).cuda()
    p1 = torch.randint(5, 2000, (1, 20), generator=g).cuda()
    tail = torch.randint(5, 2000, (1, 9), generator=g).cuda()
    return p2, m2, p24, p1, tail


def _decode_all(llm):
    """The four calls of the twin test on one graphed decoder: (tokens, last_logits) each, and the query-token hidden states."""
    p2, m2, p24, p1, tail = _cases()
    dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
    out = {}
    out["pad2"] = (dec.generate(p2, m2, max_new_tokens=8, **KW), dec.last_logits.clone())
    out["rows24"] = (dec.generate(p24, torch.ones_like(p24), max_new_tokens=6, **KW), dec.last_logits.clone())          # _FusedLayer.run64
    hs = []
    for _ in range(2):                                                # eager, then captured and replayed
        toks = dec.generate(p1, torch.ones_like(p1), max_new_tokens=16, **KW)
        hs.append(dec.continue_hidden(tail, 20 + 16 - 9).clone())
    assert torch.equal(hs[0], hs[1]) and dec._graph is not None
    out["suffix"] = (toks, hs[0])
    out["beams"] = (dec.generate(p2, m2, max_new_tokens=6, num_beams=2, **KW), dec.last_logits.clone())
    assert dec.use_graph and dec._beam_graph is not None          # nothing fell back to eager
    return out


@pytest.fixture(scope="module")
def default_outputs():
    from llamole_amd.llm_accel import accelerate_llm, restore_elementwise
    llm = e2e.build_llm("tiny-llama", "cuda", torch.bfloat16)
    try:
        assert accelerate_llm(llm)["decode_prologue_1_launch"]
        return _decode_all(llm)
    finally:
        restore_elementwise(llm)


@pytest.mark.parametrize("kind", ["llama3", "linear", "yarn"])
def test_scaled_model_decodes_fused_and_equals_its_default_rope_twin(kind, default_outputs, monkeypatch):
    from llamole_amd.llm_accel import _FusedLayer, accelerate_llm, fuse_model_decode, restore_elementwise, restore_model_decode
    spec = SCALED[kind]
    llm = e2e.build_llm("tiny-llama", "cuda", torch.bfloat16, **spec)
    twin = e2e.build_llm("tiny-llama", "cuda", torch.bfloat16, **{k: v for k, v in spec.items() if k != "rope_parameters"})
    rot, trot = llm.model.rotary_emb, twin.model.rotary_emb
    assert rot.rope_type == kind and trot.rope_type == "default" and not torch.equal(rot.inv_freq, trot.inv_freq)
    with torch.no_grad():                                             # the scaled model is a default model with other constants
        trot.inv_freq.copy_(rot.inv_freq)
        trot.original_inv_freq.copy_(rot.original_inv_freq)
    trot.attention_scaling = rot.attention_scaling
    calls = []
    for name in ("run64", "run_suffix"):
        orig = getattr(_FusedLayer, name)
        monkeypatch.setattr(_FusedLayer, name, lambda self, *a, _o=orig, _n=name, **k: (calls.append(_n), _o(self, *a, **k))[1])
    try:
        info = accelerate_llm(llm)
        assert info["decode_prologue_1_launch"] and "decode_prologue_declined" not in info
        restore_model_decode(llm)
        assert fuse_model_decode(llm) is True
        got = _decode_all(llm)
        assert "run64" in calls and "run_suffix" in calls             # the 17..64-row layers and the fused query-token forward ran
        assert accelerate_llm(twin)["decode_prologue_1_launch"]
        want = _decode_all(twin)
        for case in ("pad2", "rows24", "suffix", "beams"):
            assert torch.equal(got[case][0], want[case][0]), (kind, case)
            assert torch.equal(got[case][1], want[case][1]), (kind, case)
        # ... and not with the scaling ignored
        assert any(not torch.equal(got[case][0], default_outputs[case][0]) for case in ("pad2", "rows24", "suffix", "beams"))
    finally:
        restore_elementwise(llm)


def _prologue(lib, fn, posid, freq_args, mask2d, pos, B, S, D, maxlen):
    from llamole_amd import _lib
    R = B * S
    cos = torch.zeros(R, D, dtype=torch.bfloat16, device="cuda")
    sin = torch.zeros(R, D, dtype=torch.bfloat16, device="cuda")
    mask = torch.zeros(R, maxlen, dtype=torch.bool, device="cuda")
    shape = (B, D, maxlen) if "suffix" not in fn else (B, S, D, maxlen)
    rc = getattr(lib, fn)(posid.data_ptr(), *freq_args, mask2d.data_ptr(), mask2d.stride(0), pos.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                          mask.data_ptr(), *shape, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, fn)
    torch.cuda.synchronize()
    return cos, sin, mask


@pytest.fixture(scope="module")
def dyn_tables():
    from llamole_amd.rope import dynamic_inv_freq_table
    llm = e2e.build_llm("tiny-llama", "cuda", torch.bfloat16, **DYNAMIC)
    return llm, llm.model.rotary_emb.original_inv_freq.clone(), dynamic_inv_freq_table(llm.config, "cuda", 64)


@pytest.mark.parametrize("positions,row", [((3, 15, 15), None), ((3, 15, 16), 0), ((3, 39, 20), 23), ((63, 2, 2), 47)])
def test_decode_prologue_dyn_selects_the_row_of_the_calls_length(positions, row, dyn_tables):
    """D = 64, maxlen = 64, max_pos = 16: L = max + 1 <= 16 -> inv_freq0, beyond -> table row L - 17; bit-equal to ll_decode_prologue with
    that frequency vector, mask included."""
    from llamole_amd import _lib
    lib = _lib.load()
    _, inv0, table = dyn_tables
    assert table.shape == (48, 32) and table.is_contiguous()
    B, D, maxlen = 3, 64, 64
    posid = torch.tensor(positions, dtype=torch.long, device="cuda").view(B, 1)
    mask2d = torch.ones(B, maxlen, dtype=torch.long, device="cuda")
    mask2d[0, :5] = 0
    mask2d[2, :1] = 0
    pos = torch.tensor([41], dtype=torch.long, device="cuda")
    got = _prologue(lib, "ll_decode_prologue_dyn", posid, (inv0.data_ptr(), table.data_ptr(), 16, table.shape[0], 1.0), mask2d, pos, B, 1, D, maxlen)
    freq = inv0 if row is None else table[row]
    want = _prologue(lib, "ll_decode_prologue", posid, (freq.data_ptr(), 1.0), mask2d, pos, B, 1, D, maxlen)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert got[2][1].tolist() == [j <= 41 for j in range(maxlen)] and not got[2][0, :5].any()
    other = _prologue(lib, "ll_decode_prologue", posid, ((table[5] if row is None else inv0).data_ptr(), 1.0), mask2d, pos, B, 1, D, maxlen)
    assert not torch.equal(other[0], got[0])                         # the comparison can tell the rows apart


@pytest.mark.parametrize("positions,row", [(((10, 11, 12), (13, 14, 15)), None), (((13, 14, 15), (14, 15, 16)), 0), (((30, 31, 32), (5, 6, 7)), 16)])
def test_suffix_prologue_dyn_matches_the_plain_one(positions, row, dyn_tables):
    from llamole_amd import _lib
    lib = _lib.load()
    _, inv0, table = dyn_tables
    B, S, D, maxlen = 2, 3, 64, 64
    posid = torch.tensor(positions, dtype=torch.long, device="cuda")
    mask2d = torch.ones(B, maxlen, dtype=torch.long, device="cuda")
    mask2d[1, :4] = 0
    pos = torch.tensor([33], dtype=torch.long, device="cuda")
    got = _prologue(lib, "ll_suffix_prologue_dyn", posid, (inv0.data_ptr(), table.data_ptr(), 16, table.shape[0], 1.0), mask2d, pos, B, S, D, maxlen)
    freq = inv0 if row is None else table[row]
    want = _prologue(lib, "ll_suffix_prologue", posid, (freq.data_ptr(), 1.0), mask2d, pos, B, S, D, maxlen)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert got[2][2].tolist() == [j <= 35 for j in range(maxlen)]    # row (0, 2): slots up to pos + 2


def test_dynamic_table_rows_are_hfs_function_and_hfs_module_on_the_device(dyn_tables):
    from llamole_amd.rope import dynamic_inv_freq
    llm, inv0, table = dyn_tables
    rot = llm.model.rotary_emb
    x = torch.zeros(1, 1, 4, dtype=torch.bfloat16, device="cuda")
    try:
        for j in range(table.shape[0]):
            L = 17 + j
            assert torch.equal(table[j], dynamic_inv_freq(llm.config, "cuda", torch.tensor(L).cuda())), j
            rot(x, torch.arange(L, device="cuda")[None])              # the live module, grown one length at a time
            assert torch.equal(table[j], rot.inv_freq), j
    finally:
        from llamole_amd.rope import reset_dynamic_rope
        reset_dynamic_rope(llm)
    assert torch.equal(rot.inv_freq, inv0)


def test_prologue_dyn_refuses_a_short_table_and_null_arguments(dyn_tables):
    from llamole_amd import _lib
    lib = _lib.load()
    _, inv0, table = dyn_tables
    B, D, maxlen = 1, 64, 64
    posid = torch.zeros(B, 1, dtype=torch.long, device="cuda")
    mask2d = torch.ones(B, maxlen, dtype=torch.long, device="cuda")
    pos = torch.zeros(1, dtype=torch.long, device="cuda")
    cos = torch.zeros(B, D, dtype=torch.bfloat16, device="cuda")
    sin = torch.zeros_like(cos)
    mask = torch.zeros(B, maxlen, dtype=torch.bool, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(inv, tab, rows, max_pos=16):
        return lib.ll_decode_prologue_dyn(posid.data_ptr(), inv, tab, max_pos, rows, 1.0, mask2d.data_ptr(), maxlen, pos.data_ptr(), cos.data_ptr(),
                                          sin.data_ptr(), mask.data_ptr(), B, D, maxlen, st)
    assert call(inv0.data_ptr(), table.data_ptr(), 47) < 0 and b"table_rows" in lib.ll_last_error()
    assert call(inv0.data_ptr(), None, 48) < 0 and b"table_rows" in lib.ll_last_error()
    assert call(None, table.data_ptr(), 48) < 0 and b"null" in lib.ll_last_error()
    assert lib.ll_suffix_prologue_dyn(posid.data_ptr(), inv0.data_ptr(), table.data_ptr(), 16, 47, 1.0, mask2d.data_ptr(), maxlen, pos.data_ptr(),
                                      cos.data_ptr(), sin.data_ptr(), mask.data_ptr(), B, 1, D, maxlen, st) < 0
    assert b"ll_suffix_prologue_dyn" in lib.ll_last_error()
    assert call(inv0.data_ptr(), table.data_ptr(), 48) == 0          # covered
    assert call(inv0.data_ptr(), None, 0, max_pos=64) == 0           # a cache no longer than max_position_embeddings needs no table
    torch.cuda.synchronize()


def test_dynamic_model_decodes_in_one_graph_like_hfs_module_eager():
    """Prompt of 10 positions, 12 new tokens: the sequence length crosses max_position_embeddings = 16 inside the captured step.  Tokens and
    logits equal the per-op accelerated eager decoder running HF's rotary module from its constructed state; a second, shorter prompt
    replays the same graph and equals a fresh decoder's output."""
    from llamole_amd.llm_accel import (accelerate_elementwise, accelerate_linears, fuse_decoder_layers, fuse_model_decode,
                                       restore_decoder_layers, restore_elementwise, restore_linears, restore_model_decode, use_decode_attention)
    llm = e2e.build_llm("tiny-llama", "cuda", torch.bfloat16, **DYNAMIC)
    g = torch.Generator().manual_seed(5)
    p10 = torch.randint(5, 2000, (2, 10), generator=g).cuda()
    m10 = torch.ones_like(p10)
    m10[0, :2] = 0
    p7 = torch.randint(5, 2000, (2, 7), generator=g).cuda()
    kw = dict(max_new_tokens=12, **KW)
    try:
        accelerate_linears(llm, min_weight_elems=1)
        accelerate_elementwise(llm)
        assert use_decode_attention(llm)
        base = GraphedDecoder(llm, use_graph=False, fused_cache=True)
        ref10, ref10_logits = base.generate(p10, m10, **kw), base.last_logits.clone()
        assert int(llm.model.rotary_emb.max_seq_len_cached) == 21    # HF's module grew on the way
        ref7, ref7_logits = base.generate(p7, torch.ones_like(p7), **kw), base.last_logits.clone()
        assert fuse_decoder_layers(llm) == 2 and fuse_model_decode(llm)
        dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
        assert torch.equal(dec.generate(p10, m10, **kw), ref10) and torch.equal(dec.last_logits, ref10_logits)
        graph = dec._graph
        assert graph is not None and dec.use_graph
        table = llm.model._ll_decode["dyn"]["tables"][64]
        assert table.shape == (48, 32)
        assert torch.equal(dec.generate(p7, torch.ones_like(p7), **kw), ref7) and torch.equal(dec.last_logits, ref7_logits)
        assert dec._graph is graph and llm.model._ll_decode["dyn"]["tables"][64] is table
        fresh = GraphedDecoder(llm, use_graph=True, fused_cache=True)
        assert torch.equal(fresh.generate(p7, torch.ones_like(p7), **kw), ref7) and torch.equal(fresh.last_logits, ref7_logits)
        # the first prompt again after the shorter one: nothing of the earlier calls is left in the rotary state
        assert torch.equal(dec.generate(p10, m10, **kw), ref10) and torch.equal(dec.last_logits, ref10_logits)
    finally:
        restore_model_decode(llm)
        restore_decoder_layers(llm)
        restore_elementwise(llm)
        restore_linears(llm)


LONGROPE = dict(rope_parameters=dict(rope_type="longrope", rope_theta=1e4, short_factor=[1.0] * 32, long_factor=[2.0] * 32,
                                     original_max_position_embeddings=16, factor=4.0), max_position_embeddings=64)


@pytest.mark.parametrize("spec,accel_kw,declined", [(DYNAMIC, dict(model_decode=False), None), (LONGROPE, {}, "rope_type=longrope")])
def test_host_reading_rotary_module_is_never_captured(spec, accel_kw, declined, monkeypatch):
    """dynamic without the fused prologue, and longrope (which the prologue declines): use_graph=True decodes eagerly, warns once, equals
    use_graph=False, and enters no capture."""
    from llamole_amd.llm_accel import accelerate_llm, restore_elementwise
    llm = e2e.build_llm("tiny-llama", "cuda", torch.bfloat16, **spec)
    g = torch.Generator().manual_seed(6)
    prompt = torch.randint(5, 2000, (2, 10), generator=g).cuda()
    mask = torch.ones_like(prompt)
    kw = dict(max_new_tokens=12, **KW)
    try:
        info = accelerate_llm(llm, **accel_kw)
        assert info["decoder_layers_5_launches"] == 2 and not info.get("decode_prologue_1_launch")
        assert info.get("decode_prologue_declined") == declined
        want_dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
        want, want_logits = want_dec.generate(prompt, mask, **kw), want_dec.last_logits.clone()

        def no_capture(*a, **k):
            raise AssertionError("a capture was attempted")
        monkeypatch.setattr(torch.cuda, "graph", no_capture)
        monkeypatch.setattr(torch.cuda, "CUDAGraph", no_capture)
        dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
        with pytest.warns(UserWarning, match="runs eagerly"):
            out = dec.generate(prompt, mask, **kw)
        assert torch.equal(out, want) and torch.equal(dec.last_logits, want_logits)
        assert not dec.use_graph and not dec.graph_suffix and dec._graph is None
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*runs eagerly.*")      # warned once
            assert torch.equal(dec.generate(prompt, mask, num_beams=2, **kw), want_dec.generate(prompt, mask, num_beams=2, **kw))
    finally:
        restore_elementwise(llm)


def test_fused_dynamic_decode_does_not_depend_on_earlier_longer_calls(monkeypatch):
    """The reset before each prefill, on the fused path: after a 22-token call (12 new tokens, HF's prefill module at F(22)) an 18-token call
    -- above max_position_embeddings = 16, so transformers' own reset does not fire: without the decoder's reset HF's prefill would keep
    F(22) while the kernel decodes with F(19) onwards -- equals a fresh model's, plain and beam, on the same captured graph."""
    from llamole_amd import rope
    from llamole_amd.llm_accel import accelerate_llm, restore_elementwise
    g = torch.Generator().manual_seed(8)
    p22 = torch.randint(5, 2000, (2, 22), generator=g).cuda()
    p18 = torch.randint(5, 2000, (2, 18), generator=g).cuda()
    m18 = torch.ones_like(p18)
    m18[1, :1] = 0
    kw = dict(max_new_tokens=12, **KW)
    llm = e2e.build_llm("tiny-llama", "cuda", torch.bfloat16, **DYNAMIC)
    other = e2e.build_llm("tiny-llama", "cuda", torch.bfloat16, **DYNAMIC)
    try:
        assert accelerate_llm(llm)["decode_prologue_1_launch"] and accelerate_llm(other)["decode_prologue_1_launch"]
        dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
        for extra in ({}, dict(num_beams=2)):
            fresh = GraphedDecoder(other, use_graph=True, fused_cache=True)       # `other` has only ever seen the 18-token prompt
            want, want_logits = fresh.generate(p18, m18, **kw, **extra), fresh.last_logits.clone()
            dec.generate(p22, torch.ones_like(p22), **kw, **extra)
            graph = dec._beam_graph if extra else dec._graph
            assert graph is not None
            assert torch.equal(dec.generate(p18, m18, **kw, **extra), want) and torch.equal(dec.last_logits, want_logits), extra
            assert (dec._beam_graph if extra else dec._graph) is graph
        # the comparison sees the reset: without it the prefill keeps the longer call's frequencies
        monkeypatch.setattr(rope, "reset_dynamic_rope", lambda model: False)
        dec.generate(p22, torch.ones_like(p22), **kw, num_beams=2)
        dec.generate(p18, m18, **kw, num_beams=2)
        assert not torch.equal(dec.last_logits, want_logits)
    finally:
        restore_elementwise(llm)


@pytest.mark.parametrize("how", ["default_decoder", "rows_beyond_the_fused_step"])
def test_installed_prologue_that_does_not_serve_the_step_is_not_captured(how, monkeypatch):
    """The prologue is installed on a dynamic model but the step still reaches HF's rotary module: a decoder with default arguments (no
    fused cache append, known before the prefill), and a step the patched forward hands to HF (more rows than it takes; found by the eager
    warm-up step).  One warning, eager decode, the use_graph=False result, no capture."""
    from llamole_amd import llm_accel
    from llamole_amd.llm_accel import accelerate_llm, restore_elementwise
    llm = e2e.build_llm("tiny-llama", "cuda", torch.bfloat16, **DYNAMIC)
    g = torch.Generator().manual_seed(9)
    prompt = torch.randint(5, 2000, (2, 10), generator=g).cuda()
    mask = torch.ones_like(prompt)
    kw = dict(max_new_tokens=12, **KW)
    dec_kw = {} if how == "default_decoder" else dict(fused_cache=True)
    try:
        assert accelerate_llm(llm)["decode_prologue_1_launch"]
        if how == "rows_beyond_the_fused_step":
            monkeypatch.setattr(llm_accel, "MAX_STREAM_ROWS", 1)
        want_dec = GraphedDecoder(llm, use_graph=False, **dec_kw)
        want, want_logits = want_dec.generate(prompt, mask, **kw), want_dec.last_logits.clone()

        def no_capture(*a, **k):
            raise AssertionError("a capture was attempted")
        dec = GraphedDecoder(llm, use_graph=True, **dec_kw)
        with monkeypatch.context() as mp:
            mp.setattr(torch.cuda, "graph", no_capture)
            mp.setattr(torch.cuda, "CUDAGraph", no_capture)
            with pytest.warns(UserWarning, match="run[s]? eagerly"):
                out = dec.generate(prompt, mask, **kw)
            assert torch.equal(out, want) and torch.equal(dec.last_logits, want_logits)
            assert dec._graph is None
            with warnings.catch_warnings():
                warnings.filterwarnings("error", message=".*eagerly.*")           # warned once
                assert torch.equal(dec.generate(prompt, mask, **kw), want)
        if how == "default_decoder":
            assert not dec.use_graph and not dec.graph_suffix                     # for good: it holds for every call of this decoder
        else:
            # only this (batch, cache length) shape: a later call that the prologue serves is captured
            assert dec.use_graph and dec._key in dec._eager_keys
            one = prompt[:1].contiguous()
            eager1 = want_dec.generate(one, mask[:1], **kw)
            assert torch.equal(dec.generate(one, mask[:1], **kw), eager1) and dec._graph is not None and dec._key not in dec._eager_keys
    finally:
        restore_elementwise(llm)


def test_query_token_forward_of_a_dynamic_model(monkeypatch):
    """GraphedDecoder.continue_hidden on a dynamic model: 9 positions 13..21 (they straddle max_position_embeddings = 16, L = 22) run on
    the five-launch layers behind ll_suffix_prologue_dyn, eager and as a replayed graph.  With the fused suffix switched off the same call
    reaches HF's rotary module: its first, eager call marks the shape and no later call captures it.  Both give the same hidden states
    within the bound tests/test_llm_decode.py uses for the fused against the op-by-op query forward (3e-2 of the largest value: the MFMA
    Linears accumulate in another order)."""
    from llamole_amd.llm_accel import _FusedLayer, accelerate_llm, restore_elementwise
    llm = e2e.build_llm("tiny-llama", "cuda", torch.bfloat16, **DYNAMIC)
    g = torch.Generator().manual_seed(12)
    prompt = torch.randint(5, 2000, (1, 10), generator=g).cuda()
    tail = torch.randint(5, 2000, (1, 9), generator=g).cuda()
    kw = dict(max_new_tokens=12, **KW)
    calls = []
    orig = _FusedLayer.run_suffix
    monkeypatch.setattr(_FusedLayer, "run_suffix", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    try:
        assert accelerate_llm(llm)["decode_prologue_1_launch"]
        outs = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("LLAMOLE_FUSED_SUFFIX", mode)
            dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
            hs = []
            for i in range(3):                                        # eager, captured (fused) or still eager (HF's module), again
                dec.generate(prompt, torch.ones_like(prompt), **kw)
                hs.append(dec.continue_hidden(tail, 10 + 12 - 9).clone())
                state = dec._side_graphs[("suffix", 1, 9)]
                if mode == "0":
                    assert state == "eager"
                else:
                    assert state == "seen" if i == 0 else isinstance(state, tuple)
            assert torch.equal(hs[0], hs[1]) and torch.equal(hs[0], hs[2])
            assert dec._graph is not None                             # the decode step itself stays graphed
            outs[mode] = hs[0].float()
        assert len(calls) == 2 * llm.config.num_hidden_layers        # fused: the eager call and the capture
        assert (outs["0"] - outs["1"]).abs().max() <= 3e-2 * outs["0"].abs().max()
    finally:
        restore_elementwise(llm)
