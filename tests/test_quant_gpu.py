"""quantization_bit on the GPU: the device quantiser against its torch restatement, the packed-weight decode kernels
(ll_gemv_fused_wq, ll_linear_rows16_wq) on known answers, exact data and against torch, and the quantised decode through the fused
layers, the captured graph, the penalty / beam options, the weight refresh and `main.py eval`."""
import json

import pytest
import torch
import torch.nn.functional as F

from llamole_amd import e2e
from llamole_amd.llm_decode import GraphedDecoder
from llamole_amd.llm_quant import E2M1_VALUES, decode_codes, mx_round

pytestmark = pytest.mark.gpu

BITS = (8, 4)


def _lib():
    from llamole_amd import _lib as L
    return L, L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _quantize(w, bits, want_dq=True):
    """bf16 [N, K] on the device -> (packed uint8 buffer, dequantised bf16 matrix) through ll_wq_quantize_bf16."""
    L, lib = _lib()
    N, K = w.shape
    nbytes = int(lib.ll_wq_bytes(N, K, bits))
    assert nbytes == N * K * bits // 8 + N * K // 32
    packed = torch.full((nbytes,), 0xEE, dtype=torch.uint8, device="cuda")
    dq = torch.full_like(w, float("nan")) if want_dq else None
    L.check(lib.ll_wq_quantize_bf16(w.data_ptr(), w.stride(0), N, K, bits, packed.data_ptr(), dq.data_ptr() if want_dq else None, K, _stream()),
            "ll_wq_quantize_bf16")
    return packed, dq


def _dequantize(packed, N, K, bits):
    L, lib = _lib()
    out = torch.full((N, K), float("nan"), dtype=torch.bfloat16, device="cuda")
    L.check(lib.ll_wq_dequantize_bf16(packed.data_ptr(), N, K, bits, out.data_ptr(), K, _stream()), "ll_wq_dequantize_bf16")
    return out


def _gemv(kind, x, packed, bits, N, K, epi=0, bias=None, nw=None, res=None, eps=1e-6):
    L, lib = _lib()
    fn = lib.ll_gemv_fused_wq if kind == "gemv" else lib.ll_linear_rows16_wq
    M = x.shape[0]
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
    L.check(fn(x.data_ptr(), x.stride(0), packed.data_ptr(), bits, bias.data_ptr() if bias is not None else None,
               nw.data_ptr() if nw is not None else None, eps, res.data_ptr() if res is not None else None, N, out.data_ptr(), N, M, N, K, epi,
               _stream()), kind)
    return out


# ------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("K", [256, 3584, 18944])
def test_device_quantiser_equals_mx_round(bits, K):
    """ll_wq_quantize_bf16 followed by ll_wq_dequantize_bf16 equals mx_round exactly, on values; so does the dequantised matrix the
    quantiser writes itself, also when it aliases W.  N is not a multiple of any tile."""
    N = 37
    g = torch.Generator().manual_seed(K + bits)
    w = (0.02 * torch.randn(N, K, generator=g)).bfloat16()
    w[3, 40] = 1.75                       # one outlier in a block
    w[5, 64:96] = 0                       # an all-zero block
    w[7, 0:32] = w[7, 0:32] * 2.0 ** -20  # a block of tiny values
    w[9, 32:64] = w[9, 32:64] * 2.0 ** 30
    want, want_sb = mx_round(w, bits)
    want = want.bfloat16()
    wd = w.cuda()
    packed, dq = _quantize(wd, bits)
    assert torch.equal(dq.cpu(), want)
    assert torch.equal(_dequantize(packed, N, K, bits).cpu(), want)
    alias = wd.clone()
    L, lib = _lib()
    packed2 = torch.empty_like(packed)
    L.check(lib.ll_wq_quantize_bf16(alias.data_ptr(), K, N, K, bits, packed2.data_ptr(), alias.data_ptr(), K, _stream()), "ll_wq_quantize_bf16")
    assert torch.equal(alias.cpu(), want) and torch.equal(packed2, packed)
    only_dq = wd.clone()                  # the install path: no packed output, W rounded in place
    L.check(lib.ll_wq_quantize_bf16(only_dq.data_ptr(), K, N, K, bits, None, only_dq.data_ptr(), K, _stream()), "ll_wq_quantize_bf16")
    assert torch.equal(only_dq.cpu(), want)
    assert lib.ll_wq_bytes(N, K + 8, bits) == -1 and lib.ll_wq_bytes(N, K, 3) == -1
    assert lib.ll_wq_quantize_bf16(wd.data_ptr(), K, N, K - 8, bits, packed.data_ptr(), None, 0, _stream()) == -1
    assert lib.ll_wq_quantize_bf16(wd.data_ptr(), K, N, K, 6, packed.data_ptr(), None, 0, _stream()) == -1


def _all_codes_matrix(bits):
    """Rows that hold every element code under the scale bytes 120, 127 and 133: each block of 32 carries the format's largest value,
    which pins its scale, so quantising the matrix must reproduce exactly these codes."""
    if bits == 8:
        codes = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8)        # 254 without the two NaN codes
        per, vmax = 31, 448.0
    else:
        codes = torch.cat([torch.arange(16), torch.arange(15, -1, -1)]).to(torch.uint8)              # both nibble positions see every code
        per, vmax = 16, 6.0
    vals = decode_codes(codes, bits)
    blocks = []
    for i in range(0, len(vals), per):
        b = torch.zeros(32)
        chunk = vals[i:i + per]
        b[:len(chunk)] = chunk
        b[31] = vmax
        blocks.append(b)
    row = torch.cat(blocks)
    sbs = (120, 127, 133)
    w = torch.stack([row * 2.0 ** (sb - 127) for sb in sbs])
    return w.bfloat16(), sbs


@pytest.mark.parametrize("bits", BITS)
def test_known_answers_on_the_device(bits):
    """Every code under several scale bytes: ll_wq_dequantize_bf16 returns code * 2^e exactly, and both GEMV kernels, given one-hot x rows,
    read the same weights back exactly (their own in-register conversion and their use of the scale operand)."""
    w, sbs = _all_codes_matrix(bits)
    assert torch.equal(w.float(), w.float().bfloat16().float())
    dq, sb = mx_round(w, bits)
    assert torch.equal(dq, w.float()) and all((sb[i] == s).all() for i, s in enumerate(sbs))       # the scales are pinned, rounding is the identity
    N, K = w.shape
    wd = w.cuda()
    packed, dq_dev = _quantize(wd, bits)
    assert torch.equal(dq_dev, wd) and torch.equal(_dequantize(packed, N, K, bits), wd)
    for kind, M in (("gemv", 4), ("rows16", 16)):
        for k0 in range(0, K, M):
            ks = [min(k0 + m, K - 1) for m in range(M)]
            x = torch.zeros(M, K, dtype=torch.bfloat16, device="cuda")
            x[torch.arange(M), torch.tensor(ks)] = 1.0
            out = _gemv(kind, x, packed, bits, N, K)
            assert torch.equal(out, wd[:, ks].t().contiguous()), (kind, k0)


# ------------------------------------------------------------------------------------------------ exact data
def _grid_weights(bits, N, K, g):
    """Multiples of 0.5 up to 6 that lie on the format's grid, random signs: all of them for E4M3, the eight E2M1 values at 4 bits."""
    if bits == 8:
        mag = torch.randint(0, 13, (N, K), generator=g).float() * 0.5
    else:
        mag = torch.tensor(E2M1_VALUES)[torch.randint(0, 8, (N, K), generator=g)]
    sign = torch.randint(0, 2, (N, K), generator=g).float() * 2 - 1
    return (mag * sign).bfloat16()


WQ_GEOMS = {8: ((0, 0, 0), (128, 4, 1), (128, 8, 8), (256, 4, 2), (256, 8, 4)), 4: ((0, 0, 0), (128, 4, 1), (128, 8, 8), (128, 4, 2))}


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("kind,M", [("gemv", 1), ("gemv", 2), ("gemv", 3), ("gemv", 4),
                                    ("rows16", 1), ("rows16", 5), ("rows16", 8), ("rows16", 13), ("rows16", 16)])
def test_kernels_on_exact_data(bits, kind, M):
    """Lane maps on exact, asymmetric data: grid-valued weights (rounding is the identity -- asserted), small-integer x, K = 4608 with
    |w| <= 6 and |x| <= 4: every partial sum is an exact f32 (below 2^24 in steps of 0.5), so the output must equal the f32 torch product
    rounded to bf16 whatever the accumulation order.  Plain and residual epilogues; every geometry of the MFMA kernel."""
    L, lib = _lib()
    K, N = 4608, 203
    g = torch.Generator().manual_seed(100 * bits + M)
    w = _grid_weights(bits, N, K, g)
    assert torch.equal(mx_round(w, bits)[0], w.float())
    x = torch.randint(-4, 5, (M, K), generator=g).bfloat16()
    res = torch.randint(-8, 9, (M, N), generator=g).bfloat16()
    acc = x.float() @ w.float().t()
    want0 = acc.bfloat16()
    want1 = (res.float() + want0.float()).bfloat16()
    wd, xd, rd = w.cuda(), x.cuda(), res.cuda()
    packed, dq = _quantize(wd, bits)
    assert torch.equal(dq, wd)
    for geom in (WQ_GEOMS[bits] if kind == "rows16" else ((0, 0, 0),)):
        lib.ll_set_wq_geometry(*geom)
        try:
            got0 = _gemv(kind, xd, packed, bits, N, K)
            got1 = _gemv(kind, xd, packed, bits, N, K, epi=1, res=rd)
        finally:
            lib.ll_set_wq_geometry(0, 0, 0)
        assert torch.equal(got0.cpu(), want0), geom
        assert torch.equal(got1.cpu(), want1), geom


# ------------------------------------------------------------------------------------------------ epilogues against torch
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_gemv_fused_wq_epilogues_vs_torch(bits, M):
    """The cases and tolerances of test_gemv_fused_epilogues_vs_torch (tests/test_llm_decode.py), the reference computed from the
    dequantised weights: the operands are the same bf16 numbers, the accumulation order is this kernel's own."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(M)
    K, N = 4608, 1003
    x = torch.randn(M, K, generator=g).bfloat16().cuda()
    w0 = (torch.randn(2 * N, K, generator=g) * 0.02).bfloat16().cuda()
    bias = torch.randn(2 * N, generator=g).float().cuda()
    nw = (1 + 0.1 * torch.randn(K, generator=g)).bfloat16().cuda()
    res = torch.randn(M, N, generator=g).bfloat16().cuda()
    eps = 1e-6
    packed2, w = _quantize(w0, bits)                      # [2N, K]: gate rows then up rows
    packed1, w1 = _quantize(w0[:N].contiguous(), bits)     # [N, K]
    assert torch.equal(w1, w[:N])

    def rms(v):
        f = v.float()
        f = f * torch.rsqrt(f.pow(2).mean(-1, keepdim=True) + eps)
        return nw * f.to(torch.bfloat16)

    for norm in (False, True):
        xin = rms(x) if norm else x
        for use_bias in (False, True):
            b = bias if use_bias else torch.zeros_like(bias)
            full = (xin.float() @ w.float().t() + b).to(torch.bfloat16)
            kw = dict(bias=bias if use_bias else None, nw=nw if norm else None, eps=eps)
            got = _gemv("gemv", x, packed1, bits, N, K, epi=0, **kw)
            torch.testing.assert_close(got.float(), full[:, :N].float(), rtol=2e-2, atol=2e-2)
            got = _gemv("gemv", x, packed1, bits, N, K, epi=1, res=res, **kw)
            torch.testing.assert_close(got.float(), (res + full[:, :N]).float(), rtol=2e-2, atol=3e-2)
            got = _gemv("gemv", x, packed2, bits, N, K, epi=2, **kw)
            torch.testing.assert_close(got.float(), (F.silu(full[:, :N]) * full[:, N:]).float(), rtol=3e-2, atol=3e-2)
    s, o = _stream(), res.data_ptr()
    assert lib.ll_gemv_fused_wq(x.data_ptr(), K, packed1.data_ptr(), bits, None, None, eps, None, 0, o, N, 5, N, K, 0, s) == -1       # M out of range
    assert lib.ll_gemv_fused_wq(x.data_ptr(), K, packed1.data_ptr(), bits, None, None, eps, None, 0, o, N, M, N, K - 8, 0, s) == -1   # K % 32
    assert lib.ll_gemv_fused_wq(x.data_ptr(), K, packed1.data_ptr(), bits, None, None, eps, None, 0, o, N, M, N, K, 1, s) == -1       # no residual
    assert lib.ll_gemv_fused_wq(x.data_ptr(), K, packed1.data_ptr(), 6, None, None, eps, None, 0, o, N, M, N, K, 0, s) == -1          # bits


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("M", [5, 8, 13, 16])
def test_linear_rows16_wq_epilogues_vs_torch(bits, M):
    """The cases and tolerances of test_linear_rows16_epilogues_vs_torch on packed weights, every geometry the launcher may pick; N not a
    multiple of the 16-row tile, K not a multiple of a block; and its error behaviour."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(M)
    s = _stream()
    eps = 1e-6
    for K, N in ((4640, 1003), (96, 24), (18944, 520)):
        x = torch.randn(M, K, generator=g).bfloat16().cuda()
        w0 = (torch.randn(2 * N, K, generator=g) * 0.02).bfloat16().cuda()
        bias = torch.randn(2 * N, generator=g).float().cuda()
        nw = (1 + 0.1 * torch.randn(K, generator=g)).bfloat16().cuda()
        res = torch.randn(M, N, generator=g).bfloat16().cuda()
        packed2, w = _quantize(w0, bits)
        packed1, _ = _quantize(w0[:N].contiguous(), bits)

        def rms(v):
            f = v.float()
            f = f * torch.rsqrt(f.pow(2).mean(-1, keepdim=True) + eps)
            return nw * f.to(torch.bfloat16)

        for geom in WQ_GEOMS[bits]:
            for norm in (False, True):
                xin = rms(x) if norm else x
                for use_bias in ((False, True) if geom == (0, 0, 0) else (False,)):
                    b = bias if use_bias else torch.zeros_like(bias)
                    full = (xin.float() @ w.float().t() + b).to(torch.bfloat16)
                    want = {0: full[:, :N], 1: res + full[:, :N], 2: F.silu(full[:, :N]) * full[:, N:]}
                    for epi in (0, 1, 2):
                        if geom[0] and geom[1] * (3 if epi == 2 else 2) * 16 * (geom[0] * 16 // bits + 16) > 160 * 1024:
                            continue                       # this geometry's LDS images exceed a CU's 160 KB: the launcher refuses it
                        lib.ll_set_wq_geometry(*geom)
                        try:
                            out = _gemv("rows16", x, packed2 if epi == 2 else packed1, bits, N, K, epi=epi, bias=bias if use_bias else None,
                                        nw=nw if norm else None, res=res if epi == 1 else None, eps=eps)
                        finally:
                            lib.ll_set_wq_geometry(0, 0, 0)
                        scale = want[epi].float().abs().max().item()
                        torch.testing.assert_close(out.float(), want[epi].float(), rtol=3e-2, atol=max(3e-2, 0.01 * scale))
    o = res.data_ptr()
    assert lib.ll_linear_rows16_wq(x.data_ptr(), K, packed1.data_ptr(), bits, None, None, eps, None, 0, o, N, 17, N, K, 0, s) == -1      # M out of range
    assert lib.ll_linear_rows16_wq(x.data_ptr(), K, packed1.data_ptr(), bits, None, None, eps, None, 0, o, N, M, N, K - 8, 0, s) == -1   # K % 32
    assert lib.ll_linear_rows16_wq(x.data_ptr(), K, packed1.data_ptr(), bits, None, None, eps, None, 0, o, N, M, N, K, 1, s) == -1       # no residual
    assert lib.ll_linear_rows16_wq(x.data_ptr(), K, packed1.data_ptr(), 3, None, None, eps, None, 0, o, N, M, N, K, 0, s) == -1          # bits


# ------------------------------------------------------------------------------------------------ the quantised decode
def _restore(llm):
    from llamole_amd.llm_accel import restore_decoder_layers, restore_elementwise, restore_linears, restore_model_decode
    restore_model_decode(llm)
    restore_decoder_layers(llm)
    restore_elementwise(llm)
    restore_linears(llm)


def _count_wq(llm):
    """Call counter on the packed-code route of layer 0: [token rows of every call]."""
    calls = []
    st0 = llm.model.layers[0]._ll_fused
    orig = st0._gemv_wq
    st0._gemv_wq = lambda x, *a, **k: (calls.append(x.shape[0]), orig(x, *a, **k))[1]
    return calls


def _prompts(rows, seed):
    g = torch.Generator().manual_seed(seed)
    prompt = torch.randint(5, 1000, (rows, 12), generator=g).cuda()
    mask = torch.ones_like(prompt)
    if rows > 1:
        mask[1, :4] = 0
        mask[rows - 1, :7] = 0
    return prompt, mask


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("rows", [1, 2, 6, 16])
def test_quantised_decode_step_through_the_fused_layers(bits, rows):
    """Prefill + one decode step of a quantised tiny model: the packed-code layers against the same model with the packed route switched
    off (the bf16 five-launch layers on the dequantised weights).  Logits within 0.03 * max|logit|, the appended K/V within 5e-2 -- the
    limits of test_fused_decoder_layers_batched_rows.  Tokens are not compared across the routes: the random tiny models have top-2
    logit margins down to 1e-4, below what reordered sums change."""
    from llamole_amd.llm_accel import accelerate_llm, set_packed_route
    llm = e2e.build_llm("tiny", "cuda", torch.bfloat16)
    w0 = llm.model.layers[1].mlp.gate_proj.weight.clone()
    prompt, mask = _prompts(rows, rows)
    kw = dict(max_new_tokens=2, do_sample=False, pad_token_id=0, eos_token_id=[2047])
    try:
        info = accelerate_llm(llm, quantization_bit=bits)
        q = info["quantization"]
        L = llm.config.num_hidden_layers
        assert q["bits"] == bits and q["modules"] == 7 * L and q["packed_layers"] == L and q["bf16_layers"] == 0
        assert set(q["packed_routes"]) == {"qkv", "o", "gate_up", "down"} and q["packed_bytes"] * 64 == q["bf16_bytes"] * (4 * bits + 1)
        assert torch.equal(llm.model.layers[1].mlp.gate_proj.weight.cpu(), mx_round(w0.cpu(), bits)[0].bfloat16())     # module.weight holds the dequantised values
        assert set_packed_route(llm, False) == L
        calls = _count_wq(llm)
        base = GraphedDecoder(llm, use_graph=False, fused_cache=True)
        base.generate(prompt, mask, **kw)
        assert not calls
        ref_logits = base.last_logits.float().clone()
        ref_kv = [(l.keys.clone(), l.values.clone()) for l in base.cache.layers]
        set_packed_route(llm, True)
        from llamole_amd import llm_accel
        saved = dict(llm_accel.WQ_ROUTES)
        llm_accel.WQ_ROUTES.update(llm_accel.all_packed_routes())      # the test covers both kernels whatever the speed routing switched on
        try:
            dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
            dec.generate(prompt, mask, **kw)
        finally:
            llm_accel.WQ_ROUTES.update(saved)
        assert calls == [rows] * 4                                      # q|k|v, o_proj, gate|up, down_proj of the one decode step
        scale = ref_logits.abs().max().item()
        assert (dec.last_logits.float() - ref_logits).abs().max().item() <= 0.03 * scale
        P = prompt.shape[1]
        for (k, v), l in zip(ref_kv, dec.cache.layers):
            torch.testing.assert_close(l.keys[:, :, P].float(), k[:, :, P].float(), rtol=5e-2, atol=5e-2)
            torch.testing.assert_close(l.values[:, :, P].float(), v[:, :, P].float(), rtol=5e-2, atol=5e-2)
    finally:
        _restore(llm)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("rows", [2, 6])
def test_captured_quantised_decode_equals_the_eager_one(bits, rows, monkeypatch):
    from llamole_amd import llm_accel
    from llamole_amd.llm_accel import accelerate_llm
    monkeypatch.setattr(llm_accel, "WQ_ROUTES", llm_accel.all_packed_routes())
    llm = e2e.build_llm("tiny", "cuda", torch.bfloat16)
    prompt, mask = _prompts(rows, 3)
    kw = dict(max_new_tokens=8, do_sample=False, pad_token_id=0, eos_token_id=[2047])
    try:
        accelerate_llm(llm, quantization_bit=bits)
        calls = _count_wq(llm)
        eager = GraphedDecoder(llm, use_graph=False, fused_cache=True)
        toks = eager.generate(prompt, mask, **kw)
        assert calls
        gr = GraphedDecoder(llm, use_graph=True, fused_cache=True)
        assert torch.equal(gr.generate(prompt, mask, **kw), toks) and torch.equal(gr.last_logits, eager.last_logits)
        assert torch.equal(gr.generate(prompt, mask, **kw), toks) and torch.equal(gr.last_logits, eager.last_logits)      # replay
        gen = torch.Generator(device="cuda").manual_seed(5)
        skw = dict(max_new_tokens=12, do_sample=True, temperature=0.6, top_p=0.9, pad_token_id=0, generator=gen)
        s1 = gr.generate(prompt, mask, **skw)
        gen.manual_seed(5)
        s2 = gr.generate(prompt, mask, **skw)
        assert torch.equal(s1, s2)
    finally:
        _restore(llm)


@pytest.mark.parametrize("bits", BITS)
def test_penalty_and_beams_on_a_quantised_model(bits, monkeypatch):
    """repetition_penalty = 1.3 and num_beams = 2 on a quantised model: each equals its own sampler="torch" run on that model, as the
    penalty and beam tests assert on the bf16 one."""
    from llamole_amd import llm_accel
    from llamole_amd.llm_accel import accelerate_llm
    monkeypatch.setattr(llm_accel, "WQ_ROUTES", llm_accel.all_packed_routes())
    llm = e2e.build_llm("tiny", "cuda", torch.bfloat16)
    prompt, mask = _prompts(2, 7)
    try:
        accelerate_llm(llm, quantization_bit=bits)
        calls = _count_wq(llm)
        kw = dict(max_new_tokens=12, do_sample=False, pad_token_id=0, eos_token_id=[2047], repetition_penalty=1.3)
        got = GraphedDecoder(llm, use_graph=True, fused_cache=True).generate(prompt, mask, **kw)
        eager = GraphedDecoder(llm, use_graph=False, fused_cache=True).generate(prompt, mask, **kw)
        ref = GraphedDecoder(llm, use_graph=False, fused_cache=True, sampler="torch").generate(prompt, mask, **kw)
        assert torch.equal(got, eager) and torch.equal(got, ref)
        kw = dict(max_new_tokens=12, do_sample=False, pad_token_id=0, eos_token_id=[2047, 7, 11], num_beams=2)
        a = GraphedDecoder(llm, use_graph=True, fused_cache=True).generate(prompt, mask, **kw)
        b = GraphedDecoder(llm, use_graph=False, fused_cache=True).generate(prompt, mask, **kw)
        c = GraphedDecoder(llm, use_graph=True, fused_cache=True, sampler="torch").generate(prompt, mask, **kw)
        assert torch.equal(a, b) and torch.equal(a, c)
        assert calls and 4 in calls                                     # two beams per prompt: four rows on the MFMA stream
    finally:
        _restore(llm)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("rows", [2, 6])
def test_packed_codes_follow_their_sources(bits, rows, monkeypatch):
    """After an in-place update of the layer weights the same decoder and the same graph object decode exactly like a freshly built,
    freshly quantised copy of the updated model: the changed weights are rounded again in place, the concatenated copies rebuilt from
    them and the packed codes re-quantised in their own storage."""
    from llamole_amd import llm_accel
    from llamole_amd.llm_accel import accelerate_llm, refresh_weight_copies
    monkeypatch.setattr(llm_accel, "WQ_ROUTES", llm_accel.all_packed_routes())
    llm = e2e.build_llm("tiny", "cuda", torch.bfloat16)
    fresh = None
    try:
        accelerate_llm(llm, quantization_bit=bits)
        g = torch.Generator().manual_seed(2)
        prompt = torch.randint(5, 2000, (rows, 12), generator=g).cuda()
        kw = dict(max_new_tokens=6, do_sample=False, pad_token_id=0, eos_token_id=[])
        dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
        before = dec.generate(prompt, torch.ones_like(prompt), **kw)
        graph = dec._graph
        ptrs = [p.t.data_ptr() for p in llm.model.layers[0]._ll_fused.pq]
        assert refresh_weight_copies(llm) == 0
        with torch.no_grad():
            for n, p in llm.named_parameters():
                if any(t in n for t in ("q_proj", "k_proj", "gate_proj", "up_proj", "o_proj", "down_proj", "lm_head")):
                    p.mul_(1.5)
                    p.add_(0.01)
        updated = {k: v.clone() for k, v in llm.state_dict().items()}
        after = dec.generate(prompt, torch.ones_like(prompt), **kw)      # refreshes in place, replays the same captured graph
        assert dec._graph is graph and [p.t.data_ptr() for p in llm.model.layers[0]._ll_fused.pq] == ptrs
        assert refresh_weight_copies(llm) == 0
        w = llm.model.layers[0].self_attn.o_proj.weight
        assert torch.equal(w.cpu(), mx_round(updated["model.layers.0.self_attn.o_proj.weight"].cpu(), bits)[0].bfloat16())
        fresh = e2e.build_llm("tiny", "cuda", torch.bfloat16)
        fresh.load_state_dict(updated)
        accelerate_llm(fresh, quantization_bit=bits)
        ref = GraphedDecoder(fresh, use_graph=False, fused_cache=True).generate(prompt, torch.ones_like(prompt), **kw)
        assert torch.equal(after, ref) and not torch.equal(after, before)
    finally:
        _restore(llm)
        if fresh is not None:
            _restore(fresh)


@pytest.mark.parametrize("bits", [8, 4, 3])
def test_main_eval_with_quantization_bit(bits, tmp_path, monkeypatch, capsys):
    from llamole_amd import eval as ev
    from llamole_amd import synth
    from llamole_amd.modeling_llamole import SPECIAL_TOKENS
    from tests.test_eval_gpu import RECORD_FIELDS, _script_chemistry
    _script_chemistry(monkeypatch)
    cfg = synth.write_eval_fixture(str(tmp_path), SPECIAL_TOKENS)
    torch.manual_seed(0)
    ov = {"retro_iterations": 3, "retro_max_planning_time": 20, "quantization_bit": bits}
    if bits == 3:
        with pytest.raises(ValueError, match="4-bit or 8-bit"):
            ev.run_eval(cfg, overrides=ov)
        return
    try:
        out = ev.run_eval(cfg, overrides=ov)
    finally:
        from transformers.models.qwen2 import modeling_qwen2 as mq
        if hasattr(mq.apply_rotary_pos_emb, "_ll_orig"):
            mq.apply_rotary_pos_emb = mq.apply_rotary_pos_emb._ll_orig
    assert [r["qa_idx"] for r in out["results"]] == [0, 1, 2, 3, 4]
    for r in out["results"]:
        assert set(r) == RECORD_FIELDS and r["llm_smiles"].startswith("M")
    printed = capsys.readouterr().out
    accel = json.loads([l for l in printed.splitlines() if l.startswith('{"llm_acceleration"')][0])["llm_acceleration"]
    q = accel["quantization"]
    assert q["bits"] == bits and q["modules"] == 14 and q["packed_layers"] == 2 and accel.get("decoder_layers_5_launches") == 2
