"""The decode attention kernels against the float64 reference of tests/attn_reference.py: ll_decode_attn_rope_bf16 (per-head and grouped
form), ll_decode_attn_bf16, ll_suffix_prologue + ll_suffix_attn_rope_bf16 and ll_kv_append_bf16 through the C ABI, at the tile edges (key
255 / 256, first and last slot), with left padding, fully masked rows, loose row strides, NaN in every cache slot the call may not read, up
to the 16384 keys the entry points accept.  Every output element within 2^-8 |ref| + 2^-11 sum_j p_j |v_j| (derived in attn_reference.py;
tests/test_decode_attention_reference_cpu.py shows what it lets through and what not); the cache compared bit for bit.

Largest err / bound measured on an MI355X (-s prints them): ll_decode_attn_rope_bf16 per-head 0.885, grouped 0.885, ll_decode_attn_bf16
0.871, ll_suffix_attn_rope_bf16 0.878; 0.23 for all three at 12032 .. 16384 keys.  A plain f32 evaluation of the same inputs reaches 0.885 too:
half a bf16 ulp is most of the bound."""
import ctypes as C

import pytest
import torch

from tests import attn_reference as R

pytestmark = pytest.mark.gpu

I3, I2 = C.c_int64 * 3, C.c_int64 * 2
WORST = {}


@pytest.fixture(scope="module")
def lib():
    from llamole_amd import _lib
    yield _lib.load()
    for entry, r in sorted(WORST.items()):
        print(f"\nlargest err / bound, {entry}: {r:.3f}")


def _check(rc, what):
    from llamole_amd import _lib
    _lib.check(rc, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _nan(*shape):
    return torch.full(shape, R.NAN, dtype=R.BF, device="cuda")


def _within(entry, c, out, ref, absref):
    assert torch.isfinite(out.float()).all(), (entry, c.variant, "the output holds NaN / inf")
    r = R.err_over_bound(out, ref, absref)
    WORST[entry] = max(WORST.get(entry, 0.0), r)
    assert r <= 1.0, (entry, c.variant, r)


def _same_bits(entry, c, got, want, what):
    assert torch.equal(_bits(got), _bits(want)), (entry, c.variant, what)


# ------------------------------------------------------------------------------------------------------------------ ll_decode_attn_rope_bf16
def run_decode(lib, c, Kc, Vc):
    """one ll_decode_attn_rope_bf16 call on the case's inputs; returns out [B, nh*D]"""
    qkv, cos, sin, mask = c.qkv.cuda(), c.cos.cuda(), c.sin.cuda(), c.mask.cuda()
    pos = torch.tensor([c.pos], dtype=torch.long, device="cuda")
    out = _nan(c.B, c.nh * c.D)
    _check(lib.ll_decode_attn_rope_bf16(qkv.data_ptr(), c.ld_qkv, cos.data_ptr(), sin.data_ptr(), c.cs_stride, Kc.data_ptr(), Vc.data_ptr(),
                                        pos.data_ptr(), mask.data_ptr(), c.mask_stride, out.data_ptr(), c.B, c.nh, c.nkv, c.maxlen, c.D,
                                        c.scale, _stream()), "ll_decode_attn_rope_bf16")
    torch.cuda.synchronize()
    return out


def check_decode(lib, c, entry):
    keep = c.visible.clone()
    keep[:, c.pos] = False                                       # the stale row at *pos
    Kp, Vp = R.poison(c, c.K0, c.V0, keep)
    Kc, Vc = Kp.cuda(), Vp.cuda()
    out = run_decode(lib, c, Kc, Vc)
    inputs, (k_rot, v_new) = R.decode_expected(c)
    ref, absref = R.reference(c, inputs)
    Kp[:, :, c.pos], Vp[:, :, c.pos] = k_rot, v_new              # the appended row, every other slot as it was
    _same_bits(entry, c, Kc, Kp, "key cache")
    _same_bits(entry, c, Vc, Vp, "value cache")
    out = out.cpu().view(c.B, c.nh, 1, c.D)
    _within(entry, c, out, ref, absref)
    if c.maxlen == 1:                                            # one key: the new value row itself
        want = v_new.repeat_interleave(c.nh // c.nkv, dim=1) * c.visible[:, :1, None]
        assert torch.equal(out[:, :, 0].float(), want.float())
    return out


@pytest.mark.parametrize("maxlen,pos", R.POSITIONS)
@pytest.mark.parametrize("D,nh,nkv", R.GEOMETRIES)
def test_decode_attn_rope_per_head(lib, D, nh, nkv, maxlen, pos):
    """three sequences (full, left-padded, fully masked -> zeros): the per-head kernel"""
    for variant in R.decode_variants(maxlen, pos):
        for bcast in ((True, False) if variant == "plain" else (False,)):
            out = check_decode(lib, R.decode_case(D, nh, nkv, maxlen, pos, variant, bcast=bcast), "ll_decode_attn_rope_bf16 per-head")
            assert float(out[2].float().abs().max()) == 0.0


@pytest.mark.parametrize("maxlen,pos", R.GROUPED_POSITIONS)
@pytest.mark.parametrize("D,nh,nkv", R.GROUPED_GEOMETRIES)
def test_decode_attn_rope_grouped(lib, D, nh, nkv, maxlen, pos):
    """seventeen sequences, group sizes 2 / 4 / 7: one workgroup per (KV head, sequence), all six instances"""
    for variant in R.decode_variants(maxlen, pos):
        check_decode(lib, R.decode_case(D, nh, nkv, maxlen, pos, variant, B=17), "ll_decode_attn_rope_bf16 grouped")


@pytest.mark.parametrize("maxlen,pos", R.GROUPED_POSITIONS)
@pytest.mark.parametrize("D", [64, 128])
def test_decode_attn_rope_17_sequences_group_of_three(lib, D, maxlen, pos):
    """no grouped instance for a group of three: seventeen sequences on the per-head kernel"""
    for variant in R.decode_variants(maxlen, pos):
        check_decode(lib, R.decode_case(D, 6, 2, maxlen, pos, variant, B=17), "ll_decode_attn_rope_bf16 per-head")


@pytest.mark.parametrize("variant", ["plain", "dom_pos"])
@pytest.mark.parametrize("maxlen", R.LDS_SWITCH)
def test_decode_attn_rope_grouped_lds_switch(lib, maxlen, variant):
    """G = 7, D = 128, 17 sequences: 33 280 + 28 maxlen bytes of LDS for the group -- 4312 keys run grouped, 4320 pass 150 KB and run per head"""
    entry = "ll_decode_attn_rope_bf16 " + ("grouped" if maxlen == R.LDS_SWITCH[0] else "per-head")
    check_decode(lib, R.decode_case(128, 7, 1, maxlen, maxlen - 1, variant, B=17), entry)


# ------------------------------------------------------------------------------------------------------------------ ll_decode_attn_bf16
def run_attn(lib, c, Kc, Vc):
    """one ll_decode_attn_bf16 call on the case's inputs (q a strided view, padded mask rows); returns out [B, S, nh, D]"""
    B, S, nh, D, L = c.B, c.S, c.nh, c.D, c.maxlen
    store = torch.full((B, S, nh + 1, D), R.NAN, dtype=R.BF)     # q as a strided [B,nh,S,D] view of [B,S,nh+1,D]
    store[:, :, :nh] = c.q.transpose(1, 2)
    q = store.cuda()[:, :, :nh].transpose(1, 2)
    ms = L + 5
    mask = torch.ones(B, 1, S, ms, dtype=torch.bool)
    mask[:, 0, :, :L] = c.visible
    mask = mask.cuda()
    out = _nan(B, S, nh, D)
    _check(lib.ll_decode_attn_bf16(q.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), mask.data_ptr(), out.data_ptr(), B, nh, c.nkv, S, L, D, c.scale,
                                   I3(q.stride(0), q.stride(1), q.stride(2)), I2(mask.stride(0), mask.stride(2)), _stream()), "ll_decode_attn_bf16")
    torch.cuda.synchronize()
    return out


def check_attn(lib, c):
    entry = "ll_decode_attn_bf16"
    Kp, Vp = R.poison(c, c.K0, c.V0, c.visible.any(1))
    Kc, Vc = Kp.cuda(), Vp.cuda()
    out = run_attn(lib, c, Kc, Vc)
    ref, absref = R.reference(c)
    _same_bits(entry, c, Kc, Kp, "key cache")
    _same_bits(entry, c, Vc, Vp, "value cache")
    _within(entry, c, out.cpu().transpose(1, 2), ref, absref)


@pytest.mark.parametrize("D,nh,nkv,S,maxlen,p0", R.ATTN_CASES)
def test_decode_attn(lib, D, nh, nkv, S, maxlen, p0):
    """S query rows with a causal mask each, the second sequence left-padded, q a strided view, padded mask rows"""
    for variant in R.ATTN_VARIANTS:
        check_attn(lib, R.attn_case(D, nh, nkv, S, maxlen, p0, variant))


# ------------------------------------------------------------------------------------------------------------------ ll_suffix_attn_rope_bf16
def run_prologue(lib, c):
    """ll_suffix_prologue on the case's position ids and 2-D mask; returns cos, sin [B*S, D] and mask [B*S, maxlen] on the device"""
    B, S, D, L, rows = c.B, c.S, c.D, c.maxlen, c.B * c.S
    posid, freq, mask2d = c.position_ids.cuda(), c.inv_freq.cuda(), c.mask2d.cuda()
    pos = torch.tensor([c.pos], dtype=torch.long, device="cuda")
    cos, sin = _nan(rows, D), _nan(rows, D)
    mask = torch.ones(rows, L, dtype=torch.bool, device="cuda")
    _check(lib.ll_suffix_prologue(posid.data_ptr(), freq.data_ptr(), 1.0, mask2d.data_ptr(), c.mask2d_stride, pos.data_ptr(), cos.data_ptr(),
                                  sin.data_ptr(), mask.data_ptr(), B, S, D, L, _stream()), "ll_suffix_prologue")
    torch.cuda.synchronize()
    return cos, sin, mask


def run_suffix(lib, c, Kc, Vc, cos, sin, mask):
    """one ll_suffix_attn_rope_bf16 call behind run_prologue; returns out [B*S, nh*D]"""
    qkv = c.qkv.cuda()
    pos = torch.tensor([c.pos], dtype=torch.long, device="cuda")
    out = _nan(c.B * c.S, c.nh * c.D)
    _check(lib.ll_suffix_attn_rope_bf16(qkv.data_ptr(), c.ld_qkv, cos.data_ptr(), sin.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), pos.data_ptr(),
                                        mask.data_ptr(), out.data_ptr(), c.B, c.S, c.nh, c.nkv, c.maxlen, c.D, c.scale, _stream()),
           "ll_suffix_attn_rope_bf16")
    torch.cuda.synchronize()
    return out


def check_suffix(lib, c):
    entry = "ll_suffix_attn_rope_bf16"
    B, S, nh, D, L = c.B, c.S, c.nh, c.D, c.maxlen
    Kp, Vp = R.poison(c, c.K0, c.V0, c.old)
    Kc, Vc = Kp.cuda(), Vp.cuda()
    posid, freq = c.position_ids.cuda(), c.inv_freq.cuda()
    cos, sin, mask = run_prologue(lib, c)
    out = run_suffix(lib, c, Kc, Vc, cos, sin, mask)
    # the reference from mask2d, *pos and position_ids alone: cos / sin with torch (the rotary module's own arithmetic on this device)
    cos_t, sin_t = R.rope_tables(freq, posid)
    inputs, written = R.suffix_expected(c, cos_t.cpu(), sin_t.cpu())
    assert torch.equal(cos.cpu().view(B, S, D), cos_t.cpu()) and torch.equal(sin.cpu().view(B, S, D), sin_t.cpu())
    assert torch.equal(mask.cpu().view(B, S, L), inputs[3])
    ref, absref = R.reference(c, inputs)
    Kp[:, :, written], Vp[:, :, written] = inputs[1][:, :, written], inputs[2][:, :, written]
    _same_bits(entry, c, Kc, Kp, "key cache")
    _same_bits(entry, c, Vc, Vp, "value cache")
    _within(entry, c, out.cpu().view(B, S, nh, D).transpose(1, 2), ref, absref)


@pytest.mark.parametrize("D,nh,nkv,B,S,maxlen,pos", R.SUFFIX_CASES)
def test_suffix_attn_rope(lib, D, nh, nkv, B, S, maxlen, pos):
    """S new rows per sequence behind ll_suffix_prologue: one chain from position ids and the 2-D mask to the attention output"""
    for variant in R.SUFFIX_VARIANTS:
        check_suffix(lib, R.suffix_case(D, nh, nkv, B, S, maxlen, pos, variant))


# ------------------------------------------------------------------------------------------------------------------ ll_kv_append_bf16
@pytest.mark.parametrize("S,pos,maxlen", [(1, 0, 40), (1, 39, 40), (5, 10, 40), (5, 37, 40), (1, 40, 40), (5, 40, 40), (5, 255, 300)])
@pytest.mark.parametrize("D", [64, 128])
def test_kv_append_strided_rows_and_the_end_of_the_cache(lib, D, S, pos, maxlen):
    """k_new / v_new as [B,nkv,S,D] views of q|k|v rows; rows past the last slot are dropped, nothing else is written"""
    B, nkv = 2, 3
    g = torch.Generator().manual_seed(D + S + pos)
    ld = 3 * nkv * D + 8
    rows = torch.randn(B * S, ld, generator=g).to(R.BF).cuda()
    k = rows[:, nkv * D:2 * nkv * D].view(B, S, nkv, D).transpose(1, 2)
    v = rows[:, 2 * nkv * D:3 * nkv * D].view(B, S, nkv, D).transpose(1, 2)
    K0, V0 = torch.randn(B, nkv, maxlen, D, generator=g).to(R.BF), torch.randn(B, nkv, maxlen, D, generator=g).to(R.BF)
    K0[:, :, ::3], V0[:, :, 1::3] = R.NAN, R.NAN
    Kc, Vc = K0.cuda(), V0.cuda()
    p = torch.tensor([pos], dtype=torch.long, device="cuda")
    _check(lib.ll_kv_append_bf16(Kc.data_ptr(), Vc.data_ptr(), k.data_ptr(), v.data_ptr(), p.data_ptr(), B, nkv, S, maxlen, D,
                                 I3(k.stride(0), k.stride(1), k.stride(2)), I3(v.stride(0), v.stride(1), v.stride(2)), _stream()), "ll_kv_append_bf16")
    torch.cuda.synchronize()
    n = max(0, min(S, maxlen - pos))
    K0[:, :, pos:pos + n], V0[:, :, pos:pos + n] = k.cpu()[:, :, :n], v.cpu()[:, :, :n]
    assert torch.equal(_bits(Kc), _bits(K0)) and torch.equal(_bits(Vc), _bits(V0))


# ------------------------------------------------------------------------------------------------------------------ long contexts
@pytest.mark.parametrize("D,maxlen,variants", R.LONG_CASES)
@pytest.mark.parametrize("entry", ["decode", "suffix", "attn"])
def test_long_context(lib, entry, D, maxlen, variants):
    """one sequence, two query heads on one KV head, the new position in the last slot: 12032 keys are the last that fit 64 KB of LDS at
    D = 128, 16384 the most the entry points accept"""
    for variant in variants:
        c = R.long_case(entry, D, maxlen, variant)
        if entry == "decode":
            check_decode(lib, c, "ll_decode_attn_rope_bf16 per-head")
        elif entry == "attn":
            check_attn(lib, c)
        else:
            check_suffix(lib, c)


def test_more_keys_than_the_limit_are_refused(lib):
    """maxlen = 16385: LL_EINVAL from all three entry points, nothing launched (the buffers are a few bytes)"""
    L, D = R.MAXLEN_LIMIT + 1, 128
    t = torch.zeros(4096, dtype=R.BF, device="cuda")
    pos = torch.zeros(1, dtype=torch.long, device="cuda")
    p, st = t.data_ptr(), _stream()
    rc = [lib.ll_decode_attn_bf16(p, p, p, p, p, 1, 2, 1, 1, L, D, D ** -0.5, I3(2 * D, D, D), I2(L, L), st),
          lib.ll_decode_attn_rope_bf16(p, 4 * D, p, p, 0, p, p, pos.data_ptr(), p, L, p, 1, 2, 1, L, D, D ** -0.5, st),
          lib.ll_suffix_attn_rope_bf16(p, 4 * D, p, p, p, p, pos.data_ptr(), p, p, 1, 1, 2, 1, L, D, D ** -0.5, st)]
    torch.cuda.synchronize()
    assert rc == [-1, -1, -1]
    assert float(t.float().abs().max()) == 0.0
