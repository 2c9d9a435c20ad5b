"""The MX8 KV-cache entry points through the C ABI: ll_kv8_store_bf16 and the rows the attention entries store are bit-equal to
llm_quant.mx_round (codes and scale bytes); ll_kv8_load_bf16 is bit-equal to decode_codes x 2^e; ll_decode_attn_rope_kv8 and
ll_suffix_attn_rope_kv8 stay within attn_reference's bound 2^-8 |ref| + 2^-11 sum_j p_j |v_j| of the float64 reference evaluated on the
DEQUANTISED cache with the new rows quantised (dequantisation is exact and the summation structure is the key-split kernel's: at most 96 f32
terms per lane, tests/test_attn_split_reference_cpu.py, so the bound carries over unchanged); a row without a visible key is exactly zero;
masked slots hold NaN codes (0x7f) and the scale byte 0xff; the documented refusals return an error and write nothing.

Largest err / bound measured on an MI355X (-s prints them): ll_decode_attn_rope_kv8 0.867, with norm weights 0.682, ll_suffix_attn_rope_kv8 0.877,
with norm weights 0.678."""
import gc

import pytest
import torch

from llamole_amd.kv_cache import mx8_dequantize, mx8_quantize_rows
from tests import attn_reference as R
from tests import kv8_cases as KC
from tests import qknorm_reference as Q

pytestmark = pytest.mark.gpu

WORST = {}
NAN_CODE, NAN_SCALE = 0x7f, 0xff


@pytest.fixture(autouse=True)
def _release_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


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


def _i64x3(t):
    import ctypes as C
    return (C.c_int64 * 3)(t.stride(0), t.stride(1), t.stride(2))


def _nan(*shape):
    return torch.full(shape, R.NAN, dtype=R.BF, device="cuda")


def _within(entry, c, out, ref, absref):
    assert torch.isfinite(out.float()).all(), (entry, c.variant, "the output holds NaN / inf")
    r = R.err_over_bound(out, ref, absref)
    WORST[entry] = max(WORST.get(entry, 0.0), r)
    assert r <= 1.0, (entry, c.variant, r)


# ------------------------------------------------------------------------------------------------------------------ store / load
def _bf16_bits(bits):
    return torch.tensor(bits, dtype=torch.int16).view(torch.bfloat16)


def _store_rows(B, nkv, S, D, seed):
    """k / v [B, nkv, S, D] as strided views of q|k|v-like rows (row pitch (2 nkv D + 24), last dimension contiguous), with the blocks that
    decide a quantiser: all zero, a maximum exactly at the `thr` mantissa (1.75 x 2^x: the largest amax that keeps the smaller exponent) and one
    ulp either side of it, magnitudes of 300-500 (Qwen2's K range), 1e-30, a negative zero."""
    g = torch.Generator().manual_seed(seed)
    ld = 2 * nkv * D + 24
    buf = torch.randn(B, S, ld, generator=g).to(R.BF)
    k = buf[..., 8:8 + nkv * D].view(B, S, nkv, D).transpose(1, 2)
    v = buf[..., 16 + nkv * D:16 + 2 * nkv * D].view(B, S, nkv, D).transpose(1, 2)
    small = (torch.rand(32, generator=g) * 0.9).to(R.BF)
    for t, x in enumerate((k, v)):
        x[0, 0, 0, :32] = 0                                                      # an all-zero block
        for i, top in enumerate((0x3fe0, 0x3fdf, 0x3fe1, 0x43e0, 0x43df, 0x43e1)):   # 1.75, its neighbours; 448 = 1.75 x 2^8, its neighbours
            s, blk = (i + t) % S, (i % (D // 32)) * 32
            x[0, nkv - 1, s, blk:blk + 32] = small * (1.0 if top < 0x4000 else 200.0)
            x[0, nkv - 1, s, blk + 7] = _bf16_bits([top])[0] * (-1 if i % 2 else 1)
        x[B - 1, 0, S - 1] = (300 + 200 * torch.rand(D, generator=g)).to(R.BF) * torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0).to(R.BF)
        x[B - 1, 0, 0, 32:64] = (torch.randn(32, generator=g) * 1e-30).to(R.BF)
        x[B - 1, nkv - 1, 0, 3] = -0.0
    return buf, k, v


@pytest.mark.parametrize("S,maxlen,pos", [(1, 64, 63), (9, 576, 508), (40, 576, 490), (9, 64, 60)])
@pytest.mark.parametrize("D", [64, 128])
def test_store_is_bit_equal_to_mx_round_and_load_to_decode_codes(lib, D, S, maxlen, pos):
    """S = 9 at 508 and S = 40 at 490 put rows on both sides of slot 512; S = 9 at 60 of 64 drops the five rows past the end"""
    B, nkv = 2, 3
    buf, k, v = _store_rows(B, nkv, S, D, seed=S + D)
    dbuf = buf.cuda()
    kd = dbuf[..., 8:8 + nkv * D].view(B, S, nkv, D).transpose(1, 2)
    vd = dbuf[..., 16 + nkv * D:16 + 2 * nkv * D].view(B, S, nkv, D).transpose(1, 2)
    assert not kd.is_contiguous() and kd.stride(3) == 1
    g = torch.Generator().manual_seed(5)
    codes0 = torch.randint(0, 256, (4, B, nkv, maxlen, D), generator=g, dtype=torch.int32).to(torch.uint8)
    codes0[(codes0 & 0x7f) == 0x7f] = 0x3c                                       # no NaN codes among what the load test reads
    scales0 = torch.randint(10, 247, (4, B, nkv, maxlen, D // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    Kq, Vq, Ks, Vs = codes0[0].cuda(), codes0[1].cuda(), scales0[0].cuda(), scales0[1].cuda()
    posd = torch.tensor([pos], dtype=torch.long, device="cuda")
    _check(lib.ll_kv8_store_bf16(Kq.data_ptr(), Ks.data_ptr(), Vq.data_ptr(), Vs.data_ptr(), kd.data_ptr(), vd.data_ptr(), posd.data_ptr(), B, nkv,
                                 S, maxlen, D, _i64x3(kd), _i64x3(vd), _stream()), "ll_kv8_store_bf16")
    torch.cuda.synchronize()
    n = min(S, maxlen - pos)
    for name, got_c, got_s, new, c0, s0 in (("K", Kq, Ks, k, codes0[0], scales0[0]), ("V", Vq, Vs, v, codes0[1], scales0[1])):
        want_c, want_s = c0.clone(), s0.clone()
        want_c[:, :, pos:pos + n], want_s[:, :, pos:pos + n] = mx8_quantize_rows(new[:, :, :n].contiguous())
        assert torch.equal(got_s.cpu(), want_s), (name, "scale bytes")
        assert torch.equal(got_c.cpu(), want_c), (name, "codes")
    # ---- load: slots [0, *pos + extra) of both tensors, everything behind left as it was
    Kst, Vst = _nan(B, nkv, maxlen, D), _nan(B, nkv, maxlen, D)
    for extra in (0, S):
        _check(lib.ll_kv8_load_bf16(Kq.data_ptr(), Ks.data_ptr(), Vq.data_ptr(), Vs.data_ptr(), Kst.data_ptr(), Vst.data_ptr(), posd.data_ptr(),
                                    extra, B, nkv, maxlen, D, _stream()), "ll_kv8_load_bf16")
        torch.cuda.synchronize()
        m = min(maxlen, pos + extra)
        for got, c, s in ((Kst, Kq, Ks), (Vst, Vq, Vs)):
            want = mx8_dequantize(c.cpu()[:, :, :m], s.cpu()[:, :, :m])
            assert torch.equal(want.to(R.BF).float(), want)                      # exactly bf16
            assert torch.equal(got.cpu()[:, :, :m].view(torch.int16), want.to(R.BF).view(torch.int16))
            assert torch.isnan(got.cpu()[:, :, m:].float()).all()


# ------------------------------------------------------------------------------------------------------------------ attention
def _quantise_cache(c):
    """the case's cache as an MX8 cache: c.K0 / c.V0 become the dequantised values (what the reference attends to); returns the four tensors"""
    Kc, Ksc = mx8_quantize_rows(c.K0)
    Vc, Vsc = mx8_quantize_rows(c.V0)
    c.K0, c.V0 = mx8_dequantize(Kc, Ksc).to(R.BF), mx8_dequantize(Vc, Vsc).to(R.BF)
    return Kc, Ksc, Vc, Vsc


def _poison(t, keep, byte):
    """NaN codes / the scale byte 0xff in every slot outside `keep` (bool [B, L])"""
    return torch.where(keep[:, None, :, None], t, torch.full_like(t, byte))


def _mxdq(x):
    """mx_round of bf16 rows [..., D], as bf16"""
    return mx8_dequantize(*mx8_quantize_rows(x)).to(R.BF)


def _workspace(lib, B, S, c):
    n = int(lib.ll_attn_split_workspace_bytes(B, S, c.nh, c.nkv, c.maxlen, c.D))
    assert n == B * S * c.nh * -(-c.maxlen // KC.RANGE) * (c.D + 2) * 4
    return torch.full((n // 2,), R.NAN, dtype=R.BF, device="cuda"), n      # NaN: nothing may be read that was not written


def _norm_args(c):
    if hasattr(c, "qw"):
        c._qw, c._kw = c.qw.cuda(), c.kw.cuda()
        return c._qw.data_ptr(), c._kw.data_ptr(), c.eps
    return None, None, 0.0


def check_decode(lib, c, entry="ll_decode_attn_rope_kv8", expected=R.decode_expected):
    Kc, Ksc, Vc, Vsc = _quantise_cache(c)
    keep = c.visible.clone()
    keep[:, c.pos] = False                                       # the stale row at *pos
    host = [_poison(Kc, keep, NAN_CODE), _poison(Ksc, keep, NAN_SCALE), _poison(Vc, keep, NAN_CODE), _poison(Vsc, keep, NAN_SCALE)]
    dev = [t.cuda() for t in host]
    qkv, cos, sin, mask = c.qkv.cuda(), c.cos.cuda(), c.sin.cuda(), c.mask.cuda()
    pos = torch.tensor([c.pos], dtype=torch.long, device="cuda")
    ws, n = _workspace(lib, c.B, 1, c)
    out = _nan(c.B, c.nh * c.D)
    _check(lib.ll_decode_attn_rope_kv8(qkv.data_ptr(), c.ld_qkv, cos.data_ptr(), sin.data_ptr(), c.cs_stride, *(t.data_ptr() for t in dev),
                                       pos.data_ptr(), mask.data_ptr(), c.mask_stride, out.data_ptr(), c.B, c.nh, c.nkv, c.maxlen, c.D, c.scale,
                                       *_norm_args(c), ws.data_ptr(), n, _stream()), entry)
    # the rows ll_decode_attn_rope_split_bf16 stores from the same inputs
    Kb, Vb = _nan(c.B, c.nkv, c.maxlen, c.D), _nan(c.B, c.nkv, c.maxlen, c.D)
    ref_out = _nan(c.B, c.nh * c.D)
    _check(lib.ll_decode_attn_rope_split_bf16(qkv.data_ptr(), c.ld_qkv, cos.data_ptr(), sin.data_ptr(), c.cs_stride, Kb.data_ptr(), Vb.data_ptr(),
                                              pos.data_ptr(), mask.data_ptr(), c.mask_stride, ref_out.data_ptr(), c.B, c.nh, c.nkv, c.maxlen, c.D,
                                              c.scale, *_norm_args(c), ws.data_ptr(), n, _stream()), "ll_decode_attn_rope_split_bf16")
    torch.cuda.synchronize()
    out = out.cpu().view(c.B, c.nh, 1, c.D)
    inputs, (k_rot, v_new) = expected(c)
    q_rot, K, V, vis = inputs
    K[:, :, c.pos], V[:, :, c.pos] = _mxdq(k_rot), _mxdq(v_new)          # the new rows are attended to as the cache holds them
    ref, absref = R.reference(c, (q_rot, K, V, vis))
    kc, ks = mx8_quantize_rows(Kb[:, :, c.pos].cpu())
    vc, vs = mx8_quantize_rows(Vb[:, :, c.pos].cpu())
    assert torch.equal(kc, mx8_quantize_rows(k_rot)[0]) and torch.equal(vc, mx8_quantize_rows(v_new)[0])
    for t, new in zip(host, (kc, ks, vc, vs)):
        t[:, :, c.pos] = new                                             # the appended row, every other slot as it was
    for name, t, d in zip(("key codes", "key scales", "value codes", "value scales"), host, dev):
        assert torch.equal(d.cpu(), t), (entry, c.variant, name)
    _within(entry, c, out, ref, absref)
    for b in range(c.B):
        if not c.visible[b].any():
            assert float(out[b].float().abs().max()) == 0.0, (entry, c.variant, "a fully masked row is not zero")


@pytest.mark.parametrize("D,nh,nkv", KC.GEOMETRIES)
def test_kv8_decode_range_edges(lib, D, nh, nkv):
    """64, 576 and 1088 slots: *pos on either side of the edge 511 | 512, in the last slot, and at 40 of 1088 (two ranges fully masked); one
    dominant key on either side of both edges; left padding longer than a range; NaN codes in every slot the call may not read"""
    for case in KC.DECODE_CASES:
        if case[:3] == (D, nh, nkv):
            check_decode(lib, KC.decode_case(*case))


def test_kv8_decode_16448_slots(lib):
    check_decode(lib, KC.decode_case(*KC.LONG_CASE))


@pytest.mark.parametrize("D,nh,nkv", KC.NORM_GEOMETRIES)
def test_kv8_decode_with_head_norms(lib, D, nh, nkv):
    for maxlen, pos in KC.NORM_SHAPES:
        for v in KC.NORM_VARIANTS:
            check_decode(lib, Q.decode_case(D, nh, nkv, maxlen, pos, v), "ll_decode_attn_rope_kv8 norms", Q.decode_expected)


def check_suffix(lib, c, entry="ll_suffix_attn_rope_kv8", expected=R.suffix_expected):
    B, S, nh, D, L, rows = c.B, c.S, c.nh, c.D, c.maxlen, c.B * c.S
    Kc, Ksc, Vc, Vsc = _quantise_cache(c)
    host = [_poison(Kc, c.old, NAN_CODE), _poison(Ksc, c.old, NAN_SCALE), _poison(Vc, c.old, NAN_CODE), _poison(Vsc, c.old, NAN_SCALE)]
    dev = [t.cuda() for t in host]
    posid, freq, mask2d, qkv = c.position_ids.cuda(), c.inv_freq.cuda(), c.mask2d.cuda(), c.qkv.cuda()
    pos = torch.tensor([c.pos], dtype=torch.long, device="cuda")
    cos, sin = _nan(rows, D), _nan(rows, D)
    mask = torch.ones(rows, L, dtype=torch.bool, device="cuda")
    _check(lib.ll_suffix_prologue(posid.data_ptr(), freq.data_ptr(), 1.0, mask2d.data_ptr(), c.mask2d_stride, pos.data_ptr(), cos.data_ptr(),
                                  sin.data_ptr(), mask.data_ptr(), B, S, D, L, _stream()), "ll_suffix_prologue")
    ws, n = _workspace(lib, B, S, c)
    out = _nan(rows, nh * D)
    _check(lib.ll_suffix_attn_rope_kv8(qkv.data_ptr(), c.ld_qkv, cos.data_ptr(), sin.data_ptr(), *(t.data_ptr() for t in dev), pos.data_ptr(),
                                       mask.data_ptr(), out.data_ptr(), B, S, nh, c.nkv, L, D, c.scale, *_norm_args(c), ws.data_ptr(), n,
                                       _stream()), entry)
    Kb, Vb = _nan(B, c.nkv, L, D), _nan(B, c.nkv, L, D)
    ref_out = _nan(rows, nh * D)
    _check(lib.ll_suffix_attn_rope_split_bf16(qkv.data_ptr(), c.ld_qkv, cos.data_ptr(), sin.data_ptr(), Kb.data_ptr(), Vb.data_ptr(), pos.data_ptr(),
                                              mask.data_ptr(), ref_out.data_ptr(), B, S, nh, c.nkv, L, D, c.scale, *_norm_args(c), ws.data_ptr(), n,
                                              _stream()), "ll_suffix_attn_rope_split_bf16")
    torch.cuda.synchronize()
    (q_rot, K, V, vis), written = expected(c, cos.cpu().view(B, S, D), sin.cpu().view(B, S, D))
    assert torch.equal(Kb.cpu()[:, :, written].view(torch.int16), K[:, :, written].view(torch.int16))      # the bf16 entry stores the reference's rows
    new = [*mx8_quantize_rows(Kb.cpu()[:, :, written]), *mx8_quantize_rows(Vb.cpu()[:, :, written])]
    K[:, :, written], V[:, :, written] = _mxdq(K[:, :, written]), _mxdq(V[:, :, written])
    ref, absref = R.reference(c, (q_rot, K, V, vis))
    for t, x in zip(host, new):
        t[:, :, written] = x
    for name, t, d in zip(("key codes", "key scales", "value codes", "value scales"), host, dev):
        assert torch.equal(d.cpu(), t), (entry, c.variant, name)
    _within(entry, c, out.cpu().view(B, S, nh, D).transpose(1, 2), ref, absref)


@pytest.mark.parametrize("S,pos", KC.SUFFIX_SHAPES)
@pytest.mark.parametrize("D,nh,nkv", KC.SUFFIX_GEOMETRIES)
def test_kv8_suffix_across_a_range_edge(lib, D, nh, nkv, S, pos):
    for B in KC.SUFFIX_BATCHES:
        for v in R.SUFFIX_VARIANTS:
            check_suffix(lib, R.suffix_case(D, nh, nkv, B, S, KC.SUFFIX_MAXLEN, pos, v))


@pytest.mark.parametrize("D,nh,nkv", KC.SUFFIX_NORM_GEOMETRIES)
def test_kv8_suffix_with_head_norms(lib, D, nh, nkv):
    for S, B in ((9, 1), (3, 5)):
        for v in ("plain", "dom_own"):
            check_suffix(lib, Q.suffix_case(D, nh, nkv, B, S, KC.SUFFIX_MAXLEN, 512 - 1 - S // 2, v), "ll_suffix_attn_rope_kv8 norms",
                         Q.suffix_expected)


# ------------------------------------------------------------------------------------------------------------------ bounds
def test_documented_refusals_return_an_error_and_write_nothing(lib):
    """65 sequences, 17 new rows, a head size without an instance, a small workspace, 131073 slots, one norm weight only: LL_EINVAL from the
    attention entries (the buffers are a few bytes: nothing may be launched); D = 96 from store and load as well"""
    import ctypes as C
    L, D = 1024, 128
    t = torch.zeros(4096, dtype=R.BF, device="cuda")
    pos = torch.zeros(1, dtype=torch.long, device="cuda")
    p, st, pp = t.data_ptr(), _stream(), pos.data_ptr()
    dec = lambda B, L_, D_, qn, wsb: lib.ll_decode_attn_rope_kv8(p, 4 * D_, p, p, 0, p, p, p, p, pp, p, L_, p, B, 2, 1, L_, D_, D_ ** -0.5, qn, None,
                                                                 1e-6 if qn else 0.0, p, wsb, st)
    sfx = lambda S, D_: lib.ll_suffix_attn_rope_kv8(p, 4 * D_, p, p, p, p, p, p, pp, p, p, 1, S, 2, 1, L, D_, D_ ** -0.5, None, None, 0.0, p, 1 << 40, st)
    s3 = (C.c_int64 * 3)(D, D, D)
    rc = [dec(65, L, D, None, 1 << 40), sfx(17, D), dec(1, L, 96, None, 1 << 40), sfx(2, 96), dec(1, L, D, None, 64), dec(1, 131073, D, None, 1 << 40),
          dec(1, L, D, p, 1 << 40),
          lib.ll_kv8_store_bf16(p, p, p, p, p, p, pp, 1, 1, 1, L, 96, s3, s3, st),
          lib.ll_kv8_load_bf16(p, p, p, p, p, p, pp, 1, 1, 1, L, 96, st)]
    torch.cuda.synchronize()
    assert rc == [-1] * 9
    assert float(t.float().abs().max()) == 0.0 and int(pos) == 0
