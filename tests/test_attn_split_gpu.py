"""The key-split decode attention (ll_decode_attn_rope_split_bf16, ll_suffix_attn_rope_split_bf16, ll_attn_split_workspace_bytes) through the
C ABI against the float64 reference of tests/attn_reference.py: at the edges of the 512-key ranges (keys 511 | 512 | 1023, *pos on either side
of an edge, suffix rows across one), with fully masked ranges, left padding longer than a range, fully masked rows, NaN in every cache slot the
call may not read, groups of 1 / 2 / 4 / 7 query heads, 3 and 20 sequences, at 16385, 16904 and 131072 slots.  Every output element within
2^-8 |ref| + 2^-11 sum_j p_j |v_j| (attn_reference's bound, unchanged; tests/test_attn_split_reference_cpu.py derives the number of f32 terms
a lane sums -- at most 96 -- and shows what the bound lets through and what not); fully masked rows exactly zero; the cache compared bit for bit.

Largest err / bound measured on an MI355X (-s prints them): ll_decode_attn_rope_split_bf16 0.884, with norm weights 0.682,
ll_suffix_attn_rope_split_bf16 0.868, with norm weights 0.694; ll_decode_attn_rope_bf16 on the shared 300- / 16384-slot inputs 0.686."""
import gc

import pytest
import torch

from tests import attn_reference as R
from tests import attn_split_cases as SC
from tests import qknorm_reference as Q

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(autouse=True)
def _release_device_memory():
    """these tests hold caches of up to 131072 slots in torch's allocator, which keeps freed blocks: hand them back after every test, so that the
    engines of later tests, which allocate from the device directly, find the memory"""
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


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _nan(*shape):
    return torch.full(shape, R.NAN, dtype=R.BF, device="cuda")


def _within(entry, c, out, ref, absref):
    assert torch.isfinite(out.float()).all(), (entry, c.variant, "the output holds NaN / inf")
    r = R.err_over_bound(out, ref, absref)
    WORST[entry] = max(WORST.get(entry, 0.0), r)
    assert r <= 1.0, (entry, c.variant, r)


def _workspace(lib, B, S, c):
    n = int(lib.ll_attn_split_workspace_bytes(B, S, c.nh, c.nkv, c.maxlen, c.D))
    assert n == B * S * c.nh * -(-c.maxlen // SC.RANGE) * (c.D + 2) * 4
    return torch.full((n // 2,), R.NAN, dtype=R.BF, device="cuda"), n      # NaN: nothing may be read that was not written


def _norm_args(c):
    if hasattr(c, "qw"):
        c._qw, c._kw = c.qw.cuda(), c.kw.cuda()
        return c._qw.data_ptr(), c._kw.data_ptr(), c.eps
    return None, None, 0.0


def run_decode(lib, c, Kc, Vc):
    c._dev = [c.qkv.cuda(), c.cos.cuda(), c.sin.cuda(), c.mask.cuda(), torch.tensor([c.pos], dtype=torch.long, device="cuda")]
    qkv, cos, sin, mask, pos = c._dev
    ws, n = _workspace(lib, c.B, 1, c)
    out = _nan(c.B, c.nh * c.D)
    _check(lib.ll_decode_attn_rope_split_bf16(qkv.data_ptr(), c.ld_qkv, cos.data_ptr(), sin.data_ptr(), c.cs_stride, Kc.data_ptr(), Vc.data_ptr(),
                                              pos.data_ptr(), mask.data_ptr(), c.mask_stride, out.data_ptr(), c.B, c.nh, c.nkv, c.maxlen, c.D,
                                              c.scale, *_norm_args(c), ws.data_ptr(), n, _stream()), "ll_decode_attn_rope_split_bf16")
    torch.cuda.synchronize()
    return out.cpu().view(c.B, c.nh, 1, c.D)


def check_decode(lib, c, entry="ll_decode_attn_rope_split_bf16", expected=R.decode_expected):
    keep = c.visible.clone()
    keep[:, c.pos] = False                                       # the stale row at *pos
    Kp, Vp = R.poison(c, c.K0, c.V0, keep)
    Kc, Vc = Kp.cuda(), Vp.cuda()
    out = run_decode(lib, c, Kc, Vc)
    inputs, (k_rot, v_new) = expected(c)
    ref, absref = R.reference(c, inputs)
    Kp[:, :, c.pos], Vp[:, :, c.pos] = k_rot, v_new              # the appended row, every other slot as it was
    assert torch.equal(_bits(Kc), _bits(Kp)), (entry, c.variant, "key cache")
    assert torch.equal(_bits(Vc), _bits(Vp)), (entry, c.variant, "value cache")
    _within(entry, c, out, ref, absref)
    for b in range(c.B):
        if not c.visible[b].any():
            assert float(out[b].float().abs().max()) == 0.0, (entry, c.variant, "a fully masked row is not zero")
    return out, Kc, Vc, (ref, absref)


# ------------------------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("pos", SC.SMALL_POSITIONS)
@pytest.mark.parametrize("D,nh,nkv", SC.GEOMETRIES)
def test_split_decode_range_edges(lib, D, nh, nkv, pos):
    """four ranges (the last of eight keys), *pos in the last slot, on either side of the edge 511 | 512 and at 40 (three ranges fully masked)"""
    for v in SC.VARIANTS:
        if SC.fits(v, pos):
            for bcast in ((True, False) if v == "plain" else (False,)):
                check_decode(lib, SC.decode_case(D, nh, nkv, SC.SMALL, pos, v, bcast=bcast))


@pytest.mark.parametrize("maxlen", [R.MAXLEN_LIMIT + 1, SC.LONG])
@pytest.mark.parametrize("D,nh,nkv", SC.GEOMETRIES)
def test_split_decode_beyond_16384_slots(lib, D, nh, nkv, maxlen):
    for v in SC.LONG_VARIANTS:
        check_decode(lib, SC.decode_case(D, nh, nkv, maxlen, maxlen - 1, v))


@pytest.mark.parametrize("D,nh,nkv,pos,variant", SC.HUGE_CASES)
def test_split_decode_131072_slots(lib, D, nh, nkv, pos, variant):
    check_decode(lib, SC.decode_case(D, nh, nkv, SC.SPLIT_LIMIT, pos, variant))


def test_split_decode_20_sequences(lib):
    """many sequences run the same kernel shape: a K / V row is fetched once per KV group for every B"""
    for v in ("plain", "dom_pos"):
        check_decode(lib, SC.decode_case(64, 4, 2, SC.LONG, SC.LONG - 1, v, B=20))


@pytest.mark.parametrize("D,nh,nkv", [(128, 8, 2), (64, 7, 1), (64, 4, 2)])
def test_split_decode_with_head_norms(lib, D, nh, nkv):
    """q_norm_w / k_norm_w given: the Qwen3 layout against tests/qknorm_reference.py (tie-safe head vectors: the stored key bit for bit)"""
    for pos in (SC.RANGE - 1, SC.RANGE, SC.SMALL - 1):
        for v in ("plain", "dom_pos", "tiny"):
            check_decode(lib, Q.decode_case(D, nh, nkv, SC.SMALL, pos, v), "ll_decode_attn_rope_split_bf16 norms", Q.decode_expected)


@pytest.mark.parametrize("maxlen", [300, R.MAXLEN_LIMIT])
@pytest.mark.parametrize("D,nh,nkv", [(64, 4, 2), (128, 7, 1)])
def test_split_and_one_workgroup_entry_store_the_same_rows(lib, D, nh, nkv, maxlen):
    """where both entries apply: bit-equal caches afterwards, both outputs inside the bound of the same reference"""
    for v in ("plain", "dom_pos"):
        c = SC.decode_case(D, nh, nkv, maxlen, maxlen - 1, v)
        _, Kn, Vn, (ref, absref) = check_decode(lib, c)
        keep = c.visible.clone()
        keep[:, c.pos] = False
        Kp, Vp = R.poison(c, c.K0, c.V0, keep)
        Ko, Vo = Kp.cuda(), Vp.cuda()
        qkv, cos, sin, mask, pos = c._dev
        out = _nan(c.B, c.nh * c.D)
        _check(lib.ll_decode_attn_rope_bf16(qkv.data_ptr(), c.ld_qkv, cos.data_ptr(), sin.data_ptr(), c.cs_stride, Ko.data_ptr(), Vo.data_ptr(),
                                            pos.data_ptr(), mask.data_ptr(), c.mask_stride, out.data_ptr(), c.B, c.nh, c.nkv, c.maxlen, c.D,
                                            c.scale, _stream()), "ll_decode_attn_rope_bf16")
        torch.cuda.synchronize()
        assert torch.equal(_bits(Ko), _bits(Kn)) and torch.equal(_bits(Vo), _bits(Vn))
        _within("ll_decode_attn_rope_bf16 (same inputs)", c, out.cpu().view(c.B, c.nh, 1, c.D), ref, absref)


# ------------------------------------------------------------------------------------------------------------------ suffix
def run_suffix(lib, c, Kc, Vc, cos, sin, mask, entry="ll_suffix_attn_rope_split_bf16"):
    """one ll_suffix_attn_rope_split_bf16 call behind ll_suffix_prologue's cos / sin / mask; returns out [B*S, nh*D]"""
    qkv = c.qkv.cuda()
    pos = torch.tensor([c.pos], dtype=torch.long, device="cuda")
    ws, n = _workspace(lib, c.B, c.S, c)
    out = _nan(c.B * c.S, c.nh * c.D)
    _check(lib.ll_suffix_attn_rope_split_bf16(qkv.data_ptr(), c.ld_qkv, cos.data_ptr(), sin.data_ptr(), Kc.data_ptr(), Vc.data_ptr(),
                                              pos.data_ptr(), mask.data_ptr(), out.data_ptr(), c.B, c.S, c.nh, c.nkv, c.maxlen, c.D, c.scale,
                                              *_norm_args(c), ws.data_ptr(), n, _stream()), entry)
    torch.cuda.synchronize()
    return out


def check_suffix(lib, c, entry="ll_suffix_attn_rope_split_bf16", expected=R.suffix_expected):
    B, S, nh, D, L, rows = c.B, c.S, c.nh, c.D, c.maxlen, c.B * c.S
    Kp, Vp = R.poison(c, c.K0, c.V0, c.old)
    Kc, Vc = Kp.cuda(), Vp.cuda()
    posid, freq, mask2d = c.position_ids.cuda(), c.inv_freq.cuda(), c.mask2d.cuda()
    pos = torch.tensor([c.pos], dtype=torch.long, device="cuda")
    cos, sin = _nan(rows, D), _nan(rows, D)
    mask = torch.ones(rows, L, dtype=torch.bool, device="cuda")
    _check(lib.ll_suffix_prologue(posid.data_ptr(), freq.data_ptr(), 1.0, mask2d.data_ptr(), c.mask2d_stride, pos.data_ptr(), cos.data_ptr(),
                                  sin.data_ptr(), mask.data_ptr(), B, S, D, L, _stream()), "ll_suffix_prologue")
    out = run_suffix(lib, c, Kc, Vc, cos, sin, mask, entry)
    inputs, written = expected(c, cos.cpu().view(B, S, D), sin.cpu().view(B, S, D))
    ref, absref = R.reference(c, inputs)
    Kp[:, :, written], Vp[:, :, written] = inputs[1][:, :, written], inputs[2][:, :, written]
    assert torch.equal(_bits(Kc), _bits(Kp)), (entry, c.variant, "key cache")
    assert torch.equal(_bits(Vc), _bits(Vp)), (entry, c.variant, "value cache")
    _within(entry, c, out.cpu().view(B, S, nh, D).transpose(1, 2), ref, absref)


@pytest.mark.parametrize("S,B", SC.SUFFIX_ROWS)
@pytest.mark.parametrize("D,nh,nkv", SC.SUFFIX_GEOMETRIES)
def test_split_suffix_across_a_range_edge(lib, D, nh, nkv, S, B):
    """S new rows per sequence whose slots cross the edge 511 | 512, start on it, or end in the last slot of the cache"""
    for pos in SC.suffix_positions(S):
        for v in R.SUFFIX_VARIANTS:
            check_suffix(lib, R.suffix_case(D, nh, nkv, B, S, SC.SMALL, pos, v))


def test_split_suffix_beyond_16384_slots_and_past_the_end(lib):
    for S, pos in ((9, SC.LONG - 9), (16, SC.LONG - 5)):            # the second: eleven rows past the last slot are not stored
        for v in R.SUFFIX_VARIANTS:
            check_suffix(lib, R.suffix_case(128, 8, 2, 2, S, SC.LONG, pos, v))


@pytest.mark.parametrize("D,nh,nkv", [(128, 8, 2), (64, 7, 1)])
def test_split_suffix_with_head_norms(lib, D, nh, nkv):
    for S, B in ((9, 1), (3, 5)):
        for pos in (SC.RANGE - 1 - S // 2, SC.SMALL - S):
            for v in ("plain", "dom_own"):
                check_suffix(lib, Q.suffix_case(D, nh, nkv, B, S, SC.SMALL, pos, v), "ll_suffix_attn_rope_split_bf16 norms", Q.suffix_expected)


# ------------------------------------------------------------------------------------------------------------------ bounds
def test_more_slots_than_the_limit_are_refused(lib):
    """maxlen = 131073: LL_EINVAL from both entry points and -1 from the workspace query, nothing launched (the buffers are a few bytes)"""
    L, D = SC.SPLIT_LIMIT + 1, 128
    t = torch.zeros(4096, dtype=R.BF, device="cuda")
    pos = torch.zeros(1, dtype=torch.long, device="cuda")
    p, st = t.data_ptr(), _stream()
    rc = [lib.ll_decode_attn_rope_split_bf16(p, 4 * D, p, p, 0, p, p, pos.data_ptr(), p, L, p, 1, 2, 1, L, D, D ** -0.5, None, None, 0.0, p, 1 << 40, st),
          lib.ll_suffix_attn_rope_split_bf16(p, 4 * D, p, p, p, p, pos.data_ptr(), p, p, 1, 1, 2, 1, L, D, D ** -0.5, None, None, 0.0, p, 1 << 40, st),
          int(lib.ll_attn_split_workspace_bytes(1, 1, 2, 1, L, D))]
    # the other bounds, on the same few bytes: 65 sequences, 17 new rows, a head size that has no instance, one norm weight only, a small workspace
    L = 1024
    rc += [lib.ll_decode_attn_rope_split_bf16(p, 4 * D, p, p, 0, p, p, pos.data_ptr(), p, L, p, 65, 2, 1, L, D, D ** -0.5, None, None, 0.0, p, 1 << 40, st),
           lib.ll_suffix_attn_rope_split_bf16(p, 4 * D, p, p, p, p, pos.data_ptr(), p, p, 1, 17, 2, 1, L, D, D ** -0.5, None, None, 0.0, p, 1 << 40, st),
           int(lib.ll_attn_split_workspace_bytes(1, 1, 2, 1, L, 96)),
           lib.ll_decode_attn_rope_split_bf16(p, 4 * D, p, p, 0, p, p, pos.data_ptr(), p, L, p, 1, 2, 1, L, D, D ** -0.5, p, None, 1e-6, p, 1 << 40, st),
           lib.ll_decode_attn_rope_split_bf16(p, 4 * D, p, p, 0, p, p, pos.data_ptr(), p, L, p, 1, 2, 1, L, D, D ** -0.5, None, None, 0.0, p, 64, st)]
    torch.cuda.synchronize()
    assert rc == [-1] * 8
    assert float(t.float().abs().max()) == 0.0
