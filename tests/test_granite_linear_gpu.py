"""The scaled residual entries (ll_gemv_fused_rs_bf16, ll_linear_rows16_rs_bf16, ll_linear_rows64_rs_bf16) and ll_embed_rows_bf16 through the
C ABI, against the intervals of tests/test_granite_reference_cpu.py (the float64 reference of tests/linear_reference.py with the chain
bf16r(res + bf16r(bf16r(v) * f32(m)))).  Operands are poisoned views and outputs sit in sentinel-filled allocations, as in
tests/test_decode_linear_reference_gpu.py, whose device-side helpers are reused.

Every case runs with m = 0.22 and m = -0.5 (no element outside its interval, every sentinel intact) and with m = 1.0, where the scaled entry
must give the bits of the unscaled entry on the same operands.
  GEMV    M 1..4 on gemv-K2048, gemv-K4104, gemv-K20488 (N = 9) and, for the kernel that stages x in LDS (one row, 8192 <= K <= 20480),
          gemv-K8192; with and without bias.
  rows16  M 3, 5, 16 on rows16-K32 (the family's smallest set) and rows16-K160.
  rows64  M 17, 33, 64 on rows64-K32 (the smallest set): one launch, and the K split with a workspace (forced to 2 and 8 slices: at K = 32
          the launcher would not split), with and without next_norm_w; rows64-K1056 at M = 33 with the launcher's own split.  scaled_out /
          ssq_out are checked from the kernel's own scaled-residual output row, as _verify_next_norm does.
  embed   bit-equal to (table[ids].float() * f32(m)).to(bf16) for M 1, 7, 64, H 256, 4096 and 328 (a multiple of 8, not of 64), ids at 0 and
          V - 1; an id outside [0, V) gives a row of zeros; a zero or non-finite scale is refused and nothing is written."""
import pytest
import torch

from tests import linear_reference as R
from tests import test_decode_linear_reference_gpu as G
from tests import test_granite_reference_cpu as C

pytestmark = pytest.mark.gpu

SCALES = (0.22, -0.5)
LL_EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from llamole_amd import _lib
    return _lib.load()


_BOUNDS = {}


def bounds(d, use_bias, m, M, n):
    key = (d.name, bool(use_bias), m)
    if key not in _BOUNDS:
        if len(_BOUNDS) > 8:
            _BOUNDS.clear()
        _BOUNDS[key] = tuple(t.cuda() for t in C.scaled_bounds(d.o, use_bias, m))
    return tuple(t[:M, :n] for t in _BOUNDS[key])


def verify(tag, d, out, M, n, use_bias, m):
    assert R.sentinel_damage(out, M, n) == 0, (tag, "wrote outside [M, N]")
    outside, pos = R.check(out[:M, :n], *bounds(d, use_bias, m, M, n))
    assert outside == 0, (tag, f"{outside} elements outside their interval, largest position {pos}")


# ------------------------------------------------------------------------------------------------------------------ GEMV
def _gemv_rs(lib, d, M, n, use_bias, m):
    xb, ldx = d.xbuf(M)
    wb, ldw, bb = d.wbuf(n, R.RESIDUAL)
    rb, ldr = d.resbuf(M, n)
    out = R.out_buffer(M, n, n + 40, "cuda")
    rc = lib.ll_gemv_fused_rs_bf16(xb.data_ptr(), ldx, wb.data_ptr(), ldw, G._ptr(bb) if use_bias else None, rb.data_ptr(), ldr, out.data_ptr(),
                                   n + 40, M, n, d.K, m, G._stream())
    return rc, out


@pytest.mark.parametrize("name", ["gemv-K2048", "gemv-K4104", "gemv-K8192", "gemv-K20488"])
def test_gemv_fused_rs(lib, name):
    d = G.dev(name)
    for n in sorted({min(9, d.o.N), d.o.N}):
        for M in (1, 2, 3, 4):
            for use_bias in (False, True):
                for m in SCALES:
                    tag = f"{name} M={M} N={n} bias={use_bias} m={m}"
                    rc, out = _gemv_rs(lib, d, M, n, use_bias, m)
                    G._ok(rc, tag)
                    verify(tag, d, out, M, n, use_bias, m)
                rc, one = _gemv_rs(lib, d, M, n, use_bias, 1.0)
                G._ok(rc, "m = 1")
                rc, plain = G._gemv(lib, d, M, n, R.RESIDUAL, R.NONE, use_bias)
                G._ok(rc, "unscaled")
                assert torch.equal(G._bits(one), G._bits(plain)), (name, M, n, use_bias, "m = 1 is not the unscaled entry, bit for bit")


# ------------------------------------------------------------------------------------------------------------------ rows16
def _rows16_rs(lib, d, M, n, use_bias, m):
    xb, ldx = d.xbuf(M)
    wb, ldw, bb = d.wbuf(n, R.RESIDUAL)
    rb, ldr = d.resbuf(M, n)
    out = R.out_buffer(M, n, n + 40, "cuda")
    rc = lib.ll_linear_rows16_rs_bf16(xb.data_ptr(), ldx, wb.data_ptr(), ldw, G._ptr(bb) if use_bias else None, rb.data_ptr(), ldr, out.data_ptr(),
                                      n + 40, M, n, d.K, m, G._stream())
    return rc, out


@pytest.mark.parametrize("name", ["rows16-K32", "rows16-K160"])
def test_linear_rows16_rs(lib, name):
    d = G.dev(name)
    for n in (17, d.o.N):
        for M in (3, 5, 16):
            for use_bias in (False, True):
                for m in SCALES:
                    tag = f"{name} M={M} N={n} bias={use_bias} m={m}"
                    rc, out = _rows16_rs(lib, d, M, n, use_bias, m)
                    G._ok(rc, tag)
                    verify(tag, d, out, M, n, use_bias, m)
                rc, one = _rows16_rs(lib, d, M, n, use_bias, 1.0)
                G._ok(rc, "m = 1")
                rc, plain = G._rows16(lib, d, M, n, R.RESIDUAL, R.NONE, use_bias)
                G._ok(rc, "unscaled")
                assert torch.equal(G._bits(one), G._bits(plain)), (name, M, n, use_bias, "m = 1 is not the unscaled entry, bit for bit")


# ------------------------------------------------------------------------------------------------------------------ rows64
def _rows64_rs(lib, d, packed, bb, M, n, use_bias, ws, norm, m, tag):
    """one call of the scaled entry (m is None: the unscaled entry at the residual epilogue); out, scaled_out, ssq_out"""
    if m is None:
        xb, ldx = d.xbuf(M)
        return G._rows64(lib, d, packed, bb, M, n, R.RESIDUAL, use_bias, xb, ldx, None, ws, norm, tag)
    xb, ldx = d.xbuf(M)
    rb, ldr = d.resbuf(M, n)
    out = R.out_buffer(M, n, n + 40, "cuda")
    nch = int(lib.ll_rows64_ssq_chunks(n))
    xs = R.out_buffer(M, n, n + 24, "cuda") if norm else None
    ssq = torch.full((M + 1, nch), R.SENTINEL_F32, device="cuda") if norm else None
    wsb = int(lib.ll_linear_rows64_workspace_bytes(M, n))
    assert ws is None or ws.numel() * 4 >= wsb
    G._ok(lib.ll_linear_rows64_rs_bf16(xb.data_ptr(), ldx, packed.data_ptr(), G._ptr(bb) if use_bias else None, rb.data_ptr(), ldr, out.data_ptr(),
                                       n + 40, M, n, d.K, None, 0, d.eps, G._ptr(d.next_norm_w) if norm else None, G._ptr(xs), n + 24, G._ptr(ssq),
                                       G._ptr(ws), wsb if ws is not None else 0, m, G._stream()), tag)
    return out, xs, ssq


def _run_rows64(lib, d, n, rows, plan):
    packed, bb = G._pack(lib, d, n, R.PLAIN)
    ws = torch.empty(8 * 64 * n, dtype=torch.float32, device="cuda")
    try:
        for M in rows:
            for ksg, use_ws, norm in plan:
                lib.ll_set_rows64_ksplit(ksg)
                for use_bias in (False, True):
                    base = f"{d.name} M={M} N={n} ksplit={ksg} ws={use_ws} next_norm={norm} bias={use_bias}"
                    for m in SCALES:
                        tag = f"{base} m={m}"
                        out, xs, ssq = _rows64_rs(lib, d, packed, bb, M, n, use_bias, ws if use_ws else None, norm, m, tag)
                        verify(tag, d, out, M, n, use_bias, m)
                        if norm:
                            G._verify_next_norm(d, tag, out, xs, ssq, M, n)     # from the scaled-residual row the kernel wrote
                    one = _rows64_rs(lib, d, packed, bb, M, n, use_bias, ws if use_ws else None, norm, 1.0, base)
                    plain = _rows64_rs(lib, d, packed, bb, M, n, use_bias, ws if use_ws else None, norm, None, base)
                    assert torch.equal(G._bits(one[0]), G._bits(plain[0])), (base, "m = 1 is not the unscaled entry, bit for bit")
                    if norm:
                        assert torch.equal(G._bits(one[1]), G._bits(plain[1])) and torch.equal(one[2], plain[2]), (base, "m = 1: pre-norm differs")
    finally:
        lib.ll_set_rows64_ksplit(0)


# (K slices forced, workspace given, next_norm_w given): one launch; the K split; the slab sum with the next layer's pre-norm
ROWS64_PLAN = [(0, False, False), (0, True, False), (2, True, False), (8, True, False), (0, True, True), (2, True, True)]


@pytest.mark.parametrize("n", [80, 1003])
def test_linear_rows64_rs_smallest_set(lib, n):
    _run_rows64(lib, G.dev("rows64-K32"), n, (17, 33, 64), ROWS64_PLAN)


def test_linear_rows64_rs_the_launchers_own_split(lib):
    _run_rows64(lib, G.dev("rows64-K1056"), 1032, (33,), [(0, False, False), (0, True, False), (0, True, True)])


@pytest.mark.parametrize("bad", [0.0, float("nan"), float("inf")])
def test_a_bad_scale_is_refused_and_nothing_is_written(lib, bad):
    d = G.dev("rows16-K32")
    rc, out = _gemv_rs(lib, d, 2, 17, True, bad)
    rc16, out16 = _rows16_rs(lib, d, 5, 17, True, bad)
    torch.cuda.synchronize()
    assert rc == LL_EINVAL and rc16 == LL_EINVAL and R.sentinel_damage(out, 0, 0) == 0 and R.sentinel_damage(out16, 0, 0) == 0
    d64 = G.dev("rows64-K32")
    packed, bb = G._pack(lib, d64, 80, R.PLAIN)
    xb, ldx = d64.xbuf(17)
    rb, ldr = d64.resbuf(17, 80)
    out64 = R.out_buffer(17, 80, 120, "cuda")
    rc64 = lib.ll_linear_rows64_rs_bf16(xb.data_ptr(), ldx, packed.data_ptr(), None, rb.data_ptr(), ldr, out64.data_ptr(), 120, 17, 80, d64.K, None, 0,
                                        d64.eps, None, None, 0, None, None, 0, bad, G._stream())
    table = torch.zeros(8, 64, dtype=R.BF, device="cuda")
    oute = R.out_buffer(2, 64, 64, "cuda")
    rce = lib.ll_embed_rows_bf16(torch.zeros(2, dtype=torch.long, device="cuda").data_ptr(), table.data_ptr(), 64, oute.data_ptr(), 64, 2, 8, 64, bad,
                                 G._stream())
    torch.cuda.synchronize()
    assert rc64 == LL_EINVAL and rce == LL_EINVAL and R.sentinel_damage(out64, 0, 0) == 0 and R.sentinel_damage(oute, 0, 0) == 0
    # the unscaled entry does not take the scaled epilogue's number
    rc = lib.ll_linear_rows64_bf16(xb.data_ptr(), ldx, packed.data_ptr(), None, rb.data_ptr(), ldr, out64.data_ptr(), 120, 17, 80, d64.K, 3, None, 0,
                                   d64.eps, None, None, 0, None, None, 0, G._stream())
    torch.cuda.synchronize()
    assert rc == LL_EINVAL and R.sentinel_damage(out64, 0, 0) == 0


# ------------------------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("H", [256, 328, 4096])
def test_embed_rows(lib, H):
    from llamole_amd.llm_accel import hf_scaled_embedding
    V = 131
    g = torch.Generator().manual_seed(H)
    table_buf, table = R.padded(torch.randn(V, H, generator=g).to(R.BF).cuda(), H + 8, rows_after=2)       # NaN behind every row
    for M in (1, 7, 64):
        ids = torch.randint(0, V, (M,), generator=g)
        ids[0], ids[-1] = 0, V - 1
        if M == 7:
            ids[1], ids[2] = V - 1, 0
        ids = ids.cuda()
        for m in (12.0, 0.22, -0.5):
            out = R.out_buffer(M, H, H + 24, "cuda")
            G._ok(lib.ll_embed_rows_bf16(ids.data_ptr(), table_buf.data_ptr(), H + 8, out.data_ptr(), H + 24, M, V, H, m, G._stream()), "ll_embed_rows_bf16")
            assert R.sentinel_damage(out, M, H) == 0
            want = (table[ids].float() * torch.tensor(m, dtype=torch.float32)).to(R.BF)
            assert torch.equal(want, hf_scaled_embedding(table, ids, m))
            assert torch.equal(G._bits(out[:M, :H]), G._bits(want)), (H, M, m)
    # ids outside [0, V): rows of zeros, nothing read
    ids = torch.tensor([V, -1, 5, 1 << 40], device="cuda")
    out = R.out_buffer(4, H, H + 24, "cuda")
    G._ok(lib.ll_embed_rows_bf16(ids.data_ptr(), table_buf.data_ptr(), H + 8, out.data_ptr(), H + 24, 4, V, H, 12.0, G._stream()), "ll_embed_rows_bf16")
    assert R.sentinel_damage(out, 4, H) == 0
    assert float(out[[0, 1, 3], :H].float().abs().max()) == 0.0
    assert torch.equal(G._bits(out[2, :H]), G._bits(hf_scaled_embedding(table, ids[2:3], 12.0)[0]))
