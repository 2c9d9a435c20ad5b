"""The packed-weight (MX) decode Linears against the float64 reference and rounding intervals of tests/linear_reference.py on the cases of
tests/wq_reference.py, through the C ABI: ll_wq_quantize_bf16 / ll_wq_dequantize_bf16 against the independent float64 quantiser bit for bit,
ll_gemv_fused_wq (every M, ragged N down to 1, the RMSNorm prologue at XC = 2 | 4 with its switch at K = 4096 | 4128 and its limit, the
tail of the unrolled chunk loop, the x image padded to 64 chunks, the LDS limit per M) and ll_linear_rows16_wq (M 1..16, every geometry
ll_set_wq_geometry accepts, empty K slices, the RMSNorm in its staged form), both at 8 and 4 bits.

The kernels are judged against the weight quantize64 yields, after the device quantiser has been shown to yield the same: a quantiser bug
and a GEMV bug cannot cancel.  Every output element must lie in its interval [lo, hi]; column probes x[m] = c e_k on matrices whose scale
bytes vary along K and N (clamp ends, subnormals, saturating maxima included) pin every product and every scale byte; x, residual and output
are views with a loose row stride into NaN / sentinel memory, the packed buffer sits 16-byte (not 32-byte) aligned inside 0xFF bytes, and
everything outside [M, N] resp. the ll_wq_bytes window must survive.

-s prints, per kernel, width and path, the largest |got - chain(lin)| / (hi - lo) (1 is the edge of an interval); the figures measured on an
MI355X are in the docstring of tests/wq_reference.py."""
import pytest
import torch

from tests import linear_reference as L
from tests import wq_reference as R
from tests.test_decode_linear_reference_gpu import Dev

pytestmark = pytest.mark.gpu

WORST, COUNT = {}, {}
LL_EINVAL = -1
PACK_OFFSET = 48                 # of the packed window inside its allocation: a multiple of 16, not of 32


@pytest.fixture(scope="module")
def lib():
    from llamole_amd import _lib
    yield _lib.load()
    for path in sorted(WORST):
        print(f"\nlargest position inside the interval, {path}: {WORST[path]:.3f} ({COUNT[path]} calls)")


def _ok(rc, what):
    from llamole_amd import _lib
    _lib.check(rc, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------------------------ quantiser
def quantize(lib, src, bits, want, tag):
    """ll_wq_quantize_bf16 of src [rows,K] (device) given as a strided view inside NaN, into a window of an allocation of 0xFF bytes, Wdq with
    lddq = K + 8 inside sentinels; Wdq and the packed form read back through ll_wq_dequantize_bf16 must equal `want` bit for bit and nothing
    outside may change.  Returns (allocation, pointer to the packed form)."""
    rows, K = src.shape
    nbytes = int(lib.ll_wq_bytes(rows, K, bits))
    assert nbytes == rows * K * bits // 8 + rows * K // 32
    wb = L.padded(src, K + 40, rows_after=2)[0]
    alloc = torch.full((nbytes + 2 * PACK_OFFSET,), 0xFF, dtype=torch.uint8, device="cuda")
    ptr = alloc.data_ptr() + PACK_OFFSET
    assert ptr % 16 == 0 and ptr % 32 != 0
    dq = L.out_buffer(rows, K, K + 8, "cuda")
    _ok(lib.ll_wq_quantize_bf16(wb.data_ptr(), K + 40, rows, K, bits, ptr, dq.data_ptr(), K + 8, _stream()), tag)
    assert bool((alloc[:PACK_OFFSET] == 0xFF).all()) and bool((alloc[PACK_OFFSET + nbytes:] == 0xFF).all()), (tag, "wrote around the packed form")
    assert L.sentinel_damage(dq, rows, K) == 0, (tag, "Wdq: wrote outside [N, K]")
    assert torch.equal(_bits(dq[:rows, :K]), _bits(want)), (tag, "Wdq differs from quantize64")
    back = L.out_buffer(rows, K, K + 8, "cuda")
    _ok(lib.ll_wq_dequantize_bf16(ptr, rows, K, bits, back.data_ptr(), K + 8, _stream()), tag)
    assert L.sentinel_damage(back, rows, K) == 0, (tag, "ll_wq_dequantize_bf16: wrote outside [N, K]")
    assert torch.equal(_bits(back[:rows, :K]), _bits(want)), (tag, "the packed form differs from quantize64")
    return alloc, ptr


class WqDev(Dev):
    """an operand set of tests/wq_reference.py on the device: the poisoned views of Dev, the packed weight per call shape"""

    def __init__(self, lib, name, bits):
        self.lib, self.name, self.bits, self.o = lib, name, bits, R.operands(name, bits)
        o = self.o
        self.K, self.eps = o.K, o.eps
        self.x, self.src, self.w, self.bias, self.res = o.x.cuda(), o.src.cuda(), o.w.cuda(), o.bias.cuda(), o.res.cuda()
        self.norm_w = L.padded_vec(o.norm_w.cuda())
        self._b, self._x, self._r, self._p = {}, {}, {}, {}

    def packed(self, n, epi):
        """(pointer to the packed rows [:n] (SiLU*mul: gate rows [:n] then up rows [N:N+n]), bias + NaN)"""
        key = (n, epi == R.SILU_MUL)
        if key not in self._p:
            N = self.o.N
            rows = torch.cat((torch.arange(n), torch.arange(N, N + n))) if key[1] else torch.arange(n)
            rows = rows.cuda()
            alloc, ptr = quantize(self.lib, self.src[rows], self.bits, self.w[rows], f"{self.name} {self.bits} bits rows={len(rows)}")
            self._p[key] = (alloc, ptr, L.padded_vec(self.bias[rows]))
        return self._p[key][1:]


_DEV = {}


def dev(lib, name, bits):
    if (name, bits) not in _DEV:
        _DEV.clear()
        _DEV[(name, bits)] = WqDev(lib, name, bits)
    return _DEV[(name, bits)]


def verify(path, tag, d, out, M, n, form, use_bias, epi):
    assert L.sentinel_damage(out, M, n) == 0, (path, tag, "wrote outside [M, N]")
    outside, pos = L.check(out[:M, :n], *d.bounds(form, use_bias, epi, M, n))
    WORST[path] = max(WORST.get(path, 0.0), pos)
    COUNT[path] = COUNT.get(path, 0) + 1
    assert outside == 0, (path, tag, f"{outside} elements outside their interval, largest position {pos}")


def _call(fn, d, M, n, epi, form, use_bias, norm_form):
    xb, ldx = d.xbuf(M)
    ptr, bb = d.packed(n, epi)
    rb, ldr = d.resbuf(M, n) if epi == R.RESIDUAL else (None, 0)
    out = L.out_buffer(M, n, n + 40, "cuda")
    rc = fn(xb.data_ptr(), ldx, ptr, d.bits, _ptr(bb) if use_bias else None, _ptr(d.norm_w) if form == norm_form else None, d.eps, _ptr(rb), ldr,
            out.data_ptr(), n + 40, M, n, d.K, epi, _stream())
    return rc, out


# ------------------------------------------------------------------------------------------------------------------ ll_gemv_fused_wq
@pytest.mark.parametrize("name,bits", [c for c in R.CASES if c[0] in R.GEMV_SETS and R.has_intervals(*c)])
def test_gemv_fused_wq(lib, name, bits):
    """every M, N, epilogue, bias and norm setting of the set inside its interval; a row count whose x image passes the header's LDS rule
    (four rows of K = 18944 at 4 bits: 4 x 20480 elements) is refused and writes nothing"""
    d = dev(lib, name, bits)
    for form in R.forms(name, bits):
        where = "no norm" if form == R.NONE else f"RMSNorm prologue XC={2 if d.K <= 4096 else 4}"
        for epi in R.EPIS:
            for n in (R.GEMV_N_SILU if epi == R.SILU_MUL else R.GEMV_N):
                if n > d.o.N:
                    continue
                for M in range(1, d.o.M + 1):
                    for use_bias in (False, True):
                        rc, out = _call(lib.ll_gemv_fused_wq, d, M, n, epi, form, use_bias, R.HF)
                        tag = f"{name} {bits} bits M={M} N={n} epi={epi} {form} bias={use_bias}"
                        if R.gemv_lds_bytes(M, d.K, bits) > R.LDS_LIMIT:
                            assert rc == LL_EINVAL and L.sentinel_damage(out, 0, 0) == 0, (tag, rc)
                            continue
                        _ok(rc, tag)
                        verify(f"ll_gemv_fused_wq {bits} bits, {where}", tag, d, out, M, n, form, use_bias, epi)


# ------------------------------------------------------------------------------------------------------------------ ll_linear_rows16_wq
@pytest.mark.parametrize("name,bits", [c for c in R.CASES if c[0] in R.ROWS16_SETS])
def test_linear_rows16_wq(lib, name, bits):
    """every N, geometry, epilogue, norm and bias setting, at two to six row counts each (all of M over the sweep); K = 32 .. 160 with 2, 4 and
    8 slices has slices without a 32-block; a geometry whose LDS images pass 160 KB is refused with LL_EINVAL and writes nothing"""
    d = dev(lib, name, bits)
    turn = 0
    try:
        for ni, n in enumerate(R.ROWS16_N):
            if n > d.o.N:
                continue
            for gi, geom in enumerate(R.WQ_GEOMETRIES):
                lib.ll_set_wq_geometry(*geom)
                for epi in R.EPIS:
                    refused = geom[0] != 0 and R.rows16_wq_lds_bytes(bits, geom[0], geom[1], epi) > R.LDS_LIMIT
                    for form in R.forms(name, bits):
                        for use_bias in (False, True):
                            at = turn + gi + 5 * ni
                            for M in (R.ROWS16_M if gi == 0 else (R.ROWS16_M[at % 6], R.ROWS16_M[(at + 3) % 6])):
                                rc, out = _call(lib.ll_linear_rows16_wq, d, M, n, epi, form, use_bias, R.STAGED)
                                tag = f"{name} {bits} bits M={M} N={n} geometry={geom} epi={epi} {form} bias={use_bias}"
                                if refused:
                                    assert rc == LL_EINVAL and L.sentinel_damage(out, 0, 0) == 0, (tag, rc)
                                    continue
                                _ok(rc, tag)
                                path = f"ll_linear_rows16_wq {bits} bits, " + ("RMSNorm prologue" if form == R.STAGED else "no norm")
                                verify(path, tag, d, out, M, n, form, use_bias, epi)
                            turn += 1
    finally:
        lib.ll_set_wq_geometry(0, 0, 0)


def test_the_check_tells_the_two_widths_apart(lib):
    """the device side of the check is not vacuous: a correct 8-bit output held against the intervals of the same matrix rounded to 4 bits
    leaves them almost everywhere, and so does a 4-bit output against the 8-bit intervals"""
    M, n = 5, 17
    for bits, other in ((8, 4), (4, 8)):
        d = dev(lib, "wq-rows16-K160", bits)
        rc, out = _call(lib.ll_linear_rows16_wq, d, M, n, R.PLAIN, R.NONE, True, R.STAGED)
        _ok(rc, "ll_linear_rows16_wq")
        assert L.check(out[:M, :n], *d.bounds(R.NONE, True, R.PLAIN, M, n))[0] == 0
        wrong = tuple(t[:M, :n] for t in R.operands("wq-rows16-K160", other).bounds(R.NONE, True, R.PLAIN))
        assert L.check(out[:M, :n], *wrong)[0] > 0.5 * M * n


# ------------------------------------------------------------------------------------------------------------------ column probes
def probe_set(w, K, M, n):
    """[(x allocation with ldx = K + 8, expected output allocation with ldc = n + 40)] of the probe launches of M rows; w: quantize64's W on
    the host (the expected values are formed there, where 0.5 * 2^-126 is certain to stay a subnormal)"""
    launches = L.probe_launches(K, M)
    exp = torch.stack([R.probe_expected(w[:n], ks, cs) for ks, cs in launches]).cuda()
    for i, (ks, cs) in enumerate(launches):
        want = L.out_buffer(M, n, n + 40, "cuda")
        want[:M, :n] = exp[i]
        yield L.padded(L.probe_x(K, ks, cs, "cuda"), K + 8)[0], want


def run_probes(call, probes, K, M, n, what):
    """call(xbuf, ldx, out, ldc) on every probe launch: out[m, :] must be bf16(c W[:n, k]) bit for bit, the sentinel around it intact"""
    wrong = torch.zeros((), dtype=torch.long, device="cuda")
    count = 0
    for xb, want in probes:
        out = L.out_buffer(M, n, n + 40, "cuda")
        call(xb, K + 8, out, n + 40)
        wrong += (_bits(out) != _bits(want)).sum()
        count += 1
    assert int(wrong) == 0, (what, f"{int(wrong)} elements differ from c W[:, k] over {count} probe launches")


def _probe_weight(lib, bits, n, K, tag):
    src = R.probe_matrix(bits, n, K)
    w, _ = R.quantize64(src, bits)
    alloc, ptr = quantize(lib, src.cuda(), bits, w.cuda(), tag)
    return w, alloc, ptr


@pytest.mark.parametrize("name,bits", [c for c in R.CASES if c[0] in R.GEMV_SETS and "eps" not in c[0]])
def test_gemv_fused_wq_column_probes(lib, name, bits):
    """the set's K with the largest of its row counts the LDS rule admits (the limit of one row included: 80896 / 79872 elements of x in
    LDS, the deepest chunk loop)"""
    M, N, K, _ = R.shape(name, bits)
    M = max(m for m in range(1, M + 1) if R.gemv_lds_bytes(m, K, bits) <= R.LDS_LIMIT)
    n = min(9, N)
    w, alloc, ptr = _probe_weight(lib, bits, n, K, f"{name} {bits} bits probes")

    def call(xb, ldx, out, ldc):
        _ok(lib.ll_gemv_fused_wq(xb.data_ptr(), ldx, ptr, bits, None, None, L.EPS, None, 0, out.data_ptr(), ldc, M, n, K, R.PLAIN, _stream()), name)
    run_probes(call, probe_set(w, K, M, n), K, M, n, f"{name} {bits} bits M={M}")


@pytest.mark.parametrize("name,bits", [c for c in R.CASES if c[0] in R.ROWS16_SETS and "eps" not in c[0]])
def test_linear_rows16_wq_column_probes(lib, name, bits):
    _, _, K, _ = R.shape(name, bits)
    M, n = 16, 17
    w, alloc, ptr = _probe_weight(lib, bits, n, K, f"{name} {bits} bits probes")

    def call(xb, ldx, out, ldc):
        _ok(lib.ll_linear_rows16_wq(xb.data_ptr(), ldx, ptr, bits, None, None, L.EPS, None, 0, out.data_ptr(), ldc, M, n, K, R.PLAIN, _stream()), name)
    probes = list(probe_set(w, K, M, n))
    try:
        for geom in R.WQ_GEOMETRIES:
            if geom[0] != 0 and R.rows16_wq_lds_bytes(bits, geom[0], geom[1], R.PLAIN) > R.LDS_LIMIT:
                continue
            lib.ll_set_wq_geometry(*geom)
            run_probes(call, probes, K, M, n, f"{name} {bits} bits geometry={geom}")
    finally:
        lib.ll_set_wq_geometry(0, 0, 0)


# ------------------------------------------------------------------------------------------------------------------ refusals
def _zeros(lib, bits, rows, K):
    """(x zeros [4,K], allocation, pointer to a packed all-zero matrix [rows,K])"""
    z = torch.zeros(rows, K, dtype=R.BF, device="cuda")
    alloc, ptr = quantize(lib, z, bits, z, "zeros")
    return torch.zeros(16, K, dtype=R.BF, device="cuda"), alloc, ptr


def _refused(fn, x, ptr, bits, M, n, K, norm_w=None, ldx=None):
    out = L.out_buffer(max(M, 1), n, n + 40, "cuda")
    rc = fn(x.data_ptr(), K if ldx is None else ldx, ptr, bits, None, _ptr(norm_w), L.EPS, None, 0, out.data_ptr(), n + 40, M, n, K, R.PLAIN, _stream())
    torch.cuda.synchronize()
    return rc == LL_EINVAL and L.sentinel_damage(out, 0, 0) == 0


def _served(fn, x, ptr, bits, M, n, K, norm_w=None):
    """zero weights: the call is served and writes zeros to [M, N] only"""
    out = L.out_buffer(M, n, n + 40, "cuda")
    _ok(fn(x.data_ptr(), K, ptr, bits, None, _ptr(norm_w), L.EPS, None, 0, out.data_ptr(), n + 40, M, n, K, R.PLAIN, _stream()), "served")
    return float(out[:M, :n].float().abs().max()) == 0.0 and L.sentinel_damage(out, M, n) == 0


@pytest.mark.parametrize("bits", R.BITS)
def test_gemv_fused_wq_lds_limit(lib, bits):
    """per M the largest K of the header's rule is served and K + 32 refused, where one row fewer is still served; the limits come from the rule"""
    n = 8
    for M in R.GEMV_M:
        K = R.gemv_k_limit(M, bits)
        x, alloc, ptr = _zeros(lib, bits, n, K + 32)
        assert _refused(lib.ll_gemv_fused_wq, x, ptr, bits, M, n, K + 32), (M, K + 32, "not refused")
        assert M == 1 or _served(lib.ll_gemv_fused_wq, x, ptr, bits, M - 1, n, K + 32), (M - 1, K + 32)
        x, alloc, ptr = _zeros(lib, bits, n, K)
        assert _served(lib.ll_gemv_fused_wq, x, ptr, bits, M, n, K), (M, K)
    if bits == 8:
        x, alloc, ptr = _zeros(lib, bits, n, 20480)
        assert _refused(lib.ll_gemv_fused_wq, x, ptr, bits, 4, n, 20480) and _served(lib.ll_gemv_fused_wq, x, ptr, bits, 3, n, 20480)


@pytest.mark.parametrize("bits", R.BITS)
def test_refusals(lib, bits):
    """LL_EINVAL before anything is launched, the output untouched: the RMSNorm prologue above K = 8192 (K = 8224; served without the norm, and
    K = 8192 with it runs in test_gemv_fused_wq), M out of range, K % 32 != 0, a packed pointer that is not 16-byte aligned"""
    n = 8
    K = R.GEMV_K_NORM_LIMIT + 32
    x, alloc, ptr = _zeros(lib, bits, n, K)
    nw = torch.ones(K, dtype=R.BF, device="cuda")
    gemv, rows16 = lib.ll_gemv_fused_wq, lib.ll_linear_rows16_wq
    for M in R.GEMV_M:
        assert _refused(gemv, x, ptr, bits, M, n, K, norm_w=nw), (M, "norm beyond 8192")
        assert _served(gemv, x, ptr, bits, M, n, K), (M, "no norm")
    assert _served(rows16, x, ptr, bits, 4, n, K, norm_w=nw)                       # the MFMA kernel has no such limit
    for M in (0, 5, -1):
        assert _refused(gemv, x, ptr, bits, M, n, K), ("gemv", M)
    for M in (0, 17, -1):
        assert _refused(rows16, x, ptr, bits, M, n, K), ("rows16", M)
    for fn, M in ((gemv, 4), (rows16, 16)):
        for bad in (16, 48, K - 8, K - 16):
            assert _refused(fn, x, ptr, bits, M, n, bad, ldx=K), (M, bad, "K % 32")
        assert _refused(fn, x, ptr + 8, bits, M, n, K) and _refused(fn, x, ptr + 4, bits, M, n, K), (M, "misaligned packed pointer")
        assert _served(fn, x, ptr, bits, M, n, K)


# ------------------------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("bits", R.BITS)
@pytest.mark.parametrize("n,K", [(9, 32), (17, 288), (9, 1056), (17, 18944)])
def test_quantiser_on_the_probe_matrices(lib, bits, n, K):
    """both clamp ends of the shared exponent, bf16 subnormals, saturating maxima and the threshold of the scale rule, on the device"""
    _probe_weight(lib, bits, n, K, f"probe matrix {n}x{K} {bits} bits")


@pytest.mark.parametrize("bits", R.BITS)
def test_quantiser_grid_stride(lib, bits):
    """N K / 8 > 65536 x 256: the grid cap is reached and the loops of the quantiser and of the dequantiser iterate.  A 64-row pattern (a probe
    matrix: every special block) repeated 513 times, compared slice against slice on the device against the 64 reference rows"""
    K, reps = 4096, 513
    assert 64 * reps * K // 8 > 65536 * 256
    src = R.probe_matrix(bits, 64, K)
    want = R.quantize64(src, bits)[0].cuda()
    big = src.cuda().repeat(reps, 1)
    N = 64 * reps
    nbytes = int(lib.ll_wq_bytes(N, K, bits))
    alloc = torch.full((nbytes + 2 * PACK_OFFSET,), 0xFF, dtype=torch.uint8, device="cuda")
    ptr = alloc.data_ptr() + PACK_OFFSET
    dq = torch.full((N, K), L.SENTINEL, dtype=torch.int16, device="cuda").view(R.BF)
    _ok(lib.ll_wq_quantize_bf16(big.data_ptr(), K, N, K, bits, ptr, dq.data_ptr(), K, _stream()), "ll_wq_quantize_bf16")
    assert bool((alloc[:PACK_OFFSET] == 0xFF).all()) and bool((alloc[PACK_OFFSET + nbytes:] == 0xFF).all())
    assert bool((_bits(dq).view(reps, 64, K) == _bits(want)).all()), "Wdq"
    dq.view(torch.int16).fill_(L.SENTINEL)
    _ok(lib.ll_wq_dequantize_bf16(ptr, N, K, bits, dq.data_ptr(), K, _stream()), "ll_wq_dequantize_bf16")
    assert bool((_bits(dq).view(reps, 64, K) == _bits(want)).all()), "packed"
