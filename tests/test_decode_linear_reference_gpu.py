"""The decode Linears against the float64 reference and rounding intervals of tests/linear_reference.py, through the C ABI:
ll_gemv_fused_bf16 (both kernels, the RMSNorm prologue at XC = 2 | 4 and its limit, every M, ragged N, K % 32 != 0, the stage / non-temporal
switches), ll_linear_rows16_bf16 (M 1..16, every geometry ll_set_rows16_geometry accepts, empty K slices, the HF RMSNorm in its staged form),
ll_linear_rows64_bf16 with ll_rows64_pack_bf16 and ll_rows64_prenorm_bf16 (M 1..64, N 1..2584, every K split, with and without workspace,
the split RMSNorm on both sides), and the plain ll_linear(LL_BF16) / ll_linear_splitk_bf16 a decode reaches.

One reference per operand set, many kernel configurations against it.  Every output element must lie in its interval [lo, hi] (most are
pinned bit for bit); column probes x[m] = c e_k pin every product; every operand is a view with a loose row stride into an allocation whose
other bytes are NaN (inputs) or a sentinel (outputs), and the sentinel must survive everywhere outside [M, N].

-s prints, per kernel and path, the largest |got - chain(lin)| / (hi - lo) (1 is the edge of an interval); the figures measured on an MI355X
are in the docstring of tests/linear_reference.py."""
import pytest
import torch

from tests import linear_reference as R

pytestmark = pytest.mark.gpu

WORST, COUNT = {}, {}
LL_EINVAL = -1


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


class Dev:
    """an operand set on the device: poisoned views per call shape, the intervals as float32"""

    def __init__(self, name):
        self.name, self.o = name, R.operands(name)
        o = self.o
        self.K, self.eps = o.K, o.eps
        self.x, self.w, self.bias, self.res = o.x.cuda(), o.w.cuda(), o.bias.cuda(), o.res.cuda()
        self.norm_w = R.padded_vec(o.norm_w.cuda())
        self.next_norm_w = o.next_norm_w.cuda()
        self._b, self._x, self._w, self._r = {}, {}, {}, {}

    def bounds(self, form, use_bias, epi, M, n):
        key = (form, bool(use_bias), epi)
        if key not in self._b:
            self._b[key] = tuple(t.cuda() for t in self.o.bounds(form, use_bias, epi))
        return tuple(t[:M, :n] for t in self._b[key])

    def xbuf(self, M):
        """x[:M] with ldx = K + 8, NaN behind every row and in the row after the last"""
        if M not in self._x:
            self._x[M] = R.padded(self.x[:M], self.K + 8)[0]
        return self._x[M], self.K + 8

    def wbuf(self, n, epi):
        """(weight allocation with ldw = K + 40 and two NaN rows behind the last, ldw, bias + NaN)"""
        key = (n, epi == R.SILU_MUL)
        if key not in self._w:
            o = self.o
            if epi == R.SILU_MUL:
                w, b = torch.cat((self.w[:n], self.w[o.N:o.N + n])), torch.cat((self.bias[:n], self.bias[o.N:o.N + n]))
            else:
                w, b = self.w[:n], self.bias[:n]
            if len(self._w) > 24:
                self._w.clear()
            self._w[key] = (R.padded(w, self.K + 40, rows_after=2)[0], self.K + 40, R.padded_vec(b))
        return self._w[key]

    def resbuf(self, M, n):
        key = (M, n)
        if key not in self._r:
            if len(self._r) > 64:
                self._r.clear()
            self._r[key] = R.padded(self.res[:M, :n], n + 8)[0]
        return self._r[key], n + 8


_DEV = {}


def dev(name):
    if name not in _DEV:
        _DEV.clear()
        _DEV[name] = Dev(name)
    return _DEV[name]


def verify(path, tag, d, out, M, n, form, use_bias, epi):
    assert R.sentinel_damage(out, M, n) == 0, (path, tag, "wrote outside [M, N]")
    outside, pos = R.check(out[:M, :n], *d.bounds(form, use_bias, epi, M, n))
    WORST[path] = max(WORST.get(path, 0.0), pos)
    COUNT[path] = COUNT.get(path, 0) + 1
    assert outside == 0, (path, tag, f"{outside} elements outside their interval, largest position {pos}")


def _bits(t):
    return t.contiguous().view(torch.int16)


def probe_set(w, K, M, n):
    """[(x allocation with ldx = K + 8, expected output allocation with ldc = n + 40)] of the probe launches of M rows"""
    out = []
    for ks, cs in R.probe_launches(K, M):
        want = R.out_buffer(M, n, n + 40, "cuda")
        want[:M, :n] = R.probe_expected(w[:n], ks, cs)
        out.append((R.padded(R.probe_x(K, ks, cs, "cuda"), K + 8)[0], want))
    return out


def run_probes(call, probes, K, M, n, what):
    """call(xbuf, ldx, out, ldc) on every probe launch: out[m, :] must be bf16(c W[:n, k]) bit for bit, the sentinel around it intact"""
    wrong = torch.zeros((), dtype=torch.long, device="cuda")
    for xb, want in probes:
        out = R.out_buffer(M, n, n + 40, "cuda")
        call(xb, K + 8, out, n + 40)
        wrong += (_bits(out) != _bits(want)).sum()
    assert int(wrong) == 0, (what, f"{int(wrong)} elements differ from c W[:, k] over {len(probes)} probe launches")


# ------------------------------------------------------------------------------------------------------------------ ll_gemv_fused_bf16
def _gemv(lib, d, M, n, epi, form, use_bias, out=None):
    xb, ldx = d.xbuf(M)
    wb, ldw, bb = d.wbuf(n, epi)
    rb, ldr = d.resbuf(M, n) if epi == R.RESIDUAL else (None, 0)
    out = R.out_buffer(M, n, n + 40, "cuda") if out is None else out
    rc = lib.ll_gemv_fused_bf16(xb.data_ptr(), ldx, wb.data_ptr(), ldw, _ptr(bb) if use_bias else None, _ptr(d.norm_w) if form == R.HF else None,
                                d.eps, _ptr(rb), ldr, out.data_ptr(), n + 40, M, n, d.K, epi, _stream())
    return rc, out


def _gemv_path(M, K, epi, form, stage, nt):
    staged = stage and nt and M == 1 and form == R.NONE and epi != R.SILU_MUL and 8192 <= K <= 20480
    return "ll_gemv_fused_bf16 " + ("x staged in LDS" if staged else "RMSNorm prologue" if form == R.HF else "generic")


@pytest.mark.parametrize("name", sorted(R.GEMV_SETS))
def test_gemv_fused(lib, name):
    """every M, N, epilogue, bias and norm setting of the set under the four settings of the stage / non-temporal switches: inside the
    intervals and bit-identical to each other"""
    d = dev(name)
    try:
        for form in R.forms(name):
            for epi in R.EPIS:
                for n in (R.GEMV_N_SILU if epi == R.SILU_MUL else R.GEMV_N):
                    if n > d.o.N:
                        continue
                    for M in R.GEMV_M:
                        for use_bias in (False, True):
                            first = None
                            for stage, nt in ((1, 1), (0, 1), (1, 0), (0, 0)):
                                lib.ll_set_gemv_stage(stage)
                                lib.ll_set_gemv_nt(nt)
                                rc, out = _gemv(lib, d, M, n, epi, form, use_bias)
                                tag = f"{name} M={M} N={n} epi={epi} {form} bias={use_bias} stage={stage} nt={nt}"
                                _ok(rc, tag)
                                verify(_gemv_path(M, d.K, epi, form, stage, nt), tag, d, out, M, n, form, use_bias, epi)
                                if first is None:
                                    first = out
                                else:
                                    assert torch.equal(_bits(out), _bits(first)), (tag, "differs from stage=1 nt=1")
    finally:
        lib.ll_set_gemv_stage(1)
        lib.ll_set_gemv_nt(1)


@pytest.mark.parametrize("name", sorted(n for n in R.GEMV_SETS if "eps" not in n))
def test_gemv_fused_column_probes(lib, name):
    d = dev(name)
    n = min(9, d.o.N)
    wb, ldw, _ = d.wbuf(n, R.PLAIN)
    for M in ((4, 1) if 8192 <= d.K <= 20480 else (4,)):       # one row: the kernel that stages x in LDS
        def call(xb, ldx, out, ldc):
            _ok(lib.ll_gemv_fused_bf16(xb.data_ptr(), ldx, wb.data_ptr(), ldw, None, None, d.eps, None, 0, out.data_ptr(), ldc, M, n, d.K, R.PLAIN,
                                       _stream()), "ll_gemv_fused_bf16")
        run_probes(call, probe_set(d.w, d.K, M, n), d.K, M, n, f"{name} M={M}")


def test_gemv_fused_refuses_a_norm_beyond_its_limits(lib):
    """RMSNorm prologue: K <= 8192 and M K <= 32768 (which K <= 8192 implies for M <= 4: K = 8192 at M = 4 is the largest, and runs in
    test_gemv_fused); K = 8200 is refused for one row and for four, nothing is launched"""
    K = R.GEMV_K_NORM_LIMIT + 8
    x = torch.zeros(4, K, dtype=R.BF, device="cuda")
    w = torch.zeros(8, K, dtype=R.BF, device="cuda")
    for M in (1, 4):
        assert M * K > 32768 or M == 1
        out = R.out_buffer(M, 8, 48, "cuda")
        rc = lib.ll_gemv_fused_bf16(x.data_ptr(), K, w.data_ptr(), K, None, x.data_ptr(), 1e-6, None, 0, out.data_ptr(), 48, M, 8, K, R.PLAIN, _stream())
        torch.cuda.synchronize()
        assert rc == LL_EINVAL and R.sentinel_damage(out, 0, 0) == 0
        _ok(lib.ll_gemv_fused_bf16(x.data_ptr(), K, w.data_ptr(), K, None, None, 1e-6, None, 0, out.data_ptr(), 48, M, 8, K, R.PLAIN, _stream()), "no norm")
        assert float(out[:M, :8].float().abs().max()) == 0.0 and R.sentinel_damage(out, M, 8) == 0


# ------------------------------------------------------------------------------------------------------------------ ll_linear_rows16_bf16
def _rows16(lib, d, M, n, epi, form, use_bias, out=None):
    xb, ldx = d.xbuf(M)
    wb, ldw, bb = d.wbuf(n, epi)
    rb, ldr = d.resbuf(M, n) if epi == R.RESIDUAL else (None, 0)
    out = R.out_buffer(M, n, n + 40, "cuda") if out is None else out
    rc = lib.ll_linear_rows16_bf16(xb.data_ptr(), ldx, wb.data_ptr(), ldw, _ptr(bb) if use_bias else None,
                                   _ptr(d.norm_w) if form == R.STAGED else None, d.eps, _ptr(rb), ldr, out.data_ptr(), n + 40, M, n, d.K, epi, _stream())
    return rc, out


@pytest.mark.parametrize("name", sorted(R.ROWS16_SETS))
def test_linear_rows16(lib, name):
    """every N, geometry, epilogue, norm and bias setting, at two to six row counts each (all of M over the sweep); K = 32 .. 160 with 4 and 8 slices has
    slices without a k-step; a geometry whose LDS images pass 160 KB is refused with LL_EINVAL and writes nothing"""
    d = dev(name)
    turn = 0
    try:
        for ni, n in enumerate(R.ROWS16_N):
            if n > d.o.N:
                continue
            for gi, geom in enumerate(R.ROWS16_GEOMETRIES):
                lib.ll_set_rows16_geometry(*geom)
                for epi in R.EPIS:
                    refused = geom[0] != 0 and R.rows16_lds_bytes(geom[0], geom[1], epi) > R.LDS_LIMIT
                    for form in R.forms(name):
                        for use_bias in (False, True):
                            # the launcher's own geometry with every M; the others with two, shifted so that every (epilogue, norm, bias)
                            # meets every M over the geometries
                            at = turn + gi + 5 * ni
                            for M in (R.ROWS16_M if gi == 0 else (R.ROWS16_M[at % 6], R.ROWS16_M[(at + 3) % 6])):
                                rc, out = _rows16(lib, d, M, n, epi, form, use_bias)
                                tag = f"{name} M={M} N={n} geometry={geom} epi={epi} {form} bias={use_bias}"
                                if refused:
                                    assert rc == LL_EINVAL and R.sentinel_damage(out, 0, 0) == 0, (tag, rc)
                                    continue
                                _ok(rc, tag)
                                path = "ll_linear_rows16_bf16 " + ("RMSNorm prologue" if form == R.STAGED else "no norm")
                                verify(path, tag, d, out, M, n, form, use_bias, epi)
                            turn += 1
    finally:
        lib.ll_set_rows16_geometry(0, 0, 0)


@pytest.mark.parametrize("name", sorted(n for n in R.ROWS16_SETS if "eps" not in n))
def test_linear_rows16_column_probes(lib, name):
    d = dev(name)
    M, n = 16, 17
    wb, ldw, _ = d.wbuf(n, R.PLAIN)

    def call(xb, ldx, out, ldc):
        _ok(lib.ll_linear_rows16_bf16(xb.data_ptr(), ldx, wb.data_ptr(), ldw, None, None, d.eps, None, 0, out.data_ptr(), ldc, M, n, d.K, R.PLAIN,
                                      _stream()), "ll_linear_rows16_bf16")
    probes = probe_set(d.w, d.K, M, n)
    try:
        for geom in R.ROWS16_GEOMETRIES:
            lib.ll_set_rows16_geometry(*geom)
            run_probes(call, probes, d.K, M, n, f"{name} geometry={geom}")
    finally:
        lib.ll_set_rows16_geometry(0, 0, 0)


def test_the_check_sees_a_wrong_result_on_the_device(lib):
    """the device side of the check is not vacuous: a correct output held against the intervals of another call (bias on / off, one row
    further down, one column further right) leaves them, and a store one column past N breaks the sentinel"""
    d = dev("rows16-K160")
    M, n = 5, 17
    rc, out = _rows16(lib, d, M, n, R.PLAIN, R.NONE, True)
    _ok(rc, "ll_linear_rows16_bf16")
    got = out[:M, :n]
    assert R.check(got, *d.bounds(R.NONE, True, R.PLAIN, M, n))[0] == 0 and R.sentinel_damage(out, M, n) == 0
    assert R.check(got, *d.bounds(R.NONE, False, R.PLAIN, M, n))[0] > 0.9 * M * n
    assert R.check(got, *(t[1:] for t in d.bounds(R.NONE, True, R.PLAIN, M + 1, n)))[0] > 0.9 * M * n
    assert R.check(got, *(t[:, 1:] for t in d.bounds(R.NONE, True, R.PLAIN, M, n + 1)))[0] > 0.9 * M * n
    assert R.check(torch.full_like(got, R.NAN), *d.bounds(R.NONE, True, R.PLAIN, M, n))[0] == M * n
    assert R.sentinel_damage(out, M, n - 1) == M and R.sentinel_damage(out, M - 1, n) == n


# ------------------------------------------------------------------------------------------------------------------ ll_linear_rows64_bf16
def _pack(lib, d, n, epi):
    wb, ldw, bb = d.wbuf(n, epi)
    rows = 2 * n if epi == R.SILU_MUL else n
    elems = int(lib.ll_rows64_packed_elems(rows, d.K))
    assert elems == (rows + 15) // 16 * 16 * d.K
    packed = torch.full((elems + 64,), R.SENTINEL, dtype=torch.int16, device="cuda").view(R.BF)
    _ok(lib.ll_rows64_pack_bf16(wb.data_ptr(), ldw, rows, d.K, packed.data_ptr(), _stream()), "ll_rows64_pack_bf16")
    assert bool((_bits(packed[elems:]) == R.SENTINEL).all()) and bool(torch.isfinite(packed[:elems].float()).all())
    return packed, bb


def _prenorm(lib, d, M, staged_ref):
    """ll_rows64_prenorm_bf16 on the raw rows: scaled rows (the x of a consumer call, ldx = K + 8) and their per-chunk sums of squares"""
    xe, ssq_ref = staged_ref
    xb, ldx = d.xbuf(M)
    kch = int(lib.ll_rows64_ssq_chunks(d.K))
    assert kch == (d.K + 1023) // 1024
    xs = R.out_buffer(M, d.K, d.K + 8, "cuda")
    ssq = torch.full((M + 1, kch), R.SENTINEL_F32, device="cuda")
    _ok(lib.ll_rows64_prenorm_bf16(xb.data_ptr(), ldx, d.norm_w.data_ptr(), xs.data_ptr(), d.K + 8, ssq.data_ptr(), M, d.K, _stream()),
        "ll_rows64_prenorm_bf16")
    assert R.sentinel_damage(xs, M, d.K) == 0 and R.sentinel_damage(ssq, M, kch) == 0
    assert torch.equal(_bits(xs[:M, :d.K]), _bits(xe[:M])), (d.name, M, "scaled rows are not bf16(x * norm_w)")
    rel = ((ssq[:M].double() - ssq_ref[:M]).abs() / ssq_ref[:M]).max()
    assert float(rel) <= 2.0 ** -14, (d.name, M, float(rel))
    return xs, ssq


def _rows64(lib, d, packed, bb, M, n, epi, use_bias, x, ldx, row_ssq, ws, norm, tag, ldc_extra=40):
    """one call; returns out, scaled_out, ssq_out (the latter two None without `norm`)"""
    rb, ldr = d.resbuf(M, n) if epi == R.RESIDUAL else (None, 0)
    out = R.out_buffer(M, n, n + ldc_extra, "cuda")
    nch = int(lib.ll_rows64_ssq_chunks(n))
    xs = R.out_buffer(M, n, n + 24, "cuda") if norm else None
    ssq = torch.full((M + 1, nch), R.SENTINEL_F32, device="cuda") if norm else None
    kch = int(lib.ll_rows64_ssq_chunks(d.K))
    wsb = int(lib.ll_linear_rows64_workspace_bytes(M, n))
    assert ws is None or ws.numel() * 4 >= wsb
    _ok(lib.ll_linear_rows64_bf16(x.data_ptr(), ldx, packed.data_ptr(), _ptr(bb) if use_bias else None, _ptr(rb), ldr, out.data_ptr(), n + ldc_extra,
                                  M, n, d.K, epi, _ptr(row_ssq), kch if row_ssq is not None else 0, d.eps, _ptr(d.next_norm_w) if norm else None,
                                  _ptr(xs), n + 24, _ptr(ssq), _ptr(ws), wsb if ws is not None else 0, _stream()), tag)
    return out, xs, ssq


def _verify_next_norm(d, tag, out, xs, ssq, M, n):
    """the producer half of the next RMSNorm, from the kernel's own rounded output row"""
    nch = ssq.shape[1]
    assert R.sentinel_damage(xs, M, n) == 0 and R.sentinel_damage(ssq, M, nch) == 0, tag
    o = out[:M, :n]
    assert torch.equal(_bits(xs[:M, :n]), _bits((o.float() * d.next_norm_w[:n].float()).to(R.BF))), (tag, "scaled_out is not bf16(out * w)")
    sq = torch.zeros(M, nch * 1024, dtype=torch.float64, device="cuda")
    sq[:, :n] = o.double() ** 2
    want = sq.view(M, nch, 1024).sum(-1)
    rel = ((ssq[:M].double() - want).abs() / want.clamp_min(1e-300)).max()
    assert float(rel) <= 2.0 ** -14, (tag, "ssq_out", float(rel))


@pytest.mark.parametrize("name", sorted(R.ROWS64_SETS))
def test_linear_rows64(lib, name):
    """M 1..64 (both row-block instances), every N, every K split with the workspace and the single launch without; the consumer side of a
    split RMSNorm (x and row_ssq from ll_rows64_prenorm_bf16) in the main kernel and in the slab sum; the producer side (scaled_out,
    ssq_out); two runs bit-identical"""
    d = dev(name)
    o = d.o
    xe, r, _ = R.effective_input(o.x, o.norm_w, o.eps, R.STAGED)
    kch = (o.K + 1023) // 1024
    sq = torch.zeros(o.M, kch * 1024, dtype=torch.float64)
    sq[:, :o.K] = o.x.double() ** 2
    staged_ref = (xe.to(R.BF).cuda(), sq.view(o.M, kch, 1024).sum(-1).cuda())
    ws = torch.empty(8 * 64 * o.N, dtype=torch.float32, device="cuda")
    pre = {M: _prenorm(lib, d, M, staged_ref) for M in R.ROWS64_M}
    try:
        for n in R.ROWS64_N:
            if n > o.N:
                continue
            packed, bb = _pack(lib, d, n, R.PLAIN)
            gated = _pack(lib, d, n, R.SILU_MUL) if n % 16 == 0 else None
            for M in R.ROWS64_M:
                xb, ldx = d.xbuf(M)
                xs_in, ssq_in = pre[M]
                raw, scaled = (xb, ldx, None), (xs_in, o.K + 8, ssq_in)
                for ksg in R.ROWS64_KSPLIT:
                    lib.ll_set_rows64_ksplit(ksg)
                    base = f"{name} M={M} N={n} ksplit={ksg}"
                    # (epilogue, bias, input, workspace, next norm, path)
                    plan = [(R.PLAIN, True, raw, True, False, "K split + slab sum"), (R.RESIDUAL, True, raw, True, True, "slab sum with the next norm"),
                            (R.RESIDUAL, False, scaled, True, False, "row scale in the slab sum")]
                    if ksg in (0, 8):
                        plan += [(R.PLAIN, False, raw, False, False, "one launch"), (R.PLAIN, True, scaled, False, False, "one launch, row scale")]
                    if ksg in (0, 4):
                        plan += [(R.PLAIN, False, scaled, True, True, "slab sum with the next norm")]
                    if ksg == 0 and gated is not None:
                        plan += [(R.SILU_MUL, True, raw, True, False, "SiLU*mul"), (R.SILU_MUL, False, scaled, False, False, "SiLU*mul, row scale")]
                    for epi, use_bias, (x, ld, row_ssq), use_ws, norm, path in plan:
                        tag = f"{base} epi={epi} bias={use_bias} row_ssq={row_ssq is not None} ws={use_ws} next_norm={norm}"
                        pk, bias = gated if epi == R.SILU_MUL else (packed, bb)
                        form = R.STAGED if row_ssq is not None else R.NONE
                        out, xs, ssq = _rows64(lib, d, pk, bias, M, n, epi, use_bias, x, ld, row_ssq, ws if use_ws else None, norm, tag)
                        verify("ll_linear_rows64_bf16 " + path, tag, d, out, M, n, form, use_bias, epi)
                        if norm:
                            _verify_next_norm(d, tag, out, xs, ssq, M, n)
                            again, xs2, ssq2 = _rows64(lib, d, pk, bias, M, n, epi, use_bias, x, ld, row_ssq, ws, norm, tag)
                            assert torch.equal(_bits(again), _bits(out)) and torch.equal(_bits(xs2), _bits(xs)) and torch.equal(ssq2, ssq), (tag, "two runs differ")
    finally:
        lib.ll_set_rows64_ksplit(0)


@pytest.mark.parametrize("name", sorted(n for n in R.ROWS64_SETS if "eps" not in n))
def test_linear_rows64_column_probes(lib, name):
    d = dev(name)
    M, n = 64, 65
    packed, _ = _pack(lib, d, n, R.PLAIN)
    ws = torch.empty(8 * M * n, dtype=torch.float32, device="cuda")
    probes = probe_set(d.w, d.K, M, n)
    try:
        for ksg, use_ws in ((0, True), (0, False), (1, True), (2, True), (4, True), (8, True)):
            lib.ll_set_rows64_ksplit(ksg)

            def call(xb, ldx, out, ldc):
                _ok(lib.ll_linear_rows64_bf16(xb.data_ptr(), ldx, packed.data_ptr(), None, None, 0, out.data_ptr(), ldc, M, n, d.K, R.PLAIN, None, 0, d.eps,
                                              None, None, 0, None, _ptr(ws) if use_ws else None, ws.numel() * 4 if use_ws else 0, _stream()),
                    "ll_linear_rows64_bf16")
            run_probes(call, probes, d.K, M, n, f"{name} ksplit={ksg} ws={use_ws}")
    finally:
        lib.ll_set_rows64_ksplit(0)


# ------------------------------------------------------------------------------------------------------------------ the other entry points
def _plain_operands(d, M, n):
    xb, ldx = d.xbuf(M)
    wb, ldw, bb = d.wbuf(n, R.PLAIN)
    return xb, ldx, wb, ldw, bb, R.out_buffer(M, n, n + 40, "cuda")


@pytest.mark.parametrize("name,rows", [("linear-K2056", (1, 2, 3, 4)), ("linear-K2048", (5, 65, 128))])
def test_ll_linear_bf16_plain(lib, name, rows):
    """ll_linear(LL_BF16): the lm_head GEMV at 1..4 rows (K a multiple of 8 only), the MFMA tiles at 5, 65 and 128 rows; ragged N = 1003"""
    from llamole_amd import _lib
    d = dev(name)
    n = d.o.N
    for M in rows:
        for use_bias in (False, True):
            xb, ldx, wb, ldw, bb, out = _plain_operands(d, M, n)
            tag = f"{name} M={M} bias={use_bias}"
            _ok(lib.ll_linear(_lib.LL_BF16, xb.data_ptr(), ldx, wb.data_ptr(), ldw, _ptr(bb) if use_bias else None, out.data_ptr(), n + 40, M, n, d.K, 0, 0,
                              _stream()), tag)
            verify("ll_linear(LL_BF16) " + ("GEMV" if M <= 4 else "MFMA tiles"), tag, d, out, M, n, R.NONE, use_bias, R.PLAIN)


@pytest.mark.parametrize("M", [65, 128])
def test_ll_linear_splitk_bf16_plain(lib, M):
    """ll_linear_splitk_bf16 at the split the prefill path chooses for these shapes"""
    from llamole_amd.llm_accel import _prefill_splits
    d = dev("linear-K2048")
    n = d.o.N
    splits = _prefill_splits(M, n, d.K)
    assert splits == 2
    ws = torch.full((splits * M * n + 64,), R.SENTINEL_F32, device="cuda")
    for use_bias in (False, True):
        xb, ldx, wb, ldw, bb, out = _plain_operands(d, M, n)
        tag = f"splitk M={M} bias={use_bias}"
        _ok(lib.ll_linear_splitk_bf16(xb.data_ptr(), ldx, wb.data_ptr(), ldw, _ptr(bb) if use_bias else None, out.data_ptr(), n + 40, M, n, d.K, 0, splits,
                                      ws.data_ptr(), _stream()), tag)
        verify("ll_linear_splitk_bf16", tag, d, out, M, n, R.NONE, use_bias, R.PLAIN)
        assert bool((ws[splits * M * n:] == R.SENTINEL_F32).all()), (tag, "wrote behind the workspace")
