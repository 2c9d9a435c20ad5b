"""The tile GEMM family behind ll_linear (llamole_amd/csrc/gemm.hip) against the float64 reference and rounding intervals of
tests/gemm_reference.py, through the C ABI.

  * one row per branch of gemm_dispatch (DISPATCH_ROWS, derived from its conditions), each asserting ll_debug_last_gemm_path and run with
    all four epilogues, with and without bias, bf16 and f32 output, a vectorisable and an odd ldc; split-K rows through
    ll_linear_splitk_bf16 (every raw slab against its own K range, their sum, the bf16 result); the switches ll_set_m128_panel,
    ll_set_m64_waves and ll_set_gemm_krot on the rows they steer;
  * every entry of the tuning table, 0..67, through ll_linear_cfg at rows BM - 1, BM, 2 BM - 3, ragged N, k-tile counts below / at / above
    the ring depth, splits 1 and 2, and the calls an entry cannot honour refused with nothing written;
  * entry 59 (256 x 256, two stages) is included: the earlier test left it out without a reason, and reading it gives none -- it is the
    ring template at STAGES = 2, whose counted wait is then vmcnt(0) before every barrier (no tile in flight across it, as its comment
    says: slow, not wrong), 128 KB of LDS, 1024 threads with 64 accumulator registers each;
  * the two-group Linear (ll_linear_grouped2_probe) against the two Linears computed separately, the packed-weight panel kernels
    (ll_linear_packed_probe) bit for bit against the unpacked call, LL_F32 on random f32 operands, LL_GEMM_VARIANT=0 and 2 in child processes;
  * column probes A[m] = c e_k through every kernel family, with the k-tile rotation on: c W[:, k] bit for bit.

Every operand is a view with a loose row stride into an allocation whose other bytes are NaN (inputs; for LL_F32 the rows up to
round_up(M, 64) too) or a sentinel (outputs), and the sentinel must survive everywhere outside [M, N], behind the last slab included.

-s prints, per kernel family, the largest position inside the interval and the share of the GELU band the device used; the figures measured
on an MI355X are in the docstring of tests/gemm_reference.py."""
import contextlib
import os
import subprocess
import sys

import pytest
import torch

from tests import gemm_reference as G
from tests import linear_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST, COUNT, GELU_USE = {}, {}, {}
LL_F32, LL_BF16 = 0, 1

# ll_debug_last_gemm_path (include/llamole_hip_tuning.h)
(P_NONE, P_GEMV, P_M64, P_M128, P_ROWS16, P_RING32, P_W16_256, P_W16_128, P_RING64_2x2, P_RING128x64, P_PIPEU64, P_RING64_4x2, P_RING64x32,
 P_V0_128, P_V0_64, P_V0_64x32, P_V0_64x16, P_F32) = range(18)
P_PACKED = 1 << 24
PATH_NAMES = ["refused", "GEMV", "panel <= 64 rows", "panel 65..256 rows", "rows16", "ring 32x32x8", "16-wave 256x128", "16-wave 128x128",
              "ring 64x64 2x2", "ring 128x64", "unified 64x64 16 waves", "ring 64x64 4x2", "ring 64x32", "variant-0 128x128", "variant-0 64x64",
              "variant-0 64x32", "variant-0 64x16", "f32"]


def panel(branch, K_chunk, tiles):
    return branch | (K_chunk // 128) << 8 | tiles << 16


@pytest.fixture(scope="module")
def lib():
    from llamole_amd import _lib
    yield _lib.load()
    for path in sorted(WORST):
        print(f"\nlargest position inside the interval, {path}: {WORST[path]:.3f} ({COUNT[path]} calls)")
    for path in sorted(GELU_USE):
        print(f"\nlargest share of the GELU band used, {path}: {GELU_USE[path]:.3f}")


def _ok(rc, what):
    from llamole_amd import _lib
    _lib.check(rc, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def round_up(a, b):
    return (a + b - 1) // b * b


# ------------------------------------------------------------------------------------------------------------------ operands on the device
class Dev:
    """an operand set on the device: poisoned views per call shape, lin and e as float64"""

    def __init__(self, name):
        self.name, self.s = name, G.gemm_set(name)
        s = self.s
        self.K, self.N, self.f32 = s.K, s.N, s.f32
        self.x, self.w, self.bias = s.x.cuda(), s.w.cuda(), s.bias.cuda()
        self._lin, self._x, self._w, self._slabs = {}, {}, {}, {}

    def lin_e(self, use_bias, M, n, col0=0):
        key = bool(use_bias)
        if key not in self._lin:
            self._lin[key] = tuple(t.cuda() for t in self.s.linear(key))
        lin, e = self._lin[key]
        return lin[:M, col0:col0 + n], e[:M, col0:col0 + n]

    def slabs(self, splits, M, n, col0=0):
        if splits not in self._slabs:
            self._slabs = {splits: [(a.cuda(), b.cuda()) for a, b in self.s.slabs(splits)]}
        return [(a[:M, col0:col0 + n], b[:M, col0:col0 + n]) for a, b in self._slabs[splits]]

    def xbuf(self, M):
        """x[:M] with lda = K + 8, NaN behind every row and in the rows after the last (LL_F32: the round_up(M, 64) rows the contract wants
        readable are there, and NaN)"""
        if M not in self._x:
            if len(self._x) > 16:
                self._x.clear()
            self._x[M] = R.padded(self.x[:M], self.K + 8, rows_after=(round_up(M, 64) - M + 1) if self.f32 else 1)[0]
        return self._x[M], self.K + 8

    def wbuf(self, n, col0=0, dense=False):
        """(w[col0:col0 + n] with ldw = K + 40 (dense: K) and two NaN rows behind the last, ldw, bias + NaN)"""
        key = (n, col0, dense)
        if key not in self._w:
            if len(self._w) > 16:
                self._w.clear()
            ldw = self.K if dense else self.K + 40
            self._w[key] = (R.padded(self.w[col0:col0 + n], ldw, rows_after=2)[0], ldw, R.padded_vec(self.bias[col0:col0 + n]))
        return self._w[key]


_DEV = {}


def dev(name):
    if name not in _DEV:
        if len(_DEV) >= 2:
            _DEV.pop(next(iter(_DEV)))
        _DEV[name] = Dev(name)
    return _DEV[name]


def out_buf(rows, n, ldc, out_f32):
    """[rows + 1, ldc] holding the sentinel everywhere (split-K: rows = splits * M, the slabs one behind the other)"""
    if out_f32:
        return torch.full((rows + 1, ldc), R.SENTINEL_F32, dtype=torch.float32, device="cuda")
    return R.out_buffer(rows, n, ldc, "cuda")


def record(path, pos):
    WORST[path] = max(WORST.get(path, 0.0), pos)
    COUNT[path] = COUNT.get(path, 0) + 1


def verify(path, tag, out, M, n, lin, e, epi, out_f32):
    assert R.sentinel_damage(out, M, n) == 0, (path, tag, "wrote outside [M, N]")
    outside, pos = R.check(out[:M, :n], *G.interval(lin, e, epi, out_f32))
    record(path, pos)
    assert outside == 0, (path, tag, f"{outside} elements outside their interval, largest position {pos}")


def verify_slabs(path, tag, d, buf, M, n, splits, refs=None, whole=None):
    """buf [splits * M + 1, ldc] f32: every raw slab against its own K range, their float64 sum against the whole (refs, whole: the per-slab
    and whole (lin, e) where they are not the set's first weight matrix)"""
    assert R.sentinel_damage(buf, splits * M, n) == 0, (path, tag, "wrote outside the slabs")
    total = torch.zeros(M, n, dtype=torch.float64, device="cuda")
    for z, (lin_z, e_z) in enumerate(refs or d.slabs(splits, M, n)):
        slab = buf[z * M:(z + 1) * M, :n]
        outside, pos = R.check(slab, *G.interval(lin_z, e_z, G.NONE, 1))
        record(path + " raw slabs", pos)
        assert outside == 0, (path, tag, f"slab {z}: {outside} elements outside their interval, largest position {pos}")
        total += slab.double()
    outside, pos = G.check_sum(total, *(whole or d.lin_e(False, M, n)))
    assert outside == 0, (path, tag, f"slab sum: {outside} elements outside lin +- e, largest position {pos}")


@contextlib.contextmanager
def switches(lib, panel=None, waves=None, krot=None, packed=None):
    old = {}
    try:
        if panel is not None:
            old["panel"] = lib.ll_set_m128_panel(panel)
        if waves is not None:
            old["waves"] = lib.ll_set_m64_waves(waves)
        if krot is not None:
            old["krot"] = lib.ll_set_gemm_krot(krot)
        if packed is not None:
            old["packed"] = lib.ll_set_m64_packed(packed)
        yield
    finally:
        if "panel" in old:
            lib.ll_set_m128_panel(old["panel"])
        if "waves" in old:
            lib.ll_set_m64_waves(old["waves"])
        if "krot" in old:
            lib.ll_set_gemm_krot(old["krot"])
        if "packed" in old:
            lib.ll_set_m64_packed(old["packed"])


def linear(lib, d, M, n, epi, use_bias, out_f32, ldc=None, tag=""):
    """one ll_linear call on poisoned operands; returns the output allocation"""
    xb, lda = d.xbuf(M)
    wb, ldw, bb = d.wbuf(n)
    ldc = ldc or n + 40
    out = out_buf(M, n, ldc, out_f32 or d.f32)
    _ok(lib.ll_linear(LL_F32 if d.f32 else LL_BF16, xb.data_ptr(), lda, wb.data_ptr(), ldw, _ptr(bb) if use_bias else None, out.data_ptr(), ldc,
                      M, n, d.K, epi, out_f32, _stream()), tag)
    return out


def epilogue_sweep(lib, d, path, tag, M, n, call, want_path=None, epis=G.EPIS):
    """call(epi, use_bias, out_f32, ldc) -> output allocation: all epilogues, with and without bias, bf16 and f32 output, ldc = n + 40 with
    bias (vector stores where the kernel has them) and n + 41 without; the GELU band's use from the f32 outputs with and without epilogue"""
    f32_out = d.f32
    for out_f32 in ((1,) if f32_out else (0, 1)):
        for use_bias in (False, True):
            lin, e = d.lin_e(use_bias, M, n)
            plain = None
            for epi in epis:
                t = f"{tag} epi={G.EPI_NAMES[epi]} bias={use_bias} out_f32={out_f32}"
                out = call(epi, use_bias, out_f32, n + 40 if use_bias else n + 41)
                if want_path is not None:
                    got = lib.ll_debug_last_gemm_path()
                    assert got == want_path(epi), (t, f"took path {got:#x}, the row was written for {want_path(epi):#x}")
                verify(path, t, out, M, n, lin, e, epi, out_f32)
                if out_f32 and epi == G.NONE:
                    plain = out[:M, :n]
                    # the band's use below takes this output as the pre-activation of the GELU launch: the sum must not vary between launches
                    again = call(epi, use_bias, out_f32, n + 40 if use_bias else n + 41)
                    assert torch.equal(_bits(again), _bits(out)), (t, "two launches of the same call differ")
                if out_f32 and epi == G.GELU and plain is not None:
                    GELU_USE[path] = max(GELU_USE.get(path, 0.0), G.gelu_band_use(out[:M, :n], plain))


def splitk_sweep(lib, d, path, tag, M, n, splits, want_path=None):
    """ll_linear_splitk_bf16: the workspace slab by slab, the bf16 result with epilogues none and SiLU, with and without bias"""
    xb, lda = d.xbuf(M)
    wb, ldw, bb = d.wbuf(n)
    for epi in (G.NONE, G.SILU):
        for use_bias in (False, True):
            t = f"{tag} splits={splits} epi={G.EPI_NAMES[epi]} bias={use_bias}"
            ws = torch.full((splits * M + 1, n), R.SENTINEL_F32, dtype=torch.float32, device="cuda")
            out = out_buf(M, n, n + 41, 0)
            _ok(lib.ll_linear_splitk_bf16(xb.data_ptr(), lda, wb.data_ptr(), ldw, _ptr(bb) if use_bias else None, out.data_ptr(), n + 41, M, n, d.K,
                                          epi, splits, ws.data_ptr(), _stream()), t)
            if want_path is not None:
                got = lib.ll_debug_last_gemm_path()
                assert got == want_path, (t, f"took path {got:#x}, the row was written for {want_path:#x}")
            verify_slabs(path, t, d, ws, M, n, splits)
            verify(path + " split-K result", t, out, M, n, *d.lin_e(use_bias, M, n), epi, 0)


# ------------------------------------------------------------------------------------------------------------------ the dispatch table
# (set, M, N, splits, path, path for an epilogue other than none (rows16 takes the plain epilogue only), switches).  Conditions of
# gemm_dispatch, in its order: GEMV M <= 4 (K % 8); panel M <= 64, K chunk in {256, 512, 768, 1024}, ceil(N / 16) splits >= 8; multi-panel
# 64 < M <= 224 (256 under ll_set_m128_panel(2)), K chunk in {256, 512, 1024}, ceil(N / 32) splits >= 24, two column tiles up to 128 rows and
# four beyond; rows16 4 < M <= 16, unsplit, plain, K % 32 == 0, N >= 256; ring 32x32 M <= 32; sixteen waves M >= 1024, K chunk >= 256,
# 256x128 from 2048 rows with >= 192 tiles, 128x128 with >= 192 tiles; then 64x64 on 2x2 waves for M <= 64 with >= 256 column tiles,
# 128x64 with >= 1024 tiles, unified 64x64 with >= 200 tiles above 64 rows, 64x64 on 4x2 waves with >= 200 tiles or N % 32 != 0 and
# N < 64, else 64x32.
DISPATCH_ROWS = []


def _row(name, M, N, path, splits=1, path_epi=None, **sw):
    DISPATCH_ROWS.append((name, M, N, splits, path, path if path_epi is None else path_epi, sw))


for _M in (1, 4):
    _row("gemm-K1032", _M, 1003, P_GEMV)
    _row("gemm-K64", _M, 7, P_GEMV)
_row("gemm-K4096", 2, 515, P_GEMV)
_row("gemm-K2056", 3, 1003, P_GEMV)
_row("gemm-K1024", 3, 128, P_GEMV)
for _K in (256, 512, 768, 1024):
    for _M in (5, 33, 63, 64):
        for _N in (128, 176, 1000):
            _row(f"gemm-K{_K}", _M, _N, panel(P_M64, _K, 1))
    _row(f"gemm-K{_K}", 33, 1000, panel(P_M64, _K, 1), waves=4)
    _row(f"gemm-K{_K}", 64, 113, panel(P_M64, _K, 1))                      # ceil(113 / 16) = 8: the fewest workgroups the branch takes
    _row(f"gemm-K{_K}", 64, 112, P_RING64x32)                               # 7: one short
_row("gemm-K2048", 40, 176, panel(P_M64, 1024, 1), splits=2)
_row("gemm-K2048", 64, 1000, panel(P_M64, 512, 1), splits=4)
_row("gemm-K4096", 5, 128, panel(P_M64, 256, 1), splits=16)
_row("gemm-K1536", 63, 1000, panel(P_M64, 768, 1), splits=2)
_row("gemm-K2048", 33, 1000, panel(P_M64, 512, 1), splits=4, waves=4)
for _K in (256, 512, 1024):
    for _N in (784, 1000):
        for _M in (65, 100, 128):
            _row(f"gemm-K{_K}", _M, _N, panel(P_M128, _K, 2))
        for _M in (129, 224):
            _row(f"gemm-K{_K}", _M, _N, panel(P_M128, _K, 4))
    _row(f"gemm-K{_K}", 256, 1000, panel(P_M128, _K, 4), panel=2)
    _row(f"gemm-K{_K}", 256, 1000, P_RING64x32)                             # 225..256 rows are opt-in
    _row(f"gemm-K{_K}", 225, 1000, P_RING64x32)
    _row(f"gemm-K{_K}", 100, 1000, P_RING64x32, panel=0)
    _row(f"gemm-K{_K}", 100, 737, panel(P_M128, _K, 2))                     # ceil(737 / 32) = 24
    _row(f"gemm-K{_K}", 100, 736, P_RING64x32)                              # 23
_row("gemm-K768", 100, 1000, P_RING64x32)                                   # K chunk 768 is a <= 64-row form only
_row("gemm-K2048", 100, 1000, panel(P_M128, 1024, 2), splits=2)
_row("gemm-K2048", 224, 400, panel(P_M128, 512, 4), splits=4)
_row("gemm-K4096", 65, 176, panel(P_M128, 256, 2), splits=16)
for _K in (64, 448):
    for _M in (5, 16):
        for _N in (256, 1003):
            _row(f"gemm-K{_K}", _M, _N, P_ROWS16, path_epi=P_RING32)
    _row(f"gemm-K{_K}", 5, 255, P_RING32)
for _M in (17, 32):
    for _K in (64, 128, 448):            # 1, 2 and 7 k-tiles: below and at STAGES - 1 = 7
        for _N in (100, 1003):
            _row(f"gemm-K{_K}", _M, _N, P_RING32)
    _row("gemm-K512", _M, 100, P_RING32)  # 8 k-tiles: one above
for _krot in (1, 3, 0x0201, 1000):
    _row("gemm-K448", 32, 1003, P_RING32, krot=_krot)
    _row("gemm-K448", 100, 1003, P_RING64x32, krot=_krot)
_row("gemm-K2048", 17, 1003, P_RING32, splits=16)
_row("gemm-K128", 32, 100, P_RING32, splits=2)
_row("gemm-K1536", 32, 1003, P_RING32, splits=4, krot=3)
_row("big-K256", 2048, 2945, P_W16_256)
_row("big-K256", 2048, 2945, P_W16_256, krot=0x0201)
_row("big-K256", 1024, 2945, P_W16_128)
_row("big-K256", 2047, 2945, P_W16_128, krot=3)
_row("big-K256", 2048, 2944, P_W16_128)                                     # 8 x 23 = 184 tiles of 256 x 128: one column tile short
_row("wide-K128", 64, 16330, P_RING64_2x2)
_row("wide-K128", 33, 16321, P_RING64_2x2, krot=1)
_row("gemm-K2048", 40, 1003, P_RING64_2x2, splits=16)
_row("big-K256", 2048, 2945, P_RING128x64, splits=2)
_row("tall-K128", 2048, 4040, P_RING128x64)                                 # 16 x 64 = 1024 tiles of 128 x 64, K chunk below 256
_row("tall-K128", 1921, 4033, P_RING128x64, krot=3)
_row("tall-K128", 2048, 4032, P_PIPEU64)                                    # 16 x 63 = 1008: one column tile short
_row("big-K256", 300, 2945, P_PIPEU64)
_row("big-K256", 257, 2945, P_PIPEU64)
_row("gemm-K2048", 260, 1003, P_PIPEU64, splits=4)
_row("gemm-K2048", 65, 1000, P_PIPEU64, splits=16)
_row("wide-K128", 50, 13000, P_RING64_4x2)
_row("wide-K128", 64, 16320, P_RING64_4x2)                                  # 255 column tiles
_row("gemm-K128", 100, 40, P_RING64_4x2)
_row("gemm-K64", 64, 33, P_RING64_4x2, krot=3)
_row("gemm-K128", 100, 1003, P_RING64x32)
_row("gemm-K448", 260, 176, P_RING64x32)
_row("gemm-K512", 64, 100, P_RING64x32)
_row("gemm-K128", 33, 64, P_RING64x32)
_row("gemm-K2048", 100, 176, P_RING64x32, splits=2)


def _row_id(r):
    name, M, N, splits, path, _, sw = r
    return f"{name}-M{M}-N{N}" + (f"-s{splits}" if splits > 1 else "") + f"-{PATH_NAMES[path & 255].replace(' ', '_')}" + \
        "".join(f"-{k}{v}" for k, v in sorted(sw.items()))


DISPATCH_ROWS.sort(key=lambda r: r[0])       # one operand set after the other


@pytest.mark.parametrize("row", DISPATCH_ROWS, ids=_row_id)
def test_dispatch_row(lib, row):
    name, M, N, splits, path, path_epi, sw = row
    d = dev(name)
    label = "ll_linear " + PATH_NAMES[path & 255]
    tag = _row_id(row)
    with switches(lib, **sw):
        if splits == 1:
            if path_epi != path:        # rows16: the plain epilogue there, the others on the ring
                epilogue_sweep(lib, d, label, tag, M, N, lambda epi, b, f, ldc: linear(lib, d, M, N, epi, b, f, ldc, tag), lambda epi: path, (G.NONE,))
                epilogue_sweep(lib, d, "ll_linear " + PATH_NAMES[path_epi & 255], tag, M, N,
                               lambda epi, b, f, ldc: linear(lib, d, M, N, epi, b, f, ldc, tag), lambda epi: path_epi, (G.GELU, G.SILU, G.SOFTSIGN))
            else:
                epilogue_sweep(lib, d, label, tag, M, N, lambda epi, b, f, ldc: linear(lib, d, M, N, epi, b, f, ldc, tag), lambda epi: path)
        else:
            splitk_sweep(lib, d, label, tag, M, N, splits, path)


def test_dispatch_refusals(lib):
    """what no kernel can honour is refused with nothing written: K per split off the 64-wide k-tile above four rows, lda off 8"""
    d = dev("gemm-K1032")
    for M, splits, lda_off in ((5, 1, 0), (100, 1, 0), (4, 3, 0), (4, 1, 4)):
        xb, lda = d.xbuf(M)
        wb, ldw, bb = d.wbuf(100)
        out = out_buf(splits * M, 100, 140, 1)
        if splits == 1:
            rc = lib.ll_linear(LL_BF16, xb.data_ptr(), lda + lda_off, wb.data_ptr(), ldw, None, out.data_ptr(), 140, M, 100, d.K, 0, 1, _stream())
        else:
            o2 = out_buf(M, 100, 140, 0)
            rc = lib.ll_linear_splitk_bf16(xb.data_ptr(), lda, wb.data_ptr(), ldw, None, o2.data_ptr(), 140, M, 100, d.K, 0, splits, out.data_ptr(),
                                           _stream())
        assert rc == -1 and lib.ll_debug_last_gemm_path() == P_NONE, (M, splits, lda_off, rc)
        assert R.sentinel_damage(out, 0, 0) == 0


# ------------------------------------------------------------------------------------------------------------------ LL_F32
@pytest.mark.parametrize("name", ["f32-K16", "f32-K48", "f32-K1024", "f32-gelu-K16"])
def test_linear_f32(lib, name):
    """LL_F32 on random f32 operands: one k-ordered fmaf chain per output, e = (K + 1) 2^-24 absref; A is allocated for round_up(M, 64)
    rows and the rows behind M are NaN (readable, not zero)"""
    d = dev(name)
    for M in (1, 63, 64, 65):
        for N in (1, 63, 64, 65, 176):
            tag = f"{name} M={M} N={N}"
            epilogue_sweep(lib, d, "ll_linear(LL_F32)", tag, M, N, lambda epi, b, f, ldc: linear(lib, d, M, N, epi, b, f, ldc, tag), lambda epi: P_F32)


def test_linear_f32_column_probes(lib):
    d = dev("f32-K1024")
    M, n, K = 65, 176, d.K
    wb, ldw, _ = d.wbuf(n)
    wrong = torch.zeros((), dtype=torch.long, device="cuda")
    launches = R.probe_launches(K, M)
    for ks, cs in launches:
        x = torch.zeros(M, K, device="cuda")
        x[torch.arange(M, device="cuda"), torch.tensor(ks, device="cuda")] = torch.tensor(cs, device="cuda")
        xb = R.padded(x, K + 8, rows_after=round_up(M, 64) - M + 1)[0]
        out = out_buf(M, n, n + 41, 1)
        _ok(lib.ll_linear(LL_F32, xb.data_ptr(), K + 8, wb.data_ptr(), ldw, None, out.data_ptr(), n + 41, M, n, K, 0, 1, _stream()), "f32 probe")
        want = out_buf(M, n, n + 41, 1)
        want[:M, :n] = (d.w[:n, torch.tensor(ks, device="cuda")] * torch.tensor(cs, device="cuda")).t()
        wrong += (_bits(out) != _bits(want)).sum()
    assert int(wrong) == 0, f"{int(wrong)} elements differ from c W[:, k] over {len(launches)} probe launches"


# ------------------------------------------------------------------------------------------------------------------ column probes, bf16
def probe_set(d, M, n, rows, out_f32):
    """[(x allocation [rows, K] with lda = K + 8: M probe rows, zero rows behind them, expected output allocation with ldc = n + 40)]"""
    out = []
    for ks, cs in G.probe_launches(d.K, M):
        x = torch.zeros(rows, d.K, dtype=R.BF, device="cuda")
        x[:len(ks)] = R.probe_x(d.K, ks, cs, "cuda")
        want = out_buf(rows, n, n + 40, out_f32)
        want[:rows, :n] = 0
        exp = R.probe_expected(d.w[:n], ks, cs)
        want[:len(ks), :n] = exp.float() if out_f32 else exp
        out.append((R.padded(x, d.K + 8)[0], want))
    return out


def run_probes(call, probes, rows, n, out_f32, what):
    wrong = torch.zeros((), dtype=torch.long, device="cuda")
    for xb, want in probes:
        out = out_buf(rows, n, n + 40, out_f32)
        call(xb, out)
        wrong += (_bits(out) != _bits(want)).sum()
    assert int(wrong) == 0, (what, f"{int(wrong)} elements differ from c W[:, k] over {len(probes)} probe launches")


# (label, set, probe rows per launch, rows of the launch, N, expected path, switches): every k of every set (K <= 1088), 4096 sparsely
PROBE_ROWS = [
    ("GEMV", "gemm-K1032", 4, 4, 1003, P_GEMV, {}),
    ("GEMV K4096", "gemm-K4096", 4, 4, 9, P_GEMV, {}),
    ("panel 1024", "gemm-K1024", 64, 64, 1000, panel(P_M64, 1024, 1), {}),
    ("panel 768", "gemm-K768", 63, 63, 176, panel(P_M64, 768, 1), {}),
    ("panel 512 on four waves", "gemm-K512", 64, 64, 1000, panel(P_M64, 512, 1), {"waves": 4}),
    ("panel 256", "gemm-K256", 64, 64, 128, panel(P_M64, 256, 1), {}),
    ("two-tile panels", "gemm-K1024", 128, 128, 1000, panel(P_M128, 1024, 2), {}),
    ("four-tile panels", "gemm-K512", 224, 224, 1000, panel(P_M128, 512, 4), {}),
    ("four-tile panels 256 rows", "gemm-K256", 256, 256, 784, panel(P_M128, 256, 4), {"panel": 2}),
    ("rows16", "gemm-K448", 16, 16, 1003, P_ROWS16, {}),
    ("ring 32x32", "gemm-K448", 32, 32, 1003, P_RING32, {}),
    ("ring 32x32 rotated", "gemm-K448", 32, 32, 1003, P_RING32, {"krot": 3}),
    ("ring 32x32 K512 rotated", "gemm-K512", 32, 32, 100, P_RING32, {"krot": 0x0201}),
    ("ring 64x32", "gemm-K448", 100, 100, 1003, P_RING64x32, {}),
    ("ring 64x32 rotated", "gemm-K448", 256, 256, 1003, P_RING64x32, {"krot": 1}),
    ("ring 64x64 4x2 rotated", "gemm-K128", 100, 100, 40, P_RING64_4x2, {"krot": 3}),
    ("ring 64x64 2x2 rotated", "wide-K128", 64, 64, 16330, P_RING64_2x2, {"krot": 1000}),
    ("unified 64x64", "big-K256", 256, 300, 2945, P_PIPEU64, {}),
    ("16-wave 128x128 rotated", "big-K256", 256, 1024, 2945, P_W16_128, {"krot": 3}),
    ("16-wave 256x128 rotated", "big-K256", 256, 2048, 2945, P_W16_256, {"krot": 1}),
    ("ring 128x64 rotated", "tall-K128", 256, 2048, 4040, P_RING128x64, {"krot": 1}),
]


@pytest.mark.parametrize("probe", PROBE_ROWS, ids=[p[0].replace(" ", "_") for p in PROBE_ROWS])
def test_dispatch_column_probes(lib, probe):
    """A[m] = c e_k, no bias, no epilogue: the output is c W[:, k] bit for bit in bf16 and in f32 (a lost product gives 0, a doubled one
    2 w); rows of the launch behind the probe rows are zero and must give +0"""
    label, name, M, rows, n, path, sw = probe
    d = dev(name)
    wb, ldw, _ = d.wbuf(n)
    with switches(lib, **sw):
        for out_f32 in (0, 1):
            def call(xb, out):
                _ok(lib.ll_linear(LL_BF16, xb.data_ptr(), d.K + 8, wb.data_ptr(), ldw, None, out.data_ptr(), n + 40, rows, n, d.K, 0, out_f32, _stream()), label)
                assert lib.ll_debug_last_gemm_path() == path, (label, hex(lib.ll_debug_last_gemm_path()))
            run_probes(call, probe_set(d, M, n, rows, out_f32), rows, n, out_f32, f"{label} out_f32={out_f32}")


# ------------------------------------------------------------------------------------------------------------------ the tuning table
def cfg_call(lib, cfg, d, M, n, splits, epi, use_bias, out_f32, xb=None):
    xb, lda = (xb, d.K + 8) if xb is not None else d.xbuf(M)
    wb, ldw, bb = d.wbuf(n)
    ldc = n + 40 if use_bias else n + 41
    out = out_buf(splits * M, n, ldc, out_f32 or splits > 1)
    rc = lib.ll_linear_cfg(cfg, xb.data_ptr(), lda, wb.data_ptr(), ldw, _ptr(bb) if use_bias else None, out.data_ptr(), ldc, M, n, d.K, splits, epi,
                           out_f32, _stream())
    return rc, out


@pytest.mark.parametrize("cfg", sorted(G.CFGS))
def test_tuning_table_entry(lib, cfg):
    """every entry of g_pipe_cfgs: GELU with bias in bf16 and f32, the plain epilogue without bias, raw slabs at splits = 2"""
    fam, bm, bn, st = G.CFGS[cfg]
    label = f"ll_linear_cfg {fam}"
    for name, M, n, K, splits in sorted(G.cfg_cases(cfg)):
        d = dev(name)
        assert d.K == K
        tag = f"cfg={cfg} {name} M={M} N={n} splits={splits}"
        if splits > 1:
            rc, out = cfg_call(lib, cfg, d, M, n, splits, G.GELU, True, 0)
            _ok(rc, tag)
            verify_slabs(label, tag, d, out, M, n, splits)
            continue
        for out_f32 in (0, 1):
            for epi, use_bias in ((G.GELU, True), (G.NONE, False)):
                rc, out = cfg_call(lib, cfg, d, M, n, 1, epi, use_bias, out_f32)
                _ok(rc, tag)
                verify(label, f"{tag} epi={epi} out_f32={out_f32}", out, M, n, *d.lin_e(use_bias, M, n), epi, out_f32)


@pytest.mark.parametrize("cfg", sorted(G.CFGS))
def test_tuning_table_refusals(lib, cfg):
    """ll_linear_cfg refuses what the launcher behind an entry cannot honour: -1, nothing written"""
    fam, bm, bn, st = G.CFGS[cfg]
    if fam == G.GEMV_CFG:
        bad = [("gemm-K1032", 4, 1), ("gemm-K1032", 2, 1), ("gemm-K1024", 1, 2)]
    elif fam == G.SKINNY:
        bad = [("cfg-K576", 63, 3), ("cfg-K2048", 64, 2), ("gemm-K1032", 5, 1)]
    elif fam == G.PANEL:
        bad = [(f"gemm-K{st * 128}", 65, 1), ("gemm-K768", 64, 1), (f"gemm-K{st * 128}", 64, 2)]
    elif fam == G.RS:
        bad = [("cfg-K192", 100, 1), ("cfg-K384", 100, 2), ("cfg-K128", 100, 2)]
    else:
        bad = [("gemm-K1032", 100, 1), ("cfg-K192", 100, 2), ("cfg-K64", 100, 2)]
    for name, M, splits in bad:
        d = dev(name)
        rc, out = cfg_call(lib, cfg, d, M, 100, splits, G.GELU, True, 1)
        assert rc == -1, (cfg, name, M, splits, rc)
        assert R.sentinel_damage(out, 0, 0) == 0, (cfg, name, M, splits, "a refused call wrote")
    d = dev("cfg-K128")
    xb, lda = d.xbuf(1)
    wb, ldw, _ = d.wbuf(100)
    out = out_buf(1, 100, 140, 1)
    assert lib.ll_linear_cfg(cfg, xb.data_ptr(), lda + 4, wb.data_ptr(), ldw, None, out.data_ptr(), 140, 1, 100, d.K, 1, 0, 1, _stream()) == -1
    assert lib.ll_linear_cfg(68, xb.data_ptr(), lda, wb.data_ptr(), ldw, None, out.data_ptr(), 140, 1, 100, d.K, 1, 0, 1, _stream()) == -1
    assert R.sentinel_damage(out, 0, 0) == 0


# one entry per kernel template the dispatch does not reach (or reaches in one form only), every k, the ring rotated
CFG_PROBES = [(17, "cfg-K320", 255), (12, "cfg-K576", 125), (15, "cfg-K576", 64), (41, "cfg-K512", 256), (47, "cfg-K384", 256), (48, "cfg-K448", 256), (52, "cfg-K448", 125),
              (55, "cfg-K320", 100), (59, "cfg-K192", 256), (10, "cfg-K192", 100), (39, "cfg-K448", 61), (64, "cfg-K448", 125), (66, "cfg-K320", 100),
              (58, "cfg-K256", 255), (9, "cfg-K256", 256), (26, "gemm-K64", 1), (30, "gemm-K64", 1)]


@pytest.mark.parametrize("cfg,name,M", CFG_PROBES)
def test_tuning_table_column_probes(lib, cfg, name, M):
    d = dev(name)
    n = 300
    wb, ldw, _ = d.wbuf(n)
    with switches(lib, krot=3 if G.CFGS[cfg][0] == G.RING else None):
        for out_f32 in (0, 1):
            def call(xb, out):
                _ok(lib.ll_linear_cfg(cfg, xb.data_ptr(), d.K + 8, wb.data_ptr(), ldw, None, out.data_ptr(), n + 40, M, n, d.K, 1, 0, out_f32, _stream()),
                    f"cfg {cfg}")
            run_probes(call, probe_set(d, M, n, M, out_f32), M, n, out_f32, f"cfg={cfg} out_f32={out_f32}")


# ------------------------------------------------------------------------------------------------------------------ two row groups
def grouped_call(lib, d, M, m_split, n, splits, epi, use_bias, out_f32, second=True):
    xb, lda = d.xbuf(M)
    w1, ldw, b1 = d.wbuf(n)
    w2, _, b2 = d.wbuf(n, col0=d.N)
    f32 = out_f32 or d.f32 or splits > 1
    ldc = n + 40 if use_bias else n + 41
    out = out_buf(splits * M, n, ldc, f32)
    rc = lib.ll_linear_grouped2_probe(LL_F32 if d.f32 else LL_BF16, xb.data_ptr(), lda, w1.data_ptr(), w2.data_ptr() if second else None, ldw,
                                      _ptr(b1) if use_bias else None, _ptr(b2) if use_bias else None, out.data_ptr(), ldc, M, m_split, n, d.K, splits,
                                      epi, out_f32, _stream())
    return rc, out


def grouped_slab_refs(d, splits, M, m_split, n):
    """per-slab (lin_z, e_z) of the two-group Linear: rows below m_split from the first weight's K range z, the others from the second's"""
    first = d.slabs(splits, M, n)
    if M <= m_split:
        return first
    second = d.slabs(splits, M, n, col0=d.N)
    return [(torch.cat((a1[:m_split], a2[m_split:])), torch.cat((b1[:m_split], b2[m_split:]))) for (a1, b1), (a2, b2) in zip(first, second)]


def grouped_reference(d, use_bias, M, m_split, n, second=True):
    """rows below m_split from (W1, bias1), the others from (W2, bias2): the two Linears computed separately"""
    lin1, e1 = d.lin_e(use_bias, M, n)
    if not second or M <= m_split:
        return lin1, e1
    lin2, e2 = d.lin_e(use_bias, M, n, col0=d.N)
    return torch.cat((lin1[:m_split], lin2[m_split:])), torch.cat((e1[:m_split], e2[m_split:]))


@pytest.mark.parametrize("name", ["gemm-K512", "gemm-K1024", "f32-K1024"])
@pytest.mark.parametrize("m_split", [64, 128])
def test_grouped2(lib, name, m_split):
    """ll_linear_grouped2_probe against the two Linears computed separately: M on both sides of m_split, every epilogue, both biases, raw
    slabs at splits 2 and 4, W2 = NULL (test_grouped2_wide has the launches of more than 256 workgroups)"""
    d = dev(name)
    for M in (m_split - 1, m_split, m_split + 1, m_split + 70):
        for n in ((176,) if d.f32 else (100, 1003)):
            wgs = -(-M // 64) * -(-n // 64)
            for splits in (1, 2, 4):
                tag = f"grouped {name} M={M} m_split={m_split} N={n} splits={splits} wgs={wgs * splits}"
                if splits > 1:
                    rc, out = grouped_call(lib, d, M, m_split, n, splits, G.GELU, True, 0)
                    _ok(rc, tag)
                    verify_slabs("ll_linear_grouped2 " + ("f32" if d.f32 else "bf16"), tag, d, out, M, n, splits,
                                 grouped_slab_refs(d, splits, M, m_split, n), grouped_reference(d, False, M, m_split, n))
                    continue
                for out_f32 in ((1,) if d.f32 else (0, 1)):
                    for use_bias in (False, True):
                        lin, e = grouped_reference(d, use_bias, M, m_split, n)
                        for epi in G.EPIS:
                            rc, out = grouped_call(lib, d, M, m_split, n, 1, epi, use_bias, out_f32)
                            _ok(rc, tag)
                            verify("ll_linear_grouped2 " + ("f32" if d.f32 else "bf16"), f"{tag} epi={epi} bias={use_bias} out_f32={out_f32}", out, M, n,
                                   lin, e, epi, out_f32)
    # W2 = NULL: one group over the first min(M, m_split) rows, through the dispatch
    M = m_split + 1
    rc, out = grouped_call(lib, d, M, m_split, 176, 1, G.SILU, True, 1, second=False)
    _ok(rc, "W2 = NULL")
    rows = min(M, m_split)
    verify("ll_linear_grouped2 W2 = NULL", name, out, rows, 176, *d.lin_e(True, rows, 176), G.SILU, 1)
    assert lib.ll_linear_grouped2_probe(LL_BF16, out.data_ptr(), 64, out.data_ptr(), None, 64, None, None, out.data_ptr(), 64, 10, 48, 8, 64, 1, 0, 0,
                                        _stream()) == -1          # m_split off 64


def test_grouped2_wide(lib):
    """more than 256 workgroups: the eight-wave form of the two-group kernel, and its raw slabs"""
    d2 = dev("big-K256")
    for M, m_split, n in ((200, 128, 2945), (129, 64, 2945)):           # 4 x 47 = 188 and 3 x 47 = 141 workgroups: sixteen waves
        lin, e = grouped_reference(d2, True, M, m_split, n)
        rc, out = grouped_call(lib, d2, M, m_split, n, 1, G.GELU, True, 0)
        _ok(rc, "grouped 16 waves")
        verify("ll_linear_grouped2 bf16", f"M={M} N={n}", out, M, n, lin, e, G.GELU, 0)
    for M, m_split, n, splits in ((400, 192, 2945, 1), (200, 128, 2945, 2)):   # 7 x 47 = 329 and 4 x 47 x 2 = 376: eight waves
        if splits == 1:
            for epi in G.EPIS:
                lin, e = grouped_reference(d2, True, M, m_split, n)
                rc, out = grouped_call(lib, d2, M, m_split, n, 1, epi, True, 1)
                _ok(rc, "grouped 8 waves")
                verify("ll_linear_grouped2 bf16 eight waves", f"M={M} N={n} epi={epi}", out, M, n, lin, e, epi, 1)
        else:
            rc, out = grouped_call(lib, d2, M, m_split, n, splits, 0, False, 1)
            _ok(rc, "grouped 8 waves raw")
            verify_slabs("ll_linear_grouped2 bf16 eight waves", f"M={M} N={n} splits={splits}", d2, out, M, n, splits,
                         grouped_slab_refs(d2, splits, M, m_split, n), grouped_reference(d2, False, M, m_split, n))


@pytest.mark.parametrize("name,rows,m_split,n", [("gemm-K448", 200, 128, 1003), ("gemm-K1024", 129, 64, 100), ("big-K256", 384, 128, 2945)],
                         ids=["sixteen_waves", "sixteen_waves_K1024", "eight_waves"])
def test_grouped2_column_probes(lib, name, rows, m_split, n):
    """A[m] = c e_k on both sides of m_split: c W1[:, k] above it, c W2[:, k] from it on, bit for bit; rows behind the probe rows give +0"""
    d = dev(name)
    M = min(rows, 256)
    w1, ldw, _ = d.wbuf(n)
    w2, _, _ = d.wbuf(n, col0=d.N)
    for out_f32 in (0, 1):
        probes = []
        for ks, cs in G.probe_launches(d.K, M):
            x = torch.zeros(rows, d.K, dtype=R.BF, device="cuda")
            x[:M] = R.probe_x(d.K, ks, cs, "cuda")
            want = out_buf(rows, n, n + 40, out_f32)
            want[:rows, :n] = 0
            e1, e2 = R.probe_expected(d.w[:n], ks, cs), R.probe_expected(d.w[d.N:d.N + n], ks, cs)
            exp = torch.cat((e1[:m_split], e2[m_split:M]))
            want[:M, :n] = exp.float() if out_f32 else exp
            probes.append((R.padded(x, d.K + 8)[0], want))

        def call(xb, out):
            _ok(lib.ll_linear_grouped2_probe(LL_BF16, xb.data_ptr(), d.K + 8, w1.data_ptr(), w2.data_ptr(), ldw, None, None, out.data_ptr(), n + 40, rows,
                                             m_split, n, d.K, 1, 0, out_f32, _stream()), name)
        run_probes(call, probes, rows, n, out_f32, f"grouped {name} out_f32={out_f32}")


# ------------------------------------------------------------------------------------------------------------------ packed weights
PACKED_ROWS = [("gemm-K256", 5, 128), ("gemm-K512", 33, 176), ("gemm-K768", 63, 992), ("gemm-K1024", 64, 992), ("gemm-K1024", 100, 992),
               ("gemm-K512", 128, 784), ("gemm-K256", 224, 992), ("gemm-K1024", 129, 784)]


@pytest.mark.parametrize("name,M,n", PACKED_ROWS)
def test_packed_probe(lib, name, M, n):
    """the panel kernels reading a pack_mfma16 copy: bit-identical to the unpacked call ("same products and order"), inside the intervals,
    the registry left as found; N % 16 != 0 falls back to the row-major weight"""
    d = dev(name)
    xb, lda = d.xbuf(M)
    wb, ldw, bb = d.wbuf(n, dense=True)
    scratch = torch.full((n * d.K + 64,), float("nan"), dtype=R.BF, device="cuda")
    branch = P_M64 if M <= 64 else P_M128
    tiles = 1 if M <= 64 else 2 if M <= 128 else 4
    for waves in ((8, 4) if M <= 64 else (8,)):
        with switches(lib, waves=waves):
            for out_f32 in (0, 1):
                for epi, use_bias in ((G.NONE, False), (G.GELU, True), (G.SOFTSIGN, True)):
                    tag = f"packed {name} M={M} N={n} epi={epi} out_f32={out_f32} waves={waves}"
                    ldc = n + 40
                    got, ref = out_buf(M, n, ldc, out_f32), out_buf(M, n, ldc, out_f32)
                    _ok(lib.ll_linear_packed_probe(xb.data_ptr(), lda, wb.data_ptr(), ldw, scratch.data_ptr(), _ptr(bb) if use_bias else None, got.data_ptr(),
                                                   ldc, M, n, d.K, 1, epi, out_f32, _stream()), tag)
                    assert lib.ll_debug_last_gemm_path() == panel(branch, d.K, tiles) | P_PACKED, (tag, hex(lib.ll_debug_last_gemm_path()))
                    _ok(lib.ll_linear(LL_BF16, xb.data_ptr(), lda, wb.data_ptr(), ldw, _ptr(bb) if use_bias else None, ref.data_ptr(), ldc, M, n, d.K, epi,
                                      out_f32, _stream()), tag)
                    assert lib.ll_debug_last_gemm_path() == panel(branch, d.K, tiles), (tag, "a later ll_linear on the same W still reads a packed copy")
                    assert torch.equal(_bits(got), _bits(ref)), (tag, "packed and unpacked differ")
                    verify("ll_linear_packed_probe", tag, got, M, n, *d.lin_e(use_bias, M, n), epi, out_f32)
    assert bool(torch.isnan(scratch[n * d.K:].float()).all()), "pack_mfma16 wrote behind the packed copy"
    # N % 16 != 0: the registered copy is not read
    n2 = n - 3
    got = out_buf(M, n2, n2 + 40, 0)
    _ok(lib.ll_linear_packed_probe(xb.data_ptr(), lda, wb.data_ptr(), ldw, scratch.data_ptr(), _ptr(bb), got.data_ptr(), n2 + 40, M, n2, d.K, 1, G.GELU, 0,
                                   _stream()), "ragged N")
    assert lib.ll_debug_last_gemm_path() == panel(branch, d.K, tiles), hex(lib.ll_debug_last_gemm_path())
    verify("ll_linear_packed_probe N % 16 != 0", name, got, M, n2, *d.lin_e(True, M, n2), G.GELU, 0)


def test_packed_probe_column_probes_and_slabs(lib):
    d = dev("gemm-K2048")
    M, n, splits = 64, 992, 2
    xb, lda = d.xbuf(M)
    wb, ldw, _ = d.wbuf(n, dense=True)
    scratch = torch.empty(n * d.K, dtype=R.BF, device="cuda")
    out = out_buf(splits * M, n, n + 40, 1)
    _ok(lib.ll_linear_packed_probe(xb.data_ptr(), lda, wb.data_ptr(), ldw, scratch.data_ptr(), None, out.data_ptr(), n + 40, M, n, d.K, splits, 0, 1,
                                   _stream()), "packed slabs")
    assert lib.ll_debug_last_gemm_path() == panel(P_M64, 1024, 1) | P_PACKED
    verify_slabs("ll_linear_packed_probe", "slabs", d, out, M, n, splits)
    assert lib.ll_linear_packed_probe(xb.data_ptr(), lda, xb.data_ptr(), lda, scratch.data_ptr(), None, out.data_ptr(), n + 40, M, n, d.K, 1, 0, 1,
                                      _stream()) == -1            # ldw != K: no packed copy can stand for that weight
    for name, M in (("gemm-K1024", 64), ("gemm-K512", 128), ("gemm-K256", 224)):
        d = dev(name)
        wb, ldw, _ = d.wbuf(n, dense=True)
        scratch = torch.empty(n * d.K, dtype=R.BF, device="cuda")
        for out_f32 in (0, 1):
            def call(xb, out):
                _ok(lib.ll_linear_packed_probe(xb.data_ptr(), d.K + 8, wb.data_ptr(), ldw, scratch.data_ptr(), None, out.data_ptr(), n + 40, M, n, d.K, 1, 0,
                                               out_f32, _stream()), "packed probe")
                assert lib.ll_debug_last_gemm_path() & P_PACKED
            run_probes(call, probe_set(d, M, n, M, out_f32), M, n, out_f32, f"packed {name} out_f32={out_f32}")


# ------------------------------------------------------------------------------------------------------------------ ll_linear_splitk_bf16
@pytest.mark.parametrize("M", [8, 16, 65])
@pytest.mark.parametrize("splits", [2, 16])
def test_splitk_bf16(lib, M, splits):
    d = dev("gemm-K2048")
    for n in (96, 1003):
        splitk_sweep(lib, d, "ll_linear_splitk_bf16", f"M={M} N={n}", M, n, splits)
    xb, lda = d.xbuf(M)
    wb, ldw, _ = d.wbuf(96)
    out, ws = out_buf(M, 96, 136, 0), out_buf(M, 96, 96, 1)
    for bad in (1, 17):
        assert lib.ll_linear_splitk_bf16(xb.data_ptr(), lda, wb.data_ptr(), ldw, None, out.data_ptr(), 136, M, 96, d.K, 0, bad, ws.data_ptr(), _stream()) == -1
    assert R.sentinel_damage(out, 0, 0) == 0 and R.sentinel_damage(ws, 0, 0) == 0


# ------------------------------------------------------------------------------------------------------------------ LL_GEMM_VARIANT = 0 | 2
# (set, M, N, splits, expected path): LL_GEMM_VARIANT is read once per process, so each variant runs in a child
VARIANT_ROWS = {
    0: [("gemm-K128", 100, 1003, 1, P_V0_64), ("gemm-K1024", 40, 1003, 1, P_V0_64x32), ("gemm-K1024", 40, 176, 1, P_V0_64x16),
        ("gemm-K448", 260, 1003, 1, P_V0_64), ("big-K256", 2048, 2945, 2, P_V0_128), ("gemm-K1024", 3, 128, 1, P_V0_64x16),
        ("gemm-K2056", 3, 1003, 1, P_GEMV), ("gemm-K1032", 4, 515, 1, P_GEMV), ("gemm-K64", 3, 7, 1, P_V0_64x32)],
    2: [("gemm-K1024", 40, 1000, 1, P_RING64x32), ("gemm-K1024", 100, 1000, 1, P_RING64x32), ("gemm-K448", 8, 512, 1, P_RING32),
        ("gemm-K1032", 3, 1003, 1, P_GEMV), ("big-K256", 1024, 2945, 1, P_W16_128)],
}
VARIANT_K8 = (3, 9, 8)       # M, N, K of defect 1's other form: K = 8 under variant 0 had no k-tile at all


def variant_child():
    """runs in a child process under LL_GEMM_VARIANT: one line per row, `ROW <index> <verdict>`"""
    from llamole_amd import _lib
    lib = _lib.load()
    variant = int(os.environ["LL_GEMM_VARIANT"])
    for i, (name, M, N, splits, path) in enumerate(VARIANT_ROWS[variant]):
        d = dev(name)
        try:
            if splits == 1:
                epilogue_sweep(lib, d, f"LL_GEMM_VARIANT={variant} " + PATH_NAMES[path & 255], name, M, N,
                               lambda epi, b, f, ldc: linear(lib, d, M, N, epi, b, f, ldc, name), lambda epi: path)
                if M > 4 or path != P_GEMV:
                    wb, ldw, _ = d.wbuf(N)
                    if d.K <= 1088:
                        for out_f32 in (0, 1):
                            def call(xb, out):
                                _ok(lib.ll_linear(LL_BF16, xb.data_ptr(), d.K + 8, wb.data_ptr(), ldw, None, out.data_ptr(), N + 40, M, N, d.K, 0, out_f32,
                                                  _stream()), name)
                            run_probes(call, probe_set(d, M, N, M, out_f32), M, N, out_f32, name)
            else:
                splitk_sweep(lib, d, f"LL_GEMM_VARIANT={variant} " + PATH_NAMES[path & 255], name, M, N, splits, path)
            print(f"ROW {i} ok", flush=True)
        except (AssertionError, RuntimeError) as exc:
            print(f"ROW {i} FAILED {exc!r}"[:2000].replace("\n", " "), flush=True)
            return          # nothing more on the GPU after a failure
    if variant == 0:
        M, N, K = VARIANT_K8
        g = torch.Generator().manual_seed(8)
        x, w = torch.randn(M, K, generator=g).to(R.BF), torch.randn(N, K, generator=g).to(R.BF)
        lin, e = R.linear64(x, w, None, None, 0.0, R.NONE)
        xb, wb = R.padded(x.cuda(), K + 8)[0], R.padded(w.cuda(), K + 40, rows_after=2)[0]
        out = out_buf(M, N, N + 41, 1)
        rc = lib.ll_linear(LL_BF16, xb.data_ptr(), K + 8, wb.data_ptr(), K + 40, None, out.data_ptr(), N + 41, M, N, K, 0, 1, _stream())
        outside, pos = R.check(out[:M, :N], *G.interval(lin.cuda(), e.cuda(), G.NONE, 1))
        print(f"K8 rc={rc} path={lib.ll_debug_last_gemm_path()} outside={outside} damage={R.sentinel_damage(out, M, N)}", flush=True)
    for fam in sorted(WORST):
        print(f"largest position inside the interval, {fam}: {WORST[fam]:.3f} ({COUNT[fam]} calls)", flush=True)
    for fam in sorted(GELU_USE):
        print(f"largest share of the GELU band used, {fam}: {GELU_USE[fam]:.3f}", flush=True)
    print("DONE", flush=True)


@pytest.mark.parametrize("variant", [0, 2])
def test_gemm_variant(variant):
    """LL_GEMM_VARIANT=0: the four gemm_bf16_kernel tiles, and M = 3 at K = 2056, M = 4 at K = 1032 and M = 3 at K = 8, which must take the
    GEMV (the tiles' whole 64-wide k-steps would drop the tail, all of K at K = 8); LL_GEMM_VARIANT=2: the ring in place of the panel kernels and rows16"""
    env = dict(os.environ, LL_GEMM_VARIANT=str(variant))
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_gemm_reference_gpu import variant_child; variant_child()"
    run = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    lines = run.stdout.splitlines()
    print("\n" + "\n".join(l for l in lines if l.startswith("largest")))
    assert run.returncode == 0 and "DONE" in lines, (run.returncode, run.stdout[-3000:], run.stderr[-3000:])
    for i in range(len(VARIANT_ROWS[variant])):
        assert f"ROW {i} ok" in lines, [l for l in lines if l.startswith(f"ROW {i} ")]
    if variant == 0:
        assert f"K8 rc=0 path={P_GEMV} outside=0 damage=0" in lines, [l for l in lines if l.startswith("K8")]
