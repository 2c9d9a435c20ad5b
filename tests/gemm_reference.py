"""Float64 reference with rounding intervals for the tile GEMM family behind ll_linear (llamole_amd/csrc/gemm.hip): ll_linear(LL_BF16 | LL_F32),
ll_linear_splitk_bf16, every entry of the tuning table through ll_linear_cfg, the two-group Linear of the GIN layer (ll_linear_grouped2_probe)
and the packed-weight form of the panel kernels (ll_linear_packed_probe).  Written from the contract in include/llamole_hip.h --
C = epi(A W^T + bias), epi 0 none / 1 GELU(erf) / 2 SiLU / 3 Softsign, bf16 or f32 output -- not from the kernels; linear64, bf16r, check,
the poisoned buffers and the column probes are those of tests/linear_reference.py.

bf16 operands (float64 holds them exactly):
  lin = sum_k a w + bias,  absref = sum_k |a| |w| + |bias|,  e = U absref,  U = 2^-14 (linear_reference.U)
U is derived, not measured, per kernel family from its code; "depth" is the longest chain of f32 roundings between a product and the output,
and an MFMA step (32 products into an f32 accumulator) is counted as FIVE roundings (four 8-product groups and the accumulate), which is more
than the hardware documents:
  LDS-DMA ring, unified-piece, ping-pong, register-staged and LL_GEMM_VARIANT=0 tiles   one accumulator per output over kchunk / 32 MFMA
                              steps, + bias; split-K: + at most 16 slabs added in order (slab_reduce_bf16_kernel or the test's own sum)
  panel kernels (<= 64 rows, 65..256 rows)   at most 4 MFMA steps per wave, 8 wave partials added in wave order, at most 16 slabs, + bias
  skinny (tuning table 12..16)               K / 64 / waves tiles of 2 MFMA steps per wave, at most 16 wave partials, + bias
  GEMV                                       K / 64 fmaf per lane, a 6-level wave sum, + bias
  rows16                                     see linear_reference
so depth <= 5 K / 32 + 25, and depth * 2^-24 <= 2^-14 while depth <= 1024, i.e. for K <= 6393.  The test K stays <= 4096 (2048 for the tiles;
4096 for the GEMV, depth 71, and for the <= 64-row panel kernel at 16 slabs of 256, depth 5 + 8 + 16 + 1).  No family needs a larger U.  With
an MFMA step counted as one rounding, as linear_reference does, depth <= K / 32 + 25 <= 640 up to K = 19680: that is the count behind the
decode and GraphDiT shapes of tests/test_graphdit_gpu.py (K up to 18944), which use linear64_on below.

f32 operands (LL_F32): one k-ordered fmaf chain per output and one bias add, so e = (K + 1) 2^-24 absref (worst case of the chain, gamma_K);
the operands are random f32 values, not bf16-valued ones, so that "exact f32" is what is tested.

Split-K raw slabs: slab z is checked against lin and e of its own K range (no bias, no epilogue, f32), their sum against the whole.

Epilogue: the interval of epi(v) over [lin - e, lin + e] is taken from the two ends plus the interior minimum where the interval holds it
(SiLU at -1.27846, GELU at GELU_ARGMIN = -0.75179, computed below; Softsign is monotone), widened by a band for the device's evaluation:
  SiLU      2^-20 relative (linear_reference.SILU_BAND: expf)
  Softsign  2^-22 relative: 1 + |v| and the correctly rounded division are one f32 rounding each (2^-23 together), doubled
  GELU      0.5 |v| 2^-21 ABSOLUTE (four f32 ulps of 1 + erf(v / sqrt 2): 1 + erf cancels for v < 0, so a relative band on the result would
            be wrong by orders of magnitude at v = -3) + 2^-22 relative for the two multiplies.  ROCm's erff error is not written down in
            this tree, so the band's use is measured: gelu_band_use() compares the f32 GELU output with gelu64 of the f32 output of the same
            call without epilogue (the device's own pre-activation), i.e. against float64 erf, never against another run of the kernel.
Output: bf16 runs bf16r on both ends (most elements pinned, lo == hi), f32 rounds both ends to f32.

tests/test_gemm_reference_cpu.py shows on these very operand sets that two honest f32 evaluations stay inside every interval and that sixteen
mistakes leave them.

Measured on an MI355X (tests/test_gemm_reference_gpu.py -s prints them; position = largest |got - chain(lin)| / (hi - lo), 1 is the edge):
run of 2026-10-19, 391 test cases, about 8 300 calls, no element outside its interval, every column probe bit-exact, every sentinel intact:
  bf16 output                 1.000 in every family but rows16 (ll_linear: GEMV, both panel kernels, ring 32x32 / 64x32 / 64x64 on 2x2 and
                              4x2 waves / 128x64, unified 64x64, sixteen-wave 128x128 and 256x128; ll_linear_cfg: ring, skinny, GEMV, panel,
                              register-staged, ping-pong; ll_linear_grouped2_probe; ll_linear_packed_probe; ll_linear_splitk_bf16; under
                              LL_GEMM_VARIANT=0 the 64x64, 64x32 and 64x16 tiles, the GEMV and the split-K result of the 128x128 tile; under
                              LL_GEMM_VARIANT=2 GEMV, ring 32x32, ring 64x32, sixteen-wave 128x128): the output sits at most one rounding
                              step from chain(lin), at the other end of a one-step interval.  rows16 (K = 64 and 448) 0.001: every bf16
                              element of its rows was pinned and met
  raw split-K slabs (f32)     0.001 in every family (two-group kernel on f32 operands 0.008, packed panel kernel 0.000, variant-0 128x128
                              0.001): e has room by two to three orders of magnitude
  paths off the edge          ll_linear(LL_F32) 0.125, ll_linear_grouped2_probe f32 0.042, eight-wave two-group kernel (f32 output) 0.056,
                              W2 = NULL 0.048
  GELU band                   the device's erff and its two multiplies use at most 0.270 of the band (0.234 .. 0.270 over the twelve
                              dispatch families with f32 output, the variant-0 tiles 0.237 .. 0.257, measured against float64 erf at the
                              device's own f32 pre-activation -- the sweep asserts that two launches of the plain call agree bit for bit,
                              so that output is the pre-activation the GELU launch saw): the starting band 0.5 |v| 2^-21 + 2^-22 |gelu| stands
(torch's CPU gelu in f32, by contrast, is off by 1.16 bands at v = -2.9, which is why tests/test_gemm_reference_cpu.py evaluates its GELU
with a correctly rounded erff.)"""
import functools
import math

import torch

from tests import linear_reference as R

BF, F64 = R.BF, R.F64
NONE, GELU, SILU, SOFTSIGN = 0, 1, 2, 3
EPIS = (NONE, GELU, SILU, SOFTSIGN)
EPI_NAMES = {NONE: "none", GELU: "gelu", SILU: "silu", SOFTSIGN: "softsign"}
U = R.U
U32_STEP = 2.0 ** -24
GELU_BAND_ABS = 2.0 ** -21        # times 0.5 |v|
GELU_BAND_REL = 2.0 ** -22
SOFTSIGN_BAND = 2.0 ** -22
SQRT2 = math.sqrt(2.0)


def gelu64(x):
    """0.5 x (1 + erf(x / sqrt 2)) with 1 + erf taken as erfc of the negated argument (no cancellation for x < 0)"""
    return 0.5 * x * torch.erfc(-x / SQRT2)


def softsign64(x):
    return x / (1.0 + x.abs())


def epi64(v, epi):
    return {NONE: lambda t: t, GELU: gelu64, SILU: R.silu64, SOFTSIGN: softsign64}[epi](v)


def _gelu_argmin():
    """zero of d/dx gelu = Phi(x) + x phi(x) in [-1, -0.5], by bisection in float64"""
    f = lambda x: 0.5 * math.erfc(-x / SQRT2) + x * math.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    a, b = -1.0, -0.5
    assert f(a) < 0 < f(b)
    for _ in range(200):
        m = 0.5 * (a + b)
        a, b = (m, b) if f(m) < 0 else (a, m)
    return 0.5 * (a + b)


GELU_ARGMIN = _gelu_argmin()
GELU_MIN = float(gelu64(torch.tensor(GELU_ARGMIN, dtype=F64)))
_INTERIOR = {GELU: (GELU_ARGMIN, GELU_MIN), SILU: (R.SILU_ARGMIN, R.SILU_MIN)}


def gelu_band(v, g):
    """the device band of GELU at pre-activation v with value g"""
    return 0.5 * v.abs() * GELU_BAND_ABS + g.abs() * GELU_BAND_REL


def epi_bounds(lo, hi, epi):
    """[lo', hi'] holding epi(v) as the device may evaluate it for every v in [lo, hi] (float64, any device)"""
    if epi == NONE:
        return lo, hi
    a, b = epi64(lo, epi), epi64(hi, epi)
    elo, ehi = torch.minimum(a, b), torch.maximum(a, b)
    if epi in _INTERIOR:
        xm, fm = _INTERIOR[epi]
        elo = torch.where((lo <= xm) & (hi >= xm), torch.full_like(elo, fm), elo)
    if epi == GELU:
        band = gelu_band(torch.maximum(lo.abs(), hi.abs()), torch.maximum(elo.abs(), ehi.abs()))
        return elo - band, ehi + band
    rel = R.SILU_BAND if epi == SILU else SOFTSIGN_BAND
    return elo - elo.abs() * rel, ehi + ehi.abs() * rel


def out_round(t, out_f32):
    """float64 -> the output type -> float64"""
    return t.to(torch.float32).to(F64) if out_f32 else R.bf16r(t)


def interval(lin, e, epi, out_f32):
    """lo, hi, mid (float32) of the output for pre-activations lin +- e (float64, any device)"""
    lo, hi = epi_bounds(lin - e, lin + e, epi)
    lo, hi, mid = (out_round(t, out_f32).to(torch.float32) for t in (lo, hi, epi64(lin, epi)))
    assert bool(((lo <= mid) & (mid <= hi)).all())
    return lo, hi, mid


def linear64_f32(x, w, bias):
    """lin, e of f32 operands: e = (K + 1) 2^-24 absref"""
    xd, wd = x.to(F64), w.to(F64)
    b = bias.to(F64) if bias is not None else torch.zeros(w.shape[0], dtype=F64)
    lin = xd @ wd.t() + b
    e = (x.shape[1] + 1) * U32_STEP * (xd.abs() @ wd.abs().t() + b.abs())
    assert torch.isfinite(lin).all() and torch.isfinite(e).all()
    return lin, e


def linear64_on(x, w, bias, f32=False):
    """lin, e of bf16 (e = U absref, as linear64 without a norm) or f32 operands on the device they live on: for shapes whose float64
    products are too many for the CPU"""
    xd, wd = x.to(F64), w.to(F64)
    b = bias.to(F64) if bias is not None else torch.zeros(w.shape[0], dtype=F64, device=w.device)
    lin = xd @ wd.t() + b
    e = ((x.shape[1] + 1) * U32_STEP if f32 else U) * (xd.abs() @ wd.abs().t() + b.abs())
    assert bool(torch.isfinite(lin).all()) and bool(torch.isfinite(e).all())
    return lin, e


def gelu_band_use(got_gelu, got_plain):
    """largest |got_gelu - gelu64(got_plain)| in units of the GELU band at got_plain (both f32 outputs of the same call, with and without
    the epilogue): how much of the band the device's erff and its two multiplies use; the f32 rounding of the output is part of it"""
    v = got_plain.to(F64)
    g = gelu64(v)
    band = gelu_band(v, g)
    ok = torch.isfinite(v) & (band > 0)
    return float(((got_gelu.to(F64) - g).abs() / band.clamp_min(1e-300))[ok].max()) if bool(ok.any()) else 0.0


# ------------------------------------------------------------------------------------------------------------------ the operands
class GemmSet:
    """x [M,K], w [2N,K] (a second weight matrix w[N:] and bias[N:] for the two-group Linear), bias [2N] f32; bf16 or f32 operands.
    lin, e of the whole set are computed once per (bias) and kept; a call on m rows and n columns takes [:m, :n]."""

    def __init__(self, name, f32, M, N, K, seed, wscale=1.0, bias_range=0.0):
        g = torch.Generator().manual_seed(seed * 104729 + 31 * M + 101 * N + 3 * K)
        self.name, self.f32, self.M, self.N, self.K = name, f32, M, N, K
        x = torch.randn(M, K, generator=g)
        w = torch.randn(2 * N, K, generator=g) * (wscale / math.sqrt(K))
        self.x, self.w = (x, w) if f32 else (x.to(BF), w.to(BF))
        # bias: standard normal, or uniform over +- bias_range
        self.bias = ((torch.rand(2 * N, generator=g) * 2 - 1) * bias_range if bias_range else torch.randn(2 * N, generator=g)).float()
        self._lin, self._slab = {}, {}

    def linear(self, use_bias):
        """lin, e [M, 2N] float64"""
        key = bool(use_bias)
        if key not in self._lin:
            b = self.bias if use_bias else None
            self._lin[key] = linear64_f32(self.x, self.w, b) if self.f32 else R.linear64(self.x, self.w, b, None, 0.0, R.NONE)
        return self._lin[key]

    def slabs(self, splits):
        """[(lin_z, e_z)] of the K ranges [z K / splits, (z + 1) K / splits): no bias"""
        if splits not in self._slab:
            kc = self.K // splits
            assert kc * splits == self.K
            f = (lambda x, w: linear64_f32(x, w, None)) if self.f32 else (lambda x, w: R.linear64(x, w, None, None, 0.0, R.NONE))
            self._slab = {splits: [f(self.x[:, z * kc:(z + 1) * kc], self.w[:, z * kc:(z + 1) * kc]) for z in range(splits)]}
        return self._slab[splits]


def check_sum(total, lin, e):
    """a float64 sum of raw slabs against lin +- e: (elements outside, largest |total - lin| / (2 e))"""
    lin, e = lin.to(total.device), e.to(total.device)
    dev = (total - lin).abs()
    bad = ~(dev <= e)
    return int(bad.sum()), float((dev / (2 * e).clamp_min(1e-300)).max())


# name -> (f32 operands, rows, N, K, wscale, bias_range).  bf16: the K of every dispatch threshold and ring depth; "cfg" sets serve the
# tuning table (ragged N for every tile width up to 256, rows up to 2 * 256 - 3); "big" serves the tiles that need >= 192 workgroups;
# "tall" the 128 x 64 ring, which needs >= 1024 workgroups below a K chunk of 256;
# "wide" the 64-row weight-streaming tiles that need >= 200 column tiles; "gelu" has small sums and pre-activations spread evenly over
# +-3.5 by the bias, so that e is small where tanh-GELU and erf-GELU differ most.
SETS = {f"gemm-K{K}": (False, 260, 1003, K, 1.0, 0.0) for K in (64, 128, 256, 448, 512, 768, 1024, 1032, 1536, 2048, 2056, 4096)}
SETS.update({f"cfg-K{K}": (False, 509, 300, K, 1.0, 0.0) for K in (64, 128, 192, 256, 320, 384, 448, 512, 576, 640, 768, 896, 1024, 2048)})
SETS["big-K256"] = (False, 2048, 2945, 256, 1.0, 0.0)
SETS["wide-K128"] = (False, 64, 16330, 128, 1.0, 0.0)
SETS["tall-K128"] = (False, 2048, 4040, 128, 1.0, 0.0)
SETS["gelu-K64"] = (False, 130, 200, 64, 0.25, 3.5)
SETS.update({f"f32-K{K}": (True, 200, 176, K, 1.0, 0.0) for K in (16, 48, 1024)})
SETS["f32-gelu-K16"] = (True, 200, 176, 16, 0.25, 3.5)


@functools.lru_cache(maxsize=3)
def gemm_set(name):
    f32, M, N, K, ws, br = SETS[name]
    return GemmSet(name, f32, M, N, K, seed=sorted(SETS).index(name), wscale=ws, bias_range=br)


# ------------------------------------------------------------------------------------------------------------------ the tuning table
# id -> (family, BM, BN, stages): what include/llamole_hip_tuning.h documents of g_pipe_cfgs (gemm.hip); stages 0 = not a ring
RING, SKINNY, GEMV_CFG, PANEL, RS, PP = "ring", "skinny", "gemv", "panel", "rs", "pp"
CFGS = {}
for _i, (_bm, _bn, _st) in enumerate([(128, 64, 4), (64, 64, 4), (64, 32, 4), (64, 32, 8), (64, 64, 8), (128, 64, 6), (128, 128, 3), (128, 128, 4),
                                      (64, 128, 4), (256, 64, 3), (64, 64, 2), (64, 128, 6)]):
    CFGS[_i] = (RING, _bm, _bn, _st)
for _i in range(12, 17):
    CFGS[_i] = (SKINNY, 64, (32, 16, 32, 16, 64)[_i - 12], (8, 8, 4, 16, 8)[_i - 12])          # stages = waves that split K
for _i, (_bm, _bn, _st) in zip(range(17, 23), [(128, 64, 4), (128, 128, 3), (128, 128, 4), (64, 64, 4), (256, 64, 3), (128, 64, 6)]):
    CFGS[_i] = (RING, _bm, _bn, _st)
for _i in range(23, 31):
    CFGS[_i] = (GEMV_CFG, 1, (4, 2, 8, 4, 2, 1, 8, 1)[_i - 23], (4, 4, 2, 8, 8, 8, 4, 16)[_i - 23])   # BN = rows per wave, stages = unroll
for _i, _ns in zip(range(31, 34), (8, 4, 2)):
    CFGS[_i] = (PANEL, 64, 16, _ns)                                                              # stages = K chunk / 128
for _i, (_bm, _bn, _st) in zip(range(34, 41), [(32, 96, 4), (32, 96, 6), (32, 128, 4), (32, 64, 4), (32, 64, 6), (32, 224, 4), (32, 32, 8)]):
    CFGS[_i] = (RING, _bm, _bn, _st)
for _i, (_bm, _bn) in zip(range(41, 48), [(128, 64), (64, 128), (128, 128), (64, 64), (128, 64), (128, 32), (256, 64)]):
    CFGS[_i] = (RS, _bm, _bn, 2)
for _i, (_bm, _bn, _st) in zip(range(48, 56), [(128, 64, 4), (128, 64, 5), (128, 64, 6), (64, 64, 4), (64, 64, 6), (128, 128, 4), (128, 128, 5),
                                              (64, 128, 5)]):
    CFGS[_i] = (PP, _bm, _bn, _st)
for _i, (_bm, _bn, _st) in zip(range(56, 68), [(256, 128, 3), (256, 128, 3), (128, 256, 3), (256, 256, 2), (128, 128, 4), (128, 128, 3),
                                              (256, 128, 3), (128, 128, 5), (64, 64, 4), (64, 64, 6), (64, 128, 4), (128, 64, 4)]):
    CFGS[_i] = (RING, _bm, _bn, _st)
assert sorted(CFGS) == list(range(68))


def cfg_cases(cfg):
    """[(set name, M, N, K, splits)] of one tuning-table entry: rows BM - 1, BM and 2 BM - 3 (within the entry's row limit), ragged N, k-tile
    counts below, at and above the ring depth, splits 1 and 2"""
    fam, bm, bn, st = CFGS[cfg]
    if fam == GEMV_CFG:
        return [(f"gemm-K{K}", 1, n, K, 1) for K in (64, 1032, 4096) for n in (1, 4 * bn + 1, 1003)]
    if fam == SKINNY:
        return [(f"cfg-K{K}", m, 300, K, 1) for K in (64, 576, 2048) for m in (63, 64, 125)]
    if fam == PANEL:
        return [(f"gemm-K{st * 128 * s}", m, n, st * 128 * s, s) for s in (1, 2) if st * 128 * s <= 2048 for m in (63, 64) for n in (176, 1003)]
    bk = 128 if fam == RS else 64
    nks = sorted({max(1, st - 2), st - 1, st + 1}) if fam != RS else [1, 2, 3, 4]
    out = []
    for m in (bm - 1, bm, 2 * bm - 3):
        for nk in nks:
            out.append((f"cfg-K{bk * nk}", m, 300, bk * nk, 1))
        nk2 = max(1, st - 1) if fam != RS else 2
        out.append((f"cfg-K{2 * bk * nk2}", m, 300, 2 * bk * nk2, 2))
    assert all(c[0] in SETS for c in out), [c for c in out if c[0] not in SETS]
    return out


# ------------------------------------------------------------------------------------------------------------------ column probes
def probe_launches(K, M):
    """linear_reference.probe_launches with up to 256 rows per launch"""
    return R.probe_launches(K, min(M, 256))
