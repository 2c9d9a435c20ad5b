"""Float64 reference with rounding intervals for the decode Linears (ll_gemv_fused_bf16, ll_linear_rows16_bf16, ll_linear_rows64_bf16 with
ll_rows64_pack_bf16 / ll_rows64_prenorm_bf16, and the plain ll_linear(LL_BF16) / ll_linear_splitk_bf16) and the operands both reference tests
run on.  Written from the contract in include/llamole_hip.h and HuggingFace's formulas (Qwen2RMSNorm, nn.Linear, act_fn(gate) * up), not from
the kernels.

Everything is float64, computed from the bf16 operands (which float64 holds exactly).
  effective input xe and row scale r
    no norm                                    xe = x,                                  r = 1
    HF form     (ll_gemv_fused_bf16, norm_w)   xe = bf16(norm_w * bf16(x * rstd)),      r = 1,       rstd = (mean(x^2) + eps)^-1/2
    staged form (rows16 norm_w, rows64 row_ssq) xe = bf16(x * norm_w)  (exact in f32),  r = rstd     ("up to the place of one bf16 rounding")
  lin    = r sum_k xe w + bias
  absref = r sum_k |xe| |w| + |bias|
  e      = 2^-14 absref
The constant is derived, not measured: every kernel sums in f32 with a depth of at most K / 32 + 48 additions (an FMA chain per lane or per
wave, then a shuffle tree or an ordered sum of at most 8 slices and 4 k-parts), below 640 for K <= 18944 (K / 64 + 6 per lane for the GEMV up
to K = 20488), and 640 * 2^-24 < 2^-14: a worst-case bound, so a kernel that leaves it is wrong, not unlucky.  The HF form adds the effect of
rstd being an f32 rsqrtf: xe is evaluated at rstd (1 +- 2^-20) and |delta xe_k| |w_nk| joins e where the two differ.

The accepted interval runs the header's rounding chain (to bf16 through f32, as the kernels round) on lin - e and lin + e:
    plain      bf16(lin)
    residual   bf16(res + bf16(lin))
    SiLU*mul   bf16(bf16(silu(bf16(g))) * bf16(u))
Every step but silu is monotone; for SiLU*mul the interval of bf16(silu(.)) comes from the two ends of g (plus silu's minimum at
x = -1.27846 when g's interval holds it), widened by 2^-20 relative for the kernels' expf, times the u interval by corners.  An output passes
iff lo <= got <= hi (NaN fails).  Most elements have lo == hi, i.e. are pinned bit for bit; the others are free by the one rounding step the
f32 summation order can move.

Random data cannot show one lost product among thousands, so column probes x[m] = c e_k pin out[m, :] == bf16(c W[:, k]) exactly for the
plain epilogue (a lost product gives 0, a doubled one 2 w); an eps case (x * 2^-10: mean(x^2) ~ eps) makes the row scale depend on eps;
every operand is a view into a larger allocation whose other bytes are NaN (inputs) or a sentinel (outputs).

tests/test_decode_linear_reference_cpu.py shows on these very cases that two f32 evaluations stay inside every interval (largest |err| / e
about 1e-3) and that sixteen mistakes a kernel of this kind can make leave them.

Largest |got - chain(lin)| / (hi - lo) measured on an MI355X (tests/test_decode_linear_reference_gpu.py -s prints them; 1 is the edge: the
output sits one rounding step from chain(lin), at the other end of a one-step interval):
  ll_gemv_fused_bf16      generic 0.002, x staged in LDS 0.000, RMSNorm prologue 0.100 -- no free element of a one-step interval left
                          chain(lin): the FMA chains of the GEMV are closer to float64 than the interval can resolve
  ll_linear_rows16_bf16   1.000 with and without the RMSNorm prologue
  ll_linear_rows64_bf16   1.000 on every path (one launch, K split + slab sum, row scale in either, the next norm, SiLU*mul); 0.034 for
                          SiLU*mul with the row scale (168 calls)
  ll_linear(LL_BF16)      GEMV 0.000, MFMA tiles 1.000;  ll_linear_splitk_bf16 1.000
No element of ~39 000 calls outside its interval, every column probe bit-exact, every sentinel intact."""
import functools
import math

import torch

BF = torch.bfloat16
F64 = torch.float64
PLAIN, RESIDUAL, SILU_MUL = 0, 1, 2
NONE, HF, STAGED = "none", "hf", "staged"
EPIS = (PLAIN, RESIDUAL, SILU_MUL)
U = 2.0 ** -14                   # e = U absref
RSTD_BAND = 2.0 ** -20           # f32 rsqrtf of the HF form
SILU_BAND = 2.0 ** -20           # approximate expf inside silu
SILU_ARGMIN = -1.2784645427610738
NAN = float("nan")
SENTINEL = 0x7FA5                # bf16 bit pattern (a NaN no arithmetic produces) behind every output; as int16: 32677
SENTINEL_F32 = -(2.0 ** 120)
EPS = 1e-6


# ------------------------------------------------------------------------------------------------------------------ the reference itself
def bf16r(t):
    """float64 -> float32 -> bf16 (round to nearest even twice, as a kernel that holds the value in an f32 register does), back as float64"""
    return t.to(torch.float32).to(BF).to(F64)


def silu64(x):
    return x / (1.0 + torch.exp(-x))


SILU_MIN = float(silu64(torch.tensor(SILU_ARGMIN, dtype=F64)))


def eps32(eps):
    """the eps a kernel sees: the C ABI takes a float"""
    return float(torch.tensor(eps, dtype=torch.float32))


def rstd64(x, eps, denom=None):
    """(mean(x^2) + eps)^-1/2 per row, [M,1]"""
    xd = x.to(F64)
    return ((xd * xd).sum(-1, keepdim=True) / (denom or x.shape[-1]) + eps32(eps)).rsqrt()


def effective_input(x, norm_w, eps, form):
    """xe [M,K], r [M,1], dxe [M,K] (HF form: |xe(rstd (1 + 2^-20)) - xe(rstd (1 - 2^-20))|, else None)"""
    xd = x.to(F64)
    one = torch.ones(x.shape[0], 1, dtype=F64)
    if form == NONE:
        return xd, one, None
    nw, rs = norm_w.to(F64), rstd64(x, eps)
    if form == STAGED:
        return bf16r(xd * nw), rs, None
    assert form == HF, form
    hf = lambda s: bf16r(nw * bf16r(xd * s))
    return hf(rs), one, (hf(rs * (1 + RSTD_BAND)) - hf(rs * (1 - RSTD_BAND))).abs()


def linear64(x, w, bias, norm_w, eps, form):
    """lin, e [M, rows of w]"""
    xe, r, dxe = effective_input(x, norm_w, eps, form)
    wd = w.to(F64)
    b = bias.to(F64) if bias is not None else torch.zeros(w.shape[0], dtype=F64)
    lin = r * (xe @ wd.t()) + b
    e = U * (r * (xe.abs() @ wd.abs().t()) + b.abs())
    if dxe is not None:
        e = e + dxe @ wd.abs().t()
    assert torch.isfinite(lin).all() and torch.isfinite(e).all()
    return lin, e


def chain(v, epi, res=None, up=None):
    """the header's rounding chain on an exact pre-rounding value v (SiLU*mul: v = gate, up = up)"""
    if epi == PLAIN:
        return bf16r(v)
    if epi == RESIDUAL:
        return bf16r(res.to(F64) + bf16r(v))
    return bf16r(bf16r(silu64(bf16r(v))) * bf16r(up))


def interval(lin, e, epi, res=None):
    """lo, hi, mid (float32 holding bf16 values) of the output.  plain / residual: lin, e [M,N]; SiLU*mul: [M,2N], gate columns then up columns."""
    lo, hi = lin - e, lin + e
    if epi != SILU_MUL:
        out = chain(lo, epi, res), chain(hi, epi, res), chain(lin, epi, res)
    else:
        N = lin.shape[1] // 2
        glo, ghi, ulo, uhi = bf16r(lo[:, :N]), bf16r(hi[:, :N]), bf16r(lo[:, N:]), bf16r(hi[:, N:])
        a, b = silu64(glo), silu64(ghi)
        slo, shi = torch.minimum(a, b), torch.maximum(a, b)
        slo = torch.where((glo <= SILU_ARGMIN) & (ghi >= SILU_ARGMIN), torch.full_like(slo, SILU_MIN), slo)
        slo, shi = bf16r(slo - slo.abs() * SILU_BAND), bf16r(shi + shi.abs() * SILU_BAND)
        c = torch.stack((slo * ulo, slo * uhi, shi * ulo, shi * uhi))
        out = bf16r(c.amin(0)), bf16r(c.amax(0)), chain(lin[:, :N], epi, up=lin[:, N:])
    lo, hi, mid = (t.to(torch.float32) for t in out)
    assert bool(((lo <= mid) & (mid <= hi)).all())
    return lo, hi, mid


def check(got, lo, hi, mid):
    """(number of elements outside their interval, largest |got - mid| / (hi - lo)); NaN is outside; a pinned element (lo == hi) that differs
    counts inf.  Works on the device of `got`."""
    g = got.to(torch.float32)
    lo, hi, mid = lo.to(g.device), hi.to(g.device), mid.to(g.device)
    assert g.shape == lo.shape, (g.shape, lo.shape)
    if g.numel() == 0:
        return 0, 0.0
    bad = ~((g >= lo) & (g <= hi))
    width, dev = hi - lo, (g - mid).abs()
    inf = torch.full_like(dev, math.inf)
    ratio = torch.where(width > 0, dev / width, torch.where(dev == 0, torch.zeros_like(dev), inf))
    ratio = torch.where(torch.isnan(ratio), inf, ratio)
    return int(bad.sum()), float(ratio.max())


# ------------------------------------------------------------------------------------------------------------------ poisoned buffers
def padded(t, ld, rows_after=1, fill=NAN):
    """a [rows + rows_after, ld] allocation filled with `fill` whose [:rows, :width] corner holds t; returns (allocation, view)"""
    rows, width = t.shape
    assert ld >= width
    buf = torch.full((rows + rows_after, ld), fill, dtype=t.dtype, device=t.device)
    buf[:rows, :width] = t
    return buf, buf[:rows, :width]


def padded_vec(t, after=8, fill=NAN):
    buf = torch.full((t.numel() + after,), fill, dtype=t.dtype, device=t.device)
    buf[:t.numel()] = t
    return buf


def out_buffer(M, N, ld, device="cpu", rows_after=1):
    """bf16 [M + rows_after, ld] holding the sentinel everywhere"""
    return torch.full((M + rows_after, ld), SENTINEL, dtype=torch.int16, device=device).view(BF)


def sentinel_damage(buf, M, N):
    """number of elements outside [:M, :N] that no longer hold the sentinel"""
    if buf.dtype == torch.float32:
        hit = buf != SENTINEL_F32
    else:
        hit = buf.view(torch.int16) != SENTINEL
    hit = hit.clone()
    hit[:M, :N] = False
    return int(hit.sum())


# ------------------------------------------------------------------------------------------------------------------ the operands
class Operands:
    """One operand set: x [M,K], w [2N,K] (gate rows then up rows; a plain Linear of n <= N output rows takes w[:n], a gated one w[:n] and
    w[N:N+n]), bias [2N] f32, res [M,N], norm_w [K], next_norm_w [N], eps; references are computed once per (form, bias) and kept."""

    def __init__(self, name, M, N, K, seed, xscale=1.0):
        g = torch.Generator().manual_seed(seed * 7919 + 31 * M + 101 * N + 3 * K)
        self.name, self.M, self.N, self.K, self.eps = name, M, N, K, EPS
        self.x = (torch.randn(M, K, generator=g) * xscale).to(BF)
        self.w = (torch.randn(2 * N, K, generator=g) * 0.02).to(BF)
        self.bias = torch.randn(2 * N, generator=g).float()
        self.res = torch.randn(M, N, generator=g).to(BF)
        self.norm_w = (1 + 0.1 * torch.randn(K, generator=g)).to(BF)
        self.next_norm_w = (1 + 0.1 * torch.randn(N, generator=g)).to(BF)
        self._lin, self._iv = {}, {}

    def linear(self, form, use_bias):
        """lin, e [M,2N]"""
        key = (form, bool(use_bias))
        if key not in self._lin:
            self._lin[key] = linear64(self.x, self.w, self.bias if use_bias else None, self.norm_w, self.eps, form)
        return self._lin[key]

    def bounds(self, form, use_bias, epi):
        """lo, hi, mid [M,N] float32 of the whole set; a call on m rows and n output columns takes [:m, :n]"""
        key = (form, bool(use_bias), epi)
        if key not in self._iv:
            lin, e = self.linear(form, use_bias)
            if epi == SILU_MUL:
                self._iv[key] = interval(lin, e, epi)
            else:
                self._iv[key] = interval(lin[:, :self.N], e[:, :self.N], epi, self.res)
        return self._iv[key]


# name -> (rows, largest N, K, x scale).  K reaches every path boundary of the kernels' contracts; N stays small where K is long.
GEMV_SETS = {f"gemv-K{K}": (4, 1003 if K <= 4104 else 9, K, 1.0) for K in (8, 24, 2048, 2056, 4096, 4104, 8184, 8192, 20480, 20488)}
GEMV_SETS["gemv-eps-K2048"] = (4, 9, 2048, 2.0 ** -10)
GEMV_K_NORM = (8, 2048, 4096, 4104, 8192)                    # XC = 2 | 4 of the prologue and its limit
GEMV_K_NORM_LIMIT = 8192
GEMV_N, GEMV_N_SILU, GEMV_M = (1, 2, 7, 8, 9, 1003), (1, 3, 4, 5, 1003), (1, 2, 3, 4)

ROWS16_SETS = {f"rows16-K{K}": (16, 1003 if K <= 4640 else 24, K, 1.0) for K in (32, 64, 160, 288, 4640, 18944)}
ROWS16_SETS["rows16-eps-K160"] = (16, 24, 160, 2.0 ** -10)
ROWS16_N, ROWS16_M = (1, 15, 16, 17, 24, 1003), (1, 3, 4, 5, 15, 16)
ROWS16_GEOMETRIES = [(0, 0, 0)] + [(seg, waves, ks) for seg in (128, 256, 512) for waves in (4, 8) for ks in (1, 2, 4, 8) if ks <= waves]


def rows16_lds_bytes(seg, waves, epi):
    """the wave-private LDS images of a workgroup: (weight sub-tiles + x) x 16 rows x (segment + 16 bytes) per wave"""
    return waves * ((2 if epi == SILU_MUL else 1) + 1) * 16 * (seg + 16)


LDS_LIMIT = 160 * 1024

ROWS64_SETS = {f"rows64-K{K}": (64, 2584 if K <= 1056 else 1032, K, 1.0) for K in (32, 96, 512, 544, 1056, 4640)}
ROWS64_SETS["rows64-eps-K512"] = (64, 80, 512, 2.0 ** -10)
ROWS64_N, ROWS64_M = (1, 3, 16, 63, 64, 65, 80, 1003, 1032, 2584), (1, 16, 17, 32, 33, 48, 49, 64)
ROWS64_KSPLIT = (0, 1, 2, 4, 8)

# the other entry points a decode reaches a Linear through (plain epilogue): ll_linear(LL_BF16) and ll_linear_splitk_bf16
LINEAR_SETS = {"linear-K2056": (4, 1003, 2056, 1.0), "linear-K2048": (128, 1003, 2048, 1.0)}

SETS = dict(**GEMV_SETS, **ROWS16_SETS, **ROWS64_SETS, **LINEAR_SETS)


@functools.lru_cache(maxsize=4)
def operands(name):
    M, N, K, xscale = SETS[name]
    return Operands(name, M, N, K, seed=sorted(SETS).index(name), xscale=xscale)


def forms(name):
    """the (form, kernel) pairs a set is run with"""
    K = SETS[name][2]
    if name.startswith("gemv"):
        return (NONE, HF) if K in GEMV_K_NORM else (NONE,)
    if name.startswith("linear"):
        return (NONE,)
    return (NONE, STAGED)


# ------------------------------------------------------------------------------------------------------------------ column probes
def probe_columns(K):
    """every k for K <= 1088; beyond: every k with k % 32 in {0, 31} and every k of the first and last 512 with k % 8 in {0, 7}"""
    if K <= 1088:
        return list(range(K))
    ks = {k for k in range(K) if k % 32 in (0, 31)}
    ks |= {k for k in list(range(512)) + list(range(K - 512, K)) if k % 8 in (0, 7)}
    return sorted(ks)


PROBE_SCALES = (1.0, -2.0, 0.5, -1.0)


def probe_launches(K, M):
    """[(ks, cs)]: launches of M rows x = c e_k covering probe_columns(K) (the last launch wraps round to the first columns)"""
    cols = probe_columns(K)
    out = []
    for i in range(0, len(cols), M):
        ks = [cols[(i + j) % len(cols)] for j in range(M)]
        out.append((ks, [PROBE_SCALES[(i // M + j) % len(PROBE_SCALES)] for j in range(M)]))
    return out


def probe_x(K, ks, cs, device="cpu"):
    x = torch.zeros(len(ks), K, dtype=BF, device=device)
    x[torch.arange(len(ks), device=device), torch.tensor(ks, device=device)] = torch.tensor(cs, dtype=BF, device=device)
    return x


def probe_expected(w, ks, cs):
    """out[m, :] = bf16(c_m W[:, k_m]): exact (c is a power of two)"""
    return (w[:, torch.tensor(ks, device=w.device)].float() * torch.tensor(cs, device=w.device)).t().to(BF)
