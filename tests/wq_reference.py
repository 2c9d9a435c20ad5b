"""Cases, an independent quantiser and the constant for the packed-weight (MX) decode Linears: ll_wq_quantize_bf16 / ll_wq_dequantize_bf16,
ll_gemv_fused_wq (1..4 rows, f32 FMA) and ll_linear_rows16_wq (1..16 rows, MFMA).  The float64 reference, the rounding intervals, the poisoned
buffers and the probe helpers are those of tests/linear_reference.py: a dequantised MX matrix is an ordinary bf16 matrix, so nothing of the
reference changes.  What this module adds is the weight the kernels are judged against and the shapes they are judged at.

The quantiser (quantize64) is written from the contract in include/llamole_hip.h, in float64, without the exponent-field arithmetic of the
device code or of llm_quant.mx_round:
    amax   largest |w| of a block of 32 consecutive elements along K (bf16 values)
    e      the smallest integer with amax * 2^-e <= elem_max (448 for E4M3, 6 for E2M1): found with frexp, then checked -- e fits, e - 1 does
           not -- by exact multiplications with powers of two; clamped to [-117, 119] (8 bits) / [-125, 125] (4 bits); 0 for a zero block
    code   |w| * 2^-e rounded to the nearest value of the element grid, ties to the even code; the grid is written out value by value
    W      sign(w) * grid value * 2^e, exactly a bf16 number; the scale byte is e + 127
A block the clamp touches: at the LOW end (amax so small that e would lie below the clamp) the grid step becomes 2^-9 * 2^-117 =
0.5 * 2^-125 = 2^-126, the smallest normal bf16: elements round to multiples of 2^-126, a bf16-subnormal element to 0 or +-2^-126 (2^-127 is
a tie and goes to the even code, 0).  At the HIGH end (amax > 448 * 2^119 = 1.75 * 2^127, resp. 6 * 2^125 = 1.5 * 2^127) "no element
saturates" no longer holds: |w| * 2^-e exceeds elem_max and the element SATURATES to elem_max, so the largest finite bf16 (1.9921875 * 2^127)
dequantises to 1.75 * 2^127 at 8 bits and 1.5 * 2^127 at 4.  Nothing becomes inf, NaN or a subnormal.
tests/test_wq_reference_cpu.py asserts quantize64 == mx_round on every matrix of this module, tests/test_wq_reference_gpu.py asserts
ll_wq_quantize_bf16 (its Wdq and its packed form read back through ll_wq_dequantize_bf16) == quantize64 bit for bit, and the kernels are
then judged against quantize64's W: a quantiser bug and a GEMV bug cannot cancel.

The constant stays U = 2^-14 (e = U absref), derived again for these kernels from llamole_amd/csrc/llm_wq.hip:
  gemv_wq_kernel    chunk c (16 B of codes: 16 elements at 8 bits, 32 at 4) of a row belongs to lane c % 64; a lane adds its products by one
                    fmaf chain: ceil(K / (64 EPC)) EPC links, i.e. K / 64 rounded up to whole steps; then the 6 steps of wave_sum, then the
                    bias: depth ceil(K / (64 EPC)) EPC + 7.  At 8 bits that is <= 640 up to K = 39936 (39 steps, 631), at 4 bits up to
                    K = 38912 (19 steps, 615) -- which happen to be the largest K the LDS rule admits for two rows.  The largest K for ONE row
                    (80896 / 79872) has depth 1271 / 1255: the intervals are not derived there, so that K runs the column probes, which need
                    no U, and its refusal test; it gets no interval (gemv_interval_ok).  U is not widened.
  rows16_wq_kernel  a wave adds one v_mfma_f32_16x16x32_bf16 per 32-block of its K slice: ceil(K / 32 / ksplit) accumulator updates, the
                    31 additions inside a step counted once, at most 7 ordered additions of the other slices' partial sums, the row scale
                    and the bias: K / 32 + 31 + 7 + 2 = 632 at K = 18944 with ksplit = 1, fewer with more slices.  <= 640.
  640 * 2^-24 < 2^-14.  A kernel that leaves an interval is wrong, not unlucky.

Operand sets are built like linear_reference.Operands; the weight is 0.02 randn times a power of two in 2^-3 .. 2^3 drawn per (row, block),
with one all-zero block and one single-outlier block among the gate rows and among the up rows, then rounded by quantize64 (seven or more distinct
scale bytes per matrix; every block contributes inside the interval width).  Blocks 2^30 apart, at the clamp ends, of subnormals and of the
largest finite bf16 are in the PROBE matrices (probe_matrix), whose scale bytes vary along K and along N: x[m] = c e_k pins
out[m, :] == bf16(c W[:, k]) exactly whatever the magnitudes.

tests/test_wq_reference_cpu.py shows on these very cases that two f32 evaluations (the GEMV's chunk-to-lane order; 32-wide blocks with a
slice sum) stay inside every interval -- largest |err| / e 2.6e-3 -- and that every seeded mistake of its list leaves one.

Largest |got - chain(lin)| / (hi - lo) measured on an MI355X (tests/test_wq_reference_gpu.py -s prints them; 1 is the edge: the output sits
one rounding step from chain(lin), at the other end of a one-step interval):
  ll_gemv_fused_wq     8 bits: no norm 1.000, RMSNorm prologue
                       XC = 2 0.010, XC = 4 0.000;  4 bits: no norm 0.059, prologue XC = 2 1.000, XC = 4 0.071
  ll_linear_rows16_wq  1.000 at both widths with and without the RMSNorm prologue, as the bf16 MFMA kernel shows
No element of 6 396 GEMV calls and 33 120 rows16 calls (15 geometries) outside its interval, every column probe bit-exact (the clamp ends,
the subnormal blocks and c W = -inf behind a saturated maximum included), every sentinel and every 0xFF byte around a packed form intact,
the device quantiser equal to quantize64 bit for bit on every matrix (the 32 832-row one that makes its grid-stride loop iterate included).
One refusal the K list meets: four rows of K = 18944 at 4 bits pad to 4 x 20480 elements of x, which the header's LDS rule refuses
(gemv_k_limit(4, 4) = 18432); the tests expect LL_EINVAL there and the other three row counts run."""
import functools
import math

import torch

from tests import linear_reference as L
from tests.linear_reference import BF, F64, HF, NONE, STAGED, PLAIN, RESIDUAL, SILU_MUL, EPIS, LDS_LIMIT  # noqa: F401  (re-exported)

BITS = (8, 4)
BLOCK = 32
ELEM_MAX = {8: 448.0, 4: 6.0}
E_CLAMP = {8: (-117, 119), 4: (-125, 125)}
BF16_MAX = float.fromhex("0x1.fep127")
DEPTH_LIMIT = 640                # additions U = 2^-14 covers


# ------------------------------------------------------------------------------------------------------------------ the quantiser
@functools.lru_cache(maxsize=None)
def grid(bits):
    """the non-negative values of the element format in code order: index == code without the sign bit"""
    if bits == 4:                # E2M1
        return torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=F64)
    vals = [m * 2.0 ** -9 for m in range(8)]                                             # exponent field 0: 0 and the subnormals m 2^-9
    vals += [(1 + m / 8) * 2.0 ** (ex - 7) for ex in range(1, 16) for m in range(8)]     # E4M3, bias 7
    return torch.tensor(vals[:-1], dtype=F64)                                            # e4m3fn: the last code is NaN; the largest is 448


def pow2(e):
    """2^e in float64 (exact), e an integer tensor"""
    return torch.pow(torch.tensor(2.0, dtype=F64), e.to(F64))


def quantize64(w, bits):
    """w [N,K] bf16 -> (W [N,K] bf16: the dequantised matrix, scale bytes [N,K/32] uint8); see the module docstring"""
    assert w.dtype == BF and w.dim() == 2 and w.shape[1] % BLOCK == 0
    N, K = w.shape
    vmax, (lo, hi), g = ELEM_MAX[bits], E_CLAMP[bits], grid(bits)
    assert float(g[-1]) == vmax
    blk = w.to(F64).reshape(N, K // BLOCK, BLOCK)
    amax = blk.abs().amax(-1)
    fits = lambda e: amax * pow2(-e) <= vmax
    e = torch.frexp(amax)[1].to(torch.int64) - math.frexp(vmax)[1]
    e = e + (~fits(e)).to(torch.int64)
    nz = amax > 0
    assert bool(fits(e).all()) and not bool(fits(e - 1)[nz].any())      # the smallest e that fits
    e = torch.where(nz, e.clamp(lo, hi), torch.zeros_like(e))
    a = (blk.abs() * pow2(-e).unsqueeze(-1)).clamp(max=vmax)            # exact; the clamp acts only where e was clamped from above
    up = torch.searchsorted(g, a.reshape(-1)).reshape(a.shape)          # the first grid value >= a
    dn = (up - 1).clamp(min=0)
    d_up, d_dn = g[up] - a, a - g[dn]
    take_up = (d_up < d_dn) | ((d_up == d_dn) & (up % 2 == 0))          # nearest; a tie goes to the even code
    q = torch.where(take_up, g[up], g[dn])
    dq = torch.copysign(q * pow2(e).unsqueeze(-1), blk).reshape(N, K)   # the sign of w, of a zero as well
    out = dq.to(BF)
    assert torch.equal(out.to(F64), dq)                                 # code * 2^e is exactly a bf16 number
    return out, (e + 127).to(torch.uint8)


# ------------------------------------------------------------------------------------------------------------------ limits of the contract
def gemv_lds_bytes(M, K, bits):
    """the header's rule for ll_gemv_fused_wq: M rows of x, each padded to a multiple of 1024 (8 bits) / 2048 (4 bits) elements, plus 16 M bytes"""
    pad = 8192 // bits
    return M * ((K + pad - 1) // pad * pad) * 2 + 16 * M


def gemv_k_limit(M, bits):
    """the largest K (a multiple of 32) with gemv_lds_bytes <= 160 KB; K + 32 is the first one refused"""
    pad = 8192 // bits
    return (LDS_LIMIT // M - 16) // 2 // pad * pad


def gemv_depth(K, bits):
    epc = 128 // bits
    return -(-K // (64 * epc)) * epc + 7


def gemv_interval_ok(K, bits):
    return gemv_depth(K, bits) <= DEPTH_LIMIT


def rows16_depth(K):
    return K // 32 + 31 + 7 + 2


GEMV_K_NORM_LIMIT = 8192
WQ_GEOMETRIES = [(0, 0, 0)] + [(cseg, waves, ks) for cseg in (128, 256) for waves in (4, 8) for ks in (1, 2, 4, 8) if ks <= waves]


def rows16_wq_lds_bytes(bits, cseg, waves, epi):
    """wave-private images: (weight sub-tiles + x) x 16 rows x (bf16 image of a code segment + 16 bytes); 4-bit matrices know 128-byte code
    segments only (ll_set_wq_geometry's 256 runs them as 128)"""
    seg = cseg if bits == 8 else 128
    return waves * ((2 if epi == SILU_MUL else 1) + 1) * 16 * (seg * 16 // bits + 16)


# ------------------------------------------------------------------------------------------------------------------ the operands
class Operands(L.Operands):
    """linear_reference.Operands whose weight is an MX matrix: .src [2N,K] bf16 is what the device quantiser is given, .w = quantize64(src)
    what the reference multiplies by, .scale_bytes [2N,K/32]"""

    def __init__(self, name, bits, M, N, K, seed, xscale=1.0):
        super().__init__(name, M, N, K, seed, xscale)
        g = torch.Generator().manual_seed(seed * 104729 + K)
        nb = K // BLOCK
        s = torch.randint(-3, 4, (2 * N, nb), generator=g)
        src = (self.w.float() * pow2(s).float().repeat_interleave(BLOCK, dim=1)).to(BF)        # exact: a power of two
        for base in (0, N):                                                                    # among the gate rows and among the up rows
            src[base, 5] = 1.5                                                                 # one outlier in block 0
            zr, zb = (base, nb - 1) if nb > 1 else (base + 1, 0)
            src[zr, zb * BLOCK:(zb + 1) * BLOCK] = 0                                           # an all-zero block
        self.bits, self.src = bits, src
        self.w, self.scale_bytes = quantize64(src, bits)


GEMV_K = (32, 64, 1024, 1056, 2048, 2080, 4096, 4128, 8192, 18944)
ROWS16_K = (32, 64, 96, 160, 288, 4640, 18944)
# name -> (rows, largest N, K or None (gemv_k_limit of the name's rows), x scale); N stays small where K is long
GEMV_SETS = {f"wq-gemv-K{K}": (4, 1003 if K <= 4128 else 9, K, 1.0) for K in GEMV_K}
GEMV_SETS.update({f"wq-gemv-eps-K{K}": (4, 9, K, 2.0 ** -10) for K in (2048, 4096)})
GEMV_SETS.update({f"wq-gemv-lds-M{m}": (m, 9, None, 1.0) for m in (1, 2, 3, 4)})
ROWS16_SETS = {f"wq-rows16-K{K}": (16, 1003 if K <= 4640 else 24, K, 1.0) for K in ROWS16_K}
ROWS16_SETS["wq-rows16-eps-K160"] = (16, 24, 160, 2.0 ** -10)
SETS = dict(**GEMV_SETS, **ROWS16_SETS)
GEMV_N, GEMV_N_SILU, GEMV_M = L.GEMV_N, L.GEMV_N_SILU, L.GEMV_M
ROWS16_N, ROWS16_M = L.ROWS16_N, L.ROWS16_M
CASES = [(name, bits) for name in sorted(SETS) for bits in BITS]


def shape(name, bits):
    """(rows, largest N, K, x scale) of a set at a width"""
    M, N, K, xscale = SETS[name]
    return M, N, (gemv_k_limit(M, bits) if K is None else K), xscale


@functools.lru_cache(maxsize=None)
def operands(name, bits):
    M, N, K, xscale = shape(name, bits)
    return Operands(name, bits, M, N, K, seed=sorted(SETS).index(name), xscale=xscale)


def forms(name, bits):
    K = shape(name, bits)[2]
    if name.startswith("wq-gemv"):
        return (NONE, HF) if K <= GEMV_K_NORM_LIMIT else (NONE,)
    return (NONE, STAGED)


def has_intervals(name, bits):
    """False for the one set whose K lies beyond what U is derived for (one row at the LDS limit): probes and refusals only"""
    K = shape(name, bits)[2]
    return gemv_interval_ok(K, bits) if name.startswith("wq-gemv") else rows16_depth(K) <= DEPTH_LIMIT


# ------------------------------------------------------------------------------------------------------------------ probe matrices
def probe_matrix(bits, n, K, seed=0):
    """src [n,K] bf16 for the column probes.  Block (r, b) is randn times 2^s with s = (5 r + 3 b) % 61 - 30, so the scale byte varies along K
    and along N over 2^60.  Row r carries one special block, kind r % 4 at block (r // 4) % (K / 32):
      0  magnitudes around 2^-124: e is clamped from below          1  bf16 subnormals k 2^-133, k = 1 .. 127
      2  the largest finite bf16, both signs, and values around 2^125: e is clamped from above and the maxima saturate
      3  amax on the threshold of the scale rule: exactly elem_max's mantissa (1.75 / 1.5) times 2^10, where amax * 2^-e == elem_max, in
         rows with even r // 4, and the next bf16 above it, where e is one larger, in the others"""
    g = torch.Generator().manual_seed(1000 * K + 10 * n + bits + seed)
    nb = K // BLOCK
    r, b = torch.arange(n).unsqueeze(1), torch.arange(nb).unsqueeze(0)
    s = (5 * r + 3 * b) % 61 - 30
    src = (torch.randn(n, K, generator=g).to(BF).float() * pow2(s).float().repeat_interleave(BLOCK, dim=1)).to(BF)
    for row in range(n):
        kind, k0 = row % 4, (row // 4) % nb * BLOCK
        sign = torch.randint(0, 2, (BLOCK,), generator=g).float() * 2 - 1
        if kind == 0:
            v = (1 + torch.randint(0, 128, (BLOCK,), generator=g).float() / 128) * 2.0 ** -124 * sign
        elif kind == 1:
            v = torch.randint(1, 128, (BLOCK,), generator=g).double() * 2.0 ** -133 * sign.double()
            v[3] = 2.0 ** -127                 # the tie between 0 and 2^-126
            v[4] = 3 * 2.0 ** -128             # above the tie
        elif kind == 2:
            v = (1 + torch.randint(0, 128, (BLOCK,), generator=g).double() / 128) * 2.0 ** 125 * sign.double()
            v[0], v[31], v[7] = BF16_MAX, -BF16_MAX, 1.75 * 2.0 ** 127
        else:
            v = (1 + torch.randint(0, 128, (BLOCK,), generator=g).float() / 128) * 2.0 ** 8 * sign
            v[9] = (ELEM_MAX[bits] / 2.0 ** math.frexp(ELEM_MAX[bits])[1] * 2 + (2.0 ** -7 if (row // 4) % 2 else 0.0)) * 2.0 ** 10
        blk = v.to(F64).to(BF)
        assert torch.equal(blk.to(F64), v.to(F64))
        src[row, k0:k0 + BLOCK] = blk
    return src


def probe_expected(w, ks, cs):
    """linear_reference.probe_expected as the sum a kernel forms: c W[n, k] added to a +0 accumulator (a zero weight gives +0 whatever the
    sign of c); c W beyond the largest bf16 is inf, below the smallest normal a bf16 subnormal"""
    return (L.probe_expected(w, ks, cs).float() + 0.0).to(BF)
