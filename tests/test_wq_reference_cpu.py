"""What tests/wq_reference.py holds and what its intervals let through, on the very cases tests/test_wq_reference_gpu.py runs.

The quantiser: quantize64 (float64, from the contract) equals llm_quant.mx_round on every operand set and probe matrix, values and scale
bytes; the probe matrices hold what their docstring says (both clamp ends, subnormals, saturating maxima, the threshold of the scale rule).
(a) Two f32 evaluations of every case lie inside every interval: the GEMV's own order (chunk c of 16 / 32 elements on lane c % 64, one chain
    per lane, a tree over the 64 lanes) and 32-wide blocks added in order inside 1 / 2 / 4 / 8 K slices that are then added in order.
    Largest |err| / e over all cases: 2.6e-3 (printed with -s).
(b) Every seeded mistake of MISTAKES -- what a kernel that expands packed codes can get wrong -- leaves at least one interval or probe.
The limits of the header's LDS rule are computed from the rule, and the derivation of U covers every set that has intervals."""
import pytest
import torch

from llamole_amd.llm_quant import mx_round
from tests import linear_reference as L
from tests import wq_reference as R
from tests.test_decode_linear_reference_cpu import acc_sliced, f32_epilogue, f32_input

BF, F64 = R.BF, R.F64


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------------------------ the quantiser
def _same_as_mx_round(src, bits):
    w, sb = R.quantize64(src, bits)
    dq, sb2 = mx_round(src, bits)
    assert torch.equal(_bits(w), _bits(dq.to(BF))) and torch.equal(dq.to(BF).float(), dq), "values"
    assert torch.equal(sb, sb2), "scale bytes"
    return w, sb


@pytest.mark.parametrize("name,bits", R.CASES)
def test_quantize64_equals_mx_round_on_every_set(name, bits):
    o = R.operands(name, bits)
    w, sb = _same_as_mx_round(o.src, bits)
    assert torch.equal(_bits(w), _bits(o.w)) and torch.equal(sb, o.scale_bytes)
    assert len(sb.unique()) >= 7 or sb.numel() < 64                             # per-block powers of two 2^-3 .. 2^3 around 0.02 randn
    blocks = o.w.float().reshape(2 * o.N, o.K // 32, 32)
    assert bool((blocks == 0).all(-1).any()), "no all-zero block"
    assert float(o.w[0, 5]) == 1.5 and float(o.w[o.N, 5]) == 1.5, "the outliers"
    # every block contributes inside the interval width: none lies more than 2^10 below the largest of its row (the outlier's)
    amax = blocks.abs().amax(-1)
    assert float((amax.amax(-1, keepdim=True) / amax.clamp_min(1e-30))[amax > 0].max()) <= 2.0 ** 10


@pytest.mark.parametrize("bits", R.BITS)
@pytest.mark.parametrize("n,K", [(9, 32), (9, 64), (17, 288), (9, 1056), (9, 4128), (17, 18944)])
def test_probe_matrices(bits, n, K):
    src = R.probe_matrix(bits, n, K)
    w, sb = _same_as_mx_round(src, bits)
    lo, hi = R.E_CLAMP[bits]
    e = sb.to(torch.int32) - 127
    assert int(e.min()) == lo and int(e.max()) == hi, "both clamp ends"
    assert all(len(sb[:, b].unique()) > 1 for b in range(K // 32)), "scale bytes vary along N"
    assert K == 32 or all(len(sb[r].unique()) > 1 for r in range(n)), "scale bytes vary along K"
    wf = w.to(F64)
    assert bool(torch.isfinite(wf).all()) and bool(((wf == 0) | (wf.abs() >= 2.0 ** -126)).all()), "every dequantised value is 0 or a normal bf16"
    for row in range(n):
        k0 = (row // 4) % (K // 32) * 32
        s, d = src[row, k0:k0 + 32].to(F64), wf[row, k0:k0 + 32]
        if row % 4 == 0:
            assert int(e[row, k0 // 32]) == lo and bool(((d / 2.0 ** -126) == (d / 2.0 ** -126).round()).all()) and bool((d != 0).all())
        elif row % 4 == 1:       # subnormals: 0 or +-2^-126; the tie 2^-127 goes to 0, 3 * 2^-128 to 2^-126
            assert bool((s.abs() < 2.0 ** -126).all()) and bool(((d == 0) | (d.abs() == 2.0 ** -126)).all())
            assert float(d[3]) == 0.0 and float(d[4]) == 2.0 ** -126 and bool((d.abs() == 2.0 ** -126).any())
        elif row % 4 == 2:       # the clamp makes the maxima saturate at elem_max * 2^hi
            top = R.ELEM_MAX[bits] * 2.0 ** hi
            assert int(e[row, k0 // 32]) == hi and float(d[0]) == top and float(d[31]) == -top and float(s[0]) == R.BF16_MAX > top
            assert float(d[7]) == (1.75 * 2.0 ** 127 if bits == 8 else top)
        else:                    # amax * 2^-e == elem_max exactly, and one bf16 step above it: e + 1
            want = 10 - (8 if bits == 8 else 2) + (row // 4) % 2
            assert int(e[row, k0 // 32]) == want, (row, int(e[row, k0 // 32]), want)
            assert (float(d[9]) == float(s[9])) == ((row // 4) % 2 == 0)
    # a probe is exact whatever the magnitudes, and a zero weight gives +0
    ks, cs = [0, K - 1, 5, 31], [1.0, -2.0, 0.5, -1.0]
    want = R.probe_expected(w, ks, cs)
    exact = (wf[:, ks] * torch.tensor(cs, dtype=F64)).t()
    fin = exact.abs() <= R.BF16_MAX
    assert torch.equal(want.to(F64)[fin], exact[fin]) and bool(torch.isinf(want.float()[~fin]).all())
    assert not bool(((want.float() == 0) & (_bits(want) != 0)).any())


def test_grid_and_limits():
    """the element grids against torch's own E4M3 and the OCP E2M1 list; the LDS rule's limits computed from the rule"""
    g8 = R.grid(8)
    codes = torch.arange(127, dtype=torch.uint8)
    assert torch.equal(g8, codes.view(torch.float8_e4m3fn).to(F64)) and len(g8) == 127 and float(g8[-1]) == 448.0
    assert R.grid(4).tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    t = torch.zeros(1, 32, dtype=BF)
    t[0, :9] = torch.tensor([6.0, 2.5, 5.0, -3.5, 0.25, 0.75, 1.25, 1.75, -2.5]).to(BF)
    assert R.quantize64(t, 4)[0][0, :9].tolist() == [6.0, 2.0, 4.0, -4.0, 0.0, 1.0, 1.0, 2.0, -2.0]      # ties to the even code
    t[0, :5] = torch.tensor([448.0, 272.0, 304.0, 1.0625, 1.1875]).to(BF)
    assert R.quantize64(t, 8)[0][0, :5].tolist() == [448.0, 256.0, 320.0, 1.0, 1.25]
    for bits in R.BITS:
        for M in R.GEMV_M:
            K = R.gemv_k_limit(M, bits)
            assert K % 32 == 0 and R.gemv_lds_bytes(M, K, bits) <= R.LDS_LIMIT < R.gemv_lds_bytes(M, K + 32, bits)
            assert M == 4 or R.gemv_lds_bytes(M + 1, K, bits) > R.LDS_LIMIT      # the limits differ per M
    assert R.gemv_lds_bytes(4, 20480, 8) > R.LDS_LIMIT >= R.gemv_lds_bytes(3, 20480, 8)      # the issue's example
    assert [R.gemv_k_limit(M, 8) for M in R.GEMV_M] == [80896, 39936, 26624, 19456]
    assert [R.gemv_k_limit(M, 4) for M in R.GEMV_M] == [79872, 38912, 26624, 18432]
    # U = 2^-14 covers 640 additions; the only cases beyond are one row at its LDS limit, which therefore have no interval
    assert R.DEPTH_LIMIT * 2.0 ** -24 < L.U
    without = [(n, b) for n, b in R.CASES if not R.has_intervals(n, b)]
    assert without == [("wq-gemv-lds-M1", 8), ("wq-gemv-lds-M1", 4)]
    assert R.gemv_depth(39936, 8) == 631 and R.gemv_depth(38912, 4) == 615 and R.rows16_depth(18944) == 632
    assert len(R.WQ_GEOMETRIES) == 15
    assert R.rows16_wq_lds_bytes(8, 256, 8, R.SILU_MUL) > R.LDS_LIMIT >= R.rows16_wq_lds_bytes(8, 256, 8, R.PLAIN)
    assert R.rows16_wq_lds_bytes(4, 128, 8, R.SILU_MUL) > R.LDS_LIMIT >= R.rows16_wq_lds_bytes(4, 128, 4, R.SILU_MUL)


# ------------------------------------------------------------------------------------------------------------------ (a) f32 evaluations
def acc_gemv_order(xe, wf, bits):
    """chunk c (16 B of codes) on lane c % 64, one f32 chain per lane over its chunks' elements in order, then a tree over the lanes"""
    epc = 128 // bits
    (M, K), n = xe.shape, wf.shape[0]
    steps = -(-K // (64 * epc))
    xp, wp = torch.zeros(M, steps * 64 * epc), torch.zeros(n, steps * 64 * epc)
    xp[:, :K], wp[:, :K] = xe, wf
    xp, wp = xp.view(M, 1, steps, 64, epc), wp.view(1, n, steps, 64, epc)
    acc = torch.zeros(M, n, 64)
    for s in range(steps):
        for t in range(epc):
            acc = acc + xp[:, :, s, :, t] * wp[:, :, s, :, t]
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc[..., :off] + acc[..., off:2 * off]
    return acc[..., 0]


@pytest.mark.parametrize("name,bits", [c for c in R.CASES if R.has_intervals(*c)])
def test_f32_evaluations_lie_inside_every_interval(name, bits):
    o = R.operands(name, bits)
    wf = o.w.float()
    worst = 0.0
    for form in R.forms(name, bits):
        xe, r = f32_input(o, form)
        accs = [("gemv order", acc_gemv_order(xe, wf, bits))] + [(f"sliced{s}", acc_sliced(xe, wf, s)) for s in (1, 2, 4, 8)]
        for use_bias in (False, True):
            lin, e = o.linear(form, use_bias)
            for how, acc in accs:
                v = acc * r + (o.bias if use_bias else 0.0)
                ratio = ((v.double() - lin).abs() / e.clamp_min(1e-300))[e > 0]
                worst = max(worst, float(ratio.max()) if ratio.numel() else 0.0)
                for epi in R.EPIS:
                    lo, hi, mid = o.bounds(form, use_bias, epi)
                    outside, pos = L.check(f32_epilogue(v, epi, o.res, o.N), lo, hi, mid)
                    assert outside == 0 and pos <= 1.0, (name, bits, form, use_bias, how, epi, outside, pos)
    print(f"\n{name} at {bits} bits: largest f32 |err| / e = {worst:.2e}")
    assert worst < 0.25, (name, bits, worst)


# ------------------------------------------------------------------------------------------------------------------ (b) mistakes
def model(o, form, use_bias, epi, mut=None):
    """An exact (float64) kernel of the contract on the MX weight of `o` with one mistake `mut` built in; [M,N] float64 holding bf16 values."""
    N, K, bits = o.N, o.K, o.bits
    nb, epc, pad = K // 32, 128 // bits, 8192 // bits
    wd = o.w.double()
    sb = o.scale_bytes.to(torch.int64)
    other = {"scale_block_next": sb.roll(-1, 1), "scale_block_prev": sb.roll(1, 1), "scale_row_next": sb.roll(-1, 0), "scale_row_prev": sb.roll(1, 0)}
    if mut in other:             # the codes of a block under the scale byte of a neighbour
        wd = wd * R.pow2(other[mut] - sb).repeat_interleave(32, dim=1)
    elif mut == "nibbles_swapped":
        wd = wd.view(2 * N, K // 2, 2).flip(-1).reshape(2 * N, K)
    elif mut == "dword_halves_swapped":
        wd = wd.view(2 * N, K // 4, 2, 2).flip(-2).reshape(2 * N, K)
    x = o.x
    if mut == "x_beyond_4096_zero" and form != R.NONE:
        x = x.clone()
        x[:, 4096:] = 0
    xform = {R.HF: R.STAGED, R.STAGED: R.HF}.get(form, form) if mut == "forms_swapped" else form
    xe, r, _ = L.effective_input(x, o.norm_w, o.eps, xform)
    if mut == "mean_over_padded_k" and form != R.NONE:
        rs = L.rstd64(o.x, o.eps, denom=(K + pad - 1) // pad * pad)
        if form == R.STAGED:
            r = rs
        else:
            xe = L.bf16r(o.norm_w.double() * L.bf16r(o.x.double() * rs))
    acc = xe @ wd.t()
    part = lambda k0, k1: xe[:, k0:k1] @ wd[:, k0:k1].t()
    per = (nb + 3) // 4          # 32-blocks per slice of a four-way K split
    if mut == "last_chunk_dropped":
        acc = acc - part(K - epc, K)
    elif mut == "slice_last_block_dropped":
        acc = acc - part(per * 32 - 32, per * 32)
    elif mut == "slice_doubled":
        acc = acc + part(0, per * 32)
    if mut == "up_row_shifted":
        acc = torch.cat((acc[:, :N], acc[:, N - 1:2 * N - 1]), dim=1)
    b = o.bias.double() if use_bias else torch.zeros(2 * N, dtype=F64)
    if mut == "up_bias_shifted":
        b = torch.cat((b[:N], b[N - 1:2 * N - 1]))
    late = mut == "bias_after_rounding"
    v = r * acc + (0 if late else b)
    rnd = (lambda t: L.bf16r(L.bf16r(t) + b[:t.shape[1]])) if late else L.bf16r
    res = o.res.double()
    res = res.roll(-1, 0) if mut == "residual_next_row" else res.roll(1, 0) if mut == "residual_prev_row" else res
    if epi == R.PLAIN:
        return rnd(v[:, :N])
    if epi == R.RESIDUAL:
        return L.bf16r(res + rnd(v[:, :N]))
    return L.bf16r(L.bf16r(L.silu64(L.bf16r(v[:, :N]))) * L.bf16r(v[:, N:]))


# mistake -> (form kind, bias, epilogue, widths); "norm" = the set's norm form
MISTAKES = {
    "scale_block_next": ("none", False, R.PLAIN, R.BITS), "scale_block_prev": ("none", True, R.RESIDUAL, R.BITS),
    "scale_row_next": ("none", False, R.SILU_MUL, R.BITS), "scale_row_prev": ("none", False, R.PLAIN, R.BITS),
    "nibbles_swapped": ("none", False, R.PLAIN, (4,)), "dword_halves_swapped": ("none", False, R.PLAIN, (8,)),
    "last_chunk_dropped": ("none", False, R.PLAIN, R.BITS), "slice_last_block_dropped": ("none", True, R.SILU_MUL, R.BITS),
    "x_beyond_4096_zero": ("norm", False, R.PLAIN, R.BITS), "mean_over_padded_k": ("norm", False, R.RESIDUAL, R.BITS),
    "forms_swapped": ("norm", False, R.PLAIN, R.BITS), "up_row_shifted": ("none", False, R.SILU_MUL, R.BITS),
    "up_bias_shifted": ("none", True, R.SILU_MUL, R.BITS), "residual_next_row": ("none", False, R.RESIDUAL, R.BITS),
    "residual_prev_row": ("none", True, R.RESIDUAL, R.BITS), "bias_after_rounding": ("none", True, R.PLAIN, R.BITS),
    "slice_doubled": ("none", False, R.RESIDUAL, R.BITS),
}
MISTAKE_SETS = ("wq-gemv-K64", "wq-gemv-K1056", "wq-gemv-K4128", "wq-gemv-eps-K2048", "wq-rows16-K160", "wq-rows16-K288", "wq-rows16-eps-K160")


@pytest.mark.parametrize("mistake,bits", [(m, b) for m in sorted(MISTAKES) for b in MISTAKES[m][3]])
def test_every_mistake_leaves_an_interval(mistake, bits):
    kind, use_bias, epi, _ = MISTAKES[mistake]
    caught = {}
    for name in MISTAKE_SETS:
        o = R.operands(name, bits)
        for form in ([f for f in R.forms(name, bits) if f != R.NONE] if kind == "norm" else [R.NONE]):
            lo, hi, mid = o.bounds(form, use_bias, epi)
            assert L.check(model(o, form, use_bias, epi), lo, hi, mid)[0] == 0, (name, form, "the exact kernel itself leaves an interval")
            caught[(name, form)] = L.check(model(o, form, use_bias, epi, mistake), lo, hi, mid)[0]
    print(f"\n{mistake} at {bits} bits: elements outside, per case: {caught}")
    assert max(caught.values()) > 0, (mistake, bits, caught)
    if mistake == "x_beyond_4096_zero":       # what K = 4128 under the norm is for
        assert caught[("wq-gemv-K4128", R.HF)] > 0, caught


@pytest.mark.parametrize("mistake,bits", [(m, b) for m in ("scale_block_next", "scale_row_prev", "nibbles_swapped", "dword_halves_swapped",
                                                           "last_chunk_dropped") for b in MISTAKES[m][3]])
def test_weight_mistakes_leave_a_probe(mistake, bits):
    """the same weight-side mistakes on the probe matrices: bf16(c W'[:, k]) differs from bf16(c W[:, k]) in some probed column (a dropped
    chunk gives 0 there)"""
    n, K = 9, 1056
    w, sb = R.quantize64(R.probe_matrix(bits, n, K), bits)
    wd = w.double()
    sbl = sb.to(torch.int64)
    if mistake == "scale_block_next":
        bad = wd * R.pow2(sbl.roll(-1, 1) - sbl).repeat_interleave(32, dim=1)
    elif mistake == "scale_row_prev":
        bad = wd * R.pow2(sbl.roll(1, 0) - sbl).repeat_interleave(32, dim=1)
    elif mistake == "nibbles_swapped":
        bad = wd.view(n, K // 2, 2).flip(-1).reshape(n, K)
    elif mistake == "dword_halves_swapped":
        bad = wd.view(n, K // 4, 2, 2).flip(-2).reshape(n, K)
    else:
        bad = wd.clone()
        bad[:, K - 128 // bits:] = 0
    differ = 0
    for ks, cs in L.probe_launches(K, 4):
        c = torch.tensor(cs, dtype=F64)
        differ += int((L.bf16r(bad[:, ks] * c) != L.bf16r(wd[:, ks] * c)).sum())
    assert differ > 0
