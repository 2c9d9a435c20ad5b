"""What the intervals of tests/linear_reference.py let through and what not, on the very operand sets the GPU test runs.

(a) Two f32 evaluations of every case lie inside every interval: torch's f32 matmul plus the epilogue, and 32-term partial sums added in
    order, split into 1 / 2 / 4 / 8 slices that are then added in order, both with the norm, the row scale and the epilogue chain in f32.
    Their largest |err| / e is printed (-s): e has room by construction.
(b) Sixteen mistakes a kernel of this kind can make each leave at least one interval of at least one case: products lost or doubled, a K
    slice dropped, a bias / residual / weight row / row scale taken from a neighbour, a rounding misplaced, the two norm forms swapped,
    eps omitted, the mean over the row pitch, an output row written past N.
And the check is not vacuous: at K = 96 more than half of the output elements are pinned bit for bit (lo == hi)."""
import pytest
import torch
import torch.nn.functional as F

from tests import linear_reference as R

BF = R.BF


def rb(t):
    return t.to(BF).float()


# ------------------------------------------------------------------------------------------------------------------ (a) f32 evaluations
def f32_input(o, form):
    """xe (f32 holding bf16 values), r [M,1] f32"""
    x = o.x.float()
    if form == R.NONE:
        return x, torch.ones(o.M, 1)
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + o.eps)
    if form == R.STAGED:
        return rb(x * o.norm_w.float()), rstd
    return rb(o.norm_w.float() * rb(x * rstd)), torch.ones(o.M, 1)


def acc_sliced(xe, wf, slices):
    """32-term partial sums added in order within each of `slices` K slices, the slices then added in order"""
    K = xe.shape[1]
    bounds = list(range(0, K, 32))
    per = (len(bounds) + slices - 1) // slices
    total = None
    for s in range(slices):
        a = torch.zeros(xe.shape[0], wf.shape[0])
        for k0 in bounds[s * per:(s + 1) * per]:
            a = a + xe[:, k0:k0 + 32] @ wf[:, k0:k0 + 32].t()
        total = a if total is None else total + a
    return total


def f32_epilogue(v, epi, res, N):
    if epi == R.PLAIN:
        return rb(v[:, :N])
    if epi == R.RESIDUAL:
        return rb(res.float() + rb(v[:, :N]))
    return rb(rb(F.silu(rb(v[:, :N]))) * rb(v[:, N:]))


@pytest.mark.parametrize("name", sorted(R.SETS))
def test_f32_evaluations_lie_inside_every_interval(name):
    o = R.operands(name)
    wf = o.w.float()
    worst = 0.0
    for form in R.forms(name):
        xe, r = f32_input(o, form)
        accs = [("matmul", xe @ wf.t())] + [(f"sliced{s}", acc_sliced(xe, wf, s)) for s in (1, 2, 4, 8)]
        for use_bias in (False, True):
            lin, e = o.linear(form, use_bias)
            for how, acc in accs:
                v = acc * r + (o.bias if use_bias else 0.0)
                ratio = ((v.double() - lin).abs() / e.clamp_min(1e-300))[e > 0]
                worst = max(worst, float(ratio.max()) if ratio.numel() else 0.0)
                for epi in R.EPIS:
                    lo, hi, mid = o.bounds(form, use_bias, epi)
                    outside, pos = R.check(f32_epilogue(v, epi, o.res, o.N), lo, hi, mid)
                    assert outside == 0 and pos <= 1.0, (name, form, use_bias, how, epi, outside, pos)
    print(f"\n{name}: largest f32 |err| / e = {worst:.2e}")
    assert worst < 0.25, (name, worst)         # the measured figure is ~1e-3: e is far from tight for an honest f32 evaluation


# ------------------------------------------------------------------------------------------------------------------ (b) mistakes
def model(o, form, use_bias, epi, mut=None):
    """An exact (float64) kernel of the contract with one mistake `mut` built in; returns the output [M,N] (float64 holding bf16 values)."""
    N, K = o.N, o.K
    wd = o.w.double()
    xform = {R.HF: R.STAGED, R.STAGED: R.HF}.get(form, form) if mut == "forms_swapped" else form
    xe, r, _ = R.effective_input(o.x, o.norm_w, 0.0 if mut == "eps_omitted" else o.eps, xform)
    if form != R.NONE and mut in ("mean_over_ldx", "rstd_other_row"):
        rs = R.rstd64(o.x, o.eps, denom=K + 8 if mut == "mean_over_ldx" else None)
        if mut == "rstd_other_row":
            rs = rs.roll(-1, 0)
        if form == R.STAGED:
            r = rs
        else:
            xe = R.bf16r(o.norm_w.double() * R.bf16r(o.x.double() * rs))
    acc = xe @ wd.t()
    part = lambda k0, k1: xe[:, k0:k1] @ wd[:, k0:k1].t()
    mid32 = (K // 64) * 32
    if mut == "lost_first":
        acc = acc - part(0, 1)
    elif mut == "lost_last":
        acc = acc - part(K - 1, K)
    elif mut == "lost_at_32":
        acc = acc - part(mid32, mid32 + 1)
    elif mut == "step_doubled":
        acc = acc + part(mid32, mid32 + 32)
    elif mut == "slice_dropped":
        steps = (K + 31) // 32
        per = (steps + 7) // 8
        last = (steps - 1) // per
        acc = acc - part(last * per * 32, K)
    if mut == "up_row_padded":        # the up rows looked up behind a gate block padded to whole 16-row tiles
        idx = torch.arange(N) + (N + 15) // 16 * 16
        acc = torch.cat((acc[:, :N], acc[:, idx.clamp_max(2 * N - 1)]), dim=1)
    b = o.bias.double() if use_bias else torch.zeros(2 * N, dtype=torch.float64)
    if mut == "bias_next_column":
        b = b.roll(-1)
    elif mut == "gate_bias_for_up":
        b = torch.cat((b[:N], b[:N]))
    v = r * acc + b
    res = o.res.double().roll(-1, 0) if mut == "residual_next_row" else o.res.double()
    if epi == R.PLAIN:
        return R.bf16r(v[:, :N])
    if epi == R.RESIDUAL:
        return R.bf16r(res + (v[:, :N] if mut == "single_rounding" else R.bf16r(v[:, :N])))
    g = v[:, :N] if mut == "silu_unrounded_gate" else R.bf16r(v[:, :N])
    return R.bf16r(R.bf16r(R.silu64(g)) * R.bf16r(v[:, N:]))


# mistake -> the (form kind, bias, epilogue) it shows in; "norm" = the set's norm form
MISTAKES = {
    "lost_first": ("none", False, R.PLAIN), "lost_last": ("none", False, R.PLAIN), "lost_at_32": ("none", False, R.PLAIN),
    "step_doubled": ("none", False, R.RESIDUAL), "slice_dropped": ("none", True, R.SILU_MUL),
    "bias_next_column": ("none", True, R.PLAIN), "gate_bias_for_up": ("none", True, R.SILU_MUL), "up_row_padded": ("none", False, R.SILU_MUL),
    "residual_next_row": ("none", False, R.RESIDUAL), "single_rounding": ("none", True, R.RESIDUAL),
    "silu_unrounded_gate": ("none", True, R.SILU_MUL), "forms_swapped": ("norm", False, R.PLAIN), "eps_omitted": ("norm", True, R.PLAIN),
    "mean_over_ldx": ("norm", False, R.RESIDUAL), "rstd_other_row": ("norm", True, R.SILU_MUL),
}
MISTAKE_SETS = ("gemv-K24", "gemv-K2048", "gemv-eps-K2048", "rows16-K160", "rows16-eps-K160", "rows64-K96", "rows64-eps-K512")


def _norm_form(name):
    return [f for f in R.forms(name) if f != R.NONE]


@pytest.mark.parametrize("mistake", sorted(MISTAKES))
def test_every_mistake_leaves_an_interval(mistake):
    kind, use_bias, epi = MISTAKES[mistake]
    caught = {}
    for name in MISTAKE_SETS:
        forms = _norm_form(name) if kind == "norm" else [R.NONE]
        o = R.operands(name)
        for form in forms:
            lo, hi, mid = o.bounds(form, use_bias, epi)
            clean, _ = R.check(model(o, form, use_bias, epi), lo, hi, mid)
            assert clean == 0, (name, form, "the exact kernel itself leaves an interval")
            caught[(name, form)] = R.check(model(o, form, use_bias, epi, mistake), lo, hi, mid)[0]
    print(f"\n{mistake}: elements outside, per case: {caught}")
    assert max(caught.values()) > 0, (mistake, caught)
    if mistake == "eps_omitted":              # what the eps cases are for
        assert all(n > 0 for (name, _), n in caught.items() if "-eps-" in name), caught


def test_an_output_row_written_past_n_breaks_the_sentinel():
    """output row N - 1 duplicated into a clamped row: the interval check cannot see a write outside [M, N], the sentinel does"""
    o = R.operands("rows16-K160")
    M, N = 5, 17
    lo, hi, mid = (t[:M, :N] for t in o.bounds(R.NONE, False, R.PLAIN))
    buf = R.out_buffer(M, N, N + 40)
    buf[:M, :N] = mid.to(BF)
    assert R.sentinel_damage(buf, M, N) == 0 and R.check(buf[:M, :N], lo, hi, mid) == (0, 0.0)
    buf[:M, N] = buf[:M, N - 1]
    assert R.sentinel_damage(buf, M, N) == M
    ssq = torch.full((M + 1, 3), R.SENTINEL_F32)
    assert R.sentinel_damage(ssq, M, 2) == 0
    ssq[M, 0] = 1.0
    assert R.sentinel_damage(ssq, M, 2) == 1


@pytest.mark.parametrize("name", ["gemv-K20488", "rows16-K18944", "rows64-K1056"])
def test_column_probes_pin_every_product(name):
    """x[m] = c e_k: the plain interval without bias collapses to bf16(c W[:, k]); a lost product (0) and a doubled one (2 w) leave it.  At
    K = 18944 one product is 2^-14 of the sum of magnitudes on average -- random data cannot see it, the probes do."""
    o = R.operands(name)
    M = min(o.M, 16)
    launches = R.probe_launches(o.K, M)
    covered = {k for ks, _ in launches for k in ks}
    assert covered == set(R.probe_columns(o.K))
    if o.K > 1088:
        assert {0, 7, 8, 31, 32, 511, o.K - 512, o.K - 8, o.K - 1} <= covered and all(k % 32 in (0, 31) or k % 8 in (0, 7) for k in covered)
    w = o.w[:o.N]
    for ks, cs in launches[:3] + launches[-3:]:
        x = R.probe_x(o.K, ks, cs)
        want = R.probe_expected(w, ks, cs)
        lin, e = R.linear64(x, w, None, o.norm_w, o.eps, R.NONE)
        lo, hi, mid = R.interval(lin, e, R.PLAIN)
        assert torch.equal(lo, hi) and torch.equal(lo, want.float())
        assert R.check(want, lo, hi, mid) == (0, 0.0)
        lost, _ = R.check(torch.zeros_like(want), lo, hi, mid)
        doubled, _ = R.check((2 * want.float()).to(BF), lo, hi, mid)
        nonzero = int((want.float() != 0).sum())
        assert lost == nonzero == doubled and nonzero > 0.99 * want.numel()
    # ... while on the random rows of the same set a lost product stays inside most intervals
    if o.K >= 18944:
        lo, hi, mid = o.bounds(R.NONE, False, R.PLAIN)
        outside, _ = R.check(model(o, R.NONE, False, R.PLAIN, "lost_last"), lo, hi, mid)
        assert outside < 0.2 * lo.numel()


def test_the_intervals_pin_most_elements_bit_for_bit():
    """K = 96: at least half of the output elements have lo == hi.  With a bias (the setting of today's tests) every epilogue and norm form
    stands above one half on its own, measured 80-95 %; so do the plain and residual epilogues without one (66 %, 93 %).  SiLU*mul without a bias
    is the product of two factors that are each 66 % pinned (sums of 96 products cancelling to ~0.2 with nothing added), 48 %: asserted above
    the product of its factors' shares, and the case as a whole above one half."""
    o = R.operands("rows64-K96")
    pinned, total = 0, 0
    for form in R.forms("rows64-K96"):
        for use_bias in (False, True):
            share = {}
            for epi in R.EPIS:
                lo, hi, _ = o.bounds(form, use_bias, epi)
                share[epi] = float((lo == hi).float().mean())
                pinned, total = pinned + int((lo == hi).sum()), total + lo.numel()
                print(f"\nrows64-K96 {form} bias={use_bias} epi={epi}: {100 * share[epi]:.1f} % pinned")
            assert share[R.PLAIN] >= 0.5 and share[R.RESIDUAL] >= 0.5, (form, use_bias, share)
            if use_bias:
                assert share[R.SILU_MUL] >= 0.5, (form, use_bias, share)
            else:
                lin, e = o.linear(form, False)
                both = (R.bf16r(lin - e) == R.bf16r(lin + e))
                assert share[R.SILU_MUL] >= float((both[:, :o.N] & both[:, o.N:]).double().mean()) - 0.01, (form, share)
    assert pinned >= 0.5 * total, (pinned, total)


def test_reference_pieces():
    """the building blocks against closed forms"""
    assert abs(R.SILU_MIN - (-0.27846454276107)) < 1e-12
    x = torch.tensor([[3.0, 4.0]]).to(BF)
    assert abs(float(R.rstd64(x, 0.0)) - (12.5 ** -0.5)) < 1e-15
    assert abs(float(R.rstd64(x, 0.0, denom=4)) - (6.25 ** -0.5)) < 1e-15
    t = torch.tensor([1.0 + 2.0 ** -9, 1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 3 * 2.0 ** -9], dtype=torch.float64)
    assert R.bf16r(t).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -7]          # through f32: 2^-30 above a tie is lost first, the tie then goes to even
    assert R.rows16_lds_bytes(512, 8, R.SILU_MUL) > R.LDS_LIMIT >= R.rows16_lds_bytes(512, 8, R.PLAIN)
    assert len(R.ROWS16_GEOMETRIES) == 22
    # staged and HF forms describe the same quantity up to one bf16 rounding of the input
    o = R.operands("rows16-K160")
    a, _ = R.linear64(o.x, o.w, None, o.norm_w, o.eps, R.HF)
    b, _ = R.linear64(o.x, o.w, None, o.norm_w, o.eps, R.STAGED)
    assert float((a - b).abs().max()) < 2.0 ** -6 * float(a.abs().max()) and float((a - b).abs().max()) > 0
