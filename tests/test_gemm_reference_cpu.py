"""What the intervals of tests/gemm_reference.py let through and what not, on the very operand sets the GPU test runs (the first 260 rows of
the sets that have more: the intervals are per element).

(a) Two honest f32 evaluations of every set lie inside every interval of every epilogue, bias and output type: torch's f32 matmul, and an
    evaluation shaped like the kernels -- 32-wide chunks added in order per wave part, the wave partials added in order, the K slabs added
    in order (for the f32 sets: 16-wide chunks in k order).  Their largest |err| / e is printed (-s).
(b) Sixteen mistakes a kernel of this family can make each leave at least one interval of every set they apply to.
And the check is not vacuous: every bf16-output case has pinned elements (lo == hi)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_reference as G
from tests import linear_reference as R

ROWS = 260
F64 = torch.float64


class Case:
    def __init__(self, name):
        s = G.gemm_set(name)
        self.s, self.name, self.f32, self.K, self.N = s, name, s.f32, s.K, s.N
        self.M = min(s.M, ROWS)
        self.x, self.w, self.bias = s.x[:self.M], s.w, s.bias

    def lin_e(self, use_bias, col0=0, n=None):
        lin, e = self.s.linear(use_bias)
        n = self.N if n is None else n
        return lin[:self.M, col0:col0 + n], e[:self.M, col0:col0 + n]

    def outs(self):
        return (1,) if self.f32 else (0, 1)


def gelu_f32(v):
    """0.5f v (1 + erff(v 0.70710678f)) step by step in f32 with a correctly rounded erff (torch's CPU gelu is not one: its 1 + erf is off by
    up to nine f32 ulps at v = -2.9, more than the band allows the device)"""
    arg = v * torch.tensor(0.70710678118654752440, dtype=torch.float32)
    return (0.5 * v) * (1.0 + torch.erf(arg.double()).float())


def f32_epilogue(v, epi, out_f32):
    y = {G.NONE: lambda t: t, G.GELU: gelu_f32, G.SILU: F.silu, G.SOFTSIGN: F.softsign}[epi](v)
    return y if out_f32 else y.to(R.BF).float()


def acc_shaped(x, w, chunk, waves, slabs):
    """chunk-wide partial products added in order within each of `waves` parts of each of `slabs` K ranges, the parts then added in order,
    the slabs then added in order; all in f32"""
    K = x.shape[1]
    xf, wf = x.float(), w.float()
    total = None
    for z in range(slabs):
        k0, k1 = z * K // slabs, (z + 1) * K // slabs
        steps = list(range(k0, k1, chunk))
        per = -(-len(steps) // waves)
        slab = None
        for p in range(waves):
            a = torch.zeros(x.shape[0], w.shape[0])
            for k in steps[p * per:(p + 1) * per]:
                a = a + xf[:, k:min(k + chunk, k1)] @ wf[:, k:min(k + chunk, k1)].t()
            slab = a if slab is None else slab + a
        total = slab if total is None else total + slab
    return total


@pytest.mark.parametrize("name", sorted(G.SETS))
def test_f32_evaluations_lie_inside_every_interval(name):
    c = Case(name)
    w = c.w[:c.N]
    accs = [("matmul", c.x.float() @ w.float().t())]
    if c.f32:
        accs.append(("16-wide chunks in order", acc_shaped(c.x, w, 16, 1, 1)))
    else:
        accs += [("one accumulator", acc_shaped(c.x, w, 32, 1, 1)), ("8 wave parts", acc_shaped(c.x, w, 32, 8, 1))]
        accs += [(f"8 wave parts, {s} slabs", acc_shaped(c.x, w, 32, 8, s)) for s in (2, 16) if c.K % (64 * s) == 0]
    worst = 0.0
    for use_bias in (False, True):
        lin, e = c.lin_e(use_bias)
        for how, acc in accs:
            v = acc + (c.bias[:c.N] if use_bias else 0.0)
            ratio = ((v.double() - lin).abs() / e.clamp_min(1e-300))[e > 0]
            worst = max(worst, float(ratio.max()))
            for out_f32 in c.outs():
                for epi in G.EPIS:
                    lo, hi, mid = G.interval(lin, e, epi, out_f32)
                    outside, pos = R.check(f32_epilogue(v, epi, out_f32), lo, hi, mid)
                    assert outside == 0 and pos <= 1.0, (name, use_bias, how, epi, out_f32, outside, pos)
                    if not out_f32:
                        assert bool((lo == hi).any()), (name, use_bias, epi, "no pinned element")
    print(f"\n{name}: largest f32 |err| / e = {worst:.2e}")
    assert worst < 0.5, (name, worst)


@pytest.mark.parametrize("name", [n for n in sorted(G.SETS) if not G.SETS[n][0] and G.SETS[n][3] % 128 == 0 and G.SETS[n][3] <= 2048])
def test_f32_slabs_lie_inside_their_intervals(name):
    c = Case(name)
    for splits in (2, 16):
        if c.K % (64 * splits):
            continue
        kc = c.K // splits
        for z, (lin_z, e_z) in enumerate(c.s.slabs(splits)):
            got = acc_shaped(c.x[:, z * kc:(z + 1) * kc], c.w[:c.N, z * kc:(z + 1) * kc], 32, 8 if kc >= 256 else 1, 1)
            outside, pos = R.check(got, *G.interval(lin_z[:c.M, :c.N], e_z[:c.M, :c.N], G.NONE, 1))
            assert outside == 0, (name, splits, z, outside, pos)


# ------------------------------------------------------------------------------------------------------------------ (b) mistakes
def tanh_gelu64(v):
    return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))


def trunc_bf16(t):
    """float64 -> f32 -> bf16 by dropping the low 16 bits"""
    return (t.to(torch.float32).view(torch.int32) & -65536).view(torch.float32).to(F64)


def model(c, use_bias, epi, out_f32, mut=None):
    """An exact (float64) kernel of the contract on the whole set with one mistake built in; the output [M, N] as float64"""
    K, N = c.K, c.N
    xd, wd = c.x.double(), c.w[:N].double()
    b = c.bias[:N].double() if use_bias else torch.zeros(N, dtype=F64)
    part = lambda k0, k1: xd[:, k0:k1] @ wd[:, k0:k1].t()
    step = 16 if c.f32 else 64
    if mut == "rotation_on_A_only":
        acc = xd.roll(step, 1) @ wd.t()
    elif mut == "w_steps_swapped":
        w2 = wd.clone()
        half = step // 2
        w2[:, :half], w2[:, half:step] = wd[:, half:step], wd[:, :half]
        acc = xd @ w2.t()
    else:
        acc = xd @ wd.t()
    if mut == "last_tile_dropped":
        acc = acc - part((K - 1) // step * step, K)
    elif mut == "first_tile_dropped":
        acc = acc - part(0, step)
    elif mut == "tail_dropped":
        acc = acc - part(K // 64 * 64, K)
    if mut == "bias_next_column":
        b = b.roll(-1)
    if mut == "epilogue_per_slab":
        kc = K // 2
        v = G.epi64(part(0, kc) + b, epi) + G.epi64(part(kc, K), epi)
    else:
        v = acc + b
        if mut == "tanh_gelu":
            v = tanh_gelu64(v)
        elif mut == "silu_gelu_swapped":
            v = G.epi64(v, {G.GELU: G.SILU, G.SILU: G.GELU}[epi])
        else:
            v = G.epi64(v, epi)
    out = trunc_bf16(v) if mut == "truncation" else G.out_round(v, out_f32)
    if mut == "row_leaked":            # a clamped row index used for the store: row m - 1 lands in row m
        out = out.clone()
        out[c.M // 2] = out[c.M // 2 - 1]
    elif mut == "column_leaked":
        out = out.clone()
        out[:, N // 2] = out[:, N // 2 - 1]
    elif mut == "ldc_is_N":            # rows written N apart into an allocation read N + 40 apart
        buf = torch.full((c.M * (N + 40),), float("nan"), dtype=F64)
        buf[:c.M * N] = out.reshape(-1)
        out = buf.view(c.M, N + 40)[:, :N]
    return out


# mistake -> (the sets it applies to, the epilogues, the output types (None: all the set has))
ALL = lambda c: True
MISTAKES = {
    "last_tile_dropped": (ALL, G.EPIS, None),
    "first_tile_dropped": (ALL, G.EPIS, None),
    "tail_dropped": (lambda c: c.K % 64 != 0 and not c.f32, G.EPIS, None),
    "rotation_on_A_only": (lambda c: c.K > (16 if c.f32 else 64), G.EPIS, None),
    "w_steps_swapped": (ALL, G.EPIS, None),
    "bias_next_column": (ALL, G.EPIS, None),
    "epilogue_per_slab": (lambda c: c.K % 128 == 0, (G.GELU, G.SILU, G.SOFTSIGN), None),
    "tanh_gelu": (ALL, (G.GELU,), None),
    "silu_gelu_swapped": (ALL, (G.GELU, G.SILU), None),
    "truncation": (lambda c: not c.f32, G.EPIS, (0,)),
    "row_leaked": (lambda c: c.M >= 2, G.EPIS, None),
    "column_leaked": (lambda c: c.N >= 2, G.EPIS, None),
    "ldc_is_N": (lambda c: c.M >= 2, G.EPIS, None),
}


@pytest.mark.parametrize("name", sorted(G.SETS))
def test_mistakes_leave_the_intervals(name):
    c = Case(name)
    bounds = {}

    def outside(out, use_bias, epi, out_f32):
        key = (use_bias, epi, out_f32)
        if key not in bounds:
            bounds[key] = G.interval(*c.lin_e(use_bias), epi, out_f32)
        return R.check(out, *bounds[key])[0]

    for use_bias in (False, True):
        for epi in G.EPIS:
            for out_f32 in c.outs():
                assert outside(model(c, use_bias, epi, out_f32), use_bias, epi, out_f32) == 0, (name, "the exact model left its own interval")
    for mut, (applies, epis, outs) in MISTAKES.items():
        if not applies(c):
            continue
        for epi in epis:
            for out_f32 in (outs or c.outs()):
                if out_f32 not in c.outs():
                    continue
                n = outside(model(c, True, epi, out_f32, mut), True, epi, out_f32)
                assert n > 0, (name, mut, G.EPI_NAMES[epi], out_f32, "the mistake stays inside every interval")


@pytest.mark.parametrize("name", [n for n in sorted(G.SETS) if G.SETS[n][3] % 128 == 0 and not G.SETS[n][0]])
def test_bias_in_every_raw_slab_leaves_the_slab_intervals(name):
    c = Case(name)
    kc = c.K // 2
    for z, (lin_z, e_z) in enumerate(c.s.slabs(2)):
        exact = c.x[:, z * kc:(z + 1) * kc].double() @ c.w[:c.N, z * kc:(z + 1) * kc].double().t()
        iv = G.interval(lin_z[:c.M, :c.N], e_z[:c.M, :c.N], G.NONE, 1)
        assert R.check(exact.float(), *iv)[0] == 0
        assert R.check((exact + c.bias[:c.N].double()).float(), *iv)[0] > 0, (name, z)


@pytest.mark.parametrize("name", [n for n in sorted(G.SETS) if G.SETS[n][1] >= 130])
def test_group_mistakes_leave_the_intervals(name):
    """the two-group Linear: W2 and bias2 taken from row m_split - 64 on, and W1 for every row"""
    c = Case(name)
    m_split = 128 if c.M >= 200 else 64
    out_f32 = c.outs()[0]
    lin1, e1 = c.lin_e(True)
    lin2, e2 = c.lin_e(True, col0=c.N)
    for epi in G.EPIS:
        iv = G.interval(torch.cat((lin1[:m_split], lin2[m_split:])), torch.cat((e1[:m_split], e2[m_split:])), epi, out_f32)
        grouped = lambda split: G.out_round(G.epi64(torch.cat((lin1[:split], lin2[split:])), epi), out_f32)
        assert R.check(grouped(m_split), *iv)[0] == 0
        assert R.check(grouped(m_split - 64), *iv)[0] > 0, (name, epi, "second group from row m_split - 64")
        assert R.check(grouped(c.M), *iv)[0] > 0, (name, epi, "W1 for every row")


def test_gelu_minimum_and_band():
    """the interior minimum of GELU is where the module says, and the band is absolute: at v = -3 it is far wider than a relative band on
    the result would be, as 1 + erf cancels there"""
    x = torch.linspace(-1.0, -0.5, 200001, dtype=F64)
    g = G.gelu64(x)
    assert abs(float(x[g.argmin()]) - G.GELU_ARGMIN) < 1e-5 and abs(float(g.min()) - G.GELU_MIN) < 1e-12
    assert abs(G.GELU_ARGMIN + 0.75179) < 1e-5
    v = torch.tensor([-3.0], dtype=F64)
    assert float(G.gelu_band(v, G.gelu64(v))) > 100 * float(G.gelu64(v).abs()) * 2.0 ** -22
    lo, hi = G.epi_bounds(torch.tensor([-1.0], dtype=F64), torch.tensor([-0.5], dtype=F64), G.GELU)
    assert float(lo) < G.GELU_MIN < float(hi)
