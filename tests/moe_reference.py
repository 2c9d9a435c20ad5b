"""Float64 reference with rounding intervals for the sparse-MoE decode kernels (ll_moe_route_bf16, ll_moe_experts_bf16) and the operand sets
both MoE tests run on.  Written from the contract in include/llamole_hip.h and HuggingFace's formulas (Qwen3MoeTopKRouter, Qwen3MoeExperts with
the default grouped_mm experts path, the decoder layer's residual add), not from the kernels; the Linear part reuses linear_reference.

Router (route64).  Everything in float64 on the bf16 logits (held exactly):
    selection   the top_k largest logits, descending, equal logits by the lower index (a stable sort of -l) -- exact, no tolerance: idx must match;
    p_j         = exp(l_j - max) / sum_i exp(l_i - max);   w_j = p_j / sum_selected p  (norm_topk)  or  p_j;   one rounding to bf16.
  The kernel evaluates this in f32 (u = 2^-24).  With A = max_i |l_i - max|: the argument l_i - max is rounded (relative error of exp <= A u),
  expf is good to 2 ulp (4 u), so every term carries a <= (4 + A) u; the sum of E positive terms in any order adds (E - 1) u, a division u, the
  sum over the k selected (k - 1) u, the second division u.  In w_j the error of the common denominator cancels when norm_topk is set and stays
  when it is not; either way  |w_f32 / w_64 - 1| <= DELTA = (2 (4 + A) + E + k + 4) u.  The final rounding is monotone, so the accepted values are
  [bf16(w (1 - DELTA)), bf16(w (1 + DELTA))]: ONE bf16 value unless w lies within DELTA (relative, ~2e-5 at E = 256 against the bf16 half-step of
  2^-9 = 2e-3) of a rounding boundary, then the two neighbours.  route64 returns how many weights have two accepted values (`free`).

Experts (ExpertsRef).  For token row m and slot j with e = idx[m, j], from linear_reference (e = 2^-14 sum |x| |w| per Linear, rstd band of the HF
RMSNorm form, SiLU band):
    a_mj  in [alo, ahi]   = interval(linear64(x_m, Wgu[e], norm_w, eps, HF), SILU_MUL)                  (bf16 values, mostly alo == ahi)
    y_mj  in [bf16(sum_i min(alo_i w, ahi_i w) - ey), bf16(sum_i max(..) + ey)],  ey = 2^-14 sum_i max(|alo_i|, |ahi_i|) |Wd[e][h, i]|
    z_mj  = bf16(w_mj y_mj): the f32 product of two bf16 values is exact and w_mj >= 0, so z is monotone in y: [bf16(w ylo), bf16(w yhi)]
    s_m   = sum_j z_mj in f32, slot order: k - 1 additions, |error| <= (k - 1) 2^-24 sum_j max(|zlo|, |zhi|) = es
    out_m in [bf16(res + bf16(sum zlo - es)), bf16(res + bf16(sum zhi + es))]                            (both roundings monotone)
  An output passes iff it lies in that interval (NaN fails).  Nothing here is a chosen tolerance: each widening is one of the roundings or the
  f32 summation-order bound on the path.  HF's `eager` experts implementation differs from this contract only by keeping the running sum of the k
  terms in bf16 (index_add_ in expert order); tests/test_moe_reference_cpu.py shows both statements on HF's own modules.

The experts take idx and w as INPUTS (the GPU test passes what ll_moe_route_bf16 wrote, after checking it against route64), so ExpertsRef keeps
the w-independent part (a, y) per case and finishes with the w it is given.  Experts that no row selects hold NaN matrices in every case: a
wrong expert index shows up as NaN, not as a small error."""
import functools

import torch

from tests import linear_reference as LR

BF, F64 = torch.bfloat16, torch.float64
bf16r = LR.bf16r
U24 = 2.0 ** -24
EPS = 1e-6


# ------------------------------------------------------------------------------------------------------------------ router
def route_delta(logits, top_k):
    l = logits.to(F64)
    A = float((l - l.amax(-1, keepdim=True)).abs().max())
    return (2 * (4 + A) + logits.shape[1] + top_k + 4) * U24


def route64(logits, top_k, norm_topk, select="desc-low", softmax_over="all", renorm="selected"):
    """idx [M,k] int32, w mid / lo / hi [M,k] float32 (bf16 values), free = number of weights with two accepted values.
    The keyword arguments exist for the CPU test's deliberate mistakes; the defaults are the contract."""
    l = logits.to(F64)
    if select == "desc-low":
        idx = torch.sort(-l, dim=-1, stable=True).indices[:, :top_k]
    elif select == "desc-high":         # the mistake: ties toward the higher index
        idx = (l.shape[1] - 1 - torch.sort(-l.flip(-1), dim=-1, stable=True).indices)[:, :top_k]
    else:                               # the mistake: ascending
        idx = torch.sort(l, dim=-1, stable=True).indices[:, :top_k]
    if softmax_over == "all":
        p = torch.softmax(l, dim=-1).gather(1, idx)
    else:                               # the mistake: softmax over the selected logits only
        p = torch.softmax(l.gather(1, idx), dim=-1)
    if norm_topk and renorm == "selected":
        w = p / p.sum(-1, keepdim=True)
    elif norm_topk and renorm == "all":     # the mistake: "renormalised" over all experts = not at all
        w = p / torch.softmax(l, dim=-1).sum(-1, keepdim=True)
    else:
        w = p
    d = route_delta(logits, top_k)
    lo, hi, mid = bf16r(w * (1 - d)), bf16r(w * (1 + d)), bf16r(w)
    return idx.to(torch.int32), mid.float(), lo.float(), hi.float(), int((lo != hi).sum())


def route_logits(kind, M, E, top_k, seed):
    """bf16 logits [M, E] whose routing has the named shape."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * M + 3 * E + top_k)
    l = torch.randn(M, E, generator=g) * 2
    if kind == "same":                  # every row on the same experts: one group of M rows per selected expert
        l = l[:1].repeat(M, 1)
    elif kind == "distinct":            # every (row, slot) on its own expert
        assert M * top_k <= E
        for m in range(M):
            l[m, m * top_k:(m + 1) * top_k] = 8 + torch.arange(top_k, 0, -1) * 0.5
    elif kind == "ends":                # experts 0 and E - 1 in every row (E - 1 first), the other slots random
        assert top_k >= 2
        l[:, E - 1], l[:, 0] = 9.0, 8.5
    elif kind == "few":                 # only the first top_k + 1 experts can win: the others are selected by nobody
        l[:, top_k + 1:] -= 20
    else:
        assert kind == "random", kind
    return l.to(BF)


# ------------------------------------------------------------------------------------------------------------------ experts
class ExpertsCase:
    def __init__(self, name, H, I, E, top_k, M, kind, seed, probe=False):
        g = torch.Generator().manual_seed(7919 * seed + H + 3 * I + 5 * E + 11 * top_k + 13 * M)
        self.name, self.H, self.I, self.E, self.top_k, self.M, self.eps = name, H, I, E, top_k, M, EPS
        self.logits = route_logits(kind, M, E, top_k, seed)
        self.norm_topk = seed % 2 == 0
        self.idx, self.w, self.wlo, self.whi, self.free = route64(self.logits, top_k, self.norm_topk)
        self.x = torch.randn(M, H, generator=g).to(BF)
        if probe:                       # one-hot rows x = c e_k: a lost or misplaced column of Wgu[e] gives 0 or another weight
            self.x = torch.zeros(M, H, dtype=BF)
            for m in range(M):
                self.x[m, (37 * m + 5) % H] = (1.0, -2.0, 0.5, 4.0)[m % 4]
        self.norm_w = (1 + 0.25 * torch.randn(H, generator=g)).to(BF)
        self.res = torch.randn(M, H, generator=g).to(BF)
        self.wgu = (torch.randn(E, 2 * I, H, generator=g) * (H ** -0.5)).to(BF)
        self.wd = (torch.randn(E, H, I, generator=g) * (I ** -0.5) * 4).to(BF)
        used = torch.zeros(E, dtype=torch.bool)
        used[self.idx.long().flatten()] = True
        self.used = used
        self.wgu[~used] = float("nan")
        self.wd[~used] = float("nan")
        self._ay = None

    def ay(self):
        """the w-independent part (experts_ay), computed once"""
        if self._ay is None:
            self._ay = experts_ay(self.x, self.norm_w, self.eps, self.idx, self.wgu, self.wd)
        return self._ay

    def bounds(self, w):
        """lo, hi, mid [M,H] float32 of out for routing weights w [M,k] (bf16 values, >= 0)"""
        _, _, _, ylo, yhi, ymid = self.ay()
        return finish(ylo, yhi, ymid, w, self.res)


def experts_ay(x, norm_w, eps, idx, wgu, wd):
    """(alo, ahi, amid [M,k,I], ylo, yhi, ymid [M,k,H]) float64 holding bf16 values"""
    (M, H), k, I, E = x.shape, idx.shape[1], wd.shape[2], wd.shape[0]
    out = [torch.zeros(M, k, n, dtype=F64) for n in (I, I, I, H, H, H)]
    for e in range(E):
        rows, slots = torch.nonzero(idx == e, as_tuple=True)
        if rows.numel() == 0:
            continue
        lin, err = LR.linear64(x[rows], wgu[e], None, norm_w, eps, LR.HF)
        alo, ahi, amid = (t.to(F64) for t in LR.interval(lin, err, LR.SILU_MUL))
        w = wd[e].to(F64)
        lo_t = torch.minimum(alo[:, None, :] * w[None], ahi[:, None, :] * w[None]).sum(-1)
        hi_t = torch.maximum(alo[:, None, :] * w[None], ahi[:, None, :] * w[None]).sum(-1)
        ey = LR.U * (torch.maximum(alo.abs(), ahi.abs()) @ w.abs().t())
        vals = (alo, ahi, amid, bf16r(lo_t - ey), bf16r(hi_t + ey), bf16r(amid @ w.t()))
        for dst, v in zip(out, vals):
            dst[rows, slots] = v
    return tuple(out)


def finish(ylo, yhi, ymid, w, res, eager_order=None):
    """the contract's tail on y: z = bf16(w y), the f32 slot sum with ONE rounding, the residual add.  eager_order [M,k] (slot indices in the order
    HF's `eager` experts loop visits them: ascending expert id) switches to that implementation's bf16 running sum instead."""
    wd = w.to(F64)[:, :, None]
    assert bool((wd >= 0).all())
    zlo, zhi, zmid = bf16r(wd * ylo), bf16r(wd * yhi), bf16r(wd * ymid)
    k = w.shape[1]
    r = res.to(F64)
    if eager_order is not None:
        sums = []
        for z in (zlo, zhi, zmid):
            zs = z.gather(1, eager_order.long()[:, :, None].expand_as(z))
            acc = torch.zeros_like(r)
            for j in range(k):
                acc = bf16r(acc + zs[:, j])
            sums.append(acc)
        lo, hi, mid = (bf16r(r + t) for t in sums)
    else:
        es = (k - 1) * U24 * torch.maximum(zlo.abs(), zhi.abs()).sum(1)
        lo, hi, mid = (bf16r(r + bf16r(t)) for t in (zlo.sum(1) - es, zhi.sum(1) + es, zmid.sum(1)))
    assert bool(((lo <= mid) & (mid <= hi)).all())
    return lo.float(), hi.float(), mid.float()


check = LR.check

# name -> (H, I, E, top_k, M, routing, probe).  The smallest shapes at which the kernels can go wrong: I = 96 is no power of two (H and I are
# multiples of 8, so no workgroup has a partial tile), M = 1..4 are the four kernel variants and pass sizes, 5 the first second pass, 17 / 64 the
# row counts of the 17..64 path; "same" makes groups of M rows (up to 16 passes), "distinct" groups of one; the published widths run with few
# rows (their reference is the costly one).
EXPERT_SETS = {}
for _M in (1, 2, 3, 4, 5, 16, 17, 64):
    EXPERT_SETS[f"same-M{_M}"] = (256, 128, 8, 2, _M, "same", False)
    EXPERT_SETS[f"random-M{_M}"] = (256, 96, 8, 2, _M, "random", False)
EXPERT_SETS.update({
    "distinct-M4-k2": (256, 128, 8, 2, 4, "distinct", False),
    "distinct-M16-k8": (256, 96, 128, 8, 16, "distinct", False),
    "ends-M5-k2": (256, 128, 8, 2, 5, "ends", False),
    "ends-M17-k8-E128": (256, 96, 128, 8, 17, "ends", False),
    "few-M64-k1": (256, 128, 8, 1, 64, "few", False),
    "few-M16-k2-E128": (256, 128, 128, 2, 16, "few", False),
    "random-M64-k8-E128": (256, 96, 128, 8, 64, "random", False),
    "same-M64-k8": (256, 128, 8, 8, 64, "same", False),
    "probe-M4-k2": (256, 128, 8, 2, 4, "random", True),
    "probe-M16-k1": (256, 96, 8, 1, 16, "same", True),
    "wide-M1-k8": (2048, 768, 8, 8, 1, "random", False),           # the published widths (E = 8 keeps the operands small)
    "wide-M5-k8": (2048, 768, 8, 8, 5, "same", False),
    "wide-M3-k2": (2048, 768, 8, 2, 3, "random", False),
    # 4096 < H <= 8192: the kernels' XC = 4 instantiations (four 16-byte chunks of x per thread in the RMSNorm prologue), one row, the first
    # chunk count past 4096, and at the limit a second pass with 64 KB of normalised rows in LDS
    "xc4-M1-H8192": (8192, 8, 8, 2, 1, "random", False),
    "xc4-M3-H4104": (4104, 16, 8, 2, 3, "same", False),
    "xc4-M5-H8192": (8192, 8, 8, 2, 5, "same", False),
})


@functools.lru_cache(maxsize=None)
def experts_case(name):
    H, I, E, k, M, kind, probe = EXPERT_SETS[name]
    return ExpertsCase(name, H, I, E, k, M, kind, seed=sorted(EXPERT_SETS).index(name), probe=probe)


ROUTE_E, ROUTE_K, ROUTE_M = (8, 60, 128, 256), (1, 2, 8), (1, 3, 16, 17, 64)


@functools.lru_cache(maxsize=None)
def route_case(E, top_k, M, norm_topk):
    logits = route_logits("random", M, E, top_k, seed=E + top_k)
    return (logits,) + route64(logits, top_k, norm_topk)
