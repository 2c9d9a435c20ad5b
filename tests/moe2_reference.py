"""Float64 reference with rounding intervals for the two contracts ll_moe_route_f32 / ll_moe_experts_ex_bf16 add to the sparse-MoE decode
kernels: the Mixtral layout (f32 routing weights applied in the slot sum) and the Qwen2-MoE layout (a sigmoid-gated shared expert).  Written
from the contract in include/llamole_hip.h and HuggingFace's formulas (MixtralTopKRouter, Qwen2MoeSparseMoeBlock, the default grouped_mm experts
path, the decoder layer's residual add), not from the kernels.  It reuses tests/moe_reference.py (selection, route_delta, the w-independent
a / y intervals of the experts) and tests/linear_reference.py (the Linears of the shared expert and of its gate).

Mixtral.  The router's weight is w_j = p_j / sum_selected p in f32, NOT rounded to bf16.  moe_reference.route_delta bounds the f32 evaluation:
|w_f32 / w_64 - 1| <= DELTA, so an f32 weight passes iff it lies within DELTA (relative) of the float64 weight (route_f32_ok).  The experts
take idx and w as inputs, as in moe_reference.  With y_mj in [ylo, yhi] (moe_reference.experts_ay) and w_mj >= 0:
    t_mj  = f32(w_mj * y_mj)          an f32 times a bf16 value has 32 significant bits: ONE f32 rounding, monotone in y -> [f32(w ylo), f32(w yhi)]
    sum_j t_mj in f32, slot order:    k - 1 additions, |error| <= (k - 1) 2^-24 sum_j max(|tlo|, |thi|) = es
    out_m in [bf16(res + bf16(sum tlo - es)), bf16(res + bf16(sum thi + es))]
There is no per-slot rounding to bf16: the Qwen3 contract (bf16 weight, z = bf16(w y)) on the same operands leaves these intervals
(tests/test_moe2_reference_cpu.py).

Shared expert.  With xn the post-attention RMSNorm row in HF's form, from linear_reference (e = 2^-14 sum |x| |w| per Linear, rstd band, SiLU band):
    a_s   in interval(linear64(x, [gate_proj; up_proj], norm_w, eps, HF), SILU_MUL)
    s_m   in [bf16(sum_i min(alo w, ahi w) - es), bf16(sum_i max(..) + es)],  es = 2^-14 sum_i max(|alo_i|, |ahi_i|) |down_proj[h, i]|
    g_m   in interval(linear64(x, shared_expert_gate.weight, norm_w, eps, HF), PLAIN)
    sig_m = bf16(1 / (1 + exp(-g))) evaluated in f32 (u = 2^-24): the negation is exact, expf is good to 2 ulp (4 u; the error of exp(-g) enters
            1 + exp(-g) with a factor exp(-g) / (1 + exp(-g)) <= 1), the addition adds u, the division u:  |sig_f32 / sig_64 - 1| <= D = 6 u.
            sigmoid is monotone, so sig lies in [bf16(sigmoid(glo) (1 - D)), bf16(sigmoid(ghi) (1 + D))].
    sh_m  = bf16(sig_m * s_m): the f32 product of two bf16 values is exact; sig >= 0 but s has either sign: the four corners
    e_m   = bf16(sum_j z_mj) as in moe_reference (or the Mixtral sum above)
    out_m in [bf16(res + bf16(elo + shlo)), bf16(res + bf16(ehi + shhi))]      the f32 sum of two bf16 values, every later rounding monotone
An output passes iff it lies in its interval (NaN fails).  Nothing here is a chosen tolerance.  The kernel takes s and g as INPUTS (the caller
computes them with the dense MLP's kernels): the entry-point cases of the GPU test pass given bf16 s and g, i.e. slo == shi and glo == ghi;
the intervals of s and g serve the test of HF's own block and the GPU test of the whole shared-expert path of a fused layer (shared I 192:
router + gate logits over the stacked [E + 1, H] copy, routing with ld = E + 1, the shared expert on the dense kernels, the gated add)."""
import functools

import torch

from tests import linear_reference as LR
from tests import moe_reference as MR

BF, F64 = torch.bfloat16, torch.float64
bf16r = LR.bf16r
U24 = 2.0 ** -24
SIGMOID_DELTA = 6 * U24
check = LR.check


def f32r(t):
    return t.to(torch.float32).to(F64)


# ------------------------------------------------------------------------------------------------------------------ Mixtral router
def route64_f32(logits, top_k):
    """idx [M,k] int32, w [M,k] float64 (renormalised over the selected, always), DELTA"""
    idx = MR.route64(logits, top_k, True)[0]
    l = logits.to(F64)
    p = torch.softmax(l, dim=-1).gather(1, idx.long())
    return idx, p / p.sum(-1, keepdim=True), MR.route_delta(logits, top_k)


def route_f32_ok(w, w64, delta):
    """number of f32 weights outside [w64 (1 - DELTA), w64 (1 + DELTA)] (NaN is outside)"""
    assert w.dtype == torch.float32
    wd = w.to(F64).cpu()
    return int((~((wd >= w64 * (1 - delta)) & (wd <= w64 * (1 + delta)))).sum())


# ------------------------------------------------------------------------------------------------------------------ shared expert
def shared64(x, norm_w, eps, wg, wu, wd, wsg, form=LR.HF):
    """the intervals of s [M,H] and g [M] for HF's shared expert on rows x: (slo, shi, smid, glo, ghi, gmid), float64 holding bf16 values.
    ``form`` is linear_reference's place of the RMSNorm: HF for HF's modules and ll_gemv_fused_bf16, STAGED for ll_linear_rows16_bf16 with a
    norm weight and ll_linear_rows64_bf16 with row sums (the same value up to the place of one bf16 rounding)."""
    lin, err = LR.linear64(x, torch.cat([wg, wu], dim=0), None, norm_w, eps, form)
    alo, ahi, amid = (t.to(F64) for t in LR.interval(lin, err, LR.SILU_MUL))
    w = wd.to(F64)
    lo_t = torch.minimum(alo[:, None, :] * w[None], ahi[:, None, :] * w[None]).sum(-1)
    hi_t = torch.maximum(alo[:, None, :] * w[None], ahi[:, None, :] * w[None]).sum(-1)
    es = LR.U * (torch.maximum(alo.abs(), ahi.abs()) @ w.abs().t())
    ling, errg = LR.linear64(x, wsg, None, norm_w, eps, form)
    glo, ghi, gmid = (t.to(F64)[:, 0] for t in LR.interval(ling, errg, LR.PLAIN))
    return bf16r(lo_t - es), bf16r(hi_t + es), bf16r(amid @ w.t()), glo, ghi, gmid


GATES = {"sigmoid": torch.sigmoid, "identity": lambda g: g, "dropped": torch.ones_like}      # the contract and two deliberate mistakes


# ------------------------------------------------------------------------------------------------------------------ the tail on y
def finish2(ylo, yhi, ymid, w, res, w_f32, shared=None, gate="sigmoid"):
    """lo, hi, mid [M,H] float32 of out.  w [M,k]: f32 values when ``w_f32`` (the Mixtral sum), else bf16 values (the per-slot rounding of
    moe_reference.finish).  shared = (slo, shi, smid [M,H], glo, ghi, gmid [M]) adds the gated shared expert; ``gate`` other than "sigmoid" is
    for the CPU test's deliberate mistakes."""
    wd = w.to(F64)[:, :, None]
    assert bool((wd >= 0).all())
    k = w.shape[1]
    r = res.to(F64)
    rnd = f32r if w_f32 else bf16r
    tlo, thi, tmid = rnd(wd * ylo), rnd(wd * yhi), rnd(wd * ymid)
    es = (k - 1) * U24 * torch.maximum(tlo.abs(), thi.abs()).sum(1)
    elo, ehi, emid = bf16r(tlo.sum(1) - es), bf16r(thi.sum(1) + es), bf16r(tmid.sum(1))
    if shared is not None:
        slo, shi, smid, glo, ghi, gmid = (t.to(F64) for t in shared)
        fn = GATES[gate]
        d = SIGMOID_DELTA if gate == "sigmoid" else 0.0
        siglo, sighi, sigmid = bf16r(fn(glo) * (1 - d))[:, None], bf16r(fn(ghi) * (1 + d))[:, None], bf16r(fn(gmid))[:, None]
        if gate == "sigmoid":
            assert bool((siglo >= 0).all())
        c = torch.stack((siglo * slo, siglo * shi, sighi * slo, sighi * shi))
        shlo, shhi, shmid = bf16r(c.amin(0)), bf16r(c.amax(0)), bf16r(sigmid * smid)
        elo, ehi, emid = bf16r(elo + shlo), bf16r(ehi + shhi), bf16r(emid + shmid)
    lo, hi, mid = bf16r(r + elo), bf16r(r + ehi), bf16r(r + emid)
    if gate == "sigmoid":
        assert bool(((lo <= mid) & (mid <= hi)).all())
    return lo.float(), hi.float(), mid.float()


# ------------------------------------------------------------------------------------------------------------------ the GPU test's cases
# name -> (H, I, E, top_k, M, routing).  H 256 and I 64 are the smallest at which every workgroup still has whole tiles; M = 1, 4 are one-pass
# kernels, 5 the first second pass, 16 / 17 the two sides of the decode's 16-row threshold, 64 the limit; "same" makes groups of M rows,
# "distinct" groups of one, "ends" experts 0 and E - 1; one case at H 4104 builds and runs the wide (XC = 4) instantiation.
SETS2 = {}
for _k in (2, 4):
    for _M in (1, 4, 5, 16, 17, 64):
        for _kind in ("same", "distinct", "ends"):
            if _kind != "distinct" or _M * _k <= 8:
                SETS2[f"{_kind}-M{_M}-k{_k}"] = (256, 64, 8, _k, _M, _kind)
SETS2["wide-M3-k2"] = (4104, 16, 8, 2, 3, "same")
SHARED_I = 192         # shared intermediate size of the fused-layer case: a multiple of 32 (the streaming Linears) that is no power of two
SHARED_ROWS = (1, 2, 4, 5, 16, 17, 64)      # both FMA-GEMV row counts, the first MFMA-stream ones, both sides of the 16-row threshold, the limit


class Case2(MR.ExpertsCase):
    """moe_reference.ExpertsCase (operands, NaN matrices for the experts nobody selects, the a / y intervals) plus the f32 routing of the
    Mixtral contract and given shared-expert rows s [M,H] and gate logits g [M] (bf16)."""

    def __init__(self, name, H, I, E, top_k, M, kind, seed):
        super().__init__(name, H, I, E, top_k, M, kind, seed)
        g = torch.Generator().manual_seed(104729 * seed + 31 * M + top_k)
        idx32, self.w64, self.delta = route64_f32(self.logits, top_k)
        assert torch.equal(idx32, self.idx)
        self.s = (torch.randn(M, H, generator=g) * 0.7).to(BF)
        self.g = (torch.randn(M, generator=g) * 3).to(BF)

    def bounds2(self, w, w_f32, shared):
        _, _, _, ylo, yhi, ymid = self.ay()
        sh = None
        if shared:
            s, gg = self.s.to(F64), self.g.to(F64)
            sh = (s, s, s, gg, gg, gg)
        return finish2(ylo, yhi, ymid, w, self.res, w_f32, sh)


@functools.lru_cache(maxsize=None)
def case2(name):
    H, I, E, k, M, kind = SETS2[name]
    return Case2(name, H, I, E, k, M, kind, seed=sorted(SETS2).index(name))
