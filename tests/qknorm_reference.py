"""Float64 reference for the per-head q / k RMSNorm of the Qwen3 layout in front of the decode attention (ll_decode_attn_rope_qkn_bf16,
ll_suffix_attn_rope_qkn_bf16) and the inputs both tests of it run on.  Written from the contract in include/llamole_hip.h and HuggingFace's
Qwen3RMSNorm (x.float(); x * rsqrt(mean(x^2) + eps); cast to bf16; weight * that), not from the kernels.

    xh = bf16( x * rsqrt( mean_D(x^2) + eps ) )        float64 here, ONE rounding to bf16
    y  = bf16( w * xh )                                exact product of two bf16 values, ONE rounding to bf16

then tests/attn_reference.py unchanged: rotary_bf16, attention_f64 and its bound 2^-8 |ref| + 2^-11 absref; the appended cache rows bit for bit.

Tie-safe head vectors.  The second rounding is of an exact product, the first is not: an f32 evaluation of x * rsqrt(mean + eps) is off by up
to 128 * 2^-24 = 2^-17 (relative) in the sum of squares of 128 terms -- half of that behind the square root -- plus an ulp or so of rsqrt and the
product, and an element within that distance of a bf16 rounding midpoint may legitimately round the other way.  WINDOW = 2^-15 is 4x the
2^-17.  The q and k head vectors of the bounded cases are drawn by rejection: a vector is kept only if every element of the float64
x * rsqrt(mean + eps) is at least WINDOW (relative) away from a midpoint (38 % of N(0, 1) bf16 vectors pass at D = 128, 55 % at D = 64; about 1.1 %
of all elements lie inside the window).  On such vectors every correct evaluation gives the same bits.  On unrestricted vectors `key_candidates`
lists what a correct evaluation may store: either neighbour at the elements inside the window, the one value everywhere else."""
from types import SimpleNamespace

import torch

from tests import attn_reference as R

BF = R.BF
EPS = 1e-6
WINDOW = 2.0 ** -15


# ------------------------------------------------------------------------------------------------------------------ the reference itself
def scaled_f64(x, eps, mean_over=None):
    """x * rsqrt(mean_D(x^2) + eps) in float64, before any rounding.  mean_over: the (wrong) number of leading elements the mean is taken over."""
    xd = x.double()
    sq = xd * xd if mean_over is None else (xd * xd)[..., :mean_over]
    return xd * torch.rsqrt(sq.mean(-1, keepdim=True) + eps)


def head_norm(x, w, eps=EPS, mean_over=None, weight_first=False):
    """Qwen3RMSNorm over the last dimension of bf16 x with bf16 weight w [D].  weight_first: the (wrong) single rounding bf16(w * x * rstd)."""
    assert x.dtype == BF and w.dtype == BF
    t = scaled_f64(x, eps, mean_over)
    if weight_first:
        return (w.double() * t).to(BF)
    return (w.double() * t.to(BF).double()).to(BF)


def tie_distance(t):
    """relative distance of every float64 element from the nearest bf16 rounding midpoint (zero elements: 1)"""
    a = t.abs()
    _, e = torch.frexp(a)                                    # a = m * 2^e, m in [0.5, 1)
    u = torch.ldexp(a, 8 - e)                                # [128, 256): the bf16 grid is the integers
    d = ((u - torch.floor(u)) - 0.5).abs() / u
    return torch.where(a > 0, d, torch.ones_like(d))


def in_window(x, eps=EPS):
    """bool per element: the first rounding of the norm of bf16 x [..., D] sits within WINDOW of a midpoint"""
    return tie_distance(scaled_f64(x, eps)) < WINDOW


def tie_safe(g, shape, eps=EPS, scale=1.0):
    """N(0, 1) * scale bf16 head vectors [*shape] (last dimension = head_dim) with no element of the norm inside the window"""
    n, D = int(torch.tensor(shape[:-1]).prod()), shape[-1]
    keep, have = [], 0
    while have < n:
        x = (torch.randn(4 * n + 8, D, generator=g) * scale).to(BF)
        x = x[~in_window(x, eps).any(-1)]
        keep.append(x)
        have += x.shape[0]
    return torch.cat(keep)[:n].reshape(shape)


def norm_weight(g, D):
    """bf16(1 + 0.5 N(0, 1)): HF initialises the weights to ones, which would hide a missing or swapped weight"""
    return (1 + 0.5 * torch.randn(D, generator=g)).to(BF)


def _other_neighbour(t, xh):
    """the bf16 value on the other side of float64 t from its rounding xh"""
    bits = xh.view(torch.int16).to(torch.int32)
    up = t.abs() > xh.double().abs()                           # larger magnitude = next bit pattern
    return (bits + torch.where(up, 1, -1)).to(torch.int16).view(BF)


def key_candidates(k, kw, cos, sin, eps=EPS):
    """What a correct evaluation may store for the bf16 key rows k [..., D] (cos / sin broadcastable to k): a list of four rotated rows (the two
    elements of a rotary pair each take either neighbour of the first rounding where they lie inside the window, so the four agree wherever
    neither does) and the window flags [..., D]."""
    t = scaled_f64(k, eps)
    flag = tie_distance(t) < WINDOW
    near = t.to(BF)
    far = torch.where(flag, _other_neighbour(t, near), near)
    h = k.shape[-1] // 2
    out = []
    for a in (near, far):
        for b in (near, far):
            xh = torch.cat((a[..., :h], b[..., h:]), dim=-1)
            out.append(R.rotary_bf16((kw.double() * xh.double()).to(BF), cos, sin))
    return out, flag


# ------------------------------------------------------------------------------------------------------------------ the inputs
def _fill_qkv(c, rows):
    n = (c.nh + 2 * c.nkv) * c.D
    c.ld_qkv = n + 8
    c.qkv = torch.full((rows.shape[0], c.ld_qkv), R.NAN, dtype=BF)
    c.qkv[:, :n] = rows


def decode_case(D, nh, nkv, maxlen, pos, variant="plain", B=3, seed=0, safe=True):
    """attn_reference.decode_case (rows cycle through full / left-padded / fully masked) with tie-safe q / k head vectors and random norm weights.
    Variants: plain; dom_pos (k = q before the norm and k_norm_w = 2 q_norm_w: the new key is exactly twice the rotated query and dominates);
    tiny (q / k rows scaled by 2^-12: eps carries the norm).  safe=False: unrestricted N(0, 1) vectors."""
    c = R.decode_case(D, nh, nkv, maxlen, pos, "plain", B=B, seed=seed)
    g = torch.Generator().manual_seed(seed * 7919 + 17 * D + 31 * nh + 101 * maxlen + 3 * pos + B)
    G = nh // nkv
    c.variant, c.eps = variant, EPS
    c.qw, c.kw = norm_weight(g, D), norm_weight(g, D)
    scale = 2.0 ** -12 if variant == "tiny" else 1.0
    draw = (lambda *s: tie_safe(g, s, EPS, scale)) if safe else (lambda *s: (torch.randn(*s, generator=g) * scale).to(BF))
    c.q, c.k = draw(B, nh, D), draw(B, nkv, D)
    c.dominant = []
    if variant == "dom_pos":
        c.q = R._share_q_in_group(c.q, G)
        c.k = c.q[:, ::G].clone()
        c.kw = 2 * c.qw
        c.v = R._value_row(D).expand(B, nkv, D).clone()
        c.dominant = [(b, 0, pos) for b in range(B) if c.visible[b].any()]
    _fill_qkv(c, torch.cat((c.q.reshape(B, -1), c.k.reshape(B, -1), c.v.reshape(B, -1)), dim=1))
    return c


def suffix_case(D, nh, nkv, B, S, maxlen, pos, variant="plain", seed=0):
    """attn_reference.suffix_case with tie-safe q / k head vectors and random norm weights.  Variants: plain; dom_own (row s: its own new key,
    k = q and k_norm_w = 2 q_norm_w, dominates)."""
    c = R.suffix_case(D, nh, nkv, B, S, maxlen, pos, "plain", seed=seed)
    g = torch.Generator().manual_seed(seed * 7919 + 17 * D + 31 * nh + 101 * maxlen + 3 * pos + 1009 * S + B)
    G = nh // nkv
    c.variant, c.eps = variant, EPS
    c.qw, c.kw = norm_weight(g, D), norm_weight(g, D)
    c.q, c.k = tie_safe(g, (B, nh, S, D)), tie_safe(g, (B, nkv, S, D))
    c.dominant = []
    if variant == "dom_own":
        c.q = R._share_q_in_group(c.q, G)
        c.k = c.q[:, ::G].clone()
        c.kw = 2 * c.qw
        for s in range(S):
            c.v[:, :, s] = R._value_row(D, s)
            c.dominant += [(b, s, pos + s) for b in range(B) if pos + s < maxlen]
    rows = lambda t: t.transpose(1, 2).reshape(B * S, -1)
    _fill_qkv(c, torch.cat((rows(c.q), rows(c.k), rows(c.v)), dim=1))
    return c


def normed(c, q=None, k=None, v=None):
    """the case as attn_reference sees it: q and k replaced by their norms (or by what the caller hands in: the mistakes of the CPU test)"""
    n = SimpleNamespace(**vars(c))
    n.q = head_norm(c.q, c.qw, c.eps) if q is None else q
    n.k = head_norm(c.k, c.kw, c.eps) if k is None else k
    if v is not None:
        n.v = v
    return n


def decode_expected(c, **kw):
    """attn_reference.decode_expected of the normalised case: (q_rot, K, V, mask), (k_rot, v_new)"""
    return R.decode_expected(normed(c, **kw))


def suffix_expected(c, cos=None, sin=None, **kw):
    return R.suffix_expected(normed(c, **kw), cos, sin)


GEOMETRIES = [(3, 3), (4, 2), (4, 1), (7, 1), (5, 1)]            # nh, nkv: groups of 1, 2, 4, 7 (grouped kernel from 17 sequences on) and 5 (per-head)
MAXLENS = [64, 320]                                              # one tile of 256 keys, and a second one


def positions(maxlen):
    return sorted({p for p in (0, 37, 255, 256, maxlen - 1) if p < maxlen})


SUFFIX_ROWS = [(2, 1), (9, 1), (3, 5)]                           # S, B


def suffix_positions(S, maxlen):
    """the rows straddle slot 256 where the cache has one, and end in its last slot"""
    return [255 - S // 2, maxlen - S] if maxlen > 256 + S else [maxlen - S - 3, maxlen - S]
