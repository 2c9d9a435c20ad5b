"""Float64 reference for the decode attention entry points (ll_decode_attn_bf16, ll_decode_attn_rope_bf16, ll_suffix_attn_rope_bf16) and the
inputs both reference tests run on.  Written from the contract in include/llamole_hip.h and from HuggingFace's formulas (apply_rotary_pos_emb,
repeat_kv, sdpa with a boolean mask), not from the kernels.

The bound, per output element:   |got - ref| <= 2^-8 |ref| + 2^-11 absref,    absref = sum_j p_j |v_jd|
  2^-8 |ref|     half a bf16 ulp: the one rounding of the output;
  2^-11 absref   the f32 work in front of it: a dot product of D terms, expf, a sum of at most 512 + 32 terms per lane at 16384 keys -- about
                 2^-15 of absref, so the term has 16x room.
A fully masked query row has ref = absref = 0: the output must be exactly zero.

tests/test_decode_attention_reference_cpu.py shows on these very inputs that a plain f32 evaluation stays inside the bound and that the mistakes
a kernel of this kind can make (a key lost at a tile edge, a mask off by one, the wrong scale / rotary pairing / head map, a stale or unrotated
new key) leave it.  Random data cannot show one lost key among hundreds, so the boundary cases carry ONE dominant key: the key at j* is 4 q
(score 4 sqrt(D) against N(0, 1) for the others) with a value row unlike any other."""
import math
from types import SimpleNamespace

import torch

BF = torch.bfloat16
REL, ABS = 2.0 ** -8, 2.0 ** -11
NAN = float("nan")


# ------------------------------------------------------------------------------------------------------------------ the reference itself
def rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def rotary_bf16(x, cos, sin):
    """HF apply_rotary_pos_emb on bf16 tensors, evaluated op by op (every product and the sum rounded to bf16, as torch does)."""
    assert x.dtype == BF and cos.dtype == BF and sin.dtype == BF
    return x * cos + rotate_half(x) * sin


def inv_freq(D, base=10000.0):
    return 1.0 / (base ** (torch.arange(0, D, 2).float() / D))


def rope_tables(freq, position_ids):
    """cos / sin [..., D] bf16 of the default rotary embedding (f32 angles inv_freq * position, both halves alike), on the device of its arguments."""
    f = position_ids.float()[..., None] * freq
    emb = torch.cat((f, f), dim=-1)
    return emb.cos().to(BF), emb.sin().to(BF)


def attention_f64(q_rot, K, V, mask, scale, nh, nkv, return_weights=False):
    """softmax(scale q K^T, masked) V in float64 on the bf16 values.  q_rot [B,nh,S,D], K / V [B,nkv,L,D], mask bool [B,S,L] (True = visible).
    Masked slots of K / V may hold anything (NaN).  Returns ref, absref [B,nh,S,D] (and the weights [B,nh,S,L])."""
    B, _, S, D = q_rot.shape
    assert q_rot.shape[1] == nh and K.shape[1] == nkv and nh % nkv == 0 and mask.shape == (B, S, K.shape[2])
    ref = torch.zeros(B, nh, S, D, dtype=torch.float64)
    absref = torch.zeros_like(ref)
    weights = []
    for b in range(B):
        seen = mask[b].any(0)[None, :, None]
        Kb = torch.where(seen, K[b].double(), 0.0).repeat_interleave(nh // nkv, dim=0)      # [nh,L,D]
        Vb = torch.where(seen, V[b].double(), 0.0).repeat_interleave(nh // nkv, dim=0)
        s = scale * (q_rot[b].double() @ Kb.transpose(-1, -2))                                  # [nh,S,L]
        s = s.masked_fill(~mask[b][None], -math.inf)
        m = s.amax(-1, keepdim=True)
        e = torch.exp(s - torch.where(torch.isfinite(m), m, 0.0))
        den = e.sum(-1, keepdim=True)
        p = torch.where(den > 0, e / den, 0.0)                                                  # no visible key: zeros
        ref[b] = p @ Vb
        absref[b] = p @ Vb.abs()
        if return_weights:
            weights.append(p)
    assert torch.isfinite(ref).all() and torch.isfinite(absref).all()
    return (ref, absref, torch.stack(weights)) if return_weights else (ref, absref)


def bound(ref, absref):
    return REL * ref.abs() + ABS * absref


def err_over_bound(got, ref, absref):
    """max over the elements of |got - ref| / bound; an element whose bound is zero must be exact (inf otherwise).  NaN counts as inf."""
    err = (got.double().cpu() - ref).abs()
    bnd = bound(ref, absref)
    ratio = torch.where(bnd > 0, err / bnd, torch.where(err == 0, 0.0, math.inf))
    ratio = torch.nan_to_num(ratio, nan=math.inf, posinf=math.inf)
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------------------------ the inputs
def _rand(g, *shape):
    return torch.randn(*shape, generator=g).to(BF)


def _value_row(D, k=0):
    return ((torch.arange(D) % 16) * 0.5 + 4 + k).to(BF)          # 4 .. 11.5 (+ k): exact in bf16, unlike any N(0, 1) row


def _share_q_in_group(q, G):
    """dominant-key inputs: the heads of a KV group share one query (they share the key that is 4 q)."""
    nh = q.shape[1]
    return q[:, torch.arange(nh) // G * G].clone()


PADS = (17, 5, 200, 255, 256, 1)


def dom_index(variant, pad, pos):
    """slot of the dominant key of a decode row (left padding `pad`, new position `pos`), or None where the row has no such slot."""
    what = variant[4:]
    j = {"first": pad, "prev": pos - 1, "pos": pos}.get(what)
    if j is None:
        j = int(what)
    return j if pad <= j <= pos else None


def decode_case(D, nh, nkv, maxlen, pos, variant="plain", B=3, bcast=False, seed=0):
    """One ll_decode_attn_rope_bf16 call.  Rows cycle through full / left-padded / fully masked.  Variants: plain, dom_first|prev|pos|<slot>
    (one dominant key), qzero (uniform weights), q8 (scores x 8), tile2 (nothing visible in the first 256 slots)."""
    g = torch.Generator().manual_seed(seed * 7919 + D + 31 * nh + 101 * maxlen + 3 * pos)
    G = nh // nkv
    c = SimpleNamespace(kind="decode", D=D, nh=nh, nkv=nkv, B=B, S=1, maxlen=maxlen, pos=pos, variant=variant, scale=D ** -0.5)
    q, k, v = _rand(g, B, nh, D), _rand(g, B, nkv, D), _rand(g, B, nkv, D)
    c.K0, c.V0 = _rand(g, B, nkv, maxlen, D), _rand(g, B, nkv, maxlen, D)
    c.stale_k, c.stale_v = c.K0[:, :, pos].clone(), c.V0[:, :, pos].clone()    # what the slot held before this step
    pads, vis = [], torch.zeros(B, maxlen, dtype=torch.bool)
    for b in range(B):
        pad = min(PADS[(b // 3) % len(PADS)], pos) if b % 3 == 1 else 0
        if variant == "tile2":
            pad = pos if b % 3 == 0 else max(256, pos - 40)
        pads.append(pad)
        if b % 3 != 2:
            vis[b, pad:pos + 1] = True
        if variant == "tile2" and b % 3 == 1 and pos > 256:      # one old key of the second tile, the new one hidden
            vis[b] = False
            vis[b, pos - 1] = True
    c.pads, c.visible = pads, vis
    position = torch.tensor([pos + 11 * (b + 1) - pads[b] for b in range(B)])
    if bcast:
        position = position[:1]
    c.cos, c.sin = rope_tables(inv_freq(D), position)            # [1 or B, D]
    c.cs_stride = 0 if bcast else D
    if variant == "qzero":
        q.zero_()
    elif variant == "q8":
        q *= 8
    c.dominant = []
    if variant.startswith("dom_"):
        q = _share_q_in_group(q, G)
        for b in range(B):
            j = dom_index(variant, pads[b], pos) if vis[b].any() else None
            if j is None:
                continue
            c.dominant.append((b, 0, j))
            if j == pos:         # the new key: 4 q before the rotation (a rotation keeps the dot product, a factor 4 commutes with every rounding)
                k[b] = 4 * q[b, ::G]
                v[b] = _value_row(D)
            else:
                cs = c.cos[0 if bcast else b], c.sin[0 if bcast else b]
                c.K0[b, :, j] = 4 * rotary_bf16(q[b, ::G], *cs)
                c.V0[b, :, j] = _value_row(D)
    c.q, c.k, c.v = q, k, v
    c.ld_qkv = (nh + 2 * nkv) * D + 8
    c.qkv = torch.full((B, c.ld_qkv), NAN, dtype=BF)
    c.qkv[:, :(nh + 2 * nkv) * D] = torch.cat((q.reshape(B, -1), k.reshape(B, -1), v.reshape(B, -1)), dim=1)
    c.mask_stride = maxlen + 5
    c.mask = torch.ones(B, c.mask_stride, dtype=torch.bool)     # the bytes behind a row read as "visible": nobody may read them
    c.mask[:, :maxlen] = vis
    return c


def decode_expected(c, rotary=rotary_bf16, rotate_new_key=True, stale_key=False, stale_value=False):
    """(q_rot [B,nh,1,D], K, V [B,nkv,L,D] after the append, mask [B,1,L]) and the appended rows (k_rot, v_new).  The keyword arguments are the
    deliberately wrong variants of the CPU test."""
    cos, sin = c.cos[:, None, :], c.sin[:, None, :]
    q_rot = rotary(c.q, cos, sin)
    k_rot = rotary(c.k, cos, sin) if rotate_new_key else c.k
    K, V = c.K0.clone(), c.V0.clone()
    K[:, :, c.pos] = c.stale_k if stale_key else k_rot
    V[:, :, c.pos] = c.stale_v if stale_value else c.v
    return (q_rot[:, :, None, :], K, V, c.visible[:, None, :]), (k_rot, c.v)


def suffix_case(D, nh, nkv, B, S, maxlen, pos, variant="plain", seed=0):
    """ll_suffix_prologue + ll_suffix_attn_rope_bf16: S new rows per sequence at slots pos .. pos + S - 1 (rows past the end are not stored).
    Variants: plain, dom_own (row s: its own new key dominates), dom_first (last row: the first visible cache key dominates)."""
    g = torch.Generator().manual_seed(seed * 7919 + D + 31 * nh + 101 * maxlen + 3 * pos + 1009 * S + B)
    G = nh // nkv
    c = SimpleNamespace(kind="suffix", D=D, nh=nh, nkv=nkv, B=B, S=S, maxlen=maxlen, pos=pos, variant=variant, scale=D ** -0.5)
    q, k, v = _rand(g, B, nh, S, D), _rand(g, B, nkv, S, D), _rand(g, B, nkv, S, D)
    c.K0, c.V0 = _rand(g, B, nkv, maxlen, D), _rand(g, B, nkv, maxlen, D)
    c.pads = [7 if (B == 2 and b == 1) else 0 for b in range(B)]
    c.mask2d_stride = maxlen + 3
    c.mask2d = torch.ones(B, c.mask2d_stride, dtype=torch.long)
    for b in range(B):
        c.mask2d[b, :c.pads[b]] = 0
    c.position_ids = torch.tensor([[pos - c.pads[b] + s for s in range(S)] for b in range(B)])
    c.inv_freq = inv_freq(D)
    cos, sin = rope_tables(c.inv_freq, c.position_ids)           # [B,S,D]
    c.dominant = []
    if variant == "dom_own":
        q = _share_q_in_group(q, G)
        k = 4 * q[:, ::G]
        for s in range(S):
            v[:, :, s] = _value_row(D, s)
            c.dominant += [(b, s, pos + s) for b in range(B) if pos + s < maxlen]
    elif variant == "dom_first":
        q = _share_q_in_group(q, G)
        for b in range(B):
            c.K0[b, :, c.pads[b]] = 4 * rotary_bf16(q[b, ::G, S - 1], cos[b, S - 1], sin[b, S - 1])
            c.V0[b, :, c.pads[b]] = _value_row(D)
            c.dominant.append((b, S - 1, c.pads[b]))
    c.q, c.k, c.v = q, k, v
    c.ld_qkv = (nh + 2 * nkv) * D + 8
    c.qkv = torch.full((B * S, c.ld_qkv), NAN, dtype=BF)
    rows = lambda t: t.transpose(1, 2).reshape(B * S, -1)       # [B,H,S,D] -> [B*S, H*D]
    c.qkv[:, :(nh + 2 * nkv) * D] = torch.cat((rows(q), rows(k), rows(v)), dim=1)
    j = torch.arange(maxlen)
    c.old = torch.stack([(j >= c.pads[b]) & (j < pos) for b in range(B)])          # slots that hold keys before the call
    return c


def suffix_expected(c, cos=None, sin=None):
    """(q_rot [B,nh,S,D], K, V after the call, mask [B,S,L]) built from mask2d, pos and position_ids alone; cos / sin [B,S,D] default to
    rope_tables on the CPU (the GPU test hands in torch's on the device)."""
    if cos is None:
        cos, sin = rope_tables(c.inv_freq, c.position_ids)
    cos, sin = cos[:, None], sin[:, None]
    q_rot, k_rot = rotary_bf16(c.q, cos, sin), rotary_bf16(c.k, cos, sin)
    K, V = c.K0.clone(), c.V0.clone()
    n = max(0, min(c.S, c.maxlen - c.pos))                       # rows that fit
    K[:, :, c.pos:c.pos + n] = k_rot[:, :, :n]
    V[:, :, c.pos:c.pos + n] = c.v[:, :, :n]
    j = torch.arange(c.maxlen)
    mask = (j[None, None, :] <= (c.pos + torch.arange(c.S))[None, :, None]) & (c.mask2d[:, None, :c.maxlen] != 0)
    written = torch.zeros(c.maxlen, dtype=torch.bool)
    written[c.pos:c.pos + n] = True
    return (q_rot, K, V, mask), written


def attn_case(D, nh, nkv, S, maxlen, p0, variant="plain", B=2, seed=0):
    """One ll_decode_attn_bf16 call: query row s sees the slots up to p0 + s (causal), the second sequence is left-padded.  Variants: plain,
    dom_last (row s: slot p0 + s dominates), dom_first (last row: the first visible slot), dom_<slot> (last row)."""
    g = torch.Generator().manual_seed(seed * 7919 + D + 31 * nh + 101 * maxlen + 3 * p0 + 1009 * S)
    G = nh // nkv
    c = SimpleNamespace(kind="attn", D=D, nh=nh, nkv=nkv, B=B, S=S, maxlen=maxlen, pos=p0, variant=variant, scale=D ** -0.5)
    q = _rand(g, B, nh, S, D)
    c.K0, c.V0 = _rand(g, B, nkv, maxlen, D), _rand(g, B, nkv, maxlen, D)
    c.pads = [9 if b == 1 else 0 for b in range(B)]
    j = torch.arange(maxlen)
    c.visible = torch.stack([torch.stack([(j >= c.pads[b]) & (j <= p0 + s) for s in range(S)]) for b in range(B)])       # [B,S,L]
    c.dominant = []
    if variant.startswith("dom_"):
        q = _share_q_in_group(q, G)
        for b in range(B):
            for s in (range(S) if variant == "dom_last" else [S - 1]):
                jj = p0 + s if variant == "dom_last" else c.pads[b] if variant == "dom_first" else int(variant[4:])
                c.K0[b, :, jj] = 4 * q[b, ::G, s]
                c.V0[b, :, jj] = _value_row(D, s)
                c.dominant.append((b, s, jj))
    c.q = q
    return c


def attn_expected(c):
    return (c.q, c.K0, c.V0, c.visible), None


def expected(c):
    return {"decode": decode_expected, "suffix": suffix_expected, "attn": attn_expected}[c.kind](c)


def reference(c, inputs=None):
    """ref, absref [B,nh,S,D] of a case; checks that every dominant key of the case carries more than 0.99 of its row's weight."""
    q_rot, K, V, mask = inputs if inputs is not None else expected(c)[0]
    ref, absref, p = attention_f64(q_rot, K, V, mask, c.scale, c.nh, c.nkv, return_weights=True)
    for b, s, j in c.dominant:
        assert float(p[b, :, s, j].min()) > 0.99, (c.variant, b, s, j, float(p[b, :, s, j].min()))
    return ref, absref


def poison(c, K, V, keep):
    """K / V with NaN in every slot outside `keep` (bool [B,L]: the slots that hold keys the call may read)."""
    k = keep[:, None, :, None]
    return torch.where(k, K, torch.full_like(K, NAN)), torch.where(k, V, torch.full_like(V, NAN))


# ------------------------------------------------------------------------------------------------------------------ the case lists
GEOMETRIES = [(64, 4, 4), (64, 4, 2), (64, 6, 2), (64, 7, 1), (128, 4, 4), (128, 4, 2), (128, 6, 2), (128, 7, 1)]        # D, nh, nkv
POSITIONS = [(1, 0), (40, 0), (40, 39), (256, 255), (257, 256), (300, 255), (300, 256), (513, 512), (600, 300)]           # maxlen, *pos
DECODE_VARIANTS = ["plain", "dom_first", "dom_255", "dom_256", "dom_prev", "dom_pos", "qzero", "q8", "tile2"]


def decode_variants(maxlen, pos):
    """the variants a (maxlen, *pos) pair has room for"""
    out = []
    for v in DECODE_VARIANTS:
        if v in ("dom_255", "dom_256") and pos < int(v[4:]):
            continue
        if v == "dom_prev" and pos < 1:
            continue
        if v == "tile2" and pos < 256:
            continue
        out.append(v)
    return out


GROUPED_GEOMETRIES = [(D, nh, nkv) for D in (64, 128) for nh, nkv in ((4, 2), (8, 2), (7, 1))]       # G = 2, 4, 7: the six instances
GROUPED_POSITIONS = [(300, 255), (300, 256), (40, 0)]
LDS_SWITCH = [4312, 4320]        # G = 7, D = 128, nkv = 1, 17 sequences: 33 280 + 28 maxlen bytes of LDS against 150 KB

ATTN_CASES = [(D, nh, nkv, S, maxlen, p0) for D in (64, 128) for nh, nkv in ((2, 2), (7, 1))
              for S, maxlen, p0 in ((1, 40, 39), (5, 40, 34), (1, 300, 255), (5, 300, 252))]
ATTN_VARIANTS = ["plain", "dom_last", "dom_first"]

SUFFIX_CASES = [(D, nh, nkv, B, S, maxlen, pos) for D in (64, 128) for nh, nkv in ((2, 2), (8, 2), (7, 1)) for B in (1, 2)
                for S in (1, 9, 16) for maxlen, pos in ((96, 41), (300, 250), (300, 284))]
SUFFIX_VARIANTS = ["plain", "dom_own", "dom_first"]

# B = 1, nh = 2, nkv = 1: (D, maxlen, variants); *pos = maxlen - 1
LONG_CASES = [(128, 12032, ("plain", "dom_pos")), (128, 12040, ("plain", "dom_pos")), (128, 16384, ("plain", "dom_12100", "dom_pos")),
              (64, 16384, ("dom_12100", "dom_pos"))]
MAXLEN_LIMIT = 16384


def long_case(entry, D, maxlen, variant):
    """the long-context case of an entry point ("decode", "suffix", "attn")"""
    if entry == "decode":
        return decode_case(D, 2, 1, maxlen, maxlen - 1, variant, B=1, bcast=True)
    if entry == "attn":
        return attn_case(D, 2, 1, 1, maxlen, maxlen - 1, {"dom_pos": "dom_last"}.get(variant, variant), B=1)
    c = suffix_case(D, 2, 1, 1, 2, maxlen, maxlen - 1, {"dom_pos": "dom_own", "plain": "plain"}.get(variant, "plain"))
    if variant.startswith("dom_") and variant != "dom_pos":      # an old cache key dominates the first row
        j = int(variant[4:])
        cos, sin = rope_tables(c.inv_freq, c.position_ids)
        c.q = _share_q_in_group(c.q, 2)
        c.qkv[:, :2 * D] = c.q.transpose(1, 2).reshape(2, -1)
        c.K0[0, :, j] = 4 * rotary_bf16(c.q[0, ::2, 0], cos[0, 0], sin[0, 0])
        c.V0[0, :, j] = _value_row(D)
        c.dominant = [(0, 0, j)]
        c.variant = variant
    return c
