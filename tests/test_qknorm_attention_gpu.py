"""ll_decode_attn_rope_qkn_bf16 and ll_suffix_attn_rope_qkn_bf16 (per-head q / k RMSNorm of the Qwen3 layout inside the decode attention launches)
through the C ABI against the float64 reference of tests/qknorm_reference.py: on tie-safe head vectors every output element within
attn_reference's bound 2^-8 |ref| + 2^-11 absref and the caches bit for bit (NaN in every slot the call may not read); on unrestricted vectors the
stored key row exact outside the 2^-15 window of the first rounding and one of its two neighbours inside; one key row through the per-head
kernel, the grouped kernel and the suffix kernel leaves the same bits; null weights and eps = 0 are refused.
tests/test_qknorm_reference_cpu.py shows what these checks let through and what not.

Largest err / bound measured on an MI355X (-s prints them): ll_decode_attn_rope_qkn_bf16 per-head 0.866, grouped 0.878,
ll_suffix_attn_rope_qkn_bf16 0.814 (half a bf16 ulp of the output is most of the bound, as for the kernels without the norm); elements inside
the window on the unrestricted inputs: 0.9 - 1.1 % (139 of 13056 at D = 128, 17 sequences), against the 3 % allowed."""
import pytest
import torch

from tests import attn_reference as R
from tests import qknorm_reference as Q

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module")
def lib():
    from llamole_amd import _lib
    yield _lib.load()
    for entry, r in sorted(WORST.items()):
        print(f"\nlargest err / bound, {entry}: {r:.3f}")


def _check(rc, what):
    from llamole_amd import _lib
    _lib.check(rc, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _nan(*shape):
    return torch.full(shape, R.NAN, dtype=R.BF, device="cuda")


def _within(entry, c, out, ref, absref):
    assert torch.isfinite(out.float()).all(), (entry, c.variant, "the output holds NaN / inf")
    r = R.err_over_bound(out, ref, absref)
    WORST[entry] = max(WORST.get(entry, 0.0), r)
    assert r <= 1.0, (entry, c.variant, c.pos, c.B, r)


def run_decode(lib, c, Kc, Vc, qw=None, kw=None, eps=None):
    """one ll_decode_attn_rope_qkn_bf16 call on the case's inputs; returns (rc, out [B, nh*D])"""
    qkv, cos, sin, mask = c.qkv.cuda(), c.cos.cuda(), c.sin.cuda(), c.mask.cuda()
    qw, kw = (c.qw if qw is None else qw).cuda(), (c.kw if kw is None else kw).cuda()
    pos = torch.tensor([c.pos], dtype=torch.long, device="cuda")
    out = _nan(c.B, c.nh * c.D)
    rc = lib.ll_decode_attn_rope_qkn_bf16(qkv.data_ptr(), c.ld_qkv, cos.data_ptr(), sin.data_ptr(), c.cs_stride, Kc.data_ptr(), Vc.data_ptr(),
                                          pos.data_ptr(), mask.data_ptr(), c.mask_stride, out.data_ptr(), c.B, c.nh, c.nkv, c.maxlen, c.D,
                                          c.scale, qw.data_ptr(), kw.data_ptr(), c.eps if eps is None else eps, _stream())
    torch.cuda.synchronize()
    return rc, out


def check_decode(lib, c, entry):
    keep = c.visible.clone()
    keep[:, c.pos] = False                                       # the stale row at *pos
    Kp, Vp = R.poison(c, c.K0, c.V0, keep)
    Kc, Vc = Kp.cuda(), Vp.cuda()
    rc, out = run_decode(lib, c, Kc, Vc)
    _check(rc, "ll_decode_attn_rope_qkn_bf16")
    inputs, (k_rot, v_new) = Q.decode_expected(c)
    ref, absref = R.reference(c, inputs)
    Kp[:, :, c.pos], Vp[:, :, c.pos] = k_rot, v_new              # the appended row, every other slot as it was
    assert torch.equal(_bits(Kc), _bits(Kp)), (entry, c.variant, c.pos, c.B, "key cache")
    assert torch.equal(_bits(Vc), _bits(Vp)), (entry, c.variant, c.pos, c.B, "value cache")
    _within(entry, c, out.cpu().view(c.B, c.nh, 1, c.D), ref, absref)


@pytest.mark.parametrize("maxlen", Q.MAXLENS)
@pytest.mark.parametrize("nh,nkv", Q.GEOMETRIES)
@pytest.mark.parametrize("D", [64, 128])
def test_decode_entry(lib, D, nh, nkv, maxlen):
    """1 and 3 sequences on the per-head kernel, 17 on the grouped kernel for groups of 2 / 4 / 7 and on the per-head kernel otherwise"""
    for pos in Q.positions(maxlen):
        for B in (1, 3, 17):
            grouped = B > 16 and nh // nkv in (2, 4, 7)
            for variant in ("plain", "dom_pos", "tiny"):
                check_decode(lib, Q.decode_case(D, nh, nkv, maxlen, pos, variant, B=B),
                             "ll_decode_attn_rope_qkn_bf16 " + ("grouped" if grouped else "per-head"))


def run_suffix(lib, c, Kc, Vc, cos, sin, mask, qw=None, kw=None, eps=None):
    qkv = c.qkv.cuda()
    qw, kw = (c.qw if qw is None else qw).cuda(), (c.kw if kw is None else kw).cuda()
    pos = torch.tensor([c.pos], dtype=torch.long, device="cuda")
    out = _nan(c.B * c.S, c.nh * c.D)
    rc = lib.ll_suffix_attn_rope_qkn_bf16(qkv.data_ptr(), c.ld_qkv, cos.data_ptr(), sin.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), pos.data_ptr(),
                                          mask.data_ptr(), out.data_ptr(), c.B, c.S, c.nh, c.nkv, c.maxlen, c.D, c.scale, qw.data_ptr(),
                                          kw.data_ptr(), c.eps if eps is None else eps, _stream())
    torch.cuda.synchronize()
    return rc, out


def check_suffix(lib, c):
    entry = "ll_suffix_attn_rope_qkn_bf16"
    B, S, nh, D, L, rows = c.B, c.S, c.nh, c.D, c.maxlen, c.B * c.S
    Kp, Vp = R.poison(c, c.K0, c.V0, c.old)
    Kc, Vc = Kp.cuda(), Vp.cuda()
    posid, freq, mask2d = c.position_ids.cuda(), c.inv_freq.cuda(), c.mask2d.cuda()
    pos = torch.tensor([c.pos], dtype=torch.long, device="cuda")
    cos, sin = _nan(rows, D), _nan(rows, D)
    mask = torch.ones(rows, L, dtype=torch.bool, device="cuda")
    _check(lib.ll_suffix_prologue(posid.data_ptr(), freq.data_ptr(), 1.0, mask2d.data_ptr(), c.mask2d_stride, pos.data_ptr(), cos.data_ptr(),
                                  sin.data_ptr(), mask.data_ptr(), B, S, D, L, _stream()), "ll_suffix_prologue")
    rc, out = run_suffix(lib, c, Kc, Vc, cos, sin, mask)
    _check(rc, entry)
    inputs, written = Q.suffix_expected(c, cos.cpu().view(B, S, D), sin.cpu().view(B, S, D))
    assert torch.equal(mask.cpu().view(B, S, L), inputs[3])
    ref, absref = R.reference(c, inputs)
    Kp[:, :, written], Vp[:, :, written] = inputs[1][:, :, written], inputs[2][:, :, written]
    assert torch.equal(_bits(Kc), _bits(Kp)), (entry, c.variant, c.pos, S, B, "key cache")
    assert torch.equal(_bits(Vc), _bits(Vp)), (entry, c.variant, c.pos, S, B, "value cache")
    _within(entry, c, out.cpu().view(B, S, nh, D).transpose(1, 2), ref, absref)


@pytest.mark.parametrize("maxlen", Q.MAXLENS)
@pytest.mark.parametrize("nh,nkv", Q.GEOMETRIES)
@pytest.mark.parametrize("D", [64, 128])
def test_suffix_entry(lib, D, nh, nkv, maxlen):
    """S new rows per sequence behind ll_suffix_prologue, straddling slot 256 and ending in the last slot"""
    for S, B in Q.SUFFIX_ROWS:
        for pos in Q.suffix_positions(S, maxlen):
            for variant in ("plain", "dom_own"):
                check_suffix(lib, Q.suffix_case(D, nh, nkv, B, S, maxlen, pos, variant))


@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("nh,nkv", [(4, 2), (7, 1), (3, 3)])
@pytest.mark.parametrize("D", [64, 128])
def test_unrestricted_vectors_store_the_key_or_its_window_neighbour(lib, D, nh, nkv, B):
    """N(0, 1) head vectors as they come: the stored key row equals the reference outside the 2^-15 window of the first rounding; inside it either
    neighbour may be stored (four candidates per rotated pair).  The reference alone flags 1.1 % of the elements."""
    flagged = total = 0
    for maxlen, pos in ((64, 37), (320, 256)):
        c = Q.decode_case(D, nh, nkv, maxlen, pos, "plain", B=B, seed=3, safe=False)
        Kc, Vc = c.K0.cuda(), c.V0.cuda()
        rc, _ = run_decode(lib, c, Kc, Vc)
        _check(rc, "ll_decode_attn_rope_qkn_bf16")
        cands, flag = Q.key_candidates(c.k, c.kw, c.cos[:, None, :], c.sin[:, None, :], c.eps)
        got = Kc[:, :, pos].cpu()
        hit = torch.stack([_bits(got) == _bits(cand) for cand in cands]).any(0)
        assert hit.all(), (maxlen, pos, int((~hit).sum()))
        pair = flag | flag.roll(D // 2, -1)
        assert torch.equal(_bits(got)[~pair], _bits(cands[0])[~pair])
        assert torch.equal(_bits(Vc[:, :, pos]), _bits(c.v))
        flagged, total = flagged + int(flag.sum()), total + flag.numel()
    print(f"\nelements inside the window: {flagged} of {total}")
    assert flagged <= 0.03 * total


@pytest.mark.parametrize("nh,nkv", [(4, 2), (7, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_one_key_row_leaves_the_same_bits_through_all_three_kernels(lib, D, nh, nkv):
    """the same pre-norm k row at the same position and angle: per-head kernel (3 sequences), grouped kernel (17), suffix kernel (both of its
    rows) -- unrestricted data, so the bits are whatever the one device function gives"""
    g = torch.Generator().manual_seed(5 + D + nh)
    maxlen, pos = 320, 255
    krow = torch.randn(D, generator=g).to(R.BF)
    qw, kw = Q.norm_weight(g, D), Q.norm_weight(g, D)
    cos1, sin1 = R.rope_tables(R.inv_freq(D), torch.tensor([91]))            # [1, D]
    stored = []
    for B in (3, 17):
        c = Q.decode_case(D, nh, nkv, maxlen, pos, "plain", B=B, safe=False)
        c.qw, c.kw, c.cos, c.sin, c.cs_stride = qw, kw, cos1, sin1, 0
        c.qkv[:, nh * D:(nh + nkv) * D] = krow.repeat(nkv)
        Kc, Vc = c.K0.cuda(), c.V0.cuda()
        rc, _ = run_decode(lib, c, Kc, Vc)
        _check(rc, "ll_decode_attn_rope_qkn_bf16")
        rows = _bits(Kc[:, :, pos]).reshape(-1, D)
        assert (rows == rows[0]).all()
        stored.append(rows[0])
    c = Q.suffix_case(D, nh, nkv, 2, 2, maxlen, pos, "plain")
    c.qw, c.kw = qw, kw
    c.qkv[:, nh * D:(nh + nkv) * D] = krow.repeat(nkv)
    Kc, Vc = c.K0.cuda(), c.V0.cuda()
    cos, sin = cos1.expand(4, D).contiguous().cuda(), sin1.expand(4, D).contiguous().cuda()
    mask = (torch.arange(maxlen)[None, :] <= (pos + torch.arange(2)).repeat(2)[:, None]).cuda()
    rc, _ = run_suffix(lib, c, Kc, Vc, cos, sin, mask)
    _check(rc, "ll_suffix_attn_rope_qkn_bf16")
    rows = _bits(Kc[:, :, pos:pos + 2]).reshape(-1, D)
    assert (rows == rows[0]).all()
    stored.append(rows[0])
    assert torch.equal(stored[0], stored[1]) and torch.equal(stored[0], stored[2])
    want, _ = Q.key_candidates(krow, kw, cos1[0], sin1[0])
    assert torch.stack([stored[0] == _bits(w) for w in want]).any(0).all()


def test_null_weights_and_zero_eps_are_refused(lib):
    """LL_EINVAL from both entry points, nothing launched: the output and the caches keep their bytes"""
    D, nh, nkv, maxlen, pos = 64, 4, 2, 64, 37
    c = Q.decode_case(D, nh, nkv, maxlen, pos, "plain")
    s = Q.suffix_case(D, nh, nkv, 1, 2, maxlen, pos, "plain")
    Kc, Vc = c.K0.cuda(), c.V0.cuda()
    w = c.qw.cuda()
    qkv, cos, sin, mask = c.qkv.cuda(), c.cos.cuda(), c.sin.cuda(), c.mask.cuda()
    p = torch.tensor([pos], dtype=torch.long, device="cuda")
    out = torch.zeros(c.B * 2, nh * D, dtype=R.BF, device="cuda")
    st = _stream()
    rcs = []
    for qp, kp, eps in ((None, w.data_ptr(), Q.EPS), (w.data_ptr(), None, Q.EPS), (w.data_ptr(), w.data_ptr(), 0.0), (w.data_ptr(), w.data_ptr(), -1e-6)):
        rcs.append(lib.ll_decode_attn_rope_qkn_bf16(qkv.data_ptr(), c.ld_qkv, cos.data_ptr(), sin.data_ptr(), c.cs_stride, Kc.data_ptr(),
                                                    Vc.data_ptr(), p.data_ptr(), mask.data_ptr(), c.mask_stride, out.data_ptr(), c.B, nh, nkv,
                                                    maxlen, D, c.scale, qp, kp, eps, st))
        rcs.append(lib.ll_suffix_attn_rope_qkn_bf16(s.qkv.cuda().data_ptr(), s.ld_qkv, cos.data_ptr(), sin.data_ptr(), Kc.data_ptr(), Vc.data_ptr(),
                                                    p.data_ptr(), mask.data_ptr(), out.data_ptr(), 1, 2, nh, nkv, maxlen, D, s.scale, qp, kp, eps, st))
    torch.cuda.synchronize()
    assert rcs == [-1] * 8
    assert float(out.float().abs().max()) == 0.0
    assert torch.equal(_bits(Kc), _bits(c.K0)) and torch.equal(_bits(Vc), _bits(c.V0))
