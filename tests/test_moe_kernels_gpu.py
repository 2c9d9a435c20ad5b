"""ll_moe_route_bf16 and ll_moe_experts_bf16 through the C ABI against the float64 reference and rounding intervals of tests/moe_reference.py.

Router: idx must equal the reference exactly, every weight must be one of its accepted bf16 values (one value, or the two neighbours inside the
f32 window); known-answer rows for ties and a dominant logit; strided logits inside a NaN-filled buffer; LL_EINVAL outside the bounds.
Experts: every output inside its interval on every routing shape (random, one group of M rows, one row per expert, experts 0 and E - 1, experts
nobody selects -- whose matrices are NaN, so a wrong expert index gives NaN), one-hot probes, operands as strided views into poisoned memory,
the workspace poisoned before the calls, two calls bit-identical, and a row that is alone on its expert bit for bit the dense ll_gemv_fused_bf16.

-s prints the number of router weights that used the two-value window and the largest position inside an experts interval."""
import pytest
import torch

from tests import linear_reference as LR
from tests import moe_reference as MR

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
LL_EINVAL = -1
STATS = {"route_free": 0, "route_total": 0, "route_off_mid": 0, "experts_worst": 0.0}


@pytest.fixture(scope="module")
def lib():
    from llamole_amd import _lib
    yield _lib.load()
    print(f"\nrouter weights: {STATS['route_total']} checked, {STATS['route_free']} had two accepted values, {STATS['route_off_mid']} differ from "
          f"bf16(float64 value); largest position inside an experts interval {STATS['experts_worst']:.3f}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _workspace(lib, M, E, k, H, I):
    n = int(lib.ll_moe_workspace_bytes(M, E, k, H, I))
    assert n > 0
    return torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda"), n      # poisoned: -1 in every int32, NaN in every bf16


def _route(lib, logits, k, norm, ws, nbytes, ld=None):
    """logits [M, E] on the host -> (rc, idx [M, k], w [M, k]); the logits are a strided view into NaN, the outputs lie in front of sentinels"""
    M, E = logits.shape
    buf, view = LR.padded(logits.cuda(), ld or E + 5)
    idx = torch.full((M * k + 8,), -7, dtype=torch.int32, device="cuda")
    w = torch.full((M * k + 8,), LR.SENTINEL, dtype=torch.int16, device="cuda").view(BF)
    rc = lib.ll_moe_route_bf16(view.data_ptr(), buf.stride(0), M, E, k, int(norm), idx.data_ptr(), w.data_ptr(), ws.data_ptr(), nbytes, _stream())
    torch.cuda.synchronize()
    assert bool((idx[M * k:] == -7).all()) and bool((w[M * k:].view(torch.int16) == LR.SENTINEL).all())
    return rc, idx[:M * k].view(M, k), w[:M * k].view(M, k)


def _check_route(idx, w, ref):
    _, ridx, mid, lo, hi, free = ref
    assert torch.equal(idx.cpu(), ridx)
    wf = w.float().cpu()
    assert bool(((wf >= lo) & (wf <= hi)).all()), (wf - mid).abs().max()
    STATS["route_total"] += ridx.numel()
    STATS["route_free"] += free
    STATS["route_off_mid"] += int((wf != mid).sum())


@pytest.mark.parametrize("E", MR.ROUTE_E)
@pytest.mark.parametrize("k", MR.ROUTE_K)
def test_route_against_reference(lib, E, k):
    for M in MR.ROUTE_M:
        for norm in (True, False):
            ref = MR.route_case(E, k, M, norm)
            ws, n = _workspace(lib, M, E, k, 8, 8)
            rc, idx, w = _route(lib, ref[0], k, norm, ws, n)
            assert rc == 0, (E, k, M)
            _check_route(idx, w, ref)


def test_route_known_answers(lib):
    ws, n = _workspace(lib, 2, 8, 3, 8, 8)
    # equal logits across the k-th boundary: the lower index wins; the descending order holds among the selected
    tie = torch.tensor([[0.0, 1.0, 3.0, 1.0, 1.0, -2.0, 0.5, 1.0], [2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0]]).to(BF)
    rc, idx, w = _route(lib, tie, 3, True, ws, n)
    assert rc == 0 and idx.tolist() == [[2, 1, 3], [0, 1, 2]]
    assert w[1].float().tolist() == [float(torch.tensor(1 / 3).to(BF))] * 3
    _check_route(idx, w, (tie,) + MR.route64(tie, 3, True))
    # one dominant logit: weight 1, the rest by their exact ratios (no renormalisation: the probabilities themselves)
    dom = torch.tensor([[-60.0, 2.0, 64.0, 1.0, -60.0, 0.0, -60.0, -60.0]]).to(BF)
    rc, idx, w = _route(lib, dom, 3, False, ws, n)
    assert rc == 0 and idx.tolist() == [[2, 1, 3]] and float(w[0, 0]) == 1.0
    _check_route(idx, w, (dom,) + MR.route64(dom, 3, False))
    assert abs(float(w[0, 2]) / float(w[0, 1]) - 0.36787944) < 2 ** -7


def test_route_bounds_return_einval_and_launch_nothing(lib):
    ws, n = _workspace(lib, 64, 256, 8, 8, 8)
    for M, E, k in ((65, 8, 2), (4, 257, 2), (4, 16, 9), (4, 4, 5), (0, 8, 2), (4, 8, 0)):
        logits = torch.zeros(max(M, 1), E, dtype=BF)
        buf = logits.cuda()
        idx = torch.full((1024,), -7, dtype=torch.int32, device="cuda")
        w = torch.zeros(1024, dtype=BF, device="cuda")
        rc = lib.ll_moe_route_bf16(buf.data_ptr(), E, M, E, k, 1, idx.data_ptr(), w.data_ptr(), ws.data_ptr(), n, _stream())
        torch.cuda.synchronize()
        assert rc == LL_EINVAL and bool((idx == -7).all()), (M, E, k)
        assert lib.ll_moe_workspace_bytes(M, E, k, 256, 128) == -1
        rc = lib.ll_moe_experts_bf16(buf.data_ptr(), 256, buf.data_ptr(), 1e-6, idx.data_ptr(), w.data_ptr(), buf.data_ptr(), buf.data_ptr(),
                                     buf.data_ptr(), 256, buf.data_ptr(), 256, M, E, k, 256, 128, ws.data_ptr(), n, _stream())
        assert rc == LL_EINVAL
    assert bool((ws == 0xFF).all())          # nothing ran


def _experts(lib, c, dev, idx, w, ws, n):
    """one ll_moe_experts_bf16 call on strided views; returns the output allocation [M + 1, H + 8]"""
    M, H = c.M, c.H
    out = LR.out_buffer(M, H, H + 8, device="cuda")
    rc = lib.ll_moe_experts_bf16(dev["x"][1].data_ptr(), dev["x"][0].stride(0), dev["norm_w"].data_ptr(), c.eps, idx.data_ptr(), w.data_ptr(),
                                 dev["wgu"].data_ptr(), dev["wd"].data_ptr(), dev["res"][1].data_ptr(), dev["res"][0].stride(0), out.data_ptr(),
                                 H + 8, M, c.E, c.top_k, H, c.I, ws.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return out


def _device_case(c):
    return {"x": LR.padded(c.x.cuda(), c.H + 8), "res": LR.padded(c.res.cuda(), c.H + 16), "norm_w": LR.padded_vec(c.norm_w.cuda()),
            "wgu": c.wgu.cuda(), "wd": c.wd.cuda()}


def _routed(lib, c):
    ws, n = _workspace(lib, c.M, c.E, c.top_k, c.H, c.I)
    rc, idx, w = _route(lib, c.logits, c.top_k, c.norm_topk, ws, n)
    assert rc == 0
    _check_route(idx, w, (c.logits, c.idx, c.w, c.wlo, c.whi, c.free))
    return idx.contiguous(), w.contiguous(), ws, n


@pytest.mark.parametrize("name", sorted(MR.EXPERT_SETS))
def test_experts_against_reference(lib, name):
    c = MR.experts_case(name)
    dev = _device_case(c)
    idx, w, ws, n = _routed(lib, c)
    out = _experts(lib, c, dev, idx, w, ws, n)
    assert LR.sentinel_damage(out, c.M, c.H) == 0
    bad, pos = MR.check(out[:c.M, :c.H], *c.bounds(w.float().cpu()))
    STATS["experts_worst"] = max(STATS["experts_worst"], pos)
    assert bad == 0, (name, bad, pos)
    # the same inputs again (a fresh poisoned workspace, routed again): identical bits
    ws2, n2 = _workspace(lib, c.M, c.E, c.top_k, c.H, c.I)
    rc, idx2, w2 = _route(lib, c.logits, c.top_k, c.norm_topk, ws2, n2)
    assert rc == 0 and torch.equal(idx2, idx) and torch.equal(w2.view(torch.int16), w.view(torch.int16))
    out2 = _experts(lib, c, dev, idx2.contiguous(), w2.contiguous(), ws2, n2)
    assert torch.equal(out2.view(torch.int16), out.view(torch.int16))


@pytest.mark.parametrize("name", ["distinct-M4-k2", "distinct-M16-k8", "wide-M1-k8", "random-M1"])
def test_a_row_alone_on_its_expert_equals_the_dense_gemv(lib, name):
    """every (row, slot) pair of these cases has its expert to itself: ll_gemv_fused_bf16 on that expert's matrices, then the contract's tail in
    torch (exact f32 products, the slot sum in slot order), must give the same bits"""
    c = MR.experts_case(name)
    assert c.idx.flatten().unique().numel() == c.idx.numel()
    dev = _device_case(c)
    idx, w, ws, n = _routed(lib, c)
    out = _experts(lib, c, dev, idx, w, ws, n)[:c.M, :c.H]
    x, nw = c.x.cuda().contiguous(), c.norm_w.cuda().contiguous()
    want = torch.empty(c.M, c.H, dtype=BF, device="cuda")
    for m in range(c.M):
        s = torch.zeros(c.H, dtype=torch.float32, device="cuda")
        for j in range(c.top_k):
            e = int(c.idx[m, j])
            a = torch.empty(1, c.I, dtype=BF, device="cuda")
            y = torch.empty(1, c.H, dtype=BF, device="cuda")
            rc = lib.ll_gemv_fused_bf16(x[m].data_ptr(), c.H, dev["wgu"][e].data_ptr(), c.H, None, nw.data_ptr(), c.eps, None, 0, a.data_ptr(), c.I,
                                        1, c.I, c.H, 2, _stream())
            assert rc == 0
            rc = lib.ll_gemv_fused_bf16(a.data_ptr(), c.I, dev["wd"][e].data_ptr(), c.I, None, None, 0.0, None, 0, y.data_ptr(), c.H, 1, c.H, c.I,
                                        0, _stream())
            assert rc == 0
            s = s + (w[m, j].float() * y[0].float()).to(BF).float()
        want[m] = (c.res[m].cuda().float() + s.to(BF).float()).to(BF)
    torch.cuda.synchronize()
    assert torch.equal(out.contiguous().view(torch.int16), want.view(torch.int16))
