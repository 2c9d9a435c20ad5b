"""ll_moe_route_f32 and ll_moe_experts_ex_bf16 through the C ABI against the float64 reference and rounding intervals of tests/moe2_reference.py.

Router: idx equals the reference exactly and every f32 weight lies within route_delta (relative) of the float64 weight -- a weight rounded to bf16
does not.  Experts: every output inside its interval with f32 weights (Mixtral), with the gated shared expert (Qwen2-MoE) and with both, on
groups of M rows, one row per expert and experts 0 / E - 1, at 1, 4, 5, 16, 17 and 64 rows and once at H 4104 (the wide instantiation); the
experts nobody selects hold NaN; s, g, x and the residual are strided views into poisoned memory (g a column of a wider matrix); the workspace is
poisoned before the calls.  With both options off the call gives the bits of ll_moe_experts_bf16, and a bound violated returns LL_EINVAL and
launches nothing.  Shared-expert path: the MLP half of a fused Qwen2-MoE layer with a shared expert of I_s = 192 at 1 .. 64 rows, stage by stage against
the reference (stacked router + gate logits, routing with ld = E + 1, the shared expert on the dense kernels, the gated add).

-s prints the largest position inside an interval per option."""
import pytest
import torch

from tests import linear_reference as LR
from tests import moe2_reference as M2
from tests import moe_reference as MR

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
LL_EINVAL = -1
STATS = {"mixtral": 0.0, "shared": 0.0, "both": 0.0}


@pytest.fixture(scope="module")
def lib():
    from llamole_amd import _lib
    yield _lib.load()
    print("\nlargest position inside an interval: " + ", ".join(f"{k} {v:.3f}" for k, v in STATS.items()))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _workspace(lib, c):
    n = int(lib.ll_moe_workspace_bytes(c.M, c.E, c.top_k, c.H, c.I))
    assert n > 0
    return torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda"), n      # poisoned: -1 in every int32, NaN in every bf16


def _route(lib, c, ws, n, f32):
    """(idx [M,k] int32, w [M,k] f32 or bf16): the logits are a strided view into NaN, the outputs lie in front of sentinels"""
    M, k = c.M, c.top_k
    buf, view = LR.padded(c.logits.cuda(), c.E + 5)
    idx = torch.full((M * k + 8,), -7, dtype=torch.int32, device="cuda")
    if f32:
        w = torch.full((M * k + 8,), LR.SENTINEL_F32, dtype=torch.float32, device="cuda")
        rc = lib.ll_moe_route_f32(view.data_ptr(), buf.stride(0), M, c.E, k, 1, idx.data_ptr(), w.data_ptr(), ws.data_ptr(), n, _stream())
        torch.cuda.synchronize()
        assert bool((w[M * k:] == LR.SENTINEL_F32).all())
    else:
        w = torch.full((M * k + 8,), LR.SENTINEL, dtype=torch.int16, device="cuda").view(BF)
        rc = lib.ll_moe_route_bf16(view.data_ptr(), buf.stride(0), M, c.E, k, int(c.norm_topk), idx.data_ptr(), w.data_ptr(), ws.data_ptr(), n,
                                   _stream())
        torch.cuda.synchronize()
        assert bool((w[M * k:].view(torch.int16) == LR.SENTINEL).all())
    assert rc == 0 and bool((idx[M * k:] == -7).all())
    idx, w = idx[:M * k].view(M, k).contiguous(), w[:M * k].view(M, k).contiguous()
    assert torch.equal(idx.cpu(), c.idx)
    if f32:
        assert M2.route_f32_ok(w, c.w64, c.delta) == 0
    else:
        wf = w.float().cpu()
        assert bool(((wf >= c.wlo) & (wf <= c.whi)).all())
    return idx, w


def _device_case(c):
    gbuf = torch.full((c.M + 1, c.E + 1), float("nan"), dtype=BF, device="cuda")       # g: column E of a wider matrix
    gbuf[:c.M, c.E] = c.g.cuda()
    return {"x": LR.padded(c.x.cuda(), c.H + 8), "res": LR.padded(c.res.cuda(), c.H + 16), "norm_w": LR.padded_vec(c.norm_w.cuda()),
            "wgu": c.wgu.cuda(), "wd": c.wd.cuda(), "s": LR.padded(c.s.cuda(), c.H + 24), "g": gbuf}


def _experts_ex(lib, c, dev, idx, w, w_f32, shared, ws, n):
    M, H = c.M, c.H
    out = LR.out_buffer(M, H, H + 8, device="cuda")
    s_ptr, lds, g_ptr, ldg = (dev["s"][1].data_ptr(), dev["s"][0].stride(0), dev["g"].data_ptr() + 2 * c.E, c.E + 1) if shared else (None, 0, None, 0)
    rc = lib.ll_moe_experts_ex_bf16(dev["x"][1].data_ptr(), dev["x"][0].stride(0), dev["norm_w"].data_ptr(), c.eps, idx.data_ptr(), w.data_ptr(),
                                    int(w_f32), dev["wgu"].data_ptr(), dev["wd"].data_ptr(), dev["res"][1].data_ptr(), dev["res"][0].stride(0),
                                    s_ptr, lds, g_ptr, ldg, out.data_ptr(), H + 8, M, c.E, c.top_k, H, c.I, ws.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert LR.sentinel_damage(out, M, H) == 0
    return out


@pytest.mark.parametrize("name", sorted(M2.SETS2))
def test_route_f32_and_experts_ex_against_reference(lib, name):
    c = M2.case2(name)
    assert bool(torch.isnan(c.wd[~c.used]).all()) and (not name.startswith("same") or int(c.used.sum()) == c.top_k)      # experts nobody selects hold NaN
    dev = _device_case(c)
    for key, w_f32, shared in (("mixtral", True, False), ("shared", False, True), ("both", True, True)):
        ws, n = _workspace(lib, c)
        idx, w = _route(lib, c, ws, n, w_f32)
        out = _experts_ex(lib, c, dev, idx, w, w_f32, shared, ws, n)
        bad, pos = M2.check(out[:c.M, :c.H], *c.bounds2(w.float().cpu(), w_f32, shared))
        STATS[key] = max(STATS[key], pos)
        assert bad == 0, (name, key, bad, pos)
        # the same inputs again on a fresh poisoned workspace: identical bits
        ws2, n2 = _workspace(lib, c)
        idx2, w2 = _route(lib, c, ws2, n2, w_f32)
        assert torch.equal(idx2, idx) and torch.equal(w2.view(torch.int16), w.view(torch.int16))
        out2 = _experts_ex(lib, c, dev, idx2, w2, w_f32, shared, ws2, n2)
        assert torch.equal(out2.view(torch.int16), out.view(torch.int16))


@pytest.mark.parametrize("name", ["same-M1-k2", "ends-M5-k4", "same-M64-k2", "wide-M3-k2"])
def test_both_options_off_is_ll_moe_experts_bf16(lib, name):
    c = M2.case2(name)
    dev = _device_case(c)
    ws, n = _workspace(lib, c)
    idx, w = _route(lib, c, ws, n, False)
    got = _experts_ex(lib, c, dev, idx, w, False, False, ws, n)
    ws2, n2 = _workspace(lib, c)
    idx2, w2 = _route(lib, c, ws2, n2, False)
    want = LR.out_buffer(c.M, c.H, c.H + 8, device="cuda")
    rc = lib.ll_moe_experts_bf16(dev["x"][1].data_ptr(), dev["x"][0].stride(0), dev["norm_w"].data_ptr(), c.eps, idx2.data_ptr(), w2.data_ptr(),
                                 dev["wgu"].data_ptr(), dev["wd"].data_ptr(), dev["res"][1].data_ptr(), dev["res"][0].stride(0), want.data_ptr(),
                                 c.H + 8, c.M, c.E, c.top_k, c.H, c.I, ws2.data_ptr(), n2, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert not bool(torch.isnan(got[:c.M, :c.H].float()).any())


def test_bounds_return_einval_and_launch_nothing(lib):
    c = M2.case2("same-M4-k2")
    dev = _device_case(c)
    ws, n = _workspace(lib, c)
    M, E, k, H, I = c.M, c.E, c.top_k, c.H, c.I
    idx = torch.full((1024,), -7, dtype=torch.int32, device="cuda")
    w = torch.full((1024,), LR.SENTINEL_F32, dtype=torch.float32, device="cuda")
    logits = c.logits.cuda()
    for m, e, kk, ld, nbytes in ((65, E, k, E, n), (0, E, k, E, n), (M, 257, k, 257, n), (M, E, 9, E, n), (M, 4, 5, 4, n), (M, E, k, E - 1, n),
                                 (M, E, k, E, 8)):
        rc = lib.ll_moe_route_f32(logits.data_ptr(), ld, m, e, kk, 1, idx.data_ptr(), w.data_ptr(), ws.data_ptr(), nbytes, _stream())
        torch.cuda.synchronize()
        assert rc == LL_EINVAL and bool((idx == -7).all()) and bool((w == LR.SENTINEL_F32).all()), (m, e, kk, ld, nbytes)
    out = LR.out_buffer(M, H, H, device="cuda")
    before = out.clone()
    x, res, s, g = dev["x"][1].data_ptr(), dev["res"][1].data_ptr(), dev["s"][1].data_ptr(), dev["g"].data_ptr() + 2 * E
    ldx, ldr, lds = dev["x"][0].stride(0), dev["res"][0].stride(0), dev["s"][0].stride(0)

    def call(M=M, E=E, k=k, H=H, I=I, w_f32=1, wp=w.data_ptr(), s=s, lds=lds, g=g, ldg=E + 1, ldx=ldx, ldo=H, nbytes=n, eps=c.eps):
        return lib.ll_moe_experts_ex_bf16(x, ldx, dev["norm_w"].data_ptr(), eps, idx.data_ptr(), wp, w_f32, dev["wgu"].data_ptr(),
                                          dev["wd"].data_ptr(), res, ldr, s, lds, g, ldg, out.data_ptr(), ldo, M, E, k, H, I, ws.data_ptr(), nbytes,
                                          _stream())
    bad = (dict(M=65), dict(M=0), dict(E=257), dict(k=9), dict(k=0), dict(H=H + 4), dict(H=8200), dict(I=I + 4), dict(I=32776), dict(ldx=H - 8),
           dict(ldo=H + 4), dict(nbytes=n - 16), dict(eps=0.0), dict(wp=w.data_ptr() + 2), dict(wp=None), dict(g=None), dict(lds=H - 8),
           dict(lds=H + 4), dict(ldg=0), dict(s=s + 2), dict(g=g + 1), dict(w_f32=0, s=s + 2), dict(w_f32=0, g=None))
    for kw in bad:
        assert call(**kw) == LL_EINVAL, kw
    torch.cuda.synchronize()
    assert bool((ws == 0xFF).all()) and torch.equal(out.view(torch.int16), before.view(torch.int16))          # nothing ran


# ------------------------------------------------------------------------------------------------------------------ the shared-expert path
@pytest.fixture(scope="module")
def shared_layer():
    """one fused Qwen2-MoE decoder layer with a shared expert of I_s = 192 (H 256, E 8, top-2, I 128) and every operand of its block redrawn"""
    from llamole_amd import e2e
    from llamole_amd.llm_accel import accelerate_llm, restore_decoder_layers, restore_elementwise, restore_linears, restore_model_decode
    llm = e2e.build_llm("tiny-qwen2-moe", "cuda", BF, num_hidden_layers=1, shared_expert_intermediate_size=M2.SHARED_I)
    layer = llm.model.layers[0]
    g = torch.Generator().manual_seed(41)
    draw = lambda t, scale, mean=0.0: t.copy_((mean + scale * torch.randn(t.shape, generator=g)).to(BF))
    with torch.no_grad():
        mlp, sh = layer.mlp, layer.mlp.shared_expert
        draw(layer.post_attention_layernorm.weight, 0.25, 1.0)
        draw(mlp.gate.weight, 0.2)
        draw(mlp.shared_expert_gate.weight, 0.15)
        draw(mlp.experts.gate_up_proj, 1 / 16)
        draw(mlp.experts.down_proj, 0.35)
        draw(sh.gate_proj.weight, 1 / 16)
        draw(sh.up_proj.weight, 1 / 16)
        draw(sh.down_proj.weight, 0.2)
    info = accelerate_llm(llm)
    assert info["moe_layers_fused"] == 1
    yield layer
    for restore in (restore_model_decode, restore_decoder_layers, restore_elementwise, restore_linears):
        restore(llm)


@pytest.mark.parametrize("M", M2.SHARED_ROWS)
def test_shared_expert_path_of_a_fused_layer_against_reference(lib, shared_layer, M):
    """The MLP half of a fused Qwen2-MoE layer (_FusedMoeLayer._mlp) on M rows, every stage against the float64 reference:
    the router + gate logits over the stacked [E + 1, H] copy inside linear_reference's intervals (ll_gemv_fused_bf16 up to 2 rows, HF form;
    ll_linear_rows16_bf16 beyond, staged form), the routing -- the route entry reads the [M, E + 1] logits with ld = E + 1 -- equal to the
    reference's on those logits, the shared expert's rows (the same kernels; ll_linear_rows64_bf16 on the packed copies at 17..64 rows)
    inside shared64's interval, and the output, with column E handed to the slot sum, inside finish2(..., shared=shared64(...))."""
    from llamole_amd import llm_accel
    layer, st = shared_layer, shared_layer._ll_fused
    mlp, sh, n2 = layer.mlp, layer.mlp.shared_expert, layer.post_attention_layernorm
    E, k, H = st.E, st.top_k, st.H
    assert st.shared is sh and st.Is == M2.SHARED_I and st.router_w.shape == (E + 1, H) and st.stream_ok
    form = LR.HF if M <= llm_accel.FMA_GEMV_ROWS else LR.STAGED
    x = torch.randn(M, H, generator=torch.Generator().manual_seed(500 + M)).to(BF)
    h1 = x.cuda()
    seen = {}
    orig_rl, orig_sr = st._router_logits, st._shared_rows
    st._router_logits = lambda h: seen.setdefault("logits", orig_rl(h))
    st._shared_rows = lambda h, pre2: seen.setdefault("s", orig_sr(h, pre2))
    calls = []
    st.lib = type("Spy", (), {"__getattr__": lambda self, name: (calls.append(name), getattr(lib, name))[1]})()
    try:
        pre2 = None
        if M > llm_accel.MAX_ROWS16:
            st.packed64()
            pre2 = llm_accel._prenorm64(lib, h1, n2.weight)
        out = st._mlp(h1, pre2=pre2)
        torch.cuda.synchronize()
    finally:
        st.lib = lib
        del st._router_logits, st._shared_rows
    dense = ("ll_gemv_fused_bf16" if M <= llm_accel.FMA_GEMV_ROWS else "ll_linear_rows16_bf16")
    assert calls.count("ll_moe_route_bf16") == 1 and calls[-1] == "ll_moe_experts_ex_bf16" and dense in calls
    assert ("ll_linear_rows64_bf16" in calls) == (M > llm_accel.MAX_ROWS16)
    logits, s = seen["logits"], seen["s"]
    assert logits.shape == (M, E + 1) and logits.stride(0) == E + 1 and s.shape == (M, H)
    nw, eps = n2.weight.detach().cpu(), float(n2.variance_epsilon)
    cpu = lambda t: t.detach().cpu()
    # router + gate logits: the stacked copy is [gate.weight; shared_expert_gate.weight]
    stacked = torch.cat([cpu(mlp.gate.weight), cpu(mlp.shared_expert_gate.weight)], dim=0)
    lin, err = LR.linear64(x, stacked, None, nw, eps, form)
    bad, _ = M2.check(logits.cpu(), *LR.interval(lin, err, LR.PLAIN))
    assert bad == 0, ("logits", M, bad)
    # the routing of those logits (columns 0 .. E - 1 of rows of E + 1)
    ridx, mid, lo, hi, _ = MR.route64(logits[:, :E].cpu(), k, st.norm_topk)
    assert torch.equal(st.idx[:M].cpu(), ridx)
    w = st.w[:M].float().cpu()
    assert bool(((w >= lo) & (w <= hi)).all())
    # the shared expert and its gate
    shared = M2.shared64(x, nw, eps, cpu(sh.gate_proj.weight), cpu(sh.up_proj.weight), cpu(sh.down_proj.weight), cpu(mlp.shared_expert_gate.weight),
                         form=form)
    sd, gd = s.cpu().to(torch.float64), logits[:, E].cpu().to(torch.float64)
    assert bool(((sd >= shared[0]) & (sd <= shared[1])).all()), ("s", M)
    assert bool(((gd >= shared[3]) & (gd <= shared[4])).all()), ("g", M)
    # the output: experts on the routing above, the gated shared expert, the residual h1
    _, _, _, ylo, yhi, ymid = MR.experts_ay(x, nw, eps, ridx, cpu(mlp.experts.gate_up_proj), cpu(mlp.experts.down_proj))
    bounds = M2.finish2(ylo, yhi, ymid, w, x, w_f32=False, shared=shared)
    bad, pos = M2.check(out.cpu(), *bounds)
    STATS["shared"] = max(STATS["shared"], pos)
    assert bad == 0, ("out", M, bad, pos)
    # and not inside them with the gate dropped: the case can tell
    wrong = M2.finish2(ylo, yhi, ymid, w, x, w_f32=False, shared=shared, gate="dropped")[2]
    assert M2.check(wrong, *bounds)[0] > 0
