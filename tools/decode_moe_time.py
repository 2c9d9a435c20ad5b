"""Decode token of the graphed decoder on a sparse-MoE model at Qwen3-30B-A3B widths, or with --model at Mixtral-8x7B / Qwen1.5-MoE-A2.7B
widths (random bf16 weights, the router drawn wider than HF's init so that the routing is not a near-tie everywhere):
python tools/decode_moe_time.py [--out profiles/decode_moe_time.txt] [--new N] [--rows 1,16,64] [--model qwen3-30b-a3b] [--layers L] [--append]
(--model, or --arch: any sparse-MoE entry of e2e.LLM_CONFIGS -- qwen3-30b-a3b, mixtral-8x7b, qwen1.5-moe-a2.7b, or a tiny one for a dry run;
--layers: fewer decoder layers, stated in the output; --append: add to --out instead of replacing it).
Two models with the same weights live in one process:
  (i)   the fused stack: MoE layers as eight launches (ll_moe_route_bf16 / ll_moe_experts_bf16; Mixtral: ll_moe_route_f32 /
        ll_moe_experts_ex_bf16; Qwen2-MoE: ten, with the shared expert's two Linears), one-launch prologue;
  (ii)  accelerate_llm(layers=False): what such a model ran before its layers were accepted -- fused Linears, RMSNorm, rotary and attention
        kernels op by op under HF's layer code, HF's experts code (config._experts_implementation is recorded) per layer.
Per row count both see the same prompts; the token time is (generate(1 + n) - generate(1)) / n, median of 3, greedy, after a 128-token prompt,
the cases taken alternately over three repeats after a warm-up of both.  For (i) the file also gives the bytes of weights one decode step
touches -- the distinct experts per layer counted from the routing (`idx`) of the last step, read after the run -- and the TB/s that implies.
Then the experts call alone (ll_moe_experts_bf16, for Mixtral ll_moe_experts_ex_bf16 with f32 weights; without the shared expert; HIP events, cycling through the layers' expert matrices so that no launch finds its weights in the Infinity
Cache) at 1 / 16 / 64 rows with a routing drawn uniformly and with all rows on the same top_k experts."""
import os
import sys

os.environ.setdefault("LLAMOLE_TUNING", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llamole_amd import _lib, e2e  # noqa: E402
from llamole_amd.llm_accel import accelerate_llm  # noqa: E402
from llamole_amd.llm_decode import GraphedDecoder  # noqa: E402

argv = sys.argv[1:]
n = int(argv[argv.index("--new") + 1]) if "--new" in argv else 128
out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join("profiles", "decode_moe_time.txt")
rows = tuple(int(x) for x in argv[argv.index("--rows") + 1].split(",")) if "--rows" in argv else (1, 16, 64)
arch = next((argv[argv.index(f) + 1] for f in ("--model", "--arch") if f in argv), "qwen3-30b-a3b")
over = {"num_hidden_layers": int(argv[argv.index("--layers") + 1])} if "--layers" in argv else {}
REPEATS = 3
WINDOW_MS = 100.0       # timed window of the kernel-alone figures
lines = []
if "--append" in argv and os.path.exists(out_path):       # keep what an earlier run (another --model) wrote
    with open(out_path) as fh:
        lines = fh.read().splitlines() + [""]


def say(s):
    print(s, flush=True)
    lines.append(s)


def flush():
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def build():
    llm = e2e.build_llm(arch, "cuda", torch.bfloat16, **over)
    e2e.randomize_head_norms(llm)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for layer in llm.model.layers:
            if hasattr(layer.mlp, "gate"):
                layer.mlp.gate.weight.copy_((torch.randn(layer.mlp.gate.weight.shape, generator=g) * 0.2).to(torch.bfloat16))
    return llm


def gen_ms(dec, prompt, new):
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dec.generate(prompt, torch.ones_like(prompt), max_new_tokens=new, pad_token_id=0, eos_token_id=[], do_sample=False)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[1]


def step_bytes(llm, B):
    """bytes of weights one decode step of the fused model reads: attention and router matrices, norms, lm_head, the B embedding rows and the
    DISTINCT experts each MoE layer selected in its last step (st.idx[:B]); returns (bytes, mean distinct experts per MoE layer)"""
    total, distinct = 0, []
    for layer in llm.model.layers:
        st = layer._ll_fused
        total += st.wqkv.numel() + st.wo.numel() + st.n1.weight.numel() + st.n2.weight.numel()
        total += sum(m.weight.numel() for m in (st.qn, st.kn) if m is not None)
        if hasattr(st, "experts"):
            k = int(st.idx[:B].flatten().unique().numel())
            distinct.append(k)
            total += st.router.weight.numel() + k * 3 * st.I * st.H
            if st.shared is not None:       # the shared expert's three matrices and its gate row, read at every step
                total += st.wgu_s.numel() + st.wdown_s.numel() + st.H
        else:
            total += st.wgu.numel() + st.wdown.numel()
    total += llm.lm_head.weight.numel() + llm.model.norm.weight.numel() + B * llm.config.hidden_size
    return 2 * total, (sum(distinct) / len(distinct) if distinct else 0.0)


def experts_alone(llm):
    """ll_moe_experts_bf16 (three launches) on the model's own expert matrices, one layer after the other"""
    lib = _lib.load()
    sts = [l._ll_fused for l in llm.model.layers if hasattr(l._ll_fused, "experts")]
    st0 = sts[0]
    E, k, H, I = st0.E, st0.top_k, st0.H, st0.I
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(7)
    for M in rows:
        x = torch.randn(M, H, generator=g).to(torch.bfloat16).cuda()
        out = torch.empty_like(x)
        for kind in ("uniform", "same experts"):
            logits = torch.randn(M, E, generator=g)
            if kind == "same experts":
                logits = logits[:1].repeat(M, 1)
            logits = logits.to(torch.bfloat16).cuda()
            route = lib.ll_moe_route_f32 if st0.w_f32 else lib.ll_moe_route_bf16
            _lib.check(route(logits.data_ptr(), E, M, E, k, 1, st0.idx.data_ptr(), st0.w.data_ptr(), st0.ws.t.data_ptr(), st0.ws.bytes, stream),
                       "ll_moe_route")
            distinct = int(st0.idx[:M].flatten().unique().numel())

            def run(st):
                _lib.check(lib.ll_moe_experts_ex_bf16(x.data_ptr(), H, st.n2.weight.data_ptr(), st.eps2, st0.idx.data_ptr(), st0.w.data_ptr(),
                                                      int(st0.w_f32), st.experts.gate_up_proj.data_ptr(), st.experts.down_proj.data_ptr(),
                                                      x.data_ptr(), H, None, 0, None, 0, out.data_ptr(), H, M, E, k, H, I, st0.ws.t.data_ptr(),
                                                      st0.ws.bytes, stream), "ll_moe_experts_ex_bf16")
            def window(inner):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(inner):
                    for st in sts:
                        run(st)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1)
            window(1)                                    # warm-up of every layer's matrices and of the kernel variants
            inner = max(4, int(WINDOW_MS / max(window(1), 1e-3)) + 1)      # enough passes over the layers for a window of >= WINDOW_MS
            reps = [1000 * window(inner) / (inner * len(sts)) for _ in range(REPEATS)]
            med = sorted(reps)[1]
            nbytes = 2 * distinct * 3 * I * H
            label = ("ll_moe_experts_ex_bf16 (f32 weights)" if st0.w_f32 else
                     "ll_moe_experts_ex_bf16 (no option: it forwards to ll_moe_experts_bf16)")
            say(f"{label} alone, rows {M:2d}, {kind}: {distinct} distinct experts ({nbytes / 1e6:.1f} MB of expert weights), median "
                f"{med:.1f} us (min {min(reps):.1f} - max {max(reps):.1f}) over {len(sts)} layers' matrices in turn, {inner * len(sts)} calls per window = "
                f"{nbytes / med / 1e6:.2f} TB/s")


# the entry points a fused MoE layer of this model's family calls (llm_accel._FusedMoeLayer._mlp)
ENTRIES = {"Mixtral": "ll_moe_route_f32 / ll_moe_experts_ex_bf16 with f32 weights",
           "Qwen2Moe": "ll_moe_route_bf16 / ll_moe_experts_ex_bf16 with the shared expert"}.get(e2e.LLM_CONFIGS[arch]["cls"],
                                                                                             "ll_moe_route_bf16 / ll_moe_experts_bf16")
say(f"# decode token at {arch} widths{' with ' + str(over['num_hidden_layers']) + ' decoder layers' if over else ''}: sparse-MoE layers fused "
    f"({ENTRIES}) against the same model with accelerate_llm(layers=False)")
say(f"# n = {n} tokens after a 128-token prompt, greedy, median of 3 per figure, {REPEATS} alternated repeats")
CASES = (("(i) fused", {}), ("(ii) layers=False", dict(layers=False)))
models, llms = {}, {}
for name, accel_kw in CASES:
    llm = build()
    info = accelerate_llm(llm, **accel_kw)
    llms[name] = llm
    models[name] = GraphedDecoder(llm, use_graph=True, fused_cache=bool(info.get("decode_attention")))
    say(f"# {name}: {type(llm).__name__}, {llm.config.num_hidden_layers} layers, decoder_layers_5_launches {info.get('decoder_layers_5_launches')}, "
        f"moe_layers_fused {info.get('moe_layers_fused')}, decode_prologue_1_launch {info.get('decode_prologue_1_launch')}, "
        f"declined {info.get('decoder_layers_declined')}, config._experts_implementation {llm.config._experts_implementation}")
for B in rows:
    prompt = torch.randint(5, min(30000, llms["(i) fused"].config.vocab_size), (B, 128), generator=torch.Generator().manual_seed(B)).cuda()
    for name, _ in CASES:                        # warm-up of every case: capture both lengths
        captured = None
        for new in (1 + n, 1):
            models[name].generate(prompt, torch.ones_like(prompt), max_new_tokens=new, pad_token_id=0, eos_token_id=[], do_sample=False)
            if captured is None:         # read behind the long call: a call of another cache length prepares the decoder anew
                captured = models[name]._graph is not None
        say(f"# rows {B:2d} {name}: decode step captured = {captured}")
    res = {name: [] for name, _ in CASES}
    for _ in range(REPEATS):
        for name, _ in CASES:
            res[name].append((gen_ms(models[name], prompt, 1 + n) - gen_ms(models[name], prompt, 1)) / n)
    med = {}
    for name, _ in CASES:
        v = res[name]
        med[name] = sorted(v)[len(v) // 2]
        say(f"{arch} rows {B:2d} {name}: decode token median {med[name]:.4f} ms (runs {', '.join(f'{x:.4f}' for x in v)}; min {min(v):.4f} - max {max(v):.4f})")
    f, u = (res[name] for name, _ in CASES)
    say(f"{arch} rows {B:2d}: (ii) / (i) = {med['(ii) layers=False'] / med['(i) fused']:.3f} x by the medians; every (i) repeat "
        f"{'IS FASTER than' if max(f) < min(u) else 'is NOT faster than'} every (ii) repeat ([{min(f):.4f}, {max(f):.4f}] against [{min(u):.4f}, {max(u):.4f}])")
    nbytes, distinct = step_bytes(llms["(i) fused"], B)
    say(f"{arch} rows {B:2d} (i): {distinct:.1f} distinct experts per MoE layer in the last step, {nbytes / 1e9:.3f} GB of weights per step = "
        f"{nbytes / med['(i) fused'] / 1e9:.3f} TB/s at the median")
    flush()
experts_alone(llms["(i) fused"])
flush()
