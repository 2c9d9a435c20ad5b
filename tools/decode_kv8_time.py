"""Decode token on the bf16 static cache against the MX8 KV cache (GraphedDecoder(..., kv_cache="mxfp8")) at Llama-3.1-8B widths with the
published llama3 rope scaling (e2e.LLAMA31_ROPE; random bf16 weights), one model, both caches in one process:
python tools/decode_kv8_time.py [--out profiles/decode_kv8_time.txt] [--steps N] [--shapes 4096x16,4096x64,32768x1,32768x16,131072x1]
                                [--probe 131072x16] [--arch llama-3.1-8b] [--layers L]
(--arch: any Llama-layout entry of e2e.LLM_CONFIGS, e.g. tiny-llama for a dry run; --layers: fewer decoder layers, stated in the output;
--probe none: skip the capacity probe).
Per shape (slots x rows) each decoder prefills a 16-token prompt into a cache of that many slots (HF's modules; not what is measured), the slots
behind it are filled -- N(0, 1) rows in the bf16 cache, random finite codes and scale bytes near 2^0 in the MX8 cache -- and the position
counters are set to slots - 2 * steps - 8, so the timed steps run near the end of the cache and stay inside it.  One decode step (the decoder's
own `_step` plus the counter increments) is captured as a hipGraph after an eager warm-up that is checked on the host (the shared counter
moved by one slot, the fused decode served the step); a figure is the time of `steps` replays over steps, by device events.  Three alternated
repeats per cache type: the median with (min - max).  NO time is a pass condition: the ratios are stated as measured, slower ones included.
Then the attention call alone on either cache -- what the fused layer routes to: the one-workgroup entries up to 16384 bf16 slots, the
key-split entry beyond, ll_decode_attn_rope_kv8 on MX8 at every length -- over the layers' caches in turn (they exceed the Infinity Cache
several times), with the bytes per second over the visible K / V bytes it reads, and the cache bytes of either type.  Last, the capacity
probe: whether a shape whose bf16 cache does not fit beside the weights (131072 slots x 16 rows: 275 GB) now runs on the MX8 cache at all."""
import gc
import os
import sys

os.environ.setdefault("LLAMOLE_TUNING", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llamole_amd import e2e  # noqa: E402
from llamole_amd.llm_accel import accelerate_llm  # noqa: E402
from llamole_amd.llm_decode import GraphedDecoder  # noqa: E402

argv = sys.argv[1:]
steps = int(argv[argv.index("--steps") + 1]) if "--steps" in argv else 16
out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join("profiles", "decode_kv8_time.txt")


def _shapes(text):
    return tuple(tuple(int(v) for v in x.split("x")) for x in text.split(",")) if text != "none" else ()


shapes = _shapes(argv[argv.index("--shapes") + 1] if "--shapes" in argv else "4096x16,4096x64,32768x1,32768x16,131072x1")
probe = _shapes(argv[argv.index("--probe") + 1] if "--probe" in argv else "131072x16")
arch = argv[argv.index("--arch") + 1] if "--arch" in argv else "llama-3.1-8b"
over = {"num_hidden_layers": int(argv[argv.index("--layers") + 1])} if "--layers" in argv else {}
REPEATS = 3
PROMPT = 16
torch.set_grad_enabled(False)       # as under GraphedDecoder.generate: with gradients on, every fused path declines to HF's modules
WINDOW_MS = 100.0       # timed window of the kernel-alone figures
CACHES = (("bf16", None), ("mxfp8", "mxfp8"))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def flush():
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def cache_bytes(cache):
    ts = []
    for l in cache.layers:
        ts += [l.keys, l.values] + [getattr(l, a) for a in ("key_scales", "value_scales") if hasattr(l, a)]
    return sum(t.numel() * t.element_size() for t in ts)


class Stepper:
    """one decoder on a cache of `slots` slots x `rows` rows, its decode step captured, positioned 2 `steps` + 8 slots before the end"""

    def __init__(self, llm, kv_cache, slots, rows):
        self.dec = dec = GraphedDecoder(llm, use_graph=False, fused_cache=True, kv_cache=kv_cache)
        dec.len_bucket = slots
        prompt = torch.randint(5, min(30000, llm.config.vocab_size), (rows, PROMPT), generator=torch.Generator().manual_seed(rows)).cuda()
        dec.generate(prompt, torch.ones_like(prompt), max_new_tokens=2, pad_token_id=0, eos_token_id=[], do_sample=False)
        assert dec.cache.layers[0].keys.shape[2] == slots
        for layer in dec.cache.layers:
            if kv_cache is None:
                layer.keys[:, :, PROMPT:].normal_()
                layer.values[:, :, PROMPT:].normal_()
            else:
                layer.keys[:, :, PROMPT:].random_(0, 0x7e)           # finite E4M3 codes
                layer.values[:, :, PROMPT:].random_(0, 0x7e)
                layer.key_scales[:, :, PROMPT:].random_(120, 128)
                layer.value_scales[:, :, PROMPT:].random_(120, 128)
        self.start = slots - 2 * steps - 8
        self.base = getattr(llm, "model", llm)
        self.rewind()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self.body()
        torch.cuda.current_stream().wait_stream(s)
        got = int(dec.cache.layers[0].cumulative_length)
        if got != self.start + 1:
            raise RuntimeError(f"one decode step moved the cache position from {self.start} to {got}: not the decoder's own step")
        if not self.base.__dict__.get("_ll_decode", {}).get("served"):
            raise RuntimeError("the fused decode did not serve the step")
        self.rewind()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.body()

    def rewind(self):
        for layer in self.dec.cache.layers:
            layer.cumulative_length.fill_(self.start)
        self.dec.pos.fill_(self.start)
        self.dec.posid.fill_(self.start)

    def body(self):
        self.dec._step()
        self.dec.pos.add_(1)
        self.dec.posid.add_(1)

    def token_ms(self):
        self.rewind()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            self.graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps


def window(fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def timed_us(fn, calls_per_fn):
    window(fn, 1)
    inner = max(2, int(WINDOW_MS / max(window(fn, 1), 1e-3)) + 1)
    reps = [1000 * window(fn, inner) / (inner * calls_per_fn) for _ in range(REPEATS)]
    return sorted(reps)[1], min(reps), max(reps), inner * calls_per_fn


def attention_alone(llm, cache, slots, rows, pos):
    """the attention call of every fused layer on its own cache, one layer after the other: what the layer routes this cache to"""
    sts = [l._ll_fused for l in llm.model.layers]
    st0 = sts[0]
    nqkv = st0.nq + 2 * st0.nkv_dim
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(rows, nqkv, generator=g).to(torch.bfloat16).cuda()
    ang = torch.rand(1, 1, st0.D, generator=g) * 6.28
    pe = (ang.cos().to(torch.bfloat16).cuda(), ang.sin().to(torch.bfloat16).cuda())
    mask = torch.zeros(rows, 1, 1, slots, dtype=torch.bool, device="cuda")
    mask[..., :pos + 1] = True
    for layer in cache.layers:
        layer.cumulative_length.fill_(pos)

    def all_layers():
        for st in sts:
            st._attn(qkv, nqkv, mask, cache, pe, rows, "cuda")
    med, lo, hi, calls = timed_us(all_layers, len(sts))
    row_bytes = st0.D + st0.D // 32 if hasattr(cache.layers[0], "key_scales") else 2 * st0.D
    nbytes = 2 * rows * st0.nkv * (pos + 1) * row_bytes
    return med, lo, hi, calls, nbytes, len(sts)


def entry_name(st, cache, slots):
    from llamole_amd.llm_accel import ATTN_MAXLEN
    if hasattr(cache.layers[0], "key_scales"):
        return "ll_decode_attn_rope_kv8"
    return "ll_decode_attn_rope_split_bf16" if slots > ATTN_MAXLEN else "ll_decode_attn_rope_bf16"


say(f"# decode token at {arch} widths{' with ' + str(over['num_hidden_layers']) + ' decoder layers' if over else ''}, llama3 rope: the fused "
    f"stack on the bf16 static cache against the same stack on the MX8 KV cache (kv_cache=\"mxfp8\": E4M3 codes + one E8M0 scale per 32 "
    f"elements of head_dim)")
say(f"# per figure {steps} replays of the captured decode step from slot slots - {2 * steps + 8} on, device events; {REPEATS} alternated repeats: "
    f"median (min - max).  No time is a pass condition.")
llm = e2e.build_llm(arch, "cuda", torch.bfloat16, rope_parameters=e2e.LLAMA31_ROPE, **over)
info = accelerate_llm(llm)
say(f"# {type(llm).__name__}, {llm.config.num_hidden_layers} layers, decoder_layers_5_launches {info.get('decoder_layers_5_launches')}, "
    f"decode_prologue_1_launch {info.get('decode_prologue_1_launch')}")
for slots, rows in shapes:
    tag = f"{arch} {slots} slots x {rows:2d} rows"
    steppers = {}
    for name, kind in CACHES:
        st = steppers[name] = Stepper(llm, kind, slots, rows)
        say(f"# {tag} {name}: cache {cache_bytes(st.dec.cache) / 1e9:.3f} GB"
            + (f" + one staging pair {sum(t.numel() * 2 for t in st.dec.cache.staging) / 1e9:.3f} GB" if kind else ""))
        st.token_ms()                            # warm-up of the replay
    res = {name: [] for name, _ in CACHES}
    for _ in range(REPEATS):
        for name, _ in CACHES:
            res[name].append(steppers[name].token_ms())
    med = {}
    for name, _ in CACHES:
        v = res[name]
        med[name] = sorted(v)[len(v) // 2]
        say(f"{tag} {name}: decode token median {med[name]:.4f} ms (runs {', '.join(f'{x:.4f}' for x in v)}; min {min(v):.4f} - max {max(v):.4f})")
    b, m = res["bf16"], res["mxfp8"]
    verdict = "every mxfp8 repeat is faster than every bf16 repeat" if max(m) < min(b) else \
        ("every mxfp8 repeat is SLOWER than every bf16 repeat" if min(m) > max(b) else "the repeats overlap: no difference beyond the spread")
    say(f"{tag}: mxfp8 / bf16 = {med['mxfp8'] / med['bf16']:.3f} by the medians; {verdict}; cache bytes mxfp8 / bf16 = "
        f"{cache_bytes(steppers['mxfp8'].dec.cache) / cache_bytes(steppers['bf16'].dec.cache):.4f}")
    pos = slots - 9
    alone = {}
    for name, _ in CACHES:
        cache = steppers[name].dec.cache
        a_med, a_lo, a_hi, calls, nbytes, nl = attention_alone(llm, cache, slots, rows, pos)
        alone[name] = a_med
        say(f"{tag} {name}: {entry_name(llm.model.layers[0]._ll_fused, cache, slots)} alone, *pos = {pos}: median {a_med:.1f} us (min {a_lo:.1f} - "
            f"max {a_hi:.1f}) per call over {nl} layers' caches in turn, {calls} calls per window; {nbytes / 1e6:.1f} MB of visible K / V bytes = "
            f"{nbytes / a_med / 1e6:.2f} TB/s; x {nl} layers = {a_med * nl / 1000:.3f} ms of the {med[name]:.4f} ms token")
    say(f"{tag}: attention call alone, mxfp8 / bf16 = {alone['mxfp8'] / alone['bf16']:.3f}")
    flush()
    del steppers, st, cache
    gc.collect()                                 # a cache and its layers refer to each other
    torch.cuda.empty_cache()
for slots, rows in probe:
    tag = f"{arch} {slots} slots x {rows:2d} rows"
    cfg = llm.config
    D = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
    bf16_gb = 2 * cfg.num_hidden_layers * rows * cfg.num_key_value_heads * slots * D * 2 / 1e9
    free, total = (x / 1e9 for x in torch.cuda.mem_get_info())
    say(f"# {tag}: a bf16 cache would take {bf16_gb:.1f} GB; the device has {free:.1f} GB free of {total:.1f} GB beside the weights")
    try:
        st = Stepper(llm, "mxfp8", slots, rows)
        st.token_ms()
        v = [st.token_ms() for _ in range(REPEATS)]
        say(f"{tag} mxfp8: RUNS: cache {cache_bytes(st.dec.cache) / 1e9:.3f} GB + one staging pair "
            f"{sum(t.numel() * 2 for t in st.dec.cache.staging) / 1e9:.3f} GB; decode token median {sorted(v)[1]:.4f} ms (min {min(v):.4f} - max {max(v):.4f})")
        del st
    except (RuntimeError, torch.OutOfMemoryError) as e:
        say(f"{tag} mxfp8: does NOT run: {type(e).__name__}: {(str(e).splitlines() or [''])[0][:160]}")
    gc.collect()
    torch.cuda.empty_cache()
    flush()
flush()
