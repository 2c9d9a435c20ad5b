"""Decode token on static caches beyond 16384 slots at Llama-3.1-8B widths with the published llama3 rope scaling (e2e.LLAMA31_ROPE; random
bf16 weights):
python tools/decode_longctx_time.py [--out profiles/decode_longctx_time.txt] [--steps N] [--shapes 32768x1,32768x16,131072x1]
                                    [--arch llama-3.1-8b] [--layers L]
(--arch: any Llama-layout entry of e2e.LLM_CONFIGS, e.g. tiny-llama for a dry run; --layers: fewer decoder layers, stated in the output).
Two models with the same weights live in one process:
  (i)   the fused stack: five-launch layers whose attention is the key-split pair of launches (ll_decode_attn_rope_split_bf16);
  (ii)  accelerate_llm(layers=False): HF's layer code per token, and HF's own sdpa attention -- the registered decode attention declines beyond
        16384 slots -- i.e. the only thing such a cache can run besides (i).
A prefill over tens of thousands of tokens is HF's and is not what is measured: per shape (slots x rows) each decoder prefills a 128-token
prompt into a cache of that many slots, the slots behind it are filled with N(0, 1) keys and values, and the position counters are set to
slots - 2 * steps - 8, so the timed steps run near the end of the cache and stay inside it.  Everything runs with gradients off, as under
`GraphedDecoder.generate` (with gradients on every fused path declines to HF's modules); after the eager warm-up step the tool checks on the
host that the shared position counter moved by exactly one slot, and that (i) was served by the fused decode, before anything is captured.  One decode step (the decoder's own `_step` plus the counter
increments) is captured as a hipGraph after an eager warm-up; a figure is the time of `steps` replays over steps, by device events.  Three
alternated repeats per configuration, the median with (min - max).  Acceptance: every (i) repeat is faster than every (ii) repeat at every
shape; the tool says so per shape and exits with status 1 otherwise (the file is written either way).
Then the attention launches of (i) alone: HIP events over the layers' caches in turn (the K / V rows of all layers exceed the Infinity Cache
several times, so no call finds its cache there), with the bytes per second over the visible K / V rows.  For information only, the
one-workgroup entry and the key-split entry on the same 16384-slot caches at 1 and 16 rows."""
import os
import sys

os.environ.setdefault("LLAMOLE_TUNING", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llamole_amd import _lib, e2e  # noqa: E402
from llamole_amd.llm_accel import ATTN_MAXLEN, accelerate_llm  # noqa: E402
from llamole_amd.llm_decode import GraphedDecoder  # noqa: E402

argv = sys.argv[1:]
steps = int(argv[argv.index("--steps") + 1]) if "--steps" in argv else 16
out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join("profiles", "decode_longctx_time.txt")
shapes = tuple(tuple(int(v) for v in x.split("x")) for x in
               (argv[argv.index("--shapes") + 1] if "--shapes" in argv else "32768x1,32768x16,131072x1").split(","))
arch = argv[argv.index("--arch") + 1] if "--arch" in argv else "llama-3.1-8b"
over = {"num_hidden_layers": int(argv[argv.index("--layers") + 1])} if "--layers" in argv else {}
REPEATS = 3
torch.set_grad_enabled(False)       # as under GraphedDecoder.generate: with gradients on, every fused path declines to HF's modules
WINDOW_MS = 100.0       # timed window of the kernel-alone figures
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def flush():
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


class Stepper:
    """one decoder on a cache of `slots` slots x `rows` rows, its decode step captured, positioned 2 `steps` + 8 slots before the end"""

    def __init__(self, llm, fused_cache, slots, rows, want_served=False):
        self.dec = dec = GraphedDecoder(llm, use_graph=False, fused_cache=fused_cache)
        dec.len_bucket = slots
        prompt = torch.randint(5, min(30000, llm.config.vocab_size), (rows, 128), generator=torch.Generator().manual_seed(rows)).cuda()
        dec.generate(prompt, torch.ones_like(prompt), max_new_tokens=2, pad_token_id=0, eos_token_id=[], do_sample=False)
        assert dec.cache.layers[0].keys.shape[2] == slots
        for layer in dec.cache.layers:
            layer.keys[:, :, 128:].normal_()
            layer.values[:, :, 128:].normal_()
        self.start = slots - 2 * steps - 8
        self.base = getattr(llm, "model", llm)
        self.rewind()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self.body()
        torch.cuda.current_stream().wait_stream(s)
        # one step advances the shared position counter by exactly one slot (anything else would walk the timed steps off the cache)
        got = [int(layer.cumulative_length) for layer in dec.cache.layers[:2]]
        if got[0] != self.start + 1:
            raise RuntimeError(f"one decode step moved the cache position from {self.start} to {got}: not the decoder's own step")
        self.served = bool(self.base.__dict__.get("_ll_decode", {}).get("served"))
        if want_served and not self.served:
            raise RuntimeError("the fused decode did not serve the step of configuration (i)")
        self.rewind()
        self.graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                self.body()
        except Exception as e:      # noqa: BLE001 -- a step that does not capture is timed eagerly, and the output says so
            say(f"# capture failed ({type(e).__name__}: {(str(e).splitlines() or [''])[0]}): this configuration is timed eagerly")
            self.graph = None
            torch.cuda.synchronize()

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
            if self.graph is not None:
                self.graph.replay()
            else:
                self.body()
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


def attention_alone(llm, cache, slots, rows, pos, split=None):
    """the attention call of every fused layer on its own cache, one layer after the other; split: None = what the layer routes to, True = the
    key-split entry called directly (caches of <= 16384 slots, where the layer itself takes the one-workgroup entry)"""
    sts = [l._ll_fused for l in llm.model.layers]
    st0 = sts[0]
    dev = "cuda"
    nqkv = st0.nq + 2 * st0.nkv_dim
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(rows, nqkv, generator=g).to(torch.bfloat16).cuda()
    ang = torch.rand(1, 1, st0.D, generator=g) * 6.28
    pe = (ang.cos().to(torch.bfloat16).cuda(), ang.sin().to(torch.bfloat16).cuda())
    mask = torch.zeros(rows, 1, 1, slots, dtype=torch.bool, device=dev)
    mask[..., :pos + 1] = True
    for layer in cache.layers:
        layer.cumulative_length.fill_(pos)
    lib = _lib.load()

    def call(st):
        if not split:
            return st._attn(qkv, nqkv, mask, cache, pe, rows, dev)
        cl = cache.layers[st.layer_idx]
        att = torch.empty(rows, st.nq, dtype=torch.bfloat16, device=dev)
        _lib.check(lib.ll_decode_attn_rope_split_bf16(qkv.data_ptr(), nqkv, pe[0].data_ptr(), pe[1].data_ptr(), 0, cl.keys.data_ptr(),
                                                      cl.values.data_ptr(), cache.layers[0].cumulative_length.data_ptr(), mask.data_ptr(),
                                                      mask.stride(0), att.data_ptr(), rows, st.nh, st.nkv, slots, st.D, st.scaling,
                                                      *st._split_tail(rows, 1, slots, dev)), "ll_decode_attn_rope_split_bf16")
        return att

    def all_layers():
        for st in sts:
            call(st)
    med, lo, hi, calls = timed_us(all_layers, len(sts))
    nbytes = 2 * 2 * rows * st0.nkv * (pos + 1) * st0.D
    return med, lo, hi, calls, nbytes, len(sts)


def build():
    return e2e.build_llm(arch, "cuda", torch.bfloat16, rope_parameters=e2e.LLAMA31_ROPE, **over)


say(f"# decode token on long static caches at {arch} widths{' with ' + str(over['num_hidden_layers']) + ' decoder layers' if over else ''}, llama3 rope "
    f"{e2e.LLAMA31_ROPE}: (i) fused layers with the key-split attention against (ii) the same model with accelerate_llm(layers=False)")
say(f"# per figure {steps} replays of the captured decode step from slot slots - {2 * steps + 8} on, device events; {REPEATS} alternated repeats: median (min - max)")
CASES = (("(i) fused", {}), ("(ii) layers=False", dict(layers=False)))
llms, fused_cache = {}, {}
for name, accel_kw in CASES:
    llm = build()
    info = accelerate_llm(llm, **accel_kw)
    llms[name], fused_cache[name] = llm, bool(info.get("decode_attention"))
    say(f"# {name}: {type(llm).__name__}, {llm.config.num_hidden_layers} layers, decoder_layers_5_launches {info.get('decoder_layers_5_launches')}, "
        f"decode_prologue_1_launch {info.get('decode_prologue_1_launch')}, long_cache_attention_max_slots {info.get('long_cache_attention_max_slots')}, "
        f"declined {info.get('decoder_layers_declined')}")
ok = True
for slots, rows in shapes:
    tag = f"{arch} {slots} slots x {rows:2d} rows"
    steppers = {}
    for name, _ in CASES:
        st = steppers[name] = Stepper(llms[name], fused_cache[name], slots, rows, want_served=name.startswith("(i)"))
        say(f"# {tag} {name}: decode step captured = {st.graph is not None}, served by the fused prologue = {st.served}")
        st.token_ms()                            # warm-up of the replay
    res = {name: [] for name, _ in CASES}
    for _ in range(REPEATS):
        for name, _ in CASES:
            res[name].append(steppers[name].token_ms())
    med = {}
    for name, _ in CASES:
        v = res[name]
        med[name] = sorted(v)[len(v) // 2]
        say(f"{tag} {name}: decode token median {med[name]:.4f} ms (runs {', '.join(f'{x:.4f}' for x in v)}; min {min(v):.4f} - max {max(v):.4f})")
    f, u = (res[name] for name, _ in CASES)
    faster = max(f) < min(u)
    ok = ok and faster
    say(f"{tag}: (ii) / (i) = {med['(ii) layers=False'] / med['(i) fused']:.2f} x by the medians; every (i) repeat "
        f"{'IS FASTER than' if faster else 'is NOT faster than'} every (ii) repeat ([{min(f):.4f}, {max(f):.4f}] against [{min(u):.4f}, {max(u):.4f}])")
    # the attention launches of (i) alone, on this shape's caches
    pos = slots - 9
    a_med, a_lo, a_hi, calls, nbytes, nl = attention_alone(llms["(i) fused"], steppers["(i) fused"].dec.cache, slots, rows, pos)
    say(f"{tag}: ll_decode_attn_rope_split_bf16 alone (two launches), *pos = {pos}: median {a_med:.1f} us (min {a_lo:.1f} - max {a_hi:.1f}) per call over "
        f"{nl} layers' caches in turn, {calls} calls per window; {nbytes / 1e6:.1f} MB of visible K / V rows = {nbytes / a_med / 1e6:.2f} TB/s; "
        f"x {nl} layers = {a_med * nl / 1000:.3f} ms of the {med['(i) fused']:.4f} ms token")
    flush()
    del steppers, st
    torch.cuda.empty_cache()
# for information: both entries on the same 16384-slot caches (the layer itself routes such a cache to the one-workgroup entry)
for rows in (1, 16):
    st = Stepper(llms["(i) fused"], True, ATTN_MAXLEN, rows)
    pos = ATTN_MAXLEN - 9
    for label, split in (("one-workgroup entry (ll_decode_attn_rope_bf16)", False), ("key-split entry (ll_decode_attn_rope_split_bf16)", True)):
        a_med, a_lo, a_hi, calls, nbytes, nl = attention_alone(llms["(i) fused"], st.dec.cache, ATTN_MAXLEN, rows, pos, split)
        say(f"for information, {ATTN_MAXLEN} slots x {rows:2d} rows, *pos = {pos}, {label}: median {a_med:.1f} us (min {a_lo:.1f} - max {a_hi:.1f}) per "
            f"call over {nl} layers' caches in turn; {nbytes / 1e6:.1f} MB of visible K / V rows = {nbytes / a_med / 1e6:.2f} TB/s")
    flush()
    del st
    torch.cuda.empty_cache()
flush()
sys.exit(0 if ok else 1)
