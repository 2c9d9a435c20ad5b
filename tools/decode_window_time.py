"""Decode token of a sliding-window model at Mistral-7B-v0.1 widths (e2e "mistral-7b-v0.1": window 4096 on every layer; random bf16 weights):
python tools/decode_window_time.py [--out profiles/decode_window_time.txt] [--steps N] [--shapes 32768x1,32768x16,131072x1]
                                   [--arch mistral-7b-v0.1] [--layers L] [--window W] [--parent TREE] [--unchanged llama-3.1-8b,qwen2-7b]
(--arch: any sliding-window entry of e2e.LLM_CONFIGS, e.g. tiny-mistral-sw --window 256 for a dry run; --layers: fewer decoder layers, stated in
the output; --window: another window than the entry's, at least 192 so that the 128-token prompt fits the cache of the last part).
Three models with the same weights live in one process:
  (i)   the fused stack: five-launch layers whose attention is the windowed key-split pair of launches (ll_decode_attn_rope_win_bf16);
  (ii)  accelerate_llm(layers=False): HF's layer code per token with HF's sliding mask -- what such a model ran before;
  (iii) the same widths with sliding_window = None: the fused stack with full attention on the key-split entries (ll_decode_attn_rope_split_bf16).
As in tools/decode_longctx_time.py a prefill over tens of thousands of tokens is not what is measured: per shape (slots x rows) each decoder
prefills a 128-token prompt into a cache of that many slots, the slots behind it are filled with N(0, 1) keys and values, and the position
counters are set to slots - 2 * steps - 8, so the timed steps run near the end of the cache.  One decode step is captured as a hipGraph after an
eager warm-up; a figure is the time of `steps` replays over steps, by device events; three alternated repeats per pair, the median with
(min - max).  (i) is timed against (ii), then -- (ii)'s cache freed -- against (iii).  Acceptance, said per shape, exit status 1 otherwise:
every (i) repeat below every (ii) repeat; the windowed attention call alone below the full one beyond the spread of the repeats
(max windowed < min full).  The attention calls alone run over the layers' caches in turn (the K / V rows of all layers exceed the Infinity
Cache), with the K / V bytes each reads and its share of the token.
Then the case where the window cannot bind: a 4096-slot cache, (i) against (ii); the fused layers take the one-workgroup entries there, as a
Llama of these widths does (reported, not a pass condition).
--parent TREE (runs first): the decode tokens of models whose launches this change leaves alone (--unchanged) at 1 / 16 / 64 rows, this tree against a built
checkout of the parent commit in TREE, in alternated child processes (three per tree): every median of this tree must lie within
[min, max] of the parent's repeats, widened by nothing."""
import gc
import json
import os
import subprocess
import sys

os.environ.setdefault("LLAMOLE_TUNING", "1")
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]
TREE = argv[argv.index("--tree") + 1] if "--tree" in argv else HERE          # child mode: the package is imported from this tree
sys.path.insert(0, TREE)
import torch  # noqa: E402

from llamole_amd import e2e  # noqa: E402
from llamole_amd.llm_accel import accelerate_llm  # noqa: E402
from llamole_amd.llm_decode import GraphedDecoder  # noqa: E402

steps = int(argv[argv.index("--steps") + 1]) if "--steps" in argv else 16
out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join("profiles", "decode_window_time.txt")
shapes = tuple(tuple(int(v) for v in x.split("x")) for x in
               (argv[argv.index("--shapes") + 1] if "--shapes" in argv else "32768x1,32768x16,131072x1").split(","))
arch = argv[argv.index("--arch") + 1] if "--arch" in argv else "mistral-7b-v0.1"
over = {"num_hidden_layers": int(argv[argv.index("--layers") + 1])} if "--layers" in argv else {}
win_over = {"sliding_window": int(argv[argv.index("--window") + 1])} if "--window" in argv else {}       # another window than the entry's (dry runs)
parent = argv[argv.index("--parent") + 1] if "--parent" in argv else None
unchanged = (argv[argv.index("--unchanged") + 1] if "--unchanged" in argv else "llama-3.1-8b,qwen2-7b").split(",")
REPEATS = 3
ROWS = (1, 16, 64)
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
            raise RuntimeError("the fused decode did not serve the step of a fused configuration")
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


def release():
    """hand the device memory of dropped decoders back: they sit in reference cycles, which only a collection frees"""
    gc.collect()
    torch.cuda.empty_cache()


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
    """the attention call every fused layer routes to, on its own cache, one layer after the other; the K / V bytes a call reads: the rows the
    window shows (all rows up to *pos without a window)"""
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

    def all_layers():
        for st in sts:
            st._attn(qkv, nqkv, mask, cache, pe, rows, dev)
    med, lo, hi, calls = timed_us(all_layers, len(sts))
    seen = min(pos + 1, st0.window) if st0._windowed(slots) else pos + 1
    nbytes = 2 * 2 * rows * st0.nkv * seen * st0.D
    return med, lo, hi, calls, nbytes, len(sts)


def pair(tag, a, b, steppers):
    """three alternated repeats of two captured steps; returns {name: [ms]}"""
    for n in (a, b):
        steppers[n].token_ms()                   # warm-up of the replay
    res = {a: [], b: []}
    for _ in range(REPEATS):
        for n in (a, b):
            res[n].append(steppers[n].token_ms())
    for n in (a, b):
        v = res[n]
        say(f"{tag} {n}: decode token median {sorted(v)[1]:.4f} ms (runs {', '.join(f'{x:.4f}' for x in v)}; min {min(v):.4f} - max {max(v):.4f})")
    return res


def child():
    """--child ARCH: the decode token of one unchanged model at 1 / 16 / 64 rows on a 512-slot cache, one JSON line"""
    name = argv[argv.index("--child") + 1]
    llm = e2e.build_llm(name, "cuda", torch.bfloat16, **over)
    accelerate_llm(llm)
    out = {}
    for rows in ROWS:
        st = Stepper(llm, True, 512, rows, want_served=True)
        st.token_ms()
        out[str(rows)] = sorted(st.token_ms() for _ in range(REPEATS))[1]
        del st
        torch.cuda.empty_cache()
    print("CHILD " + json.dumps(out), flush=True)


def against_parent():
    ok = True
    trees = (("this commit", HERE), ("parent commit", parent))
    for name in unchanged:
        res = {label: {str(r): [] for r in ROWS} for label, _ in trees}
        for _ in range(REPEATS):
            for label, tree in trees:
                cmd = [sys.executable, os.path.abspath(__file__), "--tree", tree, "--child", name, "--steps", str(steps)]
                if over:
                    cmd += ["--layers", str(over["num_hidden_layers"])]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                got = [l for l in p.stdout.splitlines() if l.startswith("CHILD ")]
                if p.returncode != 0 or not got:
                    raise RuntimeError(f"child process for {name} in {tree} failed ({p.returncode}): {p.stderr[-2000:]}")
                for r, v in json.loads(got[-1][6:]).items():
                    res[label][r].append(v)
        for r in ROWS:
            a, b = res["this commit"][str(r)], res["parent commit"][str(r)]
            med = sorted(a)[1]
            inside = min(b) <= med <= max(b)
            ok = ok and (inside or med < min(b))
            say(f"{name} {r:2d} rows, 512 slots: this commit median {med:.4f} ms (min {min(a):.4f} - max {max(a):.4f}); parent commit median "
                f"{sorted(b)[1]:.4f} ms (min {min(b):.4f} - max {max(b):.4f}): this commit's median "
                f"{'lies within' if inside else 'is below' if med < min(b) else 'is ABOVE'} the parent's spread")
        flush()
    return ok


if "--child" in argv:
    child()
    sys.exit(0)

ok = True
if parent:
    # first, while this process holds no device memory: every child builds a model of its own
    say(f"# models whose launches are unchanged, decode token on a 512-slot cache at {ROWS} rows: {REPEATS} alternated child processes per tree, each "
        f"the median of {REPEATS} figures of {steps} replays")
    ok = against_parent()
say(f"# decode token of a sliding-window model at {arch} widths{' with ' + str(over['num_hidden_layers']) + ' decoder layers' if over else ''}: (i) fused "
    "layers with the windowed key-split attention, (ii) the same model with accelerate_llm(layers=False), (iii) the same widths with "
    "sliding_window = None on the fused layers (full key-split attention)")
say(f"# per figure {steps} replays of the captured decode step from slot slots - {2 * steps + 8} on, device events; {REPEATS} alternated repeats: median (min - max)")
I, II, III = "(i) fused, windowed", "(ii) layers=False", "(iii) fused, no window"
CASES = ((I, {}, win_over), (II, dict(layers=False), win_over), (III, {}, dict(sliding_window=None)))
llms, fused_cache = {}, {}
for name, accel_kw, build_kw in CASES:
    llm = e2e.build_llm(arch, "cuda", torch.bfloat16, **over, **build_kw)
    info = accelerate_llm(llm, **accel_kw)
    llms[name], fused_cache[name] = llm, bool(info.get("decode_attention"))
    say(f"# {name}: {type(llm).__name__}, {llm.config.num_hidden_layers} layers, sliding_window {llm.config.sliding_window}, decoder_layers_5_launches "
        f"{info.get('decoder_layers_5_launches')}, decode_prologue_1_launch {info.get('decode_prologue_1_launch')}, declined "
        f"{info.get('decoder_layers_declined')} / {info.get('decode_prologue_declined')}")
for slots, rows in shapes:
    tag = f"{arch} {slots} slots x {rows:2d} rows"
    steppers = {}
    for name in (I, II):
        st = steppers[name] = Stepper(llms[name], fused_cache[name], slots, rows, want_served=name != II)
        say(f"# {tag} {name}: decode step captured = {st.graph is not None}, served by the fused prologue = {st.served}, cache "
            f"{type(st.dec.cache).__name__}")
    res = pair(tag, I, II, steppers)
    f, u = res[I], res[II]
    faster = max(f) < min(u)
    ok = ok and faster
    say(f"{tag}: (ii) / (i) = {sorted(u)[1] / sorted(f)[1]:.2f} x by the medians; every (i) repeat {'IS FASTER than' if faster else 'is NOT faster than'} "
        f"every (ii) repeat ([{min(f):.4f}, {max(f):.4f}] against [{min(u):.4f}, {max(u):.4f}])")
    del steppers[II], st
    release()
    steppers[III] = Stepper(llms[III], True, slots, rows, want_served=True)
    res = pair(tag, I, III, steppers)
    tok = {n: sorted(res[n])[1] for n in (I, III)}
    say(f"{tag}: (iii) / (i) = {tok[III] / tok[I]:.2f} x by the medians ([{min(res[I]):.4f}, {max(res[I]):.4f}] against [{min(res[III]):.4f}, {max(res[III]):.4f}])")
    pos = slots - 9
    alone = {}
    for n, entry in ((I, "ll_decode_attn_rope_win_bf16"), (III, "ll_decode_attn_rope_split_bf16")):
        a_med, a_lo, a_hi, calls, nbytes, nl = alone[n] = attention_alone(llms[n], steppers[n].dec.cache, slots, rows, pos)
        say(f"{tag} {n}: {entry} alone (two launches), *pos = {pos}: median {a_med:.1f} us (min {a_lo:.1f} - max {a_hi:.1f}) per call over {nl} layers' "
            f"caches in turn, {calls} calls per window; {nbytes / 1e6:.1f} MB of K / V rows read = {nbytes / a_med / 1e6:.2f} TB/s; x {nl} layers = "
            f"{a_med * nl / 1000:.3f} ms = {100 * a_med * nl / 1000 / tok[n]:.1f} % of the {tok[n]:.4f} ms token")
    less = alone[I][2] < alone[III][1]
    ok = ok and less
    say(f"{tag}: the windowed attention call {'TAKES LESS than' if less else 'does NOT take less than'} the full one beyond the spread of the repeats "
        f"(max {alone[I][2]:.1f} us against min {alone[III][1]:.1f} us): {alone[III][0] / alone[I][0]:.2f} x by the medians")
    flush()
    del steppers
    release()
# the window cannot bind: a cache of exactly `window` slots, where the fused layers take a full-attention layer's launches (the one-workgroup
# attention entries: the figures are those of a Llama of these widths on such a cache).  Reported, not a pass condition.
slots = llms[I].config.sliding_window
for rows in (1, 16):
    tag = f"{arch} {slots} slots x {rows:2d} rows (the window cannot bind)"
    steppers = {name: Stepper(llms[name], fused_cache[name], slots, rows, want_served=name != II) for name in (I, II)}
    res = pair(tag, I, II, steppers)
    f, u = res[I], res[II]
    faster = max(f) < min(u)
    say(f"{tag}: (ii) / (i) = {sorted(u)[1] / sorted(f)[1]:.2f} x by the medians; every (i) repeat {'IS FASTER than' if faster else 'is NOT faster than'} "
        f"every (ii) repeat ([{min(f):.4f}, {max(f):.4f}] against [{min(u):.4f}, {max(u):.4f}])")
    flush()
    del steppers
    release()
flush()
sys.exit(0 if ok else 1)
