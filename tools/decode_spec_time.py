"""One prompt-lookup speculative step (GraphedDecoder.generate(prompt_lookup_num_tokens=k): the model on k + 1 rows of one sequence,
ll_spec_verify_bf16 and the next draft, one captured graph) against the plain batch-1 decode token (forward on one row + the fused sampler,
one captured graph), at Qwen2-7B and Llama-3.1-8B widths (random bf16 weights), all decoders in one process:
python tools/decode_spec_time.py [--out profiles/decode_spec_time.txt] [--steps N] [--archs qwen2-7b,llama-3.1-8b] [--ks 3,5,7,15] [--layers L]
(--archs: entries of e2e.LLM_CONFIGS, e.g. tiny-llama for a dry run; --layers: fewer decoder layers, stated in the output).
Per arch every decoder runs one generate of 8 tokens on a 16-token prompt in a cache of 1024 slots, which captures its step graph -- the
decoder's own, nothing is rebuilt here.  A figure is the time of `steps` replays of that graph over steps, by device events, after the
loop state is put back to the first step (counters, stop flag, history length; max_new_tokens out of reach, so every replay is a full
step whatever it accepts).  Three alternated repeats over all decoders: the median with (min - max).  NO time is a pass condition.
Reported: (a) the step at each k against the plain token of the same run, (b) the break-even c(k) - 1 = the accepted drafts per step at
which a speculative decode emits tokens at the plain decode's rate, (c) the plain token of this commit against the parent commit's:
`--plain-only` runs this tool for the plain decoder alone (it then works from a tree without the option as well), and
`--parent-plain a,b,c --own-plain d,e,f` quotes the figures such runs wrote, one process each, alternated, (d) tokens per forward of the
flagship workload's decode -- bench.py's synthetic checkpoint, prompt and sampling options -- which is RANDOM-WEIGHT text, not Llamole
text: the acceptance rate on real checkpoints is unmeasured."""
import gc
import os
import re
import sys

os.environ.setdefault("LLAMOLE_TUNING", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llamole_amd import e2e  # noqa: E402
from llamole_amd.llm_accel import accelerate_llm  # noqa: E402
from llamole_amd.llm_decode import GraphedDecoder  # noqa: E402

argv = sys.argv[1:]


def opt(name, default):
    return argv[argv.index(name) + 1] if name in argv else default


steps = int(opt("--steps", 32))
out_path = opt("--out", os.path.join("profiles", "decode_spec_time.txt"))
archs = opt("--archs", "qwen2-7b,llama-3.1-8b").split(",")
ks = [] if "--plain-only" in argv else [int(k) for k in opt("--ks", "3,5,7,15").split(",")]
parent_files = [p for p in opt("--parent-plain", "").split(",") if p]
own_files = [p for p in opt("--own-plain", "").split(",") if p]
over = {"num_hidden_layers": int(opt("--layers", 0))} if "--layers" in argv else {}
REPEATS, PROMPT, SLOTS = 3, 16, 1024
assert PROMPT + 16 * (steps + 1) + 16 <= SLOTS, "the replays of a window must stay inside the cache"
torch.set_grad_enabled(False)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def flush():
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


class Stepper:
    """one decoder whose own captured step (plain: k None) is replayed from the first step of its call"""

    def __init__(self, llm, k):
        self.k = k
        self.dec = dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
        dec.len_bucket = SLOTS
        prompt = torch.randint(5, min(30000, llm.config.vocab_size), (1, PROMPT), generator=torch.Generator().manual_seed(1)).cuda()
        dec.generate(prompt, torch.ones_like(prompt), max_new_tokens=8, pad_token_id=0, eos_token_id=[], do_sample=False,
                     prompt_lookup_num_tokens=k)
        self.graph = dec._spec_graph if k else dec._graph
        if self.graph is None or not getattr(llm, "model", llm).__dict__.get("_ll_decode", {}).get("served"):
            raise RuntimeError(f"k = {k}: the step was not captured on the fused forward")
        assert dec.cache.layers[0].keys.shape[2] == SLOTS

    def rewind(self):
        dec = self.dec
        dec.done.zero_()
        dec.stepc.fill_(1)
        dec.pos.fill_(PROMPT)
        dec.posid.fill_(PROMPT)
        dec.cache.layers[0].cumulative_length.fill_(PROMPT)
        if self.k:
            dec._spec_bufs["max_new"].fill_(SLOTS)
            dec._spec_bufs["hist_len"].fill_(PROMPT + 1)
            dec._spec_bufs["stats"].zero_()

    def step_ms(self):
        self.rewind()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            self.graph.replay()
        e1.record()
        torch.cuda.synchronize()
        if self.k:
            f, a = self.dec._spec_bufs["stats"].tolist()
            assert f == steps, (f, steps)              # every replay was a full step
        return e0.elapsed_time(e1) / steps


def plain_of(paths, arch):
    """the plain-token medians that earlier runs of this tool wrote to ``paths``, one per file"""
    out = []
    for path in paths:
        m = re.search(rf"^{re.escape(arch)} plain: decode token median ([0-9.]+) ms", open(path).read(), flags=re.M)
        if m:
            out.append(float(m.group(1)))
    return out


say("# prompt-lookup speculative decoding: one step on k + 1 rows of ONE sequence against the plain batch-1 decode token, random bf16 weights")
say(f"# per figure {steps} replays of the decoder's own captured step, device events; {REPEATS} alternated repeats: median (min - max).  "
    "No time is a pass condition.")
for arch in archs:
    llm = e2e.build_llm(arch, "cuda", torch.bfloat16, **over)
    info = accelerate_llm(llm)
    say(f"# {arch}{' with ' + str(over['num_hidden_layers']) + ' decoder layers' if over else ''}: {type(llm).__name__}, "
        f"{llm.config.num_hidden_layers} layers, vocabulary {llm.config.vocab_size}, decoder_layers_5_launches "
        f"{info.get('decoder_layers_5_launches')}, decode_prologue_1_launch {info.get('decode_prologue_1_launch')}")
    steppers = {k: Stepper(llm, k) for k in [None] + ks}
    for st in steppers.values():
        st.step_ms()                                 # warm-up of the replay
    res = {k: [] for k in steppers}
    for _ in range(REPEATS):
        for k, st in steppers.items():
            res[k].append(st.step_ms())
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    v = res[None]
    say(f"{arch} plain: decode token median {med[None]:.4f} ms (runs {', '.join(f'{x:.4f}' for x in v)}; min {min(v):.4f} - max {max(v):.4f})")
    for k in ks:
        v = res[k]
        c = med[k] / med[None]
        say(f"{arch} k = {k:2d} ({k + 1:2d} rows): speculative step median {med[k]:.4f} ms (runs {', '.join(f'{x:.4f}' for x in v)}; min {min(v):.4f} - "
            f"max {max(v):.4f}) = c(k) {c:.3f} x the plain token; break-even {c - 1:.3f} accepted drafts per step "
            f"({(c - 1) / k:.3f} of the {k} drafted)")
    par, own = plain_of(parent_files, arch), plain_of(own_files, arch)
    if par and own:
        mp, mo = sorted(par)[len(par) // 2], sorted(own)[len(own) // 2]
        say(f"{arch} plain token, one process per figure, parent commit and this commit alternated (--plain-only runs of this tool from either "
            f"tree): parent {', '.join(f'{x:.4f}' for x in par)} ms (median {mp:.4f}, min {min(par):.4f} - max {max(par):.4f}); this commit "
            f"{', '.join(f'{x:.4f}' for x in own)} ms (median {mo:.4f}) = {mo / mp:.4f} x; this commit's median lies "
            f"{'inside' if min(par) <= mo <= max(par) else 'OUTSIDE'} the parent's range")
    flush()
    del steppers, st
    gc.collect()
    torch.cuda.empty_cache()
    if arch == archs[0] and ks:
        # (d) the flagship workload's decode (bench.py: this checkpoint, a 128-token prompt of random ids, 128 new tokens sampled at
        # temperature 0.6 / top_p 0.9 / top_k 50), one sequence
        tok = e2e.SyntheticTokenizer(llm.config.vocab_size)
        kw = e2e.gen_kwargs(tok, 128)
        prompt = torch.randint(5, 1000, (1, 128), generator=torch.Generator().manual_seed(100)).cuda()
        say(f"# {arch}: tokens per forward on the flagship workload's decode -- RANDOM-WEIGHT text (synthetic checkpoint, random prompt), "
            "NOT Llamole text; the acceptance rate on real checkpoints is unmeasured")
        for greedy in (False, True):
            for k in ks:
                dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
                out = dec.generate(prompt, torch.ones_like(prompt), generator=torch.Generator(device="cuda").manual_seed(1000),
                                   prompt_lookup_num_tokens=k, **dict(kw, do_sample=not greedy))
                s = dec.spec_stats
                say(f"{arch} workload decode, {'greedy' if greedy else 'sampled (0.6 / 0.9 / 50)'}, k = {k:2d}: {s['tokens']} tokens in "
                    f"{s['forwards']} speculative forwards + the prefill, {s['accepted']} drafts accepted = "
                    f"{s['accepted'] / max(1, s['forwards']):.3f} per step, {(s['tokens'] - 1) / max(1, s['forwards']):.3f} tokens per forward"
                    f" ({out.shape[1] - 128} new tokens returned)")
                del dec
        flush()
    del llm
    gc.collect()
    torch.cuda.empty_cache()
flush()
