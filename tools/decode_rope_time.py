"""Decode token of the graphed decoder at Llama-3.1-8B widths with default rope and with the published llama3 rope scaling
(e2e.LLAMA31_ROPE; random bf16 weights):
python tools/decode_rope_time.py [--out profiles/decode_rope_time.txt] [--new N] [--rows 1,16,64] [--arch llama-3.1-8b]  (--arch: any
e2e.LLM_CONFIGS entry, e.g. tiny-llama for a dry run).
Three models live in one process: default rope (what README / DESIGN quote for "Llama-3.1-8B"), the scaled model on the fused decode, and
the scaled model with the one-launch prologue declined (accelerate_llm(model_decode=False): the installed state such a model had before the
scaled types were accepted -- the per-layer patch still runs the five-launch layers and, beyond 16 rows, the seven-launch ones; HF's rotary
module and mask construction run per token, and no layer hands its closing pre-norm to the next).  Per row count every case sees the same prompts; the
token time is (generate(1 + n) - generate(1)) / n, median of 3, greedy, after a 128-token prompt, and the cases are taken alternately over
three repeats after a warm-up of every case.  The scaled model issues the same launches as the default one with other constants, so its
token (the median of its repeats) has to lie within the spread [min, max] of the default-rope repeats at every row count: the tool says so
per row count and exits with status 1 when it does not (the file is written either way).  That rule is the stated one taken literally,
and with three repeats a side it has false alarms: for two identical distributions the median of three falls below (or above) all three
of the others once in five runs per side.  Read an exit 1 against the printed runs and the percentage next to the verdict -- a token a
fraction of a percent outside a spread of the same size is noise, not a regression.  The ratio declined / fused is what accepting the
scaled types gains."""
import os
import sys

os.environ.setdefault("LLAMOLE_TUNING", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llamole_amd import e2e  # noqa: E402
from llamole_amd.llm_accel import accelerate_llm  # noqa: E402
from llamole_amd.llm_decode import GraphedDecoder  # noqa: E402

argv = sys.argv[1:]
n = int(argv[argv.index("--new") + 1]) if "--new" in argv else 128
out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join("profiles", "decode_rope_time.txt")
rows = tuple(int(x) for x in argv[argv.index("--rows") + 1].split(",")) if "--rows" in argv else (1, 16, 64)
arch = argv[argv.index("--arch") + 1] if "--arch" in argv else "llama-3.1-8b"
REPEATS = 3
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


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


CASES = (("default rope", {}, {}), ("llama3 rope, fused", dict(rope_parameters=e2e.LLAMA31_ROPE), {}),
         ("llama3 rope, prologue declined", dict(rope_parameters=e2e.LLAMA31_ROPE), dict(model_decode=False)))
say(f"# decode token at {arch} widths, default rope / llama3 rope {e2e.LLAMA31_ROPE}")
say(f"# n = {n} tokens after a 128-token prompt, greedy, median of 3 per figure, {REPEATS} alternated repeats")
say("# 'prologue declined' = accelerate_llm(model_decode=False) on this tree: a stand-in for the commit before the scaled types were accepted, where "
    "fuse_model_decode declined rope_type llama3 and left the model in the same installed state")
models = {}
outside = 0
for name, build_kw, accel_kw in CASES:
    llm = e2e.build_llm(arch, "cuda", torch.bfloat16, **build_kw)
    info = accelerate_llm(llm, **accel_kw)
    models[name] = GraphedDecoder(llm, use_graph=True, fused_cache=bool(info.get("decode_attention")))
    say(f"# {name}: rope_type {llm.model.rotary_emb.rope_type}, decoder_layers_5_launches {info.get('decoder_layers_5_launches')}, "
        f"decode_prologue_1_launch {info.get('decode_prologue_1_launch')}")
for B in rows:
    prompt = torch.randint(5, 30000, (B, 128), generator=torch.Generator().manual_seed(B)).cuda()
    for name, _, _ in CASES:                        # warm-up of every case: capture both lengths
        for new in (1 + n, 1):
            models[name].generate(prompt, torch.ones_like(prompt), max_new_tokens=new, pad_token_id=0, eos_token_id=[], do_sample=False)
    res = {name: [] for name, _, _ in CASES}
    for _ in range(REPEATS):
        for name, _, _ in CASES:
            res[name].append((gen_ms(models[name], prompt, 1 + n) - gen_ms(models[name], prompt, 1)) / n)
    for name, _, _ in CASES:
        v = res[name]
        say(f"{arch} rows {B:2d} {name}: decode token {min(v):.4f} ms (runs {', '.join(f'{x:.4f}' for x in v)}; spread {max(v) - min(v):.4f})")
    d, sc, p = (res[name] for name, _, _ in CASES)
    token = sorted(sc)[len(sc) // 2]
    inside = min(d) <= token <= max(d)
    outside += 0 if inside else 1
    say(f"{arch} rows {B:2d}: fused llama3 token (median of its repeats) {token:.4f} ms {'lies WITHIN' if inside else 'lies OUTSIDE'} the default-rope "
        f"spread [{min(d):.4f}, {max(d):.4f}] ({100 * (token / sorted(d)[len(d) // 2] - 1):+.2f} % against the default-rope median); "
        f"prologue declined / fused = {min(p) / min(sc):.3f} x")
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
if outside:
    sys.exit(1)
