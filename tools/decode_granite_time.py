"""Decode token of the graphed decoder on a Granite-layout model (residual_multiplier in both residual adds, embedding_multiplier on the
embedding rows) at the widths of e2e.LLM_CONFIGS["granite-3.3-8b"] (random bf16 weights; the widths and multipliers there are written from
memory of the published config, see e2e.py, and are printed at the top of the output):
python tools/decode_granite_time.py [--out profiles/decode_granite_time.txt] [--new N] [--rows 1,16,64] [--arch granite-3.3-8b]
                                    [--parent-tree DIR]
(--arch: any Granite entry of e2e.LLM_CONFIGS, e.g. tiny-granite for a dry run).
Three models live in one process:
  (i)   the fused stack (five- / seven-launch layers on the scaled residual entries, ll_embed_rows_bf16, one-launch prologue);
  (ii)  the same model with accelerate_llm(layers=False): HF's layer code (which applies the multipliers itself) over the fused Linears,
        RMSNorm, rotary and attention kernels, HF's rotary module and mask construction per token;
  (iii) a Llama-layout model of the same widths without the multipliers: the same launches as (i) on the unscaled entries, i.e. what the
        scaled epilogue and the embedding launch cost.
The vocabulary of (i)-(iii) is the published one rounded UP to a multiple of 8 (49160): the published 49159 is not a multiple of 8, which the
HIP sampler and the lm_head GEMV need, so a checkpoint with that vocabulary samples and projects through torch -- not what is timed here.
Per row count every case sees the same prompts; the token time is (generate(1 + n) - generate(1)) / n, median of 3, greedy, after a 128-token
prompt, and the cases are taken alternately over three repeats after a warm-up of every case; median (min - max) of the repeats is reported.
--parent-tree DIR: also time llama-3.1-8b (no multipliers: existing kernels only) on this tree and on the built checkout of the parent
commit at DIR, in child processes taken alternately, three repeats each -- the existing kernels must not have moved.  The comparison ends at
the first child that fails (nothing more is started on the device), reports its figures as not measured, and the tool exits 1.
The file starts with the error of one fused decode step of tiny-granite against HF in f32, next to HF's own bf16 (the figures
tests/test_granite_decode_gpu.py asserts on)."""
import copy
import json
import os
import subprocess
import sys

os.environ.setdefault("LLAMOLE_TUNING", "1")
argv = sys.argv[1:]
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = argv[argv.index("--tree") + 1] if "--tree" in argv else HERE          # --tree: the checkout llamole_amd is imported from (children)
sys.path.insert(0, TREE)
import torch  # noqa: E402

from llamole_amd import e2e  # noqa: E402
from llamole_amd.llm_accel import (accelerate_llm, restore_decoder_layers, restore_elementwise, restore_linears,  # noqa: E402
                                   restore_model_decode)
from llamole_amd.llm_decode import GraphedDecoder  # noqa: E402

n = int(argv[argv.index("--new") + 1]) if "--new" in argv else 128
out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join("profiles", "decode_granite_time.txt")
rows = tuple(int(x) for x in argv[argv.index("--rows") + 1].split(",")) if "--rows" in argv else (1, 16, 64)
arch = argv[argv.index("--arch") + 1] if "--arch" in argv else "granite-3.3-8b"
parent_tree = argv[argv.index("--parent-tree") + 1] if "--parent-tree" in argv else None
failed = None
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


def token_ms(dec, prompt):
    return (gen_ms(dec, prompt, 1 + n) - gen_ms(dec, prompt, 1)) / n


def fmt(v):
    return f"{sorted(v)[len(v) // 2]:.4f} ms ({min(v):.4f} - {max(v):.4f})"


def llama_child():
    """--llama-child: one repeat of llama-3.1-8b at every row count on the tree of --tree; one JSON line {rows: token ms}"""
    llm = e2e.build_llm("llama-3.1-8b", "cuda", torch.bfloat16)
    info = accelerate_llm(llm)
    dec = GraphedDecoder(llm, use_graph=True, fused_cache=bool(info.get("decode_attention")))
    res = {}
    for B in rows:
        prompt = torch.randint(5, 30000, (B, 128), generator=torch.Generator().manual_seed(B)).cuda()
        for new in (1 + n, 1):
            dec.generate(prompt, torch.ones_like(prompt), max_new_tokens=new, pad_token_id=0, eos_token_id=[], do_sample=False)
        res[str(B)] = token_ms(dec, prompt)
    print("LLAMA_CHILD " + json.dumps(res), flush=True)


if "--llama-child" in argv:
    llama_child()
    sys.exit(0)


def step_error():
    """one fused decode step of tiny-granite (1 row of 13 tokens) against the untouched HF model in f32; HF's bf16 next to it; and the same
    step with the multipliers dropped from the fused path, which is what these layers computed before the layout was served"""
    llm = e2e.build_llm("tiny-granite", "cuda", torch.bfloat16)
    hf16, hf32 = copy.deepcopy(llm), copy.deepcopy(llm).float()
    prompt = torch.randint(5, 2000, (1, 13), generator=torch.Generator().manual_seed(13)).cuda()
    accelerate_llm(llm)

    def step():
        dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
        toks = dec.generate(prompt, torch.ones_like(prompt), max_new_tokens=2, do_sample=False, pad_token_id=0, eos_token_id=[])
        return toks, dec.last_logits.float().clone()
    try:
        toks, fused = step()
        for layer in llm.model.layers:
            layer._ll_fused.rscale = None
        del llm.model._ll_decode["embed_scale"]
        _, dropped = step()
    finally:
        restore_model_decode(llm), restore_decoder_layers(llm), restore_elementwise(llm), restore_linears(llm)
    with torch.no_grad():
        ref, b16 = (m(input_ids=toks[:, :14], use_cache=False).logits[:, -1, :].float() for m in (hf32, hf16))
    E, Y, E0 = float((fused - ref).abs().max()), float((b16 - ref).abs().max()), float((dropped - ref).abs().max())
    say(f"tiny-granite, one fused decode step against HF f32 (max |logit error|): fused E = {E:.5f}, HF bf16 Y = {Y:.5f}, E / Y = {E / Y:.3f}; "
        f"with the multipliers dropped from the fused step E = {E0:.5f} = {E0 / Y:.1f} Y")


spec = e2e.LLM_CONFIGS[arch]
vocab = (spec["vocab_size"] + 7) // 8 * 8
llama_twin = {k: v for k, v in spec.items() if k not in ("embedding_multiplier", "attention_multiplier", "residual_multiplier", "logits_scaling")}
llama_twin.update(cls="Llama", attention_bias=False, vocab_size=vocab)
CASES = (("(i) fused", lambda: e2e.build_llm(arch, "cuda", torch.bfloat16, vocab_size=vocab), {}),
         ("(ii) layers=False", lambda: e2e.build_llm(arch, "cuda", torch.bfloat16, vocab_size=vocab), dict(layers=False)),
         ("(iii) Llama layout, no multipliers", lambda: e2e.build_llm("tiny-llama", "cuda", torch.bfloat16, **llama_twin), {}))
say(f"# decode token at {arch} widths (from memory of the published config): hidden {spec['hidden_size']}, {spec['num_hidden_layers']} layers, "
    f"{spec['num_attention_heads']} / {spec['num_key_value_heads']} heads, intermediate {spec['intermediate_size']}, multipliers embedding "
    f"{spec['embedding_multiplier']}, attention {spec['attention_multiplier']}, residual {spec['residual_multiplier']}, logits {spec['logits_scaling']}")
say(f"# vocabulary {vocab} (published {spec['vocab_size']} rounded up to a multiple of 8: with the published one the HIP sampler and the lm_head "
    f"GEMV fall back to torch, which is not timed here)")
say(f"# n = {n} tokens after a 128-token prompt, greedy, median of 3 per figure, {REPEATS} alternated repeats: median (min - max)")
step_error()
models = {}
for name, build, accel_kw in CASES:
    llm = build()
    info = accelerate_llm(llm, **accel_kw)
    models[name] = GraphedDecoder(llm, use_graph=True, fused_cache=bool(info.get("decode_attention")))
    say(f"# {name}: {type(llm).__name__}, decoder_layers_5_launches {info.get('decoder_layers_5_launches')}, "
        f"decode_prologue_1_launch {info.get('decode_prologue_1_launch')}, declined {info.get('decoder_layers_declined')}")
for B in rows:
    prompt = torch.randint(5, min(30000, vocab), (B, 128), generator=torch.Generator().manual_seed(B)).cuda()
    for name, _, _ in CASES:                        # warm-up of every case: capture both lengths
        for new in (1 + n, 1):
            models[name].generate(prompt, torch.ones_like(prompt), max_new_tokens=new, pad_token_id=0, eos_token_id=[], do_sample=False)
    res = {name: [] for name, _, _ in CASES}
    for _ in range(REPEATS):
        for name, _, _ in CASES:
            res[name].append(token_ms(models[name], prompt))
    for name, _, _ in CASES:
        say(f"{arch} rows {B:2d} {name}: decode token {fmt(res[name])}")
    f, u, l = (res[name] for name, _, _ in CASES)
    mf, mu, ml = (sorted(v)[1] for v in (f, u, l))
    say(f"{arch} rows {B:2d}: (ii) / (i) = {mu / mf:.3f} x by the medians; (i) median {'lies WITHIN' if min(l) <= mf <= max(l) else 'lies OUTSIDE'} "
        f"the spread of (iii) ({100 * (mf / ml - 1):+.2f} % against the (iii) median)")
models.clear()
torch.cuda.empty_cache()
if parent_tree:
    say(f"# llama-3.1-8b (no multipliers, existing kernels only): this tree against the parent commit, child processes taken alternately, {REPEATS} repeats")
    res = {"this": {str(B): [] for B in rows}, "parent": {str(B): [] for B in rows}}
    turns = [(who, tree) for _ in range(REPEATS) for who, tree in (("this", HERE), ("parent", os.path.abspath(parent_tree)))]
    for who, tree in turns:
        cmd = [sys.executable, os.path.abspath(__file__), "--llama-child", "--tree", tree, "--new", str(n), "--rows", ",".join(map(str, rows))]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tree)
            line = [x for x in out.stdout.splitlines() if x.startswith("LLAMA_CHILD ")]
            if out.returncode != 0 or not line:
                failed = f"child on {who} failed (exit {out.returncode}): {out.stderr[-300:]}"
        except subprocess.TimeoutExpired:
            failed = f"child on {who} ran into its time limit"
        if failed:
            break               # a child that failed may have faulted the device: nothing more is started on it, the comparison ends here
        for B, v in json.loads(line[0][len("LLAMA_CHILD "):]).items():
            res[who][B].append(v)
    if failed:
        say(f"# {failed}")
        say("# llama-3.1-8b against the parent commit: NOT measured (the comparison stopped at the first failed child)")
    for B in rows:
        t, p = res["this"][str(B)], res["parent"][str(B)]
        if not failed and len(t) == REPEATS and len(p) == REPEATS:
            mt = sorted(t)[1]
            say(f"llama-3.1-8b rows {B:2d}: this tree {fmt(t)}, parent {fmt(p)}; this median "
                f"{'lies WITHIN' if min(p) <= mt <= max(p) else 'lies OUTSIDE'} the parent's spread ({100 * (mt / sorted(p)[1] - 1):+.2f} % by the medians)")
else:
    say("# llama-3.1-8b against the parent commit: not measured in this run (no --parent-tree)")
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
sys.exit(1 if failed else 0)
