"""Decode token of the graphed decoder on a Qwen3-layout model (per-head q / k RMSNorm) at Qwen3-8B widths (random bf16 weights, the norm
weights drawn by e2e.randomize_head_norms):
python tools/decode_qwen3_time.py [--out profiles/decode_qwen3_time.txt] [--new N] [--rows 1,16,64] [--arch qwen3-8b]  (--arch: any Qwen3 entry
of e2e.LLM_CONFIGS, e.g. tiny-qwen3 for a dry run).
Three models live in one process:
  (i)   the fused stack (five- / seven-launch layers with the norm inside the attention launch, one-launch prologue);
  (ii)  the same model with accelerate_llm(layers=False): what a model with q_norm / k_norm ran until the layout was accepted (fused Linears,
        RMSNorm, rotary and attention kernels op by op under HF's layer code, HF's rotary module and mask construction per token);
  (iii) a Llama-layout model of the same widths (same hidden / heads / head_dim / intermediate / vocabulary, no q / k norm, no bias): the same
        launches as (i) without the norm, i.e. what the norm costs inside the attention launch.
Per row count every case sees the same prompts; the token time is (generate(1 + n) - generate(1)) / n, median of 3, greedy, after a 128-token
prompt, and the cases are taken alternately over three repeats after a warm-up of every case.  No ratio is fixed in advance: the tool prints
per row count whether (ii)'s repeats lie above (i)'s beyond the spread, and whether (i)'s median lies within the spread of (iii)'s repeats.
The file starts with the error of one fused decode step of tiny-qwen3 against HF in f32, next to HF's own bf16 (the figures
tests/test_qwen3_decode_gpu.py asserts on)."""
import copy
import os
import sys

os.environ.setdefault("LLAMOLE_TUNING", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llamole_amd import e2e  # noqa: E402
from llamole_amd.llm_accel import (accelerate_llm, restore_decoder_layers, restore_elementwise, restore_linears,  # noqa: E402
                                   restore_model_decode)
from llamole_amd.llm_decode import GraphedDecoder  # noqa: E402

argv = sys.argv[1:]
n = int(argv[argv.index("--new") + 1]) if "--new" in argv else 128
out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join("profiles", "decode_qwen3_time.txt")
rows = tuple(int(x) for x in argv[argv.index("--rows") + 1].split(",")) if "--rows" in argv else (1, 16, 64)
arch = argv[argv.index("--arch") + 1] if "--arch" in argv else "qwen3-8b"
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


def step_error():
    """one fused decode step of tiny-qwen3 (3 left-padded rows of 13 tokens) against the untouched HF model in f32; HF's bf16 next to it"""
    llm = e2e.build_llm("tiny-qwen3", "cuda", torch.bfloat16)
    e2e.randomize_head_norms(llm)
    hf16, hf32 = copy.deepcopy(llm), copy.deepcopy(llm).float()
    prompt = torch.randint(5, 2000, (3, 13), generator=torch.Generator().manual_seed(13)).cuda()
    mask = torch.ones_like(prompt)
    mask[1, :4] = 0
    mask[2, :7] = 0
    accelerate_llm(llm)
    try:
        dec = GraphedDecoder(llm, use_graph=False, fused_cache=True)
        toks = dec.generate(prompt, mask, max_new_tokens=2, do_sample=False, pad_token_id=0, eos_token_id=[])
        fused = dec.last_logits.float().clone()
    finally:
        restore_model_decode(llm), restore_decoder_layers(llm), restore_elementwise(llm), restore_linears(llm)
    ids, full = toks[:, :14], torch.cat([mask, torch.ones_like(mask[:, :1])], dim=1)
    pos = (full.long().cumsum(dim=1) - 1).clamp_min(0)
    with torch.no_grad():
        ref, b16 = (m(input_ids=ids, attention_mask=full, position_ids=pos, use_cache=False).logits[:, -1, :].float() for m in (hf32, hf16))
    E, Y = float((fused - ref).abs().max()), float((b16 - ref).abs().max())
    say(f"tiny-qwen3, one fused decode step against HF f32 (max |logit error|): fused E = {E:.5f}, HF bf16 Y = {Y:.5f}, E / Y = {E / Y:.3f}")


llama_twin = dict(e2e.LLM_CONFIGS[arch], cls="Llama", attention_bias=False)
CASES = (("(i) fused", lambda: e2e.build_llm(arch, "cuda", torch.bfloat16), {}),
         ("(ii) layers=False", lambda: e2e.build_llm(arch, "cuda", torch.bfloat16), dict(layers=False)),
         ("(iii) Llama layout, no q/k norm", lambda: e2e.build_llm("tiny-llama", "cuda", torch.bfloat16, **llama_twin), {}))
say(f"# decode token at {arch} widths: per-head q / k RMSNorm inside the fused attention launch")
say(f"# n = {n} tokens after a 128-token prompt, greedy, median of 3 per figure, {REPEATS} alternated repeats")
step_error()
models = {}
for name, build, accel_kw in CASES:
    llm = build()
    e2e.randomize_head_norms(llm)
    info = accelerate_llm(llm, **accel_kw)
    models[name] = GraphedDecoder(llm, use_graph=True, fused_cache=bool(info.get("decode_attention")))
    say(f"# {name}: {type(llm).__name__}, decoder_layers_5_launches {info.get('decoder_layers_5_launches')}, "
        f"decode_prologue_1_launch {info.get('decode_prologue_1_launch')}, declined {info.get('decoder_layers_declined')}")
for B in rows:
    prompt = torch.randint(5, min(30000, e2e.LLM_CONFIGS[arch]["vocab_size"]), (B, 128), generator=torch.Generator().manual_seed(B)).cuda()
    for name, _, _ in CASES:                        # warm-up of every case: capture both lengths
        for new in (1 + n, 1):
            models[name].generate(prompt, torch.ones_like(prompt), max_new_tokens=new, pad_token_id=0, eos_token_id=[], do_sample=False)
    res = {name: [] for name, _, _ in CASES}
    for _ in range(REPEATS):
        for name, _, _ in CASES:
            res[name].append((gen_ms(models[name], prompt, 1 + n) - gen_ms(models[name], prompt, 1)) / n)
    med = {}
    for name, _, _ in CASES:
        v = res[name]
        med[name] = sorted(v)[len(v) // 2]
        say(f"{arch} rows {B:2d} {name}: decode token median {med[name]:.4f} ms (runs {', '.join(f'{x:.4f}' for x in v)}; spread {max(v) - min(v):.4f})")
    f, u, l = (res[name] for name, _, _ in CASES)
    mf, mu, ml = (med[name] for name, _, _ in CASES)
    say(f"{arch} rows {B:2d}: (ii) / (i) = {mu / mf:.3f} x by the medians; every (ii) repeat {'lies ABOVE' if min(u) > max(f) else 'does NOT lie above'} "
        f"every (i) repeat ([{min(u):.4f}, {max(u):.4f}] against [{min(f):.4f}, {max(f):.4f}])")
    say(f"{arch} rows {B:2d}: (i) median {mf:.4f} ms {'lies WITHIN' if min(l) <= mf <= max(l) else 'lies OUTSIDE'} the spread of (iii) "
        f"[{min(l):.4f}, {max(l):.4f}] ({100 * (mf / ml - 1):+.2f} % against the (iii) median)")
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
