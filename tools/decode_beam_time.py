"""Beam-search decode token of the graphed decoder on Qwen2-7B shapes (random bf16 weights): python tools/decode_beam_time.py [B ...]
[--new N] [--no-hf].  Per batch size B (default 1 and 6, the eval batch) and nb = 4, greedy beam and beam sample (temperature 0.6,
top_p 0.9, top_k 50) against the plain greedy token at the same row count B * nb, taken alternately in one process.  The token time is
(generate(1 + n) - generate(1)) / n, median of 3, after a 128-token prompt.  The EOS list holds 10 ids (K = 44) that the seeded run
never emits -- checked on the outputs -- so every run decodes all n tokens.  HF's own generate(num_beams=4) on the same accelerated
model is printed as a baseline (one run, total / n)."""
import os
import sys
import time

os.environ.setdefault("LLAMOLE_TUNING", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llamole_amd import e2e  # noqa: E402
from llamole_amd.llm_accel import accelerate_llm  # noqa: E402
from llamole_amd.llm_decode import GraphedDecoder  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(sys.argv[sys.argv.index("--new") + 1]) if "--new" in sys.argv else 128
if "--new" in sys.argv:
    args.remove(str(n))
batches = [int(a) for a in args] or [1, 6]
NB = 4
llm = e2e.build_llm("qwen2-7b", "cuda", torch.bfloat16)
info = accelerate_llm(llm)
V = llm.config.vocab_size
EOS = list(range(V - 10, V))                 # K = (1 + 10) * 4 = 44
dec = GraphedDecoder(llm, use_graph=True, fused_cache=bool(info.get("decode_attention")))
CASES = {"greedy beam": dict(do_sample=False, num_beams=NB),
         "beam sample": dict(do_sample=True, temperature=0.6, top_p=0.9, top_k=50, num_beams=NB),
         "greedy (no beams)": dict(do_sample=False)}


def run(prompt, kw, new):
    out = dec.generate(prompt, torch.ones_like(prompt), max_new_tokens=new, pad_token_id=0, eos_token_id=EOS,
                       generator=torch.Generator(device="cuda").manual_seed(0), **kw)
    return out


def gen_ms(prompt, kw, new):
    out = run(prompt, kw, new)                # capture / warm-up
    assert out.shape[1] == prompt.shape[1] + new and not bool(torch.isin(out[:, prompt.shape[1]:], torch.tensor(EOS, device="cuda")).any()), \
        "an EOS id of the timing list was emitted: pick others"
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(prompt, kw, new)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[1]


for B in batches:
    g = torch.Generator().manual_seed(B)
    prompt = torch.randint(5, 30000, (B, 128), generator=g).cuda()
    wide = prompt.repeat_interleave(NB, dim=0)          # the plain greedy decode at the same row count B * nb
    res = {}
    for _ in range(2):                                  # alternated: every case sees the same clocks
        for name, kw in CASES.items():
            p = wide if "no beams" in name else prompt
            res.setdefault(name, []).append((gen_ms(p, kw, 1 + n) - gen_ms(p, kw, 1)) / n)
    base = min(res["greedy (no beams)"])
    for name, v in res.items():
        rel = "" if "no beams" in name else f"  = {min(v) / base:.3f} x greedy at {B * NB} rows"
        print(f"B={B} nb={NB} {name}: decode token {min(v):.4f} ms ({n} tokens after a 128-token prompt; runs "
              f"{', '.join(f'{x:.4f}' for x in v)}){rel}", flush=True)
    if "--no-hf" not in sys.argv:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = llm.generate(inputs=prompt, attention_mask=torch.ones_like(prompt), max_new_tokens=n, do_sample=False, num_beams=NB,
                           pad_token_id=0, eos_token_id=EOS)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        print(f"B={B} nb={NB} HF generate(num_beams={NB}) on the same accelerated model: {ms / (out.shape[1] - 128):.4f} ms per token "
              f"(total {ms:.1f} ms incl. prefill, {out.shape[1] - 128} tokens; baseline, not gated)", flush=True)
