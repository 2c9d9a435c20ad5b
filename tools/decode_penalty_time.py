"""Decode-token time of the graphed decoder on Qwen2-7B shapes (random bf16 weights), repetition_penalty off (1.0) and on (1.3):
python tools/decode_penalty_time.py [batch] [new_tokens].  The token time is (generate(1 + n) - generate(1)) / n, median of 3, with
temperature 0.6, top_k 50, top_p 0.9 and no EOS, on the bench's stack (HIP layers, fused KV append, one hipGraph per token)."""
import os
import sys

os.environ.setdefault("LLAMOLE_TUNING", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llamole_amd import e2e  # noqa: E402
from llamole_amd.llm_accel import accelerate_llm  # noqa: E402
from llamole_amd.llm_decode import GraphedDecoder  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1
n = int(sys.argv[2]) if len(sys.argv) > 2 else 128
llm = e2e.build_llm("qwen2-7b", "cuda", torch.bfloat16)
info = accelerate_llm(llm)
dec = GraphedDecoder(llm, use_graph=True, fused_cache=bool(info.get("decode_attention")))
g = torch.Generator().manual_seed(0)
prompt = torch.randint(5, 30000, (B, 128), generator=g).cuda()
mask = torch.ones_like(prompt)


def gen_ms(p, new):
    kw = dict(max_new_tokens=new, do_sample=True, temperature=0.6, top_k=50, top_p=0.9, pad_token_id=0, repetition_penalty=p)
    dec.generate(prompt, mask, **kw)            # capture / warm-up
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dec.generate(prompt, mask, **kw)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[1]


res = {}
for p in (1.0, 1.3, 1.0, 1.3):                  # interleaved: both see the same clocks
    res.setdefault(p, []).append((gen_ms(p, 1 + n) - gen_ms(p, 1)) / n)
for p, v in res.items():
    print(f"repetition_penalty {p}: decode token {min(v):.4f} ms (B={B}, {n} tokens after a 128-token prompt; runs {', '.join(f'{x:.4f}' for x in v)})")
off, on = min(res[1.0]), min(res[1.3])
print(f"penalty on vs off: {100 * (on - off) / off:+.2f} %")
