"""Decode token of the graphed decoder with quantization_bit off, 8 and 4 (random bf16 weights):
python tools/decode_quant_time.py [--out profiles/decode_quant_time.txt] [--new N] [--only qwen2-7b] [--all-routes].
Qwen2-7B shapes at 1, 2, 6 and 16 token rows and Llama-3.1-8B at 1 row.  Per shape three models (bf16, 8-bit, 4-bit) live in one process;
the token time is (generate(1 + n) - generate(1)) / n with n = 128, median of 3, greedy, after a 128-token prompt, and the three cases are
taken alternately (twice) after a warm-up of every case, so they see the same clocks.  The yardstick is the bf16 token of the same run;
the floor no kernel can beat is the ratio of the bytes a token streams (layer weights at 1.03125 / 0.53125 bytes + the bf16 lm_head).
A case "wins" when its slowest repeat is faster than the fastest repeat of the case it is compared with."""
import os
import sys

os.environ.setdefault("LLAMOLE_TUNING", "1")
os.environ.pop("LLAMOLE_QUANT_BITS", None)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llamole_amd import e2e, llm_accel  # noqa: E402
from llamole_amd.llm_accel import accelerate_llm  # noqa: E402
from llamole_amd.llm_decode import GraphedDecoder  # noqa: E402

argv = sys.argv[1:]
n = int(argv[argv.index("--new") + 1]) if "--new" in argv else 128
out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join("profiles", "decode_quant_time.txt")
only = argv[argv.index("--only") + 1] if "--only" in argv else None
all_routes = "--all-routes" in argv          # time the packed kernels even where the product routes a pair to the bf16 kernels
PLAN = [("qwen2-7b", (1, 2, 6, 16)), ("llama-3.1-8b", (1,))]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def stream_bytes(llm, bits):
    """Bytes of weights one decode token reads: the decoder-layer Linears (packed or bf16) + lm_head."""
    c = llm.config
    H, I, D = c.hidden_size, c.intermediate_size, c.hidden_size // c.num_attention_heads
    per_layer = H * (H + 2 * c.num_key_value_heads * D) + H * H + 3 * H * I
    w = per_layer * c.num_hidden_layers
    return w * (2 if bits is None else bits / 8 + 1 / 32) + 2 * c.vocab_size * H


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


if all_routes:
    llm_accel.WQ_ROUTES.update(llm_accel.all_packed_routes())
say(f"# decode token, quantization_bit off / 8 / 4; n = {n} tokens after a 128-token prompt, greedy, median of 3, two alternated repeats")
say(f"# packed routes (token rows per matrix): {dict((f'{b}-bit {k}', sorted(v)) for (b, k), v in llm_accel.WQ_ROUTES.items())}")
for arch, row_counts in PLAN:
    if only and arch != only:
        continue
    models = {}
    for bits in (None, 8, 4):
        llm = e2e.build_llm(arch, "cuda", torch.bfloat16)
        info = accelerate_llm(llm, quantization_bit=bits)
        models[bits] = (llm, GraphedDecoder(llm, use_graph=True, fused_cache=bool(info.get("decode_attention"))), info.get("quantization"))
    q8 = models[8][2]
    say(f"# {arch}: {q8['modules']} Linears rounded, packed {q8['packed_bytes'] / 1e9:.3f} GB at 8 bits, "
        f"{models[4][2]['packed_bytes'] / 1e9:.3f} GB at 4 bits, bf16 {q8['bf16_bytes'] / 1e9:.3f} GB")
    base_bytes = stream_bytes(models[None][0], None)
    for B in row_counts:
        prompt = torch.randint(5, 30000, (B, 128), generator=torch.Generator().manual_seed(B)).cuda()
        for bits in (None, 8, 4):                       # warm-up of every case: capture both lengths
            for new in (1 + n, 1):
                models[bits][1].generate(prompt, torch.ones_like(prompt), max_new_tokens=new, pad_token_id=0, eos_token_id=[], do_sample=False)
        res = {None: [], 8: [], 4: []}
        for _ in range(2):
            for bits in (None, 8, 4):
                dec = models[bits][1]
                res[bits].append((gen_ms(dec, prompt, 1 + n) - gen_ms(dec, prompt, 1)) / n)
        for bits in (None, 8, 4):
            v = res[bits]
            name = "bf16 " if bits is None else f"{bits}-bit"
            floor = stream_bytes(models[bits][0], bits) / base_bytes
            rel = ""
            if bits is not None:
                ratio = min(v) / min(res[None])
                prev = res[None] if bits == 8 else res[8]
                verdict = "wins" if max(v) < min(prev) else "DOES NOT WIN"
                rel = (f"  = {ratio:.3f} x bf16 (byte-ratio floor {floor:.3f}; reaches {100 * (1 - ratio) / (1 - floor):.0f} % of the byte-ratio gain); "
                       f"{verdict} against {'bf16' if bits == 8 else '8-bit'} beyond the spread of the repeats")
            say(f"{arch} rows {B:2d} {name}: decode token {min(v):.4f} ms (runs {', '.join(f'{x:.4f}' for x in v)}; spread {max(v) - min(v):.4f}){rel}")
    del models
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
