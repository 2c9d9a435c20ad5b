"""Decode token of one sequence (graphed, greedy, 64 tokens after a 128-token prompt, median of three per figure, three figures) of THIS checkout,
one line per process: python tools/decode_token_time.py MODEL LAYERS TAG  (MODEL: an entry of e2e.LLM_CONFIGS, LAYERS: decoder layers kept,
TAG: printed in front, e.g. the commit).  It is the unit of a commit-against-commit comparison: run it from a checkout of each commit in
alternated processes and compare the medians with the spread between the processes of one commit (profiles/decode_moe2_parent.txt)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llamole_amd import e2e  # noqa: E402
from llamole_amd.llm_accel import accelerate_llm  # noqa: E402
from llamole_amd.llm_decode import GraphedDecoder  # noqa: E402

arch, layers, tag = sys.argv[1], int(sys.argv[2]), sys.argv[3]
n = 64
llm = e2e.build_llm(arch, "cuda", torch.bfloat16, num_hidden_layers=layers)
e2e.randomize_head_norms(llm)
g = torch.Generator().manual_seed(3)
with torch.no_grad():
    for layer in llm.model.layers:
        if hasattr(layer.mlp, "gate"):
            layer.mlp.gate.weight.copy_((torch.randn(layer.mlp.gate.weight.shape, generator=g) * 0.2).to(torch.bfloat16))
info = accelerate_llm(llm)
dec = GraphedDecoder(llm, use_graph=True, fused_cache=True)
# ids below the model's vocabulary (a tiny model has 2048 tokens: an id beyond the embedding table is an out-of-bounds gather on the device)
prompt = torch.randint(5, min(30000, llm.config.vocab_size), (1, 128), generator=torch.Generator().manual_seed(1)).cuda()
kw = dict(pad_token_id=0, eos_token_id=[], do_sample=False)


def gen_ms(new):
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dec.generate(prompt, torch.ones_like(prompt), max_new_tokens=new, **kw)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[1]


for new in (1 + n, 1):
    dec.generate(prompt, torch.ones_like(prompt), max_new_tokens=new, **kw)
vals = [(gen_ms(1 + n) - gen_ms(1)) / n for _ in range(3)]
print(f"{tag} {arch} layers {layers} fused {info.get('decoder_layers_5_launches')}: decode token ms {sorted(vals)[1]:.4f} "
      f"(runs {', '.join(f'{v:.4f}' for v in vals)})", flush=True)
