"""Packed-weight decode kernels against their bf16 counterparts on the four matrices of a decoder layer:
python tools/wq_sweep.py [--model qwen2-7b llama-3.1-8b] [--rows 1 2 ...] [--repeats 3] [--sweep].
Per model, matrix (q|k|v with the RMSNorm prologue, o_proj + residual, gate|up with prologue and SiLU*mul, down_proj + residual), token-row
count (default 1..16) and width: microseconds per launch from HIP events over distinct weight buffers (more than the 256 MiB Infinity Cache
holds), bf16 / 8-bit / 4-bit taken alternately `repeats` times.  A packed kernel WINS at a row count when its slowest repeat is faster than
the fastest repeat of the bf16 kernel.  Up to LLAMOLE_FMA_GEMV_ROWS (2) rows run ll_gemv_fused_*, more rows ll_linear_rows16_*.  The last
lines are the routing table for llm_accel.WQ_ROUTES: per (bits, matrix) the row counts that win on every model given.  --sweep also times
every geometry of ll_linear_rows16_wq (one run each)."""
import ctypes as C
import os
import sys

os.environ.setdefault("LLAMOLE_TUNING", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (initialises the HIP runtime the library shares)

from llamole_amd import _lib, e2e  # noqa: E402

argv = sys.argv[1:]


def opt(name, default):
    if name not in argv:
        return default
    vals = []
    for a in argv[argv.index(name) + 1:]:
        if a.startswith("--"):
            break
        vals.append(a)
    return vals


models = opt("--model", ["qwen2-7b"])
rows = [int(a) for a in opt("--rows", list(range(1, 17)))]
repeats = int(opt("--repeats", [3])[0])
lib = _lib.load()
FMA_ROWS = int(os.environ.get("LLAMOLE_FMA_GEMV_ROWS", "2"))
ITERS = 40
KEYS = {"q|k|v": "qkv", "o_proj": "o", "gate|up": "gate_up", "down_proj": "down"}


def nweights(nbytes):
    return max(4, -(-640 * 2 ** 20 // nbytes))


def bench(bits, M, N, K, epi, norm):
    ms = C.c_float()
    nr = (2 if epi == 2 else 1) * N
    if bits is None:
        nw = nweights(nr * K * 2)
        if M <= FMA_ROWS:
            _lib.check(lib.ll_gemv_fused_bench(M, N, K, epi, norm, 1, ITERS, nw, C.byref(ms)))
        else:
            _lib.check(lib.ll_rows16_bench(M, N, K, epi, norm, ITERS, nw, C.byref(ms)))
    else:
        nw = nweights(int(lib.ll_wq_bytes(nr, K, bits)))
        _lib.check(lib.ll_wq_bench(0 if M <= FMA_ROWS else 1, bits, M, N, K, epi, norm, ITERS, nw, C.byref(ms)))
    return ms.value * 1e3


wins = {}           # (bits, key) -> per model the set of winning row counts
for model in models:
    cfg = e2e.LLM_CONFIGS[model]
    H, I = cfg["hidden_size"], cfg["intermediate_size"]
    D = H // cfg["num_attention_heads"]
    NQKV = H + 2 * cfg["num_key_value_heads"] * D
    SHAPES = [("q|k|v", NQKV, H, 0, 1), ("o_proj", H, H, 1, 0), ("gate|up", I, H, 2, 1), ("down_proj", H, I, 1, 0)]      # name, N, K, epi, norm
    print(f"# {model}: hidden {H}, intermediate {I}; us per launch (min of {repeats} alternated repeats; [min-max]), HIP events, {ITERS} launches "
          f"over distinct weight buffers; WIN = slowest packed repeat < fastest bf16 repeat")
    for M in rows:
        for name, N, K, epi, norm in SHAPES:
            nr = (2 if epi == 2 else 1) * N
            t = {None: [], 8: [], 4: []}
            for _ in range(repeats):
                for bits in (None, 8, 4):
                    t[bits].append(bench(bits, M, N, K, epi, norm))
            b = t[None]
            line = f"{model} rows {M:2d} {name:9s} [{nr} x {K}] bf16 {min(b):7.2f} [{min(b):.2f}-{max(b):.2f}] {nr * K * 2 / min(b) / 1e6:5.2f} TB/s"
            for bits in (8, 4):
                v = t[bits]
                win = max(v) < min(b)
                wins.setdefault((bits, KEYS[name]), {}).setdefault(model, set())
                if win:
                    wins[(bits, KEYS[name])][model].add(M)
                pb = int(lib.ll_wq_bytes(nr, K, bits))
                line += (f" | {bits}-bit {min(v):7.2f} [{min(v):.2f}-{max(v):.2f}] {pb / min(v) / 1e6:5.2f} TB/s x{min(v) / min(b):.3f} "
                         f"{'WIN ' if win else 'lose'}")
            print(line, flush=True)
            if "--sweep" in argv and M > FMA_ROWS:
                for bits in (8, 4):
                    for geom in [(c, w, k) for c in ((128, 256) if bits == 8 else (128,)) for w in (4, 8) for k in (1, 2, 4, 8) if k <= w]:
                        if geom[1] * (3 if epi == 2 else 2) * 16 * (geom[0] * 16 // bits + 16) > 160 * 1024:
                            continue                      # the LDS images of this geometry exceed a CU's 160 KB
                        lib.ll_set_wq_geometry(*geom)
                        try:
                            tt = bench(bits, M, N, K, epi, norm)
                        finally:
                            lib.ll_set_wq_geometry(0, 0, 0)
                        print(f"    {bits}-bit cseg {geom[0]} waves {geom[1]} ksplit {geom[2]}: {tt:7.2f} us", flush=True)
print(f"# routing table: row counts that win on every model of {models}")
for (bits, key), per in sorted(wins.items(), reverse=True):
    both = set.intersection(*per.values()) if per else set()
    print(f"ROUTE ({bits}, \"{key}\"): {sorted(both)}", flush=True)
