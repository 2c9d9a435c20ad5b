"""Optional MI355X acceleration of the untouched HuggingFace LLM's decode step.

The HF model code is not modified; what changes is the kernel underneath its modules for decode-shaped calls (bf16, no grad):
  * 1-2 sequences : five launches per decoder layer on the f32-FMA GEMVs (RMSNorm prologue, residual / SiLU*mul epilogues; bit-identical
                    to HF's op order), rope + KV append + attention in one launch, one-launch prologue and sampler;
  * 3-16 sequences: the same five launches on the weight-streaming MFMA Linear (``ll_linear_rows16_bf16``);
  * 17-64 sequences (round 6): seven launches per layer on copies of the weights in MFMA operand order (``ll_linear_rows64_bf16``), the
                    RMSNorm between two Linears split over producer and consumer, grouped-query attention with one workgroup per
                    (KV head, sequence) -- the batch the reference's DataLoader hands ``language_model.generate`` (eval/workflow.py:89-91);
  * anything else (prefill, larger batches, a dynamic cache) falls through to the HF code, with ``ll_linear`` under ``nn.Linear`` up to 128 rows.
Everything is enqueued on the caller's current stream, so it composes with the captured hipGraph of ``llm_decode.GraphedDecoder``.
"""
from __future__ import annotations

import os
import types
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .llm_quant import check_quantization_bit, quantize_llm, reround_changed
from .rope import STATIC_ROPE_TYPES, dynamic_inv_freq_table

MAX_ROWS = 128           # GEMV / skinny-GEMM path under nn.Linear (128-token prefill: 8.7 ms vs 10.0 ms on hipBLASLt, tools/prefill_probe.py)
MAX_ROWS16 = 16         # ll_linear_rows16_bf16: one MFMA column block of token rows (batched decode: 3..16 sequences)
MAX_STREAM_ROWS = 64    # ll_linear_rows64_bf16: up to four column blocks per weight fragment (17..64 sequences per GPU, BASELINE configs[3])
# up to here the f32-FMA GEMVs run (RMSNorm prologue fused, bit-identical to the op-by-op path); from the next row count on the MFMA
# stream does (tools/batch_sweep.sh: batch 4 = 603 ms per step on the FMA path vs 467 ms, batch 2 = 456 vs 439 ms -- the default
# stays at 2 so that two-sequence decode keeps the bit-identity with HF's op order; LLAMOLE_FMA_GEMV_ROWS=1 trades it for the 4 %)
FMA_GEMV_ROWS = int(os.environ.get("LLAMOLE_FMA_GEMV_ROWS", "2"))
PACK64_MIN_N = 32768    # nn.Linear modules at least this wide (lm_head) keep a packed copy for 17..64 rows
ATTN_MAXLEN = 16384             # cache slots of ll_decode_attn_bf16 / ll_decode_attn_rope*_bf16 / ll_suffix_attn_rope*_bf16 (scores of all keys in LDS)
ATTN_SPLIT_MAXLEN = 131072      # cache slots of the key-split entries (ll_*_attn_rope_split_bf16), taken only beyond ATTN_MAXLEN
MAX_APPEND_ROWS = 16     # new positions per call served by the fused KV append / decode attention (decode, query tail)
# row-parallel elementwise kernels (RMSNorm, rotary, SiLU*mul) also serve prefill-sized calls.  Round 3: the A* value estimates push
# 256 prompts x ~144 tokens = 37 k rows through the model per forward; above the old 16 k-row limit HF's op-by-op RMSNorm (pow, mean, rsqrt,
# two casts, two multiplies: ~0.7 ms per norm at 37 k x 3584) and act_fn(gate) * up (1.3 ms per layer) were 17 % of that forward
MAX_EW_ROWS = 1 << 20
# vocabulary-sized outputs for a few hundred rows (the lm_head of a batched `logits_to_keep = 1` forward: 256 x 152 064 x 3584): hipBLASLt
# picks a 256 x 16 tile there and takes 32 ms (8.6 TFLOP/s); the LDS-DMA ring GEMM streams the 1.09 GB of weights once
MAX_WIDE_ROWS, WIDE_N = 1024, 65536
PREFILL_SPLITK = os.environ.get("LLAMOLE_PREFILL_SPLITK", "1") != "0"
# quantization_bit (llm_quant.py): at which token-row counts a matrix of a fused layer ("qkv", "o", "gate_up", "down") streams its packed MX
# codes -- up to FMA_GEMV_ROWS rows through ll_gemv_fused_wq, above through ll_linear_rows16_wq.  A row count is listed only where the
# packed kernel beat the bf16 kernel it replaces by more than the spread of the alternated repeats (tools/wq_sweep.py,
# profiles/decode_quant_kernels.txt; decode token: profiles/decode_quant_time.txt); everywhere else the bf16 kernels run on the
# dequantised weights, which is the same model.  The table was measured with FMA_GEMV_ROWS = 2: another value switches the packed route off.
WQ_MATRICES = ("qkv", "o", "gate_up", "down")
# Row counts that won on BOTH Qwen2-7B and Llama-3.1-8B shapes; o_proj, whose verdict flips between neighbouring row counts (within 4 %
# of the bf16 kernel either way), stays on the bf16 kernel.
WQ_ROUTES = {
    (8, "qkv"): frozenset({2}), (8, "o"): frozenset(), (8, "gate_up"): frozenset(range(2, 17)), (8, "down"): frozenset(range(2, 17)),
    (4, "qkv"): frozenset({2}), (4, "o"): frozenset(), (4, "gate_up"): frozenset({1, 2}), (4, "down"): frozenset(range(1, 17)),
}


def all_packed_routes() -> dict:
    """Every (bits, matrix) at every row count 1..16: what the tests and the A/B timing put into ``WQ_ROUTES`` to run the packed kernels
    whatever the measured routing switched on."""
    return {(b, m): frozenset(range(1, MAX_ROWS16 + 1)) for b in (8, 4) for m in WQ_MATRICES}


def _versions(*tensors):
    return tuple((t.data_ptr(), t._version) for t in tensors if t is not None)


class _Packed64:
    """A weight in MFMA operand order for ll_linear_rows64_bf16 (made once by ll_rows64_pack_bf16; the same size as the weight).  The copy
    follows its source: ``sync`` re-packs IN PLACE when (data_ptr, _version) of the sources changed (captured graphs hold its address)."""

    def __init__(self, lib, w: torch.Tensor, key):
        self.rows, self.K = w.shape
        n = int(lib.ll_rows64_packed_elems(self.rows, self.K))
        if n < 0:
            raise ValueError(f"ll_rows64_pack_bf16: K={self.K} must be a multiple of 32")
        self.t = torch.empty(n, dtype=torch.bfloat16, device=w.device)
        self.key = None
        self.sync(lib, w, key)

    def sync(self, lib, w: torch.Tensor, key) -> bool:
        if self.key == key:
            return False
        assert w.shape == (self.rows, self.K) and w.stride(1) == 1
        rc = lib.ll_rows64_pack_bf16(w.data_ptr(), w.stride(0), self.rows, self.K, self.t.data_ptr(), torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _lib.check(rc, "ll_rows64_pack_bf16")
        self.key = key
        return True


class _PackedWQ:
    """The MX codes + scale bytes of a (rounded) bf16 weight for ll_gemv_fused_wq / ll_linear_rows16_wq, made by ll_wq_quantize_bf16.  Like
    ``_Packed64`` the copy follows its source: ``sync`` re-quantises IN PLACE when the key changed (captured graphs hold its address)."""

    def __init__(self, lib, w: torch.Tensor, bits: int, key):
        self.rows, self.K = w.shape
        self.bits = bits
        n = int(lib.ll_wq_bytes(self.rows, self.K, bits))
        if n < 0:
            raise ValueError(f"ll_wq_quantize_bf16: K={self.K} must be a multiple of 32 and bits={bits} one of 4, 8")
        self.t = torch.empty(n, dtype=torch.uint8, device=w.device)
        self.key = None
        self.sync(lib, w, key)

    def sync(self, lib, w: torch.Tensor, key) -> bool:
        if self.key == key:
            return False
        assert w.shape == (self.rows, self.K) and w.stride(1) == 1
        rc = lib.ll_wq_quantize_bf16(w.data_ptr(), w.stride(0), self.rows, self.K, self.bits, self.t.data_ptr(), None, 0,
                                     torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _lib.check(rc, "ll_wq_quantize_bf16")
        self.key = key
        return True


def _rows64(lib, x2, ldx, wp: "_Packed64", bias, res, N, epi, row_ssq=None, eps=0.0, next_norm=None, rscale=None):
    """17..64 token rows through ll_linear_rows64_bf16 on a packed weight; matrices with few 64-row groups (o_proj, down_proj) get scratch
    for the cross-workgroup K split (f32 slabs summed in slice order by a second launch on the same stream).
    ``row_ssq`` [M, chunks] f32: x2 is a pre-scaled row bf16(h * w_norm) and the accumulator is multiplied by rsqrt(mean(h^2) + eps).
    ``next_norm``: also return (bf16(out * next_norm), per-chunk sums of out^2) -- the two halves of the NEXT Linear's RMSNorm.
    ``rscale`` (residual epilogue only): the layer's residual_multiplier -- the call goes to ll_linear_rows64_rs_bf16."""
    M, K = x2.shape[0], wp.K
    out = torch.empty(M, N, dtype=torch.bfloat16, device=x2.device)
    xs = ssq = None
    if next_norm is not None:
        xs = torch.empty(M, N, dtype=torch.bfloat16, device=x2.device)
        ssq = torch.empty(M, int(lib.ll_rows64_ssq_chunks(N)), dtype=torch.float32, device=x2.device)
    ws, wsb = None, 0
    if epi != 2 and (next_norm is not None or N < 192 * 64):
        wsb = int(lib.ll_linear_rows64_workspace_bytes(M, N))
        ws = torch.empty(wsb, dtype=torch.uint8, device=x2.device)
    head = (x2.data_ptr(), ldx, wp.t.data_ptr(), bias.data_ptr() if bias is not None else None,
            res.data_ptr() if res is not None else None, res.stride(0) if res is not None else 0, out.data_ptr(), N, M, N, K)
    tail = (row_ssq.data_ptr() if row_ssq is not None else None, row_ssq.shape[1] if row_ssq is not None else 0, eps,
            next_norm.data_ptr() if next_norm is not None else None, xs.data_ptr() if xs is not None else None, N,
            ssq.data_ptr() if ssq is not None else None, ws.data_ptr() if ws is not None else None, wsb)
    if rscale is not None:
        assert epi == 1, "the scaled residual epilogue stands in for the residual epilogue only"
        name = "ll_linear_rows64_rs_bf16"
        rc = lib.ll_linear_rows64_rs_bf16(*head, *tail, rscale, torch.cuda.current_stream().cuda_stream)
    else:
        name = "ll_linear_rows64_bf16"
        rc = lib.ll_linear_rows64_bf16(*head, epi, *tail, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        _lib.check(rc, name)
    return out if next_norm is None else (out, xs, ssq)


def _prenorm64(lib, x2, norm_w):
    """(bf16(x * norm_w), per-chunk sums of x^2) of rows that no ll_linear_rows64_bf16 call produced (the embedding rows)."""
    M, N = x2.shape
    xs = torch.empty(M, N, dtype=torch.bfloat16, device=x2.device)
    ssq = torch.empty(M, int(lib.ll_rows64_ssq_chunks(N)), dtype=torch.float32, device=x2.device)
    rc = lib.ll_rows64_prenorm_bf16(x2.data_ptr(), x2.stride(0), norm_w.data_ptr(), xs.data_ptr(), N, ssq.data_ptr(), M, N,
                                    torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        _lib.check(rc, "ll_rows64_prenorm_bf16")
    return xs, ssq


def _hip_linear_forward(self: nn.Linear, x: torch.Tensor) -> torch.Tensor:
    K = self.in_features
    if (x.is_cuda and x.dtype == torch.bfloat16 and self.weight.dtype == torch.bfloat16 and not torch.is_grad_enabled()
            and (x.numel() // K <= MAX_ROWS or (x.numel() // K <= MAX_WIDE_ROWS and self.out_features >= WIDE_N)) and x.shape[-1] == K
            and (K % 64 == 0 or (x.numel() // K <= 4 and K % 8 == 0))):      # gemm_dispatch: K % 64 == 0 beyond the 4-row GEMV
        x2 = x.reshape(-1, K)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        M, N = x2.shape[0], self.out_features
        out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
        if (FMA_GEMV_ROWS < M <= MAX_ROWS16 or (MAX_ROWS16 < M <= MAX_STREAM_ROWS and N >= PACK64_MIN_N)) and K % 32 == 0:
            # 3..16 token rows (batched decode): the weight-streaming MFMA Linear, every wave streaming its own 16 weight rows;
            # 17..64 rows x a vocabulary-sized matrix (lm_head): ll_linear_rows64_bf16 on a packed copy (the decoder layers' own
            # Linears get theirs in _FusedLayer; any other module keeps the ring GEMM below rather than a second copy of its weight)
            bias = None
            if self.bias is not None:
                bias = getattr(self, "_ll_bias_f32", None)
                if bias is None or bias.device != x.device:
                    bias = self.bias.detach().float().contiguous()
                    self._ll_bias_f32, self._ll_bias_key = bias, _versions(self.bias)
            if M > MAX_ROWS16:
                wp = self.__dict__.get("_ll_w64")
                if wp is None:
                    wp = self._ll_w64 = _Packed64(self._ll_lib, self.weight.detach(), _versions(self.weight))
                return _rows64(self._ll_lib, x2, K, wp, bias, None, N, 0).reshape(*x.shape[:-1], N)
            rc = self._ll_lib.ll_linear_rows16_bf16(x2.data_ptr(), K, self.weight.data_ptr(), K, bias.data_ptr() if bias is not None else None,
                                                    None, 0.0, None, 0, out.data_ptr(), N, M, N, K, 0, torch.cuda.current_stream().cuda_stream)
            if rc != 0:
                _lib.check(rc, "ll_linear_rows16_bf16")
            return out.reshape(*x.shape[:-1], N)
        bias = None
        if self.bias is not None:
            bias = getattr(self, "_ll_bias_f32", None)
            if bias is None or bias.device != x.device:
                bias = self.bias.detach().float().contiguous()
                self._ll_bias_f32, self._ll_bias_key = bias, _versions(self.bias)
        splits = _prefill_splits(M, N, K)
        if splits > 1:
            ws = torch.empty(splits * M * N, dtype=torch.float32, device=x.device)
            rc = self._ll_lib.ll_linear_splitk_bf16(x2.data_ptr(), K, self.weight.data_ptr(), K, bias.data_ptr() if bias is not None else None,
                                                    out.data_ptr(), N, M, N, K, 0, splits, ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
            if rc != 0:
                _lib.check(rc, "ll_linear_splitk_bf16")
            return out.reshape(*x.shape[:-1], N)
        rc = self._ll_lib.ll_linear(_lib.LL_BF16, x2.data_ptr(), K, self.weight.data_ptr(), K,
                                    bias.data_ptr() if bias is not None else None, out.data_ptr(), N, M, N, K, 0, 0,
                                    torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _lib.check(rc, "ll_linear")
        return out.reshape(*x.shape[:-1], N)
    return F.linear(x, self.weight, self.bias)


def accelerate_linears(model: nn.Module, min_weight_elems: int = 1 << 16) -> int:
    """Route decode-shaped calls of every bf16 ``nn.Linear`` of ``model`` through ``ll_linear``.  Returns the number of
    patched modules.  Weights must stay where they are (the kernel reads ``module.weight`` in place)."""
    lib = _lib.load()
    n = 0
    for mod in model.modules():
        if (type(mod) is nn.Linear and mod.weight.dtype == torch.bfloat16 and mod.weight.is_cuda and mod.weight.is_contiguous()
                and mod.in_features % 8 == 0 and mod.weight.numel() >= min_weight_elems):
            mod._ll_lib = lib
            mod.forward = types.MethodType(_hip_linear_forward, mod)
            n += 1
    return n


def refresh_weight_copies(model: nn.Module) -> int:
    """The fused decode path keeps its own copies of some weights (q|k|v and gate|up concatenated once, biases in f32); a
    captured decode graph holds their ADDRESSES.  After the source weights changed (an SFT step, a merged LoRA adapter,
    load_state_dict) the copies are rewritten IN PLACE here -- same storage, so captured graphs stay valid -- keyed on
    (data_ptr, _version) of the sources, recorded when each copy is made.  GraphedDecoder.generate calls this before every
    generation (a few hundred tuple compares).  Returns the number of copies rewritten.  The copies cost about one extra set of
    MLP gate/up + attention q/k/v weights in memory (~8.5 GB for Qwen2-7B in bf16)."""
    n = 0
    with torch.no_grad():
        # quantization_bit: a rounded source weight that changed is rounded again first (in place; its key is recorded after the write), so
        # that every copy below is made from rounded weights
        n += reround_changed(model)
        for mod in model.modules():
            d = mod.__dict__
            q = getattr(mod, "q_proj", None)
            grp = q.__dict__.get("_ll_qkv") if isinstance(q, nn.Module) else None
            if grp is not None and isinstance(getattr(mod, "k_proj", None), nn.Module):
                k, v = mod.k_proj, mod.v_proj
                key = _versions(q.weight, k.weight, v.weight, q.bias, k.bias, v.bias)
                if grp.key != key:
                    grp.w.copy_(torch.cat([q.weight.detach(), k.weight.detach(), v.weight.detach()], dim=0))
                    if grp.bias is not None:
                        grp.bias.copy_(torch.cat([(m.bias.detach().float() if m.bias is not None else
                                                   torch.zeros(m.out_features, device=grp.bias.device)) for m in (q, k, v)]))
                    grp.key = key
                    n += 1
            if "_ll_gate_up" in d and isinstance(getattr(mod, "gate_proj", None), nn.Module):
                key = _versions(mod.gate_proj.weight, mod.up_proj.weight)
                if d.get("_ll_gate_up_key") != key:
                    d["_ll_gate_up"].copy_(torch.cat([mod.gate_proj.weight.detach(), mod.up_proj.weight.detach()], dim=0))
                    d["_ll_gate_up_key"] = key
                    n += 1
            if "_ll_router_gate" in d and isinstance(getattr(mod, "shared_expert_gate", None), nn.Module):
                # a shared-expert MoE block: the stacked [E + 1, H] copy of the router and the shared gate (_FusedMoeLayer)
                key = _versions(mod.gate.weight, mod.shared_expert_gate.weight)
                if d.get("_ll_router_gate_key") != key:
                    d["_ll_router_gate"].copy_(torch.cat([mod.gate.weight.detach(), mod.shared_expert_gate.weight.detach()], dim=0))
                    d["_ll_router_gate_key"] = key
                    n += 1
            if "_ll_bias_f32" in d and getattr(mod, "bias", None) is not None:
                key = _versions(mod.bias)
                if d.get("_ll_bias_key") != key:
                    d["_ll_bias_f32"].copy_(mod.bias.detach().float())
                    d["_ll_bias_key"] = key
                    n += 1
            st = d.get("_ll_fused")
            if st is not None and st.bo is not None:
                key = _versions(mod.self_attn.o_proj.bias)
                if st.bo_key != key:
                    st.bo.copy_(mod.self_attn.o_proj.bias.detach().float())
                    st.bo_key = key
                    n += 1
            wp = d.get("_ll_w64")
            if wp is not None and getattr(mod, "weight", None) is not None:
                n += int(wp.sync(mod._ll_lib, mod.weight.detach(), _versions(mod.weight)))
        # the packed copies of the fused layers are made from the concatenated copies refreshed above
        for mod in model.modules():
            st = mod.__dict__.get("_ll_fused")
            if st is not None and st.p64 is not None:
                n += int(st.packed64(sync=True))
            if st is not None and st.pq is not None:
                n += int(st.sync_wq())
    return n


def drop_weight_copies(model: nn.Module) -> None:
    """Forget the concatenated / converted weight copies (restore_* paths): the next install rebuilds them."""
    for mod in model.modules():
        for k in ("_ll_gate_up", "_ll_gate_up_key", "_ll_bias_f32", "_ll_bias_key", "_ll_qkv", "_ll_w64", "_ll_router_gate", "_ll_router_gate_key"):
            mod.__dict__.pop(k, None)


def restore_linears(model: nn.Module) -> None:
    for mod in model.modules():
        if type(mod) is nn.Linear and "forward" in mod.__dict__:
            del mod.__dict__["forward"]


# ------------------------------------------------------------------------------------------ fused elementwise ops
def _decode_shaped(x: torch.Tensor, width: int, max_rows: int = MAX_ROWS) -> bool:
    return (x.is_cuda and x.dtype == torch.bfloat16 and not torch.is_grad_enabled() and x.shape[-1] == width
            and x.numel() // width <= max_rows)


def _rmsnorm_forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
    H = self.weight.shape[0]
    if _decode_shaped(hidden_states, H, MAX_EW_ROWS) and self.weight.dtype == torch.bfloat16 and H % 8 == 0 and H <= 8192:
        x = hidden_states.reshape(-1, H)
        if not x.is_contiguous():
            x = x.contiguous()
        out = torch.empty_like(x)
        rc = self._ll_lib.ll_rmsnorm_bf16(x.data_ptr(), self.weight.data_ptr(), out.data_ptr(), x.shape[0], H,
                                          float(self.variance_epsilon), torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _lib.check(rc, "ll_rmsnorm_bf16")
        return out.reshape(hidden_states.shape)
    return self._ll_orig_forward(hidden_states)


def _prefill_splits(M: int, N: int, K: int) -> int:
    """65..128 token rows x a matrix of at most ~6 k output rows (q|k|v, o_proj, down_proj of a 7-8 B model at prefill): 64 x 64 output tiles
    number fewer than half the CUs' worth of workgroups, so K is split in two f32 slabs + a slab sum (tools/prefill_splitk_sweep.py, 128 rows:
    down_proj 76.7 -> 51.7 us, o_proj 18.4 -> 15.1, q|k|v 20.3 -> 18.7 incl. the sum; gate|up with its 296+ tiles loses: one piece)."""
    if PREFILL_SPLITK and 64 < M <= MAX_ROWS and K % 128 == 0 and K >= 2048 and 2 * ((N + 63) // 64) < 200:
        return 2
    return 1


def _gemv(lib, x2: torch.Tensor, w: torch.Tensor, bias, N: int) -> torch.Tensor:
    M, K = x2.shape
    out = torch.empty(M, N, dtype=torch.bfloat16, device=x2.device)
    splits = _prefill_splits(M, N, K)
    if splits > 1:
        ws = torch.empty(splits * M * N, dtype=torch.float32, device=x2.device)
        rc = lib.ll_linear_splitk_bf16(x2.data_ptr(), K, w.data_ptr(), K, bias.data_ptr() if bias is not None else None, out.data_ptr(), N, M, N, K,
                                       0, splits, ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _lib.check(rc, "ll_linear_splitk_bf16")
        return out
    rc = lib.ll_linear(_lib.LL_BF16, x2.data_ptr(), K, w.data_ptr(), K, bias.data_ptr() if bias is not None else None,
                       out.data_ptr(), N, M, N, K, 0, 0, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        _lib.check(rc, "ll_linear")
    return out


def _mlp_forward(self, x: torch.Tensor) -> torch.Tensor:
    K, I = self.gate_proj.in_features, self.gate_proj.out_features
    if (_decode_shaped(x, K) and I % 8 == 0 and self.gate_proj.weight.dtype == torch.bfloat16 and self.gate_proj.bias is None
            and self.up_proj.bias is None):
        w = getattr(self, "_ll_gate_up", None)
        if w is None:   # gate and up share the input: one [2I, K] weight, one weight-streaming launch
            w = torch.cat([self.gate_proj.weight.detach(), self.up_proj.weight.detach()], dim=0).contiguous()
            self._ll_gate_up, self._ll_gate_up_key = w, _versions(self.gate_proj.weight, self.up_proj.weight)
        x2 = x.reshape(-1, K)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        gu = _gemv(self._ll_lib, x2, w, None, 2 * I)
        h = torch.empty(x2.shape[0], I, dtype=torch.bfloat16, device=x.device)
        rc = self._ll_lib.ll_silu_mul_bf16(gu.data_ptr(), gu.data_ptr() + 2 * I, h.data_ptr(), x2.shape[0], I, 2 * I,
                                           torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _lib.check(rc, "ll_silu_mul_bf16")
        return self.down_proj(h.reshape(*x.shape[:-1], I))
    if (_decode_shaped(x, K, MAX_EW_ROWS) and I % 8 == 0 and self.gate_proj.weight.dtype == torch.bfloat16):
        # prefill-sized call: BLAS projections, act_fn(gate) * up as one launch
        g, u = self.gate_proj(x), self.up_proj(x)
        g2, u2 = g.reshape(-1, I), u.reshape(-1, I)
        if g2.is_contiguous() and u2.is_contiguous():
            h = torch.empty_like(g2)
            rc = self._ll_lib.ll_silu_mul_bf16(g2.data_ptr(), u2.data_ptr(), h.data_ptr(), g2.shape[0], I, I,
                                               torch.cuda.current_stream().cuda_stream)
            if rc != 0:
                _lib.check(rc, "ll_silu_mul_bf16")
            return self.down_proj(h.reshape(g.shape))
        return self.down_proj(self.act_fn(g) * u)
    return self._ll_orig_forward(x)


class _QKVGroup:
    """q_proj / k_proj / v_proj of one attention block share their input: the q_proj call runs ONE fused GEMV over the
    concatenated [q|k|v] weight and the k_proj / v_proj calls that follow on the same tensor return views of its result."""

    def __init__(self, lib, q, k, v):
        self.lib = lib
        self.nq, self.nk, self.nv = q.out_features, k.out_features, v.out_features
        self.K = q.in_features
        self.w = torch.cat([q.weight.detach(), k.weight.detach(), v.weight.detach()], dim=0).contiguous()
        biases = [m.bias for m in (q, k, v)]
        self.bias = None
        if any(b is not None for b in biases):
            self.bias = torch.cat([(b.detach().float() if b is not None else torch.zeros(m.out_features, device=q.weight.device))
                                   for b, m in zip(biases, (q, k, v))]).contiguous()
        self.x = None
        self.buf = None
        self.key = _versions(q.weight, k.weight, v.weight, q.bias, k.bias, v.bias)

    def run(self, x):
        x2 = x.reshape(-1, self.K)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        self.buf = _gemv(self.lib, x2, self.w, self.bias, self.nq + self.nk + self.nv)
        self.x = x

    def part(self, x, lo, n):
        return self.buf[:, lo:lo + n].reshape(*x.shape[:-1], n) if x.dim() == 2 else self.buf.view(*x.shape[:-1], -1)[..., lo:lo + n]


def _q_forward(self, x):
    g = self._ll_qkv
    if _decode_shaped(x, g.K):
        g.run(x)
        return g.part(x, 0, g.nq)
    g.x = None
    return self._ll_orig_forward(x)


def _k_forward(self, x):
    g = self._ll_qkv
    if g.x is x and g.buf is not None:
        return g.part(x, g.nq, g.nk)
    return self._ll_orig_forward(x)


def _v_forward(self, x):
    g = self._ll_qkv
    if g.x is x and g.buf is not None:
        out = g.part(x, g.nq + g.nk, g.nv)
        g.x = None          # one use per attention call
        return out
    return self._ll_orig_forward(x)


def fuse_qkv(model: nn.Module) -> int:
    """Fuse the q/k/v projections of every attention block (modules with q_proj, k_proj, v_proj Linears) for decode-shaped
    calls.  Call after accelerate_linears (the non-decode path keeps whatever forward the Linears had)."""
    lib = _lib.load()
    n = 0
    for mod in model.modules():
        if all(type(getattr(mod, a, None)) is nn.Linear for a in ("q_proj", "k_proj", "v_proj")):
            q, k, v = mod.q_proj, mod.k_proj, mod.v_proj
            if q.weight.dtype != torch.bfloat16 or not q.weight.is_cuda or hasattr(q, "_ll_qkv"):
                continue
            grp = _QKVGroup(lib, q, k, v)
            for m, f in ((q, _q_forward), (k, _k_forward), (v, _v_forward)):
                m._ll_qkv = grp
                m._ll_orig_forward = m.forward
                m.forward = types.MethodType(f, m)
            n += 1
    return n


def _make_rope(orig, lib):
    import ctypes as C
    I64x3 = C.c_int64 * 3

    def apply_rotary_pos_emb(q, k, cos, sin, unsqueeze_dim=1, **kw):
        if (unsqueeze_dim == 1 and q.dim() == 4 and q.is_cuda and q.dtype == torch.bfloat16 and k.dtype == torch.bfloat16
                and cos.dtype == torch.bfloat16 and cos.dim() == 3 and not torch.is_grad_enabled() and q.shape[2] <= MAX_EW_ROWS
                and q.stride(3) == 1 and k.stride(3) == 1 and cos.stride(2) == 1 and sin.stride() == cos.stride()
                and q.shape[3] % 2 == 0 and q.shape[3] <= 128 and cos.shape[-1] == q.shape[3]):
            B, nh, S, D = q.shape
            nkv = k.shape[1]
            qo = torch.empty((B, nh, S, D), dtype=q.dtype, device=q.device)
            ko = torch.empty((B, nkv, S, D), dtype=k.dtype, device=k.device)
            cs0 = 0 if cos.shape[0] == 1 else cos.stride(0)
            rc = lib.ll_rope_bf16(q.data_ptr(), k.data_ptr(), cos.data_ptr(), sin.data_ptr(), qo.data_ptr(), ko.data_ptr(),
                                  B, nh, nkv, S, D, I64x3(q.stride(0), q.stride(1), q.stride(2)),
                                  I64x3(k.stride(0), k.stride(1), k.stride(2)), I64x3(cs0, cos.stride(1), 1),
                                  torch.cuda.current_stream().cuda_stream)
            if rc != 0:
                _lib.check(rc, "ll_rope_bf16")
            return qo, ko
        return orig(q, k, cos, sin, unsqueeze_dim=unsqueeze_dim, **kw)

    apply_rotary_pos_emb._ll_orig = orig
    return apply_rotary_pos_emb


def _is_silu(fn) -> bool:
    return fn is F.silu or type(fn).__name__ in ("SiLU", "SiLUActivation")


def accelerate_elementwise(model: nn.Module) -> dict:
    """Fuse the decode-step RMSNorm / rotary embedding / SiLU*mul of a Llama-family HF model into single launches
    (ll_rmsnorm_bf16, ll_rope_bf16, ll_silu_mul_bf16).  Non-decode shapes keep the original HF code path."""
    import sys
    lib = _lib.load()
    n_norm = n_mlp = 0
    n_qkv = fuse_qkv(model)
    for mod in model.modules():
        cls = type(mod).__name__
        if cls.endswith("RMSNorm") and hasattr(mod, "variance_epsilon") and hasattr(mod, "weight") and "forward" not in mod.__dict__:
            mod._ll_lib, mod._ll_orig_forward = lib, mod.forward
            mod.forward = types.MethodType(_rmsnorm_forward, mod)
            n_norm += 1
        elif (all(hasattr(mod, a) for a in ("gate_proj", "up_proj", "down_proj", "act_fn")) and _is_silu(mod.act_fn)
              and "forward" not in mod.__dict__):
            mod._ll_lib, mod._ll_orig_forward = lib, mod.forward
            mod.forward = types.MethodType(_mlp_forward, mod)
            n_mlp += 1
    rope = 0
    base = getattr(model, "model", model)
    m = sys.modules.get(type(base).__module__)
    if m is not None and hasattr(m, "apply_rotary_pos_emb") and not hasattr(m.apply_rotary_pos_emb, "_ll_orig"):
        m.apply_rotary_pos_emb = _make_rope(m.apply_rotary_pos_emb, lib)
        rope = 1
    return {"rmsnorm": n_norm, "mlp": n_mlp, "rope": rope, "qkv": n_qkv}


def restore_elementwise(model: nn.Module) -> None:
    import sys
    for mod in model.modules():
        if "_ll_orig_forward" in mod.__dict__ and "forward" in mod.__dict__:
            del mod.__dict__["forward"]
            del mod.__dict__["_ll_orig_forward"]
    drop_weight_copies(model)            # a later install rebuilds them from the then-current weights
    base = getattr(model, "model", model)
    m = sys.modules.get(type(base).__module__)
    if m is not None and hasattr(getattr(m, "apply_rotary_pos_emb", None), "_ll_orig"):
        m.apply_rotary_pos_emb = m.apply_rotary_pos_emb._ll_orig


# ------------------------------------------------------------------------------------------ decode attention + KV append
ATTN_NAME = "llamole_decode"


def _decode_attention_forward(module, query, key, value, attention_mask, dropout=0.0, scaling=None, **kwargs):
    """AttentionInterface entry: softmax(q K^T * scaling + mask) V with grouped-query heads straight from the static cache
    (no repeat_kv copies); anything that is not a small bf16 decode call with a boolean mask goes to HF's sdpa path."""
    import ctypes as C
    from transformers.integrations.sdpa_attention import sdpa_attention_forward
    B, nh, S, D = query.shape
    if (query.is_cuda and query.dtype == torch.bfloat16 and key.dtype == torch.bfloat16 and S <= MAX_APPEND_ROWS and D in (64, 128)
            and attention_mask is not None and attention_mask.dtype == torch.bool and attention_mask.dim() == 4
            and attention_mask.shape[1] == 1 and attention_mask.shape[-1] == key.shape[2] and attention_mask.stride(3) == 1
            and key.is_contiguous() and value.is_contiguous() and query.stride(3) == 1 and dropout == 0.0
            and not torch.is_grad_enabled() and nh % key.shape[1] == 0 and key.shape[2] <= ATTN_MAXLEN):
        nkv, maxlen = key.shape[1], key.shape[2]
        out = torch.empty((B, S, nh, D), dtype=query.dtype, device=query.device)
        scale = float(scaling) if scaling is not None else D ** -0.5
        I64x3, I64x2 = C.c_int64 * 3, C.c_int64 * 2
        rc = _lib.load().ll_decode_attn_bf16(query.data_ptr(), key.data_ptr(), value.data_ptr(), attention_mask.data_ptr(),
                                             out.data_ptr(), B, nh, nkv, S, maxlen, D, scale,
                                             I64x3(query.stride(0), query.stride(1), query.stride(2)),
                                             I64x2(attention_mask.stride(0), attention_mask.stride(2)),
                                             torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _lib.check(rc, "ll_decode_attn_bf16")
        return out, None
    return sdpa_attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling, **kwargs)


def use_decode_attention(model: nn.Module) -> bool:
    """Register the fused decode attention with transformers' AttentionInterface (boolean sdpa-style masks) and select it
    on ``model``.  Returns False (and changes nothing) if this transformers build has no such registry."""
    try:
        from transformers import AttentionInterface
        from transformers.masking_utils import AttentionMaskInterface, sdpa_mask
    except ImportError:
        return False
    AttentionInterface.register(ATTN_NAME, _decode_attention_forward)
    AttentionMaskInterface.register(ATTN_NAME, sdpa_mask)
    model.config._attn_implementation = ATTN_NAME
    for mod in model.modules():
        cfg = getattr(mod, "config", None)
        if cfg is not None and hasattr(cfg, "_attn_implementation"):
            cfg._attn_implementation = ATTN_NAME
    return True


def fuse_cache_update(cache) -> int:
    """Replace StaticLayer.update of an (already initialised) StaticCache by one fused append launch per layer for decode-
    shaped calls.  All layers write at the position held by layer 0's on-device counter; the caller advances that counter
    once per forward (GraphedDecoder does).  Returns the number of patched layers."""
    import ctypes as C
    lib = _lib.load()
    layers = list(cache.layers)
    if not layers or not all(getattr(l, "is_initialized", False) and hasattr(l, "cumulative_length") for l in layers):
        return 0
    pos = layers[0].cumulative_length
    I64x3 = C.c_int64 * 3

    def make(layer):
        orig = layer.update

        def update(key_states, value_states, *a, **k):
            S = key_states.shape[-2]
            if (S <= MAX_APPEND_ROWS and key_states.dtype == torch.bfloat16 and layer.keys.dtype == torch.bfloat16 and key_states.is_cuda
                    and key_states.stride(3) == 1 and value_states.stride(3) == 1 and not torch.is_grad_enabled()):
                B, nkv, _, D = key_states.shape
                rc = lib.ll_kv_append_bf16(layer.keys.data_ptr(), layer.values.data_ptr(), key_states.data_ptr(),
                                           value_states.data_ptr(), pos.data_ptr(), B, nkv, S, layer.keys.shape[2], D,
                                           I64x3(key_states.stride(0), key_states.stride(1), key_states.stride(2)),
                                           I64x3(value_states.stride(0), value_states.stride(1), value_states.stride(2)),
                                           torch.cuda.current_stream().cuda_stream)
                if rc != 0:
                    _lib.check(rc, "ll_kv_append_bf16")
                return layer.keys, layer.values
            return orig(key_states, value_states, *a, **k)

        layer.update = update
        layer._ll_fused_update = True

    for l in layers:
        if not getattr(l, "_ll_fused_update", False):
            make(l)
    return len(layers)


def _is_kv8(cl) -> bool:
    """Whether a cache layer holds MX8 codes (kv_cache.MX8StaticLayer: uint8 ``keys`` / ``values`` with ``key_scales`` / ``value_scales``)."""
    keys = getattr(cl, "keys", None)
    return keys is not None and keys.dtype == torch.uint8 and hasattr(cl, "key_scales")


def _kv_layer_ok(cl) -> bool:
    """A cache layer the fused attention entries take: contiguous bf16 K / V, or the four contiguous tensors of an MX8 layer."""
    if not (cl.keys.is_contiguous() and cl.values.is_contiguous()):
        return False
    if _is_kv8(cl):
        return cl.key_scales.is_contiguous() and cl.value_scales.is_contiguous()
    return cl.keys.dtype == torch.bfloat16


# ------------------------------------------------------------------------------------------ Granite layout: scalar multipliers
def hf_scaled_residual(residual: torch.Tensor, y: torch.Tensor, m: float) -> torch.Tensor:
    """GraniteDecoderLayer.forward's ``residual + hidden_states * self.residual_multiplier`` stated in torch as the kernels compute it (the
    LL_GEMV_RESIDUAL_SCALED contract of include/llamole_hip.h): y is the Linear's bf16 output, the product is taken in f32 with the multiplier
    rounded to f32 and rounded to bf16, then the sum is.  On bf16 tensors this is bit for bit what HF's line gives."""
    m32 = torch.tensor(float(m), dtype=torch.float32, device=y.device)
    scaled = (y.to(torch.bfloat16).float() * m32).to(torch.bfloat16)
    return (residual.to(torch.bfloat16).float() + scaled.float()).to(torch.bfloat16)


def hf_scaled_embedding(table: torch.Tensor, ids: torch.Tensor, m: float) -> torch.Tensor:
    """GraniteModel.forward's ``embed_tokens(input_ids) * self.embedding_multiplier`` as ll_embed_rows_bf16 computes it: f32 product with
    the multiplier rounded to f32, one rounding to bf16."""
    m32 = torch.tensor(float(m), dtype=torch.float32, device=table.device)
    return (table[ids].float() * m32).to(torch.bfloat16)


def _multiplier(owner, name: str):
    """(value as a float or None when it is not a number, whether it is a finite non-zero number) of a scalar multiplier attribute; an
    absent attribute is 1.0."""
    import math
    v = getattr(owner, name, 1.0)
    try:
        f = float(v)
    except (TypeError, ValueError):
        return None, False
    return f, (math.isfinite(f) and f != 0.0 and abs(f) <= 3.0e38 and float(torch.tensor(f, dtype=torch.float32)) != 0.0)


RESIDUAL_MULTIPLIER_DECLINED = "residual_multiplier is not a finite non-zero number"
MOE_RESIDUAL_MULTIPLIER_DECLINED = "MoE layer with a residual_multiplier (the slot-sum launch has no scaled residual)"
EMBEDDING_MULTIPLIER_DECLINED = "embedding_multiplier is not a finite non-zero number"
EMBEDDING_TABLE_DECLINED = "embedding_multiplier with an embedding table that is not a contiguous bf16 matrix of a width that is a multiple of 8"
WQ_RESIDUAL_MULTIPLIER_REASON = ("residual_multiplier: the packed-code kernels have no scaled residual epilogue; these layers run the bf16 "
                                 "kernels on their dequantised weights")


# ------------------------------------------------------------------------------------------ whole decoder layer = 5 launches
class _FusedLayer:
    """Decode-step state of one HF decoder layer (Qwen2 / Llama / Mistral layout): concatenated q|k|v and gate|up weights
    (shared with fuse_qkv / the MLP fusion when those ran first), f32 biases, norm weights.  ``run`` is
    Qwen2DecoderLayer.forward (transformers modeling_qwen2.py) for ONE new token per sequence:
      qkv  = gemv(rmsnorm(h), Wqkv) ; a = rope+append+attention(qkv) ; h = h + gemv(a, Wo)
      act  = silu(gate)*up of gemv(rmsnorm(h), Wgate|up) ; h = h + gemv(act, Wdown)
    five launches: batch <= 2 (<= 4 when the sizes are not multiples of 32) on the FMA GEMVs (ll_gemv_fused_bf16), batch 3..16 on
    the weight-streaming MFMA Linear (ll_linear_rows16_bf16) -- both with the RMSNorm as prologue and the residual / SiLU*mul
    epilogues."""

    def __init__(self, lib, layer, split_ws: Optional[dict] = None):
        att = layer.self_attn
        self.lib = lib
        self._split_ws = split_ws if split_ws is not None else {}      # the model's key-split attention workspaces (_AttnSplitWorkspace), by shape
        self._split_ok = {}                                             # (B, S, maxlen) -> whether the key-split entry takes the shape
        self.layer_idx = att.layer_idx
        q, k, v, o = att.q_proj, att.k_proj, att.v_proj, att.o_proj
        grp = getattr(q, "_ll_qkv", None) or _QKVGroup(lib, q, k, v)
        self.wqkv, self.bqkv = grp.w, grp.bias
        self.nq, self.nkv_dim = q.out_features, k.out_features
        self.D = att.head_dim
        self.nh, self.nkv = self.nq // self.D, self.nkv_dim // self.D
        self.H = q.in_features
        self.scaling = float(att.scaling)
        # a sliding-window layer (Mistral-v0.1, Qwen2 / Qwen3 layer_types): key j is seen from slot p iff j > p - window, applied inside the
        # windowed key-split entries (ll_*_attn_rope_win_bf16) wherever the window can bind (``_windowed``); None = full attention
        self.window = attn_window(att)
        # Granite layout: both residual adds are residual + y * residual_multiplier; None = the plain residual epilogue (absent or 1.0)
        rm = _multiplier(layer, "residual_multiplier")[0]
        self.rscale = None if rm == 1.0 else rm
        # Qwen3 layout: an RMSNorm over head_dim on every q and k head row in front of the rotation, done inside the attention launch; the
        # modules stay the owners of the weights (read at every call: no copy to keep in step)
        self.qn, self.kn = getattr(att, "q_norm", None), getattr(att, "k_norm", None)
        self.qk_eps = float(self.qn.variance_epsilon) if self.qn is not None else 0.0
        self.wo = o.weight.detach()
        self.bo = o.bias.detach().float().contiguous() if o.bias is not None else None
        self.bo_key = _versions(o.bias)
        self.n1, self.n2 = layer.input_layernorm, layer.post_attention_layernorm
        self.eps1, self.eps2 = float(self.n1.variance_epsilon), float(self.n2.variance_epsilon)
        self._init_mlp(layer, (q, k, v, o))
        self.p64 = None         # packed copies of the matrices for 17..64 rows (made at the first such step)
        # quantization_bit: the MX codes of [q|k|v], o_proj, [gate|up], down_proj (made from the rounded bf16 matrices, which stay: they serve the
        # prefill and 17..64 rows); None = the layer runs on bf16 weights (not quantised, or a K that is not a multiple of 32)
        bits = {m.__dict__.get("_ll_wq_bits") for m in self._mods}
        self.wq_bits = bits.pop() if len(bits) == 1 else None
        self.pq = None
        self.use_wq = True      # off: the bf16 kernels on the dequantised weights (tests, A/B timing)
        # (a layer with a residual_multiplier keeps no codes: the packed-code kernels have no scaled residual epilogue)
        if self.wq_bits is not None and self.stream_ok and self.wq_ok and self.rscale is None:
            self.pq = tuple(_PackedWQ(lib, w, self.wq_bits, key) for w, key in zip(self._srcs(), self._keys64()))

    def _init_mlp(self, layer, attn_mods):
        """The dense gated MLP: the concatenated gate|up copy and down_proj."""
        mlp = layer.mlp
        wgu = getattr(mlp, "_ll_gate_up", None)
        if wgu is None:
            wgu = torch.cat([mlp.gate_proj.weight.detach(), mlp.up_proj.weight.detach()], dim=0).contiguous()
            mlp._ll_gate_up, mlp._ll_gate_up_key = wgu, _versions(mlp.gate_proj.weight, mlp.up_proj.weight)
        self.wgu = wgu
        self.I = mlp.gate_proj.out_features
        self.wdown = mlp.down_proj.weight.detach()
        self.stream_ok = self.H % 32 == 0 and self.nq % 32 == 0 and self.I % 32 == 0 and self.n1.weight.dtype == torch.bfloat16
        self.wq_ok = self.I % 32 == 0
        self._mods = attn_mods + (mlp.gate_proj, mlp.up_proj, mlp.down_proj)

    def _srcs(self):
        """The matrices that get packed copies (rows64 order, MX codes), in the order of ``_keys64``."""
        return (self.wqkv, self.wo, self.wgu, self.wdown)

    def sync_wq(self) -> int:
        return sum(p.sync(self.lib, w, key) for p, w, key in zip(self.pq, self._srcs(), self._keys64()))

    def _keys64(self):
        q, k, v, o, g, u, d = self._mods
        return (_versions(q.weight, k.weight, v.weight), _versions(o.weight), _versions(g.weight, u.weight), _versions(d.weight))

    def _packed64_sources(self):
        """(matrices, keys) of the rows64 copies: the matrices of ``_srcs`` (a layer with a shared expert adds that expert's, which get no MX codes)."""
        return self._srcs(), self._keys64()

    def packed64(self, sync: bool = False):
        """[q|k|v], o_proj, [gate|up], down_proj in MFMA operand order (ll_rows64_pack_bf16) -- one more copy of the layer's weights,
        made the first time 17..64 sequences are decoded together; ``sync`` re-packs in place what changed at the source."""
        srcs, keys = self._packed64_sources()
        if self.p64 is None:
            self.p64 = tuple(_Packed64(self.lib, w, key) for w, key in zip(srcs, keys))
        elif sync:
            return sum(p.sync(self.lib, w, key) for p, w, key in zip(self.p64, srcs, keys))
        return 0

    def eligible(self, h, mask, cache, pe) -> bool:
        if not (h.is_cuda and h.dtype == torch.bfloat16 and h.dim() == 3 and h.shape[1] == 1
                and (h.shape[0] <= 4 or (h.shape[0] <= MAX_STREAM_ROWS and self.stream_ok))
                and not torch.is_grad_enabled() and cache is not None and pe is not None and mask is not None):
            return False
        layers = getattr(cache, "layers", None)
        if layers is None or self.layer_idx >= len(layers):
            return False
        cl = layers[self.layer_idx]
        if not (getattr(cl, "_ll_fused_update", False) and _kv_layer_ok(cl)):
            return False
        if not self.attn_serves(h.shape[0], 1, cl.keys.shape[2], _is_kv8(cl)):
            return False
        cos = pe[0]
        return (mask.dtype == torch.bool and mask.dim() == 4 and mask.shape[1] == 1 and mask.shape[2] == 1
                and mask.shape[3] == cl.keys.shape[2] and mask.stride(3) == 1 and cos.dtype == torch.bfloat16
                and cos.dim() == 3 and cos.shape[1] == 1 and cos.shape[2] == self.D and cos.stride(2) == 1
                and pe[1].stride() == cos.stride() and h.is_contiguous())

    def _gemv_wq(self, x, pk, bias, norm_w, eps, res, N, K, epi):
        """1..16 token rows on the packed MX codes ``pk``: the f32-FMA GEMV up to FMA_GEMV_ROWS rows, the MFMA weight stream beyond."""
        M = x.shape[0]
        out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
        name = "ll_linear_rows16_wq" if M > FMA_GEMV_ROWS else "ll_gemv_fused_wq"
        rc = getattr(self.lib, name)(x.data_ptr(), x.stride(0), pk.t.data_ptr(), pk.bits, bias.data_ptr() if bias is not None else None,
                                     norm_w.data_ptr() if norm_w is not None else None, eps,
                                     res.data_ptr() if res is not None else None, res.stride(0) if res is not None else 0,
                                     out.data_ptr(), N, M, N, K, epi, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _lib.check(rc, name)
        return out

    def _gemv_rs(self, x, w, bias, res, N, K):
        """o_proj / down_proj + the scaled residual add of a Granite layer on 1..16 rows: the ``_gemv`` choice of kernel, the *_rs entries."""
        M = x.shape[0]
        out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
        name = "ll_linear_rows16_rs_bf16" if M > FMA_GEMV_ROWS and self.stream_ok else "ll_gemv_fused_rs_bf16"
        rc = getattr(self.lib, name)(x.data_ptr(), x.stride(0), w.data_ptr(), K, bias.data_ptr() if bias is not None else None, res.data_ptr(),
                                     res.stride(0), out.data_ptr(), N, M, N, K, self.rscale, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _lib.check(rc, name)
        return out

    def _gemv(self, x, w, bias, norm_w, eps, res, N, K, epi, pk=None, which=None):
        M = x.shape[0]
        if epi == 1 and self.rscale is not None:
            return self._gemv_rs(x, w, bias, res, N, K)
        if pk is not None and self.use_wq and FMA_GEMV_ROWS == 2 and M in WQ_ROUTES.get((pk.bits, which), ()):
            return self._gemv_wq(x, pk, bias, norm_w, eps, res, N, K, epi)
        out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
        if M > FMA_GEMV_ROWS and self.stream_ok:
            rc = self.lib.ll_linear_rows16_bf16(x.data_ptr(), x.stride(0), w.data_ptr(), K, bias.data_ptr() if bias is not None else None,
                                                norm_w.data_ptr() if norm_w is not None else None, eps,
                                                res.data_ptr() if res is not None else None, res.stride(0) if res is not None else 0,
                                                out.data_ptr(), N, M, N, K, epi, torch.cuda.current_stream().cuda_stream)
            if rc != 0:
                _lib.check(rc, "ll_linear_rows16_bf16")
            return out
        rc = self.lib.ll_gemv_fused_bf16(x.data_ptr(), x.stride(0), w.data_ptr(), K, bias.data_ptr() if bias is not None else None,
                                         norm_w.data_ptr() if norm_w is not None else None, eps,
                                         res.data_ptr() if res is not None else None, res.stride(0) if res is not None else 0,
                                         out.data_ptr(), N, M, N, K, epi, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _lib.check(rc, "ll_gemv_fused_bf16")
        return out

    def _windowed(self, maxlen: int) -> bool:
        """Whether the window can bind on a static cache of ``maxlen`` slots: then the windowed entries run, at every cache length.  With
        ``window >= maxlen`` every slot a causal mask shows lies inside the window and the layer takes exactly a full-attention layer's calls."""
        return self.window is not None and self.window < maxlen

    def attn_serves(self, B: int, S: int, maxlen: int, kv8: bool = False) -> bool:
        """Whether this layer's attention entry points take a static cache of ``maxlen`` slots for B sequences of S new positions: up to
        ATTN_MAXLEN the one-workgroup kernels, beyond it whatever the key-split entry accepts (its own answer, asked once per shape).  An MX8
        cache (``kv8``) has the key-split entries only, at every length, with the same bounds; so has a sliding-window layer whose window can
        bind (the windowed entries; there are none for an MX8 cache)."""
        win = self._windowed(maxlen)
        if win and kv8:         # (kv_cache.MX8StaticCache refuses a config with sliding layers, so no such cache comes from GraphedDecoder)
            return False
        if maxlen <= ATTN_MAXLEN and not kv8 and not win:
            return True
        key = (B, S, maxlen)
        if key not in self._split_ok:
            n = (self.lib.ll_attn_win_workspace_bytes(B, S, self.nh, self.nkv, maxlen, self.D, self.window) if win else
                 self.lib.ll_attn_split_workspace_bytes(B, S, self.nh, self.nkv, maxlen, self.D))
            self._split_ok[key] = int(n) >= 0 and (S > 1 or B <= MAX_STREAM_ROWS)
        return self._split_ok[key]

    def _split_workspace(self, B: int, S: int, maxlen: int, device):
        """The model's workspace of the key-split attention for this shape: allocated at the first call (the eager step that precedes a capture),
        shared by the layers, which run one after the other on one stream; a captured graph holds its fixed address."""
        window = self.window if self._windowed(maxlen) else None
        key = (B, S, self.nh, self.nkv, maxlen, self.D, str(device), window)
        ws = self._split_ws.get(key)
        if ws is None:
            ws = self._split_ws[key] = _AttnSplitWorkspace(self.lib, device, B, S, self.nh, self.nkv, maxlen, self.D, window)
        return ws

    def _split_tail(self, B: int, S: int, maxlen: int, device):
        """The arguments the key-split entries take behind those of the *_qkn entries: norm weights (or NULL), eps, workspace, its size, stream."""
        ws = self._split_workspace(B, S, maxlen, device)
        qn = self.qn.weight.data_ptr() if self.qn is not None else None
        kn = self.kn.weight.data_ptr() if self.kn is not None else None
        win = (self.window,) if self._windowed(maxlen) else ()      # the windowed entries take the window in front of the workspace
        return (qn, kn, self.qk_eps, *win, ws.t.data_ptr(), ws.bytes, torch.cuda.current_stream().cuda_stream)

    def _attn(self, qkv, nqkv, mask, cache, pe, B, device):
        cl = cache.layers[self.layer_idx]
        pos = cache.layers[0].cumulative_length
        cos, sin = pe
        att = torch.empty(B, self.nq, dtype=torch.bfloat16, device=device)
        args = (qkv.data_ptr(), nqkv, cos.data_ptr(), sin.data_ptr(), 0 if cos.shape[0] == 1 else cos.stride(0), cl.keys.data_ptr(),
                cl.values.data_ptr(), pos.data_ptr(), mask.data_ptr(), mask.stride(0), att.data_ptr(), B, self.nh, self.nkv,
                cl.keys.shape[2], self.D, self.scaling)
        if _is_kv8(cl):                           # an MX8 cache: the key-split attention on codes and scales, at every length
            name = "ll_decode_attn_rope_kv8"
            rc = self.lib.ll_decode_attn_rope_kv8(*args[:5], cl.keys.data_ptr(), cl.key_scales.data_ptr(), cl.values.data_ptr(),
                                                  cl.value_scales.data_ptr(), *args[7:], *self._split_tail(B, 1, cl.keys.shape[2], device))
        elif self._windowed(cl.keys.shape[2]):    # a window that can bind: only the ranges of 512 keys it can reach, at every cache length
            name = "ll_decode_attn_rope_win_bf16"
            rc = self.lib.ll_decode_attn_rope_win_bf16(*args, *self._split_tail(B, 1, cl.keys.shape[2], device))
        elif cl.keys.shape[2] > ATTN_MAXLEN:      # beyond the one-workgroup kernels: the keys split over workgroups, two launches
            name = "ll_decode_attn_rope_split_bf16"
            rc = self.lib.ll_decode_attn_rope_split_bf16(*args, *self._split_tail(B, 1, cl.keys.shape[2], device))
        elif self.qn is not None:
            name = "ll_decode_attn_rope_qkn_bf16"
            rc = self.lib.ll_decode_attn_rope_qkn_bf16(*args, self.qn.weight.data_ptr(), self.kn.weight.data_ptr(), self.qk_eps,
                                                       torch.cuda.current_stream().cuda_stream)
        else:
            name = "ll_decode_attn_rope_bf16"
            rc = self.lib.ll_decode_attn_rope_bf16(*args, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _lib.check(rc, name)
        return att

    def run64(self, h, mask, cache, pe, pre=None, next_norm=None):
        """17..64 sequences: seven launches on the packed weights -- q|k|v (row scale in its epilogue), rope + append + attention, o_proj
        (K split into f32 slabs), slab sum + residual + the post-attention pre-norm, gate|up (row scale) + SiLU*mul, down_proj (K
        split), slab sum + residual + the NEXT layer's input pre-norm.  A "pre-norm" is the pair (bf16(h * w_norm), per-chunk sums of
        h^2): the RMSNorm is finished by the consuming Linear's epilogue.  ``pre`` = that pair for this layer's input when the previous
        layer already produced it; returns (h_out, pre_next or None)."""
        B, H = h.shape[0], self.H
        x = h.view(B, H)
        self.packed64()
        pqkv, po, pgu, pdown = self.p64
        xs, ssq = pre if pre is not None else _prenorm64(self.lib, x, self.n1.weight)
        nqkv = self.nq + 2 * self.nkv_dim
        qkv = _rows64(self.lib, xs, xs.stride(0), pqkv, self.bqkv, None, nqkv, 0, row_ssq=ssq, eps=self.eps1)
        att = self._attn(qkv, nqkv, mask, cache, pe, B, h.device)
        h1, xs2, ssq2 = _rows64(self.lib, att, att.stride(0), po, self.bo, x, H, 1, next_norm=self.n2.weight, rscale=self.rscale)
        act = _rows64(self.lib, xs2, xs2.stride(0), pgu, None, None, self.I, 2, row_ssq=ssq2, eps=self.eps2)
        if next_norm is None:
            return _rows64(self.lib, act, act.stride(0), pdown, None, h1, H, 1, rscale=self.rscale).view(B, 1, H), None
        h2, xs3, ssq3 = _rows64(self.lib, act, act.stride(0), pdown, None, h1, H, 1, next_norm=next_norm, rscale=self.rscale)
        return h2.view(B, 1, H), (xs3, ssq3)

    def run(self, h, mask, cache, pe):
        B, H = h.shape[0], self.H
        if B > MAX_ROWS16:
            return self.run64(h, mask, cache, pe)[0]
        x = h.view(B, H)
        nqkv = self.nq + 2 * self.nkv_dim
        pq = self.pq or (None, None, None, None)
        qkv = self._gemv(x, self.wqkv, self.bqkv, self.n1.weight, self.eps1, None, nqkv, H, 0, pq[0], "qkv")
        att = self._attn(qkv, nqkv, mask, cache, pe, B, h.device)
        h1 = self._gemv(att, self.wo, self.bo, None, 0.0, x, H, self.nq, 1, pq[1], "o")
        return self._mlp(h1, pq).view(B, 1, H)

    def _mlp(self, h1, pq):
        """The MLP half on 1..16 rows of the post-attention residual stream: RMSNorm-prologue gate|up + SiLU*mul, down_proj + residual."""
        act = self._gemv(h1, self.wgu, None, self.n2.weight, self.eps2, None, self.I, self.H, 2, pq[2], "gate_up")
        return self._gemv(act, self.wdown, None, None, 0.0, h1, self.H, self.I, 1, pq[3], "down")


    def run_suffix(self, h, mask, cache, pe, B, S):
        """S consecutive new positions per sequence (B*S <= 16 rows: the query-token forward on the decode's cache): the five launches of
        ``run`` with ll_suffix_attn_rope_bf16 in the middle -- query row s sees the cache up to slot pos + s, the keys of rows 0..s included."""
        H, R = self.H, B * S
        x = h.view(R, H)
        cl = cache.layers[self.layer_idx]
        pos = cache.layers[0].cumulative_length
        cos, sin = pe
        nqkv = self.nq + 2 * self.nkv_dim
        pq = self.pq or (None, None, None, None)
        qkv = self._gemv(x, self.wqkv, self.bqkv, self.n1.weight, self.eps1, None, nqkv, H, 0, pq[0], "qkv")
        att = torch.empty(R, self.nq, dtype=torch.bfloat16, device=h.device)
        args = (qkv.data_ptr(), nqkv, cos.data_ptr(), sin.data_ptr(), cl.keys.data_ptr(), cl.values.data_ptr(), pos.data_ptr(), mask.data_ptr(),
                att.data_ptr(), B, S, self.nh, self.nkv, cl.keys.shape[2], self.D, self.scaling)
        if _is_kv8(cl):
            name = "ll_suffix_attn_rope_kv8"
            rc = self.lib.ll_suffix_attn_rope_kv8(*args[:4], cl.keys.data_ptr(), cl.key_scales.data_ptr(), cl.values.data_ptr(),
                                                  cl.value_scales.data_ptr(), *args[6:], *self._split_tail(B, S, cl.keys.shape[2], h.device))
        elif self._windowed(cl.keys.shape[2]):
            name = "ll_suffix_attn_rope_win_bf16"
            rc = self.lib.ll_suffix_attn_rope_win_bf16(*args, *self._split_tail(B, S, cl.keys.shape[2], h.device))
        elif cl.keys.shape[2] > ATTN_MAXLEN:
            name = "ll_suffix_attn_rope_split_bf16"
            rc = self.lib.ll_suffix_attn_rope_split_bf16(*args, *self._split_tail(B, S, cl.keys.shape[2], h.device))
        elif self.qn is not None:
            name = "ll_suffix_attn_rope_qkn_bf16"
            rc = self.lib.ll_suffix_attn_rope_qkn_bf16(*args, self.qn.weight.data_ptr(), self.kn.weight.data_ptr(), self.qk_eps,
                                                       torch.cuda.current_stream().cuda_stream)
        else:
            name = "ll_suffix_attn_rope_bf16"
            rc = self.lib.ll_suffix_attn_rope_bf16(*args, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _lib.check(rc, name)
        h1 = self._gemv(att, self.wo, self.bo, None, 0.0, x, H, self.nq, 1, pq[1], "o")
        return self._mlp(h1, pq).view(B, S, H)


class _AttnSplitWorkspace:
    """Device scratch of ``ll_decode_attn_rope_split_bf16`` / ``ll_suffix_attn_rope_split_bf16`` (per-range softmax statistics and partial
    outputs) for one shape, or with a ``window`` that of the windowed entries (sized by the ranges a window reaches); one per model and shape,
    allocated once, so a captured graph holds a fixed address."""

    def __init__(self, lib, device, B, S, nh, nkv, maxlen, D, window=None):
        if window is None:
            name, n = "ll_attn_split_workspace_bytes", int(lib.ll_attn_split_workspace_bytes(B, S, nh, nkv, maxlen, D))
        else:
            name, n = "ll_attn_win_workspace_bytes", int(lib.ll_attn_win_workspace_bytes(B, S, nh, nkv, maxlen, D, window))
        if n < 0:
            raise ValueError(f"{name}: unsupported sizes B={B} S={S} nh={nh} nkv={nkv} maxlen={maxlen} D={D} window={window}")
        self.bytes = n
        self.t = torch.empty(n, dtype=torch.uint8, device=device)


class _MoeWorkspace:
    """Device scratch of ``ll_moe_route_bf16`` / ``ll_moe_experts_bf16`` for up to 64 token rows, shared by the MoE layers of one model that have
    the same sizes (they run one after the other on one stream); allocated once, so a captured graph holds a fixed address."""

    def __init__(self, lib, device, E, top_k, H, I):
        n = int(lib.ll_moe_workspace_bytes(MAX_STREAM_ROWS, E, top_k, H, I))
        if n < 0:
            raise ValueError(f"ll_moe_workspace_bytes: unsupported sizes E={E} top_k={top_k} H={H} I={I}")
        self.bytes = n
        self.t = torch.empty(n, dtype=torch.uint8, device=device)


class _FusedMoeLayer(_FusedLayer):
    """``_FusedLayer`` for a decoder layer whose MLP is a sparse mixture-of-experts block (Qwen3MoeSparseMoeBlock): the attention half is the
    parent's; the MLP half is router logits (the dense Linear on mlp.gate.weight with the post-attention RMSNorm as prologue), ll_moe_route_bf16
    and ll_moe_experts_bf16 (gate|up, down, slot sum + residual) -- eight launches per layer at 1..16 rows.  The expert and router parameters
    are read in place: no copy, nothing for ``refresh_weight_copies`` to follow.  ``idx`` / ``w`` keep the routing of the latest call (static
    buffers: a captured graph rewrites them at every replay).
    Mixtral layout (``w_f32``): the routing weights stay f32 (ll_moe_route_f32) and the slot sum applies them (ll_moe_experts_ex_bf16) -- eight
    launches as well.  Qwen2-MoE layout (``shared``): the router Linear runs over a stacked [E + 1, H] copy of gate.weight and
    shared_expert_gate.weight (column E of its output is the shared gate's logit; the copy follows its sources in
    ``refresh_weight_copies``), the shared expert is the dense MLP's gate|up and down launches on its own concatenated copy, and the slot sum
    adds sigmoid(gate) * shared -- ten launches."""

    def __init__(self, lib, layer, workspaces: dict, split_ws: Optional[dict] = None):
        self._workspaces = workspaces
        super().__init__(lib, layer, split_ws)

    def _init_mlp(self, layer, attn_mods):
        mlp = layer.mlp
        self.experts, self.router = mlp.experts, mlp.gate
        self.E, _, self.I = (int(v) for v in mlp.experts.down_proj.shape)
        family = _moe_family(mlp)
        self.w_f32 = family == "mixtral"          # MixtralTopKRouter: f32 weights, always renormalised
        self.top_k, self.norm_topk = int(mlp.gate.top_k), True if self.w_f32 else bool(mlp.gate.norm_topk_prob)
        self.stream_ok = self.H % 32 == 0 and self.nq % 32 == 0 and self.n1.weight.dtype == torch.bfloat16
        self.wq_ok = True
        self._mods = attn_mods
        self.shared = None
        if family == "qwen2":
            sh = self.shared = mlp.shared_expert
            wgu = getattr(sh, "_ll_gate_up", None)
            if wgu is None:
                wgu = torch.cat([sh.gate_proj.weight.detach(), sh.up_proj.weight.detach()], dim=0).contiguous()
                sh._ll_gate_up, sh._ll_gate_up_key = wgu, _versions(sh.gate_proj.weight, sh.up_proj.weight)
            self.wgu_s, self.wdown_s, self.Is = wgu, sh.down_proj.weight.detach(), sh.gate_proj.out_features
            wr = mlp.__dict__.get("_ll_router_gate")
            if wr is None:
                wr = torch.cat([mlp.gate.weight.detach(), mlp.shared_expert_gate.weight.detach()], dim=0).contiguous()
                mlp._ll_router_gate, mlp._ll_router_gate_key = wr, _versions(mlp.gate.weight, mlp.shared_expert_gate.weight)
            self.router_w = wr
            self.stream_ok = self.stream_ok and self.Is % 32 == 0
        dev = mlp.gate.weight.device
        key = (self.E, self.top_k, self.H, self.I, str(dev))
        if key not in self._workspaces:
            self._workspaces[key] = _MoeWorkspace(self.lib, dev, self.E, self.top_k, self.H, self.I)
        self.ws = self._workspaces[key]
        self.idx = torch.zeros(MAX_STREAM_ROWS, self.top_k, dtype=torch.int32, device=dev)
        self.w = torch.zeros(MAX_STREAM_ROWS, self.top_k, dtype=torch.float32 if self.w_f32 else torch.bfloat16, device=dev)

    def _srcs(self):
        return (self.wqkv, self.wo)

    def _keys64(self):
        q, k, v, o = self._mods
        return (_versions(q.weight, k.weight, v.weight), _versions(o.weight))

    def _packed64_sources(self):
        if self.shared is None:
            return self._srcs(), self._keys64()
        sh = self.shared
        return (self._srcs() + (self.wgu_s, self.wdown_s),
                self._keys64() + (_versions(sh.gate_proj.weight, sh.up_proj.weight), _versions(sh.down_proj.weight)))

    def _router_logits(self, h1):
        """[M, E] bf16 = F.linear(rmsnorm(h1), gate.weight): the f32-FMA GEMV up to FMA_GEMV_ROWS rows, the MFMA weight stream beyond, in
        chunks of 16 rows (the router matrix is small and read in place: no packed copy to keep in step)."""
        M, H = h1.shape[0], self.H
        # a shared-expert layer: the stacked [E + 1, H] copy -- the output is [M, E + 1], column E the shared gate's logit
        wr = self.router_w if self.shared is not None else self.router.weight
        E = wr.shape[0]
        if M <= FMA_GEMV_ROWS or not self.stream_ok:
            return self._gemv(h1, wr, None, self.n2.weight, self.eps2, None, E, H, 0)
        out = torch.empty(M, E, dtype=torch.bfloat16, device=h1.device)
        for r0 in range(0, M, MAX_ROWS16):
            n = min(MAX_ROWS16, M - r0)
            rc = self.lib.ll_linear_rows16_bf16(h1.data_ptr() + r0 * h1.stride(0) * 2, h1.stride(0), wr.data_ptr(), H, None, self.n2.weight.data_ptr(),
                                                self.eps2, None, 0, out.data_ptr() + r0 * E * 2, E, n, E, H, 0, torch.cuda.current_stream().cuda_stream)
            if rc != 0:
                _lib.check(rc, "ll_linear_rows16_bf16")
        return out

    def _shared_rows(self, h1, pre2):
        """[M, H] bf16 = shared_expert(rmsnorm(h1)) on the dense MLP's kernels: gate|up with the RMSNorm prologue and the SiLU*mul epilogue, down
        with the plain one -- 1..16 rows on the concatenated copy, 17..64 on the packed copies with ``pre2`` = the pre-norm pair o_proj made."""
        M, H = h1.shape[0], self.H
        if M > MAX_ROWS16:
            xs2, ssq2 = pre2
            act = _rows64(self.lib, xs2, xs2.stride(0), self.p64[2], None, None, self.Is, 2, row_ssq=ssq2, eps=self.eps2)
            return _rows64(self.lib, act, act.stride(0), self.p64[3], None, None, H, 0)
        act = self._gemv(h1, self.wgu_s, None, self.n2.weight, self.eps2, None, self.Is, H, 2)
        return self._gemv(act, self.wdown_s, None, None, 0.0, None, H, self.Is, 0)

    def _mlp(self, h1, pq=None, pre2=None):
        """Router logits, routing, experts + residual on 1..64 rows of the un-normalised post-attention residual stream h1 [M, H]."""
        M, H = h1.shape[0], self.H
        stream = torch.cuda.current_stream().cuda_stream
        logits = self._router_logits(h1)
        route = "ll_moe_route_f32" if self.w_f32 else "ll_moe_route_bf16"
        rc = getattr(self.lib, route)(logits.data_ptr(), logits.stride(0), M, self.E, self.top_k, int(self.norm_topk), self.idx.data_ptr(),
                                      self.w.data_ptr(), self.ws.t.data_ptr(), self.ws.bytes, stream)
        if rc != 0:
            _lib.check(rc, route)
        out = torch.empty(M, H, dtype=torch.bfloat16, device=h1.device)
        if not self.w_f32 and self.shared is None:
            rc = self.lib.ll_moe_experts_bf16(h1.data_ptr(), h1.stride(0), self.n2.weight.data_ptr(), self.eps2, self.idx.data_ptr(),
                                              self.w.data_ptr(), self.experts.gate_up_proj.data_ptr(), self.experts.down_proj.data_ptr(),
                                              h1.data_ptr(), h1.stride(0), out.data_ptr(), H, M, self.E, self.top_k, H, self.I,
                                              self.ws.t.data_ptr(), self.ws.bytes, stream)
            if rc != 0:
                _lib.check(rc, "ll_moe_experts_bf16")
            return out
        s = self._shared_rows(h1, pre2) if self.shared is not None else None
        rc = self.lib.ll_moe_experts_ex_bf16(h1.data_ptr(), h1.stride(0), self.n2.weight.data_ptr(), self.eps2, self.idx.data_ptr(),
                                             self.w.data_ptr(), int(self.w_f32), self.experts.gate_up_proj.data_ptr(),
                                             self.experts.down_proj.data_ptr(), h1.data_ptr(), h1.stride(0),
                                             s.data_ptr() if s is not None else None, s.stride(0) if s is not None else 0,
                                             logits.data_ptr() + 2 * self.E if s is not None else None, logits.stride(0) if s is not None else 0,
                                             out.data_ptr(), H, M, self.E, self.top_k, H, self.I, self.ws.t.data_ptr(), self.ws.bytes, stream)
        if rc != 0:
            _lib.check(rc, "ll_moe_experts_ex_bf16")
        return out

    def run64(self, h, mask, cache, pe, pre=None, next_norm=None):
        """17..64 sequences: q|k|v and o_proj on the packed copies as in the parent -- o_proj without the pre-norm hand-over, the MoE calls take
        the un-normalised h1 and the norm weight themselves -- then the MoE calls.  Returns (h_out, None): the next layer makes its own pre-norm."""
        B, H = h.shape[0], self.H
        x = h.view(B, H)
        self.packed64()
        pqkv, po = self.p64[:2]
        xs, ssq = pre if pre is not None else _prenorm64(self.lib, x, self.n1.weight)
        nqkv = self.nq + 2 * self.nkv_dim
        qkv = _rows64(self.lib, xs, xs.stride(0), pqkv, self.bqkv, None, nqkv, 0, row_ssq=ssq, eps=self.eps1)
        att = self._attn(qkv, nqkv, mask, cache, pe, B, h.device)
        if self.shared is not None:      # the shared expert's gate|up takes the post-attention pre-norm from o_proj's closing launch
            h1, xs2, ssq2 = _rows64(self.lib, att, att.stride(0), po, self.bo, x, H, 1, next_norm=self.n2.weight)
            return self._mlp(h1, pre2=(xs2, ssq2)).view(B, 1, H), None
        h1 = _rows64(self.lib, att, att.stride(0), po, self.bo, x, H, 1)
        return self._mlp(h1).view(B, 1, H), None


def _layer_forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                   position_embeddings=None, **kwargs):
    st = self._ll_fused
    if st.eligible(hidden_states, attention_mask, past_key_values, position_embeddings):
        return st.run(hidden_states, attention_mask, past_key_values, position_embeddings)
    return self._ll_layer_orig(hidden_states, attention_mask=attention_mask, position_ids=position_ids,
                               past_key_values=past_key_values, use_cache=use_cache, position_embeddings=position_embeddings,
                               **kwargs)


def _head_norm_declined(att) -> Optional[str]:
    """The structural part of ``decoder_layer_declined`` for per-head q / k norms (Qwen3 layout): both or none, the model's own *RMSNorm with
    ``variance_epsilon`` (the condition of ``accelerate_elementwise``), one weight per element of a head, one eps."""
    qn, kn = getattr(att, "q_norm", None), getattr(att, "k_norm", None)
    if qn is None and kn is None:
        return None
    if qn is None or kn is None:
        return "only one of q_norm / k_norm"
    for name, m in (("q_norm", qn), ("k_norm", kn)):
        if not (type(m).__name__.endswith("RMSNorm") and hasattr(m, "variance_epsilon") and isinstance(getattr(m, "weight", None), torch.Tensor)):
            return f"{name} is not an RMSNorm with variance_epsilon"
        if m.weight.numel() != getattr(att, "head_dim", 0):
            return f"{name} is not a norm over head_dim"
    if float(qn.variance_epsilon) != float(kn.variance_epsilon):
        return "q_norm and k_norm differ in variance_epsilon"
    return None


MOE_MAX_EXPERTS, MOE_MAX_TOP_K, MOE_MAX_INTERMEDIATE = 256, 8, 32768       # bounds of ll_moe_route_bf16 / ll_moe_experts_bf16 (include/llamole_hip.h)


def _is_moe_block(mlp) -> bool:
    """Whether ``mlp`` is a mixture-of-experts block of any family (as opposed to a dense gated MLP), judged by its parts."""
    return (hasattr(mlp, "experts") or hasattr(mlp, "shared_expert") or hasattr(mlp, "shared_experts")
            or type(mlp).__name__.endswith(("MoeBlock", "MoE")))


# block class -> (family, router class, experts class): a family is taken by ALL its parts, never by the block's name alone -- the router class
# decides the arithmetic of the routing weights (Mixtral: f32, always renormalised; Qwen2-MoE / Qwen3-MoE: bf16, norm_topk_prob)
MOE_FAMILIES = {"Qwen3MoeSparseMoeBlock": ("qwen3", None, None),
                "MixtralSparseMoeBlock": ("mixtral", "MixtralTopKRouter", "MixtralExperts"),
                "Qwen2MoeSparseMoeBlock": ("qwen2", "Qwen2MoeTopKRouter", "Qwen2MoeExperts")}


def _moe_family(mlp) -> Optional[str]:
    """"qwen3" | "mixtral" | "qwen2" for a block of a fused family, None for any other."""
    family, router, experts = MOE_FAMILIES.get(type(mlp).__name__, (None, None, None))
    if family is None or (router is not None and (type(getattr(mlp, "gate", None)).__name__ != router
                                                  or type(getattr(mlp, "experts", None)).__name__ != experts)):
        return None
    return family


def _shared_expert_declined(mlp, hidden: int) -> Optional[str]:
    """The shared expert of a Qwen2MoeSparseMoeBlock: a dense gated MLP of three plain bias-free nn.Linear with SiLU, and a one-row gate."""
    sh, sg = getattr(mlp, "shared_expert", None), getattr(mlp, "shared_expert_gate", None)
    lin = [getattr(sh, a, None) for a in ("gate_proj", "up_proj", "down_proj")]
    if not all(type(m) is nn.Linear for m in lin) or type(sg) is not nn.Linear:
        return "shared expert whose projections are not plain nn.Linear"
    if any(m.bias is not None for m in lin) or sg.bias is not None:
        return "shared expert bias"
    if not _is_silu(getattr(sh, "act_fn", None)):
        return "shared expert activation is not SiLU"
    Is = lin[0].out_features
    if (tuple(lin[0].weight.shape) != (Is, hidden) or tuple(lin[1].weight.shape) != (Is, hidden) or tuple(lin[2].weight.shape) != (hidden, Is)
            or tuple(sg.weight.shape) != (1, hidden)):
        return "shared expert is not gate_proj / up_proj [I_s, H], down_proj [H, I_s] with a shared_expert_gate [1, H]"
    if Is % 8 != 0:
        return "shared_expert_intermediate_size is not a multiple of 8"
    if Is > MOE_MAX_INTERMEDIATE:
        return f"shared_expert_intermediate_size above {MOE_MAX_INTERMEDIATE}"
    return None


def _moe_block_declined(mlp, hidden: int) -> Optional[str]:
    """The structural part of ``decoder_layer_declined`` for a sparse-MoE block.  Fused: the Qwen3-MoE layout (softmax over all experts, top-k,
    optional renormalisation, SiLU experts stored as [E, 2I, H] / [E, H, I], no shared expert, no biases), the Mixtral layout (the same with
    f32 routing weights, always renormalised) and the Qwen2-MoE layout (the Qwen3 routing plus a sigmoid-gated shared expert).  Other router
    families (DeepSeek, GPT-OSS) have different semantics and are named, not guessed at."""
    kind = type(mlp).__name__
    family = _moe_family(mlp)
    if family is None:
        return f"MoE block of an unsupported kind ({kind})"
    if family == "qwen2":
        why = _shared_expert_declined(mlp, hidden)
        if why is not None:
            return why
    elif any(getattr(mlp, a, None) is not None for a in ("shared_expert", "shared_experts", "shared_expert_gate")):
        return "MoE block of an unsupported kind (shared expert)"
    experts, gate = getattr(mlp, "experts", None), getattr(mlp, "gate", None)
    wgu, wd, wr = getattr(experts, "gate_up_proj", None), getattr(experts, "down_proj", None), getattr(gate, "weight", None)
    if not all(isinstance(t, nn.Parameter) for t in (wgu, wd, wr)) or wgu.dim() != 3 or wd.dim() != 3 or wr.dim() != 2:
        return "MoE block of an unsupported kind (experts are not gate_up_proj [E, 2I, H] / down_proj [E, H, I] parameters with a gate.weight [E, H])"
    E, H, I = wd.shape
    if tuple(wgu.shape) != (E, 2 * I, H) or tuple(wr.shape) != (E, H) or H != hidden:
        return "MoE block of an unsupported kind (experts are not gate_up_proj [E, 2I, H] / down_proj [E, H, I] parameters with a gate.weight [E, H])"
    if not hasattr(gate, "top_k") or (family != "mixtral" and not hasattr(gate, "norm_topk_prob")):      # (Mixtral's router always renormalises)
        return "MoE router without top_k / norm_topk_prob"
    if any(getattr(m, a, None) is not None for m in (experts, gate) for a in ("bias", "gate_up_proj_bias", "down_proj_bias")):
        return "MoE expert bias"
    if not _is_silu(getattr(experts, "act_fn", None)):
        return "activation is not SiLU"
    if E > MOE_MAX_EXPERTS:
        return f"more than {MOE_MAX_EXPERTS} experts"
    if not 1 <= int(gate.top_k) <= min(E, MOE_MAX_TOP_K):
        return f"top_k is not in 1..min(E, {MOE_MAX_TOP_K})"
    if I % 8 != 0:
        return "moe_intermediate_size is not a multiple of 8"
    if I > MOE_MAX_INTERMEDIATE:
        return f"moe_intermediate_size above {MOE_MAX_INTERMEDIATE}"
    return None


def attn_window(att):
    """The sliding window of an HF attention module, None for full attention: its ``sliding_window`` attribute where the class has one (Qwen2 /
    Qwen3 / Ministral: None on the full layers of a mixed model), else its config's -- MistralAttention keeps none and hands
    ``config.sliding_window`` to the attention call.  Qwen2MoeAttention sets the attribute on its sliding layers only and its config holds
    ``sliding_window = 0`` when windows are off: a layer without the attribute that ``layer_types`` names "full_attention" has no window."""
    if hasattr(att, "sliding_window"):
        return att.sliding_window
    cfg = getattr(att, "config", None)
    types, idx = getattr(cfg, "layer_types", None), getattr(att, "layer_idx", None)
    if types is not None and isinstance(idx, int) and 0 <= idx < len(types) and types[idx] != "sliding_attention":
        return None
    return getattr(cfg, "sliding_window", None)


def _config_window(att):
    """The window HF's mask construction applies to this attention module's layer, read off the module's config: ``sliding_window`` where
    ``layer_types`` names the layer "sliding_attention" (Qwen2 / Qwen3 / Ministral), or for a config without ``layer_types`` on every layer
    (Mistral); None = a full causal mask."""
    cfg = getattr(att, "config", None)
    types = getattr(cfg, "layer_types", None)
    if types is not None:
        idx = getattr(att, "layer_idx", None)
        if not (isinstance(idx, int) and 0 <= idx < len(types) and types[idx] == "sliding_attention"):
            return None
    return getattr(cfg, "sliding_window", None)


def decoder_layer_declined(layer: nn.Module) -> Optional[str]:
    """Why ``fuse_decoder_layers`` would not fuse this decoder layer (None: it would) -- the sibling of ``model_decode_declined``.  Structural
    reasons come first and dtype / device reasons last, so the layout of a model can be judged on the CPU."""
    att, mlp = getattr(layer, "self_attn", None), getattr(layer, "mlp", None)
    if att is None or mlp is None:
        return "no self_attn / mlp"
    if hasattr(layer, "_ll_fused"):
        return "already installed"
    moe = _is_moe_block(mlp)
    if not (all(type(getattr(att, a, None)) is nn.Linear for a in ("q_proj", "k_proj", "v_proj", "o_proj"))
            and (moe or all(type(getattr(mlp, a, None)) is nn.Linear for a in ("gate_proj", "up_proj", "down_proj")))):
        return "projections are not plain nn.Linear"
    if moe:
        why = _moe_block_declined(mlp, att.q_proj.in_features)
        if why is not None:
            return why
    elif not _is_silu(getattr(mlp, "act_fn", None)):
        return "activation is not SiLU"
    if not (hasattr(layer, "input_layernorm") and hasattr(layer, "post_attention_layernorm")
            and hasattr(layer.input_layernorm, "variance_epsilon")):
        return "no RMSNorm pair with variance_epsilon"
    if getattr(att, "head_dim", 0) not in (64, 128):
        return "head_dim is not 64 or 128"
    if att.q_proj.in_features % 8 != 0 or att.q_proj.in_features > 8192:
        return "hidden size is not a multiple of 8 up to 8192"
    if not moe and (mlp.gate_proj.bias is not None or mlp.up_proj.bias is not None or mlp.down_proj.bias is not None):
        return "MLP bias"
    win = attn_window(att)
    if win is not None and not (type(win) is int and win >= 1):
        return f"sliding_window={win!r} is not a positive int"
    if win != _config_window(att):
        # a window on the module that its config does not state for this layer: HF builds the masks of the prompt pass and of the op-by-op
        # decode from the config, so the windowed kernels would decode another model than the prefill filled the cache for
        return "sliding-window layer"
    why = _head_norm_declined(att)
    if why is not None:
        return why
    rm, rm_ok = _multiplier(layer, "residual_multiplier")
    if not rm_ok:
        return RESIDUAL_MULTIPLIER_DECLINED
    if moe and rm != 1.0:
        return MOE_RESIDUAL_MULTIPLIER_DECLINED
    norms = [m for m in (getattr(att, "q_norm", None), getattr(att, "k_norm", None)) if m is not None]
    extra = [m.weight for m in norms] + ([mlp.experts.gate_up_proj, mlp.experts.down_proj, mlp.gate.weight] if moe else [])
    if moe and _moe_family(mlp) == "qwen2":
        sh = mlp.shared_expert
        extra += [sh.gate_proj.weight, sh.up_proj.weight, sh.down_proj.weight, mlp.shared_expert_gate.weight]
    if att.q_proj.weight.dtype != torch.bfloat16 or any(t.dtype != torch.bfloat16 for t in extra):
        return "weights are not bf16"
    if not att.q_proj.weight.is_cuda or not all(t.is_cuda for t in extra):
        return "weights are not on the device"
    if moe and not all(t.is_contiguous() for t in extra[len(norms):]):
        return "MoE weights are not contiguous"
    return None


def fuse_decoder_layers(model: nn.Module) -> int:
    """Run every decoder layer of a Qwen2 / Llama / Mistral / Qwen3-layout HF model as five launches at decode (batch <= 16), static cache with the fused append of ``fuse_cache_update``, boolean sdpa-style mask.  Any other call --
    prefill, larger batches, a dynamic cache -- takes the layer's previous forward.  Returns the number of patched layers."""
    lib = _lib.load()
    base = getattr(model, "model", model)
    layers = getattr(base, "layers", None)
    if layers is None:
        return 0
    n = 0
    workspaces: dict = {}       # one MoE scratch per model and size
    split_ws: dict = {}         # one key-split attention scratch per model and shape (caches beyond ATTN_MAXLEN slots)
    for layer in layers:
        if decoder_layer_declined(layer) is not None:
            continue
        layer._ll_fused = (_FusedMoeLayer(lib, layer, workspaces, split_ws) if _is_moe_block(layer.mlp)
                           else _FusedLayer(lib, layer, split_ws))
        layer._ll_layer_orig = layer.forward
        layer.forward = types.MethodType(_layer_forward, layer)
        n += 1
    return n


def restore_decoder_layers(model: nn.Module) -> None:
    base = getattr(model, "model", model)
    for layer in getattr(base, "layers", []):
        if "_ll_fused" in layer.__dict__:
            del layer.__dict__["forward"]
            del layer.__dict__["_ll_fused"]
            del layer.__dict__["_ll_layer_orig"]
            for sub in layer.modules():       # the layer's concatenated gate|up copy goes with it (rebuilt on the next install)
                sub.__dict__.pop("_ll_gate_up", None)
                sub.__dict__.pop("_ll_gate_up_key", None)
                sub.__dict__.pop("_ll_router_gate", None)
                sub.__dict__.pop("_ll_router_gate_key", None)


# ------------------------------------------------------------------------------------------ whole decode step of the base model
def _model_forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None,
                   use_cache=None, **kwargs):
    """Qwen2Model.forward / LlamaModel.forward for ONE new token per sequence on the fused layers: embedding gather, one
    prologue launch (rotary cos/sin + causal/padding key mask, instead of ~12 ATen launches of rotary_emb and
    create_causal_mask), the five-launch layers, final norm.  Anything else goes to the original forward."""
    st = self._ll_decode
    st["served"] = False          # whether this call ran on the fused path (GraphedDecoder reads it after its eager warm-up step)
    st["declined"] = None         # why a decode-shaped call on a long static cache went to HF's layers instead (the reason, for this call)
    layers = self.layers[: self.config.num_hidden_layers]
    if (input_ids is not None and inputs_embeds is None and input_ids.dim() == 2 and input_ids.shape[1] == 1
            and input_ids.shape[0] <= MAX_STREAM_ROWS and input_ids.is_cuda and not torch.is_grad_enabled() and past_key_values is not None
            and (st.get("embed_scale") is None or input_ids.dtype == torch.long)      # ll_embed_rows_bf16 reads int64 ids
            and attention_mask is not None and attention_mask.dim() == 2 and attention_mask.dtype == torch.long
            and attention_mask.stride(1) == 1 and position_ids is not None and position_ids.shape == input_ids.shape
            and position_ids.dtype == torch.long and not kwargs.get("output_hidden_states") and not kwargs.get("output_attentions")
            and getattr(past_key_values, "layers", None) and all(getattr(l, "_ll_fused_update", False) for l in past_key_values.layers)
            and attention_mask.shape[1] == past_key_values.layers[0].keys.shape[2]
            and (past_key_values.layers[0].keys.dtype == torch.bfloat16 or _is_kv8(past_key_values.layers[0]))
            and all(f.attn_serves(input_ids.shape[0], 1, attention_mask.shape[1], _is_kv8(past_key_values.layers[0])) for f in st["attn_kinds"])):
        B, maxlen, D = input_ids.shape[0], attention_mask.shape[1], st["D"]
        dev = input_ids.device
        h = _embed(self, st, input_ids)
        if h.dtype == torch.bfloat16 and h.is_contiguous():
            cos = torch.empty(B, 1, D, dtype=torch.bfloat16, device=dev)
            sin = torch.empty(B, 1, D, dtype=torch.bfloat16, device=dev)
            mask = torch.empty(B, 1, 1, maxlen, dtype=torch.bool, device=dev)
            pos = past_key_values.layers[0].cumulative_length
            posid = position_ids.contiguous()
            if st.get("dyn") is None:
                inv_freq = self.rotary_emb.inv_freq
                rc = st["lib"].ll_decode_prologue(posid.data_ptr(), inv_freq.data_ptr(), float(self.rotary_emb.attention_scaling),
                                                  attention_mask.data_ptr(), attention_mask.stride(0), pos.data_ptr(), cos.data_ptr(),
                                                  sin.data_ptr(), mask.data_ptr(), B, D, maxlen, torch.cuda.current_stream().cuda_stream)
                if rc != 0:
                    _lib.check(rc, "ll_decode_prologue")
            else:
                # dynamic NTK: the kernel picks the frequencies from the call's own position ids (never rotary_emb.inv_freq, which HF replaces)
                inv0, table, rows = _dyn_freqs(self, st, maxlen)
                rc = st["lib"].ll_decode_prologue_dyn(posid.data_ptr(), inv0.data_ptr(), table.data_ptr() if table is not None else None,
                                                      st["dyn"]["max_pos"], rows, 1.0, attention_mask.data_ptr(), attention_mask.stride(0),
                                                      pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), mask.data_ptr(), B, D, maxlen,
                                                      torch.cuda.current_stream().cuda_stream)
                if rc != 0:
                    _lib.check(rc, "ll_decode_prologue_dyn")
            pe = (cos, sin)
            if layers[0]._ll_fused.eligible(h, mask, past_key_values, pe):
                if B > MAX_ROWS16:
                    # 17..64 sequences: every layer's closing launch also produces the next layer's input pre-norm
                    pre = None
                    for i, layer in enumerate(layers):
                        nxt = layers[i + 1]._ll_fused if i + 1 < len(layers) else None
                        h, pre = layer._ll_fused.run64(h, mask, past_key_values, pe, pre, nxt.n1.weight if nxt is not None else None)
                else:
                    for layer in layers:
                        h = layer._ll_fused.run(h, mask, past_key_values, pe)
                h = self.norm(h)
                st["served"] = True
                return st["out_cls"](last_hidden_state=h, past_key_values=past_key_values if use_cache else None)
    if st.get("suffix") and input_ids is not None and inputs_embeds is None and input_ids.dim() == 2:
        out = _suffix_forward(self, st, layers, input_ids, attention_mask, position_ids, past_key_values, use_cache, kwargs)
        if out is not None:
            st["served"] = True
            return out
    clayers = getattr(past_key_values, "layers", None)
    keys = getattr(clayers[0], "keys", None) if clayers else None
    if input_ids is not None and input_ids.dim() == 2 and input_ids.shape[1] <= MAX_APPEND_ROWS and keys is not None and keys.dim() == 4 \
            and (keys.shape[2] > ATTN_MAXLEN or _is_kv8(clayers[0]) or any(f._windowed(keys.shape[2]) for f in st["attn_kinds"])) \
            and not all(f.attn_serves(input_ids.shape[0], input_ids.shape[1], keys.shape[2], _is_kv8(clayers[0])) for f in st["attn_kinds"]):
        st["declined"] = (f"decoder_layers: a static cache of {keys.shape[2]} slots ({input_ids.shape[0]} x {input_ids.shape[1]} new positions) is "
                          f"outside the bounds of the key-split attention (at most {ATTN_SPLIT_MAXLEN} slots, {MAX_STREAM_ROWS} sequences at decode)")
    return self._ll_model_orig(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids,
                               past_key_values=past_key_values, inputs_embeds=inputs_embeds, use_cache=use_cache, **kwargs)


def _embed(self, st, input_ids):
    """The input rows of the layers: ``embed_tokens(input_ids)``, or for a model with an embedding_multiplier (Granite layout) the gather
    and the scale in one launch (ll_embed_rows_bf16) -- [B, S, H] bf16 either way."""
    m = st.get("embed_scale")
    if m is None:
        return self.embed_tokens(input_ids)
    table = self.embed_tokens.weight
    V, H = table.shape
    assert input_ids.dtype == torch.long, "ll_embed_rows_bf16 reads int64 ids (the callers send other dtypes to HF's forward)"
    ids = input_ids.contiguous()
    out = torch.empty(*ids.shape, H, dtype=torch.bfloat16, device=ids.device)
    rc = st["lib"].ll_embed_rows_bf16(ids.data_ptr(), table.data_ptr(), table.stride(0), out.data_ptr(), H, ids.numel(), V, H, m,
                                      torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        _lib.check(rc, "ll_embed_rows_bf16")
    return out


def _suffix_forward(self, st, layers, input_ids, attention_mask, position_ids, cache, use_cache, kwargs):
    """[B,S] new tokens (3 <= B*S <= 16) appended at the cache position held by layer 0's counter -- GraphedDecoder.continue_hidden, the
    reference's query-token re-forward -- on the five-launch layers: one prologue launch (cos/sin per row, key mask per row: slot
    j <= pos + s and not padding), then per layer q|k|v with the RMSNorm prologue, rope + append + attention, o_proj + residual, gate|up
    + SiLU*mul, down_proj + residual (ll_linear_rows16_bf16).  None = not this shape: the caller takes the HF forward."""
    B, S = input_ids.shape
    R = B * S
    clayers = getattr(cache, "layers", None)
    if not (S >= 2 and FMA_GEMV_ROWS < R <= MAX_ROWS16 and input_ids.is_cuda and not torch.is_grad_enabled() and clayers
            and (st.get("embed_scale") is None or input_ids.dtype == torch.long)      # ll_embed_rows_bf16 reads int64 ids
            and all(getattr(l, "_ll_fused_update", False) for l in clayers) and attention_mask is not None and attention_mask.dim() == 2
            and attention_mask.dtype == torch.long and attention_mask.stride(1) == 1 and attention_mask.shape[0] == B
            and attention_mask.shape[1] == clayers[0].keys.shape[2] and _kv_layer_ok(clayers[0])
            and clayers[0].keys.shape[0] == B
            and position_ids is not None and position_ids.shape == input_ids.shape and position_ids.dtype == torch.long
            and not kwargs.get("output_hidden_states") and not kwargs.get("output_attentions")
            and all(l._ll_fused.stream_ok for l in layers)
            and all(f.attn_serves(B, S, attention_mask.shape[1], _is_kv8(clayers[0])) for f in st["attn_kinds"])):
        return None
    h = _embed(self, st, input_ids)
    if h.dtype != torch.bfloat16 or not h.is_contiguous():
        return None
    maxlen, D, dev = attention_mask.shape[1], st["D"], input_ids.device
    cos = torch.empty(R, D, dtype=torch.bfloat16, device=dev)
    sin = torch.empty(R, D, dtype=torch.bfloat16, device=dev)
    mask = torch.empty(R, maxlen, dtype=torch.bool, device=dev)
    posid = position_ids.contiguous()
    if st.get("dyn") is None:
        rc = st["lib"].ll_suffix_prologue(posid.data_ptr(), self.rotary_emb.inv_freq.data_ptr(), float(self.rotary_emb.attention_scaling),
                                          attention_mask.data_ptr(), attention_mask.stride(0), clayers[0].cumulative_length.data_ptr(),
                                          cos.data_ptr(), sin.data_ptr(), mask.data_ptr(), B, S, D, maxlen, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _lib.check(rc, "ll_suffix_prologue")
    else:
        inv0, table, rows = _dyn_freqs(self, st, maxlen)
        rc = st["lib"].ll_suffix_prologue_dyn(posid.data_ptr(), inv0.data_ptr(), table.data_ptr() if table is not None else None,
                                              st["dyn"]["max_pos"], rows, 1.0, attention_mask.data_ptr(), attention_mask.stride(0),
                                              clayers[0].cumulative_length.data_ptr(), cos.data_ptr(), sin.data_ptr(), mask.data_ptr(), B, S, D,
                                              maxlen, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _lib.check(rc, "ll_suffix_prologue_dyn")
    for layer in layers:
        h = layer._ll_fused.run_suffix(h, mask, cache, (cos, sin), B, S)
    h = self.norm(h)
    return st["out_cls"](last_hidden_state=h, past_key_values=cache if use_cache else None)


def suffix_on_fused_layers(model: nn.Module, on: bool) -> bool:
    """Switch for the query-token forward of ``fuse_model_decode``-patched models: while on, a [B,S] call with B*S <= 16 rows that
    continues a fused static cache runs on the five-launch layers (GraphedDecoder.continue_hidden turns it on around its call).
    Returns whether the model has the patch."""
    base = getattr(model, "model", model)
    st = base.__dict__.get("_ll_decode")
    if st is None:
        return False
    st["suffix"] = bool(on)
    return True


def _dyn_freqs(base, st, maxlen: int):
    """(inv_freq0, table or None, table rows) of a dynamic NTK model for a static cache of ``maxlen`` slots; the table (rope.py) is built
    once per cache length -- in the eager warm-up step that precedes every capture -- and kept with the patch."""
    dyn = st["dyn"]
    rot = base.rotary_emb
    if maxlen not in dyn["tables"]:
        dyn["tables"][maxlen] = dynamic_inv_freq_table(rot.config, rot.original_inv_freq.device, maxlen)
    table = dyn["tables"][maxlen]
    return rot.original_inv_freq, table, 0 if table is None else table.shape[0]


def model_decode_declined(model: nn.Module) -> Optional[str]:
    """Why ``fuse_model_decode`` would not install on this model (None: it would).  Rotary types: default and the ones with constants fixed at
    construction (linear, llama3, yarn) run on the existing prologue, dynamic NTK on its device-side form; longrope, proportional and
    modules with per-layer-type tables stay on HF's module."""
    base = getattr(model, "model", model)
    layers = getattr(base, "layers", None)
    rot = getattr(base, "rotary_emb", None)
    if layers is None or rot is None or not hasattr(base, "embed_tokens") or not hasattr(base, "norm"):
        return "not a Llama-layout base model"
    if hasattr(base, "_ll_decode"):
        return "already installed"
    if not all(hasattr(l, "_ll_fused") for l in layers):
        return "not every decoder layer is fused"
    rope_type = getattr(rot, "rope_type", "default")
    if not isinstance(rope_type, str):
        return "rope_type per layer type"
    if rope_type not in STATIC_ROPE_TYPES and rope_type != "dynamic":
        return f"rope_type={rope_type}"
    if not hasattr(rot, "inv_freq") or rot.inv_freq.dtype != torch.float32 or not rot.inv_freq.is_cuda:
        return "inv_freq is not an f32 device tensor"
    if rot.inv_freq.numel() * 2 != layers[0]._ll_fused.D:
        return "partial rotary dimension"
    if rope_type == "dynamic":
        inv0 = getattr(rot, "original_inv_freq", None)
        if (inv0 is None or inv0.dtype != torch.float32 or not inv0.is_cuda or inv0.shape != rot.inv_freq.shape
                or not getattr(getattr(rot, "config", None), "max_position_embeddings", None)):
            return "dynamic rope without an f32 device original_inv_freq"
    em, em_ok = _multiplier(base, "embedding_multiplier")
    if not em_ok:
        return EMBEDDING_MULTIPLIER_DECLINED
    if em != 1.0:
        w = getattr(base.embed_tokens, "weight", None)
        if not (type(base.embed_tokens) is nn.Embedding and w is not None and w.dtype == torch.bfloat16 and w.dim() == 2 and w.is_contiguous()
                and w.shape[1] % 8 == 0):
            return EMBEDDING_TABLE_DECLINED
    return None


def fuse_model_decode(model: nn.Module) -> bool:
    """Run the base model's decode step without HF's per-token mask / rotary-table construction (call after
    ``fuse_decoder_layers``; needs every layer fused, f32 ``inv_freq`` and a rope type of ``model_decode_declined``'s list: default,
    linear, llama3, yarn, dynamic).  Returns whether it was installed."""
    if model_decode_declined(model) is not None:
        return False
    base = getattr(model, "model", model)
    rot = base.rotary_emb
    import sys
    from transformers.modeling_outputs import BaseModelOutputWithPast
    # the output class of the base model's own forward: a MoE model's causal-LM head reads `router_logits` (None here) off it
    out_cls = getattr(sys.modules.get(type(base).__module__), "MoeModelOutputWithPast", BaseModelOutputWithPast)
    base._ll_decode = {"lib": _lib.load(), "D": base.layers[0]._ll_fused.D, "out_cls": out_cls}
    # one fused layer per attention kind (full, or a sliding window): the layers of a model share every other size, so these answer for all of
    # them whether the attention entries take a shape (``attn_serves``)
    kinds = {}
    for l in base.layers[: base.config.num_hidden_layers]:
        kinds.setdefault(l._ll_fused.window, l._ll_fused)
    base._ll_decode["attn_kinds"] = tuple(kinds.values())
    em = _multiplier(base, "embedding_multiplier")[0]
    if em != 1.0:
        base._ll_decode["embed_scale"] = em         # Granite layout: gather and scale in one launch (_embed)
    if rot.rope_type == "dynamic":
        base._ll_decode["dyn"] = {"max_pos": int(rot.config.max_position_embeddings), "tables": {}}
    base._ll_model_orig = base.forward
    base.forward = types.MethodType(_model_forward, base)
    return True


def restore_model_decode(model: nn.Module) -> None:
    base = getattr(model, "model", model)
    if "_ll_decode" in base.__dict__:
        del base.__dict__["forward"]
        del base.__dict__["_ll_decode"]
        del base.__dict__["_ll_model_orig"]


# ------------------------------------------------------------------------------------------ one call for the whole stack
def set_packed_route(model: nn.Module, on: bool) -> int:
    """Switch the packed-code route of every quantised fused layer: off = the bf16 five-launch layers on the dequantised weights (the same
    model).  Returns the number of layers that hold packed codes."""
    n = 0
    base = getattr(model, "model", model)
    for layer in getattr(base, "layers", None) or []:
        st = layer.__dict__.get("_ll_fused")
        if st is not None and st.pq is not None:
            st.use_wq = bool(on)
            n += 1
    return n


def accelerate_llm(model: nn.Module, linears: bool = True, fuse: bool = True, layers: bool = True, model_decode: bool = True,
                   quantization_bit=None) -> dict:
    """Apply the decode acceleration stack to an (untouched) HF Llama-family causal LM on a HIP device and report what took
    effect: GEMV under nn.Linear -> fused RMSNorm / rotary / SiLU*mul and q|k|v, gate|up fusion -> decode attention through
    the AttentionInterface registry -> five-launch decoder layers -> one-launch decode prologue.  Every stage falls back to
    the HF code for shapes or architectures it does not cover; pair it with ``GraphedDecoder(..., fused_cache=True)``.
    ``quantization_bit`` 8 | 4 (None: the environment variable LLAMOLE_QUANT_BITS, unset by default) first rounds the decoder-layer Linears
    onto the MX grid in place (``llm_quant.quantize_llm``; on a CPU model that is all it does), so the concatenated copies are made from
    rounded weights; the fused layers then keep the packed codes and stream them at 1..16 token rows."""
    info: dict = {"linears": 0}
    if quantization_bit is None and os.environ.get("LLAMOLE_QUANT_BITS"):
        quantization_bit = int(os.environ["LLAMOLE_QUANT_BITS"])
    bits = check_quantization_bit(quantization_bit)
    if bits is not None:
        info["quantization"] = quantize_llm(model, bits)
    if not next(model.parameters()).is_cuda:
        return info
    if linears:
        info["linears"] = accelerate_linears(model)
    if linears and fuse:
        info.update(accelerate_elementwise(model))
        info["decode_attention"] = bool(use_decode_attention(model))
        if info["decode_attention"] and layers:
            all_layers = list(getattr(getattr(model, "model", model), "layers", None) or [])
            reasons = [decoder_layer_declined(l) for l in all_layers]
            info["decoder_layers_5_launches"] = fuse_decoder_layers(model)
            # static caches beyond ATTN_MAXLEN slots stay fused up to this many (the key-split attention entries); longer ones run HF's layers
            info["long_cache_attention_max_slots"] = ATTN_SPLIT_MAXLEN
            n_moe = sum(isinstance(l.__dict__.get("_ll_fused"), _FusedMoeLayer) for l in all_layers)
            n_win = sum(getattr(l.__dict__.get("_ll_fused"), "window", None) is not None for l in all_layers)
            if n_win:
                # of the fused layers, the sliding-window ones: the windowed key-split attention wherever the cache is longer than the window
                info["sliding_window_layers_fused"] = n_win
            if n_moe:
                # of the fused layers, the ones whose MLP half is the MoE calls (eight launches at 1..16 rows; the key above counts them too)
                info["moe_layers_fused"] = n_moe
            if info["decoder_layers_5_launches"] < len(all_layers):
                info["decoder_layers_declined"] = next((r for r in reasons if r is not None), None)
            if model_decode:
                declined = model_decode_declined(model)
                info["decode_prologue_1_launch"] = fuse_model_decode(model)
                if not info["decode_prologue_1_launch"]:
                    info["decode_prologue_declined"] = declined
    if bits is not None:
        base = getattr(model, "model", model)
        fused = [l.__dict__.get("_ll_fused") for l in (getattr(base, "layers", None) or [])]
        q = info["quantization"]
        q["packed_layers"] = sum(1 for st in fused if st is not None and st.pq is not None)
        # layers without packed codes (not fused, or a size that is not a multiple of 32) run the bf16 kernels on their dequantised weights
        q["bf16_layers"] = len(fused) - q["packed_layers"]
        # token-row counts at which each matrix streams its packed codes; every other call runs the bf16 kernels on the dequantised weights
        q["packed_routes"] = {m: (sorted(WQ_ROUTES.get((bits, m), ())) if FMA_GEMV_ROWS == 2 else []) for m in WQ_MATRICES}
        if any(_is_moe_block(getattr(l, "mlp", None)) for l in (getattr(base, "layers", None) or [])):
            q["experts"] = "bf16"       # expert and router weights are neither rounded nor packed: only the attention Linears of a MoE layer are
        if any(getattr(getattr(l, "mlp", None), "shared_expert", None) is not None for l in (getattr(base, "layers", None) or [])):
            q["shared_expert"] = "bf16"     # a shared expert's Linears are rounded, not packed: they run the bf16 kernels on the dequantised weights
        if any(st is not None and st.rscale is not None and st.wq_bits is not None for st in fused):
            q["bf16_reason"] = WQ_RESIDUAL_MULTIPLIER_REASON
    return info
