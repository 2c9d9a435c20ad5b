"""Weight-only MX quantisation of the LLM's decoder-layer Linears (the reference's ``quantization_bit: 4 | 8``, hparams/model_args.py:112,
model/model_utils/quantization.py:155-170, which loads the LLM through bitsandbytes).

Here the seven Linear weights of every decoder layer (q, k, v, o, gate, up, down) are rounded ONCE onto an OCP microscaling grid: blocks
of 32 consecutive elements along K share one E8M0 scale 2^e (stored as the byte e + 127); elements are FP8 E4M3 (``e4m3fn``, max 448) at 8
bits and FP4 E2M1 (0, 0.5, 1, 1.5, 2, 3, 4, 6) at 4 bits -- the formats gfx950 converts to bf16 in hardware.  The quantiser is exact and
reproducible (``mx_round`` below and ``ll_wq_quantize_bf16`` agree bit for bit):

  * amax = max |w| of the block, on the bf16 values;
  * e = the smallest integer with amax * 2^-e <= elem_max, from the exponent and mantissa bits of amax (no float log2), clamped so that every
    dequantised value is a normal bf16 number; e = 0 for an all-zero block.  Rounding e UP means no element saturates (the OCP floor rule
    clips the block maximum by up to 25 % at 4 bits);
  * element = w * 2^-e rounded to the nearest grid value, ties to even.

E4M3 has 3 mantissa bits, E2M1 one, and the scale is a power of two, so every dequantised weight code * 2^e is EXACTLY a bf16 number.
``quantize_llm`` therefore overwrites ``module.weight`` in place with the dequantised values: the quantised model is an ordinary bf16 model,
and every path that reads bf16 weights (prefill, 17..64-row layers, HF's own generate, a CPU run) computes the same model as the packed-code
decode kernels (``ll_gemv_fused_wq`` / ``ll_linear_rows16_wq``, llm_accel._FusedLayer).  ``lm_head``, the embeddings and the norms stay bf16.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn

FORMATS = {
    # p / thr: elem_max = M * 2^p with the 7 mantissa bits of M in thr; lo / hi: clamp of e; mbits / emin: the element grid
    8: dict(name="mxfp8_e4m3", p=8, thr=0x60, lo=-117, hi=119, mbits=3, emin=-6, vmax=448.0),
    4: dict(name="mxfp4_e2m1", p=2, thr=0x40, lo=-125, hi=125, mbits=1, emin=0, vmax=6.0),
}
BLOCK = 32
LAYER_LINEARS = (("self_attn", "q_proj"), ("self_attn", "k_proj"), ("self_attn", "v_proj"), ("self_attn", "o_proj"),
                 ("mlp", "gate_proj"), ("mlp", "up_proj"), ("mlp", "down_proj"))
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def check_quantization_bit(v) -> Optional[int]:
    """None = off; 4 and 8 are accepted; anything else is refused like the reference does (hparams/finetuning_args.py:371)."""
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, int) or v not in (4, 8):
        raise ValueError(f"We only accept 4-bit or 8-bit quantization, got quantization_bit={v!r}.")
    return int(v)


def decode_codes(codes: torch.Tensor, bits: int) -> torch.Tensor:
    """Element codes (uint8; the low 4 bits at 4 bits) -> f32 values at scale 1.  The two E4M3 NaN codes (0x7f, 0xff) decode to NaN."""
    c = codes.to(torch.int32)
    if bits == 8:
        sign, ex, man = c >> 7, (c >> 3) & 15, (c & 7).float()
        mag = torch.where(ex == 0, man * 2.0 ** -9, torch.ldexp(1.0 + man / 8.0, ex - 7))
        mag = torch.where((c & 0x7f) == 0x7f, torch.full_like(mag, float("nan")), mag)
    elif bits == 4:
        sign, mag = (c >> 3) & 1, torch.tensor(E2M1_VALUES)[(c & 7).long()]
    else:
        raise ValueError("bits must be 4 or 8")
    return torch.where(sign == 1, -mag, mag)


def encode_codes8(dq: torch.Tensor, scale_bytes: torch.Tensor) -> torch.Tensor:
    """The inverse of ``decode_codes(., 8)`` on ``mx_round``'s output: dq [N, K] (values code * 2^e, on the grid: nothing is rounded here) and
    the scale bytes [N, K / 32] -> the E4M3 code bytes [N, K] uint8.  The sign bit follows the sign of dq (of a zero as well, as the device
    quantiser keeps it)."""
    N, K = dq.shape
    one = torch.ones((), dtype=torch.float32, device=dq.device)
    e = scale_bytes.to(torch.int32) - 127
    v = dq.float().reshape(N, K // BLOCK, BLOCK) * torch.ldexp(one, -e).unsqueeze(-1)      # exact: a power of two
    a = v.abs().contiguous()
    b = a.view(torch.int32)
    normal = ((((b >> 23) & 0xff) - 127 + 7) << 3) | ((b >> 20) & 7)
    code = torch.where(a < 2.0 ** -6, (a * 512.0).to(torch.int32), normal) | (torch.signbit(v).to(torch.int32) << 7)
    return code.to(torch.uint8).reshape(N, K)


def mx_round(w: torch.Tensor, bits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The quantiser in plain torch: w [N, K] (rounded to bf16 first) -> (w_dq f32 [N, K], scale bytes uint8 [N, K / 32]).  Works on CPU;
    the oracle of ``ll_wq_quantize_bf16`` and the CPU install path."""
    f = FORMATS[check_quantization_bit(bits)]
    if w.dim() != 2 or w.shape[1] % BLOCK != 0:
        raise ValueError(f"mx_round: K={tuple(w.shape)[-1] if w.dim() else None} must be a multiple of {BLOCK} (one scale per {BLOCK} elements)")
    N, K = w.shape
    blk = w.detach().to(torch.bfloat16).contiguous().reshape(N, K // BLOCK, BLOCK)
    am = (blk.view(torch.int16).to(torch.int32) & 0x7fff).amax(-1)                 # bf16 bits of amax
    e = (am >> 7) - 127 - f["p"] + ((am & 0x7f) > f["thr"]).to(torch.int32)
    e = torch.where(am == 0, torch.zeros_like(e), e.clamp(f["lo"], f["hi"]))
    one = torch.ones((), dtype=torch.float32, device=w.device)
    v = blk.float() * torch.ldexp(one, -e).unsqueeze(-1)                          # exact: a power of two
    a = v.abs().clamp(max=f["vmax"]).contiguous()
    ex = (((a.view(torch.int32) >> 23) & 0xff) - 127).clamp(min=f["emin"])
    q = torch.ldexp(one, ex - f["mbits"])                                          # grid step at this magnitude
    g = torch.round(a / q) * q                                                     # torch.round: half to even
    dq = torch.copysign(g, v) * torch.ldexp(one, e).unsqueeze(-1)
    return dq.reshape(N, K), (e + 127).to(torch.uint8)


def _key(t: torch.Tensor):
    return (t.data_ptr(), t._version)


def round_linear_(mod: nn.Linear, bits: int) -> None:
    """Overwrite ``mod.weight`` in place with its MX-rounded values (the device quantiser on a bf16 HIP weight, ``mx_round`` elsewhere) and
    record (bits, key of the weight AFTER the write) on the module: ``refresh_weight_copies`` rounds again when the key changed."""
    w = mod.weight
    N, K = w.shape
    with torch.no_grad():
        if w.is_cuda and w.dtype == torch.bfloat16 and w.is_contiguous():
            from . import _lib
            rc = _lib.load().ll_wq_quantize_bf16(w.data_ptr(), K, N, K, bits, None, w.data_ptr(), K, torch.cuda.current_stream().cuda_stream)
            if rc != 0:
                _lib.check(rc, "ll_wq_quantize_bf16")
        else:
            w.copy_(mx_round(w, bits)[0].to(w.dtype))
    mod.__dict__["_ll_wq_bits"] = bits
    mod.__dict__["_ll_wq_key"] = _key(w)


def layer_linears(model: nn.Module):
    """(name, module) of the seven Linears of every decoder layer of a Qwen2 / Llama / Mistral-layout HF model."""
    base = getattr(model, "model", model)
    for i, layer in enumerate(getattr(base, "layers", None) or []):
        for parent, name in LAYER_LINEARS:
            mod = getattr(getattr(layer, parent, None), name, None)
            if isinstance(mod, nn.Linear):
                yield f"layers.{i}.{parent}.{name}", mod
        # a shared-expert MoE block (Qwen2-MoE): the shared expert's three Linears are rounded like any other; they keep running the bf16 kernels
        shared = getattr(getattr(layer, "mlp", None), "shared_expert", None)
        for name in ("gate_proj", "up_proj", "down_proj"):
            mod = getattr(shared, name, None)
            if isinstance(mod, nn.Linear):
                yield f"layers.{i}.mlp.shared_expert.{name}", mod


def quantize_llm(model: nn.Module, bits: int) -> dict:
    """Round the decoder-layer Linears of ``model`` in place and report: bits, format name, modules rounded, the ones left alone (K not a
    multiple of 32), packed bytes against bf16 bytes of the rounded matrices."""
    bits = check_quantization_bit(bits)
    if bits is None:
        raise ValueError("quantize_llm: quantization_bit is None")
    done, skipped, packed, dense = 0, [], 0, 0
    for name, mod in layer_linears(model):
        N, K = mod.weight.shape
        if K % BLOCK != 0:
            skipped.append(name)
            continue
        round_linear_(mod, bits)
        done += 1
        packed += N * K * bits // 8 + N * (K // BLOCK)
        dense += 2 * N * K
    return {"bits": bits, "format": FORMATS[bits]["name"], "modules": done, "skipped": skipped, "packed_bytes": packed, "bf16_bytes": dense,
            "byte_ratio": round(packed / dense, 5) if dense else None}


def reround_changed(model: nn.Module) -> int:
    """Round again, in place, every rounded weight whose (data_ptr, _version) changed since it was rounded (an optimiser step, a merged
    adapter, load_state_dict).  Returns the number of weights rounded."""
    n = 0
    for mod in model.modules():
        bits = mod.__dict__.get("_ll_wq_bits")
        if bits is not None and isinstance(getattr(mod, "weight", None), torch.Tensor) and mod.__dict__.get("_ll_wq_key") != _key(mod.weight):
            round_linear_(mod, bits)
            n += 1
    return n
