"""The microscaled FP8 (OCP MXFP8) static KV cache of the fused decode: ``GraphedDecoder(..., kv_cache="mxfp8")``, opt-in.

Storage format (the one place it is defined on the Python side; include/llamole_hip.h and DESIGN.md 4v say the same).  Per cache layer four
contiguous ``uint8`` tensors:
  * ``keys`` / ``values``               [B, nkv, maxlen, D]       FP8 E4M3 codes (OCP e4m3fn);
  * ``key_scales`` / ``value_scales``   [B, nkv, maxlen, D / 32]  E8M0 scale bytes: e + 127 of the scale 2^e that 32 consecutive elements of
                                                                  head_dim share.
The stored row of a slot is ``llm_quant.mx_round(row, 8)`` of the bf16 row a bf16 ``StaticCache`` stores: K behind the optional head RMSNorm and
the rotation, V as it leaves q|k|v.  A row is D + D / 32 bytes against 2 D (0.516); every dequantised value is exactly a bf16 number.

``keys.shape[2]`` is the slot count and ``keys.dtype == torch.uint8`` identifies the cache type to ``llm_accel``, whose fused layers then call
``ll_decode_attn_rope_kv8`` / ``ll_suffix_attn_rope_kv8`` at every cache length.  A call from HF's own modules (the prompt pass, a layer the fused
path declines, the op-by-op query-token forward) goes through ``update``: the new rows are stored quantised (``ll_kv8_store_bf16``), the layer's
slots up to the last new one are dequantised (``ll_kv8_load_bf16``) into ONE bf16 staging pair shared by all layers of the cache -- layers run
one after the other on one stream -- and that pair is returned, so HF's attention works unchanged on the numbers the fused kernels see.  No
bf16 cache is ever allocated.  On a CPU model the same class runs on ``mx_round`` in torch.

Position counters follow the cache they stand in for.  On a HIP device the fused convention of ``llm_accel.fuse_cache_update`` holds from the
start (``_ll_fused_update``): every layer writes at the position in layer 0's on-device ``cumulative_length`` and the caller advances it once per
forward.  On the CPU every layer advances its own counter, like transformers' ``StaticLayer``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from transformers.cache_utils import Cache, StaticCache, StaticLayer

from .llm_quant import BLOCK, decode_codes, encode_codes8, mx_round

KV_CACHE_KINDS = ("mxfp8",)
HEAD_DIMS = (64, 128)


def check_kv_cache(v) -> Optional[str]:
    """None = the bf16 ``StaticCache``; "mxfp8" = ``MX8StaticCache``; anything else is refused."""
    if v is None:
        return None
    if not isinstance(v, str) or v not in KV_CACHE_KINDS:
        raise ValueError(f"kv_cache must be None or one of {KV_CACHE_KINDS}, got {v!r}")
    return v


def cache_layer_types(config) -> list:
    """The kind of every cache layer of ``config`` as transformers' ``StaticCache`` would dispatch it ("full_attention", "sliding_attention",
    ...): ``layer_types`` where the config has them, else derived from ``sliding_window`` (Mistral-v0.1: every layer sliding)."""
    from transformers.cache_utils import get_layer_types_and_kwargs
    return list(get_layer_types_and_kwargs(config.get_text_config(decoder=True))[0])


class FullLengthStaticCache(StaticCache):
    """A static cache in which EVERY layer is a full-length ``StaticLayer`` of ``max_cache_len`` slots, for a config with sliding-window layers.
    transformers' own choice for those, ``StaticSlidingWindowLayer``, keeps its length in a Python int and picks its branch on the host (index
    copy while filling, ``roll`` once full): a captured graph would replay whichever branch ran at capture time.  Here slot j always holds
    position j; the window is applied by the mask (HF's sliding mask over ``get_mask_sizes() == (max_cache_len, 0)``) or inside the windowed
    attention kernels.  All slots are kept: no memory is saved (a ring buffer is not what this is)."""

    def __init__(self, config, max_cache_len: int):
        Cache.__init__(self, layers=[StaticLayer(max_cache_len=max_cache_len) for _ in cache_layer_types(config)])


def static_cache_for(config, max_cache_len: int) -> StaticCache:
    """The bf16 static cache of the graphed decode: transformers' ``StaticCache`` for a config whose layers are all full attention, a
    ``FullLengthStaticCache`` for one with sliding-window layers."""
    if any(k != "full_attention" for k in cache_layer_types(config)):
        return FullLengthStaticCache(config, max_cache_len)
    return StaticCache(config=config, max_cache_len=max_cache_len)


def mx8_cache_bytes(B: int, nkv: int, maxlen: int, D: int, layers: int) -> int:
    """Bytes of the codes and scales of an MX8 cache (the shared staging pair, one bf16 layer, comes on top)."""
    return 2 * layers * B * nkv * maxlen * (D + D // BLOCK)


def mx8_quantize_rows(x: torch.Tensor):
    """[..., D] -> (codes uint8 [..., D], scale bytes uint8 [..., D / 32]) through ``mx_round``."""
    D = x.shape[-1]
    dq, sb = mx_round(x.reshape(-1, D), 8)
    return encode_codes8(dq, sb).reshape(x.shape), sb.reshape(*x.shape[:-1], D // BLOCK)


def mx8_dequantize(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """codes [..., D], scale bytes [..., D / 32] -> f32 [..., D] = ``decode_codes`` x 2^e (exact)."""
    one = torch.ones((), dtype=torch.float32, device=codes.device)
    s = torch.ldexp(one, scales.to(torch.int32) - 127).repeat_interleave(BLOCK, dim=-1)
    return decode_codes(codes, 8).to(codes.device) * s


class MX8StaticLayer(StaticLayer):
    """One layer of ``MX8StaticCache``: ``keys`` / ``values`` are the code tensors, ``key_scales`` / ``value_scales`` the scale bytes."""

    _ll_fused_update = True

    def __init__(self, cache: "MX8StaticCache", max_cache_len: int, batch_size: int, num_heads: int, head_dim: int, device):
        super().__init__(max_cache_len=max_cache_len)
        self._cache = cache
        self.device, self.dtype = torch.device(device), torch.uint8
        self.batch_size, self.num_heads, self.k_head_dim, self.v_head_dim = batch_size, num_heads, head_dim, head_dim
        shape = (batch_size, num_heads, max_cache_len, head_dim)
        sshape = (batch_size, num_heads, max_cache_len, head_dim // BLOCK)
        self.keys = torch.zeros(shape, dtype=torch.uint8, device=device)
        self.values = torch.zeros(shape, dtype=torch.uint8, device=device)
        self.key_scales = torch.zeros(sshape, dtype=torch.uint8, device=device)
        self.value_scales = torch.zeros(sshape, dtype=torch.uint8, device=device)
        self.cumulative_length = torch.zeros((), dtype=torch.long, device=device)
        self.is_initialized = True

    def lazy_initialization(self, key_states, value_states) -> None:      # allocated at construction
        return None

    def reset(self) -> None:
        for t in (self.keys, self.values, self.key_scales, self.value_scales, self.cumulative_length):
            t.zero_()

    def reorder_cache(self, beam_idx) -> None:
        raise NotImplementedError("MX8StaticCache does not implement the beam reorder (num_beams > 1 needs the bf16 cache: kv_cache=None)")

    def update(self, key_states: torch.Tensor, value_states: torch.Tensor, *args, **kwargs):
        """Store the S new rows quantised at the slots behind the position counter, dequantise the layer's slots up to the last new one into
        the cache's staging pair and return that pair."""
        cache = self._cache
        S = key_states.shape[-2]
        pos = cache.position_of(self)
        Kst, Vst = cache.staging
        if self.keys.is_cuda:
            from . import _lib
            lib = _lib.load()
            k = key_states if key_states.dtype == torch.bfloat16 and key_states.stride(3) == 1 else key_states.to(torch.bfloat16).contiguous()
            v = value_states if value_states.dtype == torch.bfloat16 and value_states.stride(3) == 1 else value_states.to(torch.bfloat16).contiguous()
            B, nkv, _, D = k.shape
            L = self.max_cache_len
            I64x3 = C.c_int64 * 3
            stream = torch.cuda.current_stream().cuda_stream
            rc = lib.ll_kv8_store_bf16(self.keys.data_ptr(), self.key_scales.data_ptr(), self.values.data_ptr(), self.value_scales.data_ptr(),
                                       k.data_ptr(), v.data_ptr(), pos.data_ptr(), B, nkv, S, L, D, I64x3(k.stride(0), k.stride(1), k.stride(2)),
                                       I64x3(v.stride(0), v.stride(1), v.stride(2)), stream)
            if rc != 0:
                _lib.check(rc, "ll_kv8_store_bf16")
            rc = lib.ll_kv8_load_bf16(self.keys.data_ptr(), self.key_scales.data_ptr(), self.values.data_ptr(), self.value_scales.data_ptr(),
                                      Kst.data_ptr(), Vst.data_ptr(), pos.data_ptr(), S, B, nkv, L, D, stream)
            if rc != 0:
                _lib.check(rc, "ll_kv8_load_bf16")
        else:
            p = int(pos)
            n = max(0, min(S, self.max_cache_len - p))        # rows past the last slot are dropped
            for codes, scales, new, st in ((self.keys, self.key_scales, key_states, Kst), (self.values, self.value_scales, value_states, Vst)):
                if n:
                    c, s = mx8_quantize_rows(new[:, :, :n])
                    codes[:, :, p:p + n], scales[:, :, p:p + n] = c, s
                st[:, :, :p + n] = mx8_dequantize(codes[:, :, :p + n], scales[:, :, :p + n]).to(st.dtype)
        if not cache.shared_counter:
            self.cumulative_length.add_(S)
        return Kst, Vst


class MX8StaticCache(StaticCache):
    """A static cache of ``MX8StaticLayer``s, allocated at construction for ``batch_size`` sequences of ``max_cache_len`` slots, with the one
    bf16 staging pair ``update`` returns (``dtype``: the model's dtype on the CPU; bf16 on the device, where the kernels write it)."""

    def __init__(self, config, batch_size: int, max_cache_len: int, device, dtype=torch.bfloat16):
        cfg = config.get_text_config(decoder=True)
        kinds = cache_layer_types(cfg)
        if any(k != "full_attention" for k in kinds):
            raise ValueError(f"MX8StaticCache serves full-attention layers only: kv_cache=\"mxfp8\" cannot be combined with a model whose "
                             f"config has layers of other kinds (sliding_window={getattr(cfg, 'sliding_window', None)!r}, layer types "
                             f"{sorted(set(kinds))}); use kv_cache=None for it")
        nkv = getattr(cfg, "num_key_value_heads", None) or cfg.num_attention_heads
        D = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
        if D not in HEAD_DIMS:
            raise ValueError(f"MX8StaticCache: head_dim={D} is not one of {HEAD_DIMS}")
        device = torch.device(device)
        if device.type == "cuda" and dtype != torch.bfloat16:
            raise ValueError("MX8StaticCache on the device needs a bf16 model")
        self.shared_counter = device.type == "cuda"
        self.head_dim = D
        layers = [MX8StaticLayer(self, max_cache_len, batch_size, nkv, D, device) for _ in range(cfg.num_hidden_layers)]
        Cache.__init__(self, layers=layers)
        self.staging = tuple(torch.zeros((batch_size, nkv, max_cache_len, D), dtype=dtype, device=device) for _ in range(2))

    def position_of(self, layer: MX8StaticLayer) -> torch.Tensor:
        return self.layers[0].cumulative_length if self.shared_counter else layer.cumulative_length

    def nbytes(self) -> int:
        """Bytes of the codes and scales of all layers (the staging pair is one bf16 layer on top)."""
        return sum(t.numel() for l in self.layers for t in (l.keys, l.values, l.key_scales, l.value_scales))
