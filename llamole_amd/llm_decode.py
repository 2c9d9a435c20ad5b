"""HIP-graph autoregressive decode around an untouched HuggingFace causal LM.

Row f2 of SURVEY.md section 8 ("LLM-side hot loop"): the reference calls ``language_model.generate`` eagerly
(modeling_llamole.py:599, :849), i.e. ~10^3 small launches per token from Python.  On MI355X the decode step
of a 7-8 B model is launch-bound long before it is HBM-bound, so the step -- the stock HF ``forward`` over a
``StaticCache`` -- is captured ONCE as a hipGraph (``torch.cuda.CUDAGraph``; no tracing compiler, no Triton)
and replayed per token; sampling (temperature, top-p, multinomial) stays on the device -- on a HIP device with bf16
logits it is ONE launch (``ll_sample_token_bf16``) captured in the same graph together with the loop bookkeeping --
and the only host sync is an EOS check every ``sync_every`` tokens.  The LLM forward itself is HF code on
PyTorch-ROCm; ``llm_accel`` swaps HIP kernels in underneath its modules.

``GraphedDecoder.generate(input_ids, attention_mask, ...)`` returns prompt + new tokens like ``generate``
(rows that stopped are padded with ``pad_token_id``).  Greedy mode is token-identical to HF ``generate``.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import os

import torch


def check_repetition_penalty(p) -> Optional[float]:
    """HF generate's handling: None or 1.0 (an int 1 included) = off, no processor; anything else goes to RepetitionPenaltyLogitsProcessor,
    which takes a strictly positive Python float only (an int such as 2 raises ValueError, as it does there)."""
    if p is None or (not isinstance(p, (bool, str)) and isinstance(p, (int, float)) and p == 1.0):
        return None
    if not isinstance(p, float) or not (p > 0):
        raise ValueError(f"`penalty` has to be a strictly positive float, but is {p}")
    return float(p)


def apply_repetition_penalty(logits: torch.Tensor, ids: torch.Tensor, penalty: float) -> torch.Tensor:
    """HF RepetitionPenaltyLogitsProcessor on a float32 copy of ``logits`` [B,V]: every token of ``ids`` [B,L] (duplicates harmless)
    gets x < 0 ? x * penalty : x / penalty."""
    logits = logits.float().clone()
    if ids.shape[1] == 0:
        return logits
    s = torch.gather(logits, 1, ids)
    s = torch.where(s < 0, s * penalty, s / penalty)
    return logits.scatter_(1, ids, s)


def sample_top_p(logits: torch.Tensor, temperature: float, top_p: float, generator=None, top_k: Optional[int] = None,
                 repetition_penalty: Optional[float] = None, penalty_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """HF TemperatureLogitsWarper + TopKLogitsWarper + TopPLogitsWarper + multinomial, without host syncs.  logits [B,V] float.
    With ``repetition_penalty`` and ``penalty_ids`` [B,L], HF's RepetitionPenaltyLogitsProcessor runs first."""
    if repetition_penalty is not None and repetition_penalty != 1.0 and penalty_ids is not None:
        logits = apply_repetition_penalty(logits, penalty_ids, repetition_penalty)
    logits = logits.float()
    logits = torch.nan_to_num(logits, nan=0.0, posinf=torch.finfo(torch.float32).max, neginf=torch.finfo(torch.float32).min)
    if temperature is not None and temperature != 1.0:
        logits = logits / temperature
    if top_k is not None and 0 < top_k < logits.shape[-1]:
        kth = torch.topk(logits, top_k, dim=-1).values[..., -1:]
        logits = logits.masked_fill(logits < kth, float("-inf"))      # ties with the k-th value stay, as in HF
    if top_p is not None and top_p < 1.0:
        sorted_logits, sorted_idx = torch.sort(logits, descending=False)
        cum = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
        remove = cum <= (1 - top_p)
        remove[..., -1:] = False                      # keep at least one token
        remove = remove.scatter(1, sorted_idx, remove)
        logits = logits.masked_fill(remove, float("-inf"))
    probs = torch.softmax(logits, dim=-1)
    return torch.multinomial(probs, 1, generator=generator).squeeze(1)


def _reject_unsupported_generation_options(other: dict) -> None:
    """The decoder implements temperature, top_k, top_p, greedy, eos / pad handling.  Anything else HF ``generate`` would honour
    must be at its neutral value -- a silently dropped option would sample from another distribution than the reference."""
    bad = []
    for k, v in other.items():
        if v is None:
            continue
        if k == "repetition_penalty" and float(v) == 1.0:
            continue
        if k == "length_penalty" and float(v) == 1.0:
            continue
        if k == "num_beams" and int(v) == 1:
            continue
        if k == "logits_processor":
            # the reference passes get_logits_processor() = [InfNanRemoveLogitsProcessor] (extras/misc.py:146-152): the samplers
            # here sanitise inf / nan themselves; any other processor changes the distribution
            if all(type(p).__name__ == "InfNanRemoveLogitsProcessor" for p in v):
                continue
        if k in ("use_cache", "return_dict_in_generate", "output_scores", "output_hidden_states", "synced_gpus"):
            if not v or k == "use_cache":
                continue
        bad.append(k)
    if bad:
        raise NotImplementedError(f"GraphedDecoder.generate does not implement {sorted(bad)}: set them to their neutral values or "
                                  f"use the HF path (llm_decode='hf')")


def check_beam_options(num_beams, early_stopping):
    """HF GenerationConfig's validation of the beam options: num_beams a positive int, early_stopping one of False, True, "never"
    (None = HF's default False).  Returns (num_beams, early_stopping)."""
    import numbers
    if isinstance(num_beams, bool) or not isinstance(num_beams, numbers.Integral) or num_beams < 1:
        raise ValueError(f"`num_beams` has to be a strictly positive integer, but is {num_beams}")
    if early_stopping is None:
        early_stopping = False
    if not (early_stopping is True or early_stopping is False or early_stopping == "never"):
        raise ValueError(f"`early_stopping` must be a boolean or 'never', but is {early_stopping}.")
    return int(num_beams), early_stopping


MAX_HIP_VOCAB = 163840   # ll_sample_token_bf16 keeps a whole row of logits in one workgroup's registers
N_EOS_SLOTS = 32
# bounds of the HIP beam step (ll_beam_step_bf16): beams per item, K = max(2, 1 + n_eos) * nb continuations kept per item, nb * K
# (the item's merge sorts them in LDS), and the top-k of beam sample (its survivors are sorted in LDS); outside them the torch step
# runs, with the same results
MAX_HIP_BEAMS, MAX_HIP_BEAM_K, MAX_HIP_BEAM_NK, MAX_HIP_BEAM_TOPK = 16, 512, 4096, 512


class GraphedDecoder:
    def __init__(self, model, use_graph: bool = True, sync_every: int = 16, fused_cache: bool = False, sampler: str = "hip",
                 kv_cache: Optional[str] = None):
        self.model = model
        # None: transformers' bf16 StaticCache.  "mxfp8": kv_cache.MX8StaticCache -- FP8 E4M3 codes with one E8M0 scale per 32 elements of
        # head_dim, 0.516 of the bytes; the fused layers then run ll_decode_attn_rope_kv8 / ll_suffix_attn_rope_kv8, HF's modules a dequantised
        # staging pair.  Opt-in, never a default; the environment variable LLAMOLE_KV_CACHE is the A/B switch (like LLAMOLE_QUANT_BITS).
        from .kv_cache import check_kv_cache
        if kv_cache is None and os.environ.get("LLAMOLE_KV_CACHE"):
            kv_cache = os.environ["LLAMOLE_KV_CACHE"]
        self.kv_cache = check_kv_cache(kv_cache)
        self.use_graph = use_graph and next(model.parameters()).is_cuda
        self.sync_every = sync_every
        self.fused_cache = fused_cache    # one fused KV-append launch per layer (llm_accel.fuse_cache_update)
        # "hip": on a HIP device with bf16 logits the sampler (temperature / top-p / multinomial, or argmax) and the loop
        # bookkeeping are ONE launch inside the captured step (ll_sample_token_bf16); "torch": op-by-op PyTorch sampler
        self.sampler = sampler
        self.len_bucket = 64
        # the eager query-token forward over the decode's KV cache (continue_hidden: <= 16 new positions, so the attention is this
        # library's decode kernel and HF's mask is the explicit one either way) is host-bound -- 28 layers x ~20 Python-dispatched ops,
        # 7.4 ms of host time for 3.7 ms of kernels at Qwen2-7B: a (batch, length) shape seen a second time is captured as a hipGraph
        # and replayed from then on (LLAMOLE_GRAPH_SUFFIX=0: always eager).  The prompt prefill is NOT captured: transformers takes
        # other mask decisions while a stream is capturing (masking_utils.is_tracing), i.e. other SDPA kernels and roundings than the
        # eager prefill, and under the overlapped trajectory the prefill is device-bound anyway (HISTORY R5.8).
        self.graph_suffix = self.use_graph and os.environ.get("LLAMOLE_GRAPH_SUFFIX", "1") != "0"
        self.split_sampler = os.environ.get("LLAMOLE_SPLIT_SAMPLER", "1") != "0"     # top-k sampling as two launches (candidates, finish)
        self.sample_ws = None
        self.max_side_graphs = 4
        self._side_graphs = {}
        self._sample_key = None
        self._cache_fused = False
        self._key = None
        self._graph = None
        self._spec_graph = None         # prompt-lookup speculative step (_generate_spec): forward over k + 1 rows + verify + next draft
        self._spec_key = None
        self._spec_bufs = None
        self.spec_stats = None          # {"forwards", "accepted", "tokens"} of the last speculative generate
        self._eager_keys = set()        # (batch, cache length) shapes whose step is not captured (_warm_up)

    def _host_read_rope(self):
        """The model's rope type when its rotary module reads the position ids on the host (dynamic NTK, longrope: transformers
        dynamic_rope_update), else None.  Such a forward cannot be captured: the host read raises inside a capture, and a replay would keep
        the frequency tensor of the capture."""
        from .rope import HOST_READ_ROPE_TYPES, rope_type_of
        rope_type = rope_type_of(self.model)
        return rope_type if isinstance(rope_type, str) and rope_type in HOST_READ_ROPE_TYPES else None

    def _served_by_fused_prologue(self) -> bool:
        """Whether the last forward of the base model ran on the fused decode (llm_accel._model_forward), which picks a dynamic model's
        frequencies on the device and never calls HF's rotary module."""
        base = getattr(self.model, "model", self.model)
        return bool(base.__dict__.get("_ll_decode", {}).get("served"))

    def _graphs_off(self, rope_type: str, why: str):
        """For good: the reason (what is installed on the model, how this decoder was built) holds for every later call."""
        import warnings
        warnings.warn(f"rope_type={rope_type} reads the position ids on the host and {why}: this decoder runs eagerly (no hipGraph) "
                      "from now on")
        self.use_graph = self.graph_suffix = False
        self._graph = self._beam_graph = self._spec_graph = None
        self._side_graphs = {}

    def _graph_on(self) -> bool:
        """Whether the decode step of the current (batch, cache length) shape is replayed as a graph."""
        return self.use_graph and self._key not in self._eager_keys

    def _before_prefill(self):
        """A dynamic NTK module is put back to its constructed state before each prefill: a call's result then does not depend on the
        lengths of earlier calls, and prefill (HF's eager module) and decode (the fused prologue) agree.  A model whose rotary module reads
        the device on the host is captured only when the fused prologue serves its decode step; where that is known not to be the case
        before the first step -- the prologue is not installed, or this decoder does not use the fused cache append the prologue needs --
        the decoder turns its graphs off here, everything else is decided after the eager warm-up step (_warm_up)."""
        rope_type = self._host_read_rope()
        if rope_type is None:
            return
        from .rope import reset_dynamic_rope
        reset_dynamic_rope(self.model)
        base = getattr(self.model, "model", self.model)
        if (self.use_graph or self.graph_suffix) and ("_ll_decode" not in base.__dict__ or not self.fused_cache):
            self._graphs_off(rope_type, "the fused decode prologue is not installed" if "_ll_decode" not in base.__dict__
                             else "this decoder runs without the fused cache append that the fused prologue needs")

    def _warm_up(self, run=None):
        """The eager step on a side stream that precedes the capture of the decode step (its state is rewound; ``run``: another step's
        forward and rewind in place of the one-token step's).  For a rotary module that
        reads the device on the host this is also where the capture is decided: if the step was not served by the fused prologue (more
        rows than it takes, a layer that is not eligible at this shape, an embedding that is not bf16) HF's module ran, and the decoder
        runs this (batch, cache length) shape eagerly from then on (one warning per shape) instead of entering a capture with a host read
        inside; calls at shapes the prologue serves stay graphed."""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            if run is not None:
                run()
            else:
                self._step()
                # the warm-up advanced the cache's on-device length counters; rewind them so that the captured step (replayed for this same
                # token) writes the same slot again
                self._rewind(self.tok.shape[1])
        torch.cuda.current_stream().wait_stream(s)
        rope_type = self._host_read_rope()
        if rope_type is not None and not self._served_by_fused_prologue():
            import warnings
            warnings.warn(f"rope_type={rope_type} reads the position ids on the host and the fused decode prologue does not serve this "
                          f"model's step at {self.tok.shape[0]} rows: calls of this shape run eagerly (no hipGraph)")
            self._eager_keys.add(self._key)
            self._graph = self._beam_graph = self._spec_graph = None

    def _capture(self, attr: str, body) -> bool:
        """Capture ``body`` (the decode step and what follows it on the device) into a new graph stored as ``self.<attr>``.  A step that the
        installed transformers / torch cannot capture -- an op that is not permitted while a stream is capturing, e.g. the grouped GEMM of
        HF's experts code under a sparse-MoE model whose layers are not fused -- turns this (batch, cache length) shape eager, with one
        warning per shape, as a rotary module with a host read does; nothing of a failed capture has run on the device.  Only errors that
        name the capture are taken this way, and only when the step ran HF's own model forward: anything else is raised."""
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                body()
        except Exception as e:          # noqa: BLE001 -- narrowed below: only what a capture refuses, only under HF's own step
            # a step served by the fused prologue is all this library's launches and must capture: that failure is a bug and is raised, as is
            # any error that does not come from the capture itself
            if self._served_by_fused_prologue() or "captur" not in str(e).lower():
                raise
            import warnings
            why = (str(e).splitlines() or [""])[0]
            warnings.warn(f"hipGraph capture of the decode step failed ({type(e).__name__}: {why}); calls of this shape "
                          f"({self.tok.shape[0]} rows) run eagerly (no hipGraph)")
            self._eager_keys.add(self._key)
            self._graph = self._beam_graph = self._spec_graph = None
            torch.cuda.synchronize()
            return False
        setattr(self, attr, g)
        return True

    # static buffers + captured step for a (batch, max_len) shape
    def _prepare(self, B: int, max_len: int, device, use_embeds: bool):
        key = (B, max_len, use_embeds)
        if self._key == key:
            self.cache.reset()
            return
        self._key = key
        cfg = self.model.config
        if self.kv_cache == "mxfp8":
            from .kv_cache import MX8StaticCache
            on_device = torch.device(device).type == "cuda"
            self.cache = MX8StaticCache(cfg, B, max_len, device, torch.bfloat16 if on_device else next(self.model.parameters()).dtype)
        else:
            # (a config with sliding-window layers gets full-length layers: HF's sliding cache layer branches on the host, kv_cache.py)
            from .kv_cache import static_cache_for
            self.cache = static_cache_for(cfg, max_len)
        self.tok = torch.zeros(B, 1, dtype=torch.long, device=device)
        self.pos = torch.zeros(1, dtype=torch.long, device=device)
        self.mask = torch.zeros(B, max_len, dtype=torch.long, device=device)
        self.posid = torch.zeros(B, 1, dtype=torch.long, device=device)   # static: the captured graph reads it
        self.out_buf = torch.zeros(B, max_len, dtype=torch.long, device=device)
        self.done = torch.zeros(B, dtype=torch.uint8, device=device)
        self.stepc = torch.zeros(B, dtype=torch.long, device=device)
        self.seed_buf = torch.zeros(1, dtype=torch.long, device=device)
        self.eos_buf = torch.full((N_EOS_SLOTS,), -1, dtype=torch.long, device=device)
        self.logits = None
        self.sample_ws = None
        self.seen = None                # per-row set of seen tokens of the repetition penalty (ll_seen_set_*), allocated on first use
        self._beam_key = None           # beam search: state buffer (llm_beam.py) and the captured forward + beam step
        self._beam_graph = None
        self._graph = None
        self._spec_graph = None         # prompt lookup: the captured speculative step and its static buffers (_generate_spec)
        self._spec_key = None
        self._spec_bufs = None
        # an MX8 cache on the device follows the fused convention from its construction (every layer at layer 0's counter, advanced per forward)
        self._cache_fused = self.kv_cache is not None and self.cache.shared_counter
        self._side_graphs = {}          # captured against the buffers above

    def _captured(self, key, statics, fn):
        """``fn(*static buffers)`` eager the first time ``key`` is seen, captured the second time, replayed afterwards; ``statics`` are
        (static buffer factory, current value) pairs.  Returns fn's output (a tensor that the next replay overwrites).  A capture that
        fails (an op that synchronises) switches the shape back to eager for good."""
        values = [v for _, v in statics]
        st = self._side_graphs.get(key)
        if not self.graph_suffix or st == "eager":
            return fn(*values)
        if st is None:
            if len(self._side_graphs) >= self.max_side_graphs:      # shapes that do not repeat (A* expansion prompts) stay eager
                # evict a shape that was only SEEN, oldest first; captured graphs and "eager" tombstones stay (dropping a live graph means
                # a re-capture -- a device-wide synchronise inside the pipelined step -- and a forgotten tombstone retries a failed capture)
                victim = next((k for k, v in self._side_graphs.items() if v == "seen"), None)
                if victim is None:
                    return fn(*values)                              # table full of live graphs / tombstones: this shape runs eager
                self._side_graphs.pop(victim)
            self._side_graphs[key] = "seen"
            return fn(*values)
        if st == "seen":
            bufs = [mk(v) for (mk, _), v in zip(statics, values)]
            for b, v in zip(bufs, values):
                b.copy_(v)
            g = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    out = fn(*bufs)
            except Exception as e:          # noqa: BLE001 -- whatever the capture refuses: this shape runs eager from now on
                import warnings
                warnings.warn(f"hipGraph capture of the {key[0]} forward failed ({type(e).__name__}: {e}); it stays eager")
                self._side_graphs[key] = "eager"
                torch.cuda.synchronize()
                return fn(*values)
            st = self._side_graphs[key] = (g, bufs, out)
        g, bufs, out = st
        for b, v in zip(bufs, values):
            b.copy_(v)
        g.replay()
        return out

    def _step(self):
        out = self.model(input_ids=self.tok, attention_mask=self.mask, past_key_values=self.cache,
                         cache_position=self.pos, position_ids=self.posid, use_cache=True, return_dict=True)
        if self._cache_fused:   # the fused per-layer appends all used layer 0's counter; advance it once per forward
            self.cache.layers[0].cumulative_length.add_(self.tok.shape[1])
        return out.logits[:, -1, :]

    def _rewind(self, n: int):
        layers = self.cache.layers[:1] if self._cache_fused else self.cache.layers
        for layer in layers:
            layer.cumulative_length.sub_(n)

    @torch.no_grad()
    def continue_hidden(self, tail_ids: torch.Tensor, start: int) -> torch.Tensor:
        """Final hidden states of ``tail_ids`` [B,S] run ON TOP of the KV cache of the last ``generate`` call, at cache
        slots ``start .. start+S-1`` (slots >= start are overwritten).  This is the reference's query-token re-forward
        (modeling_llamole.py:641-646) without recomputing the prompt + analysis prefix."""
        info = self._last
        if info is None:
            raise RuntimeError("continue_hidden needs a preceding generate() on this decoder")
        if info.get("beams", 1) > 1:
            raise RuntimeError("continue_hidden after a beam search: the cache holds the running beams, not the returned sequences")
        B, S = tail_ids.shape
        P = info["P"]
        if start < P or start + S > self.mask.shape[1]:
            raise ValueError(f"continuation [{start},{start + S}) outside the cache window [{P},{self.mask.shape[1]})")
        for layer in self.cache.layers:
            layer.cumulative_length.fill_(start)
        device = tail_ids.device
        pos = torch.arange(start, start + S, device=device)
        posid = info["plen"] + (start - P) + torch.arange(S, device=device).unsqueeze(0)
        base = getattr(self.model, "model", self.model)

        def fwd(ids, cache_pos, pos_ids):
            return base(input_ids=ids, attention_mask=self.mask, past_key_values=self.cache, cache_position=cache_pos,
                        position_ids=pos_ids, use_cache=True, return_dict=True).last_hidden_state

        from .llm_accel import suffix_on_fused_layers
        fused = self._cache_fused and os.environ.get("LLAMOLE_FUSED_SUFFIX", "1") != "0" and suffix_on_fused_layers(self.model, True)
        key = ("suffix", B, S)
        try:
            hidden = self._captured(key, [(torch.empty_like, tail_ids), (torch.empty_like, pos), (torch.empty_like, posid)], fwd)
        finally:
            if fused:
                suffix_on_fused_layers(self.model, False)
        if self._side_graphs.get(key) == "seen" and self._host_read_rope() is not None and not self._served_by_fused_prologue():
            self._side_graphs[key] = "eager"        # the eager first call ran HF's rotary module (a host read): this shape is never captured
        if self._cache_fused:
            self.cache.layers[0].cumulative_length.add_(S)
        return hidden

    def _hip_sample(self, logits: torch.Tensor, sp, advance: int):
        """One launch: sample (or argmax) from bf16 logits [B,V], write tok / out_buf[:, step], update done / step and,
        with ``advance``, the position counters the next forward reads."""
        from . import _lib
        greedy, inv_temp, top_p, pad, top_k, penalty = sp
        B, V = logits.shape
        lib = _lib.load()
        if penalty != 1.0:
            rc = lib.ll_sample_token_penalty_bf16(logits.data_ptr(), logits.stride(0), B, V, inv_temp, top_p, int(top_k), int(greedy),
                                                  self.seed_buf.data_ptr(), self.eos_buf.data_ptr(), N_EOS_SLOTS, pad,
                                                  self.done.data_ptr(), self.tok.data_ptr(), self.out_buf.data_ptr(),
                                                  self.out_buf.stride(0), self.out_buf.shape[1], self.stepc.data_ptr(),
                                                  self.posid.data_ptr(), self.pos.data_ptr(), advance, self.seen.data_ptr(), self.seen.numel(),
                                                  self.seen_cap, penalty, torch.cuda.current_stream().cuda_stream)
            if rc != 0:
                _lib.check(rc, "ll_sample_token_penalty_bf16")
            return
        if self.sample_ws is None or self.sample_ws.device != logits.device:
            # workspace of the split top-k sampler (candidate lists; zero-filled once, the sampler leaves it clean): a static buffer of the graph
            self.sample_ws = torch.zeros(int(lib.ll_sample_workspace_bytes(B)), dtype=torch.uint8, device=logits.device)
        rc = lib.ll_sample_token_topk_ws_bf16(logits.data_ptr(), logits.stride(0), B, V, inv_temp, top_p, int(top_k), int(greedy),
                                              self.seed_buf.data_ptr(), self.eos_buf.data_ptr(), N_EOS_SLOTS, pad,
                                              self.done.data_ptr(), self.tok.data_ptr(), self.out_buf.data_ptr(),
                                              self.out_buf.stride(0), self.out_buf.shape[1], self.stepc.data_ptr(),
                                              self.posid.data_ptr(), self.pos.data_ptr(), advance, None,
                                              self.sample_ws.data_ptr() if self.split_sampler else None, self.sample_ws.numel(),
                                              torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _lib.check(rc, "ll_sample_token_topk_ws_bf16")

    def _generate_hip(self, logits, sp, P, plen, eos_list, max_new_tokens, generator, device, penalty_ids=None):
        """Decode loop with the fused sampler: per token the host only replays ONE graph (forward + sampler)."""
        if sp[5] != 1.0:
            # the repetition penalty's set of seen tokens: a static buffer of the captured step, reseeded here by one launch
            from . import _lib
            lib = _lib.load()
            B, V = logits.shape
            cap = self.out_buf.shape[1]             # the static-cache length >= prompt + new tokens
            if self.seen is None or self.seen_cap != cap or self.seen_V != V:
                self.seen = torch.empty(int(lib.ll_seen_set_bytes(B, V, cap)), dtype=torch.uint8, device=device)
                self.seen_cap, self.seen_V = cap, V
                self._graph = None
            ids = penalty_ids if penalty_ids is not None else torch.zeros(B, 0, dtype=torch.long, device=device)
            ids = ids.contiguous()
            rc = lib.ll_seen_set_init(self.seen.data_ptr(), self.seen.numel(), B, V, cap, ids.data_ptr() if ids.numel() else None,
                                      max(1, ids.shape[1]), ids.shape[1], torch.cuda.current_stream().cuda_stream)
            if rc != 0:
                _lib.check(rc, "ll_seen_set_init")
        self.done.zero_()
        self.stepc.zero_()
        self.out_buf.fill_(sp[3])
        self.eos_buf.fill_(-1)
        if eos_list:
            self.eos_buf[:len(eos_list)] = torch.tensor(eos_list, dtype=torch.long, device=device)
        gen_dev = generator.device.type if generator is not None else device.type
        self.seed_buf.copy_(torch.randint(0, 2 ** 62, (1,), device=gen_dev, generator=generator))
        self.posid.copy_(plen)
        self.pos.fill_(P)
        if self._sample_key != sp:          # sampler parameters are baked into the captured launch
            self._sample_key = sp
            self._graph = None
        self._hip_sample(logits, sp, 0)
        from ._trace import mark
        mark("generate: first token sampled")
        n = 1
        for t in range(1, max_new_tokens):
            if eos_list and t % self.sync_every == 0:
                if bool(self.done.all()):
                    break
                mark("generate: rendezvous")
            if self._graph_on() and self._graph is None:
                self._warm_up()                                   # the forward only, state rewound; may turn this shape's graph off
            if self._graph_on() and self._graph is None:
                def body():
                    self.logits = self._step()
                    self._hip_sample(self.logits, sp, 1)
                self._capture("_graph", body)                     # a step that cannot be captured turns this shape eager
            if self._graph_on():
                self._graph.replay()
                logits = self.logits
            else:
                logits = self._step()
                self._hip_sample(logits, sp, 1)
            n = t + 1
        self.last_logits = logits
        self._last["n_new"] = n
        return self.out_buf[:, :n].clone()

    # ------------------------------------------------------------------ prompt-lookup speculative decoding (llm_spec.py), one sequence
    def _spec_forward(self, ids, cache_pos, pos_ids):
        """Logits [S,V] of the S = k + 1 rows ``ids`` [1,S] at cache slots ``cache_pos``.  On a fused cache the query-token forward of the
        fused layers serves it (llm_accel._suffix_forward: five launches per layer, the slot read from layer 0's counter on the device);
        anywhere else -- a CPU model, layers=False, a declined layout -- HF's own forward runs the same rows."""
        from .llm_accel import suffix_on_fused_layers
        fused = self._cache_fused and suffix_on_fused_layers(self.model, True)
        try:
            out = self.model(input_ids=ids, attention_mask=self.mask, past_key_values=self.cache, cache_position=cache_pos,
                             position_ids=pos_ids, use_cache=True, return_dict=True)
        finally:
            if fused:
                suffix_on_fused_layers(self.model, False)
        return out.logits[0]

    def _spec_counters(self, pos):
        """Every cache layer's next-slot counter to ``pos`` (int, or the device counter).  Only an unfused cache needs it after a step: its
        layers each advanced by S, not by the accepted tokens (a fused cache has the one counter, which the verify launch sets)."""
        for layer in self.cache.layers:
            c = getattr(layer, "cumulative_length", None)
            if c is not None:
                c.fill_(pos) if isinstance(pos, int) else c.copy_(pos.reshape(c.shape))

    def _generate_spec_torch(self, logits, spec, do_sample, temperature, top_p, top_k, eos_list, P, plen, max_new_tokens, generator, device,
                             input_ids):
        """The step of llm_spec.py op by op, host-driven (CPU models, sampler="torch", logits the HIP sampler does not take).  Row i is only
        sampled while every earlier draft was accepted, so a generator advances once per emitted token, as in the plain torch loop."""
        from .llm_spec import accept, draft_rows
        k, n = spec
        S = k + 1
        eos_set = set(eos_list)

        def pick(row):
            return int(sample_top_p(row, temperature, top_p, generator, top_k)) if do_sample else int(row.argmax(dim=-1))
        if self._sample_key is not None:     # as in the torch-sampler loop of generate
            self._sample_key = None
            self._graph = None
        history = input_ids[0].tolist() if input_ids is not None else []
        out = [pick(logits[:1])]
        history.append(out[0])
        done = out[0] in eos_set
        pos, posid, forwards, accepted = P, int(plen[0, 0]), 0, 0
        ar = torch.arange(S, device=device)
        while not done and len(out) < max_new_tokens:
            rows = draft_rows(history, out[-1], k, n)
            self._spec_counters(pos)
            logits = self._spec_forward(torch.tensor([rows], dtype=torch.long, device=device), pos + ar, (posid + ar).unsqueeze(0))
            x = []
            for i in range(S):
                x.append(pick(logits[i:i + 1]))
                if i >= k or x[i] != rows[i + 1] or x[i] in eos_set:
                    break
            emitted, done = accept(rows, x, eos_set, max_new_tokens - len(out))
            out += emitted
            history += emitted
            pos += len(emitted)
            posid += len(emitted)
            forwards += 1
            accepted += len(emitted) - 1
        self._spec_counters(pos)
        self.last_logits = logits
        self._last["n_new"] = len(out)
        self.spec_stats = {"forwards": forwards, "accepted": accepted, "tokens": len(out)}
        return torch.tensor([out], dtype=torch.long, device=device)

    def _generate_spec(self, logits, spec, sp, P, plen, eos_list, max_new_tokens, generator, device, input_ids):
        """Decode loop of prompt-lookup decoding with the HIP step: per forward the host replays ONE graph = the model on the k + 1 static
        rows, ll_spec_verify_bf16 (sample every row, accept, emit, bookkeeping) and, as that entry's tail, the next step's draft.  The
        first token comes from the prefill logits through the plain sampler, the first draft from ll_spec_draft.  ``last_logits`` are the
        [S,V] logits of the last forward."""
        from . import _lib
        from ._trace import mark
        lib = _lib.load()
        k, n = spec
        S = k + 1
        V = logits.shape[1]
        cap = self.out_buf.shape[1]
        stream = lambda: torch.cuda.current_stream().cuda_stream      # noqa: E731
        if self._spec_bufs is None or self._spec_bufs["ids"].shape[1] != S:
            z = lambda *shape: torch.zeros(*shape, dtype=torch.long, device=device)      # noqa: E731
            # static buffers of the captured step: its input rows, the lookup history and its length, the sampled rows, counters
            self._spec_bufs = dict(ids=z(1, S), posids=z(1, S), cpos=z(S), hist=z(cap), hist_len=z(1), xs=z(16), stats=z(2), max_new=z(1))
            self._spec_graph = None
        b = self._spec_bufs
        self.done.zero_()
        self.stepc.zero_()
        self.out_buf.fill_(sp[3])
        self.eos_buf.fill_(-1)
        if eos_list:
            self.eos_buf[:len(eos_list)] = torch.tensor(eos_list, dtype=torch.long, device=device)
        gen_dev = generator.device.type if generator is not None else device.type
        self.seed_buf.copy_(torch.randint(0, 2 ** 62, (1,), device=gen_dev, generator=generator))
        self.posid.copy_(plen)
        self.pos.fill_(P)
        b["stats"].zero_()
        b["max_new"].fill_(max_new_tokens)
        if input_ids is not None:                   # the history starts from the call's input_ids row as given, or empty (inputs_embeds)
            b["hist"][:P] = input_ids[0]
        b["hist_len"].fill_(P if input_ids is not None else 0)
        self._hip_sample(logits, sp, 0)             # first token, from the prefill logits: step = 1
        rc = lib.ll_spec_draft(b["hist"].data_ptr(), cap, b["hist_len"].data_ptr(), self.tok.data_ptr(), 1, k, n, self.pos.data_ptr(),
                               self.posid.data_ptr(), b["ids"].data_ptr(), b["posids"].data_ptr(), b["cpos"].data_ptr(), stream())
        if rc != 0:
            _lib.check(rc, "ll_spec_draft")
        mark("generate: first token sampled")
        greedy, inv_temp, top_p, _, top_k, _ = sp

        def forward():
            return self._spec_forward(b["ids"], b["cpos"], b["posids"])

        def verify(lg):
            fused = self._cache_fused
            rc = lib.ll_spec_verify_bf16(lg.data_ptr(), lg.stride(0), S, V, inv_temp, top_p, int(top_k), int(greedy), self.seed_buf.data_ptr(),
                                         self.eos_buf.data_ptr(), N_EOS_SLOTS, self.done.data_ptr(), self.tok.data_ptr(),
                                         self.out_buf.data_ptr(), cap, b["max_new"].data_ptr(), self.stepc.data_ptr(), self.posid.data_ptr(),
                                         self.pos.data_ptr(), self.cache.layers[0].cumulative_length.data_ptr() if fused else None,
                                         b["ids"].data_ptr(), b["posids"].data_ptr(), b["cpos"].data_ptr(), b["hist"].data_ptr(), cap,
                                         b["hist_len"].data_ptr(), n, 1, b["stats"].data_ptr(), b["xs"].data_ptr(), stream())
            if rc != 0:
                _lib.check(rc, "ll_spec_verify_bf16")
            if not fused:
                self._spec_counters(self.pos)

        def warm():             # the forward only; an unfused cache's layers advanced by S (a fused cache's counter is not touched)
            forward()
            if not self._cache_fused:
                for layer in self.cache.layers:
                    layer.cumulative_length.sub_(S)

        def body():
            self.logits = forward()
            verify(self.logits)

        gkey = (k, n, sp, self._cache_fused)        # the captured launches hold these by value
        if self._spec_key != gkey:
            self._spec_key = gkey
            self._spec_graph = None
        left, until = max_new_tokens - 1, 0         # tokens still to emit as of the last host read; replays until the next one
        while left > 0:
            if until == 0:
                # at most every sync_every replays, and no later than the fewest replays that can finish the call (S tokens each):
                # a replay after the end changes nothing but costs a forward
                until = max(1, min(self.sync_every, -(-left // S)))
            if self._graph_on() and self._spec_graph is None:
                self._warm_up(warm)
            if self._graph_on() and self._spec_graph is None:
                self._capture("_spec_graph", body)
            if self._graph_on():
                self._spec_graph.replay()
                logits = self.logits
            else:
                logits = forward()
                verify(logits)
            until -= 1
            if until == 0:
                done, step = torch.stack([self.done[0].long(), self.stepc[0]]).tolist()       # one host read
                left = 0 if done else max_new_tokens - step
                mark("generate: rendezvous")
        step, forwards, accepted = torch.cat([self.stepc, b["stats"]]).tolist()
        self.last_logits = logits
        self._last["n_new"] = step
        self.spec_stats = {"forwards": forwards, "accepted": accepted, "tokens": step}
        return self.out_buf[:, :step].clone()

    @torch.no_grad()
    def generate(self, input_ids: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None,
                 inputs_embeds: Optional[torch.Tensor] = None, max_new_tokens: int = 128, do_sample: bool = True,
                 temperature: float = 1.0, top_p: float = 1.0, eos_token_id: Optional[Sequence[int]] = None,
                 pad_token_id: Optional[int] = None, generator=None, top_k: Optional[int] = None,
                 repetition_penalty: Optional[float] = None, num_beams: Optional[int] = None, length_penalty: Optional[float] = None,
                 early_stopping=None, prompt_lookup_num_tokens: Optional[int] = None, max_matching_ngram_size: Optional[int] = None,
                 **other) -> torch.Tensor:
        # HF RepetitionPenaltyLogitsProcessor: every token of the call's input_ids (prompt, pads included, then each generated token;
        # an inputs_embeds call starts from none) gets x < 0 ? x * p : x / p ahead of the sampling options below
        penalty = check_repetition_penalty(repetition_penalty)
        penalty = 1.0 if penalty is None else penalty
        # HF's prompt-lookup decoding (llm_spec.py): opt-in, one sequence; absent / None / 0 = the plain decode, not one launch changed
        from .llm_spec import check_prompt_lookup
        spec = check_prompt_lookup(prompt_lookup_num_tokens, max_matching_ngram_size)
        beams = num_beams is not None and (isinstance(num_beams, bool) or num_beams != 1)
        rows = (input_ids if input_ids is not None else inputs_embeds).shape[0]
        if spec is None and os.environ.get("LLAMOLE_PROMPT_LOOKUP") and rows == 1 and not beams and penalty == 1.0:
            # A/B switch (like LLAMOLE_KV_CACHE): every call that can take prompt lookup runs with k = its value, the default ngram size
            spec = check_prompt_lookup(int(os.environ["LLAMOLE_PROMPT_LOOKUP"]), None)
        if spec is not None:
            if rows != 1:
                raise ValueError(f"GraphedDecoder.generate: prompt_lookup_num_tokens needs a batch of 1 sequence, got {rows} (HF's assisted "
                                 "generation is batch-1 only as well)")
            if beams:
                raise NotImplementedError("GraphedDecoder.generate does not implement prompt_lookup_num_tokens together with num_beams > 1")
            if penalty != 1.0:
                raise NotImplementedError("GraphedDecoder.generate does not implement prompt_lookup_num_tokens together with "
                                          "repetition_penalty != 1 (the seen set of a row would depend on the accepted prefix)")
        if num_beams is not None and (isinstance(num_beams, bool) or num_beams != 1):
            nb, es = check_beam_options(num_beams, early_stopping)
            if self.kv_cache is not None:
                raise NotImplementedError(f"GraphedDecoder.generate does not implement num_beams > 1 together with kv_cache={self.kv_cache!r}: "
                                          "the beam KV reorder is bf16-only (use kv_cache=None for beam search)")
            if penalty != 1.0:
                raise NotImplementedError("GraphedDecoder.generate does not implement repetition_penalty together with num_beams > 1")
            _reject_unsupported_generation_options(other)
            return self._generate_beam(input_ids, attention_mask, inputs_embeds, max_new_tokens, bool(do_sample), temperature, top_p,
                                       eos_token_id, pad_token_id, generator, int(top_k) if top_k else 0, nb,
                                       1.0 if length_penalty is None else float(length_penalty), es)
        # no beam search: the beam options go through the same check as before (a non-neutral one raises there)
        for k, v in (("num_beams", num_beams), ("length_penalty", length_penalty), ("early_stopping", early_stopping)):
            if v is not None:
                other[k] = v
        _reject_unsupported_generation_options(other)
        from ._trace import mark
        mark("generate: enter")
        top_k = int(top_k) if top_k else 0
        from .llm_accel import refresh_weight_copies
        refresh_weight_copies(self.model)       # concatenated / converted weight copies follow their sources (in place)
        ref = input_ids if input_ids is not None else inputs_embeds
        B, P = ref.shape[0], ref.shape[1]
        self._before_prefill()
        device = ref.device
        if attention_mask is None:
            attention_mask = torch.ones(B, P, dtype=torch.long, device=device)
        # static-cache length rounded up to a bucket: prompts of slightly different lengths (A* expansion prompts, eval
        # batches) then share one cache allocation and ONE captured graph; unused tail slots stay masked by causality
        # (prompt lookup: k slots of slack -- the last step's rejected drafts write K/V past the last emitted token)
        max_len = -(-(P + max_new_tokens + (spec[0] if spec is not None else 0)) // self.len_bucket) * self.len_bucket
        self._prepare(B, max_len, device, inputs_embeds is not None)
        self._last = None
        eos = torch.tensor(list(eos_token_id) if isinstance(eos_token_id, (list, tuple)) else
                           ([] if eos_token_id is None else [eos_token_id]), dtype=torch.long, device=device)
        pad = pad_token_id if pad_token_id is not None else (int(eos[0]) if eos.numel() else 0)
        # ---- prefill (eager, one call)
        # 2-D key mask for the whole static cache: prompt padding as given, every future slot open (causality
        # -- cache_position inside the HF mask builder -- already hides the slots not written yet), so the mask
        # never changes between replays of the captured step.
        self.mask.fill_(1)
        self.mask[:, :P] = attention_mask
        plen = attention_mask.long().sum(dim=1, keepdim=True)            # valid prompt tokens per row (left padding)
        pos_ids = (attention_mask.long().cumsum(dim=1) - 1).clamp_min(0)
        kw = dict(inputs_embeds=inputs_embeds) if inputs_embeds is not None else dict(input_ids=input_ids)
        pre = dict(attention_mask=self.mask[:, :P], past_key_values=self.cache, cache_position=torch.arange(P, device=device),
                   position_ids=pos_ids, use_cache=True, return_dict=True, **kw)
        try:
            out = self.model(logits_to_keep=1, **pre)       # only the last position's logits are used
        except TypeError:                                   # a model class without that argument
            out = self.model(**pre)
        logits = out.logits[:, -1, :]
        mark("generate: prefill enqueued")
        for layer in self.cache.layers:          # the next free slot is P whichever update path the prefill took (a short
            if hasattr(layer, "cumulative_length"):   # prompt on a re-used cache goes through the fused append, which
                layer.cumulative_length.fill_(P)      # leaves advancing layer 0's shared counter to its caller)
        self._last = dict(P=P, plen=plen, max_new=max_new_tokens, from_ids=input_ids is not None)
        if self.fused_cache and not self._cache_fused and device.type == "cuda":
            from .llm_accel import fuse_cache_update
            self._cache_fused = fuse_cache_update(self.cache) > 0
        hip_sampler = (self.sampler == "hip" and logits.is_cuda and logits.dtype == torch.bfloat16 and logits.shape[1] % 8 == 0
                       and logits.shape[1] <= MAX_HIP_VOCAB and logits.stride(1) == 1 and eos.numel() <= N_EOS_SLOTS
                       and (not do_sample or (temperature or 1.0) > 0))
        if spec is not None and not hip_sampler:
            new_tokens = self._generate_spec_torch(logits, spec, do_sample, temperature, top_p, top_k, eos.tolist(), P, plen, max_new_tokens,
                                                   generator, device, input_ids)
            return torch.cat([input_ids, new_tokens], dim=1) if input_ids is not None else new_tokens
        if hip_sampler:
            import numpy as np
            temp = 1.0 if temperature is None else float(temperature)
            sp = (not do_sample, float(np.float32(1.0) / np.float32(temp)), 1.0 if top_p is None else float(top_p), int(pad), top_k,
                  float(np.float32(penalty)))
            if spec is not None:
                new_tokens = self._generate_spec(logits, spec, sp, P, plen, eos.tolist(), max_new_tokens, generator, device, input_ids)
                mark("generate: decode loop done")
                return torch.cat([input_ids, new_tokens], dim=1) if input_ids is not None else new_tokens
            new_tokens = self._generate_hip(logits, sp, P, plen, eos.tolist(), max_new_tokens, generator, device, input_ids)
            mark("generate: decode loop done")
            return torch.cat([input_ids, new_tokens], dim=1) if input_ids is not None else new_tokens
        if self._sample_key is not None:     # a graph captured with the fused sampler does not fit the torch-sampler loop
            self._sample_key = None
            self._graph = None
        new_tokens = torch.full((B, max_new_tokens), pad, dtype=torch.long, device=device)
        done = torch.zeros(B, dtype=torch.bool, device=device)
        self.posid.copy_(plen)                                           # position id of the next token, per row
        n_done_steps = 0
        seen = None
        if penalty != 1.0:
            seen = input_ids if input_ids is not None else torch.zeros(B, 0, dtype=torch.long, device=device)
        for t in range(max_new_tokens):
            if seen is not None:
                pl = apply_repetition_penalty(logits, seen, penalty)
                nxt = sample_top_p(pl, temperature, top_p, generator, top_k) if do_sample else pl.argmax(dim=-1)
            else:
                nxt = sample_top_p(logits, temperature, top_p, generator, top_k) if do_sample else logits.argmax(dim=-1)
            nxt = torch.where(done, torch.full_like(nxt, pad), nxt)
            new_tokens[:, t] = nxt
            if seen is not None:
                seen = torch.cat([seen, nxt.view(B, 1)], dim=1)
            if eos.numel():
                done = done | torch.isin(nxt, eos)
            n_done_steps = t + 1
            if t + 1 == max_new_tokens:
                break
            if eos.numel() and (t + 1) % self.sync_every == 0 and bool(done.all()):
                break
            # ---- one decode step at cache position P + t
            self.tok.copy_(nxt.view(B, 1))
            self.pos.fill_(P + t)
            if t > 0:
                self.posid.add_(1)
            if self._graph_on() and self._graph is None:
                self._warm_up()                                   # on a side stream, state rewound; may turn this shape's graph off
            if self._graph_on() and self._graph is None:
                # capture the forward once (thread-local capture: a RCCL watchdog thread polling events must not invalidate it)
                self._capture("_graph", lambda: setattr(self, "logits", self._step()))
            if self._graph_on():
                self._graph.replay()
                logits = self.logits
            else:
                logits = self._step()
        new_tokens = new_tokens[:, :n_done_steps]
        self._last["n_new"] = n_done_steps
        self.last_logits = logits
        if input_ids is not None:
            return torch.cat([input_ids, new_tokens], dim=1)
        return new_tokens

    # ------------------------------------------------------------------ beam search (num_beams > 1)
    def _beam_hip_ok(self, logits: torch.Tensor, p) -> bool:
        """The HIP beam step's bounds (ll_beam_step_bf16); elsewhere the torch step runs."""
        V = logits.shape[1]
        return (self.sampler == "hip" and logits.is_cuda and logits.dtype == torch.bfloat16 and V % 8 == 0 and V <= MAX_HIP_VOCAB
                and logits.stride(1) == 1 and logits.stride(0) % 8 == 0 and p.eos.numel() <= N_EOS_SLOTS and p.nb <= MAX_HIP_BEAMS
                and p.K <= MAX_HIP_BEAM_K and p.nb * p.K <= MAX_HIP_BEAM_NK
                and (not p.do_sample or ((p.temperature or 1.0) > 0 and 1 <= p.top_k and max(p.top_k, p.min_keep) <= MAX_HIP_BEAM_TOPK)))

    def _kv_table(self, B: int, nb: int):
        """Device table of the StaticCache K / V tensors ([B*nb, nkv, maxlen, D] bf16 each) for ll_beam_kv_reorder_bf16, or None outside
        the kernel's bounds (D % 8 == 0, nb * D <= 16384, tensors * B * nkv <= 65535)."""
        R = B * nb
        ts = []
        for layer in self.cache.layers:
            ts += [getattr(layer, "keys", None), getattr(layer, "values", None)]
        if not ts or any(x is None or not x.is_cuda or x.dtype != torch.bfloat16 or x.dim() != 4 or not x.is_contiguous()
                         or x.shape != ts[0].shape or x.shape[0] != R for x in ts):
            return None
        nkv, D = ts[0].shape[1], ts[0].shape[3]
        if D % 8 != 0 or nb * D > 16384 or len(ts) * B * nkv > 65535:
            return None
        ptrs = tuple(x.data_ptr() for x in ts)
        if getattr(self, "_kv_ptrs_key", None) != ptrs:
            self._kv_ptrs_key = ptrs
            self._kv_ptrs = torch.tensor(ptrs, dtype=torch.int64, device=ts[0].device)
        return self._kv_ptrs, len(ts), tuple(ts[0].shape)

    def _hip_beam(self, logits: torch.Tensor, p, advance: int, step0: bool):
        """Two launches of the beam step (candidates per row, then the merge per item) and one of the KV reorder.  Step 0: every row
        takes beam 0's slots [0, pos) (the prompt); later steps: slots [P, pos) of every layer follow the step's parents, with P read
        from the device counter ``beam_first`` (set per call: a captured step serves every prompt length of its bucket)."""
        import numpy as np
        from . import _lib
        lib = _lib.load()
        V = logits.shape[1]
        stream = torch.cuda.current_stream().cuda_stream
        es = 2 if p.early_stopping == "never" else int(p.early_stopping is True)
        temp = 1.0 if p.temperature is None else float(p.temperature)
        rc = lib.ll_beam_step_bf16(logits.data_ptr(), logits.stride(0), p.B, p.nb, V, p.K, p.T, self.beam_buf.data_ptr(), self.beam_buf.numel(),
                                   self.eos_buf.data_ptr(), int(p.eos.numel()), p.max_new, float(p.length_penalty), es, int(p.do_sample),
                                   float(np.float32(1.0) / np.float32(temp)), int(p.top_k), float(p.top_p), self.seed_buf.data_ptr(),
                                   self.tok.data_ptr(), self.posid.data_ptr(), self.pos.data_ptr(), advance, stream)
        if rc != 0:
            _lib.check(rc, "ll_beam_step_bf16")
        ptrs, n, (R, nkv, maxlen, D) = self._kv
        first = self.beam_first[1:] if step0 else self.beam_first[:1]
        rc = lib.ll_beam_kv_reorder_bf16(ptrs.data_ptr(), n, p.B, p.nb, nkv, maxlen, D, self._beam_state.par.data_ptr(), first.data_ptr(),
                                         int(step0), self.pos.data_ptr(), stream)
        if rc != 0:
            _lib.check(rc, "ll_beam_kv_reorder_bf16")

    def _generate_beam(self, input_ids, attention_mask, inputs_embeds, max_new_tokens, do_sample, temperature, top_p, eos_token_id,
                       pad_token_id, generator, top_k, nb, length_penalty, early_stopping):
        """HF beam search / beam sample (llm_beam.py) over the B prompts expanded to B*nb rows: per token one captured step = forward
        + beam step + KV reorder.  Returns the best hypothesis of each item, prompt first for an input_ids call (HF's output)."""
        from ._trace import mark
        from .llm_accel import refresh_weight_copies
        from .llm_beam import BeamParams, BeamState, beam_step_torch, beams_to_keep, finalize, reorder_cache_torch, state_layout
        mark("generate: enter")
        refresh_weight_copies(self.model)
        ref = input_ids if input_ids is not None else inputs_embeds
        B, P = ref.shape[0], ref.shape[1]
        self._before_prefill()
        device = ref.device
        if attention_mask is None:
            attention_mask = torch.ones(B, P, dtype=torch.long, device=device)
        R = B * nb

        def ex(x):
            return None if x is None else x.repeat_interleave(nb, dim=0)
        ids_x, mask_x, emb_x = ex(input_ids), ex(attention_mask), ex(inputs_embeds)
        max_len = -(-(P + max_new_tokens) // self.len_bucket) * self.len_bucket
        self._prepare(R, max_len, device, inputs_embeds is not None)
        self._last = None
        eos = torch.tensor(list(eos_token_id) if isinstance(eos_token_id, (list, tuple)) else
                           ([] if eos_token_id is None else [eos_token_id]), dtype=torch.long, device=device)
        pad = pad_token_id if pad_token_id is not None else (int(eos[0]) if eos.numel() else 0)
        fill = (int(pad) if pad else int(eos[0])) if eos.numel() else -1      # HF: pad_token_id or eos[0]
        # ---- prefill of all B*nb rows (HF's expanded input), then every row's prompt slots are made beam 0's by the step-0 reorder
        self.mask.fill_(1)
        self.mask[:, :P] = mask_x
        plen = mask_x.long().sum(dim=1, keepdim=True)
        pos_ids = (mask_x.long().cumsum(dim=1) - 1).clamp_min(0)
        kw = dict(inputs_embeds=emb_x) if emb_x is not None else dict(input_ids=ids_x)
        pre = dict(attention_mask=self.mask[:, :P], past_key_values=self.cache, cache_position=torch.arange(P, device=device),
                   position_ids=pos_ids, use_cache=True, return_dict=True, **kw)
        try:
            out = self.model(logits_to_keep=1, **pre)
        except TypeError:
            out = self.model(**pre)
        logits = out.logits[:, -1, :]
        mark("generate: prefill enqueued")
        for layer in self.cache.layers:
            if hasattr(layer, "cumulative_length"):
                layer.cumulative_length.fill_(P)
        # the cache ends up holding running beams, not the returned sequences: continue_hidden refuses after a beam call
        self._last = dict(P=P, plen=plen, max_new=max_new_tokens, from_ids=input_ids is not None, beams=nb)
        if self.fused_cache and not self._cache_fused and device.type == "cuda":
            from .llm_accel import fuse_cache_update
            self._cache_fused = fuse_cache_update(self.cache) > 0
        K = beams_to_keep(nb, eos.numel())
        p = BeamParams(B, nb, K, max_len, max_new_tokens, eos, length_penalty, early_stopping, do_sample, temperature, top_k,
                       1.0 if top_p is None else float(top_p))
        skey = (B, nb, K, max_len)
        if getattr(self, "_beam_key", None) != skey or self.beam_buf.device != device:
            self._beam_key = skey
            self.beam_buf = torch.zeros(state_layout(B, nb, K, max_len)[1], dtype=torch.uint8, device=device)
            self.beam_first = torch.zeros(2, dtype=torch.int64, device=device)    # [P of the call, 0]: first slot the reorder moves
            self._beam_graph = None
        st = self._beam_state = BeamState(self.beam_buf, B, nb, K, max_len)
        st.reset()
        self._kv = self._kv_table(B, nb) if self._beam_hip_ok(logits, p) else None
        hip = self._kv is not None
        self.posid.copy_(plen)
        self.pos.fill_(P)
        if hip:
            self.eos_buf.fill_(-1)
            if eos.numel():
                self.eos_buf[:eos.numel()] = eos
            gen_dev = generator.device.type if generator is not None else device.type
            self.seed_buf.copy_(torch.randint(0, 2 ** 62, (1,), device=gen_dev, generator=generator))
            self.beam_first[0] = P
            self._hip_beam(logits, p, 0, True)
        else:
            self.tok.copy_(beam_step_torch(logits, st, 0, p, generator).view(R, 1))
            reorder_cache_torch(self.cache, torch.arange(R, device=device) // nb * nb)
        # the captured launches hold these by value; the prompt length, EOS ids, seed and counters are device buffers set per call
        gkey = (("hip", nb, K, int(eos.numel()), max_new_tokens, length_penalty, early_stopping, do_sample, temperature, top_k, p.top_p)
                if hip else ("torch",))
        if getattr(self, "_beam_gkey", None) != gkey:
            self._beam_gkey = gkey
            self._beam_graph = None
        for t in range(1, max_new_tokens):
            if t % self.sync_every == 0:
                if bool(st.stopped(early_stopping)):
                    break
                mark("generate: rendezvous")
            if not hip:
                self.pos.fill_(P + t - 1)
                if t > 1:
                    self.posid.add_(1)
            if self._graph_on() and self._beam_graph is None:
                self._warm_up()                                   # the forward only, state rewound; may turn this shape's graph off
            if self._graph_on() and self._beam_graph is None:
                def body():
                    self._beam_logits = self._step()
                    if hip:
                        self._hip_beam(self._beam_logits, p, 1, False)
                self._capture("_beam_graph", body)
            if self._graph_on():
                self._beam_graph.replay()
                logits = self._beam_logits
            else:
                logits = self._step()
                if hip:
                    self._hip_beam(logits, p, 1, False)
            if not hip:
                self.tok.copy_(beam_step_torch(logits, st, t, p, generator).view(R, 1))
                reorder_cache_torch(self.cache, st.par)
        self.last_logits = logits
        new_tokens = finalize(st, fill)
        self._last["n_new"] = new_tokens.shape[1]
        mark("generate: decode loop done")
        return torch.cat([input_ids, new_tokens], dim=1) if input_ids is not None else new_tokens
