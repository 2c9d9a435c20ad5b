"""Rotary-embedding scaling on the host side: the reference's ``rope_scaling: linear | dynamic`` YAML key (hparams/model_args.py:128, applied by
model_utils/rope.py:34-62 with ``model_max_length = cutoff_len``, hparams/parser.py:303) restated for transformers' ``rope_parameters``, and
what the decode path needs to know about a model's rotary module: its type, the constructed state of a dynamic NTK module, and the frequency
table that the device-side prologue (ll_decode_prologue_dyn) selects from.  Nothing here needs a device or ``llm_accel``."""
from __future__ import annotations

import math
import warnings
from typing import Optional

import torch

ROPE_SCALING_CHOICES = ("linear", "dynamic")
# rotary types whose inv_freq / attention_scaling never change after construction: the one-launch prologue with other constants
STATIC_ROPE_TYPES = ("default", "linear", "llama3", "yarn")
# rotary types whose forward reads the position ids on the host (transformers dynamic_rope_update): not capturable as they are
HOST_READ_ROPE_TYPES = ("dynamic", "longrope")


def check_rope_scaling(v) -> Optional[str]:
    if v is None:
        return None
    if v not in ROPE_SCALING_CHOICES:
        raise ValueError(f"rope_scaling has to be one of 'linear' and 'dynamic', got {v!r}.")
    return v


def configure_rope(config, rope_scaling, model_max_length, is_trainable: bool = False) -> None:
    """Reference model_utils/rope.py:34-62 on ``config.rope_parameters`` (in place).  ``None`` does nothing; a config without rotary
    parameters gets a warning and stays as it is; ``model_max_length`` above ``max_position_embeddings`` raises that to it with
    factor = ceil(ratio), otherwise the factor is 1.0; without a ``model_max_length`` the factor is 2.0.  ``rope_theta`` and every other
    parameter the config already holds are kept."""
    rope_scaling = check_rope_scaling(rope_scaling)
    if rope_scaling is None:
        return
    if not hasattr(config, "rope_parameters"):
        warnings.warn("Current model does not support RoPE scaling.")
        return
    if model_max_length is not None:
        if is_trainable and rope_scaling == "dynamic":
            warnings.warn("Dynamic NTK scaling may not work well with fine-tuning. "
                          "See: https://github.com/huggingface/transformers/pull/24653")
        current = getattr(config, "max_position_embeddings", None)
        if current and model_max_length > current:
            config.max_position_embeddings = int(model_max_length)
            factor = float(math.ceil(model_max_length / current))
        else:
            warnings.warn("Input length is smaller than max length. Consider increase input length.")
            factor = 1.0
    else:
        factor = 2.0
    config.rope_parameters = dict(config.rope_parameters or {}, rope_type=rope_scaling, factor=factor)


def rotary_module(model):
    return getattr(getattr(model, "model", model), "rotary_emb", None)


def rope_type_of(model):
    """``rope_type`` of the model's rotary module: a string, a dict for modules with per-layer-type tables, None without a module."""
    rot = rotary_module(model)
    return None if rot is None else getattr(rot, "rope_type", "default")


def reset_dynamic_rope(model) -> bool:
    """Put a dynamic NTK rotary module back to its constructed state (``inv_freq = original_inv_freq``, ``max_seq_len_cached =
    original_max_seq_len``), so that the next eager forward depends on its own length only and not on earlier calls.  Returns whether the
    model has such a module."""
    rot = rotary_module(model)
    if rot is None or getattr(rot, "rope_type", None) != "dynamic" or not hasattr(rot, "original_inv_freq"):
        return False
    rot.inv_freq = rot.original_inv_freq
    rot.max_seq_len_cached = rot.original_max_seq_len
    rot.attention_scaling = 1.0
    return True


def dynamic_inv_freq(config, device, seq_len) -> torch.Tensor:
    """F(seq_len): transformers' own dynamic NTK init function (it clamps seq_len to max_position_embeddings from below)."""
    from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS
    return ROPE_INIT_FUNCTIONS["dynamic"](config, device, seq_len=seq_len)[0]


def dynamic_inv_freq_table(config, device, maxlen: int) -> Optional[torch.Tensor]:
    """Row j = F(max_position_embeddings + 1 + j) for every sequence length above ``max_position_embeddings`` that a cache of ``maxlen``
    slots can reach ([maxlen - max_position_embeddings, D/2] f32), None when there is none.  Each row is one call of transformers' function
    with the length as a 0-dim int64 tensor on ``device`` -- the form ``torch.max(position_ids) + 1`` has inside dynamic_rope_update -- so the
    values are the eager module's by construction."""
    max_pos = int(config.max_position_embeddings)
    if maxlen <= max_pos:
        return None
    lens = torch.arange(max_pos + 1, maxlen + 1, dtype=torch.long, device=device)
    return torch.stack([dynamic_inv_freq(config, device, lens[j]).to(torch.float32) for j in range(maxlen - max_pos)]).contiguous()
