"""Prompt-lookup speculative decoding of one sequence, stated once in torch / Python: the specification of the HIP step
(csrc/llm_spec.hip: ll_spec_draft, ll_spec_verify_bf16) and what CPU models and ``sampler="torch"`` run.

HF reaches the same drafting rule through ``generate(prompt_lookup_num_tokens=k, max_matching_ngram_size=n)``
(transformers generation/candidate_generator.py, PromptLookupCandidateGenerator.get_candidates).  One step:

  * the history is the call's ``input_ids`` row as given (an ``inputs_embeds`` call starts from none), then every emitted token;
  * drafts d_1..: ngram sizes min(n, len - 1) down to 1, the LEFTMOST earlier occurrence of the history's last ngram that has a non-empty
    continuation, up to k tokens behind it (HF's ``max_length`` cut and EOS trimming are not needed: verification cuts at EOS, a draft is
    only a guess); draft slots without a draft hold the last emitted token -- a valid id, and if the model happens to emit it, it is
    accepted like any draft, which is correct because an accepted token is always the model's own;
  * the model forwards the S = k + 1 tokens [last emitted, d_1..d_k] at cache slots pos..pos+S-1, position ids posid+i, causal among
    themselves; logits row i gives x_i (argmax, lowest index on ties, or the sampler's draw at step value t + i);
  * a = the number of leading i < k with x_i == d_{i+1}; x_0..x_a are emitted, cut after the first EOS and at max_new_tokens (e emitted);
  * step, posid, pos advance by e; the last emitted token is the next input.  K/V rows written beyond the accepted prefix are stale: the
    next step overwrites them, and no query sees them before that because row s attends to slots <= pos + s only.
"""
from __future__ import annotations

import numbers
from typing import List, Optional, Sequence, Tuple

MIN_DRAFTS, MAX_DRAFTS = 2, 15          # S = k + 1 rows must lie in the 3..16 rows the fused query-token forward serves


def check_prompt_lookup(num_tokens, ngram_size) -> Optional[Tuple[int, int]]:
    """(k, n) of a request, or None when prompt lookup is off (``prompt_lookup_num_tokens`` absent, None or 0).  HF's option names and
    default (max_matching_ngram_size = 2)."""
    def is_int(v):
        return isinstance(v, numbers.Integral) and not isinstance(v, bool)
    if num_tokens is None or (is_int(num_tokens) and num_tokens == 0):
        if ngram_size is not None:
            raise ValueError("`max_matching_ngram_size` is given without `prompt_lookup_num_tokens`: it only applies to prompt-lookup decoding")
        return None
    if not is_int(num_tokens) or not MIN_DRAFTS <= num_tokens <= MAX_DRAFTS:
        raise ValueError(f"`prompt_lookup_num_tokens` has to be an integer in [{MIN_DRAFTS}, {MAX_DRAFTS}] (k + 1 rows of one forward), "
                         f"but is {num_tokens!r}")
    if ngram_size is None:
        ngram_size = 2
    if not is_int(ngram_size) or ngram_size < 1:
        raise ValueError(f"`max_matching_ngram_size` has to be a strictly positive integer, but is {ngram_size!r}")
    return int(num_tokens), int(ngram_size)


def draft(history: Sequence[int], k: int, n: int) -> List[int]:
    """The up to k draft tokens for ``history`` (may be empty)."""
    L = len(history)
    for ng in range(min(n, L - 1), 0, -1):
        tail = list(history[L - ng:])
        for idx in range(L - ng):                       # idx + ng < L: a non-empty continuation
            if list(history[idx:idx + ng]) == tail:
                return list(history[idx + ng:min(idx + ng + k, L)])
    return []


def draft_rows(history: Sequence[int], last: int, k: int, n: int) -> List[int]:
    """The S = k + 1 input tokens of a step: the last emitted token, the drafts, and the last emitted token in the slots without one."""
    d = draft(history, k, n)
    return [int(last)] + [int(t) for t in d] + [int(last)] * (k - len(d))


def accept(rows: Sequence[int], x: Sequence[int], eos: Sequence[int], room: int) -> Tuple[List[int], bool]:
    """(emitted tokens, stopped) of a step: ``rows`` the S forwarded tokens, ``x`` the tokens of the logits rows (at least as many as
    get looked at: x_i is only needed while every earlier draft was accepted), ``room`` >= 1 the tokens left to max_new_tokens."""
    out: List[int] = []
    k = len(rows) - 1
    for i in range(k + 1):
        t = int(x[i])
        out.append(t)
        if t in eos:
            return out, True
        if len(out) >= room or i >= k or int(rows[i + 1]) != t:
            break
    return out, False
