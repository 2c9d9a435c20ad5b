"""Beam search of the graphed decode: HF ``GenerationMixin._beam_search`` (transformers 5.15) restated over static buffers.

One step takes the logits of the B*nb running beams and updates a state that lives in ONE device buffer (layout below, shared
with ``ll_beam_step_bf16``, include/llamole_hip.h), so the step can sit inside the captured decode graph and needs no host
sync.  Per batch item (HF's names in brackets):
  * log_softmax of the f32 logits; under beam sample HF's Temperature / TopK / TopP warpers with ``min_tokens_to_keep = n_eos + 1``;
  * plus the running score [running_beam_scores], over all nb*V continuations: top K (greedy) or K draws without replacement
    from softmax (beam sample; here Gumbel-top-K, the same distribution), K = max(2, 1 + n_eos) * nb [beams_to_keep];
  * a candidate hits if its token is an EOS id or the step is the last one; the running beams are the top nb of
    score + hit * -1e9 [_get_running_beams_for_next_iteration];
  * hits among the first nb become hypotheses with score / gen_len ** length_penalty, merged with the old ones by top nb
    [_update_finished_beams]; the early-stop heuristic and the global stop follow [_check_early_stop_heuristic,
    _beam_search_has_unfinished_sequences].  A step after the global stop changes nothing.
Ties: a higher score first, at equal scores the lower flat index (beam * V + token) first (torch.topk leaves it open).
Instead of HF's running sequences the state records, per step, each running beam's token and parent; ``finalize`` walks the
parents back from the best hypothesis once per call.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

NEG = -1.0e9

# int32 / f32 segments of the state buffer, in this order, each padded to a multiple of 4 elements (16 bytes); R = B * nb rows,
# T = the history length (the static-cache length).  ll_beam_state_bytes computes the same layout.
# flags [B, 8]: (heuristic unsatisfied, all hypotheses finished, all K candidates hit) of an even step at 0..2, of an odd one at 4..6
# (the merge of one item reads every item's flags of the last step while writing its own), the step count at 3.
_SEGMENTS = (("run", "R"), ("hyp", "R"), ("fin", "R"), ("hyp_t", "R"), ("hyp_beam", "R"), ("hyp_tok", "R"), ("flags", "B8"),
             ("par", "R"), ("rtok", "RT"), ("rpar", "RT"), ("cand", "RK3"))
_FLOAT = ("run", "hyp")


def state_layout(B: int, nb: int, K: int, T: int):
    """{name: (offset in 4-byte words, count)} and the total size in bytes."""
    R = B * nb
    n = dict(R=R, B8=8 * B, RT=R * T, RK3=R * K * 3)
    out, off = {}, 0
    for name, kind in _SEGMENTS:
        cnt = n[kind]
        out[name] = (off, cnt)
        off += (cnt + 3) // 4 * 4
    return out, 4 * off


def beams_to_keep(nb: int, n_eos: int) -> int:
    return max(2, 1 + n_eos) * nb


@dataclass
class BeamParams:
    B: int
    nb: int
    K: int
    T: int
    max_new: int
    eos: torch.Tensor                 # [n_eos] long
    length_penalty: float
    early_stopping: object            # False, True or "never"
    do_sample: bool
    temperature: float
    top_k: int
    top_p: float

    @property
    def min_keep(self) -> int:
        """HF _get_logits_processor's min_tokens_to_keep under beam search."""
        return int(self.eos.numel()) + 1 if self.eos.numel() else 2

    def warpers(self):
        """HF's warpers under beam sample, in its order (none under greedy beam search)."""
        from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
        w = []
        if not self.do_sample:
            return w
        if self.temperature is not None and self.temperature != 1.0:
            w.append(TemperatureLogitsWarper(self.temperature))
        if self.top_k:
            w.append(TopKLogitsWarper(top_k=self.top_k, min_tokens_to_keep=self.min_keep))
        if self.top_p is not None and self.top_p < 1.0:
            w.append(TopPLogitsWarper(top_p=self.top_p, min_tokens_to_keep=self.min_keep))
        return w


class BeamState:
    """Views of one uint8 buffer in the layout above."""

    def __init__(self, buf: torch.Tensor, B: int, nb: int, K: int, T: int):
        self.buf, self.B, self.nb, self.K, self.T = buf, B, nb, K, T
        lay, nbytes = state_layout(B, nb, K, T)
        assert buf.numel() >= nbytes and buf.dtype == torch.uint8
        i32 = buf[:nbytes].view(torch.int32)
        f32 = buf[:nbytes].view(torch.float32)
        for name, (off, cnt) in lay.items():
            setattr(self, name, (f32 if name in _FLOAT else i32)[off:off + cnt])

    def reset(self):
        """HF's initial values: running scores [0, -1e9, ...], hypotheses at -1e9, heuristic unsatisfied, step 0."""
        B, nb = self.B, self.nb
        run = self.run.view(B, nb)
        run.zero_()
        run[:, 1:] = NEG
        self.hyp.fill_(NEG)
        self.fin.zero_()
        self.hyp_t.fill_(-1)
        self.hyp_beam.zero_()
        self.hyp_tok.zero_()
        f = self.flags.view(B, 8)
        f.zero_()
        f[:, 0] = 1
        self.par.copy_(torch.arange(B * nb, dtype=torch.int32, device=self.buf.device))

    def cur_flags(self) -> torch.Tensor:
        """[B, 3] flags of the last step (the set of its parity)."""
        f = self.flags.view(self.B, 8)
        odd = (f[:, 3:4] & 1) != 0
        return torch.where(odd, f[:, 4:7], f[:, 0:3])

    def stopped(self, early_stopping) -> torch.Tensor:
        """HF's ``not _beam_search_has_unfinished_sequences`` after the last step, over the whole batch (0-dim bool tensor)."""
        f = self.cur_flags()
        improvement = (f[:, 0] != 0).any()
        open_beam = ~((f[:, 1] != 0).all() & (early_stopping is True))
        valid = ~(f[:, 2] != 0).all()
        return ~(improvement & open_beam & valid)


def _topk_det(x: torch.Tensor, k: int) -> torch.Tensor:
    """Indices of the k largest along the last dim; equal values: the lower index first."""
    return torch.sort(x, dim=-1, descending=True, stable=True)[1][..., :k]


def beam_step_torch(logits: torch.Tensor, st: BeamState, t: int, p: BeamParams, generator=None) -> torch.Tensor:
    """One step on logits [B*nb, V] at generated position t (0-based).  Updates ``st`` in place (nothing once the search has
    stopped) and returns the next input tokens [B*nb] (long).  HF's f32 arithmetic, in its order."""
    B, nb, K = p.B, p.nb, p.K
    V = logits.shape[1]
    dev = logits.device
    stop = st.stopped(p.early_stopping)
    lp = torch.log_softmax(logits.float(), dim=-1)
    for w in p.warpers():
        lp = w(None, lp)
    run = st.run.view(B, nb)
    acc = (lp.view(B, nb, V) + run[:, :, None]).reshape(B, nb * V)
    if p.do_sample:
        # Gumbel-top-K: the K largest of acc - log(E), E ~ Exp(1), are K draws without replacement from softmax(acc)
        e = torch.empty(acc.shape, dtype=torch.float32, device=dev)
        e.exponential_(generator=generator)
        key = torch.where(torch.isfinite(acc), acc - torch.log(e), torch.full_like(acc, float("-inf")))
        idx = _topk_det(key, K)
    else:
        idx = _topk_det(acc, K)
    cacc = acc.gather(1, idx)                                        # [B, K] topk_log_probs
    beam = idx // V
    tok = idx % V
    hits = torch.isin(tok, p.eos.to(dev)) if p.eos.numel() else torch.zeros_like(tok, dtype=torch.bool)
    if t + 1 >= p.max_new:
        hits = torch.ones_like(hits)
    # running beams of the next step
    rs = cacc + hits.to(torch.float32) * NEG
    sel = _topk_det(rs, nb)
    new_run = rs.gather(1, sel)
    new_par = beam.gather(1, sel)
    new_tok = tok.gather(1, sel)
    # finished hypotheses
    fin = st.fin.view(B, nb) != 0
    flags = st.flags.view(B, 8)
    heur = st.cur_flags()[:, 0:1] != 0
    did = hits & (torch.arange(K, device=dev) < nb)[None, :]
    s = cacc / (float(t + 1) ** p.length_penalty)
    full = fin.all(dim=1, keepdim=True) & (p.early_stopping is True)
    s = s + full.to(torch.float32) * NEG
    s = s + (~heur).to(torch.float32) * NEG
    s = s + (~did) * NEG
    ms = torch.cat([st.hyp.view(B, nb), s], dim=1)
    msel = _topk_det(ms, nb)
    new_hyp = ms.gather(1, msel)
    is_new = msel >= nb
    kpos = (msel - nb).clamp_min(0)
    old = msel.clamp_max(nb - 1)
    new_fin = torch.where(is_new, did.gather(1, kpos), fin.gather(1, old))
    new_ht = torch.where(is_new, torch.full_like(msel, t), st.hyp_t.view(B, nb).long().gather(1, old))
    new_hb = torch.where(is_new, beam.gather(1, kpos), st.hyp_beam.view(B, nb).long().gather(1, old))
    new_hk = torch.where(is_new, tok.gather(1, kpos), st.hyp_tok.view(B, nb).long().gather(1, old))
    # early-stop heuristic with cur_len advanced
    bl = p.max_new if (p.early_stopping == "never" and p.length_penalty > 0.0) else t + 1
    bp = new_run[:, :1] / (bl ** p.length_penalty)
    worst = torch.where(new_fin, new_hyp.min(dim=1, keepdim=True)[0], torch.full_like(new_hyp, NEG))
    new_heur = heur & (bp > worst).any(dim=-1, keepdim=True)

    def put(dst, val):
        dst.copy_(torch.where(stop, dst, val.to(dst.dtype).reshape(dst.shape)))

    rtok = st.rtok.view(B, nb, st.T)
    rpar = st.rpar.view(B, nb, st.T)
    last = rtok[:, :, max(t - 1, 0)].reshape(-1).long()
    put(rtok[:, :, t], new_tok)
    put(rpar[:, :, t], new_par)
    ident = torch.arange(B * nb, dtype=torch.int32, device=dev)
    st.par.copy_(torch.where(stop, ident, (torch.arange(B, device=dev)[:, None] * nb + new_par).view(-1).int()))
    put(st.run, new_run)
    put(st.hyp, new_hyp)
    put(st.fin, new_fin)
    put(st.hyp_t, new_ht)
    put(st.hyp_beam, new_hb)
    put(st.hyp_tok, new_hk)
    nf = torch.stack([new_heur[:, 0].int(), new_fin.all(dim=1).int(), hits.all(dim=1).int()], dim=1)
    odd_next = ((flags[:, 3:4] + 1) & 1) != 0
    put(flags[:, 0:3], torch.where(odd_next, flags[:, 0:3], nf))
    put(flags[:, 4:7], torch.where(odd_next, nf, flags[:, 4:7]))
    put(flags[:, 3], flags[:, 3] + 1)
    return torch.where(stop, last, new_tok.reshape(-1))


def reorder_cache_torch(cache, par: torch.Tensor) -> None:
    """Permute the rows of every StaticCache layer by ``par`` [B*nb] (flat parent row), in place: a captured forward keeps reading
    the same tensors, and the on-device length counters (a fused cache's shared one included) are left alone."""
    idx = par.long()
    for layer in cache.layers:
        for name in ("keys", "values"):
            x = getattr(layer, name, None)
            if x is not None and x.numel():
                x.copy_(x.index_select(0, idx.to(x.device)))


def finalize(st: BeamState, fill: int) -> torch.Tensor:
    """Tokens of each item's best hypothesis [B, L], L = the longest of them, shorter ones padded with ``fill`` (HF's output
    without the prompt)."""
    B, nb, T = st.B, st.nb, st.T
    ht = st.hyp_t.view(B, nb)[:, 0].long().cpu()
    hb = st.hyp_beam.view(B, nb)[:, 0].long().cpu()
    hk = st.hyp_tok.view(B, nb)[:, 0].long().cpu()
    rtok = st.rtok.view(B, nb, T).long().cpu()
    rpar = st.rpar.view(B, nb, T).long().cpu()
    L = int((ht + 1).max()) if B else 0
    out = torch.full((B, L), fill, dtype=torch.long)
    rows = torch.arange(B)
    has = ht >= 0
    out[rows[has], ht[has]] = hk[has]
    j = hb.clone()
    for s in range(L - 2, -1, -1):                  # the hypothesis of step ht extends running beam hb of step ht - 1
        m = has & (s < ht)
        if bool(m.any()):
            out[rows[m], s] = rtok[rows[m], j[m], s]
            j[m] = rpar[rows[m], j[m], s]
    return out.to(st.buf.device)
