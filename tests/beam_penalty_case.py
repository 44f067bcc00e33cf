"""Shared CPU pieces of the tests of beam search WITH a repetition penalty (tests/test_beam_penalty_host.py,
tests/test_beam_topk_penalty_gpu.py, tests/test_beam_penalty_search_gpu.py, tests/test_omnilmm_generate_gpu.py; a plain helper
module like beam_case.py, on which it builds):

  * HF's ``RepetitionPenaltyLogitsProcessor`` where ``GenerationMixin._beam_search`` runs its logits processors - on
    log_softmax(logits), BEFORE the running beam's score is added - restated in float64: every distinct id of the beam's history that
    lies in [0, V) is penalised once, ``lp < 0 ? lp * penalty : lp / penalty`` (the processor gathers the scores at the ids, rescales
    and scatters them back, so a duplicate id writes the same value twice);
  * ``topk_candidates`` and ``Group64`` of beam_case.py with that processor between the two operations, the margins of a step
    taken from the penalised candidates;
  * the fp32 bound of a penalised value, from beam_case.logsoftmax_add_bound;
  * the case stored in tests/golden/beam_penalty_tiny.pt (make_beam_penalty_golden.py).

The history of a running beam is the list of tokens it has generated (generation from ``inputs_embeds`` starts from an empty id
tensor: no prompt id is penalised).  The penalty a kernel applies is the fp32 value of the Python float (HF multiplies an fp32
tensor by it), so comparisons with a device use ``f32(penalty)``."""
import os

import numpy as np
import torch

import beam_case as BC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beam_penalty_tiny.pt")
U32 = BC.U32


def load_case():
    return torch.load(GOLD, weights_only=True)


def f32(penalty):
    """the penalty as an fp32 kernel argument holds it"""
    return float(np.float32(penalty))


def distinct_ids(hist, V):
    """the ids of one history that count: distinct, inside [0, V)"""
    return sorted({int(t) for t in hist if 0 <= int(t) < V})


def hf_repetition_penalty(lp, hist, penalty):
    """float64 [V] -> a penalised copy: RepetitionPenaltyLogitsProcessor on one row"""
    out = np.array(lp, dtype=np.float64, copy=True)
    ids = distinct_ids(hist, out.shape[0])
    if ids:
        v = out[ids]
        out[ids] = np.where(v < 0, v * penalty, v / penalty)
    return out


def penalised_logprobs(logits, hists, penalty):
    """float64 [K, V]: the processor on log_softmax(logits[b]) with beam b's history ``hists[b]``"""
    lp = BC.log_softmax64(logits)
    return np.stack([hf_repetition_penalty(lp[b], hists[b], penalty) for b in range(lp.shape[0])])


def topk_candidates(logits, score, n, hists, penalty):
    """beam_case.topk_candidates with the processor between the log-softmax and the score add.  Returns (value [n + 1], parent
    [n + 1], token [n + 1]): entry n is the first DROPPED candidate (for margins)."""
    lp = penalised_logprobs(logits, hists, penalty) + np.asarray(score, dtype=np.float64)[:, None]
    K, V = lp.shape
    flat = lp.reshape(-1)
    order = np.lexsort((np.arange(flat.shape[0]), -flat))[:n + 1]
    return flat[order], order // V, order % V


def penalised_bound(logits, score, hists, penalty):
    """(value, E) float64 [rows, V] of the fp32 evaluation  round(round(lp * penalty) + score)  on the penalised ids and
    round(lp + score) on the others.  lp and its bound E0 are beam_case.logsoftmax_add_bound at score 0; a penalised id then
    carries E0 * penalty plus the product's rounding 2^-24 |lp * penalty|; the score add contributes 2^-24 |value| once more
    (on every id: the bound at score 0 counted the rounding of an add that changes nothing)."""
    lp, e0 = BC.logsoftmax_add_bound(logits, np.zeros(np.asarray(logits).shape[0]))
    v, e = lp.copy(), e0.copy()
    for r in range(lp.shape[0]):
        ids = distinct_ids(hists[r], lp.shape[1])
        if ids:
            pv = np.where(lp[r, ids] < 0, lp[r, ids] * penalty, lp[r, ids] / penalty)
            e[r, ids] = e0[r, ids] * penalty + U32 * np.abs(pv)
            v[r, ids] = pv
    v = v + np.asarray(score, dtype=np.float64)[:, None]
    return v, e + U32 * np.abs(v)


def step_margins(own, K, j, T, eos):
    """(margin, margin_keep) of beam_case.Group64.step from the n + 1 float64 candidates ``own`` of step j"""
    v64, t64 = own[0], own[2]
    n = 2 * K
    last = j + 1 >= T
    stop = lambda t: bool(last or (eos is not None and int(t) == eos))        # noqa: E731
    margin = float(np.min(v64[:-1] - v64[1:]))
    if last:
        return margin, float(v64[K - 1] - v64[K])
    go = [c for c in range(n + 1) if not stop(t64[c])]
    keep = float(v64[go[K - 1]] - v64[go[K]])
    if stop(t64[K - 1]) or stop(t64[K]):
        keep = min(keep, float(v64[K - 1] - v64[K]))
    return margin, keep


class Group64(BC.Group64):
    """beam_case.Group64 whose selection runs the processor over each running beam's own tokens; ``penalty`` 1.0 is the parent
    class.  With ``cand`` the bookkeeping alone runs (the parent's), as there."""

    def __init__(self, K, T, eos=None, length_penalty=1.0, penalty=1.0):
        super().__init__(K, T, eos, length_penalty)
        self.penalty = float(penalty)

    def candidates(self, logits):
        return topk_candidates(logits, self.run_score, 2 * self.K, self.tokens, self.penalty)

    def step(self, logits, cand=None):
        if logits is None:
            return super().step(None, cand)
        j = self.j
        own = self.candidates(logits)
        out = super().step(None, own if cand is None else cand)
        out["margin"], out["margin_keep"] = step_margins(own, self.K, j, self.T, self.eos)
        return out


def beam_search64(logits_fn, K, T, eos=None, length_penalty=1.0, penalty=1.0):
    """beam_case.beam_search64 with the penalty.  Returns (Group64, [step dicts])."""
    g = Group64(K, T, eos, length_penalty, penalty)
    steps = []
    for j in range(T):
        steps.append(g.step(np.asarray(logits_fn(j, g.tokens))))
        if g.done:
            break
    return g, steps
