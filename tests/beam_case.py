"""Shared CPU pieces of the beam-search tests (tests/test_beam_host.py, tests/test_beam_kernels_gpu.py,
tests/test_beam_search_gpu.py; a plain helper module like generate_case.py):

  * a float64 numpy restatement of transformers' ``GenerationMixin._beam_search`` (written from transformers 5.15.0,
    generation/utils.py: _get_top_k_continuations, _get_running_beams_for_next_iteration, _update_finished_beams,
    _check_early_stop_heuristic, _beam_search_has_unfinished_sequences) for what the reference's evaluation calls:
    ``generate(do_sample=False, num_beams=K, max_new_tokens=T)`` from ``inputs_embeds`` with ONE prompt per call,
    ``early_stopping=False``, at most one EOS id, no logits processor;
  * the case stored in tests/golden/beam_tiny.pt (make_beam_golden.py).

What that code does, per step j = 0 .. T - 1 (``cur_len`` = j: generation from inputs_embeds starts from an EMPTY id tensor, so the
prompt counts 0 tokens, ``max_length`` = T, and a hypothesis' "length" is its number of generated tokens, EOS included):

  b. log_probs = log_softmax(fp32 logits of the K running beams) + running score[beam]; running scores start at (0, -1e9, ...,
     -1e9), so step 0 sees beam 0 only;
  c. the 2K best of the K * V values (torch.topk; here equal values order by the lower flat index beam * V + token);
     parent = index // V, token = index % V;
  d. a candidate STOPS if its token is the EOS id or if j + 1 >= T (MaxLengthCriteria: at the last step every candidate stops);
  e. running beams: top-K of (value - 1e9 * stops): the K best candidates that do not stop, in order; their scores are these
     values (a stopped candidate that must fill a slot carries value - 1e9; only at the last step);
  f. finished set: the candidates of RANK < K that stop enter with score value / (j + 1) ** length_penalty; the set keeps the K
     best of old and new (top-K of the merged scores; free slots hold -1e9);
  g. stop rule: improvable = best running score / (j + 1) ** length_penalty > (min finished score if all K slots are finished
     else -1e9); the flag is sticky; the search ends when it is False or when every one of the 2K candidates stopped.
  At the end the best finished hypothesis is returned with its score (``sequences_scores``); ``beam_indices`` are the parents of
  its tokens.  (With one prompt per call nothing happens to a group after its search ended; ``rv_beam_step`` freezes the finished
  set of a done group, which is the same thing.)"""
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beam_tiny.pt")
DEAD = -1.0e9
U32 = 2.0 ** -24


def load_case():
    return torch.load(GOLD, weights_only=True)


def log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def logsoftmax_add_bound(logits, score):
    """(value, E) float64 numpy [rows, V]: ((x - max) - log Z) + score and the bound on |its fp32 evaluation - value|, derived the
    way tests/accuracy.py derives every bound - the kernel's formula written once with accuracy.Val, each operation adding its own
    term: x - max one rounding (the max is exact); expf 1 ulp (2 x 2^-24 relative) plus the propagated argument error; Z = a sum
    in which no term passes through more than 86 additions (64 in a thread, 6 butterfly steps, 16 wave results):
    86 x 2^-24 sum |terms|; logf FEW x 2^-24 |log Z| plus log(Z / (Z - e)); the subtraction and the add one rounding each."""
    import accuracy as A
    x = torch.as_tensor(np.asarray(logits, dtype=np.float64))
    d = A.Val(x) - x.max(-1, keepdim=True).values
    z = d.exp(fast=False).sum(-1, keepdim=True, depth=86)
    v = (d - z.log()) + torch.as_tensor(np.asarray(score, dtype=np.float64))[:, None]
    return v.v.numpy(), v.e.numpy()


def topk_candidates(logits, score, n):
    """float64: the n best of log_softmax(logits[b])[v] + score[b] over (b, v), by value descending then flat index ascending.
    Returns (value [n + 1], parent [n + 1], token [n + 1]): entry n is the first DROPPED candidate (for margins)."""
    lp = log_softmax64(logits) + np.asarray(score, dtype=np.float64)[:, None]
    K, V = lp.shape
    flat = lp.reshape(-1)
    order = np.lexsort((np.arange(flat.shape[0]), -flat))[:n + 1]
    return flat[order], order // V, order % V


class Group64:
    """The beam-search state of ONE prompt and its step, float64."""

    def __init__(self, K, T, eos=None, length_penalty=1.0):
        self.K, self.T, self.eos, self.lp = K, T, eos, float(length_penalty)
        self.run_score = np.array([0.0] + [DEAD] * (K - 1))
        self.tokens = [[] for _ in range(K)]           # running beams' tokens
        self.bidx = [[] for _ in range(K)]             # running beams' parent history (HF's beam_indices)
        self.hyps = []                                 # finished: dict(score, tokens, bidx), at most K, kept sorted descending
        self.done = False
        self.j = 0

    def step(self, logits, cand=None):
        """One step on the running beams' logits [K, V] (None with ``cand``: no margins).  ``cand`` = (value, parent, token)
        replaces the top-2K selection (the device's candidates, for testing the bookkeeping alone).  Returns a dict: the 2K candidates (+ the first dropped one),
        the new running beams, what entered the finished set, done, and three margins.  ``margin`` = the smallest gap between
        adjacent candidate values from rank 0 to the first dropped candidate: every decision of this step, the ORDER of the
        beams included, is decided when the values are known to better than margin / 2.  ``margin_keep`` = the keep / drop
        margin: the value of the last kept running beam minus the first dropped candidate that does not stop (and, where a
        stopping candidate sits at rank K - 1 or K, also the gap across that rank): the SET of running beams and of finished
        hypotheses is decided, not their order.  ``margin_fin``: the same for the two comparisons against finished scores
        (eviction, stop rule; inf when none was made)."""
        K, n, j = self.K, 2 * self.K, self.j
        own = topk_candidates(logits, self.run_score, n) if logits is not None else None
        val, par, tok = own if cand is None else (np.asarray(c) for c in cand)
        last = j + 1 >= self.T
        stop = lambda t: bool(last or (self.eos is not None and int(t) == self.eos))        # noqa: E731
        stops = [stop(tok[c]) for c in range(n)]
        div = float(j + 1) ** self.lp
        # e. running beams
        sel = [c for c in range(n) if not stops[c]][:K]
        filled = [(c, val[c]) for c in sel]
        for c in range(n):
            if len(filled) < K and stops[c]:
                filled.append((c, val[c] + DEAD))
        margin = margin_keep = np.inf                      # from the float64 candidates of the logits (n + 1 of them)
        if own is not None:
            v64, t64 = own[0], own[2]
            margin = float(np.min(v64[:-1] - v64[1:]))
            if last:
                margin_keep = float(v64[K - 1] - v64[K])
            else:
                go = [c for c in range(n + 1) if not stop(t64[c])]
                margin_keep = float(v64[go[K - 1]] - v64[go[K]])
                if stop(t64[K - 1]) or stop(t64[K]):      # a stopping candidate at the rank < K boundary of step f
                    margin_keep = min(margin_keep, float(v64[K - 1] - v64[K]))
        margin_fin = np.inf
        entered = []
        if not self.done:
            # f. finished set
            for c in range(K):
                if not stops[c]:
                    continue
                s = val[c] / div
                hyp = dict(score=float(s), tokens=self.tokens[int(par[c])] + [int(tok[c])], bidx=self.bidx[int(par[c])] + [int(par[c])],
                           step=j, rank=c)
                if len(self.hyps) == K:
                    margin_fin = min(margin_fin, abs(s - self.hyps[-1]["score"]))
                    if not s > self.hyps[-1]["score"]:
                        continue
                    self.hyps.pop()
                pos = len([h for h in self.hyps if h["score"] >= s])
                self.hyps.insert(pos, hyp)
                entered.append(hyp)
            # g. stop rule
            worst = self.hyps[-1]["score"] if len(self.hyps) == K else DEAD
            best = filled[0][1] / div
            if len(self.hyps) == K:
                margin_fin = min(margin_fin, abs(best - worst))
            self.done = bool(all(stops) or not best > worst)
        new_tokens = [self.tokens[int(par[c])] + [int(tok[c])] for c, _ in filled]
        new_bidx = [self.bidx[int(par[c])] + [int(par[c])] for c, _ in filled]
        self.tokens, self.bidx = new_tokens, new_bidx
        self.run_score = np.array([s for _, s in filled])
        self.j = j + 1
        return dict(cand_val=val, cand_parent=par, cand_tok=tok, parent=np.array([int(par[c]) for c, _ in filled]),
                    token=np.array([int(tok[c]) for c, _ in filled]), score=self.run_score.copy(), entered=entered,
                    done=self.done, margin=margin, margin_keep=margin_keep, margin_fin=float(margin_fin),
                    hyp_scores=[h["score"] for h in self.hyps])

    def best(self):
        """(tokens, sequences_scores, beam_indices) of the best finished hypothesis"""
        h = self.hyps[0]
        return h["tokens"], h["score"], h["bidx"]


def beam_search64(logits_fn, K, T, eos=None, length_penalty=1.0):
    """Runs one prompt.  ``logits_fn(j, beams)`` -> [K, V] logits behind the running beams' token lists ``beams`` at step j.
    Returns (Group64, [step dicts])."""
    g = Group64(K, T, eos, length_penalty)
    steps = []
    for j in range(T):
        steps.append(g.step(np.asarray(logits_fn(j, g.tokens))))
        if g.done:
            break
    return g, steps
