"""Shared pieces of the top-k sampler tests (tests/test_topk_host.py, tests/test_sample_topk_gpu.py,
tests/test_generate_topk_gpu.py; a plain helper module like generate_case.py and divide_case.py):

  * the float64 numpy restatement of HF's processor order WITH top-k - RepetitionPenaltyLogitsProcessor,
    TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper, softmax - which returns, next to the distribution, the two
    distances that say whether fp32 can decide the kept set: the top-p edge (as generate_case.sampler_probs64) and the relative
    gap between the k-th largest score and the next one below it;
  * transformers' own warpers on a float64 row, for the cross-check of that restatement;
  * the runners that call rv_sample_token[_topk] and rv_sample_token_wide[_topk] on tests/guarded.py windows;
  * the check of tokens and logp against the restatement."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import divide_case as DC  # noqa: E402
import generate_case as GC  # noqa: E402
from guarded import Guarded  # noqa: E402

U32 = DC.U32
U_LAST = DC.U_LAST
F32, I32 = torch.float32, torch.int32
GAP_MIN = 8.0 * 2.0 ** -23            # two scores closer than this (relatively) may change order when fp32 divides by T


# ------------------------------------------------------------------------------------------------ restatement
def sampler_probs64_topk(logits, temperature, top_p, top_k, seen_ids=None, penalty=1.0):
    """-> (p float64 [V], edge, gap).  p: the final distribution of one row (zeros outside the kept set).  Top-k as
    TopKLogitsWarper: with tau the k-th largest score, scores < tau are removed and EVERYTHING tied with tau stays; top_k 0 or
    >= V is off.  edge: min |cumulative - (1 - top_p)| over the decision points of top-p among the survivors (inf when top_p >= 1
    or one survivor).  gap: (tau - s) / max(|tau|, |s|) for s the largest score below tau - the k-th against the (k+1)-th when
    nothing is tied at tau (inf when top-k is off or nothing is dropped).  temperature 0: the distribution at temperature 1
    without top-k and top-p, as sampler_probs64."""
    x = GC.penalised(logits, seen_ids, penalty)
    if temperature == 0:
        temperature, top_p, top_k = 1.0, 1.0, 0
    x = x / float(np.float32(temperature))
    V = x.shape[0]
    keep = np.ones(V, dtype=bool)
    gap = np.inf
    if 0 < top_k < V:
        tau = np.sort(x)[V - top_k]
        keep = x >= tau
        if not keep.all():
            nxt = x[~keep].max()
            gap = float((tau - nxt) / max(abs(tau), abs(nxt), 1e-300))
    p = np.where(keep, np.exp(x - x.max()), 0.0)
    p /= p.sum()
    edge = np.inf
    if top_p < 1.0:
        ids = np.nonzero(keep)[0]
        order = ids[np.argsort(x[ids], kind="stable")]          # ascending, as TopPLogitsWarper sorts (-inf first: mass 0)
        cum = np.cumsum(p[order])
        thr = 1.0 - float(np.float32(top_p))
        remove = cum <= thr
        remove[-1] = False                                      # min_tokens_to_keep = 1
        edge = float(np.abs(cum[:-1] - thr).min()) if cum.shape[0] > 1 else np.inf
        kept = np.zeros(V, dtype=bool)
        kept[order] = ~remove
        p = np.where(kept, p, 0.0)
        p /= p.sum()
    return p, edge, gap


def hf_warped_probs_topk(logits, temperature, top_p, top_k):
    """softmax(TopP(TopK(Temperature(x)))) of the installed transformers' warpers on one float64 row (top_k 0: no TopK)"""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = torch.as_tensor(np.asarray(logits), dtype=torch.float64)[None]
    ids = torch.zeros(1, 1, dtype=torch.long)
    s = TemperatureLogitsWarper(float(np.float32(temperature)))(ids, s)
    if top_k > 0:
        s = TopKLogitsWarper(int(top_k))(ids, s)
    if top_p < 1.0:
        s = TopPLogitsWarper(float(np.float32(top_p)))(ids, s)
    return torch.softmax(s, -1)[0].numpy()


def tie_row(V, ids_top, ids_tied, seed, zero_tie=False):
    """fp32 [V] for T = 1 without penalty (the scores are the logits bit for bit): a background below -6, distinct values 0.05
    apart at ``ids_top`` and ONE value 0.3 below the last of them at every id of ``ids_tied`` - flat enough that with five top
    and four tied ids every kept token holds more than 8 % of the mass.  zero_tie: the tied value is 0 with alternating signs
    (+0.0, -0.0, ...) under top values 0.5 ... 0.3, else 2.2 under 2.7 ... 2.5."""
    g = np.random.default_rng(seed)
    row = (-6.0 - 3.0 * g.random(V)).astype(np.float32)
    top = (0.5 if zero_tie else 2.7) - 0.05 * np.arange(len(ids_top))
    row[list(ids_top)] = top.astype(np.float32)
    if zero_tie:
        row[list(ids_tied)] = np.asarray([0.0 if i % 2 == 0 else -0.0 for i in range(len(ids_tied))], dtype=np.float32)
    else:
        row[list(ids_tied)] = np.float32(top[-1] - 0.3)
    return row


# ------------------------------------------------------------------------------------------------ the kernels on guarded windows
def _seen_tensors(seens, n, dev):
    if seens is None:
        return None, None
    if not isinstance(seens[0], (list, tuple)):
        seens = [seens] * n
    si = torch.tensor([i for s in seens for i in s], dtype=I32, device=dev)
    so = torch.tensor(np.concatenate([[0], np.cumsum([len(s) for s in seens])]), dtype=I32, device=dev)
    return so, si


def run(dev, wide, rows, V, ldl, us, temperature, top_p, top_k, seens=None, penalty=1.0):
    """n = len(us) rows through rv_sample_token_topk (wide False) or rv_sample_token_wide_topk (True); top_k None: the BASE entry
    point of the family.  rows: fp32 [V] (every row the same logits) or [n][V].  The columns behind V, the rows around the
    window and the band around the workspace (exactly rv_sample_token_wide_workspace_floats(n, V) floats) are poisoned and
    checked; logits and u are unchanged, token and logp fully written.
    -> (token int64 [n], logp float64 [n], token tensor, logp tensor: the device values for bit comparisons)"""
    from rlaif_v_amd import hip
    n = len(us)
    rows = np.asarray(rows, dtype=np.float32)
    fill = torch.zeros(n, ldl)
    fill[:, :V] = torch.from_numpy(rows).reshape(-1, V)
    inner = torch.zeros(n, ldl, dtype=torch.bool)
    inner[:, V:] = True
    gl = Guarded(n, ldl, F32, dev, fill=fill, name="logits", inner=inner, guard_cols=0, guard_rows=4)
    assert gl.ld == ldl
    gu = Guarded(1, n, F32, dev, fill=torch.tensor(us, dtype=F32)[None], name="u", guard_rows=0)
    gt = Guarded(1, n, I32, dev, name="token", guard_rows=0)
    gp = Guarded(1, n, F32, dev, name="logp", guard_rows=0)
    so, si = _seen_tensors(seens, n, dev)
    head = (gl.view, gl.ld, n, V, so, si, float(penalty), float(temperature), float(top_p))
    k = () if top_k is None else (int(top_k),)
    if wide:
        need = int(hip.lib().lib.rv_sample_token_wide_workspace_floats(n, V))
        assert need > 0
        gws = Guarded(1, need, F32, dev, name="workspace", guard_rows=0)
        DC.call("rv_sample_token_wide" + ("_topk" if k else ""), *head, *k, gu.view, gt.view, gp.view, gws.view, need)
        gws.check()
    else:
        DC.call("rv_sample_token" + ("_topk" if k else ""), *head, *k, gu.view, gt.view, gp.view)
    gl.check(), gu.check()
    gt.check(written=True), gp.check(written=True)
    tok_t, logp_t = gt.view[0].clone(), gp.view[0].clone()
    return tok_t.cpu().numpy().astype(np.int64), logp_t.cpu().double().numpy(), tok_t, logp_t


def check(row, V, us, temperature, top_p, top_k, seen=None, penalty=1.0, max_undecidable=0.0, planted_from=2,
          need_gap=True):
    """the caps on the restatement (top-p edge > 4 bounds, top-k gap > 8 * 2^-23 unless ties are the point), then: every decidable
    token is the restatement's, every token is in the kept set, logp inside the fp32 evaluation bound.  -> (p, want, decidable)"""
    bound = V * U32
    p, edge, gap = sampler_probs64_topk(row, temperature, top_p, top_k, seen, penalty)
    assert edge > 4 * bound, f"the nucleus edge is {edge:.3e} from a tie (4 x bound = {4 * bound:.3e}): pick another row"
    if need_gap:
        assert gap > GAP_MIN, f"the k-th and (k+1)-th scores are {gap:.3e} apart (relative): pick another row"
    want, dist = GC.sampler_choice64(p, np.asarray(np.float32(us), dtype=np.float64))
    ok = dist > bound
    if max_undecidable == 0.0:
        assert ok[planted_from:].all(), "every planted interval middle is decidable by construction"
    else:
        assert 1.0 - ok.mean() <= max_undecidable, "the row leaves too many of the uniforms undecidable"
    return p, want, ok


def compare(row, p, want, ok, us, tok, logp, temperature, seen=None, penalty=1.0):
    assert (p[tok] > 0).all(), f"a token outside the kept set was drawn: {sorted(set(tok[p[tok] == 0].tolist()))[:8]}"
    bad = np.nonzero(ok & (tok != want))[0]
    assert bad.size == 0, f"{bad.size} draws differ from the restatement, first u = {us[bad[0]]!r}: {tok[bad[0]]} vs {want[bad[0]]}"
    eb = DC.logp_bound(row, p, temperature, seen, penalty)
    for t in np.unique(tok):
        err = np.abs(logp[tok == t] - np.log(p[t])).max()
        assert err <= eb(t), f"logp of token {t}: error {err:.3e} > bound {eb(t):.3e}"
