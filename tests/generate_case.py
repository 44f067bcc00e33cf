"""Shared CPU pieces of the candidate-generation tests (tests/test_generate_host.py, tests/test_decode_kernels_gpu.py,
tests/test_generate_gpu.py; a plain helper module like autocheck_case.py):

  * the float64 numpy restatement of rv_sample_token's distribution - HF's processor order (RepetitionPenaltyLogitsProcessor,
    TemperatureLogitsWarper, TopPLogitsWarper, softmax) - and of the kernel's own inverse-CDF draw in vocabulary-index order;
  * the case stored in tests/golden/generate_tiny.pt (make_generate_golden.py) and its oracle: ``oracle.dpo_oracle.llama_logits``
    re-run on prompt + tokens so far, fp32, no cache."""
import os

import numpy as np
import torch

from oracle import dpo_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_tiny.pt")
U32 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ sampler restatement
def penalised(logits, seen_ids, penalty):
    """RepetitionPenaltyLogitsProcessor on one row (float64): l / penalty if l > 0 else l * penalty at the seen ids."""
    x = np.asarray(logits, dtype=np.float64).copy()
    if seen_ids is not None and penalty != 1.0:
        ids = np.unique(np.asarray(seen_ids, dtype=np.int64))
        ids = ids[(ids >= 0) & (ids < x.shape[0])]
        x[ids] = np.where(x[ids] > 0, x[ids] / penalty, x[ids] * penalty)
    return x


def sampler_probs64(logits, temperature, top_p, seen_ids=None, penalty=1.0):
    """The final distribution of one row, float64 [V] (zeros outside the kept set), and the distance of the nucleus edge from a
    tie: min over the decision points |cumulative - (1 - top_p)| (inf when top_p >= 1).  temperature 0: the distribution at
    temperature 1 without top_p (what rv_sample_token's logp refers to for a greedy token)."""
    x = penalised(logits, seen_ids, penalty)
    if temperature == 0:
        temperature, top_p = 1.0, 1.0
    x = x / float(np.float32(temperature))
    p = np.exp(x - x.max())
    p /= p.sum()
    edge = np.inf
    if top_p < 1.0:
        order = np.argsort(x, kind="stable")                 # ascending, as TopPLogitsWarper sorts
        cum = np.cumsum(p[order])
        thr = 1.0 - float(np.float32(top_p))
        remove = cum <= thr
        remove[-1] = False                                   # min_tokens_to_keep = 1
        edge = float(np.abs(cum[:-1] - thr).min()) if cum.shape[0] > 1 else np.inf
        keep = np.zeros_like(remove)
        keep[order] = ~remove
        p = np.where(keep, p, 0.0)
        p /= p.sum()
    return p, edge


def sampler_choice64(p, u):
    """The kernel's draw restated: the first kept id whose running sum (vocabulary order) exceeds u; also the distance of u from
    the nearest CDF boundary.  p float64 [V], u float64 [n] -> (int64 [n], float64 [n])."""
    kept = np.nonzero(p > 0)[0]
    cdf = np.cumsum(p[kept])
    cdf[-1] = max(cdf[-1], 1.0)
    u = np.asarray(u, dtype=np.float64)
    j = np.searchsorted(cdf, u, side="right")
    j = np.minimum(j, kept.shape[0] - 1)
    inner = cdf[:-1]                                          # the boundaries a draw can fall on the wrong side of
    if inner.shape[0] == 0:
        dist = np.full(u.shape, np.inf)
    else:
        k = np.clip(np.searchsorted(inner, u), 0, inner.shape[0] - 1)
        dist = np.minimum(np.abs(inner[k] - u), np.abs(inner[np.maximum(k - 1, 0)] - u))
    return kept[j], dist


def hf_warped_probs(logits, temperature, top_p):
    """softmax of transformers' own TemperatureLogitsWarper + TopPLogitsWarper on one fp64 row (the installed transformers)."""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopPLogitsWarper
    s = torch.as_tensor(np.asarray(logits), dtype=torch.float64)[None]
    ids = torch.zeros(1, 1, dtype=torch.long)
    s = TemperatureLogitsWarper(float(np.float32(temperature)))(ids, s)
    if top_p < 1.0:
        s = TopPLogitsWarper(float(np.float32(top_p)))(ids, s)
    return torch.softmax(s, -1)[0].numpy()


def peaked_row(V, seed, scale=4.0):
    """fp32 logits whose mass sits on a few tokens: most CDF boundaries coincide to within the fp32 summation error, so nearly
    every planted uniform is decidable."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(V, generator=g) * scale).float().numpy()


# ------------------------------------------------------------------------------------------------ the generate fixture
def load_case():
    return torch.load(GOLD, weights_only=True)


def prompt_embeds(cfg, W, prompts, pixels, tokens=None):
    """Per prompt the stand-alone spliced input embeddings [1, L, d] (fp32) of prompt (+ the first n tokens of tokens[k])."""
    feats = O.encode_images(pixels, W, cfg)
    emb_w = W["model.embed_tokens.weight"]
    out = []
    for k, p in enumerate(prompts):
        ids = p if tokens is None else torch.cat([p, torch.as_tensor(tokens[k], dtype=p.dtype)])
        out.append(O.prepare_inputs_labels_for_multimodal(ids[None], torch.full_like(ids[None], -100), feats[k:k + 1], emb_w, None)[0])
    return out


def oracle_step_logits(cfg, W, prompts, pixels, tokens):
    """[n_prompts, T, V] fp32: entry [k, j] = the oracle's next-token logits behind prompt k + tokens[k][:j].  Under a causal mask
    that is position L_k - 1 + j of ONE no-cache forward over prompt k + tokens[k][:T - 1] - the same numbers as re-running the
    forward per step, T times cheaper."""
    T = len(tokens[0])
    embeds = prompt_embeds(cfg, W, prompts, pixels, [t[:T - 1] for t in tokens])
    rows = []
    with torch.no_grad():
        for e in embeds:
            lg = O.llama_logits(e, W, cfg)[0]
            rows.append(lg[lg.shape[0] - T:].float())
    return torch.stack(rows)
