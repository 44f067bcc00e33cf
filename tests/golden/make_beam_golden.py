"""Generate tests/golden/beam_tiny.pt by executing the REFERENCE ITSELF (the read-only checkout make_golden.py puts on sys.path) on
CPU: the beam search of the evaluation stage (muffin/eval/muffin_vqa.py, llava15_chair.py, chat.py: num_beams=3) on the tiny MHA
and GQA configurations.

Run where the reference checkout exists (the build container; the GPU box has none):

    python tests/golden/make_beam_golden.py

What runs: the reference's ``LlavaLlamaForCausalLM`` (built as in make_golden.py, weights from ``oracle.dpo_oracle.make_weights``)
and, per prompt (one prompt per call, as the evaluation scripts call it), its own ``generate(inputs, images, image_sizes,
do_sample=False, num_beams=3, max_new_tokens=12, use_cache=True, output_scores=True, output_logits=True,
return_dict_in_generate=True, eos_token_id=E)``, twice per configuration:

  run "a": E = 2, the Llama EOS id, which no candidate of any step carries (screened): no hypothesis finishes before step 12;
  run "b": E = an id the beams emit mid-way, chosen so that for at least one prompt the returned answer is shorter than 12 tokens
           and for at least one prompt the search stops before step 12.

Recorded per run and prompt: ``sequences``, ``sequences_scores``, ``beam_indices``, the per-step raw logits of the K running beams
(``out.logits``), and the per-step running-beam trace (parent, token, score, margin) - the trace comes from the float64
restatement tests/beam_case.py run on the RECORDED logits, and the generator validates it: the restatement must return the
reference's sequences, beam_indices and sequences_scores (1e-5), and step j + 1's recorded logits row b must equal the CPU oracle's
logits behind the trace's running beam b (prompt + its tokens) to 1e-4 - so the trace names the beams the reference really ran.

Seeds: the candidates SEEDS are screened with the CPU oracle alone (``oracle.dpo_oracle.llama_logits`` under the restatement) for
the largest share of steps, over both runs, whose keep / drop margin (tests/beam_case.py ``margin_keep``: the value of the last
kept running beam minus the first dropped candidate) exceeds 2 x ``GAP_BAR`` of make_generate_golden.py.  A beam step compares
the K-th and (K + 1)-th of K V values where a greedy step compares the best two, so no seed makes every step decidable; the
margins (keep / drop, the stricter order margin, and the finished-score margin) are stored per step and the tests skip what
they cannot decide.

The fixture is data only: pixels (bf16: the values are bf16-representable, the reference ran on their fp32 copies), prompts,
the weight recipe (seed, std) and the recorded results."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import O, build_reference_model  # noqa: E402  (sets up sys.path, the wandb stub and the reference imports)
import beam_case as BC  # noqa: E402

IMAGE_TOKEN_INDEX = -200
STD, STEPS, K, GAP_BAR = 0.04, 12, 3, 1.95e-2
SEEDS = {"mha": range(1000, 1030), "gqa": range(1000, 1030)}
TEXT = [(4, 2), (7, 5), (5, 11)]            # words in front of / behind the image: three prompts of different lengths


def make_case(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    pixels = torch.randn(len(TEXT), 3, cfg.image_size, cfg.image_size, generator=g).bfloat16()
    prompts = [torch.cat([torch.tensor([1]), torch.randint(3, cfg.vocab, (a,), generator=g), torch.tensor([IMAGE_TOKEN_INDEX]),
                          torch.randint(3, cfg.vocab, (b,), generator=g)]) for a, b in TEXT]
    return pixels, prompts


class Oracle:
    """next-token logits of the CPU oracle behind prompt k + tokens, fp32, no cache"""

    def __init__(self, cfg, W, pixels, prompts):
        self.cfg, self.W, self.prompts = cfg, W, prompts
        self.feats, self.emb_w = O.encode_images(pixels.float(), W, cfg), W["model.embed_tokens.weight"]
        self.memo = {}

    def logits(self, k, tokens):
        key = (k, tuple(tokens))
        if key not in self.memo:
            ids = torch.cat([self.prompts[k], torch.tensor(list(tokens), dtype=self.prompts[k].dtype)])
            with torch.no_grad():
                e = O.prepare_inputs_labels_for_multimodal(ids[None], torch.full_like(ids[None], -100), self.feats[k:k + 1],
                                                           self.emb_w, None)[0]
                self.memo[key] = O.llama_logits(e, self.W, self.cfg)[0, -1].float().numpy()
        return self.memo[key]

    def search(self, k, eos):
        return BC.beam_search64(lambda j, beams: np.stack([self.logits(k, b) for b in beams]), K, STEPS, eos)


def screen(cfg, seed):
    """(share of decidable steps over both runs, eos id of run b) from the CPU oracle, or None when the seed cannot serve"""
    W = O.make_weights(cfg, seed=seed, std=STD)
    pixels, prompts = make_case(cfg, seed)
    orc = Oracle(cfg, W, pixels, prompts)
    runs_a = [orc.search(k, 2) for k in range(len(prompts))]
    if any(2 in st["cand_tok"][:2 * K].tolist() for _, steps in runs_a for st in steps):
        return None
    emitted = sorted({int(t) for _, steps in runs_a for st in steps[2:STEPS - 2] for t in st["cand_tok"][:K]})
    best = None
    for eos in emitted:
        runs_b = [orc.search(k, eos) for k in range(len(prompts))]
        short = any(len(g.best()[0]) < STEPS for g, _ in runs_b)
        early = any(len(steps) < STEPS for _, steps in runs_b)
        if not (short and early):
            continue
        m = [st["margin_keep"] for _, steps in runs_a + runs_b for st in steps]
        share = float(np.mean(np.array(m) > 2 * GAP_BAR))
        if best is None or share > best[0]:
            best = (share, eos)
    return best


def reference_run(model, cfg, pixels, prompt, k, eos):
    out = model.generate(inputs=prompt[None], images=pixels[k:k + 1].float(), image_sizes=[(cfg.image_size, cfg.image_size)],
                         do_sample=False, num_beams=K, max_new_tokens=STEPS, use_cache=True, output_scores=True,
                         output_logits=True, return_dict_in_generate=True, eos_token_id=eos, pad_token_id=0)
    assert type(out).__name__ == "GenerateBeamDecoderOnlyOutput", type(out).__name__
    return dict(sequences=out.sequences[0].clone(), sequences_scores=out.sequences_scores[0].clone(),
                beam_indices=out.beam_indices[0].clone(), logits=torch.stack([l.float() for l in out.logits]))


def restate_and_validate(rec, orc, k, eos):
    """the trace of the restatement on the recorded logits; validated against the reference's outputs and the oracle"""
    lg = rec["logits"].numpy()
    g, steps = BC.beam_search64(lambda j, beams: lg[j], K, STEPS, eos)
    assert len(steps) == lg.shape[0], (len(steps), lg.shape)
    toks, score, bidx = g.best()
    seq = rec["sequences"].tolist()
    assert seq[:len(toks)] == toks and all(t in (0, eos) for t in seq[len(toks):]), (seq, toks)
    n = int((rec["beam_indices"] >= 0).sum())
    assert rec["beam_indices"][:n].tolist() == bidx, (rec["beam_indices"].tolist(), bidx)
    assert abs(float(rec["sequences_scores"]) - score) <= 1e-5, (float(rec["sequences_scores"]), score)
    beams = [[] for _ in range(K)]
    for j, st in enumerate(steps):
        if j > 0:
            for b in range(K):
                err = float(np.abs(orc.logits(k, beams[b]) - lg[j, b]).max())
                assert err <= 1e-4, (k, j, b, err)
        beams = [beams[int(p)] + [int(t)] for p, t in zip(st["parent"], st["token"])]
    rec["parent"] = torch.tensor(np.stack([st["parent"] for st in steps]), dtype=torch.int32)
    rec["token"] = torch.tensor(np.stack([st["token"] for st in steps]), dtype=torch.int32)
    rec["score"] = torch.tensor(np.stack([st["score"] for st in steps]), dtype=torch.float32)
    rec["margin"] = torch.tensor([st["margin"] for st in steps], dtype=torch.float64)
    rec["margin_keep"] = torch.tensor([st["margin_keep"] for st in steps], dtype=torch.float64)
    rec["margin_fin"] = torch.tensor([st["margin_fin"] for st in steps], dtype=torch.float64)
    rec["answer"] = torch.tensor(toks, dtype=torch.int64)
    rec["sequences"] = rec["sequences"][:max(len(toks), 1)].clone()
    return rec


def main():
    torch.set_num_threads(8)
    out = dict(std=STD, steps=STEPS, num_beams=K, gap_bar=GAP_BAR)
    for name, cfg in (("mha", O.tiny_cfg()), ("gqa", O.tiny_gqa_cfg())):
        found = []
        for seed in SEEDS[name]:
            r = screen(cfg, seed)
            print(name, "seed", seed, r, flush=True)
            if r is not None:
                found.append((r[0], seed, r[1]))
        if not found:
            raise RuntimeError("no seed meets the conditions of run b")
        share, seed, eos_b = max(found, key=lambda t: (t[0], -t[1]))
        torch.manual_seed(0)
        W = O.make_weights(cfg, seed=seed, std=STD)
        model = build_reference_model(cfg, {k: v.clone() for k, v in W.items()})
        model.eval()
        pixels, prompts = make_case(cfg, seed)
        orc = Oracle(cfg, W, pixels, prompts)
        runs = {}
        for run, eos in (("a", 2), ("b", eos_b)):
            recs = []
            with torch.no_grad():
                for k, p in enumerate(prompts):
                    recs.append(restate_and_validate(reference_run(model, cfg, pixels, p, k, eos), orc, k, eos))
            runs[run] = dict(eos=eos, prompts=recs)
            print(name, "run", run, "eos", eos, "answer lengths", [int(r["answer"].numel()) for r in recs], "steps",
                  [int(r["logits"].shape[0]) for r in recs], "scores", [round(float(r["sequences_scores"]), 4) for r in recs],
                  "smallest keep / drop margins", [round(float(r["margin_keep"].min()), 4) for r in recs])
        assert all(r["answer"].numel() == STEPS and r["logits"].shape[0] == STEPS for r in runs["a"]["prompts"])
        assert any(r["answer"].numel() < STEPS for r in runs["b"]["prompts"])
        assert any(r["logits"].shape[0] < STEPS for r in runs["b"]["prompts"])
        m = torch.cat([r["margin_keep"] for run in runs.values() for r in run["prompts"]])
        print(name, "seed", seed, "share of steps with margin > 2 GAP_BAR:", float((m > 2 * GAP_BAR).double().mean()), "(screened",
              share, ")")
        out[name] = dict(cfg=O.asdict(cfg), seed=seed, pixels=pixels, prompts=prompts, runs=runs)
    path = os.path.join(HERE, "beam_tiny.pt")
    torch.save(out, path)
    print("->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
