"""Generate tests/golden/beam_penalty_tiny.pt by executing the REFERENCE ITSELF (the read-only checkout make_golden.py puts on
sys.path) on CPU: beam search WITH a repetition penalty, the ``--num_beam`` branch of omnilmm/omnilmm_gen_data.py:306-314
(``num_beams=, repetition_penalty=1.1``), on the tiny MHA and GQA configurations.

Run where the reference checkout exists (the build container; the GPU box has none):

    python tests/golden/make_beam_penalty_golden.py

What runs: the reference's ``LlavaLlamaForCausalLM`` and, per prompt, its own ``generate(inputs, images, image_sizes,
do_sample=False, num_beams=3, repetition_penalty=1.1, max_new_tokens=12, use_cache=True, output_scores=True, output_logits=True,
return_dict_in_generate=True, eos_token_id=E)``.  Prompts, runs "a" / "b", the recorded fields and the seed screening are
make_beam_golden.py's (imported, not copied), with tests/beam_penalty_case.py - the float64 restatement with HF's
RepetitionPenaltyLogitsProcessor between the log-softmax and the score add - in place of tests/beam_case.py.  The generator
validates the restatement against the reference's ``sequences``, ``beam_indices`` and ``sequences_scores`` (1e-5) and the recorded
logits against the CPU oracle behind the trace's beams (1e-4).

A seed for which the penalty changes nothing is not a fixture: for at least one prompt per configuration the running beams of run
"a" must differ from those of the reference's own search without the penalty (asserted; ``differs`` is stored per prompt; the
screening asks the same of the CPU oracle's restatements).

The fixture is data only, the size of beam_tiny.pt."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_beam_golden as MB  # noqa: E402  (sets up sys.path, the wandb stub and the reference imports)
from make_beam_golden import GAP_BAR, K, O, STD, STEPS, build_reference_model, make_case  # noqa: E402
import beam_case as BC  # noqa: E402
import beam_penalty_case as PC  # noqa: E402

PENALTY = 1.1
SEEDS = {"mha": range(1000, 1030), "gqa": range(1000, 1030)}


class Oracle(MB.Oracle):
    def search(self, k, eos, penalty=PENALTY):
        return PC.beam_search64(lambda j, beams: np.stack([self.logits(k, b) for b in beams]), K, STEPS, eos, penalty=penalty)


def _beams(steps):
    return [sorted(zip(st["parent"].tolist(), st["token"].tolist())) for st in steps]


def screen(cfg, seed):
    """make_beam_golden.screen under the penalty, plus: the penalty must change the running beams of some prompt of run a"""
    W = O.make_weights(cfg, seed=seed, std=STD)
    pixels, prompts = make_case(cfg, seed)
    orc = Oracle(cfg, W, pixels, prompts)
    runs_a = [orc.search(k, 2) for k in range(len(prompts))]
    if any(2 in st["cand_tok"][:2 * K].tolist() for _, steps in runs_a for st in steps):
        return None
    if not any(_beams(orc.search(k, 2, penalty=1.0)[1]) != _beams(runs_a[k][1]) for k in range(len(prompts))):
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
                         do_sample=False, num_beams=K, repetition_penalty=PENALTY, max_new_tokens=STEPS, use_cache=True,
                         output_scores=True, output_logits=True, return_dict_in_generate=True, eos_token_id=eos, pad_token_id=0)
    assert type(out).__name__ == "GenerateBeamDecoderOnlyOutput", type(out).__name__
    return dict(sequences=out.sequences[0].clone(), sequences_scores=out.sequences_scores[0].clone(),
                beam_indices=out.beam_indices[0].clone(), logits=torch.stack([l.float() for l in out.logits]))


def differs_from_the_plain_run(rec, model, cfg, pixels, prompt, k, eos):
    """True when the reference's own search WITHOUT the penalty (make_beam_golden.reference_run, restated by tests/beam_case.py on
    its recorded logits) runs other beams than the penalised one at some step"""
    plain = MB.reference_run(model, cfg, pixels, prompt, k, eos)
    lg = plain["logits"].numpy()
    _, steps = BC.beam_search64(lambda j, beams: lg[j], K, STEPS, eos)
    mine = [sorted(zip(p, t)) for p, t in zip(rec["parent"].tolist(), rec["token"].tolist())]
    return bool(_beams(steps) != mine)


def restate_and_validate(rec, orc, k, eos):
    """make_beam_golden.restate_and_validate with the penalised restatement"""
    lg = rec["logits"].numpy()
    g, steps = PC.beam_search64(lambda j, beams: lg[j], K, STEPS, eos, penalty=PENALTY)
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
    out = dict(std=STD, steps=STEPS, num_beams=K, gap_bar=GAP_BAR, penalty=PENALTY)
    for name, cfg in (("mha", O.tiny_cfg()), ("gqa", O.tiny_gqa_cfg())):
        found = []
        for seed in SEEDS[name]:
            r = screen(cfg, seed)
            print(name, "seed", seed, r, flush=True)
            if r is not None:
                found.append((r[0], seed, r[1]))
        if not found:
            raise RuntimeError("no seed meets the conditions of run b and of the penalty")
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
                    recs[-1]["differs"] = differs_from_the_plain_run(recs[-1], model, cfg, pixels, p, k, eos)
            runs[run] = dict(eos=eos, prompts=recs)
            print(name, "run", run, "eos", eos, "answer lengths", [int(r["answer"].numel()) for r in recs], "steps",
                  [int(r["logits"].shape[0]) for r in recs], "scores", [round(float(r["sequences_scores"]), 4) for r in recs],
                  "smallest keep / drop margins", [round(float(r["margin_keep"].min()), 4) for r in recs],
                  "penalty changes the beams", [r["differs"] for r in recs])
        assert all(r["answer"].numel() == STEPS and r["logits"].shape[0] == STEPS for r in runs["a"]["prompts"])
        assert any(r["answer"].numel() < STEPS for r in runs["b"]["prompts"])
        assert any(r["logits"].shape[0] < STEPS for r in runs["b"]["prompts"])
        assert any(r["differs"] for r in runs["a"]["prompts"]), "the penalty changes no running beam: not a fixture"
        m = torch.cat([r["margin_keep"] for run in runs.values() for r in run["prompts"]])
        print(name, "seed", seed, "share of steps with margin > 2 GAP_BAR:", float((m > 2 * GAP_BAR).double().mean()), "(screened",
              share, ")")
        out[name] = dict(cfg=O.asdict(cfg), seed=seed, pixels=pixels, prompts=prompts, runs=runs)
    path = os.path.join(HERE, "beam_penalty_tiny.pt")
    torch.save(out, path)
    print("->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
