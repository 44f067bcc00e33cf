"""Beam search WITH a repetition penalty on the GPU (LlavaDPOModel.beam_search(repetition_penalty=1.1): rv_beam_topk_penalty in
the loop) on the tiny MHA and GQA configurations, against tests/golden/beam_penalty_tiny.pt: what the reference's own
``generate(do_sample=False, num_beams=3, repetition_penalty=1.1, max_new_tokens=12, ...)`` returned for three prompts, without
(run "a") and with (run "b") an EOS id that the beams emit.

The three tests of tests/test_beam_search_gpu.py, with that file's bars and allowances and tests/beam_penalty_case.py as the
float64 restatement:

  * Replayed beams: the device follows the fixture's running beams (``_forced``); every step's logits of every beam against the
    CPU oracle, at most 2 x the error of the existing NO-CACHE path on the same sequences (measured here, printed); against the
    reference's recorded logits 2 x that + 1e-4.  Step 0 is the prefill bit for bit.
  * Selection on the device's own logits: where float64 orders the 2K + 1 best PENALISED values by more than their fp32 bound
    (beam_penalty_case.penalised_bound) the device's candidates are float64's; the bookkeeping behind them is the restatement's
    on the device's own candidates at every step.  At most 10 % of the steps undecided.
  * Running beams against the reference, up to the first step whose recorded margin is at most 2 x the measured no-cache error.

And: ``repetition_penalty=1.0`` is the call without the keyword, key by key of the trace."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_case as BC  # noqa: E402
import beam_penalty_case as PC  # noqa: E402
from oracle import dpo_oracle as O  # noqa: E402

U32 = 2.0 ** -24
_STATE = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _beams_before(rec, K):
    """per recorded step j the K running beams' token lists BEFORE the step, and after the last one"""
    beams, out = [[] for _ in range(K)], []
    for j in range(rec["parent"].shape[0]):
        out.append(beams)
        beams = [beams[int(p)] + [int(t)] for p, t in zip(rec["parent"][j], rec["token"][j])]
    return out + [beams]


def _setup(name):
    """Model, case, and per run: the replayed (teacher-forced) search, the oracle and the no-cache prefills on the same sequences,
    and the free search - computed once, shared, never modified."""
    if name in _STATE:
        return _STATE[name]
    from rlaif_v_amd.model import LlavaConfig, LlavaDPOModel
    gold = PC.load_case()
    case = gold[name]
    cfg = O.tiny_cfg() if name == "mha" else O.tiny_gqa_cfg()
    assert O.asdict(cfg) == case["cfg"]
    W = O.make_weights(cfg, seed=case["seed"], std=gold["std"])
    model = LlavaDPOModel(LlavaConfig(**O.asdict(cfg)), with_optimizer=False)
    model.load_state_dict(W)
    prompts, pixels, T, K, pen = case["prompts"], case["pixels"].float(), gold["steps"], gold["num_beams"], gold["penalty"]
    G, V = len(prompts), cfg.vocab
    M = G * K
    feats, emb_w, memo = O.encode_images(pixels, W, cfg), W["model.embed_tokens.weight"], {}

    def oracle(k, toks):
        key = (k, tuple(toks))
        if key not in memo:
            ids = torch.cat([prompts[k], torch.tensor(list(toks), dtype=prompts[k].dtype)])
            with torch.no_grad():
                e = O.prepare_inputs_labels_for_multimodal(ids[None], torch.full_like(ids[None], -100), feats[k:k + 1], emb_w, None)[0]
                memo[key] = O.llama_logits(e, W, cfg)[0, -1].float()
        return memo[key]

    prefill3 = model._prefill(prompts, pixels)[:G, :V].cpu()
    runs = {}
    for run, r in case["runs"].items():
        recs, eos = r["prompts"], r["eos"]
        before = [_beams_before(rec, K) for rec in recs]
        n_k = [rec["parent"].shape[0] for rec in recs]
        fp = torch.arange(K, dtype=torch.int32).repeat(T, G)             # behind a prompt's last recorded step: stay, token 3
        ft, fs = torch.full((T, M), 3, dtype=torch.int32), torch.zeros(T, M)
        for k, rec in enumerate(recs):
            fp[:n_k[k], k * K:(k + 1) * K], ft[:n_k[k], k * K:(k + 1) * K] = rec["parent"], rec["token"]
            fs[:n_k[k], k * K:(k + 1) * K] = rec["score"]
        _, _, tr = model.beam_search(prompts, pixels, T, num_beams=K, eos_token_id=eos, return_trace=True, repetition_penalty=pen,
                                     _forced=(fp, ft, fs))
        forced = tr["logits"].cpu()                                         # [T, M, V]
        rows = [(j, k, b) for k in range(G) for j in range(n_k[k]) for b in range(K)]
        want = torch.stack([oracle(k, before[k][j][b]) for j, k, b in rows])
        got = torch.stack([forced[j, k * K + b] for j, k, b in rows])
        recorded = torch.stack([recs[k]["logits"][j, b] for j, k, b in rows])
        nocache = {}
        for j in range(max(n_k)):                                           # one no-cache prefill per step: every live beam's sequence
            live = [(k, b) for k in range(G) if j < n_k[k] for b in range(K)]
            ext = [torch.cat([prompts[k], torch.tensor(before[k][j][b], dtype=prompts[k].dtype)]) for k, b in live]
            out = model._prefill(ext, pixels[[k for k, _ in live]])[:len(live), :V].cpu()
            for i, (k, b) in enumerate(live):
                nocache[(j, k, b)] = out[i]
        nc = torch.stack([nocache[x] for x in rows])
        free = model.beam_search(prompts, pixels, T, num_beams=K, eos_token_id=eos, return_trace=True, repetition_penalty=pen)
        runs[run] = dict(eos=eos, recs=recs, n_k=n_k, rows=rows, want=want, got=got, recorded=recorded, nc=nc, forced=forced,
                         forced_trace={k: v.cpu() for k, v in tr.items()}, free=(free[0], free[1], {k: v.cpu() for k, v in free[2].items()}))
    _STATE[name] = dict(gold=gold, case=case, cfg=cfg, W=W, model=model, prompts=prompts, pixels=pixels, T=T, K=K, G=G, V=V, runs=runs,
                        prefill3=prefill3, pen=pen)
    return _STATE[name]


def _e_nc(st):
    return max(float((r["nc"] - r["want"]).abs().max()) for r in st["runs"].values())


@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_replayed_beams_logits_within_twice_the_no_cache_error(name):
    _need_gpu()
    st = _setup(name)
    K, G = st["K"], st["G"]
    for run, r in st["runs"].items():
        e_nc = float((r["nc"] - r["want"]).abs().max())
        e_c = float((r["got"] - r["want"]).abs().max())
        e_ref = float((r["got"] - r["recorded"]).abs().max())
        print(f"[{name} run {run}, penalty {st['pen']}] max |logit - oracle| over {r['want'].numel()} logits of {len(r['rows'])} (step, beam) "
              f"rows: no-cache prefill {e_nc:.4e}, beam search with the row table {e_c:.4e} (bar {2 * e_nc:.4e}); against the "
              f"reference's recorded logits {e_ref:.4e}")
        assert torch.isfinite(r["forced"]).all()
        assert e_nc > 0
        assert e_c <= 2 * e_nc
        assert e_ref <= 2 * e_nc + 1e-4                       # the oracle reproduces the reference to 1e-4
        for m in range(G * K):
            assert torch.equal(r["forced"][0, m], st["prefill3"][m // K])
        tr = r["forced_trace"]
        for k, rec in enumerate(r["recs"]):
            n = r["n_k"][k]
            assert torch.equal(tr["parent"][:n, k * K:(k + 1) * K], rec["parent"]) and torch.equal(tr["token"][:n, k * K:(k + 1) * K], rec["token"])


@pytest.mark.parametrize("run", ["a", "b"])
@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_selection_on_the_devices_own_logits(name, run):
    _need_gpu()
    st = _setup(name)
    K, G, T, pen = st["K"], st["G"], st["T"], PC.f32(st["pen"])
    r = st["runs"][run]
    tokens, scores, tr = r["free"]
    steps = tr["logits"].shape[0]
    n = 2 * K
    undecided = total = penalised = 0
    smallest = np.inf
    for g in range(G):
        ref = PC.Group64(K, T, r["eos"], penalty=pen)
        sl = slice(g * K, (g + 1) * K)
        lost = False
        total += steps
        for j in range(steps):
            lg = tr["logits"][j, sl].numpy()
            cand = (tr["cand_val"][j, g].double().numpy(), tr["cand_parent"][j, g].numpy(), tr["cand_tok"][j, g].numpy())
            # 1. the candidates: float64's wherever float64 orders the 2K + 1 best by more than the fp32 bound
            v64, e64 = PC.penalised_bound(lg, ref.run_score, ref.tokens, pen)
            fv, fe = v64.reshape(-1), e64.reshape(-1)
            order = np.lexsort((np.arange(fv.shape[0]), -fv))[:n + 1]
            gaps, need = fv[order][:-1] - fv[order][1:], fe[order][:-1] + fe[order][1:]
            penalised += sum(int(t) in ref.tokens[int(p)] for p, t in zip(order[:n] // st["V"], order[:n] % st["V"]))
            if j > 0 or K == 1:
                smallest = min(smallest, float(gaps.min()))
            if bool((gaps > need).all()):
                assert cand[1].tolist() == (order[:n] // st["V"]).tolist() and cand[2].tolist() == (order[:n] % st["V"]).tolist(), \
                    f"prompt {g} step {j}: the device's candidates are not float64's (smallest gap {gaps.min():.3e})"
                assert np.abs(cand[0] - fv[order][:n]).max() <= fe[order].max() + U32 * np.abs(fv[order][:n]).max()
            else:
                undecided += 1
            # 2. the bookkeeping on the device's own candidates
            was_done = ref.done
            s = ref.step(None, cand)
            if not was_done and not s["margin_fin"] > 4 * U32 * max(1.0, abs(s["hyp_scores"][-1]) if s["hyp_scores"] else 1.0):
                undecided += steps - j
                lost = True
                break
            what = f"prompt {g} step {j}"
            assert tr["parent"][j, sl].tolist() == s["parent"].tolist() and tr["token"][j, sl].tolist() == s["token"].tolist(), what
            assert np.allclose(tr["score"][j, sl].numpy(), s["score"], rtol=2 * U32, atol=0), what
            assert bool(tr["done"][j, g]) == s["done"] and int(tr["n_hyp"][j, g]) == len(ref.hyps), what
            dev_scores = sorted(tr["hyp_score"][j, g, :len(ref.hyps)].tolist(), reverse=True)
            assert np.allclose(dev_scores, s["hyp_scores"], rtol=4 * U32, atol=0), what
        if lost:
            continue
        assert ref.done, f"prompt {g}: the search ended although the restatement is not done"
        toks, score, _ = ref.best()
        assert tokens[g] == toks and abs(scores[g] - score) <= 4 * U32 * abs(score), f"prompt {g}: final answer / sequences_scores"
    if r["eos"] is not None and run == "b":
        assert steps <= T
    print(f"[{name} run {run}] selection: {total - undecided} of {total} steps decided by float64 (smallest gap among the 2K + 1 best "
          f"after step 0: {smallest:.3e}); {penalised} penalised candidates among the selected")
    assert undecided <= 0.1 * total


@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_running_beams_against_the_reference(name):
    _need_gpu()
    st = _setup(name)
    K, G, T = st["K"], st["G"], st["T"]
    thr = 2 * _e_nc(st)
    compared = total = answers = 0
    for run, r in st["runs"].items():
        tokens, scores, tr = r["free"]
        for g, rec in enumerate(r["recs"]):
            want = _beams_before(rec, K)[1:]
            beams = [[] for _ in range(K)]
            ok = True
            for j in range(rec["parent"].shape[0]):
                total += 1
                if j >= tr["parent"].shape[0]:
                    ok = False
                    continue
                beams = [beams[int(p)] + [int(t)] for p, t in zip(tr["parent"][j, g * K:(g + 1) * K], tr["token"][j, g * K:(g + 1) * K])]
                if not ok or not min(float(rec["margin_keep"][j]), float(rec["margin_fin"][j])) > thr:
                    ok = ok and sorted(beams) == sorted(want[j])           # an undecidable step that went the other way: the rest is skipped
                    continue
                compared += 1
                assert sorted(beams) == sorted(want[j]), \
                    f"run {run} prompt {g} step {j}: running beams {sorted(beams)}, the reference ran {sorted(want[j])} (margin {float(rec['margin_keep'][j]):.3e})"
            if ok and bool((torch.minimum(rec["margin_keep"], rec["margin_fin"]) > thr).all()):
                answers += 1
                assert tokens[g] == rec["answer"].tolist(), f"run {run} prompt {g}: the answer"
                assert abs(scores[g] - float(rec["sequences_scores"])) <= thr, f"run {run} prompt {g}: sequences_scores"
    print(f"[{name}] against the reference: {compared} of {total} steps compared (threshold 2 x no-cache error = {thr:.3e}), "
          f"{answers} of {2 * G} final answers compared")


@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_penalty_one_is_the_call_without_the_keyword(name):
    _need_gpu()
    st = _setup(name)
    model, K, T = st["model"], st["K"], st["T"]
    eos = st["runs"]["b"]["eos"]
    a = model.beam_search(st["prompts"], st["pixels"], T, num_beams=K, eos_token_id=eos, return_trace=True)
    b = model.beam_search(st["prompts"], st["pixels"], T, num_beams=K, eos_token_id=eos, return_trace=True, repetition_penalty=1.0)
    assert a[0] == b[0] and a[1] == b[1] and sorted(a[2]) == sorted(b[2])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    # ... and the penalty is not a no-op on this case: the penalised search runs other beams
    free = st["runs"]["b"]["free"][2]
    n = min(free["token"].shape[0], a[2]["token"].shape[0])
    assert not torch.equal(free["token"][:n], a[2]["token"][:n].cpu())
    with pytest.raises(ValueError, match="repetition_penalty"):
        model.beam_search(st["prompts"], st["pixels"], 2, num_beams=K, repetition_penalty=0.0)
