"""Yes / no feedback scoring on the GPU (LlavaDPOModel.forward_next_token_scores, rlaif_v_amd.autocheck.score_yesno).

Three images with 1, 4 and 7 questions of different lengths (tests/golden/autocheck_tiny.pt; the tiny MHA and GQA
configurations of the oracle).

Oracle: ``oracle.dpo_oracle.llama_logits`` per question on its stand-alone spliced sequence, fp32 on the CPU, log-softmax at
the last position, read at the four wanted ids.

Bar: the packed path's maximum |logp - oracle| is at most 2 x the ``packed=False`` path's maximum error against the same
oracle on the same questions - both are bf16 noise of the same stack in a different summation order (if the un-packed error
is 0: the packed precompute's per-token bar, ``atol=3e-2`` of tests/test_precompute_packed_gpu.py).  Both errors are printed
and recorded (bench_outputs/r10_autocheck.json or $RV_RECORD_DIR; the committed copy is profiles/r10_autocheck.json).

Discrimination, asserted on the ORACLE side with the measured bar: (a) under a wrong mask - a question also sees the tail
packed in front of it - every such question's four logp values move by at least 10 x the bar (the largest of the four moves;
autocheck_case.leaked_logits); (b) any two questions differ in their four logp values by at least 10 x the bar (the largest
of the four differences), so rows handed out in a wrong order cannot pass either.  The weight scale (make_weights(std=0.04))
and the prompts were chosen on the CPU oracle for that: with bf16 emulation of the same oracle standing in for the device
noise both ratios were >= 1.4 x the requirement for both configurations."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import autocheck_case as AC  # noqa: E402
from oracle import dpo_oracle as O  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECOMPUTE_PER_TOKEN_BAR = 3e-2


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _record(key, value):
    path = os.path.join(os.environ.get("RV_RECORD_DIR") or os.path.join(REPO, "bench_outputs"), "r10_autocheck.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    blob = {}
    if os.path.exists(path):
        try:
            blob = json.load(open(path))
        except ValueError:
            blob = {}
    blob.setdefault("parity", {})[key] = value
    json.dump(blob, open(path, "w"), indent=1)


_STATE = {}


def _setup(name):
    """Model, case, oracle and both device results of one configuration: computed once, shared, never modified."""
    if name not in _STATE:
        from rlaif_v_amd.model import LlavaConfig, LlavaDPOModel
        case = AC.load_case()
        cfg = O.tiny_cfg() if name == "mha" else O.tiny_gqa_cfg()
        W = O.make_weights(cfg, seed=case["seed"], std=case["std"])
        model = LlavaDPOModel(LlavaConfig(**O.asdict(cfg)), with_optimizer=False)
        model.load_state_dict(W)
        embeds = AC.question_embeds(cfg, W, case["prompts"], case["pixels"])
        logits = AC.oracle_logits(cfg, W, embeds)
        res = {p: [t.cpu() for t in model.forward_next_token_scores(case["prompts"], case["pixels"], case["want_ids"], packed=p)]
               for p in (False, True)}
        _STATE[name] = dict(case=case, cfg=cfg, W=W, model=model, embeds=embeds, logits=logits, res=res)
    return _STATE[name]


def _bar(st):
    want = st["case"]["want_ids"]
    ref = torch.log_softmax(st["logits"], -1)[:, want]
    e_un = float((st["res"][False][1] - ref).abs().max())
    e_pk = float((st["res"][True][1] - ref).abs().max())
    return e_un, e_pk, (2.0 * e_un if e_un > 0 else PRECOMPUTE_PER_TOKEN_BAR), ref


@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_packed_scores_within_twice_the_unpacked_error(name):
    _need_gpu()
    st = _setup(name)
    want = st["case"]["want_ids"]
    e_un, e_pk, bar, ref = _bar(st)
    print(f"[{name}] max |logp - oracle| at the four ids: packed=False {e_un:.4e}, packed=True {e_pk:.4e}, bar {bar:.4e}")
    _record(f"{name}_logp_err_unpacked", e_un)
    _record(f"{name}_logp_err_packed", e_pk)
    # ---- discrimination, on the oracle side
    leaked, idx = AC.leaked_logits(st["cfg"], st["W"], st["embeds"])
    move = (torch.log_softmax(leaked, -1)[:, want] - ref[idx]).abs().amax(1)
    diff = (ref[:, None] - ref[None]).abs().amax(-1)
    diff.fill_diagonal_(float("inf"))
    print(f"[{name}] oracle: smallest move under the wrong mask {float(move.min()):.4e}, smallest difference between two "
          f"questions {float(diff.min()):.4e}; required {10 * bar:.4e}")
    _record(f"{name}_oracle_min_move_wrong_mask", float(move.min()))
    _record(f"{name}_oracle_min_question_difference", float(diff.min()))
    assert float(move.min()) >= 10 * bar, "the case cannot tell a wrong mask from bf16 noise"
    assert float(diff.min()) >= 10 * bar, "the case cannot tell two questions apart"
    # ---- the bar
    assert e_pk <= bar
    for p in (False, True):
        probs, logp, argmax, lse = st["res"][p]
        assert torch.isfinite(logp).all() and torch.isfinite(lse).all()
        assert torch.equal(probs, torch.exp(logp)) or float((probs - torch.exp(logp)).abs().max()) <= 1e-6
        # greedy token = the oracle's wherever its top-two margin exceeds the bar
        top2 = torch.topk(st["logits"], 2, -1)
        sure = (top2.values[:, 0] - top2.values[:, 1]) > bar
        assert int(sure.sum()) > 0
        assert torch.equal(argmax.long()[sure], top2.indices[:, 0][sure])


def test_against_the_reference_generate_fixture():
    """The product against what the reference's own generate(max_new_tokens=1, output_scores=True) returned: same bar."""
    _need_gpu()
    st = _setup("mha")
    case = st["case"]
    _, _, bar, _ = _bar(st)
    ref = torch.log(case["probs"])
    for p in (False, True):
        probs, logp, argmax, _ = st["res"][p]
        err = float((logp - ref).abs().max())
        print(f"packed={p}: max |logp - reference generate| {err:.4e} (bar {bar:.4e})")
        _record(f"mha_logp_err_vs_reference_generate_packed_{p}", err)
        assert err <= bar
        top2 = torch.topk(case["logits_last"], 2, -1)
        sure = (top2.values[:, 0] - top2.values[:, 1]) > bar
        assert torch.equal(argmax.long()[sure], case["new_token"][sure])


@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_batch_independence_is_exact(name):
    """Image 2's questions alone or together with images 1 and 3: bit-equal outputs."""
    _need_gpu()
    st = _setup(name)
    case = st["case"]
    n0, n1 = len(case["prompts"][0]), len(case["prompts"][1])
    for p in (True, False):
        alone = st["model"].forward_next_token_scores(case["prompts"][1:2], case["pixels"][1:2], case["want_ids"], packed=p)
        for a, b in zip(alone, st["res"][p]):
            assert torch.equal(a.cpu(), b[n0:n0 + n1]), f"packed={p}"


def test_max_row_tokens_split_stays_within_the_bar():
    """An image whose row is split carries the prefix again in every row: same scores within the bar, first row bit-equal."""
    _need_gpu()
    st = _setup("mha")
    case = st["case"]
    _, _, bar, ref = _bar(st)
    out = st["model"].forward_next_token_scores(case["prompts"], case["pixels"], case["want_ids"], packed=True, max_row_tokens=160)
    assert float((out[1].cpu() - ref).abs().max()) <= bar
    assert torch.equal(out[1].cpu()[:2], st["res"][True][1][:2])


def test_omnilmm_with_repetition_penalty():
    """Precomputed tower tokens, the replacement splice, repetition_penalty=1.1 against HF's processor restated in
    autocheck_case.hf_repetition_penalty on the oracle's logits."""
    _need_gpu()
    from rlaif_v_amd.omnilmm import OmniLMMDPOModel
    cfg, ocfg = AC.omni_cfgs()
    W = AC.omni_weights(ocfg, std=0.04)
    tower, prompts = AC.omni_case(ocfg)
    model = OmniLMMDPOModel(cfg, with_optimizer=False)
    model.load_state_dict(W)
    want = [17, 101, 250, 300]
    flat = [p for plist in prompts for p in plist]
    logits = AC.omni_oracle_logits(ocfg, W, tower, prompts)
    want[0] = int(flat[0][2])                      # a wanted id that the first prompt contains: its logit is penalised
    pen = torch.stack([AC.hf_repetition_penalty(l, p, 1.1) for l, p in zip(logits, flat)])
    assert float((pen - logits).abs().max()) > 0
    ref = torch.log_softmax(pen, -1)[:, want]
    res = {p: [t.cpu() for t in model.forward_next_token_scores(prompts, tower, want, packed=p, repetition_penalty=1.1)]
           for p in (False, True)}
    e_un, e_pk = float((res[False][1] - ref).abs().max()), float((res[True][1] - ref).abs().max())
    bar = 2.0 * e_un if e_un > 0 else PRECOMPUTE_PER_TOKEN_BAR
    print(f"[omnilmm] max |logp - oracle|: packed=False {e_un:.4e}, packed=True {e_pk:.4e}, bar {bar:.4e}")
    _record("omnilmm_logp_err_unpacked", e_un)
    _record("omnilmm_logp_err_packed", e_pk)
    assert e_pk <= bar
    # without the penalty the scores differ from the penalised ones by far more than the bar at the penalised id
    plain = model.forward_next_token_scores(prompts, tower, want, packed=True)[1].cpu()
    ref_plain = torch.log_softmax(logits, -1)[:, want]
    print(f"[omnilmm] the penalty moves the oracle's logp at the penalised id by {float((ref_plain[0, 0] - ref[0, 0]).abs()):.4e}")
    assert float((plain - ref_plain).abs().max()) <= bar
    top2 = torch.topk(pen, 2, -1)
    sure = (top2.values[:, 0] - top2.values[:, 1]) > bar
    assert torch.equal(res[True][2].long()[sure], top2.indices[:, 0][sure])


def test_omnilmm_default_against_the_reference_fixture():
    """The default (no penalty) against the reference OmniLMM model's own scores (tests/golden/autocheck_omnilmm_tiny.pt;
    the reference passes repetition_penalty=1.1 to a generate that has no ids to penalise).  Bar as above: the packed error is
    at most 2 x the un-packed error against the CPU oracle on the same questions."""
    _need_gpu()
    from rlaif_v_amd.omnilmm import OmniLMMDPOModel
    case = AC.load_omni_case()
    cfg, ocfg = AC.omni_cfgs()
    W = AC.omni_weights(ocfg, std=case["std"])
    model = OmniLMMDPOModel(cfg, with_optimizer=False)
    model.load_state_dict(W)
    want = case["want_ids"]
    oracle = torch.log_softmax(AC.omni_oracle_logits(ocfg, W, case["tower"], case["prompts"]), -1)[:, want]
    res = {p: [t.cpu() for t in model.forward_next_token_scores(case["prompts"], case["tower"], want, packed=p)] for p in (False, True)}
    e_un = float((res[False][1] - oracle).abs().max())
    bar = 2.0 * e_un if e_un > 0 else PRECOMPUTE_PER_TOKEN_BAR
    ref = torch.log(case["probs"])
    for p in (False, True):
        err = float((res[p][1] - ref).abs().max())
        print(f"[omnilmm fixture] packed={p}: max |logp - reference| {err:.4e} (bar {bar:.4e})")
        _record(f"omnilmm_logp_err_vs_reference_packed_{p}", err)
        top2 = torch.topk(case["logits_last"], 2, -1)
        sure = (top2.values[:, 0] - top2.values[:, 1]) > bar
        assert torch.equal(res[p][2].long()[sure], case["new_token"][sure])
    assert float((res[True][1] - ref).abs().max()) <= bar


class _Tok:
    """tests/golden/toy_tokenizer.ToyTokenizer with the two calls the scoring stage adds (encode / decode)."""

    def __new__(cls):
        sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
        from toy_tokenizer import ToyTokenizer

        class Tok(ToyTokenizer):
            def encode(self, text):
                return self._ids(text.replace("<s>", ""))

            def decode(self, ids, skip_special_tokens=True):
                return " " + " ".join(f"t{int(i)}" for i in ids if not (skip_special_tokens and int(i) in (0, 1, 2))) + " "
        return Tok()


def test_score_yesno_records():
    _need_gpu()
    from rlaif_v_amd import autocheck
    st = _setup("mha")
    model, case = st["model"], st["case"]
    tok = _Tok()
    px = case["pixels"]
    questions = ["Is there a dog in the picture ?", "Is the dog running on the grass ?", "Is it raining ?",
                 "Are there two people walking along the beach at sunset ?", "Is the cat asleep ?", "Is it a sofa ?"]
    items = [dict(question=questions[0], image=px[0], question_id="q0", metainfos={"ds_question_id": 70, "origin": "a"}),
             dict(question=questions[1], image=px[0], question_id="q1", metainfos={"origin": "a"}),
             dict(question=questions[2], image=px[0]),
             dict(question=questions[3], image=px[1], question_id=11, image_id="b", metainfos={}),
             dict(question=questions[4], image=px[2], question_id=12, image_id="b", metainfos={}),      # same image_id: one group
             dict(question=questions[5], image=px[2], question_id=13, image_id="c", metainfos={})]
    assert autocheck.group_by_image(items) == [[0, 1, 2], [3, 4], [5]]
    recs = autocheck.score_yesno(model, tok, items, images_per_call=2, model_path="ckpt")
    assert [r["question_id"] for r in recs] == ["q0", "q1", 2, 11, 12, 13]
    assert list(recs[0]) == ["question_id", "ds_question_id", "raw_question", "answer", "scores", "metainfos", "model_path"]
    assert list(recs[1]) == ["question_id", "raw_question", "answer", "scores", "metainfos", "model_path"]
    assert recs[0]["ds_question_id"] == 70 and recs[0]["metainfos"] == {"ds_question_id": 70, "origin": "a"}
    assert [r["raw_question"] for r in recs] == questions and all(list(r["scores"]) == ["yes", "Yes", "no", "No"] for r in recs)
    # the values against the direct call on the same grouping
    want = autocheck.yesno_ids(tok, omnilmm=False)
    assert want == [tok.encode("<s> " + w)[-1] for w in ("yes", "Yes", "no", "No")]
    prompts = [[autocheck.wrap_question_for_llava15(items[i]["question"], tok) for i in g] for g in ([0, 1, 2], [3, 4], [5])]
    assert int((prompts[0][0] == -200).sum()) == 1 and int(prompts[0][0][0]) == tok.bos_token_id
    probs, _, argmax, _ = model.forward_next_token_scores(prompts[:2], torch.stack([px[0], px[1]]), want)
    probs2, _, argmax2, _ = model.forward_next_token_scores(prompts[2:], px[2:3], want)
    probs, argmax = torch.cat([probs, probs2]).cpu(), torch.cat([argmax, argmax2]).cpu()
    for n, r in enumerate(recs):
        assert [r["scores"][k] for k in ("yes", "Yes", "no", "No")] == [float(v) for v in probs[n]]
        assert r["answer"] == f"t{int(argmax[n])}" or (int(argmax[n]) in (0, 1, 2) and r["answer"] == "")
    assert "model_path" not in autocheck.score_yesno(model, tok, items[:1])[0]
