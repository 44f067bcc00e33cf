"""KV-cached candidate generation on the GPU (LlavaDPOModel.generate, rlaif_v_amd.gen_data) on the tiny MHA and GQA
configurations, against tests/golden/generate_tiny.pt: what the reference's own ``generate(do_sample=False, num_beams=1,
max_new_tokens=12, output_scores=True, return_dict_in_generate=True)`` returned for three prompts of different lengths.

Oracle: ``oracle.dpo_oracle.llama_logits`` on prompt + tokens so far, fp32 on the CPU, no cache (generate_case.oracle_step_logits).

Bar of the teacher-forced logits: the cached path's maximum |logit - oracle| over all prompts, steps and vocabulary ids is at
most 2 x the error of the existing NO-CACHE path - a prefill of prompt + tokens so far through the forward that
forward_next_token_scores runs, one per step - against the same oracle on the same sequences, measured in the same test (the
precedent of tests/test_autocheck_gpu.py: both are bf16 noise of the same stack in a different summation order).  Both errors
are printed."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import generate_case as GC  # noqa: E402
from oracle import dpo_oracle as O  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_STATE = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _setup(name):
    """Model, case, oracle, the teacher-forced cached run, the no-cache prefills and the free greedy run of one configuration:
    computed once, shared, never modified."""
    if name not in _STATE:
        from rlaif_v_amd.model import LlavaConfig, LlavaDPOModel
        gold = GC.load_case()
        case = gold[name]
        cfg = O.tiny_cfg() if name == "mha" else O.tiny_gqa_cfg()
        assert O.asdict(cfg) == case["cfg"]
        W = O.make_weights(cfg, seed=case["seed"], std=gold["std"])
        model = LlavaDPOModel(LlavaConfig(**O.asdict(cfg)), with_optimizer=False)
        model.load_state_dict(W)
        prompts, pixels, seqs, T = case["prompts"], case["pixels"], case["sequences"], gold["steps"]
        oracle = GC.oracle_step_logits(cfg, W, prompts, pixels, seqs.tolist())               # [3, T, V]
        forced_out, forced = model.generate(prompts, pixels, T, _forced_tokens=seqs, return_scores=True)
        nocache = []
        for j in range(T):
            ext = [torch.cat([p, seqs[k, :j].to(p.dtype)]) for k, p in enumerate(prompts)]
            nocache.append(model._prefill(ext, pixels)[:len(prompts), :cfg.vocab].cpu())
        greedy, greedy_scores = model.generate(prompts, pixels, T, return_scores=True)
        _STATE[name] = dict(gold=gold, case=case, cfg=cfg, W=W, model=model, oracle=oracle, forced_out=forced_out,
                            forced=forced.cpu().transpose(0, 1), nocache=torch.stack(nocache, 1), greedy=greedy,
                            greedy_scores=greedy_scores.cpu(), T=T)
    return _STATE[name]


def _errors(st):
    e_nc = float((st["nocache"] - st["oracle"]).abs().max())
    e_c = float((st["forced"] - st["oracle"]).abs().max())
    return e_nc, e_c


@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_teacher_forced_logits_within_twice_the_no_cache_error(name):
    _need_gpu()
    st = _setup(name)
    e_nc, e_c = _errors(st)
    e_ref = float((st["forced"] - st["case"]["scores"]).abs().max())
    print(f"[{name}] max |logit - oracle| over {st['oracle'].numel()} logits: no-cache prefill per step {e_nc:.4e}, KV-cached "
          f"{e_c:.4e} (bar {2 * e_nc:.4e}); KV-cached against the reference's generate scores {e_ref:.4e}; "
          f"generate_ran={st['case']['generate_ran']}")
    assert torch.isfinite(st["forced"]).all()
    assert e_nc > 0
    assert e_c <= 2 * e_nc
    assert e_ref <= 2 * e_nc + 1e-4                       # the oracle reproduces the reference to 1e-4
    assert [s[0] for s in st["forced_out"]] == st["case"]["sequences"].tolist()     # forced tokens come back as the output
    # step 0 is the prefill itself: the existing forward's bits
    assert torch.equal(st["forced"][:, 0], st["nocache"][:, 0])


@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_greedy_tokens_equal_the_reference_generate(name):
    """every step whose recorded top-1 / top-2 gap exceeds twice the measured no-cache logit error must give the reference's
    token; behind an undecidable step that went the other way the rest of that sequence is undecidable too (its context
    differs).  At most 10 % of the steps may be skipped."""
    _need_gpu()
    st = _setup(name)
    e_nc, _ = _errors(st)
    gaps, want = st["case"]["gaps"], st["case"]["sequences"].tolist()
    assert float(gaps.min()) > 2 * st["gold"]["gap_bar"]          # the generator's seed condition, stored with the fixture
    skipped = total = 0
    for k, seq in enumerate(want):
        got = st["greedy"][k][0]
        assert len(got) == st["T"]
        lost = False
        for j in range(st["T"]):
            total += 1
            if lost or not float(gaps[k, j]) > 2 * e_nc:
                skipped += 1
                lost = lost or got[j] != seq[j]
                continue
            assert got[j] == seq[j], f"prompt {k} step {j}: token {got[j]}, the reference generated {seq[j]} (gap {float(gaps[k, j]):.3e})"
    print(f"[{name}] greedy: {total - skipped} of {total} steps compared (smallest recorded gap {float(gaps.min()):.3e}, 2 x no-cache "
          f"error {2 * e_nc:.3e})")
    assert skipped <= 0.1 * total


def _uniform_plan(T, n_prompts, repeat, seed):
    base = torch.rand(T, n_prompts, generator=torch.Generator().manual_seed(seed))
    return base, base.repeat_interleave(repeat, dim=1)


@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_repeats_share_the_prompt_and_sampling_is_reproducible(name):
    _need_gpu()
    st = _setup(name)
    model, case, T = st["model"], st["case"], st["T"]
    prompts, pixels = case["prompts"], case["pixels"]
    base, planted = _uniform_plan(T, len(prompts), 4, seed=7)
    one, s1 = model.generate(prompts, pixels, T, repeat=1, temperature=0.7, top_p=0.95, _uniforms=base, return_scores=True)
    four, s4 = model.generate(prompts, pixels, T, repeat=4, temperature=0.7, top_p=0.95, _uniforms=planted, return_scores=True)
    for k in range(len(prompts)):
        assert len(four[k]) == 4 and all(four[k][r] == one[k][0] for r in range(4)), "identical uniforms, identical samples"
        for r in range(4):
            assert torch.equal(s4[:, 4 * k + r], s1[:, k]), "a sample's logits do not depend on the rows next to it"
    assert any(one[k][0] != st["greedy"][k][0] for k in range(len(prompts))), "temperature 0.7 should leave the greedy path somewhere"
    # a seeded generator fixes the output; another seed changes it
    runs = [model.generate(prompts, pixels, T, repeat=3, temperature=0.7, generator=torch.Generator().manual_seed(s))
            for s in (11, 11, 12)]
    assert runs[0] == runs[1]
    assert runs[0] != runs[2]
    assert len({tuple(x) for x in runs[0][2]}) > 1, "three samples of one prompt from different uniforms should not all agree"
    # greedy with repeats: every copy is the greedy sequence
    g2 = model.generate(prompts, pixels, T, repeat=2)
    assert all(g2[k][r] == st["greedy"][k][0] for k in range(len(prompts)) for r in range(2))


@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_eos_cuts_one_sequence_and_leaves_the_others(name):
    _need_gpu()
    st = _setup(name)
    model, case, T = st["model"], st["case"], st["T"]
    greedy = [g[0] for g in st["greedy"]]
    pick = None
    for k, seq in enumerate(greedy):                       # a token one sequence first emits mid-way
        for j in range(2, T - 1):
            if seq[j] not in seq[:j]:
                pick = (k, j, seq[j])
                break
        if pick:
            break
    if pick is None:                                       # a degenerate greedy loop: cut at a repeated token's first place
        k = 0
        pick = (k, greedy[k].index(greedy[k][T // 2]), greedy[k][T // 2])
    k, j, eos = pick
    out, scores = model.generate(case["prompts"], case["pixels"], T, eos_token_id=eos, return_scores=True)
    for i, seq in enumerate(greedy):
        want = seq[:seq.index(eos) + 1] if eos in seq else seq
        assert out[i][0] == want
    assert len(out[k][0]) == j + 1 < T and out[k][0][-1] == eos
    assert torch.equal(scores.cpu(), st["greedy_scores"][:scores.shape[0]]), "the logits of the other sequences, bit for bit"


@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_repetition_penalty_covers_the_generated_ids_only(name):
    """greedy with repetition_penalty = 1.5: at every step the token is the argmax of that step's own logits (return_scores) after
    RepetitionPenaltyLogitsProcessor over the ids the sequence has generated so far - no prompt id, as the reference's generate
    from inputs_embeds sees none - restated in float64 (generate_case.penalised).  The kernel divides and multiplies in fp32:
    one rounding of relative size 2^-24 on each logit, so a step is decided when its penalised top-1 / top-2 gap exceeds
    2 * 2^-24 * max |logit|; at most 10 % of the steps may fall below that."""
    _need_gpu()
    import numpy as np
    st = _setup(name)
    model, case, T = st["model"], st["case"], st["T"]
    pen = 1.5
    out, scores = model.generate(case["prompts"], case["pixels"], T, repetition_penalty=pen, return_scores=True)
    scores = scores.cpu().double().numpy()                              # [T, n_prompts, V]
    skipped = 0
    for k in range(len(case["prompts"])):
        got = out[k][0]
        assert len(got) == T
        for j in range(T):
            x = GC.penalised(scores[j, k], got[:j] if j else None, float(np.float32(pen)))
            top = np.sort(x)[-2:]
            if not top[1] - top[0] > 2 * GC.U32 * np.abs(scores[j, k]).max():
                skipped += 1
                continue
            assert got[j] == int(x.argmax()), f"prompt {k} step {j}: token {got[j]}, penalised argmax {int(x.argmax())}"
        assert got[0] == st["greedy"][k][0][0], "nothing is generated before step 0: no id is penalised, the prompt's neither"
    assert torch.equal(torch.as_tensor(scores[0]).float(), st["greedy_scores"][0]), "the penalty changes decisions, not logits"
    print(f"[{name}] repetition penalty {pen}: {skipped} of {T * len(out)} steps undecided")
    assert skipped <= 0.1 * T * len(out)
    assert any(out[k][0] != st["greedy"][k][0] for k in range(len(out))), "the greedy sequences repeat tokens: 1.5 must change one"


def test_unsupported_modes_name_the_gap():
    _need_gpu()
    st = _setup("mha")
    model, case = st["model"], st["case"]
    with pytest.raises(NotImplementedError, match="beam"):
        model.generate(case["prompts"], case["pixels"], 2, num_beams=3)
    from rlaif_v_amd.model import LlavaConfig, LlavaDPOModel, LoraConfig
    lora = LlavaDPOModel(LlavaConfig(**O.asdict(st["cfg"])), with_optimizer=False, lora=LoraConfig(r=8))
    with pytest.raises(NotImplementedError, match="LoRA"):
        lora.generate(case["prompts"], case["pixels"], 2)
    with pytest.raises(ValueError):
        model.generate(case["prompts"], case["pixels"][:2], 2)


class _Tok:
    def __new__(cls):
        sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
        from toy_tokenizer import ToyTokenizer

        class Tok(ToyTokenizer):
            eos_token_id = None                            # the random tiny model would emit it at random

            def decode(self, ids, skip_special_tokens=True):
                return " " + " ".join(f"t{int(i)}" for i in ids if not (skip_special_tokens and int(i) in (0, 1, 2))) + " "
        return Tok()


def test_gen_data_records_from_a_jsonl(tmp_path):
    """two images x repeat 3 through read_gen_dataset + generate_answers: 6 records with the reference's keys and order, the
    values those of the direct generate call with the same seed"""
    _need_gpu()
    import numpy as np
    from PIL import Image
    from rlaif_v_amd import autocheck, gen_data
    st = _setup("mha")
    model, tok = st["model"], _Tok()
    rng = np.random.default_rng(3)
    lines = []
    for n, q in enumerate(["What is shown in the picture ?", "Describe the scene in detail ."]):
        path = str(tmp_path / f"img{n}.png")
        Image.fromarray(rng.integers(0, 256, (60 + 8 * n, 72, 3), dtype=np.uint8)).save(path)
        item = dict(image_path=path, question=q, question_id=f"q{n}")
        if n == 0:
            item["ds_question_id"] = 70
        lines.append(json.dumps(item))
    qa = tmp_path / "questions.jsonl"
    qa.write_text("\n".join(lines) + "\n")
    items = autocheck.read_gen_dataset(str(qa))
    recs = gen_data.generate_answers(model, tok, items, repeat=3, temperature=0.7, max_tokens=6, seed=4, model_path="ckpt")
    assert len(recs) == 6 and [r["question_id"] for r in recs] == ["q0"] * 3 + ["q1"] * 3
    assert list(recs[0]) == ["question_id", "ds_question_id", "raw_question", "answer", "metainfos", "model_path"]
    assert list(recs[3]) == ["question_id", "raw_question", "answer", "metainfos", "model_path"]
    assert recs[0]["ds_question_id"] == 70 and recs[3]["raw_question"] == "Describe the scene in detail ."
    prompts = [autocheck.wrap_question_for_llava15(it["question"], tok) for it in items]
    direct = model.generate(prompts, [it["image"] for it in items], 6, repeat=3, temperature=0.7,
                            generator=torch.Generator().manual_seed(4))
    assert [r["answer"] for r in recs] == [tok.decode(direct[k][r]).strip() for k in range(2) for r in range(3)]
    assert all(len(direct[k][r]) == 6 for k in range(2) for r in range(3))
    json.dumps(recs)
