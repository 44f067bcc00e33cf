"""Continuous batching on the GPU (LlavaDPOModel.generate_continuous) on the tiny MHA and GQA models and the prompts of
tests/golden/generate_tiny.pt.  The reference of every comparison is ``generate()`` - the code of before, untouched - run
alone on one request: tokens are compared as integers, logits with torch.equal.  Prompts and budgets are short enough that
n_split is 1 on both paths."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import generate_case as GC  # noqa: E402
from oracle import dpo_oracle as O  # noqa: E402

T, REPEAT = 12, 2
BUDGETS = [12, 3, 7, 1, 12, 5, 9]
SAMPLING = dict(temperature=0.7, top_p=0.95, repetition_penalty=1.3)
_STATE = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _planted(index):
    """the uniforms of request ``index``: fp32 [T, REPEAT], a function of the index alone"""
    return torch.rand(T, REPEAT, generator=torch.Generator().manual_seed(1000 + index))


def _setup(name):
    """Model, the 7 requests cycling the fixture's three prompts, and per request the stand-alone ``generate()`` run with its
    planted uniforms and budget: computed once, shared, never modified."""
    if name not in _STATE:
        from rlaif_v_amd.model import LlavaConfig, LlavaDPOModel
        gold = GC.load_case()
        case = gold[name]
        cfg = O.tiny_cfg() if name == "mha" else O.tiny_gqa_cfg()
        assert O.asdict(cfg) == case["cfg"] and gold["steps"] == T
        model = LlavaDPOModel(LlavaConfig(**O.asdict(cfg)), with_optimizer=False)
        model.load_state_dict(O.make_weights(cfg, seed=case["seed"], std=gold["std"]))
        prompts, pixels = case["prompts"], case["pixels"]
        longest = max(int(p.numel()) - 1 + model.cfg.n_image_tokens for p in prompts)
        assert longest + T < 512, "n_split is 1 on both paths"
        requests = [(prompts[i % 3], pixels[i % 3], BUDGETS[i]) for i in range(len(BUDGETS))]
        alone = []
        for i, (p, px, budget) in enumerate(requests):
            toks, scores = model.generate([p], px[None], budget, repeat=REPEAT, _uniforms=_planted(i)[:budget], return_scores=True,
                                          **SAMPLING)
            assert all(len(t) == budget for t in toks[0])
            alone.append((toks[0], scores.cpu()))                      # ([REPEAT][budget], [budget, REPEAT, V])
        _STATE[name] = dict(model=model, case=case, cfg=cfg, requests=requests, alone=alone, longest=longest)
    return _STATE[name]


def _run(st, slots, order=None, poll_every=4, scores=None, **kw):
    order = list(range(len(st["requests"]))) if order is None else order
    sched = []
    args = dict(SAMPLING, slots=slots, repeat=REPEAT, max_prompt_tokens=st["longest"], poll_every=poll_every, _uniforms=_planted,
                request_indices=order, _scheduler=sched)
    args.update(kw)
    out = list(st["model"].generate_continuous((st["requests"][i] for i in order), T, _scores=scores, **args))
    assert sorted(i for i, _ in out) == sorted(order), "every request comes back once"
    return dict(out), sched[0]


@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_tokens_and_logits_equal_generate_run_alone(name):
    _need_gpu()
    st = _setup(name)
    rows = {}
    got, sched = _run(st, slots=6, scores=lambda i, r, j, row: rows.setdefault((i, r), {}).setdefault(j, row.cpu()))
    compared = 0
    for i, (toks, scores) in enumerate(st["alone"]):
        for r in range(REPEAT):
            assert got[i][r] == toks[r], f"request {i} sample {r}"
            for j in range(BUDGETS[i]):
                assert torch.equal(rows[(i, r)][j], scores[j, r]), f"request {i} sample {r} step {j}: the logits, bit for bit"
                compared += 1
    assert compared == REPEAT * sum(BUDGETS)
    assert len({tuple(t) for toks, _ in st["alone"] for t in toks}) > len(BUDGETS), "the samples of a request differ somewhere"
    # 3 requests fit 6 slots: the others were admitted into slots and regions that earlier ones had left
    assert [q for q, _, _ in sched.history] == list(range(7)) and len({tuple(s) for _, _, s in sched.history}) <= 3
    assert sched.steps_executed < sum(b - 1 for b in BUDGETS), "fewer steps than one request after the other"
    print(f"[{name}] {compared} logit rows bit-equal; {sched.steps_executed} decode steps, {sched.polls} polls for "
          f"{REPEAT * sum(BUDGETS)} tokens in 6 slots")


@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_results_do_not_depend_on_slots_or_arrival_order(name):
    _need_gpu()
    st = _setup(name)
    want = {i: toks for i, (toks, _) in enumerate(st["alone"])}
    for slots in (2, 6, 64):
        got, sched = _run(st, slots=slots)
        assert got == want, f"slots = {slots}"
        assert sched.steps_executed > 0
    got, _ = _run(st, slots=6, order=list(reversed(range(len(BUDGETS)))))
    assert got == want, "reversed arrival order"
    got, _ = _run(st, slots=64, regions=2, prefill_prompts=1, poll_every=1)
    assert got == want, "two prompt regions, one prompt per prefill, a poll after every step"


@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_eos_cuts_behind_it_and_leaves_the_others(name):
    _need_gpu()
    st = _setup(name)
    pick = None
    for i, (toks, _) in enumerate(st["alone"]):            # a token one sequence first emits mid-way
        for r, seq in enumerate(toks):
            for j in range(2, len(seq) - 1):
                if seq[j] not in seq[:j]:
                    pick = (i, r, j, seq[j])
                    break
            if pick:
                break
        if pick:
            break
    assert pick is not None
    i0, r0, j0, eos = pick

    def cut(seq):
        return seq[:seq.index(eos) + 1] if eos in seq else seq
    got, _ = _run(st, slots=6, eos_token_id=eos)
    for i, (toks, _) in enumerate(st["alone"]):
        assert got[i] == [cut(t) for t in toks], f"request {i}"
    assert len(got[i0][r0]) == j0 + 1 < BUDGETS[i0] and got[i0][r0][-1] == eos
    assert any(eos not in t and len(t) == BUDGETS[i] for i, (toks, _) in enumerate(st["alone"]) for t in toks), "others run to their budget"
    # two EOS ids, the second one an id nobody emits: the same cut
    emitted = {t for toks, _ in st["alone"] for seq in toks for t in seq}
    unused = next(v for v in range(st["cfg"].vocab) if v not in emitted)
    got2, _ = _run(st, slots=6, eos_token_id=[unused, eos])
    assert got2 == got


@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_a_reused_slot_forgets_its_earlier_occupant(name):
    """slots = 2, repeat = 1, six requests of 8 tokens, greedy with repetition penalty 1.5: each slot serves three sequences and
    each equals its stand-alone generate() run, so no id of an earlier occupant is penalised"""
    _need_gpu()
    st = _setup(name)
    model, case = st["model"], st["case"]
    reqs = [(case["prompts"][i % 3], case["pixels"][i % 3], 8) for i in range(6)]
    sched = []
    got = dict(model.generate_continuous(iter(reqs), T, slots=2, repeat=1, repetition_penalty=1.5, max_prompt_tokens=st["longest"],
                                         poll_every=4, _scheduler=sched))
    served = {}
    for q, _, slots in sched[0].history:
        served.setdefault(slots[0], []).append(q)
    assert served == {0: [0, 2, 4], 1: [1, 3, 5]}, "each slot serves three sequences"
    alone = [model.generate([case["prompts"][k]], case["pixels"][k][None], 8, repetition_penalty=1.5)[0][0] for k in range(3)]
    plain = [model.generate([case["prompts"][k]], case["pixels"][k][None], 8)[0][0] for k in range(3)]
    assert any(a != b for a, b in zip(alone, plain)), "the penalty changes a decision"
    for i in range(6):
        assert got[i] == [alone[i % 3]], f"request {i}"
    assert sched[0].steps_executed == 3 * 7


def test_text_only_requests():
    _need_gpu()
    import divide_case as DC
    gold = torch.load(DC.GOLD_TEXT, weights_only=True)
    model = DC.tiny_text_model(DC.tiny_text_weights(1024, gold["seed"], gold["std"], gold["head_scale"]), 1024)
    prompts, n = gold["prompts"], 8
    longest = max(int(p.numel()) for p in prompts)
    budgets = [n, 3, n, 5, 2]
    reqs = [(prompts[i % 3], None, budgets[i]) for i in range(len(budgets))]
    got = dict(model.generate_continuous(reqs, n, slots=2, repeat=1, max_prompt_tokens=longest, poll_every=4))
    for i, b in enumerate(budgets):
        assert got[i] == model.generate([prompts[i % 3]], None, b)[0], f"request {i}"
    with pytest.raises(ValueError, match="image=None"):
        list(model.generate_continuous([(prompts[0], torch.zeros(3, 4, 4))], n, slots=2, max_prompt_tokens=longest))


def test_refusals_name_the_gap():
    _need_gpu()
    st = _setup("mha")
    model, reqs = st["model"], st["requests"]
    k = max(range(3), key=lambda k: int(reqs[k][0].numel()))
    with pytest.raises(ValueError, match="longer than max_prompt_tokens"):
        list(model.generate_continuous([reqs[k]], T, slots=2, max_prompt_tokens=st["longest"] - 1))
    with pytest.raises(ValueError, match="outside"):
        list(model.generate_continuous([(reqs[0][0], reqs[0][1], T + 1)], T, slots=2, max_prompt_tokens=st["longest"]))
    with pytest.raises(NotImplementedError, match="beam"):
        model.generate_continuous(reqs, T, num_beams=3)
    with pytest.raises(ValueError, match="repeat 3 > slots 2"):
        model.generate_continuous(reqs, T, slots=2, repeat=3)
    from rlaif_v_amd.model import LlavaConfig, LlavaDPOModel, LoraConfig
    lora = LlavaDPOModel(LlavaConfig(**O.asdict(st["cfg"])), with_optimizer=False, lora=LoraConfig(r=8))
    with pytest.raises(NotImplementedError, match="LoRA"):
        lora.generate_continuous(reqs, T)
