"""Host side of beam search with a repetition penalty and of OmniLMM candidate generation: the float64 restatement
(tests/beam_penalty_case.py) against the reference's recorded runs (tests/golden/beam_penalty_tiny.pt), the processor's semantics,
rv_beam_topk_penalty's declaration and refusals (every call is refused before any launch), rlaif_v_amd.omnilmm_gen_data's
parser and records on a stubbed model, and the base class's refusals of a splicing model it was not told about.  No GPU."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import beam_case as BC  # noqa: E402
import beam_penalty_case as PC  # noqa: E402

P = 0x7F0000010000          # an "operand": 64 KiB aligned, never dereferenced


# ------------------------------------------------------------------------------------------------ restatement vs the reference
@pytest.mark.parametrize("run", ["a", "b"])
@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_restatement_reproduces_the_reference_from_its_recorded_logits(name, run):
    gold = PC.load_case()
    K, T, pen = gold["num_beams"], gold["steps"], gold["penalty"]
    assert pen == 1.1 and K == 3 and T == 12
    r = gold[name]["runs"][run]
    for k, rec in enumerate(r["prompts"]):
        lg = rec["logits"].numpy()
        g, steps = PC.beam_search64(lambda j, beams: lg[j], K, T, r["eos"], penalty=pen)
        assert len(steps) == lg.shape[0], "the search stops at the step the reference stopped at"
        toks, score, bidx = g.best()
        assert toks == rec["sequences"].tolist() == rec["answer"].tolist()
        n = int((rec["beam_indices"] >= 0).sum())
        assert bidx == rec["beam_indices"][:n].tolist() and n == len(toks)
        assert abs(score - float(rec["sequences_scores"])) <= 1e-5
        assert np.array_equal(np.stack([s["parent"] for s in steps]), rec["parent"].numpy())
        assert np.array_equal(np.stack([s["token"] for s in steps]), rec["token"].numpy())
        assert np.allclose([s["margin_keep"] for s in steps], rec["margin_keep"].numpy(), rtol=0, atol=1e-9)


def test_fixture_needs_the_penalty():
    """the un-penalised restatement on the same recorded logits does NOT return the reference's answer and score for every
    prompt, and the generator recorded that the reference's own un-penalised search runs other beams"""
    gold = PC.load_case()
    K, T = gold["num_beams"], gold["steps"]
    for name in ("mha", "gqa"):
        a, b = gold[name]["runs"]["a"], gold[name]["runs"]["b"]
        assert any(r["differs"] for r in a["prompts"])
        wrong = 0
        for rec in a["prompts"]:
            lg = rec["logits"].numpy()
            g, _ = BC.beam_search64(lambda j, beams: lg[j], K, T, a["eos"])
            toks, score, _ = g.best()
            wrong += int(toks != rec["answer"].tolist() or abs(score - float(rec["sequences_scores"])) > 1e-5)
        assert wrong >= 1
        assert all(r["answer"].numel() == T and r["logits"].shape[0] == T for r in a["prompts"])
        assert any(r["answer"].numel() < T and int(r["answer"][-1]) == b["eos"] for r in b["prompts"])
        assert any(r["logits"].shape[0] < T for r in b["prompts"])


# ------------------------------------------------------------------------------------------------ the processor's semantics
def test_each_distinct_id_once_sign_rule_and_range():
    lp = np.array([-1.0, -2.0, 0.0, 3.0, -4.0, 0.5])              # a general score row: the rule has two signs
    out = PC.hf_repetition_penalty(lp, [1, 1, 1, 3, -1, 6, 2 ** 30, 5, 1], 2.0)
    assert out.tolist() == [-1.0, -4.0, 0.0, 1.5, -4.0, 0.25], "id 1 once (not -16), 3 and 5 divided, -1 / 6 / 2^30 ignored"
    assert PC.hf_repetition_penalty(lp, [], 2.0).tolist() == lp.tolist() and PC.hf_repetition_penalty(lp, [2], 2.0)[2] == 0.0
    assert PC.distinct_ids([4, -1, 4, 9, 3, 8], 9) == [3, 4, 8]
    # it is HF's processor: gather, rescale, scatter (tests/autocheck_case.py restates it on torch tensors)
    import autocheck_case as AC
    row = torch.tensor(lp)
    assert torch.equal(AC.hf_repetition_penalty(row, [1, 1, 3, 5], 2.0), torch.tensor(out))
    # in beam-search position: on the log-softmax, before the score - not on the logits, not after the add
    logits = np.array([[2.0, 1.0, 0.0, -1.0], [0.0, 0.5, 1.0, 1.5]])
    score = np.array([-0.25, -3.0])
    hists = [[0, 0], [3, 7]]
    lsm = BC.log_softmax64(logits)
    want = lsm.copy()
    want[0, 0] *= 1.1
    want[1, 3] *= 1.1
    want += score[:, None]
    val, par, tok = PC.topk_candidates(logits, score, 4, hists, 1.1)
    flat = want.reshape(-1)
    order = np.lexsort((np.arange(8), -flat))[:5]
    assert np.array_equal(par, order // 4) and np.array_equal(tok, order % 4) and np.allclose(val, flat[order], rtol=0, atol=0)
    assert not np.allclose(val, BC.topk_candidates(logits, score, 4)[0])
    # penalty 1 is beam_case
    for a, b in zip(PC.topk_candidates(logits, score, 4, hists, 1.0), BC.topk_candidates(logits, score, 4)):
        assert np.array_equal(a, b)


def test_group64_with_penalty_one_is_beam_case_and_penalises_its_own_tokens():
    rng = np.random.default_rng(0)
    K, T, V = 3, 5, 40
    lgs = rng.normal(size=(T, K, V)) * 3
    a, sa = BC.beam_search64(lambda j, beams: lgs[j], K, T, eos=7)
    b, sb = PC.beam_search64(lambda j, beams: lgs[j], K, T, eos=7, penalty=1.0)
    assert a.best() == b.best() and all(x["margin_keep"] == y["margin_keep"] and x["margin"] == y["margin"] for x, y in zip(sa, sb))
    # a row that always prefers token 3: with a strong penalty the beam cannot repeat it for ever
    lg = np.zeros((K, V))
    lg[:, 3] = 1.0
    plain, _ = BC.beam_search64(lambda j, beams: lg, K, T)
    pen, steps = PC.beam_search64(lambda j, beams: lg, K, T, penalty=50.0)
    assert plain.best()[0] == [3] * T and pen.best()[0].count(3) == 1
    # the bound of a penalised value: E0 x penalty + 2^-24 |lp x penalty|, then + 2^-24 |value|
    v, e = PC.penalised_bound(lgs[0], np.array([-1.0, -2.0, -3.0]), [[5, 5], [], [40, -1]], 1.1)
    v0, e0 = BC.logsoftmax_add_bound(lgs[0], np.zeros(K))
    assert np.isclose(v[0, 5], v0[0, 5] * 1.1 - 1.0) and np.isclose(e[0, 5], e0[0, 5] * 1.1 + PC.U32 * abs(v0[0, 5] * 1.1) + PC.U32 * abs(v[0, 5]))
    assert np.isclose(v[1, 5], v0[1, 5] - 2.0) and np.isclose(e[2, 0], e0[2, 0] + PC.U32 * abs(v[2, 0])), "ids out of range: nothing"


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_point_declared_exported_and_abi_stays_7():
    from rlaif_v_amd import hip
    decls = hip.parse_header()
    assert [t for t, _ in decls["rv_beam_topk_penalty"][1]] == \
        ["const float*", "long", "const float*", "int", "int", "int", "const int*", "long", "int", "float", "float*", "int*", "int*",
         "float*", "float*", "long", "void*"]
    lib = hip.lib()
    assert hasattr(lib.lib, "rv_beam_topk_penalty") and lib.lib.rv_abi_version() == 7


def _call(**kw):
    from rlaif_v_amd import hip
    lib = hip.lib()
    a = dict(logits=P, ldl=512, score=P, G=2, K=3, V=512, hist=P, ld_h=16, n_hist=4, penalty=1.1, val=P, par=P, tok=P, lse=P, ws=P,
             wsn=int(lib.lib.rv_beam_topk_workspace_floats(2, 3)))
    a.update(kw)
    rc = lib.lib.rv_beam_topk_penalty(*[a[k] for k in ("logits", "ldl", "score", "G", "K", "V", "hist", "ld_h", "n_hist", "penalty", "val",
                                                        "par", "tok", "lse", "ws", "wsn")], None)
    return rc, lib.last_error()


@pytest.mark.parametrize("kw,text", [
    (dict(K=0), "1 <= K <= 8"), (dict(K=9), "1 <= K <= 8"), (dict(G=0), "G >= 1"), (dict(G=30000), "65535"),
    (dict(V=65537, ldl=65537), "V_valid <= 65536"), (dict(V=5), "2 K"), (dict(ldl=511), "ldl >= V_valid"),
    (dict(logits=None), "NULL"), (dict(score=None), "NULL"), (dict(val=None), "NULL"), (dict(par=None), "NULL"), (dict(tok=None), "NULL"),
    (dict(lse=None), "NULL"), (dict(ws=None), "NULL"), (dict(logits=P + 2), "4-byte aligned"), (dict(lse=P + 1), "4-byte aligned"),
    (dict(wsn=71), "workspace smaller"),
    (dict(penalty=0.0), "penalty must be > 0"), (dict(penalty=-1.1), "penalty must be > 0"), (dict(penalty=float("nan")), "penalty must be > 0"),
    (dict(n_hist=-1), "n_hist"), (dict(n_hist=17), "n_hist"), (dict(hist=None), "hist is NULL"),
    (dict(hist=P + 2), "hist must be 4-byte aligned"), (dict(ld_h=2 ** 31 // 6 + 1), "int32"),
])
def test_refusals_before_any_launch(kw, text):
    rc, msg = _call(**kw)
    assert rc == 1 and msg.startswith("rv_beam_topk_penalty: ") and text in msg, (kw, rc, msg)


def test_plain_entry_point_keeps_its_name_in_the_shared_checks():
    from rlaif_v_amd import hip
    lib = hip.lib()
    assert lib.lib.rv_beam_topk(P, 512, P, 2, 9, 512, P, P, P, P, P, 72, None) == 1
    assert lib.last_error() == "rv_beam_topk: 1 <= K <= 8 beams"


def test_ops_beam_topk_validates_the_history_before_any_launch():
    from rlaif_v_amd import ops

    class T:                                                           # no device here: operands that only CLAIM to be on one
        def __init__(self, shape, dtype, device="cuda:0", stride=None):
            self.shape, self.dtype, self.device, self.is_cuda = tuple(shape), dtype, device, True
            self._stride = stride or tuple(int(np.prod(shape[i + 1:])) for i in range(len(shape)))

        def dim(self):
            return len(self.shape)

        def stride(self, i=None):
            return self._stride if i is None else self._stride[i]

        def numel(self):
            return int(np.prod(self.shape))

        def is_contiguous(self):
            return True
    lg, sc = T((6, 512), torch.float32), T((6,), torch.float32)
    for hist, kw in ((T((6, 8), torch.int64), {}), (T((5, 8), torch.int32), {}), (T((6, 8), torch.int32), dict(n_hist=9)),
                     (T((6, 8), torch.int32, stride=(8, 2)), {}), (T((6, 8), torch.int32, device="cuda:1"), {}),
                     (T((6, 8), torch.int32), dict(penalty=0.0)), (None, dict(n_hist=3)), (None, dict(penalty=1.1))):
        with pytest.raises(ValueError, match="beam_topk"):
            ops.beam_topk(lg, sc, 2, 3, 512, hist=hist, **{"n_hist": 0, "penalty": 1.1, **kw} if hist is not None else kw)


# ------------------------------------------------------------------------------------------------ omnilmm_gen_data
def _tok():
    from toy_tokenizer import OmniToyTokenizer

    class Tok(OmniToyTokenizer):
        def decode(self, ids, skip_special_tokens=True):
            return " " + " ".join(f"t{int(i)}" for i in ids if not (skip_special_tokens and int(i) in (0, 1, 2))) + " "
    return Tok()


def _stub(n_image_tokens=4):
    calls = []

    def check(prompts):
        for p in prompts:                                              # wrap_question_for_omni_lmm's ids: <im_start> <im_patch> x n <im_end>
            ids = p.tolist()
            assert ids[0] == 1 and ids.count(7) == 1 and ids.count(8) == 1 and ids.count(9) == n_image_tokens and ids[-2:] == [6, 3]

    def beam_search(prompts, images, max_new_tokens, num_beams=3, eos_token_id=None, length_penalty=1.0, return_trace=False,
                    repetition_penalty=1.0):
        check(prompts)
        calls.append(dict(kind="beam", n=len(prompts), max_new_tokens=max_new_tokens, num_beams=num_beams, eos=eos_token_id,
                          penalty=repetition_penalty, images=tuple(images.shape) if torch.is_tensor(images) else len(images)))
        return [[10 * len(calls) + k, 7, 2] for k in range(len(prompts))], [-1.0] * len(prompts)

    def generate(prompts, images, max_new_tokens, repeat=1, temperature=0.0, top_p=1.0, repetition_penalty=1.0, eos_token_id=None,
                 generator=None, return_scores=False, top_k=0):
        check(prompts)
        calls.append(dict(kind="generate", n=len(prompts), temperature=temperature, top_p=top_p, repeat=repeat, top_k=top_k,
                          penalty=repetition_penalty, eos=eos_token_id, max_new_tokens=max_new_tokens,
                          u=float(torch.rand(1, generator=generator))))
        return [[[100 * len(calls) + 10 * k + r, 2] for r in range(repeat)] for k in range(len(prompts))]

    def generate_continuous(requests, max_new_tokens, slots=64, repeat=1, temperature=0.0, top_p=1.0, top_k=0, repetition_penalty=1.0,
                            eos_token_id=None, seed=0, max_prompt_tokens=None, request_indices=None):
        reqs = list(requests)
        check([r[0] for r in reqs])
        idx = list(request_indices)
        calls.append(dict(kind="continuous", n=len(reqs), slots=slots, repeat=repeat, penalty=repetition_penalty, seed=seed,
                          max_prompt_tokens=max_prompt_tokens, longest=max(int(r[0].numel()) for r in reqs), indices=idx))
        for i in reversed(idx):                                        # completion order is not request order
            yield i, [[500 + 10 * i + r, 2] for r in range(repeat)]
    model = types.SimpleNamespace(cfg=types.SimpleNamespace(arch="omnilmm", n_image_tokens=n_image_tokens), generate=generate,
                                  beam_search=beam_search, generate_continuous=generate_continuous)
    return model, calls


ITEMS = [dict(question="What is shown ?", image=torch.zeros(5, 6), question_id="q0", metainfos={"ds_question_id": 70, "origin": "a"}),
         dict(question="Describe the scene .", image=torch.zeros(5, 6), metainfos={"origin": "b"}),
         dict(question="How many apples ?", image=torch.zeros(5, 6), question_id=12)]
KEYS = ["question_id", "raw_question", "answer", "metainfos", "model_path"]


def test_records_of_the_sampling_branch_on_a_stubbed_model():
    from rlaif_v_amd import omnilmm_gen_data as G
    model, calls = _stub()
    recs = G.generate_answers(model, _tok(), ITEMS, repeat=3, temperature=0.7, max_tokens=8, seed=5, prompts_per_call=2, model_path="ckpt")
    assert [(c["kind"], c["n"], c["repeat"], c["max_new_tokens"], c["eos"], c["penalty"], c["temperature"]) for c in calls] == \
        [("generate", 2, 3, 8, 2, 1.1, 0.7), ("generate", 1, 3, 8, 2, 1.1, 0.7)], "the reference's hard-coded 1.1"
    assert calls[0]["u"] == float(torch.rand(1, generator=torch.Generator().manual_seed(5)))        # the seeded CPU generator
    assert len(recs) == 9 and [r["question_id"] for r in recs] == ["q0"] * 3 + [1] * 3 + [12] * 3
    assert list(recs[0]) == [KEYS[0], "ds_question_id"] + KEYS[1:] and list(recs[3]) == KEYS
    assert recs[0]["ds_question_id"] == 70 and recs[0]["metainfos"] == {"ds_question_id": 70, "origin": "a"} and recs[8]["metainfos"] == {}
    assert [r["answer"] for r in recs] == ["t100", "t101", "t102", "t110", "t111", "t112", "t200", "t201", "t202"]
    assert all(r["model_path"] == "ckpt" for r in recs) and recs[4]["raw_question"] == "Describe the scene ."
    # --continuous: the same records in item order whatever the completion order; the replacement splice keeps the prompt length
    model, calls = _stub()
    recs = G.generate_answers(model, _tok(), ITEMS, repeat=2, max_tokens=8, seed=5, continuous=True, slots=4, index_base=40)
    c, = calls
    assert (c["kind"], c["n"], c["slots"], c["repeat"], c["penalty"], c["seed"], c["indices"]) == ("continuous", 3, 4, 2, 1.1, 5, [40, 41, 42])
    assert c["max_prompt_tokens"] == c["longest"]
    assert [r["answer"] for r in recs] == ["t900", "t901", "t910", "t911", "t920", "t921"] and [r["question_id"] for r in recs] == ["q0", "q0", 1, 1, 12, 12]


def test_records_of_the_beam_branch_on_a_stubbed_model():
    from rlaif_v_amd import omnilmm_gen_data as G
    model, calls = _stub()
    recs = G.generate_answers(model, _tok(), ITEMS, repeat=3, max_tokens=9, num_beam=3, prompts_per_call=2, model_path="ckpt")
    assert [(c["kind"], c["n"], c["num_beams"], c["max_new_tokens"], c["eos"], c["penalty"], c["images"]) for c in calls] == \
        [("beam", 2, 3, 9, 2, 1.1, (2, 5, 6)), ("beam", 1, 3, 9, 2, 1.1, (1, 5, 6))], "one search per item, not per copy"
    assert [r["answer"] for r in recs] == ["t10 t7"] * 3 + ["t11 t7"] * 3 + ["t20 t7"] * 3, "the copies of an item are equal"
    assert list(recs[0]) == [KEYS[0], "ds_question_id"] + KEYS[1:] and list(recs[3]) == KEYS and len(recs) == 9
    with pytest.raises(NotImplementedError, match="num_beam <= 8"):
        G.generate_answers(model, _tok(), ITEMS, num_beam=9)
    with pytest.raises(NotImplementedError, match="OmniLMM"):
        G.generate_answers(types.SimpleNamespace(cfg=types.SimpleNamespace(arch="llava")), _tok(), ITEMS)
    assert G.generate_answers(model, _tok(), []) == []


def test_command_line_accepts_the_reference_scripts_flags():
    from rlaif_v_amd import omnilmm_gen_data as G
    a = G.build_parser().parse_args("--checkpoint c --ds_name d --answer_file a --max_sample 7 --start_pos 3 --end_pos 9 --repeat 10 "
                                    "--temperature 0.7 --num_beam 3 --max_tokens 512 --seed 4 --batch-size 2 --num-workers 5".split())
    assert (a.max_sample, a.start, a.end, a.repeat, a.num_beam, a.max_tokens, a.seed, a.batch_size, a.num_workers) == (7, 3, 9, 10, 3, 512, 4, 2, 5)
    assert G.sampling_args(a) == {"temperature": 0.7, "top_p": 1.0, "top_k": 0, "repetition_penalty": 1.1}
    d = G.build_parser().parse_args("--checkpoint c --ds_name d --answer_file a".split())
    assert (d.num_beam, d.repeat, d.max_tokens, d.temperature, d.batch_size, d.continuous, d.slots, d.hf_defaults) == \
        (-1, 1, 10, 0.7, 1, False, 64, False)
    h = G.build_parser().parse_args("--checkpoint /nonexistent --ds_name d --answer_file a --hf_defaults --top_p 0.9 --continuous --slots 8".split())
    assert G.sampling_args(h) == {"temperature": 1.0, "top_p": 0.9, "top_k": 50, "repetition_penalty": 1.1}, \
        "HF's defaults for what the call leaves open; the penalty is the call's own"
    with pytest.raises(NotImplementedError, match="rlaif_v_amd.autocheck"):
        G.main("--checkpoint c --ds_name d --answer_file a --is_yesno".split())
    with pytest.raises(NotImplementedError, match="num_beam <= 8"):
        G.main("--checkpoint c --ds_name d --answer_file a --num_beam 9".split())
    with pytest.raises(NotImplementedError, match="continuous"):
        G.main("--checkpoint c --ds_name d --answer_file a --num_beam 3 --continuous".split())


# ------------------------------------------------------------------------------------------------ who may decode with a splicer
def test_base_class_still_refuses_a_splicing_model_by_name_and_omnilmm_opens_itself():
    from rlaif_v_amd import gen_data, vqa
    from rlaif_v_amd.model import LlavaDPOModel
    from rlaif_v_amd.omnilmm import OmniLMMDPOModel
    for cfg_arch, splicer in (("omnilmm", object()), ("omnilmm", None), ("llava", object())):
        m = types.SimpleNamespace(cfg=types.SimpleNamespace(arch=cfg_arch, head_dim=128), lora=None, store=None,
                                  _row_splicer=lambda s=splicer: s)
        with pytest.raises(NotImplementedError, match="OmniLMM"):
            LlavaDPOModel.generate(m, [torch.tensor([1, 2])], [None], 2)
        with pytest.raises(NotImplementedError, match="OmniLMM"):
            LlavaDPOModel.generate_continuous(m, [], 2)
        with pytest.raises(NotImplementedError, match="OmniLMM"):
            LlavaDPOModel.beam_search(m, [torch.tensor([1, 2])], [None], 2)
    assert OmniLMMDPOModel._decodes_spliced_rows is True and not hasattr(LlavaDPOModel, "_decodes_spliced_rows")
    # told so, the shared bodies go on to their next check
    m = types.SimpleNamespace(cfg=types.SimpleNamespace(arch="omnilmm", head_dim=128), lora=None, store=None,
                              _row_splicer=lambda: object(), _decodes_spliced_rows=True)
    with pytest.raises(NotImplementedError, match="beam search"):
        LlavaDPOModel.generate(m, [torch.tensor([1, 2])], [None], 2, num_beams=3)
    with pytest.raises(NotImplementedError, match="num_beams must be 1..8"):
        LlavaDPOModel.beam_search(m, [torch.tensor([1, 2])], [None], 2, num_beams=9)
    # the three stages that stay closed
    omni = types.SimpleNamespace(cfg=types.SimpleNamespace(arch="omnilmm"))
    with pytest.raises(NotImplementedError):
        gen_data.generate_answers(omni, _tok(), ITEMS)
    with pytest.raises(NotImplementedError, match="OmniLMM"):
        vqa.answer_questions(omni, _tok(), ITEMS)
    with pytest.raises(NotImplementedError):
        gen_data.main(["--checkpoint", "x", "--ds_name", "y", "--answer_file", "z", "--num_beam", "3"])
