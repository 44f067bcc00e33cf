"""Host side of beam-search decoding: the float64 restatement of transformers' beam search (tests/beam_case.py) against the
reference's recorded runs (tests/golden/beam_tiny.pt), the cache-row planner, the three new C-ABI entry points (declared,
exported, bad arguments refused before any launch) and the record format of rlaif_v_amd.vqa on a stubbed model.  No GPU."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_case as BC  # noqa: E402

P = 0x7F0000010000          # an "operand": 64 KiB aligned, never dereferenced (every call below is refused before any launch)
Q = P + 0x100000            # a second one, 1 MiB behind


def _lib():
    from rlaif_v_amd import hip
    return hip.lib()


# ------------------------------------------------------------------------------------------------ restatement vs the reference
@pytest.mark.parametrize("run", ["a", "b"])
@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_restatement_reproduces_the_reference_from_its_recorded_logits(name, run):
    gold = BC.load_case()
    K, T = gold["num_beams"], gold["steps"]
    r = gold[name]["runs"][run]
    for k, rec in enumerate(r["prompts"]):
        lg = rec["logits"].numpy()
        g, steps = BC.beam_search64(lambda j, beams: lg[j], K, T, r["eos"])
        assert len(steps) == lg.shape[0], "the search stops at the step the reference stopped at"
        toks, score, bidx = g.best()
        assert toks == rec["sequences"].tolist() == rec["answer"].tolist()
        n = int((rec["beam_indices"] >= 0).sum())
        assert bidx == rec["beam_indices"][:n].tolist() and n == len(toks)
        assert abs(score - float(rec["sequences_scores"])) <= 1e-5
        assert np.array_equal(np.stack([s["parent"] for s in steps]), rec["parent"].numpy())
        assert np.array_equal(np.stack([s["token"] for s in steps]), rec["token"].numpy())
        assert np.allclose([s["margin_keep"] for s in steps], rec["margin_keep"].numpy(), rtol=0, atol=1e-9)


def test_fixture_covers_an_early_finish_and_an_early_stop():
    gold = BC.load_case()
    T = gold["steps"]
    for name in ("mha", "gqa"):
        a, b = gold[name]["runs"]["a"], gold[name]["runs"]["b"]
        assert all(r["answer"].numel() == T and r["logits"].shape[0] == T for r in a["prompts"])
        assert not any(int(a["eos"]) in r["token"].tolist() for r in a["prompts"])
        assert any(r["answer"].numel() < T and int(r["answer"][-1]) == b["eos"] for r in b["prompts"]), "a hypothesis finished early and won"
        assert any(r["logits"].shape[0] < T for r in b["prompts"]), "a search stopped before the last step"


def test_restatement_rules_on_planted_steps():
    """the finished set keeps the K best, rank >= K EOS candidates are ignored, the stop rule fires only with a full set"""
    K, T, eos, V = 2, 6, 5, 8
    g = BC.Group64(K, T, eos)
    # step 0: EOS is the best candidate (rank 0 < K): it finishes with score value / 1; the two running beams are the next two
    c = (np.array([-0.5, -1.0, -1.5, -2.0]), np.array([0, 0, 0, 0]), np.array([eos, 1, 2, 3]))
    s = g.step(None, c)
    assert s["token"].tolist() == [1, 2] and s["score"].tolist() == [-1.0, -1.5] and not s["done"]
    assert [h["tokens"] for h in g.hyps] == [[eos]] and g.hyps[0]["score"] == -0.5
    # step 1: EOS at rank 2 >= K is ignored by the finished set, and skipped by the running beams
    s = g.step(None, (np.array([-1.1, -1.2, -1.3, -1.4]), np.array([1, 0, 0, 1]), np.array([3, 4, eos, 6])))
    assert s["token"].tolist() == [3, 4] and s["parent"].tolist() == [1, 0] and len(g.hyps) == 1 and not s["done"]
    assert g.tokens == [[2, 3], [1, 4]] and g.bidx == [[0, 1], [0, 0]]
    # step 2: EOS at rank 1: score -3.0 / 3 = -1.0 fills the set; best running -2.9 / 3 > -1.0: not done (narrowly)
    s = g.step(None, (np.array([-2.9, -3.0, -3.1, -3.2]), np.array([0, 1, 0, 1]), np.array([1, eos, 2, 3])))
    assert [h["score"] for h in g.hyps] == [-0.5, -1.0] and not s["done"] and s["token"].tolist() == [1, 2]
    assert g.hyps[1]["tokens"] == [1, 4, eos] and g.hyps[1]["bidx"] == [0, 0, 1]
    # step 3: EOS at rank 0 with -3.6 / 4 = -0.9 evicts the worst (-1.0); best running -4.0 / 4 = -1.0 <= -0.9: done
    s = g.step(None, (np.array([-3.6, -4.0, -4.1, -4.2]), np.array([0, 1, 0, 1]), np.array([eos, 1, 2, 3])))
    assert [h["score"] for h in g.hyps] == [-0.5, -0.9] and s["done"]
    assert g.best()[0] == [eos] and g.best()[1] == -0.5
    # the last step: every candidate stops, the first K become hypotheses whatever their token
    g = BC.Group64(2, 1, None)
    s = g.step(np.log(np.array([[0.1, 0.2, 0.3, 0.4, 0.0001], [0.2] * 5])))
    assert s["done"] and [h["tokens"] for h in g.hyps] == [[3], [2]] and abs(g.hyps[0]["score"] - np.log(0.4 / 1.0001)) < 1e-12
    assert s["score"][0] < -9e8                               # what the reference's running top-k leaves behind
    # ties order by the lower flat index; a dead beam loses to every live candidate
    v, p, t = BC.topk_candidates(np.zeros((2, 4)), np.array([0.0, BC.DEAD]), 4)
    assert p.tolist() == [0, 0, 0, 0, 1] and t.tolist() == [0, 1, 2, 3, 0]
    v, p, t = BC.topk_candidates(np.zeros((2, 4)), np.array([0.0, 0.0]), 4)
    assert (p * 4 + t).tolist() == [0, 1, 2, 3, 4]


# ------------------------------------------------------------------------------------------------ cache rows
def test_plan_beam_rows_shared_prompts_and_step_major_own_rows():
    from rlaif_v_amd.splice import plan_beam_rows
    lens, K, T = [8, 12, 9], 3, 5
    off = [0, 8, 20]
    rows = plan_beam_rows(off, lens, K, T)
    n_pre, M = sum(lens), 9
    assert rows.n_seq == M and rows.n_rows == n_pre + M * T and rows.own_base == n_pre and rows.num_beams == K
    assert rows.prompt_of.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    assert rows.pre_off.tolist() == [0] * 3 + [8] * 3 + [20] * 3 and rows.pre_len.tolist() == [8] * 3 + [12] * 3 + [9] * 3
    owner = {}
    for j in range(T):
        pos, dst, own_len = rows.step(j)
        assert pos.tolist() == [lens[m // K] + j for m in range(M)] and own_len.tolist() == [j + 1] * M
        assert dst.tolist() == [n_pre + j * M + m for m in range(M)]                      # step-major
        for m in range(M):
            assert owner.setdefault(int(dst[m]), (m, j)) == (m, j) and n_pre <= int(dst[m]) < rows.n_rows
    assert len(owner) == M * T
    for t in (rows.prompt_of, rows.pre_off, rows.pre_len, rows.seq_idx):
        assert t.dtype == torch.int32
    assert rows.chunks == [(0, 9)]
    big = plan_beam_rows([0, 4] + [8 + 2 * i for i in range(28)], [4, 4] + [2] * 28, 5, 2)      # 150 sequences
    assert big.chunks == [(0, 60), (60, 120), (120, 150)] and all((c1 - c0) % 5 == 0 and c1 - c0 <= 64 for c0, c1 in big.chunks)
    assert plan_beam_rows([0], [4], 8, 3, max_rows=20).chunks == [(0, 8)]
    for bad in (dict(num_beams=0), dict(max_new=0), dict(max_rows=0), dict(num_beams=5, max_rows=4)):
        with pytest.raises(ValueError):
            plan_beam_rows([0], [4], **{**dict(num_beams=1, max_new=1), **bad})
    with pytest.raises(ValueError):
        plan_beam_rows([0], [0], 3, 1)
    with pytest.raises(ValueError):
        plan_beam_rows([0, 4], [4], 3, 1)
    with pytest.raises(ValueError):
        plan_beam_rows([], [], 3, 1)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_declared_and_exported_in_abi_7():
    lib = _lib()
    assert lib.lib.rv_abi_version() == 7
    ret, args = lib.decls["rv_beam_topk"]
    assert ret == "int" and [n for _, n in args] == ["logits", "ldl", "score", "G", "K", "V_valid", "cand_val", "cand_parent",
                                                     "cand_tok", "lse", "workspace", "workspace_floats", "stream"]
    ret, args = lib.decls["rv_beam_step"]
    assert ret == "int" and [n for _, n in args][:11] == ["cand_val", "cand_parent", "cand_tok", "G", "K", "T", "j", "eos_token_id",
                                                          "len_div", "last", "own_base"]
    ret, args = lib.decls["rv_attn_decode_indexed"]
    assert ret == "int" and [n for _, n in args] == ["q", "ldq", "kv", "ldkv", "kv_rows", "k_col0", "v_col0", "pre_off", "pre_len",
                                                     "own_rows", "ld_rows", "cur_own_len", "own_len", "out", "ldo", "lse", "M", "H",
                                                     "hd", "kv_group", "scale", "n_split", "workspace", "workspace_floats", "stream"]
    for name in ("rv_beam_topk", "rv_beam_topk_workspace_floats", "rv_beam_step", "rv_attn_decode_indexed"):
        assert hasattr(lib.lib, name)
    from rlaif_v_amd import ops, splice
    from rlaif_v_amd.model import LlavaDPOModel
    assert all(hasattr(ops, n) for n in ("beam_topk", "beam_step", "attn_decode_indexed"))
    assert hasattr(splice, "plan_beam_rows") and hasattr(LlavaDPOModel, "beam_search")
    assert lib.lib.rv_beam_topk_workspace_floats(2, 3) == 2 * 3 * 6 * 2
    assert lib.lib.rv_beam_topk_workspace_floats(2, 0) == 0 and lib.lib.rv_beam_topk_workspace_floats(2, 9) == 0


def _topk(**kw):
    a = dict(logits=P, ldl=512, score=P, G=2, K=3, V_valid=512, cand_val=P, cand_parent=P, cand_tok=P, lse=P, workspace=P,
             workspace_floats=1 << 20)
    a.update(kw)
    return _lib().lib.rv_beam_topk(*a.values(), None)


def test_beam_topk_refuses_bad_arguments():
    lib = _lib()
    assert _topk(K=0) == 1 and "1 <= K <= 8" in lib.last_error() and lib.last_error().startswith("rv_beam_topk")
    assert _topk(K=9) == 1 and "1 <= K <= 8" in lib.last_error()
    assert _topk(G=0) == 1
    assert _topk(V_valid=65537, ldl=65540) == 1 and "65536" in lib.last_error()
    assert _topk(V_valid=600) == 1 and "ldl >= V_valid" in lib.last_error()
    assert _topk(V_valid=5) == 1 and "2 K" in lib.last_error()
    for name in ("logits", "score", "cand_val", "cand_parent", "cand_tok", "lse", "workspace"):
        assert _topk(**{name: None}) == 1 and "NULL" in lib.last_error(), name
        assert _topk(**{name: P + 2}) == 1 and "aligned" in lib.last_error(), name
    assert _topk(workspace_floats=71) == 1 and "workspace" in lib.last_error()


def _step(**kw):
    a = dict(cand_val=P, cand_parent=P, cand_tok=P, G=2, K=3, T=12, j=4, eos_token_id=2, len_div=5.0, last=0, own_base=100,
             force_parent=None, force_token=None, force_score=None, run_score=P, parent=P, token=P, hist_a=P, hist_b=Q, rows_a=P,
             rows_b=Q, ld_t=12, hyp_tokens=P, hyp_len=P, hyp_score=P, n_hyp=P, done=P)
    a.update(kw)
    return _lib().lib.rv_beam_step(*a.values(), None)


def test_beam_step_refuses_bad_arguments():
    lib = _lib()
    assert _step(K=0) == 1 and "1 <= K <= 8" in lib.last_error() and lib.last_error().startswith("rv_beam_step")
    assert _step(K=9) == 1 and "1 <= K <= 8" in lib.last_error()
    assert _step(G=0) == 1
    assert _step(j=12) == 1 and "0 <= j < T" in lib.last_error()
    assert _step(j=-1) == 1
    assert _step(ld_t=11) == 1 and "ld_t" in lib.last_error()
    assert _step(last=1) == 1 and "last" in lib.last_error()
    assert _step(j=11, last=0) == 1 and "last" in lib.last_error()
    assert _step(len_div=0.0) == 1 and "len_div" in lib.last_error()
    assert _step(own_base=-1) == 1
    assert _step(own_base=2 ** 31 - 10) == 1 and "int32" in lib.last_error()
    for name in ("cand_val", "cand_parent", "cand_tok", "run_score", "parent", "token", "hist_a", "hist_b", "rows_a", "rows_b",
                 "hyp_tokens", "hyp_len", "hyp_score", "n_hyp", "done"):
        assert _step(**{name: None}) == 1 and "NULL" in lib.last_error(), name
    for name in ("cand_val", "run_score", "hist_a", "rows_b", "hyp_tokens", "done"):
        assert _step(**{name: (Q if name.endswith("_b") else P) + 2}) == 1 and "aligned" in lib.last_error(), name
    assert _step(force_parent=P) == 1 and "come together" in lib.last_error()
    assert _step(force_parent=P, force_token=P) == 1 and "come together" in lib.last_error()
    # aliased ping-pong buffers: the same buffer, and overlapping ones (G K ld_t int32 = 288 bytes)
    assert _step(hist_b=P) == 1 and "distinct" in lib.last_error()
    assert _step(rows_b=P) == 1 and "distinct" in lib.last_error()
    assert _step(hist_b=P + 284) == 1 and "distinct" in lib.last_error()
    assert _step(rows_a=Q + 4) == 1 and "distinct" in lib.last_error()


def _attn_idx(**kw):
    H, hd = 4, 128
    a = dict(q=P, ldq=H * hd, kv=P, ldkv=2 * H * hd, kv_rows=100, k_col0=0, v_col0=H * hd, pre_off=P, pre_len=P, own_rows=P,
             ld_rows=12, cur_own_len=5, own_len=P, out=P, ldo=H * hd, lse=None, M=6, H=H, hd=hd, kv_group=2, scale=0.1, n_split=1,
             workspace=P, workspace_floats=1 << 20)
    a.update(kw)
    return _lib().lib.rv_attn_decode_indexed(*a.values(), None)


def test_attn_decode_indexed_refuses_bad_arguments():
    lib = _lib()
    assert _attn_idx(hd=64) == 1 and "hd must be 128" in lib.last_error() and lib.last_error().startswith("rv_attn_decode_indexed")
    assert _attn_idx(ld_rows=4) == 1 and "ld_rows" in lib.last_error()
    assert _attn_idx(cur_own_len=-1) == 1
    assert _attn_idx(kv_rows=0) == 1 and "kv_rows" in lib.last_error()
    assert _attn_idx(own_rows=None) == 1 and "NULL" in lib.last_error()
    assert _attn_idx(own_rows=P + 2) == 1 and "aligned" in lib.last_error()
    assert _attn_idx(q=P + 8) == 1 and "16-byte aligned" in lib.last_error()
    assert _attn_idx(kv_group=3) == 1
    assert _attn_idx(n_split=0) == 1 and "n_split" in lib.last_error()
    assert _attn_idx(M=0) == 1
    assert _attn_idx(workspace_floats=7) == 1 and "workspace" in lib.last_error()
    for name in ("q", "kv", "out", "pre_off", "pre_len", "own_len", "workspace"):
        assert _attn_idx(**{name: None}) == 1 and "NULL" in lib.last_error(), name


# ------------------------------------------------------------------------------------------------ vqa records
def _tok():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from toy_tokenizer import ToyTokenizer

    class Tok(ToyTokenizer):
        def decode(self, ids, skip_special_tokens=True):
            return " " + " ".join(f"t{int(i)}" for i in ids if not (skip_special_tokens and int(i) in (0, 1, 2))) + " "
    return Tok()


def _stub():
    calls = []

    def beam_search(prompts, images, max_new_tokens, num_beams=3, eos_token_id=None, length_penalty=1.0, return_trace=False):
        calls.append(dict(kind="beam", n=len(prompts), max_new_tokens=max_new_tokens, num_beams=num_beams, eos=eos_token_id))
        assert all(int((p == -200).sum()) == 1 and int(p[0]) == 1 for p in prompts)
        return [[10 * len(calls) + k, 7, 2] for k in range(len(prompts))], [-1.0] * len(prompts)

    def generate(prompts, images, max_new_tokens, repeat=1, temperature=0.0, top_p=1.0, repetition_penalty=1.0, eos_token_id=None,
                 generator=None, return_scores=False):
        calls.append(dict(kind="generate", n=len(prompts), temperature=temperature, top_p=top_p, repeat=repeat))
        return [[[50 + k, 2]] for k in range(len(prompts))]
    model = types.SimpleNamespace(cfg=types.SimpleNamespace(arch="llava", n_image_tokens=2), generate=generate, beam_search=beam_search)
    return model, calls


def test_answer_questions_records_on_a_stubbed_model():
    from rlaif_v_amd import vqa
    img = torch.zeros(3, 4, 4)
    lines = [dict(question="What is shown ?", image=img, image_id="im0"),
             dict(question="Describe the scene .", image=img, metainfos={"image_url": "http://x/1.jpg"}),
             dict(question="How many apples ?", image=img, image_id=17, image_url="unused")]
    model, calls = _stub()
    recs = vqa.answer_questions(model, _tok(), lines, num_beams=3, temperature=0.0, max_new_tokens=9, prompts_per_call=2)
    assert [(c["kind"], c["n"], c["num_beams"], c["max_new_tokens"], c["eos"]) for c in calls] == [("beam", 2, 3, 9, 2), ("beam", 1, 3, 9, 2)]
    assert all(list(r) == ["question_id", "image_id", "prompt", "text", "model_id"] for r in recs)
    assert [r["question_id"] for r in recs] == [0, 1, 2] and [r["image_id"] for r in recs] == ["im0", "http://x/1.jpg", 17]
    assert [r["text"] for r in recs] == ["t10 t7", "t11 t7", "t20 t7"] and recs[1]["prompt"] == "Describe the scene ."
    assert all(r["model_id"] == "llava-v1.5-7b" for r in recs)
    # num_beams == 1 goes to generate (greedy or sampling)
    model, calls = _stub()
    recs = vqa.answer_questions(model, _tok(), lines, num_beams=1, temperature=0.2, top_p=0.9, max_new_tokens=9)
    assert [(c["kind"], c["temperature"], c["top_p"], c["repeat"]) for c in calls] == [("generate", 0.2, 0.9, 1)]
    assert [r["text"] for r in recs] == ["t50", "t51", "t52"]
    # beams with temperature > 0 is beam-sample: refused by name
    with pytest.raises(NotImplementedError, match="beam-sample"):
        vqa.answer_questions(model, _tok(), lines, num_beams=3, temperature=0.2)
    with pytest.raises(NotImplementedError, match="OmniLMM"):
        vqa.answer_questions(types.SimpleNamespace(cfg=types.SimpleNamespace(arch="omnilmm")), _tok(), lines)


def test_vqa_command_line_accepts_the_eval_scripts_flags():
    from rlaif_v_amd import vqa
    args = vqa.build_parser().parse_args(["--model-path", "m", "--question-file", "q", "--answers-file", "a", "--temperature", "0",
                                          "--num_beam", "3"])
    assert args.num_beams == 3 and args.temperature == 0 and args.max_new_tokens == 1024 and args.conv_mode == "llava_v1"
    args = vqa.build_parser().parse_args(["--model-path", "m", "--question-file", "q", "--answers-file", "a"])
    assert args.num_beams == 3 and args.temperature == 0.2 and args.top_p is None and (args.num_chunks, args.chunk_idx) == (1, 0)
    with pytest.raises(NotImplementedError, match="beam-sample"):
        vqa.main(["--model-path", "m", "--question-file", "q", "--answers-file", "a", "--num_beam", "3"])       # default 0.2
    assert vqa.get_chunk(list(range(7)), 3, 2) == [6] and vqa.get_chunk(list(range(7)), 3, 0) == [0, 1, 2]
