"""The text-only language model on the GPU (rlaif_v_amd.textlm, LlavaDPOModel.generate with images=None, two end-of-sequence ids,
the wide sampler behind a vocabulary above 65536, rlaif_v_amd.divide end to end) on the tiny Llama of tests/divide_case.py.

tests/golden/text_generate_tiny.pt (make_text_generate_golden.py): what transformers' own ``LlamaForCausalLM.generate`` returned,
greedy, for a left-padded batch of three prompts of different lengths - sequences, per-step logits, top-1 / top-2 gaps, and the
run with two EOS ids.  Protocol of tests/test_generate_gpu.py: teacher-forced cached logits within twice the error of the existing
no-cache forward against ``oracle.dpo_oracle.llama_logits``, greedy tokens equal at every step whose gap exceeds twice that error."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import divide_case as DC  # noqa: E402
import generate_case as GC  # noqa: E402
from oracle import dpo_oracle as O  # noqa: E402

_STATE = {}
WIDE_V = 66048


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _tiny():
    """the fixture's model, its oracle logits, the teacher-forced cached run, the no-cache prefills and the free greedy run:
    computed once, shared, never modified"""
    if "tiny" not in _STATE:
        gold = torch.load(DC.GOLD_TEXT, weights_only=True)
        assert gold["cfg"] == dict(DC.TINY, vocab=1024)
        W = DC.tiny_text_weights(1024, gold["seed"], gold["std"], gold["head_scale"])
        model = DC.tiny_text_model(W, 1024)
        prompts, seqs, T = gold["prompts"], gold["free_sequences"], gold["steps"]
        ocfg = O.LlavaCfg(vocab=1024, **DC.TINY)
        rows = []
        with torch.no_grad():
            for k, p in enumerate(prompts):
                ids = torch.cat([p, seqs[k, :T - 1].long()])
                rows.append(O.llama_logits(W["model.embed_tokens.weight"][ids][None], W, ocfg)[0][p.numel() - 1:].float())
        oracle = torch.stack(rows)                                                           # [3, T, V]
        forced_out, forced = model.generate(prompts, None, T, _forced_tokens=seqs, return_scores=True)
        nocache = []
        for j in range(T):
            ext = [torch.cat([p, seqs[k, :j].to(p.dtype)]) for k, p in enumerate(prompts)]
            nocache.append(model._prefill(ext, None)[:len(prompts), :1024].cpu())
        greedy, greedy_scores = model.generate(prompts, None, T, return_scores=True)
        _STATE["tiny"] = dict(gold=gold, W=W, model=model, oracle=oracle, forced_out=forced_out, forced=forced.cpu().transpose(0, 1),
                              nocache=torch.stack(nocache, 1), greedy=greedy, greedy_scores=greedy_scores.cpu(), T=T)
    return _STATE["tiny"]


def _errors(st):
    return float((st["nocache"] - st["oracle"]).abs().max()), float((st["forced"] - st["oracle"]).abs().max())


def test_teacher_forced_logits_within_twice_the_no_cache_error():
    _need_gpu()
    st = _tiny()
    e_nc, e_c = _errors(st)
    e_ref = float((st["forced"] - st["gold"]["scores"]).abs().max())
    print(f"[text] max |logit - oracle| over {st['oracle'].numel()} logits: no-cache prefill per step {e_nc:.4e}, KV-cached {e_c:.4e} "
          f"(bar {2 * e_nc:.4e}); KV-cached against LlamaForCausalLM.generate's logits {e_ref:.4e}")
    assert torch.isfinite(st["forced"]).all()
    assert e_nc > 0
    assert e_c <= 2 * e_nc
    assert e_ref <= 2 * e_nc + 1e-4                       # the oracle reproduces transformers to 1e-4 (stored: oracle_vs_hf)
    assert st["gold"]["oracle_vs_hf"] <= 1e-4
    assert [s[0] for s in st["forced_out"]] == st["gold"]["free_sequences"].tolist()
    assert torch.equal(st["forced"][:, 0], st["nocache"][:, 0])      # step 0 is the prefill itself: the existing forward's bits


def test_greedy_tokens_equal_transformers_generate_with_two_eos_ids():
    """the recorded run with eos_token_id = [e1, e2]: prompt 0 stops at e1, prompt 1 later at e2, prompt 2 runs to the end; every
    step whose recorded gap exceeds twice the measured no-cache error must give the recorded token (at most 10 % skipped)"""
    _need_gpu()
    st = _tiny()
    gold, T = st["gold"], st["T"]
    e_nc, _ = _errors(st)
    out = st["model"].generate(gold["prompts"], None, T, eos_token_id=gold["eos_ids"])
    gaps, want = gold["gaps"], gold["sequences"]
    assert [len(w) for w in want] == [gold["eos_steps"][0] + 1, gold["eos_steps"][1] + 1, T]
    assert gold["min_compared_gap"] > 2 * gold["gap_bar"]         # the generator's seed condition, stored with the fixture
    skipped = total = 0
    for k, seq in enumerate(want):
        got = out[k][0]
        lost = False
        for j in range(len(seq)):
            total += 1
            if lost or not float(gaps[k, j]) > 2 * e_nc:
                skipped += 1
                lost = lost or j >= len(got) or got[j] != seq[j]
                continue
            assert j < len(got) and got[j] == seq[j], f"prompt {k} step {j}: {got[:j + 1]}, transformers generated {seq[j]}"
        if not lost:
            assert got == seq, f"prompt {k}: cut behind its own end-of-sequence id"
    print(f"[text] greedy, two EOS ids {gold['eos_ids']}: {total - skipped} of {total} steps compared (smallest gap "
          f"{float(gaps.min()):.3e}, 2 x no-cache error {2 * e_nc:.3e})")
    assert skipped <= 0.1 * total


def test_two_eos_ids_cut_each_sequence_behind_its_own():
    """_forced_tokens plants id A in sequence 0 at step 3 and id B in sequence 1 at step 6: each is cut behind its own id, the third
    runs to max_new_tokens; an int eos_token_id gives what it gave before"""
    _need_gpu()
    st = _tiny()
    model, gold, T = st["model"], st["gold"], st["T"]
    A, B = 1001, 1002
    forced = gold["free_sequences"].clone()
    assert not bool(((forced == A) | (forced == B)).any())
    forced[0, 3], forced[1, 6], forced[0, 8] = A, B, B
    out = model.generate(gold["prompts"], None, T, eos_token_id=[A, B], _forced_tokens=forced)
    f = forced.tolist()
    assert out[0][0] == f[0][:4] and out[1][0] == f[1][:7] and out[2][0] == f[2] and len(out[2][0]) == T
    assert model.generate(gold["prompts"], None, T, eos_token_id=(B, A), _forced_tokens=forced) == out
    one = model.generate(gold["prompts"], None, T, eos_token_id=B, _forced_tokens=forced)
    assert one[0][0] == f[0][:9] and one[1][0] == f[1][:7] and one[2][0] == f[2]
    assert model.generate(gold["prompts"], None, T, eos_token_id=[B], _forced_tokens=forced) == one
    # everything finished before the end: the loop stops at a multiple of 8 steps and the cut is the same
    forced[2, 2] = A
    short = model.generate(gold["prompts"], None, T, eos_token_id=[A, B], _forced_tokens=forced)
    assert [len(s[0]) for s in short] == [4, 7, 3]


def _wide():
    if "wide" not in _STATE:
        W = DC.tiny_text_weights(WIDE_V, seed=5, std=0.05, head_scale=4.0)
        model = DC.tiny_text_model(W, WIDE_V)
        g = torch.Generator().manual_seed(9)
        prompts = [torch.cat([torch.tensor([1]), torch.randint(8, WIDE_V, (n,), generator=g)]) for n in (4, 11, 7)]
        _STATE["wide"] = (model, prompts)
    return _STATE["wide"]


def test_vocab_66048_reaches_the_wide_sampler(monkeypatch):
    _need_gpu()
    from rlaif_v_amd import ops
    model, prompts = _wide()
    T, calls = 6, []
    real_wide, real_reg = ops.sample_token_wide, ops.sample_token
    monkeypatch.setattr(ops, "sample_token_wide", lambda *a, **kw: (calls.append("wide"), real_wide(*a, **kw))[1])
    monkeypatch.setattr(ops, "sample_token", lambda *a, **kw: (calls.append("reg"), real_reg(*a, **kw))[1])
    # greedy with a repetition penalty: every token is the lowest-index argmax of its own step's penalised logits
    pen = 1.5
    out, scores = model.generate(prompts, None, T, repetition_penalty=pen, return_scores=True)
    assert calls == ["wide"] * T
    scores = scores.cpu()
    assert scores.shape == (T, 3, WIDE_V) and float(scores.max() - scores.min()) > 6.0, "logits spread over several units"
    s64 = scores.double().numpy()
    for k in range(3):
        got = out[k][0]
        assert len(got) == T
        for j in range(T):
            x = GC.penalised(s64[j, k], got[:j] if j else None, float(np.float32(pen)))
            top = np.sort(x)[-2:]
            if top[1] - top[0] > 2 * GC.U32 * np.abs(s64[j, k]).max():            # else one fp32 rounding decides: not compared
                assert got[j] == int(x.argmax()), f"prompt {k} step {j}"
    # planted uniforms at T = 0.2, top-p = 0.9: every token is ops.sample_token_wide alone on that step's logits
    del calls[:]
    u = torch.rand(T, 3, generator=torch.Generator().manual_seed(3))
    out, scores = model.generate(prompts, None, T, temperature=0.2, top_p=0.9, repetition_penalty=1.3, _uniforms=u, return_scores=True)
    assert calls == ["wide"] * T
    dev = scores.device
    for j in range(T):
        for k in range(3):
            row = torch.zeros(1, WIDE_V, device=dev)
            row.copy_(scores[j, k])
            seen = None
            if j:
                ids = torch.tensor(out[k][0][:j], dtype=torch.int32, device=dev)
                seen = (torch.tensor([0, j], dtype=torch.int32, device=dev), ids)
            tok, _ = real_wide(row, 1, WIDE_V, u[j, k:k + 1].to(dev).contiguous(), 0.2, 0.9, seen=seen, penalty=1.3)
            assert int(tok[0]) == out[k][0][j], f"step {j} prompt {k}"
    # the same seed gives the same tokens, another seed other ones
    runs = [model.generate(prompts, None, T, temperature=0.7, top_p=0.9, generator=torch.Generator().manual_seed(s)) for s in (11, 11, 12)]
    assert runs[0] == runs[1] and runs[0] != runs[2]


def test_images_and_text_models_do_not_mix():
    _need_gpu()
    st = _tiny()
    model, gold = st["model"], st["gold"]
    with pytest.raises(ValueError, match="text-only model .* takes images=None"):
        model.generate(gold["prompts"], torch.zeros(3, 3, 56, 56), 2)
    bad = [torch.cat([gold["prompts"][0], torch.tensor([-200])])]
    with pytest.raises(ValueError, match="image placeholder"):
        model.generate(bad, None, 2)
    with pytest.raises(NotImplementedError, match="TextLMModel.forward_logps: training a text-only model"):
        model.forward_logps(None, None, None)
    with pytest.raises(NotImplementedError, match="training a text-only model"):
        model.train()
    assert model.encode_images(None).shape == (0, 256)
    from rlaif_v_amd.model import LlavaConfig, LlavaDPOModel
    cfg = O.tiny_cfg()
    llava = LlavaDPOModel(LlavaConfig(**O.asdict(cfg)), with_optimizer=False)
    with pytest.raises(ValueError, match="images=None needs a text-only model"):
        llava.generate([torch.tensor([1, -200, 5])], None, 2)


def test_divide_end_to_end_on_the_tiny_model(tmp_path):
    """rlaif_v_amd.divide.run with the tiny model as both checkpoints and the stub tokenizer: the three files, the record keys and
    their order, the answers those of a direct generate call with the stage's sampling settings, and resume"""
    _need_gpu()
    from rlaif_v_amd import divide
    st = _tiny()
    model = st["model"]
    items = [{"question_id": i, "raw_question": f"What is item {i} ?", "answer": f"It shows thing {i} and thing {i + 1} .",
              "metainfos": {"image_path": f"img/{i}.jpg", "ds_question_id": 40 + i}} for i in range(5)]
    src = tmp_path / "answers.jsonl"
    src.write_text("".join(json.dumps(d) + "\n" for d in items))
    toks = []

    def load(name):
        toks.append(DC.StubTokenizer(1024))
        return model, toks[-1]
    p_div, p_gq, p_qas = divide.run(str(src), load, "div", "chg", bs=2, seed=5)
    assert [os.path.basename(p) for p in (p_div, p_gq, p_qas)] == [
        "answers.s0-e-1.chunk1-0.llama3-8b_divide.jsonl", "answers.s0-e-1.chunk1-0.llama3-8b_divide.gq.jsonl",
        "answers.s0-e-1.chunk1-0.llama3-8b_divide.gq.qas.jsonl"]
    div = [json.loads(line) for line in open(p_div)]
    gq = [json.loads(line) for line in open(p_gq)]
    qas = [json.loads(line) for line in open(p_qas)]
    assert len(div) == len(gq) == 5 and [r["question_id"] for r in gq] == list(range(5))
    assert list(div[0]) == ["question_id", "raw_question", "answer", "metainfos", "raw_facts", "facts"]
    assert list(gq[0]) == list(div[0]) + ["raw_changed_facts", "changed_facts"]
    assert all(r["facts"] == divide.get_facts(r["raw_facts"]) and isinstance(r["facts"], list) and r["facts"] for r in gq)
    assert len(qas) == sum(min(len(r["facts"]), len(r["changed_facts"])) for r in gq)
    assert all(list(q) == ["question_id", "ds_question_id", "image_path", "question", "metainfos"] for q in qas)
    # the divide stage's first call, made directly: the stage's sampling settings, the seeded generator, two EOS ids
    tok = DC.StubTokenizer(1024)
    prompts = [divide.prompt_ids(tok, divide.divide_messages(it)) for it in items[:2]]
    assert all(p[:2].tolist() == [1, 1] for p in prompts), "the template's BOS and the tokenizer's"
    direct = model.generate(prompts, None, max_new_tokens=256, temperature=0.2, top_p=0.9, eos_token_id=[2, 3],
                            generator=torch.Generator().manual_seed(5))
    assert [r["raw_facts"] for r in div[:2]] == [tok.decode(direct[k][0]) for k in range(2)]
    # resume: the answer file cut back to 3 lines, the run appends the 2 that are missing and leaves the 3 alone
    kept = open(p_div).read().splitlines(keepends=True)[:3]
    open(p_div, "w").write("".join(kept))
    n_before = len(toks[0].templated)
    recs = divide.batch_inference(model, toks[0], str(src), p_div, "facts", divide.divide_messages, batch_size=2, seed=5)
    assert len(toks[0].templated) == n_before + 2 and "item 3" in toks[0].templated[n_before]
    lines = open(p_div).read().splitlines(keepends=True)
    assert lines[:3] == kept and len(lines) == 5 and [r["question_id"] for r in recs] == list(range(5))
