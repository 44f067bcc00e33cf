"""OmniLMM candidate generation on the GPU (OmniLMMDPOModel.generate / generate_continuous / beam_search,
rlaif_v_amd.omnilmm_gen_data) on the tiny OmniLMM configuration (autocheck_case.omni_cfgs), tower tokens as images, T = 12,
against tests/golden/omnilmm_generate_tiny.pt: the reference model's greedy decoding at repetition_penalty = 1.1 of three
prompts of different lengths (make_omnilmm_generate_golden.py).

CPU oracle of a step: ``oracle.omnilmm_oracle.resampler_forward`` + ``omnilmm_splice`` + ``oracle.dpo_oracle.llama_logits`` on
prompt + tokens so far, fp32, no cache (a helper of this file; oracle/ is unchanged).

Bars, the rule of tests/test_generate_gpu.py: the teacher-forced KV-cached logits are held to 2 x the error of the existing
NO-CACHE path (a prefill of prompt + tokens so far) against the same oracle on the same sequences, measured here and printed;
against the fixture 2 x that + 1e-4.  A greedy token is compared on every step whose recorded gap exceeds 2 x that error; at most
10 % of the steps may be skipped."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import autocheck_case as AC  # noqa: E402
import beam_penalty_case as PC  # noqa: E402
from oracle import dpo_oracle as O  # noqa: E402
from oracle import omnilmm_oracle as OO  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "omnilmm_generate_tiny.pt")
U32 = 2.0 ** -24
_STATE = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _weights(ocfg, seed, std):
    W = {k: v for k, v in O.make_weights(ocfg, seed=seed, std=std).items() if "vision_tower" not in k and "mm_projector" not in k}
    W.update(OO.make_resampler_weights(ocfg.hidden, AC.OMNI_KV, AC.OMNI_NQ))
    return W


def _oracle_step_logits(ocfg, W, tower, prompts, seqs):
    """[n_prompts, T, V]: last-position logits behind prompt k + seqs[k][:j]"""
    with torch.no_grad():
        feats = OO.resampler_forward(tower, W, AC.OMNI_RS_HEADS)
        out = []
        for k, p in enumerate(prompts):
            rows = []
            for j in range(len(seqs[k])):
                ids = torch.cat([p, torch.tensor(seqs[k][:j], dtype=p.dtype)])
                emb = OO.omnilmm_splice(ids[None], W["model.embed_tokens.weight"], feats[k:k + 1], *AC.OMNI_TOKENS)
                rows.append(O.llama_logits(emb, W, ocfg)[0, -1].float())
            out.append(torch.stack(rows))
    return torch.stack(out)


def _setup():
    """Model, fixture, oracle, the teacher-forced cached run, the no-cache prefills and the free greedy run: computed once, shared,
    never modified."""
    if not _STATE:
        from rlaif_v_amd.omnilmm import OmniLMMDPOModel
        gold = torch.load(GOLD, weights_only=True)
        cfg, ocfg = AC.omni_cfgs()
        assert O.asdict(ocfg) == gold["cfg"] and tuple(gold["tokens"]) == AC.OMNI_TOKENS and gold["num_query"] == AC.OMNI_NQ
        W = _weights(ocfg, gold["weight_seed"], gold["std"])
        model = OmniLMMDPOModel(cfg, with_optimizer=False)
        model.load_state_dict(W)
        prompts, tower, seqs, T, pen = gold["prompts"], gold["tower"], gold["sequences"], gold["steps"], gold["penalty"]
        oracle = _oracle_step_logits(ocfg, W, tower, prompts, seqs.tolist())
        forced_out, forced = model.generate(prompts, tower, T, repetition_penalty=pen, _forced_tokens=seqs, return_scores=True)
        nocache = []
        for j in range(T):
            ext = [torch.cat([p, seqs[k, :j].to(p.dtype)]) for k, p in enumerate(prompts)]
            nocache.append(model._prefill(ext, tower)[:len(prompts), :cfg.vocab].cpu())
        greedy, greedy_scores = model.generate(prompts, tower, T, repetition_penalty=pen, return_scores=True)
        _STATE.update(gold=gold, cfg=cfg, ocfg=ocfg, W=W, model=model, prompts=prompts, tower=tower, T=T, pen=pen, oracle=oracle,
                      forced_out=forced_out, forced=forced.cpu().transpose(0, 1), nocache=torch.stack(nocache, 1), greedy=greedy,
                      greedy_scores=greedy_scores.cpu())
    return _STATE


def _errors(st):
    return float((st["nocache"] - st["oracle"]).abs().max()), float((st["forced"] - st["oracle"]).abs().max())


def test_teacher_forced_logits_within_twice_the_no_cache_error():
    _need_gpu()
    st = _setup()
    e_nc, e_c = _errors(st)
    e_ref = float((st["forced"] - st["gold"]["logits"]).abs().max())
    print(f"[omnilmm] max |logit - oracle| over {st['oracle'].numel()} logits: no-cache prefill per step {e_nc:.4e}, KV-cached "
          f"{e_c:.4e} (bar {2 * e_nc:.4e}); KV-cached against the reference model's logits {e_ref:.4e}; "
          f"generate_ran={st['gold']['generate_ran']}")
    assert torch.isfinite(st["forced"]).all()
    assert e_nc > 0
    assert e_c <= 2 * e_nc
    assert e_ref <= 2 * e_nc + 1e-4                       # the oracle reproduces the reference to 1e-4
    assert [s[0] for s in st["forced_out"]] == st["gold"]["sequences"].tolist()     # forced tokens come back as the output
    assert torch.equal(st["forced"][:, 0], st["nocache"][:, 0]), "step 0 is the prefill itself: the existing forward's bits"


def test_greedy_tokens_equal_the_reference():
    _need_gpu()
    st = _setup()
    e_nc, _ = _errors(st)
    gaps, want = st["gold"]["gaps"], st["gold"]["sequences"].tolist()
    assert float(gaps.min()) > 2 * st["gold"]["gap_bar"]          # the generator's seed condition, stored with the fixture
    assert any(st["gold"]["differs"]), "without the penalty the reference decodes other tokens"
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
    print(f"[omnilmm] greedy at penalty {st['pen']}: {total - skipped} of {total} steps compared (smallest recorded gap "
          f"{float(gaps.min()):.3e}, 2 x no-cache error {2 * e_nc:.3e})")
    assert skipped <= 0.1 * total


BUDGETS = [12, 5, 9, 12, 3]
REPEAT = 2
SAMPLING = dict(temperature=0.7, top_p=0.95, repetition_penalty=1.1)


def _planted(index):
    return torch.rand(12, REPEAT, generator=torch.Generator().manual_seed(2000 + index))


def test_continuous_batching_equals_generate_run_alone():
    """tokens and per-step logits, bit for bit, at slots 2 and 5 and in two arrival orders, with the penalty on"""
    _need_gpu()
    st = _setup()
    model, prompts, tower, T = st["model"], st["prompts"], st["tower"], st["T"]
    longest = max(int(p.numel()) for p in prompts)                  # the replacement splice keeps the length
    reqs = [(prompts[i % 3], tower[i % 3], BUDGETS[i]) for i in range(len(BUDGETS))]
    alone = []
    for i, (p, tw, budget) in enumerate(reqs):
        toks, scores = model.generate([p], tw[None], budget, repeat=REPEAT, _uniforms=_planted(i)[:budget], return_scores=True, **SAMPLING)
        alone.append((toks[0], scores.cpu()))
    assert len({tuple(t) for toks, _ in alone for t in toks}) > len(BUDGETS), "the samples of a request differ somewhere"
    compared = 0
    for slots, order in ((2, [0, 1, 2, 3, 4]), (5, [0, 1, 2, 3, 4]), (2, [4, 3, 2, 1, 0]), (5, [3, 0, 4, 2, 1])):
        rows = {}
        got = dict(model.generate_continuous((reqs[i] for i in order), T, slots=slots, repeat=REPEAT, max_prompt_tokens=longest,
                                             poll_every=4, _uniforms=_planted, request_indices=order,
                                             _scores=lambda i, r, j, row: rows.setdefault((i, r), {}).setdefault(j, row.cpu()), **SAMPLING))
        assert sorted(got) == sorted(order)
        for i, (toks, scores) in enumerate(alone):
            for r in range(REPEAT):
                assert got[i][r] == toks[r], f"slots {slots} order {order}: request {i} sample {r}"
                for j in range(BUDGETS[i]):
                    assert torch.equal(rows[(i, r)][j], scores[j, r]), f"slots {slots}: request {i} sample {r} step {j}: the logits"
                    compared += 1
    print(f"[omnilmm] continuous batching: {compared} logit rows bit-equal with generate() run alone")


def test_beam_search_selects_as_the_restatement_on_its_own_logits():
    _need_gpu()
    st = _setup()
    model, prompts, tower, T, V = st["model"], st["prompts"], st["tower"], st["T"], st["cfg"].vocab
    K, pen = 3, PC.f32(st["pen"])
    G, n = len(prompts), 2 * K
    tokens, scores, tr = model.beam_search(prompts, tower, T, num_beams=K, repetition_penalty=st["pen"], return_trace=True)
    tr = {k: v.cpu() for k, v in tr.items()}
    steps = tr["logits"].shape[0]
    undecided = total = penalised = 0
    for g in range(G):
        ref = PC.Group64(K, T, None, penalty=pen)
        sl = slice(g * K, (g + 1) * K)
        total += steps
        for j in range(steps):
            lg = tr["logits"][j, sl].numpy()
            cand = (tr["cand_val"][j, g].double().numpy(), tr["cand_parent"][j, g].numpy(), tr["cand_tok"][j, g].numpy())
            v64, e64 = PC.penalised_bound(lg, ref.run_score, ref.tokens, pen)
            fv, fe = v64.reshape(-1), e64.reshape(-1)
            order = np.lexsort((np.arange(fv.shape[0]), -fv))[:n + 1]
            gaps, need = fv[order][:-1] - fv[order][1:], fe[order][:-1] + fe[order][1:]
            penalised += sum(int(t) in ref.tokens[int(p)] for p, t in zip(order[:n] // V, order[:n] % V))
            if bool((gaps > need).all()):
                assert cand[1].tolist() == (order[:n] // V).tolist() and cand[2].tolist() == (order[:n] % V).tolist(), \
                    f"prompt {g} step {j}: the device's candidates are not float64's (smallest gap {gaps.min():.3e})"
                assert np.abs(cand[0] - fv[order][:n]).max() <= fe[order].max() + U32 * np.abs(fv[order][:n]).max()
            else:
                undecided += 1
            s = ref.step(None, cand)
            what = f"prompt {g} step {j}"
            assert tr["parent"][j, sl].tolist() == s["parent"].tolist() and tr["token"][j, sl].tolist() == s["token"].tolist(), what
            assert np.allclose(tr["score"][j, sl].numpy(), s["score"], rtol=2 * U32, atol=0), what
        toks, score, _ = ref.best()
        assert tokens[g] == toks and abs(scores[g] - score) <= 4 * U32 * abs(score), f"prompt {g}: final answer / sequences_scores"
    print(f"[omnilmm] beam search at penalty {st['pen']}: {total - undecided} of {total} steps decided by float64; {penalised} penalised "
          f"candidates among the selected")
    assert undecided <= 0.1 * total and penalised > 0
    # step 0 is the prefill's logits for every beam, and a prompt's result does not change with its neighbours in the call
    for g in (0, 2):
        t1, s1, tr1 = model.beam_search(prompts[g:g + 1], tower[g:g + 1], T, num_beams=K, repetition_penalty=st["pen"], return_trace=True)
        assert t1[0] == tokens[g] and s1[0] == scores[g]
        assert torch.equal(tr1["logits"].cpu(), tr["logits"][:, g * K:(g + 1) * K]) and torch.equal(tr1["token"].cpu(), tr["token"][:, g * K:(g + 1) * K])
    plain, _ = model.beam_search(prompts, tower, T, num_beams=K)
    assert plain != tokens, "the penalty changes an answer of this case"


def test_tower_tokens_and_a_registered_tower_give_the_same_bits():
    _need_gpu()
    st = _setup()
    model, prompts, tower, T = st["model"], st["prompts"], st["tower"], st["T"]
    pixels = torch.arange(len(prompts), dtype=torch.float32).reshape(-1, 1, 1, 1).expand(-1, 3, 8, 8).contiguous()
    seen = []

    def fake_tower(px):                                            # pixels [B, 3, H, W] -> tower tokens: image b is tower[b]
        seen.append(tuple(px.shape))
        return tower[px[:, 0, 0, 0].long().cpu()]
    model.set_vision_tower(fake_tower)
    try:
        out, scores = model.generate(prompts, pixels, T, repetition_penalty=st["pen"], return_scores=True)
        bt, bs = model.beam_search(prompts, pixels, 4, num_beams=3, repetition_penalty=st["pen"])
    finally:
        model.set_vision_tower(None)
    assert seen and all(s == (len(prompts), 3, 8, 8) for s in seen)
    assert out == st["greedy"] and torch.equal(scores.cpu(), st["greedy_scores"])
    assert (bt, bs) == model.beam_search(prompts, tower, 4, num_beams=3, repetition_penalty=st["pen"])
    with pytest.raises(NotImplementedError, match="vision tower"):
        model.generate(prompts, pixels, 2)


class _Tok:
    def __new__(cls):
        from toy_tokenizer import OmniToyTokenizer
        pt, st, en = AC.OMNI_TOKENS

        class Tok(OmniToyTokenizer):
            eos_token_id = None                            # the random tiny model would emit it at random
            SPECIAL = dict(OmniToyTokenizer.SPECIAL, **{"<im_start>": st, "<im_end>": en, "<im_patch>": pt})

            def encode(self, text, add_special_tokens=True):
                ids = [self.bos_token_id] if add_special_tokens else []
                for p in self._pieces(text):               # words stay below the image tokens of the 325-id vocabulary
                    ids.append(self.SPECIAL[p] if p in self.SPECIAL else 10 + (sum(ord(c) * (i + 1) for i, c in enumerate(p)) % 300))
                return ids

            def decode(self, ids, skip_special_tokens=True):
                return " " + " ".join(f"t{int(i)}" for i in ids if not (skip_special_tokens and int(i) in (0, 1, 2))) + " "
        return Tok()


def test_gen_data_records_from_a_jsonl(tmp_path):
    """two question lines with PNGs through autocheck.read_gen_dataset + omnilmm_gen_data.generate_answers, both branches: the
    reference's record keys in its order, answers equal to the decode of the direct calls.  The images reach the model as raw
    uint8 pixels; a registered stand-in tower (image n is 60 + 8 n pixels high) hands out the fixture's tower tokens."""
    _need_gpu()
    from PIL import Image
    from rlaif_v_amd import autocheck
    from rlaif_v_amd import omnilmm_gen_data as G
    from rlaif_v_amd.omni_data import wrap_question_for_omni_lmm
    st = _setup()
    model, tower, tok = st["model"], st["tower"], _Tok()
    rng = np.random.default_rng(3)
    lines = []
    for n, q in enumerate(["What is shown in the picture ?", "Describe the scene in detail ."]):
        path = str(tmp_path / f"img{n}.png")
        Image.fromarray(rng.integers(0, 256, (60 + 8 * n, 72, 3), dtype=np.uint8)).save(path)
        lines.append(json.dumps(dict(image_path=path, question=q, question_id=f"q{n}", **({"ds_question_id": 7} if n else {}))))
    qa = tmp_path / "questions.jsonl"
    qa.write_text("\n".join(lines) + "\n")
    items = autocheck.read_gen_dataset(str(qa))
    assert [tuple(it["image"].shape) for it in items] == [(60, 72, 3), (68, 72, 3)] and items[1]["metainfos"]["ds_question_id"] == 7

    def stand_in(images):
        return tower[[(int(im.shape[0]) - 60) // 8 for im in images]]
    model.set_vision_tower(stand_in)
    try:
        _records(model, tok, items, tower, G, wrap_question_for_omni_lmm)
    finally:
        model.set_vision_tower(None)


def _records(model, tok, items, tower, G, wrap_question_for_omni_lmm):
    prompts = [torch.as_tensor(wrap_question_for_omni_lmm(it["question"], model.cfg.n_image_tokens, tok)["input_ids"]) for it in items]
    assert all(int((p == AC.OMNI_TOKENS[0]).sum()) == AC.OMNI_NQ and int(p.max()) < model.cfg.vocab for p in prompts)
    keys = ["question_id", "raw_question", "answer", "metainfos", "model_path"]
    # beam branch: one search per item, written `repeat` times
    recs = G.generate_answers(model, tok, items, repeat=2, max_tokens=6, num_beam=3, model_path="ckpt", prompts_per_call=2)
    direct, _ = model.beam_search(prompts, tower[:2], 6, num_beams=3, repetition_penalty=1.1)
    assert [r["answer"] for r in recs] == [tok.decode(d).strip() for d in direct for _ in range(2)] and all(len(d) == 6 for d in direct)
    assert list(recs[0]) == keys and list(recs[2]) == [keys[0], "ds_question_id"] + keys[1:] and recs[2]["ds_question_id"] == 7
    assert [r["question_id"] for r in recs] == ["q0", "q0", "q1", "q1"] and all(r["model_path"] == "ckpt" for r in recs)
    # sampling branch: generate(repetition_penalty=1.1) from the seeded CPU generator
    recs = G.generate_answers(model, tok, items, repeat=3, temperature=0.7, max_tokens=6, seed=9, model_path="ckpt", prompts_per_call=2)
    direct = model.generate(prompts, tower[:2], 6, repeat=3, temperature=0.7, repetition_penalty=1.1,
                            generator=torch.Generator().manual_seed(9))
    assert [r["answer"] for r in recs] == [tok.decode(t).strip() for d in direct for t in d] and len(recs) == 6
    assert list(recs[0]) == keys and list(recs[3]) == [keys[0], "ds_question_id"] + keys[1:]
    # --continuous: the same records from generate_continuous
    recs_c = G.generate_answers(model, tok, items, repeat=3, temperature=0.7, max_tokens=6, seed=9, model_path="ckpt", continuous=True, slots=4)
    want = dict(model.generate_continuous(zip(prompts, tower[:2]), 6, slots=4, repeat=3, temperature=0.7, repetition_penalty=1.1, seed=9,
                                          max_prompt_tokens=max(int(p.numel()) for p in prompts)))
    assert [r["answer"] for r in recs_c] == [tok.decode(t).strip() for i in (0, 1) for t in want[i]]
    json.dumps(recs + recs_c)
    # the stages that stay closed for OmniLMM
    from rlaif_v_amd import gen_data, vqa
    with pytest.raises(NotImplementedError):
        gen_data.generate_answers(model, tok, items)
    with pytest.raises(NotImplementedError, match="OmniLMM"):
        vqa.answer_questions(model, tok, items)
