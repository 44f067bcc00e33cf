"""Host side of the yes / no feedback scoring: the two new C-ABI entry points and ``splice.build_branch_plan``.

The plan is checked against a brute-force construction that never looks at the builder's code path: every prompt is spliced
token by token in plain Python, the shared prefix is found by comparing the spliced rows position by position, and the
attention rule ``query i sees key j  <=>  j <= i and (j < seg_sh or j >= q_lo[i])`` is expanded into a dense visibility
matrix that must equal "each question sees exactly its own stand-alone sequence"."""
import pytest
import torch

from rlaif_v_amd.splice import (IMAGE_TOKEN_INDEX, build_branch_plan, check_branch_rows, make_omnilmm_splicer)

P = 6                                   # image tokens
IM_PATCH, IM_START, IM_END = 900, 901, 902
OMNI = make_omnilmm_splicer(IM_PATCH, IM_START, IM_END)


def test_entry_points_declared_and_exported_in_abi_7():
    from rlaif_v_amd import hip
    lib = hip.lib()
    assert lib.lib.rv_abi_version() == 7
    ret, args = lib.decls["rv_attn_fwd_branches"]
    assert ret == "int" and [n for _, n in args] == ["qkv", "ld", "q_col0", "k_col0", "v_col0", "out", "ldo", "lse", "S", "L", "H",
                                                     "hd", "scale", "seg_sh", "q_lo", "kv_group", "row_off", "row_len", "stream"]
    ret, args = lib.decls["rv_next_token_scores"]
    assert ret == "int" and [n for _, n in args] == ["logits", "ldl", "M", "V_valid", "seen_off", "seen_ids", "penalty",
                                                     "want_ids", "K", "probs", "logp", "argmax", "lse", "stream"]
    assert hasattr(lib.lib, "rv_attn_fwd_branches") and hasattr(lib.lib, "rv_next_token_scores")
    # argument errors come back through the ABI before any launch
    assert lib.lib.rv_attn_fwd_branches(None, 128, 0, 0, 0, None, 128, None, 1, 8, 2, 128, 1.0, None, None, 1, None, None, None) == 1
    assert "seg_sh and q_lo" in lib.last_error()
    assert lib.lib.rv_next_token_scores(None, 64, 1, 128, None, None, 1.0, None, 0, None, None, None, None, None) == 1
    assert "ldl >= V_valid" in lib.last_error()


# ------------------------------------------------------------------------------------------------ brute force
def _llava_prompt(head, tail):
    return torch.tensor([1] + head + [IMAGE_TOKEN_INDEX] + tail)


def _omni_prompt(head, tail):
    return torch.tensor([1] + head + [IM_START] + [IM_PATCH] * P + [IM_END] + tail)


def _brute_splice(ids, image, omni):
    """Stand-alone spliced sequence as a list of sources (>= 0 token id, <= -2 feature row -2 - r)."""
    ids = ids.tolist()
    out = []
    if omni:
        k = 0
        for t in ids:
            if t == IM_PATCH:
                out.append(-2 - (image * P + k))
                k += 1
            else:
                out.append(t)
        return out
    for t in ids:
        out.extend([-2 - (image * P + k) for k in range(P)] if t == IMAGE_TOKEN_INDEX else [t])
    return out


def _brute_shared(seqs):
    if len(seqs) == 1:
        return 0
    sh = 0
    while all(sh < len(s) - 1 for s in seqs) and all(s[sh] == seqs[0][sh] for s in seqs):
        sh += 1
    while sh > 0 and any(s[sh - 1] <= -2 and s[sh] == s[sh - 1] - 1 for s in seqs):     # never inside an image block
        sh -= 1
    return sh


def _check_plan(plan, prompts, omni, pad_free):
    """Every table of the plan against the stand-alone sequences."""
    seqs = [[_brute_splice(p, k, omni) for p in plist] for k, plist in enumerate(prompts)]
    S = plan.S
    starts = plan.row_off.tolist() if pad_free else [s * plan.L for s in range(S)]
    lens = plan.row_len.tolist() if pad_free else None
    src, pos, q_lo = plan.src.tolist(), plan.pos.tolist(), plan.q_lo.tolist()
    last = plan.last_idx.tolist()
    assert plan.n_seq == len(last) == sum(len(x) for x in seqs)
    row_of = lambda n: max(s for s in range(S) if starts[s] <= n)                       # noqa: E731
    qi = 0
    seen_rows = set()
    for k, img in enumerate(seqs):
        sh = _brute_shared(img)
        for seq in img:
            n_last = last[qi]
            s = row_of(n_last)
            seen_rows.add(s)
            assert int(plan.seg_sh[s]) == sh
            a = starts[s]
            # the keys the question's last token sees, in order, are exactly its stand-alone sequence at its own positions
            lo = q_lo[n_last]
            keys = [j for j in range(n_last - a + 1) if j < sh or j >= lo]
            assert [src[a + j] for j in keys] == seq
            assert [pos[a + j] for j in keys] == list(range(len(seq)))
            # and every token of the tail sees the same branch start (so the whole tail is one causal sequence)
            assert all(q_lo[a + j] == lo for j in range(lo, n_last - a + 1)) and lo >= sh
            if len(img) == 1:
                assert sh == 0 and lo == 0 and n_last - a + 1 == len(seq)                # a plain causal row
            qi += 1
    assert seen_rows == set(range(S))
    if pad_free:
        assert plan.n_tokens == sum(lens) == plan.src.numel() and plan.L == max(lens)
    else:
        assert plan.n_tokens == S * plan.L == plan.src.numel()
    return seqs


PROMPTS = {
    False: [[_llava_prompt([7, 8], [20, 21, 22, 23, 24]), _llava_prompt([7, 8], [20, 21, 30]), _llava_prompt([7, 8], [20, 41])],
            [_llava_prompt([7], [50, 51, 52])],
            [_llava_prompt([], [60, 61]), _llava_prompt([], [60, 62, 63, 64, 65, 66, 67]), _llava_prompt([], [70])]],
    True: [[_omni_prompt([7, 8], [20, 21, 22, 23, 24]), _omni_prompt([7, 8], [20, 21, 30]), _omni_prompt([7, 8], [20, 41])],
           [_omni_prompt([7], [50, 51, 52])],
           [_omni_prompt([], [60, 61]), _omni_prompt([], [60, 62, 63, 64, 65, 66, 67]), _omni_prompt([], [70])]],
}


@pytest.mark.parametrize("omni", [False, True])
@pytest.mark.parametrize("pad_free", [True, False])
def test_branch_plan_against_brute_force(omni, pad_free):
    prompts = PROMPTS[omni]
    plan = build_branch_plan(prompts, P, 64, splicer=OMNI if omni else None, pad_free=pad_free)
    seqs = _check_plan(plan, prompts, omni, pad_free)
    assert plan.S == 3 and plan.seg is None and plan.branches is not None
    # image 0: system | image | 20 is common ([1, 7, 8] + P features (+ im_start / im_end) + [20]); image 1: one question
    assert plan.seg_sh.tolist() == ([3 + P + 2 + 1, 0, 1 + P + 2] if omni else [3 + P + 1, 0, 1 + P])
    n_rows = sum(_brute_shared(img) + sum(len(s) - _brute_shared(img) for s in img) for img in seqs)
    assert plan.n_real_tokens == n_rows
    # every image's features are used once
    assert sorted(-2 - int(v) for v in plan.src.tolist() if v <= -2) == list(range(3 * P))


@pytest.mark.parametrize("omni", [False, True])
def test_layouts_agree_up_to_row_renumbering(omni):
    prompts = PROMPTS[omni]
    a = build_branch_plan(prompts, P, 64, splicer=OMNI if omni else None, pad_free=True)
    b = build_branch_plan(prompts, P, 64, splicer=OMNI if omni else None, pad_free=False)
    assert a.S == b.S and a.L == b.L and torch.equal(a.seg_sh, b.seg_sh)
    off, ln = a.row_off.tolist(), a.row_len.tolist()
    for s in range(a.S):
        for name in ("src", "pos", "q_lo"):
            assert torch.equal(getattr(a, name)[off[s]:off[s] + ln[s]], getattr(b, name)[s * b.L:s * b.L + ln[s]]), (name, s)
        assert bool((b.src[s * b.L + ln[s]:(s + 1) * b.L] == -1).all())
    rows_a = [(max(s for s in range(a.S) if off[s] <= n), n) for n in a.last_idx.tolist()]
    assert [(s, n - off[s]) for s, n in rows_a] == [(n // b.L, n % b.L) for n in b.last_idx.tolist()]


def test_prefix_never_cuts_an_image_block():
    # the second prompt ENDS with its image block: the rows agree on [1, 7, image...] but each needs a token of its own, and
    # the cut may not fall inside the block -> the prefix stops in front of the image
    prompts = [[torch.tensor([1, 7, IMAGE_TOKEN_INDEX, 20, 21]), torch.tensor([1, 7, IMAGE_TOKEN_INDEX])]]
    plan = build_branch_plan(prompts, P, 64)
    assert plan.seg_sh.tolist() == [2]
    _check_plan(plan, prompts, False, True)
    src = plan.src.tolist()
    sh = 2
    assert not (src[sh - 1] <= -2 and src[sh] <= -2)
    # OmniLMM: a prompt that stops inside the patch run (malformed for the splicer) is refused by the splicer itself
    with pytest.raises(ValueError):
        build_branch_plan([[torch.tensor([1, IM_START] + [IM_PATCH] * P)]], P, 64, splicer=OMNI)


@pytest.mark.parametrize("omni", [False, True])
def test_max_row_tokens_splits_and_repeats_the_prefix(omni):
    prompts = [PROMPTS[omni][0]]
    full = build_branch_plan(prompts, P, 64, splicer=OMNI if omni else None)
    sh = int(full.seg_sh[0])
    tails = [4, 2, 1]
    assert full.row_len.tolist() == [sh + sum(tails)]
    plan = build_branch_plan(prompts, P, 64, splicer=OMNI if omni else None, max_row_tokens=sh + 6)
    assert plan.S == 2 and plan.row_len.tolist() == [sh + 6, sh + 1] and plan.seg_sh.tolist() == [sh, sh]
    _check_plan(plan, prompts, omni, True)
    a, b = plan.row_off.tolist()
    assert torch.equal(plan.src[a:a + sh], plan.src[b:b + sh])                          # the prefix travels with every row
    # a limit below prefix + one tail still places one tail per row
    tight = build_branch_plan(prompts, P, 64, splicer=OMNI if omni else None, max_row_tokens=sh)
    assert tight.S == 3 and tight.row_len.tolist() == [sh + t for t in tails]
    _check_plan(tight, prompts, omni, True)


def test_errors():
    prompts = PROMPTS[False]
    longest = max(len(_brute_splice(p, 0, False)) for plist in prompts for p in plist)
    build_branch_plan(prompts, P, longest)
    with pytest.raises(ValueError, match="model_max_length"):
        build_branch_plan(prompts, P, longest - 1)
    with pytest.raises(ValueError, match="no question"):
        build_branch_plan([[]], P, 64)
    # malformed q_lo tables: below the prefix, beyond the query, decreasing
    seg_sh = torch.tensor([2], dtype=torch.int32)
    ok = torch.tensor([0, 0, 2, 2, 4, 4], dtype=torch.int32)
    check_branch_rows(seg_sh, ok, [0], [6])
    for bad in ([0, 0, 1, 2, 4, 4], [0, 0, 3, 3, 4, 4], [0, 0, 2, 2, 4, 3]):
        with pytest.raises(ValueError, match="q_lo"):
            check_branch_rows(seg_sh, torch.tensor(bad, dtype=torch.int32), [0], [6])
    with pytest.raises(ValueError, match="do not fit"):
        check_branch_rows(seg_sh, ok, [2], [6])


def test_unpacked_plan_is_one_plain_row_per_question():
    prompts = PROMPTS[False]
    plan = build_branch_plan(prompts, P, 64, packed=False)
    seqs = [_brute_splice(p, k, False) for k, plist in enumerate(prompts) for p in plist]
    assert plan.S == len(seqs) and plan.branches is None and plan.seg is None and plan.q_lo is None
    assert plan.row_len.tolist() == [len(s) for s in seqs]
    off = plan.row_off.tolist()
    for s, seq in enumerate(seqs):
        assert plan.src[off[s]:off[s] + len(seq)].tolist() == seq
        assert plan.pos[off[s]:off[s] + len(seq)].tolist() == list(range(len(seq)))
        assert int(plan.last_idx[s]) == off[s] + len(seq) - 1


# ------------------------------------------------------------------------------------------------ pin to the reference
def test_oracle_matches_the_reference_generate_fixture():
    """tests/golden/autocheck_tiny.pt holds what the reference's own generate(max_new_tokens=1, output_scores=True) returned
    per question (make_autocheck_golden.py): the CPU oracle the GPU tests measure against reproduces it, with the bar
    tests/test_oracle_golden.py uses for per-token log-probs (rtol = atol = 1e-4)."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import autocheck_case as AC
    from oracle import dpo_oracle as O
    case = AC.load_case()
    assert case["generate_ran"] and case["cfg"] == O.asdict(O.tiny_cfg())
    assert [len(p) for p in case["prompts"]] == [1, 4, 7]
    cfg = O.tiny_cfg()
    W = O.make_weights(cfg, seed=case["seed"], std=case["std"])
    logits = AC.oracle_logits(cfg, W, AC.question_embeds(cfg, W, case["prompts"], case["pixels"]))
    torch.testing.assert_close(logits, case["logits_last"], rtol=1e-4, atol=1e-4)
    logp = torch.log_softmax(logits, -1)[:, case["want_ids"]]
    torch.testing.assert_close(logp, torch.log(case["probs"]), rtol=1e-4, atol=1e-4)
    top2 = torch.topk(case["logits_last"], 2, -1)
    sure = (top2.values[:, 0] - top2.values[:, 1]) > 1e-3
    assert torch.equal(logits.argmax(-1)[sure], case["new_token"][sure])
    # the plan of the stored case: the prefix lengths the oracle-side helpers assume
    plan = build_branch_plan(case["prompts"], 16, cfg.model_max_length)
    assert plan.seg_sh.tolist() == [0, AC.n_prefix(1), AC.n_prefix(2)]


def test_omnilmm_oracle_matches_the_reference_fixture():
    """tests/golden/autocheck_omnilmm_tiny.pt: the reference OmniLMMForCausalLM's last-position logits per question (what its
    generate_vllm(repetition_penalty=1.1) returns as scores[0]: it generates from inputs_embeds, no id is penalised).  The CPU
    oracle WITHOUT a penalty reproduces them; with HF's processor over the prompt ids it would not."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import autocheck_case as AC
    case = AC.load_omni_case()
    assert tuple(case["tokens"]) == AC.OMNI_TOKENS and case["num_query"] == AC.OMNI_NQ and case["kv_dim"] == AC.OMNI_KV
    assert [len(p) for p in case["prompts"]] == [1, 4, 7] and case["want_ids"][0] in case["prompts"][0][0].tolist()
    _, ocfg = AC.omni_cfgs()
    W = AC.omni_weights(ocfg, std=case["std"])
    logits = AC.omni_oracle_logits(ocfg, W, case["tower"], case["prompts"])
    torch.testing.assert_close(logits, case["logits_last"], rtol=1e-4, atol=1e-4)
    want = case["want_ids"]
    torch.testing.assert_close(torch.log_softmax(logits, -1)[:, want], torch.log(case["probs"]), rtol=1e-4, atol=1e-4)
    flat = [p for plist in case["prompts"] for p in plist]
    pen = torch.stack([AC.hf_repetition_penalty(l, p, 1.1) for l, p in zip(logits, flat)])
    moved = (torch.log_softmax(pen, -1)[:, want] - torch.log(case["probs"])).abs().max()
    assert float(moved) > 1e-2, "a penalty over the prompt ids would be visible in this case"


def test_hf_repetition_penalty_restatement():
    """autocheck_case.hf_repetition_penalty against transformers' own processor when it is importable."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import autocheck_case as AC
    from transformers import RepetitionPenaltyLogitsProcessor      # a hard import: the goldens of this project need it too
    proc = RepetitionPenaltyLogitsProcessor(penalty=1.1)
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(3, 50, generator=g)
    ids = torch.randint(0, 50, (3, 9), generator=g)
    want = proc(ids, logits.clone())
    got = torch.stack([AC.hf_repetition_penalty(l, i, 1.1) for l, i in zip(logits, ids)])
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ command-line pieces
def test_expand2square_matches_pil_paste(tmp_path):
    """autocheck.expand2square against llava/mm_utils.py's expand2square restated on PIL, and read_gen_dataset honouring the
    checkpoint's image_aspect_ratio."""
    import json
    import numpy as np
    from PIL import Image
    from rlaif_v_amd import autocheck
    from rlaif_v_amd.image import CLIP_MEAN
    bg = tuple(int(x * 255) for x in CLIP_MEAN)
    rng = np.random.default_rng(0)
    for h, w in ((5, 9), (9, 4), (6, 6), (7, 2)):
        a = rng.integers(0, 255, (h, w, 3), dtype=np.uint8)
        pil = Image.fromarray(a)
        n = max(h, w)
        ref = Image.new(pil.mode, (n, n), bg)
        ref.paste(pil, (0, (w - h) // 2) if w > h else ((h - w) // 2, 0))
        assert np.array_equal(np.asarray(ref), autocheck.expand2square(torch.from_numpy(a), bg).numpy()), (h, w)
    wide = rng.integers(0, 255, (4, 10, 3), dtype=np.uint8)
    Image.fromarray(wide).save(tmp_path / "wide.png")
    rows = [dict(image_path=str(tmp_path / "wide.png"), question="Is it wide ?", question_id=7, ds_question_id=3),
            dict(image_path=str(tmp_path / "wide.png"), question="Is it tall ?")]
    qa = tmp_path / "q.jsonl"
    qa.write_text("\n".join(json.dumps(r) for r in rows))
    plain = autocheck.read_gen_dataset(str(qa))
    assert plain[0]["image"].shape == (4, 10, 3) and plain[0]["image"] is plain[1]["image"]
    assert [p["question_id"] for p in plain] == [7, 1] and plain[0]["metainfos"]["ds_question_id"] == 3
    padded = autocheck.read_gen_dataset(str(qa), image_aspect_ratio="pad")
    assert padded[0]["image"].shape == (10, 10, 3) and padded[0]["image"] is padded[1]["image"]
    assert torch.equal(padded[0]["image"][3:7], torch.from_numpy(wide))
    assert padded[0]["image"][0, 0].tolist() == list(bg) and padded[0]["image"][9, 9].tolist() == list(bg)
    with pytest.raises(NotImplementedError):
        autocheck.read_gen_dataset(str(qa), image_aspect_ratio="anyres")


@pytest.mark.parametrize("arch", ["llava", "omnilmm"])
def test_score_yesno_default_penalises_nothing(arch):
    """Neither labeler's reference scores carry a repetition penalty: llava15_gen_data.py sets none, and omnilmm_gen_data.py's
    1.1 reaches a generate() that starts from inputs_embeds, i.e. from an empty id tensor (omnilmm/model/omnilmm.py:371-396).
    score_yesno's default must therefore ask the model for penalty 1.0; an explicit value is passed through."""
    import os
    import sys
    import types
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from toy_tokenizer import OmniToyTokenizer, ToyTokenizer
    from rlaif_v_amd import autocheck

    class Omni(OmniToyTokenizer):
        def decode(self, ids, skip_special_tokens=True):
            return super().decode(ids)

    class Llava(ToyTokenizer):
        def encode(self, text):
            return self._ids(text.replace("<s>", ""))

        def decode(self, ids, skip_special_tokens=True):
            return " ".join(str(int(i)) for i in ids)

    calls = []

    def forward_next_token_scores(prompts, images, want, packed=True, repetition_penalty=1.0, max_row_tokens=None):
        calls.append(repetition_penalty)
        n = sum(len(p) for p in prompts)
        return torch.full((n, 4), 0.25), torch.zeros(n, 4), torch.full((n,), 5, dtype=torch.int32), torch.zeros(n)
    model = types.SimpleNamespace(cfg=types.SimpleNamespace(arch=arch, n_image_tokens=2), forward_next_token_scores=forward_next_token_scores)
    tok = Omni() if arch == "omnilmm" else Llava()
    img = torch.zeros(3, 4, 4)
    items = [dict(question="Is there a dog ?", image=img), dict(question="Is it yes or no ?", image=img)]
    recs = autocheck.score_yesno(model, tok, items)
    assert calls == [1.0] and len(recs) == 2 and recs[0]["scores"] == {"yes": 0.25, "Yes": 0.25, "no": 0.25, "No": 0.25}
    autocheck.score_yesno(model, tok, items, repetition_penalty=1.1)
    assert calls == [1.0, 1.1]
