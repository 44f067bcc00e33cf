"""Token weights in the splice plans (host side, no GPU): ``build_splice_plan`` / ``build_packed_plan`` gather the collator's
``token_weight [2B, T-1]`` onto the selected rows (``SplicePlan.w_sel``) in the order of ``tgt`` / ``seq_of_row``, for the
rectangular, packed and pad-free layouts of OmniLMM-style batches; the length-changing LLaVA splice refuses weights."""
import os

import pytest
import torch

from oracle import dpo_oracle as O
from oracle import omnilmm_oracle as OO
from rlaif_v_amd.splice import build_packed_plan, build_splice_plan, make_omnilmm_splicer

TOKENS = (322, 323, 324)
NQ = 16
GOLD = os.path.join(os.path.dirname(__file__), "golden", "omnilmm_token_weighted.pt")
LAYOUTS = ("rect", "packed", "pad_free")


def _batch(answer_lens, seed=5):
    cfg = O.LlavaCfg(hidden=64, layers=1, heads=1, kv_heads=1, ffn=64, vocab=325, model_max_length=256)
    return OO.make_omnilmm_batch(cfg, len(answer_lens), 72, NQ, TOKENS, seed=seed, answer_lens=answer_lens)


def _coded_weight(ids):
    """token_weight[s, t] = 1000 s + t + 1: every selected row's weight names its (sequence, column)."""
    S, T = ids.shape
    return (1000.0 * torch.arange(S)[:, None] + torch.arange(T - 1)[None] + 1.0).float()


def _plan(layout, ids, labels, max_len, token_weight=None, splicer="omni"):
    sp = make_omnilmm_splicer(*TOKENS) if splicer == "omni" else None
    n_img = ids.shape[0] // 2
    if layout == "rect":
        return build_splice_plan(ids, labels, NQ, n_img, max_len, splicer=sp, token_weight=token_weight)
    return build_packed_plan(ids, labels, NQ, n_img, max_len, 0, splicer=sp, pad_free=layout == "pad_free",
                             token_weight=token_weight)


def _reference_gather(labels, token_weight, max_len):
    """compute_weighted_logp's view (trainers.py:128-137): weights of the positions whose next label counts, row-major."""
    lab = labels if max_len is None else labels[:, :max_len]
    mask = lab[:, 1:] != -100
    s_idx, l_idx = torch.nonzero(mask, as_tuple=True)
    return token_weight[:, :lab.shape[1] - 1][mask], s_idx, lab[:, 1:][mask]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("max_len", [None, 58])
def test_w_sel_is_the_reference_gather_in_row_order(layout, max_len):
    b = _batch([(38, 30), (25, 38), (31, 31)])               # ragged answers; 58 cuts every answer short
    ids, labels = b["concatenated_input_ids"], b["concatenated_labels"]
    tw = _coded_weight(ids)
    plan = _plan(layout, ids, labels, max_len, tw)
    want, s_idx, tgt = _reference_gather(labels, tw, max_len)
    assert plan.w_sel is not None and plan.w_sel.dtype == torch.float32 and plan.w_sel.numel() == plan.n_sel
    assert torch.equal(plan.w_sel, want)
    # same row order as tgt / seq_of_row: the weight's code names the row's sequence, and its column's next label is tgt
    seq_from_w = ((plan.w_sel - 1) // 1000).long()
    col_from_w = ((plan.w_sel - 1) % 1000).long()
    assert torch.equal(seq_from_w, plan.seq_of_row.long()) and torch.equal(seq_from_w, s_idx)
    assert torch.equal(labels[seq_from_w, col_from_w + 1], plan.tgt.long())
    assert torch.equal(plan.tgt.long(), tgt)
    if max_len is not None:
        assert int(col_from_w.max()) <= max_len - 2           # truncated rows take their weights with them


@pytest.mark.parametrize("layout", LAYOUTS)
def test_collator_weights_and_an_all_ones_answer(layout):
    G = torch.load(GOLD, weights_only=False)
    b = G["batch"]
    ids, labels = b["concatenated_input_ids"], b["concatenated_labels"]
    tw = b["concatenated_token_weight"].clone()
    B = b["win_input_ids"].shape[0]
    tw[B + 1] = 1.0                                            # one sequence's answer entirely weight 1
    plan = _plan(layout, ids, labels, None, tw)
    want, _, _ = _reference_gather(labels, tw, None)
    assert torch.equal(plan.w_sel, want)
    assert set(plan.w_sel.unique().tolist()) == {1.0, G["meta"]["mod_token_weight"]}
    off = plan.seq_off.long()
    assert bool((plan.w_sel[off[B + 1]:off[B + 2]] == 1.0).all())
    # weighted count per sequence = compute_weighted_logp's denominator
    den = (tw * (labels[:, 1:] != -100)).sum(1)
    cnt = torch.stack([plan.w_sel[off[s]:off[s + 1]].sum() for s in range(2 * B)])
    torch.testing.assert_close(cnt, den, rtol=0, atol=0)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_plans_without_weights_are_unchanged(layout):
    b = _batch([(38, 30), (25, 38)])
    ids, labels = b["concatenated_input_ids"], b["concatenated_labels"]
    p0 = _plan(layout, ids, labels, 64)
    p1 = _plan(layout, ids, labels, 64, _coded_weight(ids))
    assert p0.w_sel is None
    for k, v in p0.__dict__.items():
        if k == "w_sel":
            continue
        w = getattr(p1, k)
        assert (torch.equal(v, w) if torch.is_tensor(v) else v == w), k


def test_plan_to_moves_w_sel():
    b = _batch([(30, 28)])
    ids, labels = b["concatenated_input_ids"], b["concatenated_labels"]
    p = _plan("rect", ids, labels, None, _coded_weight(ids)).to("cpu")
    assert p.w_sel is not None and p.w_sel.numel() == p.n_sel


@pytest.mark.parametrize("layout", LAYOUTS)
def test_length_changing_splice_refuses_token_weights(layout):
    cfg = O.tiny_cfg()
    b = O.make_synthetic_batch(cfg, 2, 40, 12, seed=3)
    ids, labels = b["concatenated_input_ids"], b["concatenated_labels"]
    with pytest.raises(NotImplementedError, match="keeps text positions"):
        if layout == "rect":
            build_splice_plan(ids, labels, 9, 2, cfg.model_max_length, token_weight=_coded_weight(ids))
        else:
            build_packed_plan(ids, labels, 9, 2, cfg.model_max_length, 0, pad_free=layout == "pad_free",
                              token_weight=_coded_weight(ids))


def test_weight_shape_is_checked():
    b = _batch([(30, 28)])
    ids, labels = b["concatenated_input_ids"], b["concatenated_labels"]
    with pytest.raises(ValueError):
        _plan("rect", ids, labels, None, _coded_weight(ids)[:1])
    with pytest.raises(ValueError):
        _plan("packed", ids, labels, None, _coded_weight(ids)[:, :20])


def test_generic_branch_needs_a_position_keeping_model():
    """get_beta_and_logps(is_llava15=False) and OmniLMMDPOTrainer refuse a LLaVA-style model before touching the device."""
    from rlaif_v_amd.trainer import OmniLMMDPOTrainer, TrainingArguments, get_beta_and_logps

    class _Llava:
        device = "cpu"
        training = True
        lora = None
        splice_keeps_positions = False
    b = _batch([(30, 28)])
    with pytest.raises(ValueError, match="keeps the text positions"):
        get_beta_and_logps(dict(b, images=torch.zeros(1, 4, 4)), _Llava(), TrainingArguments(task="DPO"), is_llava15=False)
    with pytest.raises(ValueError, match="OmniLMMDPOModel"):
        OmniLMMDPOTrainer(model=_Llava(), args=TrainingArguments())
    with pytest.raises(NotImplementedError, match="MiniCPM"):
        get_beta_and_logps(dict(b), _Llava(), TrainingArguments(task="DPO"), is_minicpm=True, is_llava15=False)
    with pytest.raises(NotImplementedError, match="LLaVA-1.5"):
        get_beta_and_logps(dict(b), _Llava(), TrainingArguments(task="DPO", dpo_token_weighted=True), is_llava15=True)
