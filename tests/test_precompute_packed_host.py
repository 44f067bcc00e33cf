"""The all-positions tables of the packed plan (host side, no GPU): ``build_packed_plan(all_rows=True)`` returns the normal
packed training plan plus ``ev_*``, the evaluation of EVERY position on the packed row that the packed log-prob precompute
runs (get_batch_logps(return_all=True) on the layout of the training forward).

Checked against the un-packed ``build_splice_plan`` of the same batch: every (sequence, position) with a successor maps to a
packed row with the same source and RoPE position and the target ``labels[s, t + 1]`` (token id 0 where masked); shared-prefix
rows are evaluated once and land in both sequences' per-token rows; the compact slots are the training plan's selection."""
from types import SimpleNamespace

import pytest
import torch

from oracle import dpo_oracle as O
from rlaif_v_amd.splice import build_packed_plan, build_splice_plan

CFG = O.tiny_cfg()
NIMG = (CFG.image_size // CFG.patch) ** 2


def _ragged():
    return O.make_synthetic_batch(CFG, 3, 130, 40, seed=3, answer_lens=[(70, 45), (33, 90), (2, 64)])


def _truncated():
    return O.make_synthetic_batch(CFG, 2, 255, 40, seed=3, answer_lens=[(10, 215), (150, 20)])


def _plans(batch, pad_free):
    ids, labels = batch["concatenated_input_ids"], batch["concatenated_labels"]
    B = ids.shape[0] // 2
    ev = build_packed_plan(ids, labels, NIMG, B, CFG.model_max_length, CFG.pad_token_id, pad_free=pad_free, all_rows=True)
    train = build_packed_plan(ids, labels, NIMG, B, CFG.model_max_length, CFG.pad_token_id, pad_free=pad_free)
    flat = build_splice_plan(ids, labels, NIMG, B, CFG.model_max_length)
    return ev, train, flat


def _own_lengths(batch, flat):
    """n_s of every sequence: spliced, truncated, the collator's right padding dropped."""
    ids = batch["concatenated_input_ids"]
    text = (ids != CFG.pad_token_id).sum(1)                        # pad id 0 appears only as padding in these batches
    return [min(int(n) + NIMG - 1, CFG.model_max_length, flat.L) for n in text]


def _check(batch, pad_free):
    ev, train, flat = _plans(batch, pad_free)
    S2, B, ld = ev.n_seq, ev.n_seq // 2, ev.ev_ld
    n = _own_lengths(batch, flat)
    # ---- the training plan is untouched by all_rows
    for k in ("src", "pos", "seg_sh", "seg_e1", "sel_idx", "tgt", "seq_off", "seq_of_row", "row_off", "row_len"):
        a, b = getattr(ev, k), getattr(train, k)
        assert (a is None and b is None) or torch.equal(a, b), k
    assert (ev.S, ev.L, ev.n_sel, ev.n_tokens) == (train.S, train.L, train.n_sel, train.n_tokens)
    assert (ev.row_off is not None) == pad_free
    # ---- per-row lengths and the matrix width
    assert ev.ev_len == [x - 1 for x in n] and ld == max(n) - 1
    assert ev.n_ev == ev.ev_idx.numel() == ev.ev_tgt.numel() == ev.ev_dst_a.numel() == ev.ev_dst_b.numel() == ev.ev_dst_c.numel()
    assert all(t.dtype == torch.int32 for t in (ev.ev_idx, ev.ev_tgt, ev.ev_dst_a, ev.ev_dst_b, ev.ev_dst_c))
    # ---- every (sequence, position) of the un-packed plan -> one packed row with its source, position and target
    slot_row = torch.full((S2 * ld,), -1, dtype=torch.long)
    for dst in (ev.ev_dst_a, ev.ev_dst_b):
        ok = dst >= 0
        assert int(dst.max()) < S2 * ld
        assert bool((slot_row[dst[ok].long()] == -1).all()), "a per-token slot has two writers"
        assert dst[ok].unique().numel() == int(ok.sum())
        slot_row[dst[ok].long()] = torch.nonzero(ok, as_tuple=True)[0]
    src_flat, lab_flat = flat.src.view(S2, flat.L).long(), flat.labels
    for s in range(S2):
        for t in range(ld):
            i = int(slot_row[s * ld + t])
            if t >= n[s] - 1:
                assert i == -1, (s, t)                              # no writer beyond the row's own length
                continue
            assert i >= 0, (s, t)
            row = int(ev.ev_idx[i])
            assert int(ev.src[row]) == int(src_flat[s, t]) and int(ev.pos[row]) == t, (s, t)
            nxt = int(lab_flat[s, t + 1])
            assert int(ev.ev_tgt[i]) == (nxt if nxt != -100 else 0), (s, t)
    # ---- evaluated rows are distinct; prefix rows appear once and carry two slots, branch rows one
    assert ev.ev_idx.unique().numel() == ev.n_ev
    two = ev.ev_dst_b >= 0
    starts = ev.row_off.long() if pad_free else torch.arange(B) * ev.L
    pair_of = (torch.bucketize(ev.ev_idx.long(), starts, right=True) - 1)
    within = ev.ev_idx.long() - starts[pair_of]
    assert torch.equal(two, within < ev.seg_sh.long()[pair_of])
    assert int(two.sum()) == int(ev.seg_sh.sum())
    assert torch.equal(ev.ev_dst_b[two].long() - ev.ev_dst_a[two].long(), torch.full((int(two.sum()),), B * ld))
    assert ev.n_ev == sum(n) - S2 - int(ev.seg_sh.sum())          # every position with a successor, the prefix counted once
    # ---- the compact slots reproduce the training selection exactly
    has = ev.ev_dst_c >= 0
    assert int(has.sum()) == train.n_sel and not bool((has & two).any())
    order = torch.argsort(ev.ev_dst_c[has])
    assert torch.equal(ev.ev_dst_c[has][order].long(), torch.arange(train.n_sel))
    assert torch.equal(ev.ev_idx[has][order], train.sel_idx)
    assert torch.equal(ev.ev_tgt[has][order], train.tgt)
    assert torch.equal(ev.ev_tgt[~has], torch.zeros(int((~has).sum()), dtype=torch.int32))
    return ev


@pytest.mark.parametrize("pad_free", [False, True])
def test_all_rows_tables_of_the_ragged_batch(pad_free):
    ev = _check(_ragged(), pad_free)
    assert ev.seg_sh.tolist() == [54, 54, 54] and ev.seg_e1.tolist() == [125, 88, 57]
    assert ev.n_sel == 304
    if pad_free:
        assert ev.row_len.tolist() == [171, 179, 122]
    assert ev.ev_len == [124, 87, 56, 99, 144, 118]


@pytest.mark.parametrize("pad_free", [False, True])
def test_all_rows_tables_when_model_max_length_cuts_a_sequence(pad_free):
    batch = _truncated()
    ev = _check(batch, pad_free)
    assert ev.ev_len == [64, 204, 255, 74]                          # the rejected row of pair 0 ends at model_max_length
    # the cut row's last evaluated position predicts the last KEPT label, not one behind the cut
    lab = build_splice_plan(batch["concatenated_input_ids"], batch["concatenated_labels"], NIMG, 2, CFG.model_max_length).labels
    assert lab.shape[1] == CFG.model_max_length
    i = int(torch.nonzero(ev.ev_dst_a == 2 * ev.ev_ld + 254, as_tuple=True)[0])
    assert int(ev.ev_tgt[i]) == int(lab[2, 255])


def test_a_row_without_targets_keeps_a_zero_count():
    batch = _ragged()
    labels = batch["concatenated_labels"].clone()
    labels[4] = -100                                                 # the rejected sequence of pair 1 has no target
    ids = batch["concatenated_input_ids"]
    ev = build_packed_plan(ids, labels, NIMG, 3, CFG.model_max_length, CFG.pad_token_id, pad_free=True, all_rows=True)
    cnt = (ev.seq_off[1:] - ev.seq_off[:-1]).tolist()
    assert cnt[4] == 0 and all(c > 0 for i, c in enumerate(cnt) if i != 4)
    mine = (ev.ev_dst_a // ev.ev_ld) == 4
    assert int(mine.sum()) > 0                                      # its positions are still evaluated (per-token values) ...
    assert bool((ev.ev_dst_c[mine] == -1).all()) and bool((ev.ev_tgt[mine] == 0).all())    # ... none of them is summed


def test_all_rows_refuses_token_weights():
    b = _ragged()
    with pytest.raises(ValueError):
        build_packed_plan(b["concatenated_input_ids"], b["concatenated_labels"], NIMG, 3, 256, 0, all_rows=True,
                          token_weight=b["concatenated_token_weight"])


def test_packed_mode_argument_checks():
    """forward_logps(packed=True) is forward only, all-positions only, label_shift=1 only: refused before any device work."""
    from rlaif_v_amd.model import LlavaDPOModel
    b = _ragged()
    args = (SimpleNamespace(), b["concatenated_input_ids"], b["concatenated_labels"], b["images"])
    with pytest.raises(ValueError, match="forward-only"):
        LlavaDPOModel.forward_logps(*args, save_for_backward=True, all_rows=True, packed=True)
    with pytest.raises(ValueError, match="all_rows"):
        LlavaDPOModel.forward_logps(*args, save_for_backward=False, packed=True)
    with pytest.raises(ValueError, match="label_shift"):
        LlavaDPOModel.forward_logps(*args, save_for_backward=False, all_rows=True, packed=True, label_shift=0)
    with pytest.raises(ValueError, match="2B"):
        LlavaDPOModel.forward_logps(SimpleNamespace(), b["win_input_ids"], b["win_labels"], b["images"],
                                    save_for_backward=False, all_rows=True, packed=True)


def test_precompute_flag_and_environment(monkeypatch):
    from rlaif_v_amd.inference_logp import precompute_packed_default
    from rlaif_v_amd.train_llava15 import parse_args
    monkeypatch.delenv("RV_PRECOMPUTE_PACKED", raising=False)
    assert precompute_packed_default() is False
    monkeypatch.setenv("RV_PRECOMPUTE_PACKED", "1")
    assert precompute_packed_default() is True
    assert parse_args([])[1].precompute_packed is False
    assert parse_args(["--precompute_packed", "True"])[1].precompute_packed is True


def test_entry_point_declared_and_exported_in_abi_7():
    from rlaif_v_amd import hip
    lib = hip.lib()
    assert lib.lib.rv_abi_version() == 7
    ret, args = lib.decls["rv_logp_finish_unpack"]
    assert ret == "int" and [n for _, n in args] == ["pmax", "psum", "tgt_logit", "nblk", "M", "dst_a", "dst_b", "dst_c",
                                                     "per_token", "n_per_token", "compact", "n_compact", "stream"]
    assert hasattr(lib.lib, "rv_logp_finish_unpack")
