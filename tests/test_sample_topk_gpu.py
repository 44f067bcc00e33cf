"""rv_sample_token_topk (csrc/decode.hip, the row in registers) and rv_sample_token_wide_topk (csrc/sample_wide.hip, the row
streamed) through the C ABI: operands in tests/guarded.py windows with the columns behind V_valid poisoned, tokens against the
float64 restatement of tests/topk_case.py (HF's RepetitionPenalty -> Temperature -> TopK -> TopP), logp inside the fp32
evaluation bound, and with top-k off the bits of the base entry points.

    python -m pytest tests/test_sample_topk_gpu.py -m gpu -q"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import divide_case as DC  # noqa: E402
import generate_case as GC  # noqa: E402
import topk_case as TK  # noqa: E402
from topk_case import U32, U_LAST  # noqa: E402

pytestmark = pytest.mark.gpu

FAMILIES = [pytest.param(False, id="reg"), pytest.param(True, id="wide")]
REG_ROWS = {8193: 44, 32000: 59, 65536: 23}      # V: seed of generate_case.peaked_row(V, seed, scale=8) - chosen on the CPU so
#                                                  that every combination below keeps the caps of topk_case.check


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _ldl(V, tight=False):
    return V if tight else (V + 3) // 4 * 4 + 64


# =========================================================================================== stratified uniforms, V = 512
@pytest.mark.parametrize("top_p", [1.0, 0.9])
@pytest.mark.parametrize("temperature", [0.2, 0.7, 1.0])
@pytest.mark.parametrize("top_k", [1, 2, 50, 512, 612])
@pytest.mark.parametrize("wide", FAMILIES)
def test_v512_stratified_uniforms(wide, top_k, temperature, top_p):
    """test_decode_kernels_gpu.py::test_sample_token's row (peaked_row(512, seed=3), ldl 576) with u = 0, the last float below 1
    and 4096 stratified values.  Asserted on the restatement before the launch: at most 1 % of the uniforms within V 2^-24 of a
    CDF boundary, the top-p edge more than 4 bounds from a tie, the k-th and (k+1)-th scores more than 8 * 2^-23 apart (on the
    CPU the worst of the 30 combinations are 0.85 %, 1.2e-3 and 2.2e-3).  The streamed kernel takes this kind at V = 512 as
    well and not at its larger sizes: there V 2^-24 leaves up to 6 % (32000) and 26 % (128256) of stratified uniforms undecidable, so
    those sizes get planted uniforms (test_streamed_kernel_planted_rows).  Then every decidable draw is the restatement's, no
    token outside the kept set is drawn, logp inside the fp32 evaluation bound."""
    V, ldl = 512, 576
    row = GC.peaked_row(V, seed=3)
    us = [0.0, U_LAST] + [(k + 0.5) / 4096 for k in range(4096)]
    p, want, ok = TK.check(row, V, us, temperature, top_p, top_k, max_undecidable=0.01)
    n_keep = int((p > 0).sum())
    assert n_keep <= (top_k if top_k < V else V)
    tok, logp, _, _ = TK.run(_dev(), wide, row, V, ldl, us, temperature, top_p, top_k)
    print(f"[topk] wide={wide} k={top_k} T={temperature} top_p={top_p}: kept {n_keep}, {100 * (1 - ok.mean()):.3f} % undecidable, "
          f"{len(set(tok.tolist()))} distinct tokens")
    TK.compare(row, p, want, ok, us, tok, logp, temperature)


# =========================================================================================== larger rows, planted uniforms
def _planted(dev, wide, row, V, ldl, temperature, top_p, top_k, seen, penalty, need_gap=True):
    bound = V * U32
    p, _, _ = TK.sampler_probs64_topk(row, temperature, top_p, top_k, seen, penalty)
    us = DC.planted_uniforms(p, bound)
    p, want, ok = TK.check(row, V, us, temperature, top_p, top_k, seen, penalty, need_gap=need_gap)
    tok, logp, _, _ = TK.run(dev, wide, row, V, ldl, us, temperature, top_p, top_k, seen, penalty)
    TK.compare(row, p, want, ok, us, tok, logp, temperature, seen, penalty)
    return p, tok


@pytest.mark.parametrize("penalty", [1.0, 1.3])
@pytest.mark.parametrize("top_k", [1, 50])
@pytest.mark.parametrize("V", [8193, 32000, 65536])
def test_register_kernel_larger_rows(V, top_k, penalty):
    """the three ids-per-thread variants (8, 32, 64) with a ragged end (8193), unpadded rows (ldl = V at 32000) and the full
    register row; with and without a repetition penalty over a list that holds the top token, ids out of range and duplicates.
    V 2^-24 is coarse here, so the uniforms are planted at the middles of the CDF intervals wider than 8 bounds."""
    dev = _dev()
    row = GC.peaked_row(V, seed=REG_ROWS[V], scale=8.0)
    top = int(np.argmax(row))
    seen = [top, top, 5, V - 1, -1, V + 7, int(np.argsort(row)[-2])] if penalty != 1.0 else None
    for temperature, top_p in ((0.7, 0.9), (1.0, 1.0)):
        p, tok = _planted(dev, False, row, V, V if V == 32000 else _ldl(V), temperature, top_p, top_k, seen, penalty)
        assert int((p > 0).sum()) <= top_k
        if top_k == 1:
            assert (tok == int(np.argmax(GC.penalised(row, seen, penalty)))).all()


@pytest.mark.parametrize("combo", [(0.2, 0.9, 1.0), (0.7, 0.9, 1.3), (1.0, 1.0, 1.3)], ids=lambda c: "T%g-p%g-pen%g" % c)
@pytest.mark.parametrize("top_k", [1, 3, 50])
@pytest.mark.parametrize("V,tight", [(1, False), (63, True), (4097, False), (65537, False), (70001, True), (128256, False)])
def test_streamed_kernel_planted_rows(V, tight, top_k, combo):
    """divide_case.planted_row: seven planted tokens carry the mass in different waves' segments, the background holds 1e-13 per
    token.  top_k = 3 cuts through the planted tokens, top_k = 50 through the background (whose order fp32 need not resolve: no
    planted uniform can reach a token of 1e-13, so the gap cap is asked of the cuts through the planted tokens only); V = 1 and
    top_k >= V are top-k off.  One workgroup's tail (63), 16-byte loads with a ragged end (4097, 65537), unaligned rows that
    touch each other (70001, ldl = V) and the Llama-3 row."""
    temperature, top_p, penalty = combo
    row = DC.planted_row(V, temperature, seed=V % 1000 + int(10 * temperature))
    seen = DC.planted_seen(V, row)
    p, tok = _planted(_dev(), True, row, V, _ldl(V, tight), temperature, top_p, top_k, seen, penalty, need_gap=top_k < 7)
    assert int((p > 0).sum()) <= max(1, min(top_k, V))


# =========================================================================================== exact ties
def _tie_case(dev, wide, V, ldl, ids_top, ids_tied, zero_tie=False):
    """T = 1 without penalty: the scores are the logits bit for bit.  top_k = len(ids_top) + 1 reaches the tied value and keeps
    ALL of its ids; top_k = len(ids_top) keeps the distinct top values alone.  Every kept token is drawn at the middle of its
    CDF interval."""
    row = TK.tie_row(V, ids_top, ids_tied, seed=V % 97, zero_tie=zero_tie)
    for top_k, kept in ((len(ids_top) + 1, sorted(list(ids_top) + list(ids_tied))), (len(ids_top), sorted(ids_top))):
        p, _, _ = TK.sampler_probs64_topk(row, 1.0, 1.0, top_k)
        assert np.nonzero(p > 0)[0].tolist() == kept
        us = DC.planted_uniforms(p, V * U32)
        assert len(us) == 2 + len(kept), "every kept token holds an interval wider than 8 bounds"
        p, want, ok = TK.check(row, V, us, 1.0, 1.0, top_k, need_gap=False)
        tok, logp, _, _ = TK.run(dev, wide, row, V, ldl, us, 1.0, 1.0, top_k)
        TK.compare(row, p, want, ok, us, tok, logp, 1.0)
        assert sorted(set(tok.tolist())) == kept, f"top_k {top_k}: drew {sorted(set(tok.tolist()))}, the kept set is {kept}"


@pytest.mark.parametrize("zero_tie", [False, True], ids=["tie", "signed-zero-tie"])
def test_register_kernel_keeps_everything_tied_with_the_kth(zero_tie):
    """five distinct top values, four ids tied at the sixth: top_k = 6 keeps nine, top_k = 5 keeps five; with zero_tie the sixth
    value is 0 as +0.0, -0.0, +0.0, -0.0, which tie by float value"""
    _tie_case(_dev(), False, 512, 576, (7, 100, 255, 256, 511), (3, 64, 300, 510), zero_tie)


@pytest.mark.parametrize("zero_tie", [False, True], ids=["tie", "signed-zero-tie"])
@pytest.mark.parametrize("V", [63, 4097, 65537, 70001, 128256])
def test_streamed_kernel_keeps_everything_tied_with_the_kth(V, zero_tie):
    """the same with the tied ids in different waves' segments, ids 3 and V - 1 among them (65537: V - 1 is the one id of the last
    wave's segment).  V = 1 of the streamed sizes cannot hold the nine ids of a tie case."""
    tied = (3, V // 3, (2 * V) // 3 + 1, V - 1)
    top = (0, V // 5, V // 2, V // 2 + 1, V - 2)
    _tie_case(_dev(), True, V, _ldl(V, tight=(V in (63, 70001))), top, tied, zero_tie)


# =========================================================================================== top-k off: the base entry's bits
def _off_case(dev, wide, V, ldl):
    rows = np.stack([GC.peaked_row(V, seed=5), GC.peaked_row(V, seed=6, scale=1.5), GC.peaked_row(V, seed=7)])
    us = [0.37, 0.81, 0.05]
    seens = [[int(np.argmax(rows[0])), 3, V + 1], [3, 3, V - 1], [int(np.argmax(rows[2]))]]
    for temperature, top_p, penalty in ((0.7, 0.9, 1.3), (1.0, 1.0, 1.0), (0.0, 1.0, 1.3)):
        args = (dev, wide, rows, V, ldl, us, temperature, top_p)
        _, _, t0, l0 = TK.run(*args, None, seens=seens, penalty=penalty)
        for top_k in (0, V, V + 100):
            _, _, t1, l1 = TK.run(*args, top_k, seens=seens, penalty=penalty)
            assert torch.equal(t0, t1) and torch.equal(l0.view(torch.int32), l1.view(torch.int32)), (temperature, top_k)
    # greedy ignores top_k as it ignores top_p
    _, _, t0, l0 = TK.run(dev, wide, rows, V, ldl, us, 0.0, 1.0, None)
    _, _, t1, l1 = TK.run(dev, wide, rows, V, ldl, us, 0.0, 0.5, 2)
    assert torch.equal(t0, t1) and torch.equal(l0.view(torch.int32), l1.view(torch.int32))


@pytest.mark.parametrize("V", [512, 8193, 65536])
def test_register_entry_with_top_k_off_gives_the_base_entrys_bits(V):
    _off_case(_dev(), False, V, _ldl(V))


@pytest.mark.parametrize("V", [1, 63, 4097, 65537, 70001, 128256])
def test_streamed_entry_with_top_k_off_gives_the_base_entrys_bits(V):
    _off_case(_dev(), True, V, _ldl(V, tight=(V in (63, 70001))))


# =========================================================================================== the streamed kernel's spill
def test_streamed_kernel_spills_survivors_to_the_workspace():
    """a flat row with 4000 of its 5000 highest scores in ONE wave's segment, top_k = 5000, top_p = 0.9: that wave's candidate
    list runs past its 512 LDS entries into its part of the workspace (whose guard band topk_case.run checks).  The survivors are the
    planted ids exactly - their scores lie 2 above everything else - and the nucleus edge inside them is not decidable token by
    token, so as test_sample_wide_gpu.py's flat-row test: no drawn token may lie more than 4 V 2^-24 below 1 - top_p in the
    ascending cumulative mass of the survivors, tokens do not decrease with u, the call is deterministic and logp is within
    8 V 2^-24 of the restatement's."""
    dev, V, top_k, top_p = _dev(), 70001, 5000, 0.9
    seg = ((V + 15) // 16 + 255) // 256 * 256
    g = np.random.default_rng(12)
    row = (g.standard_normal(V) * 0.5).astype(np.float32)
    ids = np.concatenate([seg * 2 + np.sort(g.choice(seg, size=4000, replace=False)),      # 4000 in wave 2's segment,
                          seg * 9 + np.sort(g.choice(seg, size=1000, replace=False))])     # 1000 in wave 9's
    row[ids] = (4.0 + 0.5 * g.random(top_k)).astype(np.float32)
    assert row[ids].min() - np.delete(row, ids).max() > 1.0 and top_k > 512 + 1024
    bound = V * U32
    x = row.astype(np.float64)
    surv = np.zeros(V, dtype=bool)
    surv[ids] = True
    p_all = np.where(surv, np.exp(x - x.max()), 0.0)
    p_all /= p_all.sum()
    order = ids[np.argsort(p_all[ids], kind="stable")]
    cum_at = np.zeros(V)
    cum_at[order] = np.cumsum(p_all[order])
    thr = 1.0 - float(np.float32(top_p))
    us = [0.0, U_LAST] + [(k + 0.5) / 64 for k in range(64)]
    tok, logp, t0, l0 = TK.run(dev, True, row, V, _ldl(V), us, 1.0, top_p, top_k)
    assert surv[tok].all(), "a token outside the top_k survivors was drawn"
    assert (cum_at[tok] > thr - 4 * bound).all(), "a token from far below the nucleus was drawn"
    assert len(set(tok.tolist())) >= 32
    assert (np.diff(tok[2:]) >= 0).all() and tok[0] <= tok[2] and tok[1] >= tok[-1]
    _, _, t1, l1 = TK.run(dev, True, row, V, _ldl(V), us, 1.0, top_p, top_k)
    assert torch.equal(t0, t1) and torch.equal(l0.view(torch.int32), l1.view(torch.int32))
    kept_mass = p_all[cum_at > thr].sum()
    assert np.abs(logp - np.log(p_all[tok] / kept_mass)).max() <= 8 * bound
    # without top-p every survivor can be drawn and nothing else: the kept mass is the survivors'
    tok, logp, _, _ = TK.run(dev, True, row, V, _ldl(V), us, 1.0, 1.0, top_k)
    assert surv[tok].all() and np.abs(logp - np.log(p_all[tok])).max() <= 8 * bound


# =========================================================================================== rows alone and among others
@pytest.mark.parametrize("wide", FAMILIES)
def test_rows_are_independent_and_the_call_is_deterministic(wide):
    """M = 3 rows with different logits, uniforms and seen lists against each row alone, against the same call again and against
    the row in another position of another batch: tokens and logp bit for bit"""
    dev, V = _dev(), 70001 if wide else 8193
    rows = np.stack([DC.planted_row(V, 0.7, 1), GC.peaked_row(V, seed=2, scale=1.5), DC.planted_row(V, 0.7, 3)])
    us = [0.37, 0.81, 0.05]
    seens = [DC.planted_seen(V, rows[0]), [3, 3, V // 2, V + 1], [int(np.argmax(rows[2]))]]
    a = dict(temperature=0.7, top_p=0.9, top_k=50, penalty=1.3)
    _, _, t3, l3 = TK.run(dev, wide, rows, V, _ldl(V), us, seens=seens, **a)
    _, _, t3b, l3b = TK.run(dev, wide, rows, V, _ldl(V), us, seens=seens, **a)
    assert torch.equal(t3, t3b) and torch.equal(l3.view(torch.int32), l3b.view(torch.int32)), "the same call twice"
    for m in range(3):
        _, _, t1, l1 = TK.run(dev, wide, rows[m], V, _ldl(V), [us[m]], seens=[seens[m]], **a)
        assert t1[0] == t3[m] and l1.view(torch.int32)[0] == l3.view(torch.int32)[m], f"row {m} alone against row {m} among 3"
    rows5 = np.concatenate([rows[[1, 2, 1, 2]], rows[:1]])
    _, _, t5, l5 = TK.run(dev, wide, rows5, V, _ldl(V), [0.5, 0.5, 0.1, 0.9, us[0]],
                          seens=[seens[1], seens[2], seens[1], seens[2], seens[0]], **a)
    assert t5[4] == t3[0] and l5.view(torch.int32)[4] == l3.view(torch.int32)[0]
