"""rv_sample_token_wide (csrc/sample_wide.hip) through the C ABI: operands in tests/guarded.py windows with the columns behind
V_valid poisoned, tokens against the float64 restatement of tests/generate_case.py, logp inside the fp32 evaluation bound.

    python -m pytest tests/test_sample_wide_gpu.py -m gpu -q"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import divide_case as DC  # noqa: E402
import generate_case as GC  # noqa: E402
from divide_case import U32, U_LAST  # noqa: E402

pytestmark = pytest.mark.gpu

COMBOS = [(0.0, 1.0, 1.0), (0.2, 0.9, 1.0), (0.7, 0.9, 1.0), (0.7, 0.9, 1.3), (1.0, 1.0, 1.3)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _ldl(V, tight=False):
    return V if tight else (V + 3) // 4 * 4 + 64


def _planted_case(dev, V, ldl, temperature, top_p, penalty, seed):
    row = DC.planted_row(V, temperature, seed)
    seen = DC.planted_seen(V, row)
    bound = V * U32
    p, _ = GC.sampler_probs64(row, temperature, top_p, seen, penalty)
    us = DC.planted_uniforms(p, bound)
    tok, logp, _ = DC.run_wide(dev, row, V, ldl, us, temperature, top_p, seen, penalty)
    _, want, ok = DC.check_against_restatement(row, V, us, tok, logp, temperature, top_p, seen, penalty)
    print(f"[wide] V={V} ldl={ldl} T={temperature} top_p={top_p} pen={penalty}: kept {int((p > 0).sum())}, "
          f"{len(us)} uniforms, {len(set(tok.tolist()))} distinct tokens")
    return tok


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "T%g-p%g-pen%g" % c)
@pytest.mark.parametrize("V,tight", [(65537, False), (70001, True), (128256, False)])
def test_planted_rows(V, tight, combo):
    """16-byte loads with a ragged end (65537), unaligned rows that touch each other (70001, ldl = V) and the Llama-3 row"""
    temperature, top_p, penalty = combo
    tok = _planted_case(_dev(), V, _ldl(V, tight), temperature, top_p, penalty, seed=V % 1000 + int(10 * temperature))
    if temperature:
        assert len(set(tok.tolist())) >= 4


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "T%g-p%g-pen%g" % c)
@pytest.mark.parametrize("V", [1, 63, 4097, 32000])
def test_small_vocabularies_through_the_wide_entry(V, combo):
    temperature, top_p, penalty = combo
    _planted_case(_dev(), V, _ldl(V, tight=(V == 63)), temperature, top_p, penalty, seed=V)


@pytest.mark.parametrize("top_p", [1.0, 0.9, 1e-6])
@pytest.mark.parametrize("temperature", [0.0, 0.2, 0.7, 1.0])
def test_v512_stratified_uniforms(temperature, top_p):
    """test_decode_kernels_gpu.py::test_sample_token's row and 4098 uniforms: at most 1 % of them within V 2^-24 of a CDF boundary"""
    V, ldl = 512, 576
    row = GC.peaked_row(V, seed=3)
    us = [0.0, U_LAST] + [(k + 0.5) / 4096 for k in range(4096)]
    tok, logp, _ = DC.run_wide(_dev(), row, V, ldl, us, temperature, top_p)
    DC.check_against_restatement(row, V, us, tok, logp, temperature, top_p, None, 1.0, max_undecidable=0.01)


def test_greedy_takes_the_lowest_index_among_equal_maxima():
    V = 128256
    row = np.zeros(V, dtype=np.float32)
    row[[37, 70000, V - 1]] = 2.5
    tok, logp, _ = DC.run_wide(_dev(), row, V, _ldl(V), [0.3, 0.9], 0.0, 1.0)
    assert tok.tolist() == [37, 37]
    assert abs(logp[0] - (2.5 - math.log(3 * math.exp(2.5) + (V - 3)))) < 1e-5


@pytest.mark.parametrize("V", [65537, 128256])
def test_tiny_top_p_keeps_exactly_the_top_token(V):
    row = DC.planted_row(V, 0.7, seed=4)
    top = int(np.argmax(row))
    us = [0.0, 0.25, 0.5, 0.999, U_LAST]
    tok, logp, _ = DC.run_wide(_dev(), row, V, _ldl(V), us, 0.7, 1e-6)
    assert tok.tolist() == [top] * len(us)
    assert np.abs(logp).max() <= 4 * U32                       # the kept set is one token: log 1


def _flat_row(V, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(V, generator=g) * 1.5).numpy()


def test_flat_row_spills_candidates_to_the_workspace():
    """T = 1, top_p = 0.9 on a flat row: nearly every token is above (1 - top_p) / (2 V), so every wave's candidate list runs past
    its 512 LDS entries into the workspace.  The nucleus edge of such a row is not decidable token by token; what fp32 decides is
    its place in the ascending cumulative mass to within the V-term summation error: no drawn token may lie more than 4 V 2^-24
    below 1 - top_p there, every uniform whose token the float64 restatement decides AND whose kept set is the same must agree."""
    dev, V, top_p = _dev(), 70001, 0.9
    row = _flat_row(V, 7)
    bound = V * U32
    x = row.astype(np.float64)
    p_all = np.exp(x - x.max())
    p_all /= p_all.sum()
    order = np.argsort(p_all, kind="stable")
    cum_at = np.empty(V)
    cum_at[order] = np.cumsum(p_all[order])                    # ascending cumulative mass up to and including each token
    thr = 1.0 - float(np.float32(top_p))
    assert int((p_all > 0.5 * thr / V).sum()) > 16 * 512 + 16 * 1024, "the row must overflow the LDS lists by far"
    us = [0.0, U_LAST] + [(k + 0.5) / 64 for k in range(64)]
    tok, logp, bits = DC.run_wide(dev, row, V, _ldl(V), us, 1.0, top_p)
    assert (cum_at[tok] > thr - 4 * bound).all(), "a token from far below the nucleus was drawn"
    assert len(set(tok.tolist())) >= 32
    # the draw follows vocabulary order: tokens do not decrease with u (u = 0 and the last float come first)
    assert (np.diff(tok[2:]) >= 0).all() and tok[0] <= tok[2] and tok[1] >= tok[-1]
    tok2, _, bits2 = DC.run_wide(dev, row, V, _ldl(V), us, 1.0, top_p)
    assert np.array_equal(tok, tok2) and np.array_equal(bits, bits2)
    # logp: the kept mass is within the summation error of the restatement's, and so is log p of every token
    kept_mass = p_all[cum_at > thr].sum()
    ref = np.log(p_all[tok] / kept_mass)
    assert np.abs(logp - ref).max() <= 8 * bound


def test_rows_are_independent_and_the_call_is_deterministic():
    """M = 3 rows with different logits, uniforms and seen lists (a planted row, a flat one that spills, another planted one)
    against each row alone and against the same call again: tokens and logp bit for bit"""
    dev, V = _dev(), 70001
    rows = np.stack([DC.planted_row(V, 0.7, 1), _flat_row(V, 2), DC.planted_row(V, 0.7, 3)])
    us = [0.37, 0.81, 0.05]
    seens = [DC.planted_seen(V, rows[0]), [3, 3, 40000, V + 1], [int(np.argmax(rows[2]))]]
    args = (0.7, 0.9)
    tok, _, bits = DC.run_wide(dev, rows, V, _ldl(V), us, *args, seens=seens, penalty=1.3)
    tok2, _, bits2 = DC.run_wide(dev, rows, V, _ldl(V), us, *args, seens=seens, penalty=1.3)
    assert np.array_equal(tok, tok2) and np.array_equal(bits, bits2), "the same call twice"
    for m in range(3):
        t1, _, b1 = DC.run_wide(dev, rows[m], V, _ldl(V), [us[m]], *args, seens=[seens[m]], penalty=1.3)
        assert t1[0] == tok[m] and b1[0] == bits[m], f"row {m} alone against row {m} among 3"
    # another batch size and row position: the row last among 5
    rows5 = np.concatenate([rows[[1, 2, 1, 2]], rows[:1]])
    t5, _, b5 = DC.run_wide(dev, rows5, V, _ldl(V), [0.5, 0.5, 0.1, 0.9, us[0]], *args,
                            seens=[seens[1], seens[2], seens[1], seens[2], seens[0]], penalty=1.3)
    assert t5[4] == tok[0] and b5[4] == bits[0]


def test_nothing_is_written_outside_the_declared_workspace():
    """the workspace window is exactly rv_sample_token_wide_workspace_floats(M, V) floats (DC.run_wide checks the band around
    it on every call); here the call that uses most of it - every wave spills - at the largest vocabulary"""
    from rlaif_v_amd import hip
    dev, V = _dev(), 262144
    assert int(hip.lib().lib.rv_sample_token_wide_workspace_floats(2, V)) == 2 * 16 * 16384
    row = _flat_row(V, 11)
    tok, logp, _ = DC.run_wide(dev, row, V, _ldl(V), [0.25, 0.75], 1.0, 0.95)
    assert 0 <= tok[0] <= tok[1] < V and np.isfinite(logp).all()
