"""rv_beam_topk_penalty (csrc/beam.hip) through the C ABI: rv_beam_topk with HF's RepetitionPenaltyLogitsProcessor between the
log-softmax and the score add.  Every operand, the history table included, is a tests/guarded.py window; outputs are held against
float64 (tests/beam_penalty_case.py).

Bound (beam_penalty_case.penalised_bound): beam_case.logsoftmax_add_bound at score 0 gives lp and E per element; a penalised id
carries E x penalty + 2^-24 |lp x penalty| (the product's rounding); the score add contributes 2^-24 |value| once more.  Order and
values are then checked the way tests/test_beam_kernels_gpu.py::_check_topk checks rv_beam_topk: float64's candidate at every rank
whose two neighbours are more than the sum of their bounds away, at most 10 % of the ranks undecided, every value within the
largest bound of its group.  The float64 side uses the fp32 value of the penalty, which is what the kernel is handed.

Inputs: test_beam_topk_random_rows' logits and scores (the same seeds); every row has a history of 9 ids - the ids of its 4
largest logits, 4 random ids, and the first id again - at penalty 1.1.  Penalising the leaders reorders the candidates, so a
kernel that ignores the history fails the comparison with the un-penalised list, which the test asserts to differ.

    python -m pytest tests/test_beam_topk_penalty_gpu.py -m gpu -q"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy as A  # noqa: E402
import beam_case as BC  # noqa: E402
import beam_penalty_case as PC  # noqa: E402
from accuracy import U32  # noqa: E402
from guarded import Guarded  # noqa: E402
from test_beam_kernels_gpu import _dev, _topk, call  # noqa: E402  (call() stops the session on a HIP error)

pytestmark = pytest.mark.gpu

F32, F64, I32 = torch.float32, torch.float64, torch.int32
PENALTY = 1.1
_DIFFERS = {}


def _inputs(V, G, K):
    gen = torch.Generator().manual_seed(1000 * K + 10 * G + V % 7)
    logits = (torch.randn(G * K, V, generator=gen) * 3).float()
    score = (-torch.rand(G * K, generator=gen) * 4).float()
    return logits, score, gen


def _history(logits, gen):
    """int32 [rows, 9]: the ids of the row's 4 largest logits, 4 random ids, the first id again"""
    M, V = logits.shape
    top = torch.topk(logits, 4, dim=-1).indices
    rnd = torch.randint(0, V, (M, 4), generator=gen)
    return torch.cat([top, rnd, top[:, :1]], 1).to(I32)


def _pen(dev, logits, score, G, K, V, hist, n_hist, penalty, vec=True, ld_h=None, hist_fill=-7, null_hist=False, tight=False):
    """rv_beam_topk_penalty on guarded operands (the layout of test_beam_kernels_gpu._topk: 7 NaN columns behind V_valid).
    ``hist`` int32 [G K, <= ld_h] (CPU) fills the first columns of a [G K, ld_h] window whose other entries are ``hist_fill``;
    ``tight``: no guard columns, the table's row stride IS ld_h (guard rows above and below stay).
    Returns (value [G, 2K], parent, token, lse [G K]) on the CPU."""
    from rlaif_v_amd import hip
    M, n = G * K, 2 * K
    cols = V + 7
    fill = torch.full((M, cols), float("nan"), dtype=F32)
    fill[:, :V] = logits
    gl = Guarded(M, cols, F32, dev, fill=fill, name="logits", ld_multiple=4 if vec else 1,
                 guard_cols=256 if vec or (cols + 512) % 4 else 257)
    assert (gl.ld % 4 == 0) == vec
    gs = Guarded(1, M, F32, dev, fill=torch.as_tensor(score, dtype=F32).reshape(1, M), name="score", guard_rows=0)
    width = int(ld_h if ld_h is not None else max(hist.shape[1], 1))
    hf = torch.full((M, width), hist_fill, dtype=I32)
    hf[:, :hist.shape[1]] = hist
    gh = Guarded(M, width, I32, dev, fill=hf, name="hist", **(dict(guard_cols=0) if tight else {}))
    assert gh.ld == (width if tight else width + 512)
    gv = Guarded(1, G * n, F32, dev, name="cand_val", guard_rows=0)
    gp = Guarded(1, G * n, I32, dev, name="cand_parent", guard_rows=0)
    gt = Guarded(1, G * n, I32, dev, name="cand_tok", guard_rows=0)
    glse = Guarded(1, M, F32, dev, name="lse", guard_rows=0)
    need = int(hip.lib().lib.rv_beam_topk_workspace_floats(G, K))
    gws = Guarded(1, need, F32, dev, name="workspace", guard_rows=0)
    call("rv_beam_topk_penalty", gl.view, gl.ld, gs.view, G, K, V, None if null_hist else gh.view, gh.ld, int(n_hist), float(penalty),
         gv.view, gp.view, gt.view, glse.view, gws.view, need)
    gl.check(), gs.check(), gh.check()
    for g in (gv, gp, gt, glse, gws):
        g.check(written=True)
    return (gv.view.reshape(G, n).cpu(), gp.view.reshape(G, n).cpu(), gt.view.reshape(G, n).cpu(), glse.view.reshape(M).cpu())


def _check(logits, score, G, K, V, hist, got, what, allow=0.1):
    """test_beam_kernels_gpu._check_topk on the penalised values; returns (undecided ranks, ranks, groups whose candidate list
    differs from the un-penalised float64 list)"""
    val, par, tok, lse = got
    n = 2 * K
    hists = [h.tolist() for h in hist]
    v64, e64 = PC.penalised_bound(logits.numpy(), np.asarray(score, dtype=np.float64), hists, PC.f32(PENALTY))
    p64 = BC.log_softmax64(logits.numpy()) + np.asarray(score, dtype=np.float64)[:, None]
    undecided = differs = 0
    ref_v, ref_e = [], []
    for g in range(G):
        fv, fe = v64[g * K:(g + 1) * K].reshape(-1), e64[g * K:(g + 1) * K].reshape(-1)
        order = np.lexsort((np.arange(fv.shape[0]), -fv))[:n + 1]
        rv, re = fv[order], fe[order]
        apart = (rv[:-1] - rv[1:]) > (re[:-1] + re[1:])
        for i in range(n):
            if (i == 0 or apart[i - 1]) and apart[i]:
                assert (int(par[g, i]), int(tok[g, i])) == (int(order[i] // V), int(order[i] % V)), \
                    f"{what}: group {g} rank {i}: device ({int(par[g, i])}, {int(tok[g, i])}), float64 ({order[i] // V}, {order[i] % V})"
            else:
                undecided += 1
        assert all(0 <= int(t) < V and 0 <= int(p) < K for p, t in zip(par[g], tok[g])), f"{what}: a candidate outside [0, V_valid)"
        ref_v.append(torch.as_tensor(rv[:n])), ref_e.append(torch.full((n,), float(re.max()), dtype=F64))
        pf = p64[g * K:(g + 1) * K].reshape(-1)
        plain = np.lexsort((np.arange(pf.shape[0]), -pf))[:n]
        differs += int(plain.tolist() != order[:n].tolist())
    A.check(val.reshape(-1), torch.cat(ref_v), torch.cat(ref_e), F32, what + " values")
    lse64 = torch.logsumexp(torch.as_tensor(logits.numpy().astype(np.float64)), -1)           # un-penalised
    e_lse = BC.logsoftmax_add_bound(logits.numpy(), np.zeros(G * K))[1].max(-1)
    A.check(lse, lse64, torch.as_tensor(e_lse) + U32 * lse64.abs(), F32, what + " lse")
    assert undecided <= allow * G * n, f"{what}: {undecided} of {G * n} ranks undecided"
    return undecided, G * n, differs


SHAPES = [(V, G, K) for V in (512, 8192, 8193, 32000, 32003) for G, K in ((1, 1), (3, 3), (1, 8), (3, 8))]


@pytest.mark.parametrize("V,G,K", SHAPES)
def test_penalised_rows(V, G, K):
    dev = _dev()
    logits, score, gen = _inputs(V, G, K)
    hist = _history(logits, gen)
    got = _pen(dev, logits, score, G, K, V, hist, 9, PENALTY)
    und, tot, differs = _check(logits, score, G, K, V, hist, got, f"rv_beam_topk_penalty (V {V}, G {G}, K {K})")
    _DIFFERS[(V, G, K)] = differs
    print(f"[beam_topk_penalty] V {V} G {G} K {K}: {und} of {tot} ranks undecided, the penalty changes the list of {differs} of {G} groups")


def test_the_penalty_changes_a_candidate_list_of_the_run():
    """float64 alone, on the inputs of test_penalised_rows: a kernel that ignored ``hist`` would have to return the un-penalised
    list, and that list is another one in at least one group (in most with K >= 3) - so it cannot have passed above."""
    _dev()
    differs = 0
    for V, G, K in SHAPES:
        if (V, G, K) not in _DIFFERS:
            logits, score, gen = _inputs(V, G, K)
            hists = [h.tolist() for h in _history(logits, gen)]
            n = 2 * K
            for g in range(G):
                sl = slice(g * K, (g + 1) * K)
                pen = PC.topk_candidates(logits[sl].numpy(), score[sl].numpy(), n, hists[sl], PC.f32(PENALTY))
                plain = BC.topk_candidates(logits[sl].numpy(), score[sl].numpy(), n)
                _DIFFERS[(V, G, K)] = _DIFFERS.get((V, G, K), 0) + int((pen[1][:n].tolist(), pen[2][:n].tolist())
                                                                        != (plain[1][:n].tolist(), plain[2][:n].tolist()))
        differs += _DIFFERS[(V, G, K)]
    assert differs >= 1


@pytest.mark.parametrize("V,G,K", [(512, 3, 3), (8193, 1, 8), (32003, 3, 3)])
def test_penalty_off_is_rv_beam_topk_bit_for_bit(V, G, K):
    dev = _dev()
    logits, score, gen = _inputs(V, G, K)
    hist = _history(logits, gen)
    plain = _topk(dev, logits, score, G, K, V)
    for what, kw in (("penalty 1.0", dict(n_hist=9, penalty=1.0)), ("n_hist 0", dict(n_hist=0, penalty=PENALTY)),
                     ("hist NULL", dict(n_hist=0, penalty=PENALTY, null_hist=True)),
                     ("hist NULL, penalty 1.0", dict(n_hist=9, penalty=1.0, null_hist=True))):
        got = _pen(dev, logits, score, G, K, V, hist, **kw)
        for a, b in zip(got, plain):
            assert torch.equal(a, b), f"{what}: rv_beam_topk's bits on every output"


@pytest.mark.parametrize("V", [512, 32003])
def test_long_history_with_ids_out_of_range(V):
    """n_hist = ld_h = 1024 (one id per thread): the row's 9 ids repeated, with -1, V_valid, 2^30, -2^31 and V_valid + 31 (inside the
    last word of the bit set when V_valid is no multiple of 32) strewn among them.  Same bits as the 9 ids alone - a duplicate is
    penalised once, an id outside [0, V_valid) not at all - and nothing but the outputs written."""
    dev = _dev()
    G, K = 3, 3
    logits, score, gen = _inputs(V, G, K)
    hist = _history(logits, gen)
    want = _pen(dev, logits, score, G, K, V, hist, 9, PENALTY)
    long = hist.repeat(1, 114)[:, :1024].clone()                 # 9 x 114 = 1026 columns
    junk = torch.tensor([-1, V, 2 ** 30, -2 ** 31, V + 31], dtype=torch.int64).to(I32)
    for i, c in enumerate(range(9, 1024, 50)):                   # columns >= 9: the first 9 keep every distinct id in the row
        long[:, c] = junk[i % 5]
    assert all(set(PC.distinct_ids(long[m].tolist(), V)) == set(PC.distinct_ids(hist[m].tolist(), V)) for m in range(G * K))
    got = _pen(dev, logits, score, G, K, V, long, 1024, PENALTY, ld_h=1024, tight=True)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    _check(logits, score, G, K, V, hist, got, f"rv_beam_topk_penalty (V {V}, 1024 ids)")


def test_entries_behind_n_hist_are_not_read():
    dev = _dev()
    V, G, K = 8193, 3, 3
    logits, score, gen = _inputs(V, G, K)
    hist = _history(logits, gen)
    want = _pen(dev, logits, score, G, K, V, hist, 9, PENALTY)
    poison = torch.cat([hist, torch.topk(logits, 12, dim=-1).indices[:, 4:].to(I32)], 1)       # the next 8 leaders behind n_hist
    got = _pen(dev, logits, score, G, K, V, poison, 9, PENALTY, ld_h=40, hist_fill=int(logits[0].argmax()))
    for a, b in zip(got, want):
        assert torch.equal(a, b), "ld_h > n_hist: in-range ids behind n_hist change nothing"
    moved = _pen(dev, logits, score, G, K, V, poison, 17, PENALTY, ld_h=40)
    assert not all(torch.equal(a, b) for a, b in zip(moved[:3], want[:3])), "... and do once n_hist covers them"


@pytest.mark.parametrize("V", [512, 8193, 32003])
def test_row_stride_that_defeats_the_vector_loads(V):
    dev = _dev()
    G, K = 3, 3
    logits, score, gen = _inputs(V, G, K)
    hist = _history(logits, gen)
    got = _pen(dev, logits, score, G, K, V, hist, 9, PENALTY, vec=False)
    _check(logits, score, G, K, V, hist, got, f"rv_beam_topk_penalty (V {V}, scalar loads)")
    vec = _pen(dev, logits, score, G, K, V, hist, 9, PENALTY, vec=True)
    for a, b in zip(got, vec):
        assert torch.equal(a, b), "the same bits whichever way the row is loaded"


def test_refusals():
    """rc 1 and a text that starts with the entry point's name; nothing is launched"""
    dev = _dev()
    from rlaif_v_amd import hip
    G, K, V = 2, 3, 512
    M, n = G * K, 2 * K
    lg = torch.zeros(M, V, dtype=F32, device=dev)
    sc = torch.zeros(M, dtype=F32, device=dev)
    hs = torch.zeros(M, 16, dtype=I32, device=dev)
    val, par, tok = (torch.zeros(G * n, dtype=dt, device=dev) for dt in (F32, I32, I32))
    lse = torch.zeros(M, dtype=F32, device=dev)
    need = int(hip.lib().lib.rv_beam_topk_workspace_floats(G, K))
    ws = torch.zeros(need + 1, dtype=F32, device=dev)
    off1 = lambda t: t.data_ptr() + 1                                     # noqa: E731  (a misaligned address)

    def args(**kw):
        a = dict(logits=lg, ldl=V, score=sc, G=G, K=K, V=V, hist=hs, ld_h=16, n_hist=4, penalty=PENALTY, val=val, par=par, tok=tok,
                 lse=lse, ws=ws, wsn=need)
        a.update(kw)
        return [a[k] for k in ("logits", "ldl", "score", "G", "K", "V", "hist", "ld_h", "n_hist", "penalty", "val", "par", "tok", "lse",
                               "ws", "wsn")]

    call("rv_beam_topk_penalty", *args())                                # the base case is accepted
    bad = [
        # everything rv_beam_topk refuses
        (dict(K=0), "K <= 8"), (dict(K=9), "K <= 8"), (dict(G=0), "G >= 1"), (dict(G=30000, K=3), "65535"),
        (dict(V=65537, ldl=65537), "65536"), (dict(V=5), "2 K"), (dict(ldl=V - 1), "ldl"),
        (dict(logits=None), "NULL"), (dict(score=None), "NULL"), (dict(val=None), "NULL"), (dict(par=None), "NULL"),
        (dict(tok=None), "NULL"), (dict(lse=None), "NULL"), (dict(ws=None), "NULL"),
        (dict(logits=off1(lg)), "aligned"), (dict(ws=off1(ws)), "aligned"), (dict(wsn=need - 1), "workspace"),
        # its own
        (dict(penalty=0.0), "penalty"), (dict(penalty=-1.1), "penalty"), (dict(penalty=float("nan")), "penalty"),
        (dict(n_hist=-1), "n_hist"), (dict(n_hist=17), "n_hist"),
        (dict(hist=None), "hist is NULL"), (dict(hist=off1(hs)), "hist must be 4-byte aligned"),
        (dict(ld_h=2 ** 31 // M + 1), "int32"),
    ]
    for kw, text in bad:
        with pytest.raises(RuntimeError) as e:
            call("rv_beam_topk_penalty", *args(**kw))
        msg = str(e.value)
        assert "rc=1" in msg and ": rv_beam_topk_penalty: " in msg and text in msg, (kw, msg)
    # rv_beam_topk keeps its own name in the shared checks
    with pytest.raises(RuntimeError, match=r"rc=1\): rv_beam_topk: 1 <= K <= 8"):
        call("rv_beam_topk", lg, V, sc, G, 9, V, val, par, tok, lse, ws, need)
