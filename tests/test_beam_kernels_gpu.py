"""The three kernels of beam-search decoding (csrc/beam.hip, rv_attn_decode_indexed in csrc/decode.hip) through the C ABI:
containment on tests/guarded.py windows, every output against float64 with tests/accuracy.py bounds (rv_beam_topk,
rv_attn_decode_indexed) or against the float64 restatement of transformers' beam search (rv_beam_step, tests/beam_case.py).

rv_beam_topk's bound: beam_case.logsoftmax_add_bound - the kernel's formula ((x - max) - log Z) + score written with
accuracy.Val, E per element (about 1e-5 for logits of size 10, 60 for a dead beam's values near -1e9).  Two candidates are
ORDERED by float64 when their values differ by more than the sum of their two E; the device must give float64's candidate at
every rank whose two neighbours are ordered that way, and at most 10 % of the ranks may be left undecided.  The values are held
to E at every rank (the i-th largest of a set moves by at most the largest perturbation of an element).

    python -m pytest tests/test_beam_kernels_gpu.py -m gpu -q"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy as A  # noqa: E402
import beam_case as BC  # noqa: E402
from accuracy import U32  # noqa: E402
from guarded import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
HD = 128


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def call(name, *args):
    from rlaif_v_amd import hip
    try:
        hip.call(name, *args)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):      # a faulted device: start nothing more on it
            pytest.exit(f"GPU fault in {name}: {e}", returncode=3)
        raise


# =========================================================================================== rv_beam_topk
def _topk(dev, logits, score, G, K, V, vec=True, pad="nan"):
    """logits fp32 [G K, V] (CPU), score [G K]: runs rv_beam_topk on guarded operands whose logits window has 7 padding columns
    behind V_valid (NaN or huge: never a candidate).  ``vec=False``: a row stride that is no multiple of 4 (the scalar loads).
    Returns (value [G, 2K], parent, token, lse [G K]) on the CPU."""
    from rlaif_v_amd import hip
    M, n = G * K, 2 * K
    cols = V + 7
    fill = torch.full((M, cols), float("nan") if pad == "nan" else 3.0e38, dtype=F32)
    fill[:, :V] = logits
    gl = Guarded(M, cols, F32, dev, fill=fill, name="logits", ld_multiple=4 if vec else 1,
                 guard_cols=256 if vec or (cols + 512) % 4 else 257)
    assert (gl.ld % 4 == 0) == vec
    gs = Guarded(1, M, F32, dev, fill=torch.as_tensor(score, dtype=F32).reshape(1, M), name="score", guard_rows=0)
    gv = Guarded(1, G * n, F32, dev, name="cand_val", guard_rows=0)
    gp = Guarded(1, G * n, I32, dev, name="cand_parent", guard_rows=0)
    gt = Guarded(1, G * n, I32, dev, name="cand_tok", guard_rows=0)
    glse = Guarded(1, M, F32, dev, name="lse", guard_rows=0)
    need = int(hip.lib().lib.rv_beam_topk_workspace_floats(G, K))
    assert need == M * n * 2
    gws = Guarded(1, need, F32, dev, name="workspace", guard_rows=0)
    call("rv_beam_topk", gl.view, gl.ld, gs.view, G, K, V, gv.view, gp.view, gt.view, glse.view, gws.view, need)
    gl.check(), gs.check()
    for g in (gv, gp, gt, glse, gws):
        g.check(written=True)
    return (gv.view.reshape(G, n).cpu(), gp.view.reshape(G, n).cpu(), gt.view.reshape(G, n).cpu(), glse.view.reshape(M).cpu())


def _check_topk(logits, score, G, K, V, got, what, allow=0.1):
    """against float64: order where decided, values everywhere; returns (undecided ranks, ranks)"""
    val, par, tok, lse = got
    n = 2 * K
    v64, e64 = BC.logsoftmax_add_bound(logits.numpy(), np.asarray(score, dtype=np.float64))
    undecided = 0
    ref_v, ref_e = [], []
    for g in range(G):
        fv, fe = v64[g * K:(g + 1) * K].reshape(-1), e64[g * K:(g + 1) * K].reshape(-1)
        order = np.lexsort((np.arange(fv.shape[0]), -fv))[:n + 1]
        rv, re = fv[order], fe[order]
        apart = (rv[:-1] - rv[1:]) > (re[:-1] + re[1:])                    # rank i and i + 1 are ordered by float64
        for i in range(n):
            if (i == 0 or apart[i - 1]) and apart[i]:
                assert (int(par[g, i]), int(tok[g, i])) == (int(order[i] // V), int(order[i] % V)), \
                    f"{what}: group {g} rank {i}: device ({int(par[g, i])}, {int(tok[g, i])}), float64 ({order[i] // V}, {order[i] % V})"
            else:
                undecided += 1
        assert all(0 <= int(t) < V and 0 <= int(p) < K for p, t in zip(par[g], tok[g])), f"{what}: a candidate outside [0, V_valid)"
        ref_v.append(torch.as_tensor(rv[:n])), ref_e.append(torch.full((n,), float(re.max()), dtype=F64))
    A.check(val.reshape(-1), torch.cat(ref_v), torch.cat(ref_e), F32, what + " values")
    x = torch.as_tensor(logits.numpy().astype(np.float64))
    lse64 = torch.logsumexp(x, -1)
    e_lse = BC.logsoftmax_add_bound(logits.numpy(), np.zeros(G * K))[1].max(-1)        # max + log Z: the same terms, no score
    A.check(lse, lse64, torch.as_tensor(e_lse) + U32 * lse64.abs(), F32, what + " lse")
    assert undecided <= allow * G * n, f"{what}: {undecided} of {G * n} ranks undecided"
    return undecided, G * n


@pytest.mark.parametrize("G,K", [(1, 1), (3, 1), (1, 3), (3, 3), (1, 4), (3, 4), (1, 8), (3, 8)])
@pytest.mark.parametrize("V", [512, 8192, 8193, 32000, 32003])
def test_beam_topk_random_rows(V, G, K):
    dev = _dev()
    gen = torch.Generator().manual_seed(1000 * K + 10 * G + V % 7)
    logits = (torch.randn(G * K, V, generator=gen) * 3).float()
    score = (-torch.rand(G * K, generator=gen) * 4).float()
    got = _topk(dev, logits, score, G, K, V, pad="nan" if (G + K) % 2 else "huge")
    und, tot = _check_topk(logits, score, G, K, V, got, f"rv_beam_topk (V {V}, G {G}, K {K})")
    print(f"[beam_topk] V {V} G {G} K {K}: {und} of {tot} ranks undecided")


@pytest.mark.parametrize("V", [512, 8193, 32003])
def test_beam_topk_row_stride_that_defeats_the_vector_loads(V):
    dev = _dev()
    gen = torch.Generator().manual_seed(V)
    logits = (torch.randn(9, V, generator=gen) * 3).float()
    score = (-torch.rand(9, generator=gen) * 4).float()
    got = _topk(dev, logits, score, 3, 3, V, vec=False)
    _check_topk(logits, score, 3, 3, V, got, f"rv_beam_topk (V {V}, scalar loads)")
    vec = _topk(dev, logits, score, 3, 3, V, vec=True)
    for a, b in zip(got, vec):
        assert torch.equal(a, b), "the same bits whichever way the row is loaded"


def test_beam_topk_planted_rows():
    """V = 8200 (32 ids per thread: thread boundaries at multiples of 32, wave boundaries at multiples of 2048), G = 2, K = 3.  Every
    planted winner stands at least 0.01 above the next one (the float64 reference leaves no rank undecided) or is an EXACT tie."""
    dev = _dev()
    V, G, K = 8200, 2, 3
    n = 2 * K
    base = (torch.randn(G * K, V, generator=torch.Generator().manual_seed(5)) * 0.5).float()
    # group 0: the step-0 score vector (one live beam, K - 1 dead); winners in the last ids before V_valid and across thread
    # and wave boundaries
    lg = base.clone()
    for i, t in enumerate([V - 1, 2047, 2048, 31, V - 2, 32]):
        lg[0, t] = 20.0 - 0.5 * i
    # group 1: all 2K winners in one row (beam 1), inside ONE thread's ids (64 .. 69): the owner rescans after every round
    lg[4, 64:64 + n] = torch.tensor([30.0 - 0.25 * i for i in range(n)])
    score = torch.tensor([0.0, -1.0e9, -1.0e9, -3.0, 0.0, -3.0])
    got = _topk(dev, lg, score, G, K, V)
    val, par, tok, lse = got
    und, tot = _check_topk(lg, score, G, K, V, got, "rv_beam_topk (planted)", allow=0.0)
    assert und == 0
    assert par[0].tolist() == [0] * n and tok[0].tolist() == [V - 1, 2047, 2048, 31, V - 2, 32]
    assert par[1].tolist() == [1] * n and tok[1].tolist() == list(range(64, 64 + n))
    assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(lse).all())
    # a dead beam loses to EVERY live candidate: with 2K > V_valid-many live ones impossible, so ask for them at K = 3, V = 6:
    # all six candidates come from beam 0 although beams 1 and 2 hold larger logits
    small = torch.tensor([[0.0, 1.0, 2.0, 3.0, 4.0, 5.0], [50.0] * 6, [60.0] * 6])
    v2, p2, t2, _ = _topk(dev, small, torch.tensor([0.0, -1.0e9, -1.0e9]), 1, 3, 6)
    assert p2[0].tolist() == [0] * 6 and t2[0].tolist() == [5, 4, 3, 2, 1, 0] and bool(torch.isfinite(v2).all())
    # exact ties: equal values order by the lower flat index beam * V + token - inside a row and across rows of equal score
    tie = torch.zeros(3, 512)
    tie[:, 100] = tie[:, 7] = tie[:, 300] = 4.0
    v3, p3, t3, _ = _topk(dev, tie, torch.tensor([-1.0, -1.0, -1.0]), 1, 3, 512)
    assert list(zip(p3[0].tolist(), t3[0].tolist())) == [(0, 7), (0, 100), (0, 300), (1, 7), (1, 100), (1, 300)]
    assert len(set(v3[0].tolist())) == 1, "equal rows, equal scores: equal bits"
    # ... and all of a dead group's candidates tie at -1e9: the first 2K ids of its first row
    v4, p4, t4, _ = _topk(dev, tie, torch.tensor([-1.0e9, -1.0e9, -1.0e9]), 1, 3, 512)
    assert bool(torch.isfinite(v4).all()) and float(v4.max()) <= -9.9e8 and p4[0].tolist() == [0] * 6


# =========================================================================================== rv_beam_step
EOS = 5


class _DevBeams:
    """rv_beam_step's buffers as guarded windows; the two table buffers swap after every step"""

    def __init__(self, dev, G, K, T, own_base):
        M = G * K
        self.G, self.K, self.T, self.M, self.own_base, self.dev = G, K, T, M, own_base, dev
        sc = torch.full((G, K), -1.0e9)
        sc[:, 0] = 0.0
        z = lambda r, c, v: torch.full((r, c), v, dtype=I32)                # noqa: E731
        self.score = Guarded(1, M, F32, dev, fill=sc.reshape(1, M), name="run_score", guard_rows=0, role="io")
        self.parent = Guarded(1, M, I32, dev, name="parent", guard_rows=0)
        self.token = Guarded(1, M, I32, dev, name="token", guard_rows=0)
        self.hist = [Guarded(M, T, I32, dev, fill=z(M, T, -7), name=f"hist {s}", role="io") for s in "AB"]
        self.rows = [Guarded(M, T, I32, dev, fill=z(M, T, -7), name=f"own_rows {s}", role="io") for s in "AB"]
        self.hyp_tokens = Guarded(1, M * T, I32, dev, fill=z(1, M * T, -7), name="hyp_tokens", guard_rows=0, role="io")
        self.hyp_len = Guarded(1, M, I32, dev, fill=z(1, M, 0), name="hyp_len", guard_rows=0, role="io")
        self.hyp_score = Guarded(1, M, F32, dev, fill=torch.full((1, M), -1.0e9), name="hyp_score", guard_rows=0, role="io")
        self.n_hyp = Guarded(1, G, I32, dev, fill=z(1, G, 0), name="n_hyp", guard_rows=0, role="io")
        self.done = Guarded(1, G, I32, dev, fill=z(1, G, 0), name="done", guard_rows=0, role="io")
        self.cur = 0

    def step(self, j, cand, eos=EOS, lp=1.0, forced=None):
        G, K, T = self.G, self.K, self.T
        n = 2 * K
        gc = [Guarded(1, G * n, dt, self.dev, fill=torch.as_tensor(np.asarray(c)).to(dt).reshape(1, G * n), name=nm, guard_rows=0)
              for c, dt, nm in zip(cand, (F32, I32, I32), ("cand_val", "cand_parent", "cand_tok"))]
        f = [None, None, None]
        if forced is not None:
            f = [torch.as_tensor(np.asarray(x)).to(device=self.dev, dtype=dt).contiguous() for x, dt in zip(forced, (I32, I32, F32))]
        a, b = self.cur, 1 - self.cur
        assert self.hist[a].ld == T + 512 and self.rows[a].ld == self.hist[a].ld
        call("rv_beam_step", gc[0].view, gc[1].view, gc[2].view, G, K, T, j, eos, float((j + 1) ** lp), int(j == T - 1), self.own_base,
             f[0], f[1], f[2], self.score.view, self.parent.view, self.token.view, self.hist[a].view, self.hist[b].view,
             self.rows[a].view, self.rows[b].view, self.hist[a].ld, self.hyp_tokens.view, self.hyp_len.view, self.hyp_score.view,
             self.n_hyp.view, self.done.view)
        for g in gc + [self.score, self.hist[a], self.hist[b], self.rows[a], self.rows[b], self.hyp_tokens, self.hyp_len,
                       self.hyp_score, self.n_hyp, self.done]:
            g.check()
        self.parent.check(written=True), self.token.check(written=True)
        self.cur = b
        cpu = lambda g, *shape: g.view.cpu().reshape(*shape)                # noqa: E731
        return dict(parent=cpu(self.parent, G, K), token=cpu(self.token, G, K), score=cpu(self.score, G, K),
                    hist=cpu(self.hist[b], G, K, T), rows=cpu(self.rows[b], G, K, T), hyp_tokens=cpu(self.hyp_tokens, G, K, T),
                    hyp_len=cpu(self.hyp_len, G, K), hyp_score=cpu(self.hyp_score, G, K), n_hyp=cpu(self.n_hyp, G),
                    done=cpu(self.done, G))


def _script(K, T, nb, eos_ranks, parents=None, seed=0):
    """One group's candidate lists: step j has the 2K values -(j + 1) nb[j] - c / 8 (c = rank: descending, exact in fp32), tokens
    10 .. 99 with EOS planted at eos_ranks[j], parents random or as given."""
    rng = np.random.default_rng(seed)
    steps = []
    for j in range(T):
        n = 2 * K
        val = np.array([-(j + 1) * nb[j] - c / 8.0 for c in range(n)])
        tok = rng.integers(10, 100, n)
        for c in eos_ranks[j]:
            tok[c] = EOS
        par = rng.integers(0, K, n) if parents is None or parents[j] is None else np.array(parents[j])
        steps.append((val, par, tok))
    return steps


def _run_step_case(dev, scripts, K, T, eos=EOS, lp=1.0):
    """the groups' scripts through rv_beam_step and through beam_case.Group64, compared after every step"""
    G, own_base = len(scripts), 1000
    M = G * K
    devb = _DevBeams(dev, G, K, T, own_base)
    refs = [BC.Group64(K, T, eos, lp) for _ in range(G)]
    ref_rows = [[[] for _ in range(K)] for _ in range(G)]
    log = []
    for j in range(T):
        cand = [np.stack([scripts[g][j][i] for g in range(G)]) for i in range(3)]
        got = devb.step(j, cand, eos, lp)
        outs = []
        for g in range(G):
            was_done = refs[g].done
            r = refs[g].step(None, scripts[g][j])
            outs.append(r)
            what = f"group {g} step {j}"
            assert got["parent"][g].tolist() == r["parent"].tolist() and got["token"][g].tolist() == r["token"].tolist(), what
            assert np.allclose(got["score"][g].numpy(), r["score"], rtol=2 * U32, atol=0), what
            ref_rows[g] = [ref_rows[g][int(p)] + [own_base + j * M + g * K + b] for b, p in enumerate(r["parent"])]
            for b in range(K):
                assert got["hist"][g, b, :j + 1].tolist() == refs[g].tokens[b], what + f" beam {b}: token history"
                assert got["rows"][g, b, :j + 1].tolist() == ref_rows[g][b], what + f" beam {b}: cache-row table"
                assert got["hist"][g, b, j + 1:].tolist() == [-7] * (T - j - 1), what + ": entries past j are not written"
            assert int(got["n_hyp"][g]) == len(refs[g].hyps), what
            # slots are not sorted and equal scores have no order: both sides by (tokens, score); hypotheses may share their tokens
            dev_h = sorted((got["hyp_tokens"][g, s, :int(got["hyp_len"][g, s])].tolist(), float(got["hyp_score"][g, s]))
                           for s in range(int(got["n_hyp"][g])))
            ref_h = sorted((h["tokens"], h["score"]) for h in refs[g].hyps)
            assert [t for t, _ in dev_h] == [t for t, _ in ref_h], what + ": finished set"
            for (_, ds), (_, hs) in zip(dev_h, ref_h):
                assert abs(ds - hs) <= 2 * U32 * abs(hs), what + ": finished score"
            assert bool(got["done"][g]) == r["done"], what
            assert not was_done or not r["entered"]
        log.append(outs)
    return refs, log


def test_beam_step_against_the_restatement():
    dev = _dev()
    K, T = 3, 8
    none = [[]] * T
    scripts = [
        # 0: no EOS; a permutation, then a collapse (all parents equal), alternating
        _script(K, T, [2.0] * T, none, parents=[[2, 0, 1, 1, 2, 0] if j % 2 else [1] * 6 for j in range(T)], seed=1),
        # 1: EOS at rank < K (twice): finished early, search goes on
        _script(K, T, [2.0, 2.0, 2.0, 2.1, 2.2, 2.3, 2.4, 2.5], [[], [0], [2], [], [], [], [], []], seed=2),
        # 2: EOS at rank >= K only: ignored by the finished set, skipped by the running beams
        _script(K, T, [2.0] * T, [[], [3], [4, 5], [3, 4, 5], [], [], [], []], seed=3),
        # 3: the finished set overflows K (the worst, -3.0, is evicted at step 3), then the done condition is met at step 4
        _script(K, T, [3.0, 2.5, 2.0, 1.5, 4.0, 4.0, 4.0, 4.0], [[0], [1], [0], [2], [], [], [], []], seed=4),
        # 4: the set fills at step 1; step 2 narrowly NOT done (best running -2.0625 > worst -2.125), step 3 done on equality
        _script(K, T, [2.0, 1.0, 2.0625, 2.125, 9.0, 9.0, 9.0, 9.0], [[0, 1], [2], [], [], [1], [], [], []], seed=5),
    ]
    refs, log = _run_step_case(dev, scripts, K, T)
    assert [len(r.hyps) for r in refs] == [3, 3, 3, 3, 3]
    assert not any(s["done"] for s in log[T - 2][:3]) and all(s["done"] for s in log[T - 1]), "groups 0 - 2 end at the last step"
    assert [h["step"] for h in refs[0].hyps] == [T - 1] * 3 and all(len(h["tokens"]) == T for h in refs[0].hyps)
    assert sorted(h["step"] for h in refs[1].hyps) == [1, 2, T - 1] and refs[1].best()[0][-1] == EOS and len(refs[1].best()[0]) == 2
    assert all(h["step"] == T - 1 and EOS not in h["tokens"][:-1] for h in refs[2].hyps)
    assert [s[3]["done"] for s in log[:6]] == [False, False, False, False, True, True]
    assert sorted(h["score"] for h in refs[3].hyps) == [-2.5625, -2.0, -1.5625], "the worst (-3.0) was evicted"
    assert [s[4]["done"] for s in log[:5]] == [False, False, False, True, True] and log[2][4]["margin_fin"] == 0.0625
    assert len(refs[4].hyps) == 3 and not log[4][4]["entered"], "a done group's finished set is frozen"


def test_beam_step_single_beam_and_length_penalty():
    dev = _dev()
    T = 5
    scripts = [_script(1, T, [2.0] * T, [[], [1], [0], [], []], seed=7), _script(1, T, [2.0, 1.5, 1.0, 3.0, 3.0], [[], [], [0], [], []], seed=8)]
    refs, log = _run_step_case(dev, scripts, 1, T)
    assert refs[0].best()[0][-1] == EOS and len(refs[0].best()[0]) == 3
    for lp in (0.0, 2.0):
        _run_step_case(dev, [_script(3, 6, [2.0, 1.9, 1.8, 1.7, 2.5, 2.5], [[1], [0], [], [2], [], []], seed=9)], 3, 6, lp=lp)
    _run_step_case(dev, [_script(8, 4, [2.0] * 4, [[0, 9], [3], [], []], seed=10)], 8, 4)


def test_beam_step_forced_beams_leave_the_finished_set_alone():
    dev = _dev()
    K, T = 3, 4
    devb = _DevBeams(dev, 1, K, T, 50)
    sc = _script(K, T, [2.0] * T, [[0], [], [], []], seed=11)
    forced = [(np.array([0, 0, 0]), np.array([11, 12, 13]), np.array([-1.0, -2.0, -3.0])),
              (np.array([2, 2, 0]), np.array([21, 22, 23]), np.array([-1.5, -2.5, -3.5]))]
    for j in range(2):
        got = devb.step(j, [c[None] for c in sc[j]], forced=forced[j])
        assert got["parent"][0].tolist() == forced[j][0].tolist() and got["token"][0].tolist() == forced[j][1].tolist()
        assert got["score"][0].tolist() == forced[j][2].tolist()
        assert int(got["n_hyp"][0]) == 0 and int(got["done"][0]) == 0
    assert got["hist"][0, :, :2].tolist() == [[13, 21], [13, 22], [11, 23]]
    assert got["rows"][0, :, :2].tolist() == [[52, 53], [52, 54], [50, 55]]


# =========================================================================================== rv_attn_decode_indexed
_ATTN_IN = {}


def _attn_inputs(G, T):
    """six sequences (G = 2 groups of K = 3 beams), H = 8 query heads on 8 / G kv heads: q [H][hd], k, v [kvh][T][hd] from
    accuracy.spiked_attention_rows (the query is the LAST position), as tests/test_decode_kernels_gpu.py builds them"""
    if (G, T) not in _ATTN_IN:
        kvh = 8 // G
        seqs = []
        for seed in (0, 1, 2):
            q, k, v = A.spiked_attention_rows(2, T, 8, HD, seed=60 + seed, kv_heads=kvh)
            for s in range(2):
                seqs.append([q[s, :, T - 1].clone(), k[s].clone(), v[s].clone()])
        _ATTN_IN[(G, T)] = seqs
    return [list(s) for s in _ATTN_IN[(G, T)]]


def _attn_bound(q, k, v, dev):
    """tests/test_decode_kernels_gpu.py's bound of rv_attn_decode (the indexed kernel's arithmetic is the same): accuracy.attn_fwd_bound
    for one query row without its documented bf16 rounding of P, plus 16 x 2^-24 for the four merges"""
    q, k, v = q.to(dev).double()[None], k.to(dev).double(), v.to(dev).double()
    ok = torch.ones(1, k.shape[0], dtype=torch.bool, device=dev)
    scale = 1.0 / math.sqrt(HD)
    ov, doc, lv = A.attn_fwd_bound(q, k, v, ok, scale)
    P = torch.softmax(scale * (q @ k.t()), -1)
    extra = 16.0 * U32 * (ov.v.abs() + P @ v.abs())
    return ov.v[0], (ov.e - doc + extra)[0], lv.v, lv.e + 16.0 * U32


def _idx_case(dev, G, n_split, pre, own, identity=False, seed=0):
    """M = 6 sequences = 2 groups of 3 beams.  The beams of a group share ONE prompt span and the cache rows of their first
    own // 2 own tokens (a common ancestor).  Own rows lie scattered through the cache in a random permutation; every cache row
    no sequence names is guard (NaN), table entries past the own length name such a row INSIDE the buffer.
    ``identity``: contiguous own rows in order instead (what rv_attn_decode can express) and no sharing of own rows."""
    from rlaif_v_amd import hip
    M, K, H, T, LD = 6, 3, 8, pre + own, own + 3
    kvh = H // G
    seqs = _attn_inputs(G, T)
    shared = 0 if identity else own // 2
    for m in range(M):
        lead = (m // K) * K
        if m != lead:
            for i in (1, 2):
                seqs[m][i] = torch.cat([seqs[lead][i][:, :pre + shared], seqs[m][i][:, pre + shared:]], 1)
    kw = kvh * HD
    k_col0, v_col0, cols = 8, 8 + kw + 16, 8 + kw + 16 + kw
    n_own = M * own if identity else 2 * shared + M * (own - shared)
    rows = 3 + 2 * (pre + 2) + n_own + 5
    rng = np.random.default_rng(seed + 100 * pre + own)
    pool = list(range(3 + 2 * (pre + 2), rows - 2))
    if not identity:
        pool = rng.permutation(pool).tolist()
    nan_row = rows - 1
    pre_off = [3 + (m // K) * (pre + 2) for m in range(M)]
    table = np.full((M, LD), nan_row, dtype=np.int64)
    for m in range(M):
        lead = (m // K) * K
        for t in range(own):
            table[m, t] = table[lead, t] if (m != lead and t < shared) else pool.pop(0)
    fill = torch.zeros(rows, cols)
    inner = torch.ones(rows, cols, dtype=torch.bool)
    for m, (q, k, v) in enumerate(seqs):
        dst = [pre_off[m] + t for t in range(pre)] + table[m, :own].tolist()
        for t, r in enumerate(dst):
            fill[r, k_col0:k_col0 + kw] = k[:, t].reshape(kw).float()
            fill[r, v_col0:v_col0 + kw] = v[:, t].reshape(kw).float()
            inner[r, k_col0:k_col0 + kw] = False
            inner[r, v_col0:v_col0 + kw] = False
    gkv = Guarded(rows, cols, BF, dev, fill=fill, name="kv cache", inner=inner, ld_multiple=8)
    gq = Guarded(M, H * HD, BF, dev, fill=torch.stack([s[0].reshape(-1) for s in seqs]), name="q", ld_multiple=8)
    gtab = Guarded(M, LD, I32, dev, fill=torch.as_tensor(table), name="own_rows")
    need = int(hip.lib().lib.rv_attn_decode_workspace_floats(M, H, n_split))
    i32 = lambda v: torch.tensor(v, dtype=I32, device=dev)                 # noqa: E731
    res = []
    for plain in ((False, True) if identity else (False,)):
        go = Guarded(M, H * HD, BF, dev, name="out", ld_multiple=8)
        glse = Guarded(1, M * H, F32, dev, name="lse", guard_rows=0)
        gws = Guarded(1, need, F32, dev, name="workspace", guard_rows=0)
        if plain:
            call("rv_attn_decode", gq.view, gq.ld, gkv.view, gkv.ld, k_col0, v_col0, i32(pre_off), i32([pre] * M), i32(table[:, 0]),
                 i32([own] * M), go.view, go.ld, glse.view, M, H, HD, G, 1.0 / math.sqrt(HD), n_split, gws.view, need)
        else:
            call("rv_attn_decode_indexed", gq.view, gq.ld, gkv.view, gkv.ld, rows, k_col0, v_col0, i32(pre_off), i32([pre] * M),
                 gtab.view, gtab.ld, own, i32([own] * M), go.view, go.ld, glse.view, M, H, HD, G, 1.0 / math.sqrt(HD), n_split,
                 gws.view, need)
        gkv.check(), gq.check(), gtab.check(), gws.check()
        go.check(written=True), glse.check(written=True)
        res.append((go.view.clone(), glse.view.reshape(M, H).clone()))
    return seqs, res


PRE, OWN = [1, 5, 70], [1, 2, 17, 65]


@pytest.mark.parametrize("n_split", [1, 3])
@pytest.mark.parametrize("G", [1, 4])
def test_attn_decode_indexed(G, n_split):
    """H = 8, M = 6, every (pre_len, own length) pair: own spans that cross the 16-key batches and the 64-key trip, n_split = 3 with
    empty splits on the short ones.  A wrong row shows as NaN (every unused cache row is guard), never as a fault."""
    dev = _dev()
    go, ro, eo, gl, rl, el = [], [], [], [], [], []
    for pre in PRE:
        for own in OWN:
            seqs, [(out, lse)] = _idx_case(dev, G, n_split, pre, own)
            for m, (q, k, v) in enumerate(seqs):
                for h in range(8):
                    r, e, lr, le = _attn_bound(q[h], k[h // G], v[h // G], dev)
                    go.append(out[m, h * HD:(h + 1) * HD]), ro.append(r), eo.append(e)
                    gl.append(lse[m, h:h + 1]), rl.append(lr), el.append(le)
    what = f"rv_attn_decode_indexed (kv_group {G}, n_split {n_split})"
    A.check(torch.cat(go), torch.cat(ro), torch.cat(eo), BF, what + " out")
    A.check(torch.cat(gl), torch.cat(rl), torch.cat(el), F32, what + " lse")


@pytest.mark.parametrize("n_split", [1, 3])
@pytest.mark.parametrize("G", [1, 4])
def test_attn_decode_indexed_identity_table_is_rv_attn_decode_bit_for_bit(G, n_split):
    dev = _dev()
    for pre, own in ((1, 1), (5, 17), (70, 65), (5, 2)):
        _, [(out_i, lse_i), (out_p, lse_p)] = _idx_case(dev, G, n_split, pre, own, identity=True)
        A.check_bits(out_i.contiguous(), out_p.contiguous(), f"identity table against rv_attn_decode (spans {pre}, {own})")
        A.check_bits(lse_i.contiguous(), lse_p.contiguous(), "its lse")
