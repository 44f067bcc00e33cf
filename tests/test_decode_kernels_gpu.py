"""The three kernels of KV-cached generation (csrc/decode.hip) through the C ABI: containment on tests/guarded.py windows and every
output element against float64 with tests/accuracy.py bounds, built the way test_accuracy_gpu.py builds them for rv_gemm_nt_bf16
and rv_attn_fwd.

    python -m pytest tests/test_decode_kernels_gpu.py -m gpu -q"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy as A  # noqa: E402
import generate_case as GC  # noqa: E402
from accuracy import U32, Val  # noqa: E402
from guarded import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32


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


def rnd(*shape, scale=1.0, seed=0, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


# =========================================================================================== skinny GEMM
# K = 64 c: wave w of the kernel's 8 takes the chunks w, w + 8, ...; four at a time in its deep loop while at least four are left,
# then one at a time.  Up to K = 704 (11 chunks) no wave enters the deep loop.  K = 2112 (33 chunks): every wave runs the deep loop
# once, wave 0 then takes one single chunk (the hand-over).  K = 1792 (28 chunks): waves 0..3 run the deep loop, waves 4..7 only three
# single chunks each.  The 7B depths 4096 and 11008 are these paths repeated.
SKINNY_NK = [(512, 256), (520, 704), (772, 64), (520, 2112), (512, 1792)]
SKINNY_NNZ = 352          # non-zero elements of an A row from K = 704 on
_GEMM_IN = {}


def _gemm_inputs(N, K):
    """(a [64][K], w [N][K], residual [64][N]) on the CPU, computed once.  From K = 704 on an element of a is non-zero with
    probability SKINNY_NNZ / K (a half at K = 704), about 32 of every 64-deep chunk at K = 704 and 10 at K = 2112: the
    accumulation term of the bound counts the non-zero products (accuracy.gemm_E), E grows as nnz^2 and the output ulp as
    sqrt(nnz), so a fixed nnz keeps E under the discrimination cap at any depth, and a chunk left out or taken twice still moves
    an output by several units where the bound is a fraction of an ulp."""
    if (N, K) not in _GEMM_IN:
        a, w, r = rnd(64, K, seed=11 + K), rnd(N, K, seed=12 + N), rnd(64, N, seed=13 + N, scale=3.0)
        if K > 256:
            g = torch.Generator().manual_seed(14)
            a = a * (torch.rand(64, K, generator=g) < SKINNY_NNZ / K).to(BF)
        _GEMM_IN[(N, K)] = (a, w, r)
    return _GEMM_IN[(N, K)]


def _skinny(dev, a, w, res, M, out_f32):
    """one guarded call; returns the output window (checked for containment)"""
    N, K = w.shape
    ga = Guarded(M, K, BF, dev, fill=a[:M], name="A", ld_multiple=8)
    gw = Guarded(N, K, BF, dev, fill=w, name="W", ld_multiple=8)
    gc = Guarded(M, N, F32 if out_f32 else BF, dev, name="C", ld_multiple=4)
    gr = Guarded(M, N, BF, dev, fill=res[:M], name="residual", ld_multiple=4) if res is not None else None
    call("rv_gemm_nt_skinny_bf16", ga.view, ga.ld, gw.view, gw.ld, gc.view, gc.ld, M, N, K, gr.view if gr else None,
         gr.ld if gr else 0, int(out_f32))
    for g in (ga, gw, gr):
        if g is not None:
            g.check()
    gc.check(written=True)
    return gc.view


@pytest.mark.parametrize("out_f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("N,K", SKINNY_NK)
def test_skinny_gemm(N, K, with_res, out_f32):
    """C = A W^T (+ residual): fp32 accumulation of K exact products in any order ((K + 2) 2^-24 |A| |W|), the residual added in
    fp32 (one more rounding, inside Val's +), one rounding at the store."""
    dev = _dev()
    a, w, r = _gemm_inputs(N, K)
    res = r if with_res else None
    for M in (1, 3, 16, 17, 64):
        c = _skinny(dev, a, w, res, M, out_f32)
        acc = A.matmul(a[:M].to(dev), w.to(dev).t())
        val = acc if res is None else acc + res[:M].to(dev).double()
        A.check(c, val.v, val.e, F32 if out_f32 else BF, f"rv_gemm_nt_skinny_bf16 C (M={M} N={N} K={K} res={with_res} f32={out_f32})")


@pytest.mark.parametrize("out_f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("N,K", SKINNY_NK)
def test_skinny_gemm_row_is_independent_of_m(N, K, out_f32):
    """the header's property: row r at M = 1 has the bits of row r at M = 64 (and at M = 17, whose other rows differ)"""
    dev = _dev()
    a, w, r = _gemm_inputs(N, K)
    c64 = _skinny(dev, a, w, r, 64, out_f32).clone()
    other = torch.cat([a[:16], rnd(1, K, seed=5) * 50.0])
    c17 = _skinny(dev, other.to(BF), w, r, 17, out_f32).clone()
    A.check_bits(c17[:16].contiguous(), c64[:16].contiguous(), "rows 0..15 at M = 17 next to a different row 16")
    for row in (0, 15, 16, 63):
        c1 = _skinny(dev, a[row:row + 1], w, r[row:row + 1], 1, out_f32)
        A.check_bits(c1.contiguous(), c64[row:row + 1].contiguous(), f"row {row} at M = 1 against M = 64")


# =========================================================================================== decode attention
SPANS = [(0, 1), (1, 0), (63, 1), (64, 2), (65, 33), (700, 300)]
HD = 128
_ATTN_IN = {}


def _attn_inputs(G, T):
    """Per sequence m < 5: q [H][hd], k, v [kvh][T][hd] from accuracy.spiked_attention_rows (the query is the LAST position):
    sequence 0 = its sequence 0 (query head 0: dominating LAST key; query head H - 1: dominating key 0), sequence 1 = its
    sequence 1 (equal keys in the first quarter, near one-hot head), sequences 2..4 the same recipe from other seeds."""
    if (G, T) not in _ATTN_IN:
        kvh = 2 if G < 4 else 1
        H = G * kvh
        seqs = []
        for seed in (0, 1, 2):
            q, k, v = A.spiked_attention_rows(2, T, H, HD, seed=40 + seed, kv_heads=kvh)
            for s in range(2):
                seqs.append((q[s, :, T - 1].clone(), k[s].clone(), v[s].clone()))
        _ATTN_IN[(G, T)] = (H, kvh, seqs[:5])
    return _ATTN_IN[(G, T)]


def _attn_case(dev, G, M, n_split, pre, own):
    """Lays the sequences into one guarded cache [rows][gap | K heads | gap | V heads] - sequences 0 and 1 share ONE prompt span -
    runs rv_attn_decode and returns per (m, h) the pieces of the check."""
    T = pre + own
    H, kvh, seqs = _attn_inputs(G, T)
    seqs = [list(s) for s in seqs[:M]]
    if M > 1 and pre > 0:                       # sequence 1 continues sequence 0's prompt: the same keys and values in front
        seqs[1][1] = torch.cat([seqs[0][1][:, :pre], seqs[1][1][:, pre:]], 1)
        seqs[1][2] = torch.cat([seqs[0][2][:, :pre], seqs[1][2][:, pre:]], 1)
    kw = kvh * HD
    k_col0, v_col0, cols = 8, 8 + kw + 16, 8 + kw + 16 + kw
    pre_off, own_off, rows = [], [], 3
    for m in range(M):
        if m == 1 and pre > 0:
            pre_off.append(pre_off[0])
        else:
            pre_off.append(rows)
            rows += pre + 2
    for m in range(M):
        own_off.append(rows)
        rows += own + 1
    fill = rnd(rows, cols, seed=77)             # rows and columns no span names hold ordinary values no result may depend on
    inner = torch.ones(rows, cols, dtype=torch.bool)
    for m, (q, k, v) in enumerate(seqs):
        for off, lo, hi in ((pre_off[m], 0, pre), (own_off[m], pre, T)):
            n = hi - lo
            if n == 0:
                continue
            fill[off:off + n, k_col0:k_col0 + kw] = k[:, lo:hi].transpose(0, 1).reshape(n, kw)
            fill[off:off + n, v_col0:v_col0 + kw] = v[:, lo:hi].transpose(0, 1).reshape(n, kw)
            inner[off:off + n, k_col0:k_col0 + kw] = False
            inner[off:off + n, v_col0:v_col0 + kw] = False
    gkv = Guarded(rows, cols, BF, dev, fill=fill, name="kv cache", inner=inner, ld_multiple=8)
    gq = Guarded(M, H * HD, BF, dev, fill=torch.stack([s[0].reshape(-1) for s in seqs]), name="q", ld_multiple=8)
    go = Guarded(M, H * HD, BF, dev, name="out", ld_multiple=8)
    glse = Guarded(1, M * H, F32, dev, name="lse", guard_rows=0)
    from rlaif_v_amd import hip
    need = int(hip.lib().lib.rv_attn_decode_workspace_floats(M, H, n_split))
    assert need == M * H * n_split * 132
    gws = Guarded(1, need, F32, dev, name="workspace", guard_rows=0)
    i32 = lambda v: torch.tensor(v, dtype=I32, device=dev)                 # noqa: E731
    call("rv_attn_decode", gq.view, gq.ld, gkv.view, gkv.ld, k_col0, v_col0, i32(pre_off), i32([pre] * M), i32(own_off),
         i32([own] * M), go.view, go.ld, glse.view, M, H, HD, G, 1.0 / math.sqrt(HD), n_split, gws.view, need)
    gkv.check(), gq.check(), gws.check()
    go.check(written=True), glse.check(written=True)
    return H, seqs, go.view.clone(), glse.view.reshape(M, H).clone()


def _attn_bound(q, k, v, dev):
    """rv_attn_decode, one head: accuracy.attn_fwd_bound's derivation for one query row over T keys WITHOUT its documented bf16
    rounding of P (the header: p stays fp32), plus the merges this kernel adds to the per-batch rescales the bound counts as
    `tiles` (64 keys per batch and workgroup): two butterfly steps, the wave merge and the split merge - each multiplies l and o
    by an exp2 of a difference of maxima (4 x 2^-24 relative, as a tile) = 16 x 2^-24 on |out| + P |v|, and on lse."""
    q, k, v = q.to(dev).double()[None], k.to(dev).double(), v.to(dev).double()
    T = k.shape[0]
    ok = torch.ones(1, T, dtype=torch.bool, device=dev)
    scale = 1.0 / math.sqrt(HD)
    ov, doc, lv = A.attn_fwd_bound(q, k, v, ok, scale)
    P = torch.softmax(scale * (q @ k.t()), -1)
    extra = 16.0 * U32 * (ov.v.abs() + P @ v.abs())
    return ov.v[0], (ov.e - doc + extra)[0], lv.v, lv.e + 16.0 * U32


@pytest.mark.parametrize("n_split", [1, 3, 8])
@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("G", [1, 2, 4])
def test_attn_decode(G, M, n_split):
    """every span pair of the issue; one check per output tensor over all of them (as test_accuracy_gpu.py checks all sequences
    and heads of a case at once).  n_split = 3 and 8 leave splits without keys on the short spans."""
    dev = _dev()
    go, ro, eo, gl, rl, el = [], [], [], [], [], []
    for pre, own in SPANS:
        H, seqs, out, lse = _attn_case(dev, G, M, n_split, pre, own)
        for m, (q, k, v) in enumerate(seqs):
            for h in range(H):
                r, e, lr, le = _attn_bound(q[h], k[h // G], v[h // G], dev)
                go.append(out[m, h * HD:(h + 1) * HD]), ro.append(r), eo.append(e)
                gl.append(lse[m, h:h + 1]), rl.append(lr), el.append(le)
    what = f"rv_attn_decode (kv_group {G}, M {M}, n_split {n_split})"
    A.check(torch.cat(go), torch.cat(ro), torch.cat(eo), BF, what + " out")
    A.check(torch.cat(gl), torch.cat(rl), torch.cat(el), F32, what + " lse")


@pytest.mark.parametrize("n_split", [1, 3])
@pytest.mark.parametrize("G", [1, 4])
def test_attn_decode_sequence_is_independent_of_the_others(G, n_split):
    dev = _dev()
    for pre, own in ((65, 33), (0, 1)):
        _, _, out5, lse5 = _attn_case(dev, G, 5, n_split, pre, own)
        _, _, out1, lse1 = _attn_case(dev, G, 1, n_split, pre, own)
        A.check_bits(out1.contiguous(), out5[:1].contiguous(), f"sequence 0 alone against sequence 0 among 5 (spans {pre}, {own})")
        A.check_bits(lse1.contiguous(), lse5[:1].contiguous(), "its lse")


# =========================================================================================== sampler
V, LDL = 512, 576
U_LAST = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
_ROW = {}


def _row(Vn=V):
    """The logits row, chosen on the CPU: peaked (generate_case.peaked_row), so that the restatement itself leaves at most 1 % of
    the planted uniforms undecidable and no nucleus edge near a tie - asserted by the tests that use it."""
    if Vn not in _ROW:
        _ROW[Vn] = GC.peaked_row(Vn, seed=3) if Vn == V else GC.peaked_row(Vn, seed=10, scale=8.0)
    return _ROW[Vn]


def _sample(dev, row, Vn, ldl, us, temperature, top_p, seen=None, penalty=1.0):
    """n = len(us) rows holding the same logits, the columns behind V_valid and the rows around the window poisoned"""
    n = len(us)
    inner = torch.zeros(n, ldl, dtype=torch.bool)
    inner[:, Vn:] = True
    fill = torch.zeros(n, ldl)
    fill[:, :Vn] = torch.from_numpy(row)[None]
    gl = Guarded(n, ldl, F32, dev, fill=fill, name="logits", inner=inner, guard_cols=0)
    assert gl.ld == ldl
    gu = Guarded(1, n, F32, dev, fill=torch.tensor(us, dtype=F32)[None], name="u", guard_rows=0)
    gt = Guarded(1, n, I32, dev, name="token", guard_rows=0)
    gp = Guarded(1, n, F32, dev, name="logp", guard_rows=0)
    so = si = None
    if seen is not None:                        # every row names the same list
        si = torch.tensor(list(seen) * n, dtype=I32, device=dev)
        so = torch.arange(n + 1, dtype=I32, device=dev) * len(seen)
    call("rv_sample_token", gl.view, gl.ld, n, Vn, so, si, float(penalty), float(temperature), float(top_p), gu.view, gt.view, gp.view)
    gl.check(), gu.check()
    gt.check(written=True), gp.check(written=True)
    return gt.view[0].cpu().numpy().astype(np.int64), gp.view[0].cpu().double().numpy()


def _logp_bound(row, p, temperature, seen=None, penalty=1.0):
    """|logp - log p_tok| of the fp32 evaluation (x_t - max) - log(sum exp(x_i - max)): the division by the temperature and the
    penalty (2^-24 |x| each, on x_t and on the maximum), the subtraction, per term exp's (|x_i - max| + 2) 2^-23 and the two
    operand roundings weighted by the term's share, the V-term sum, logf (FEW) and the last subtraction."""
    x = GC.penalised(row, seen, penalty) / (float(np.float32(temperature)) if temperature else 1.0)
    mx = x.max()
    kept = p > 0
    rel = ((np.abs(x - mx) + 2.0) * 2.0 * U32 + 2.0 * U32 * (np.abs(x) + abs(mx)))
    zerr = float((p * rel)[kept].sum()) + int(kept.sum()) * U32
    lz = np.log(np.exp(x[kept] - mx).sum())
    return lambda t: (2.0 * U32 * (abs(x[t]) + abs(mx)) + U32 * abs(x[t] - mx) + zerr + A.FEW * U32 * abs(lz)
                      + U32 * abs(np.log(p[t])) + 2.0 * U32)


@pytest.mark.parametrize("top_p", [1.0, 0.9, 1e-6])
@pytest.mark.parametrize("temperature", [0.0, 0.2, 0.7, 1.0])
def test_sample_token(temperature, top_p):
    """u = 0, the largest float below 1 and 4096 stratified values on one row: the token is the float64 restatement's for every
    u farther from a CDF boundary than the fp32 error of a V-term sum (V 2^-24, accuracy.py's n 2^-24 sum |terms| with the
    terms summing to 1); at most 1 % of the planted values may be that close, asserted on the restatement."""
    dev = _dev()
    row = _row()
    us = [0.0, U_LAST] + [(k + 0.5) / 4096 for k in range(4096)]
    p, edge = GC.sampler_probs64(row, temperature, top_p)
    bound = V * U32
    assert edge > 4 * bound, f"the nucleus edge is {edge:.3e} from a tie: pick another row"
    tok, logp = _sample(dev, row, V, LDL, us, temperature, top_p)
    u64 = np.asarray(np.float32(us), dtype=np.float64)
    if temperature == 0.0:
        want, dist = np.full(len(us), int(np.argmax(row))), np.full(len(us), np.inf)
    else:
        want, dist = GC.sampler_choice64(p, u64)
    decidable = dist > bound
    frac = 1.0 - decidable.mean()
    print(f"[sampler] T={temperature} top_p={top_p}: kept {int((p > 0).sum())} of {V}, {100 * frac:.3f} % of the uniforms within "
          f"{bound:.2e} of a CDF boundary, tokens drawn: {len(set(tok.tolist()))} distinct")
    assert frac <= 0.01, "the row leaves more than 1 % of the planted uniforms undecidable: pick another row"
    assert (p[tok] > 0).all(), "a token outside the kept set was drawn"
    bad = np.nonzero(decidable & (tok != want))[0]
    assert bad.size == 0, f"{bad.size} draws differ from the restatement, first u = {us[bad[0]]!r}: {tok[bad[0]]} vs {want[bad[0]]}"
    eb = _logp_bound(row, p, temperature)
    for t in np.unique(tok):
        err = np.abs(logp[tok == t] - np.log(p[t])).max()
        assert err <= eb(t), f"logp of token {t}: error {err:.3e} > bound {eb(t):.3e}"


def test_sample_token_full_vocabulary_and_penalty():
    """one row at V_valid = 32000 (the 32-ids-per-thread kernel, unpadded rows) with a repetition penalty over a seen list that
    contains the top token, ids out of range and duplicates"""
    dev = _dev()
    Vn = 32000
    row = _row(Vn)
    top = int(np.argmax(row))
    seen = [top, top, 5, Vn - 1, -1, Vn + 7, int(np.argsort(row)[-2])]
    bound = Vn * U32                            # 1.9e-3: coarse, so the uniforms are planted where the restatement can decide -
    for temperature, top_p, pen in ((0.0, 1.0, 1.0), (0.7, 0.9, 1.0), (0.7, 0.9, 1.3), (1.0, 1.0, 1.3), (0.0, 1.0, 4.0)):
        sl = seen if pen != 1.0 else None
        p, edge = GC.sampler_probs64(row, temperature, top_p, sl, pen)
        assert edge > 4 * bound
        kept = np.nonzero(p > 0)[0]             # - the middle of every CDF interval wider than 8 bounds (at most 64), 0 and the last float
        hi = np.cumsum(p[kept])
        wide = np.argsort(-p[kept])[:64]
        wide = wide[p[kept][wide] > 8 * bound]
        us = [0.0, U_LAST] + [float(np.float32(hi[i] - 0.5 * p[kept][i])) for i in wide]
        tok, logp = _sample(dev, row, Vn, Vn, us, temperature, top_p, seen=sl, penalty=pen)
        if temperature == 0.0:
            want, dist = np.full(len(us), int(np.argmax(GC.penalised(row, sl, pen)))), np.full(len(us), np.inf)
        else:
            want, dist = GC.sampler_choice64(p, np.asarray(np.float32(us), dtype=np.float64))
            assert len(set(want.tolist())) >= min(3, len(wide)), "the planted uniforms should reach several tokens"
        ok = dist > bound
        assert ok[2:].all(), "every planted interval middle is decidable by construction"
        assert (tok[ok] == want[ok]).all(), (temperature, top_p, pen)
        eb = _logp_bound(row, p, temperature, sl, pen)
        for t in np.unique(tok):
            assert np.abs(logp[tok == t] - np.log(p[t])).max() <= eb(t)


def test_sample_token_greedy_takes_the_lowest_index_among_equal_maxima():
    dev = _dev()
    row = np.zeros(V, dtype=np.float32)
    row[[37, 300, 511]] = 2.5
    tok, logp = _sample(dev, row, V, LDL, [0.3, 0.9], 0.0, 1.0)
    assert tok.tolist() == [37, 37]
    assert abs(logp[0] - (2.5 - math.log(3 * math.exp(2.5) + (V - 3)))) < 1e-5
