"""Host tests of tests/accuracy.py: the per-element bound must pass every honest fp32 evaluation (one rounding at the store), reject
the planted defects that the whole-tensor bounds of close() let through, and stay silent on a legitimate 1-ulp variation.  The
"kernels" are torch functions on the CPU; no GPU is needed."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy as A  # noqa: E402
from accuracy import Val, BF, F32, F64, U32  # noqa: E402


def rnd(*shape, scale=1.0, seed=0, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def trunc_bf16(x32: torch.Tensor) -> torch.Tensor:
    """the planted store defect: drop the low 16 bits instead of rounding to nearest even"""
    return (x32.contiguous().view(torch.int32) & -65536).view(F32).to(BF)


def fails(what: str, got, val: Val, dtype=BF, doc=None):
    """the check must fail and name the operand"""
    with pytest.raises(A.AccuracyError) as e:
        A.check(got, val.v, val.e, dtype, what, doc=doc)
    assert not isinstance(e.value, A.CapError), f"{what}: refused by the cap, not by the bound: {e.value}"
    assert str(e.value).startswith(what + ":"), str(e.value)
    return str(e.value)


def passes(what: str, got, val: Val, dtype=BF, doc=None, cap_unit="ulp"):
    return A.check(got, val.v, val.e, dtype, what, doc=doc, cap_unit=cap_unit)


# ------------------------------------------------------------------------------------------------------ the helper itself
def test_ulp_at_binade_edges():
    r = torch.tensor([1.0, 2.0 - 2.0 ** -20, 2.0, 0.75, 2.0 ** -126, 2.0 ** -140, 0.0], dtype=F64)
    assert A.ulp(r, BF).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -133, 2.0 ** -133, 2.0 ** -133]
    assert A.ulp(r, F32).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24, 2.0 ** -149, 2.0 ** -149, 2.0 ** -149]
    # the ulp of the bound is taken at |ref64| + E: a reference just below a binade whose unrounded value may sit above it
    ref = torch.tensor([2.0 - 2.0 ** -9], dtype=F64)
    assert A.bound(ref, torch.tensor([2.0 ** -8], dtype=F64), BF).item() == 0.5 * 2.0 ** -6 + 2.0 ** -8
    assert A.bound(ref, torch.tensor([0.0], dtype=F64), BF).item() == 0.5 * 2.0 ** -7


def test_rne_matches_torch_and_ties_go_to_even():
    g = torch.Generator().manual_seed(0)
    t = (torch.randn(100000, generator=g, dtype=F64) * torch.exp(torch.randn(100000, generator=g, dtype=F64) * 20)).float().double()
    assert torch.equal(A.rne(t, BF), t.float().to(BF).double())
    assert A.rne(torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=F64), BF).tolist() == [1.0, 1.0 + 2.0 ** -6]
    x, want = A.bf16_midpoints()
    assert x.numel() == 3 * 65280 and torch.equal(x.to(BF).view(torch.int16).to(torch.int32) & 0xFFFF, want)
    assert A.all_finite_bf16().numel() == 65280 and bool(torch.isfinite(A.all_finite_bf16().float()).all())


def test_overflow_to_inf_and_flush_to_zero():
    big = torch.tensor([3.4e38, -3.4e38], dtype=F64)                        # RNE to bf16 overflows
    A.check(torch.tensor([math.inf, -math.inf]).to(BF), big, 0.0, BF, "overflow")
    for bad in ([3.3895e38, -math.inf], [math.inf, math.inf]):
        with pytest.raises(A.AccuracyError, match="must be that inf"):
            A.check(torch.tensor(bad).to(BF), big, 0.0, BF, "overflow")
    tiny = torch.tensor([1e-39, -1e-39, 0.0, 1e-39], dtype=F64)
    A.check(torch.tensor([0.0, 0.0, -0.0, -(2.0 ** -126)]), tiny, 0.0, F32, "flush")          # zero of either sign, up to 2^-126
    with pytest.raises(A.AccuracyError):
        A.check(torch.tensor([0.0, 0.0, 0.0, 3e-38]), tiny, 0.0, F32, "flush")
    with pytest.raises(A.AccuracyError, match="NaN"):
        A.check(torch.tensor([0.0, math.nan, 0.0, 0.0]), tiny, 0.0, F32, "flush")
    with pytest.raises(A.AccuracyError):                                                        # a normal value is not flushed
        A.check(torch.tensor([0.0]), torch.tensor([2.0 ** -120], dtype=F64), 0.0, F32, "flush")


def test_cap_fires_and_message_format():
    ref = torch.linspace(1.0, 2.0, 64, dtype=F64).reshape(8, 8)
    with pytest.raises(A.CapError, match="median E / ulp"):
        A.check(ref.to(BF), ref, 2.0 ** -7, BF, "inflated")
    E = torch.zeros_like(ref)
    E[0] = 1.0                                                               # a few cancelling elements may have a large E
    A.check(ref.to(BF), ref, E, BF, "one loose row")
    got = ref.to(BF).clone()
    got[5, 3] += 0.125
    with pytest.raises(A.AccuracyError) as e:
        A.check(got, ref, 0.0, BF, "C of some kernel")
    msg = str(e.value)
    for part in ("C of some kernel:", "1 of 64 element(s)", "worst at index (5, 3)", "ref64 1.68253968", "got 1.8046875", "bound 0.00390625",
                 "max error / bound", "% of the elements differ from RNE(ref64)", "mean signed error"):
        assert part in msg, (part, msg)
    with pytest.raises(ValueError):                                          # nothing of the bound may come from a broken case
        A.check(got, ref, -1.0, BF, "negative E")
    with pytest.raises(ValueError, match="cannot be switched off"):
        A.check(ref.to(BF), ref, 0.0, BF, "no cap", cap=False)


def test_val_terms():
    x = Val(torch.tensor([3.0], dtype=F64))
    assert (x + 1.0).e.item() == pytest.approx(4 * U32) and (x * 2.0).e.item() == pytest.approx(6 * U32 + A.DENORM)
    assert (x * x).sum(0).e.item() == pytest.approx(9 * U32 + A.DENORM)      # a single term: no addition
    s = Val(torch.ones(8, dtype=F64)).sum(0)
    assert s.e.item() == pytest.approx(7 * 8 * U32) and Val(torch.ones(8, dtype=F64)).sum(0, depth=3).e.item() == pytest.approx(24 * U32)
    y = x.bf16()
    with A.no_doc():
        assert x.bf16().e.item() == 0.0
    assert y.e.item() == 3 * A.U16
    with pytest.raises(ValueError):
        (1.0 / Val(torch.tensor([1e-9], dtype=F64), 1e-8))


# ------------------------------------------------------------------------------------------------------ GEMM + epilogue
def act32(z, act):
    if act == 1:
        return z / (1 + torch.exp(-1.702 * z))
    if act == 2:
        return 0.5 * z * (1 + torch.erf(z * 0.70710678118654752))
    if act == "tanh":
        return 0.5 * z * (1 + torch.tanh(0.7978845608028654 * (z + 0.044715 * z ** 3)))
    return z


def gemm_val(a, b, bias, res, act, alpha):
    z = A.matmul(a, b.t(), alpha) + bias.double()[None, :]
    y = z / (1.0 + (-(Val.const(1.702) * z)).exp()) if act == 1 else A.gelu(z) if act == 2 else z
    return y + res.double()


def gemm32(a, b, bias, res, act, alpha, acc_bf16=False, round_before_residual=False):
    """the honest stand-in (fp32 throughout, one rounding) and its planted accumulation / residual defects"""
    af, bf = a.float(), b.float()
    if acc_bf16:
        acc = torch.zeros(a.shape[0], b.shape[0])
        for k in range(0, a.shape[1], 64):
            acc = (acc + af[:, k:k + 64] @ bf[:, k:k + 64].t()).to(BF).float()
    else:
        acc = af @ bf.t()
    y = act32(alpha * acc + bias.float(), act)
    if round_before_residual:
        y = y.to(BF).float()
    return y + res.float()


EPI_SHAPES = {"test_gemm_epilogues": (300, 256, 320, 0.5), "K64": (130, 136, 64, 0.7071)}


def epi_inputs(name):
    M, N, K, s = EPI_SHAPES[name]
    return rnd(M, K, seed=3, scale=s), rnd(N, K, seed=4, scale=s), rnd(N, seed=5), rnd(M, N, seed=6)


@pytest.mark.parametrize("shape", list(EPI_SHAPES))
@pytest.mark.parametrize("act", [0, 1, 2])
def test_gemm_epilogue_honest_passes(shape, act):
    a, b, bias, res = epi_inputs(shape)
    e = passes("C", gemm32(a, b, bias, res, act, 0.5).to(BF), gemm_val(a, b, bias, res, act, 0.5))
    assert e["ratio"] <= 1.0


@pytest.mark.parametrize("asked,computed,shape", [(2, 1, "test_gemm_epilogues"), (1, 2, "test_gemm_epilogues"), (2, "tanh", "K64")])
def test_gemm_epilogue_wrong_activation_fails(asked, computed, shape):
    a, b, bias, res = epi_inputs(shape)
    fails("C", gemm32(a, b, bias, res, computed, 0.5).to(BF), gemm_val(a, b, bias, res, asked, 0.5))


def test_gemm_truncating_store_bf16_accumulator_and_early_rounding_fail():
    a, b, bias, res = epi_inputs("test_gemm_epilogues")
    val = gemm_val(a, b, bias, res, 2, 0.5)
    fails("C", trunc_bf16(gemm32(a, b, bias, res, 2, 0.5)), val)
    fails("C", gemm32(a, b, bias, res, 2, 0.5, acc_bf16=True).to(BF), val)
    fails("C", gemm32(a, b, bias, res, 2, 0.5, round_before_residual=True).to(BF), val)


def test_cancelling_gemm_builder():
    a, b = A.cancelling_gemm(130, 136, 256, seed=7)
    ref, mag = a.double() @ b.double().t(), a.double().abs() @ b.double().abs().t()
    small = (ref.abs() < 2.0 ** -6 * mag)
    assert 0.30 < small.double().mean().item() < 0.5 and bool(small[:, torch.arange(136) % 8 < 3].double().mean() > 0.95)
    val = A.matmul(a, b.t())
    passes("C", (a.float() @ b.float().t()).to(BF), val)
    fails("C", trunc_bf16(a.float() @ b.float().t()), val)


# ------------------------------------------------------------------------------------------------------ unary kernels
def test_gelu_exhaustive_honest_and_tanh():
    x = A.all_finite_bf16()
    passes("y", act32(x.float(), 2).to(BF), A.gelu(x))
    fails("y", act32(x.float(), "tanh").to(BF), A.gelu(x))
    fails("y", trunc_bf16(act32(x.float(), 2)), A.gelu(x))


def swiglu_val(g, u):
    gv = Val(g)
    return gv / (1.0 + (-gv).exp()) * u.double()


@pytest.mark.parametrize("up", [1.0, -3.0, 2.0 ** -20])
def test_swiglu_exhaustive_honest_and_one_ulp_sigmoid(up):
    g = A.all_finite_bf16()
    u = torch.full_like(g, up)
    gf, uf = g.float(), u.float()
    passes("act", (gf / (1 + torch.exp(-gf)) * uf).to(BF), swiglu_val(g, u))
    # the withdrawn v_rcp_f32 experiment: the logistic one fp32 ulp off, in either direction - another legitimate fp32 evaluation
    sg = 1 / (1 + torch.exp(-gf))
    for direction in (math.inf, -math.inf):
        sg1 = torch.nextafter(sg, torch.full_like(sg, direction))
        passes("act", (gf * sg1 * uf).to(BF), swiglu_val(g, u))
    fails("act", trunc_bf16(gf / (1 + torch.exp(-gf)) * uf), swiglu_val(g, u))


def test_log_sigmoid_naive_at_minus_104_fails():
    bz = Val(torch.tensor([-104.0, -20.0, 0.0, 20.0], dtype=F64))
    loss = (-bz).maximum(0.0) + (-(bz.abs())).exp().log1p()
    loss = Val(F.softplus(-bz.v), loss.e)
    x = bz.v.float()
    passes("losses", torch.clamp(-x, min=0) + torch.log1p(torch.exp(-x.abs())), loss, F32)
    fails("losses", -torch.log(1 / (1 + torch.exp(-x))), loss, F32)


# ------------------------------------------------------------------------------------------------------ norms
def rms32(x, w, eps):
    xf = x.float()
    return xf * torch.rsqrt((xf * xf).sum(1, keepdim=True) / x.shape[1] + eps) * w.float()


def rms_val(x, w, eps):
    xv, d = Val(x), x.shape[1]
    rs = ((xv * xv).sum(1, keepdim=True) / float(d) + float(torch.tensor(eps, dtype=F32))).rsqrt()
    return xv * rs * w.double()[None, :]


@pytest.mark.parametrize("d", [520, 4104])
def test_rmsnorm_honest_passes_and_eps_defects_fail(d):
    x, w = A.eps_rows(37, d, seed=1), (1 + 0.1 * rnd(d, seed=2).float()).to(BF)
    passes("y", rms32(x, w, 1e-5).to(BF), rms_val(x, w, 1e-5))
    assert "NaN" in fails("y", rms32(x, w, 0.0).to(BF), rms_val(x, w, 1e-5))        # the all-zero row
    keep = torch.ones(37, dtype=torch.bool)
    keep[1] = False
    val = rms_val(x[keep], w, 1e-5)
    fails("y", rms32(x[keep], w, 0.0).to(BF), val)                                    # the rows with mean(x^2) ~ eps
    fails("y", rms32(x[keep], w, 1e-3).to(BF), val)
    # ... and N(0,1) rows alone cannot see it: why the inputs matter as much as the bound
    xn = rnd(37, d, seed=3)
    passes("y", rms32(xn, w, 0.0).to(BF), rms_val(xn, w, 1e-5))


def ln32(x, w, b, eps):
    xf = x.float()
    mean = xf.sum(1, keepdim=True) / x.shape[1]
    rs = torch.rsqrt(((xf - mean) ** 2).sum(1, keepdim=True) / x.shape[1] + eps)
    return (xf - mean) * rs * w.float() + b.float()


def test_layernorm_honest_passes_and_missing_eps_fails():
    d = 520
    x, w, b = A.eps_rows(37, d, seed=1), (1 + 0.1 * rnd(d, seed=2).float()).to(BF), rnd(d, seed=6, scale=0.1)
    xv = Val(x)
    mean = xv.sum(1, keepdim=True) / float(d)
    xc = xv - mean
    rs = ((xc * xc).sum(1, keepdim=True) / float(d) + float(torch.tensor(1e-5, dtype=F32))).rsqrt()
    val = xc * rs * w.double()[None, :] + b.double()[None, :]
    passes("y", ln32(x, w, b, 1e-5).to(BF), val)
    assert "NaN" in fails("y", ln32(x, w, b, 0.0).to(BF), val)                       # the constant and the zero row
    # ... and without those two rows (a kernel that special-cases var = 0 but drops eps): the 2^-10-scaled rows, var ~ 1e-6
    keep = torch.ones(37, dtype=torch.bool)
    keep[1] = keep[2] = False
    kept = Val(val.v[keep], val.e[keep])
    passes("y", ln32(x[keep], w, b, 1e-5).to(BF), kept)
    assert "NaN" not in fails("y", ln32(x[keep], w, b, 0.0).to(BF), kept)
    assert "NaN" not in fails("y", ln32(x[keep], w, b, 1e-3).to(BF), kept)


# ------------------------------------------------------------------------------------------------------ AdamW
def test_adamw_honest_passes_and_eps_inside_sqrt_fails():
    n, lr, b1, b2, eps, step = 4096, 1e-4, 0.9, 0.999, 1e-8, 1
    gen = torch.Generator().manual_seed(1)
    g = (torch.sign(torch.randn(n, generator=gen)) * 10.0 ** (-12 + 3 * torch.rand(n, generator=gen))).to(BF)
    w0 = torch.randn(n, generator=gen) * 0.02
    f = lambda x: torch.tensor(x, dtype=F32)                                          # noqa: E731
    bc1, bc2s = 1 - f(b1) ** step, torch.sqrt(1 - f(b2) ** step)

    def step32(inside):
        m = (1 - f(b1)) * g.float()
        v = (1 - f(b2)) * g.float() * g.float()
        denom = torch.sqrt(v / (bc2s * bc2s) + f(eps)) if inside else torch.sqrt(v) / bc2s + f(eps)
        return w0 - (f(lr) / bc1) * (m / denom)
    f64s = lambda x: Val(torch.tensor(float(f(x)), dtype=F64))                        # noqa: E731
    gv = Val(g)
    mv = (1.0 - f64s(b1)) * gv
    vv = ((1.0 - f64s(b2)) * gv) * gv
    w = Val(w0) - (float(f(lr)) / (1.0 - f64s(b1))) * (mv / (vv.sqrt() / (1.0 - f64s(b2)).sqrt() + float(f(eps))))
    passes("master", step32(False), w, F32)
    fails("master", step32(True), w, F32)


# ------------------------------------------------------------------------------------------------------ attention
def attn_case(L, hd, seed=0, kvh=2, mask="causal"):
    """[(q, k, v, allowed)] for the four input rows of spiked_attention_rows; the last one also as a packed pair.  mask: "causal";
    "full" = every query sees every key (causal = 0), the packed window [40, 120) still hidden from the queries >= 120; "resampler" =
    the first 64 queries against all L keys (Lq = 64, Lk = L: the OmniLMM Resampler's live queries)"""
    q, k, v = A.spiked_attention_rows(2, L, 2, hd, seed=seed, kv_heads=kvh)
    Lq = 64 if mask == "resampler" else L
    allowed = A.causal_allowed if mask == "causal" else A.full_allowed
    out = [(q[s, h, :Lq], k[s, h * kvh // 2], v[s, h * kvh // 2], allowed(Lq, L)) for s in range(2) for h in range(2)]
    if L > 100 and mask != "resampler":
        out.append((q[0, 1], k[0, kvh - 1], v[0, kvh - 1], allowed(L, L, seg=(40, 120))))
    return out


def attn_masks(L, hd=128):
    """the masks an emulation test runs at this shape: the non-causal ones next to the causal one, the Resampler shape at L = 200"""
    return ("causal", "full") + (("resampler",) if (L, hd) == (200, 128) else ())


def test_full_allowed_is_the_documented_mask():
    """hidden(q, key) <=> key >= L || (CAUSAL && key > q) || (q >= e1 && sh <= key < e1), element by element, for both mask builders"""
    L, sh, e1 = 9, 2, 5
    for causal, fn in ((True, A.causal_allowed), (False, A.full_allowed)):
        for seg in (None, (sh, e1), (0, 0), (3, 3)):
            s0, s1 = seg or (0, 0)
            want = torch.tensor([[not ((causal and key > q) or (q >= s1 and s0 <= key < s1)) for key in range(L)] for q in range(L)])
            assert torch.equal(fn(L, L, seg=seg), want), (causal, seg)
    assert torch.equal(A.full_allowed(4, L, seg=(sh, e1)), A.full_allowed(L, L, seg=(sh, e1))[:4])        # Lq != Lk: the first Lq queries
    assert bool(A.full_allowed(64, 200).all()) and A.full_allowed(64, 200).shape == (64, 200)


@pytest.mark.parametrize("kvh", [2, 1])
@pytest.mark.parametrize("L,hd", [(65, 128), (200, 128), (65, 64), (200, 64)])
def test_attention_builder_delivers_its_row_kinds(L, hd, kvh):
    """spiked_attention_rows: the late key, the early key that dominates (nearly) every query of its head, the uniform first quarter and
    the nearly one-hot scale-3 rows exist, for kv_heads = 2 and for the one shared kv head of kv_group 2"""
    q, k, v = A.spiked_attention_rows(2, L, 2, hd, kv_heads=kvh)
    ok = A.causal_allowed(L, L)

    def probs(s, h):
        sc = (q[s, h].double() @ k[s, h * kvh // 2].double().t()) / math.sqrt(hd)
        return torch.softmax(sc.masked_fill(~ok, -math.inf), -1), q[s, h].double() @ k[s, h * kvh // 2].double().t()
    P, _ = probs(0, 0)
    assert P[-1, -1] > 0.95 and (P[:-1].max(-1).values.median() < 0.2)               # late: only the last query, in the last tile
    P, _ = probs(0, 1)
    assert (P[:, 0] > 0.5).double().mean() > 0.95 and P[L - 1, 0] > 0.5               # early: key 0 for queries many tiles later
    plain, _ = probs(1, 0)
    assert (plain[:, 0] > 0.5).sum() <= 3                                             # ... which an ordinary head does not have
    quarter = max(1, L // 4)
    for h in range(2 if kvh == 1 else 1):                                             # the query heads that read kv head 0
        P, _ = probs(1, h)
        i = torch.arange(quarter)
        want = 1.0 / (i + 1.0)
        assert torch.allclose(P[:quarter, :quarter].max(-1).values, want.double(), rtol=1e-9)   # uniform over the keys a query sees
    P, raw = probs(1, 1)
    assert P[quarter:].max(-1).values.median() > 0.6 and raw.abs().max() > 100       # nearly one-hot, raw scores past +-100


@pytest.mark.parametrize("kvh", [2, 1])
@pytest.mark.parametrize("online", [True, False])
@pytest.mark.parametrize("L,hd", [(1, 128), (65, 128), (200, 128), (65, 64), (200, 64)])
def test_attention_forward_emulation_within_bound(L, hd, online, kvh):
    scale = 1.0 / math.sqrt(hd)
    for mask in attn_masks(L, hd):
        outs, docs, lses, got_o, got_l = [], [], [], [], []
        for q, k, v, ok in attn_case(L, hd, kvh=kvh, mask=mask):     # one check per output tensor: the row kinds are rows of one case
            out, doc, lse = A.attn_fwd_bound(q, k, v, ok, scale)
            o, l = A.emulate_attn_fwd(q, k, v, ok, scale, online=online)
            outs.append(out), docs.append(doc), lses.append(lse), got_o.append(o), got_l.append(l)
        assert passes(f"out ({mask})", torch.cat(got_o), cat_vals(outs), BF, doc=torch.cat(docs))["ratio"] <= 1.0
        assert passes(f"lse ({mask})", torch.cat(got_l), cat_vals(lses), F32)["ratio"] <= 1.0


def cat_vals(vals):
    return Val(torch.cat([x.v for x in vals]), torch.cat([x.e for x in vals]))


def full_mask_bound(hd, kvh, L=200):
    """(cases, out Val, doc, lse Val) of the all-true mask (with its packed-window case) at L = 200: what a defective emulation is held to"""
    scale = 1.0 / math.sqrt(hd)
    cases = attn_case(L, hd, kvh=kvh, mask="full")
    b = [A.attn_fwd_bound(q, k, v, ok, scale) for q, k, v, ok in cases]
    return cases, cat_vals([x[0] for x in b]), torch.cat([x[1] for x in b]), cat_vals([x[2] for x in b])


@pytest.mark.parametrize("kvh", [2, 1])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("defect", ["tail-keys-dropped", "causal-mask-applied", "final-rescale-skipped"])
def test_attention_noncausal_defects_fail(defect, hd, kvh):
    """what the non-causal GPU cases must be able to see, at L = 200 (three full key tiles and a ragged one of 8 keys): an emulation
    that leaves out the keys of the last partial tile (k >= 64 * (Lk // 64)), one that applies the causal mask when the full one was
    asked for, and one whose last tile moves the running maximum without rescaling o and l.  The honest emulation passes the same
    bound (test_attention_forward_emulation_within_bound)"""
    L = 200
    scale = 1.0 / math.sqrt(hd)
    cases, out, doc, lse = full_mask_bound(hd, kvh, L)
    got_o, got_l = [], []
    for q, k, v, ok in cases:
        if defect == "tail-keys-dropped":
            o, l = A.emulate_attn_fwd(q, k, v, ok & (torch.arange(L)[None, :] < 64 * (L // 64)), scale)
        elif defect == "causal-mask-applied":
            o, l = A.emulate_attn_fwd(q, k, v, ok & A.causal_allowed(L, L), scale)
        else:
            o, l = A.emulate_attn_fwd(q, k, v, ok, scale, rescale_last=False)
        got_o.append(o), got_l.append(l)
    fails("out", torch.cat(got_o), out, BF, doc=doc)
    fails("lse", torch.cat(got_l), lse, F32)


def test_attention_denominator_from_rounded_p_fails():
    """the row sum taken AFTER P is rounded to bf16: `out` hides it (numerator and denominator share the rounding), lse does not"""
    L, hd = 200, 128
    scale = 1.0 / math.sqrt(hd)
    q, k, v, ok = attn_case(L, hd)[0]
    _, _, lse = A.attn_fwd_bound(q, k, v, ok, scale)
    S = torch.where(ok, (q.float() @ k.float().t()) * scale, torch.tensor(-math.inf))
    m = S.max(-1, keepdim=True).values
    p = torch.exp(S - m)
    passes("lse", (m + torch.log(p.sum(-1, keepdim=True)))[:, 0], lse, F32)
    fails("lse", (m + torch.log(p.to(BF).float().sum(-1, keepdim=True)))[:, 0], lse, F32)


@pytest.mark.parametrize("kvh", [2, 1])
@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("L", [1, 65, 200])
def test_attention_backward_emulation_within_bound(L, rope, kvh):
    hd = 128
    fr = (torch.arange(L, dtype=F32)[:, None] * 37 + 5) / (10000.0 ** (torch.arange(0, hd, 2, dtype=F32) / hd))[None, :]
    scale = 1.0 / math.sqrt(hd)
    for mask in attn_masks(L):
        acc = {n: ([], [], [], []) for n in ("dQ", "dK", "dV")}
        for i, (q, k, v, ok) in enumerate(attn_case(L, hd, seed=1, kvh=kvh, mask=mask)):
            Lq = q.shape[0]
            O, lse = A.emulate_attn_fwd(q, k, v, ok, scale)
            dO = rnd(Lq, hd, seed=5 + i, scale=0.5)
            res = A.attn_bwd_bound(q, k, v, dO, O, lse, ok, scale)
            for name, got in zip(("dQ", "dK", "dV"), A.emulate_attn_bwd(q, k, v, dO, O, lse, ok, scale)):
                val, doc = res[name]
                if rope and name != "dV":                  # the fused inverse RoPE: round to bf16, rotate in fp32, round at the store
                    n = got.shape[0]
                    cos, sin = fr[:n].cos(), fr[:n].sin()
                    a, b = got.float()[:, :64], got.float()[:, 64:]
                    got = torch.cat([a * cos + b * sin, b * cos - a * sin], 1).to(BF)
                    val, doc = A.rope_bwd_val(val, doc, cos.double(), sin.double())
                for lst, x in zip(acc[name], (got, val.v, val.e, doc)):
                    lst.append(x)
        for name, (got, v, e, doc) in acc.items():
            assert passes(f"{name} ({mask})", torch.cat(got), Val(torch.cat(v), torch.cat(e)), BF, doc=torch.cat(doc),
                          cap_unit="ulp+doc")["ratio"] <= 1.0


# ------------------------------------------------------------------------------------------------------ the GPU cases' layouts
def _emulated_layout(layout, hd, G, seed):
    """tests/test_accuracy_gpu.py's layout with the CPU emulation standing in for the kernels: (c, qkv parts, out, lse) as
    rv_attn_fwd leaves them, the dead query rows of a Resampler layout included (zero q: a uniform softmax over all keys)"""
    import test_accuracy_gpu as T
    c = T.ATTN_LAYOUTS[layout]
    L, H, scale = c["L"], 2, 1.0 / math.sqrt(hd)
    qkv, q, k, v, starts, lens = T._attn_layout("cpu", L, hd, G, c.get("lens"), seed=seed, nq=c.get("nq"))
    out, lse = torch.zeros(qkv.shape[0], H * hd, dtype=BF), torch.zeros(2, H, L)
    masks = []
    for s_ in range(2):
        n, a = lens[s_], starts[s_]
        masks.append(T._allowed(c, s_, n, "cpu"))                  # the kernel's view: all n queries of the row
        for h in range(H):
            o, l = A.emulate_attn_fwd(qkv[a:a + n, h * hd:(h + 1) * hd], k[s_, h // G, :n], v[s_, h // G, :n], masks[s_], scale)
            out[a:a + n, h * hd:(h + 1) * hd], lse[s_, h, :n] = o, l
    return T, c, (qkv, q, k, v, starts, lens), masks, out, lse


def _full_cases():
    import test_accuracy_gpu as T
    return sorted({(kw["layout"], kw["hd"], kw["G"]) for _, kw in T.full_layout_cases(hd=[64, 128], G=[1, 2])})


@pytest.mark.parametrize("layout,hd,G", _full_cases())
def test_noncausal_gpu_layouts_pass_through_the_emulation(layout, hd, G):
    """every non-causal layout of tests/test_accuracy_gpu.py at every head dim / kv_group it is admitted at, through the GPU cases' own
    checkers with the CPU emulation in the kernels' place: inside the bound and under the discrimination cap (a layout over the cap
    raises CapError here, before it costs a GPU run); the figures are printed.  Backward at head dim 128, as on the GPU."""
    T, c, (qkv, q, k, v, starts, lens), masks, out, lse = _emulated_layout(layout, hd, G, seed=0)
    what = f"emulated rv_attn_fwd (hd {hd}, kv_group {G}, {layout})"
    for e in T._check_attn_fwd(c, "cpu", hd, G, out, lse, q, k, v, starts, lens, what):
        assert e["ratio"] <= 1.0 and e["median_E_ulps"] <= A.CAP
    if hd != 128:
        return
    T, c, (qkv, q, k, v, starts, lens), masks, out, lse = _emulated_layout(layout, hd, G, seed=1)
    H, Hkv, scale = 2, 2 // G, 1.0 / math.sqrt(hd)
    dO = T._attn_bwd_dO(c, "cpu", qkv.shape[0], starts, lens)
    dqkv = torch.zeros_like(qkv)
    for s_ in range(2):
        n, a = lens[s_], starts[s_]
        dk = torch.zeros(Hkv, n, hd)
        dv = torch.zeros(Hkv, n, hd)
        for h in range(H):
            cols = slice(h * hd, (h + 1) * hd)
            # the kernels accumulate the group's query heads in fp32 and round once: emulate_attn_bwd rounds per head, so its parts are
            # recomputed here in fp32 from the same formula (dS and P rounded to bf16 for their MFMAs)
            dq_, dk_, dv_ = _emulate_bwd_f32(qkv[a:a + n, cols], k[s_, h // G, :n], v[s_, h // G, :n], dO[a:a + n, cols], out[a:a + n, cols],
                                             lse[s_, h, :n], masks[s_], scale)
            dqkv[a:a + n, cols] = dq_.to(BF)
            dk[h // G] += dk_
            dv[h // G] += dv_
        dqkv[a:a + n, H * hd:(H + Hkv) * hd] = dk.transpose(0, 1).reshape(n, Hkv * hd).to(BF)
        dqkv[a:a + n, (H + Hkv) * hd:] = dv.transpose(0, 1).reshape(n, Hkv * hd).to(BF)
    res = T._check_attn_bwd(c, "cpu", G, dqkv, dO, out, lse, q, k, v, starts, lens, f"emulated rv_attn_bwd (kv_group {G}, {layout})")
    for e in res.values():
        assert e["ratio"] <= 1.0 and e["median_E_ulps"] <= A.CAP


def _emulate_bwd_f32(q, k, v, dO, O, lse, allowed, scale):
    """accuracy.emulate_attn_bwd before its store: (dQ, dK, dV) in fp32"""
    LOG2E = torch.tensor(1.4426950408889634, dtype=F32)
    qf, kf, vf, dof = q.float(), k.float(), v.float(), dO.float()
    c = torch.tensor(scale, dtype=F32) * LOG2E
    S = torch.where(allowed, qf @ kf.t(), torch.tensor(-math.inf))
    P = torch.exp2(S * c - (lse.float() * LOG2E)[:, None])
    dS = P * (dof @ vf.t() - (dof * O.float()).sum(-1, keepdim=True))
    sc = torch.tensor(scale, dtype=F32)
    return (dS.to(BF).float() @ kf) * sc, (dS.to(BF).float().t() @ qf) * sc, P.to(BF).float().t() @ dof


# ------------------------------------------------------------------------------------------------------ LM head
def test_lmhead_emulation_within_bound_and_defects_fail():
    h, w, tgt = A.lmhead_inputs()
    logp, lse, x, _ = A.lmhead_bound(h, w, tgt, 121)
    assert 30 < x[:, :121].abs().max() < 80
    ok = tgt >= 0
    assert logp.v[:10].min() > -1e-4 and logp.v[10:20].max() < -25                    # the argmax rows and the deep tail
    got_p, got_l = A.emulate_lmhead(h, w, tgt, 121)
    assert passes("lse", got_l, lse, F32)["ratio"] <= 1.0
    assert passes("logp", got_p[ok], logp[ok], F32)["ratio"] <= 1.0
    # the padding columns counted into the softmax; logits rounded to bf16 before the softmax
    bad_l = torch.logsumexp(h.float() @ w.float().t(), -1)
    fails("lse", bad_l, lse, F32)
    xb = (h.float() @ w.float().t()).to(BF).float()[:, :121]
    fails("lse", torch.logsumexp(xb, -1), lse, F32)
    # backward: dlogits with the forward's lse; p -> 1 at the argmax rows
    coef = rnd(70, seed=9, dtype=F32) * 0.1
    val = A.lmhead_bwd_bound(h, w, tgt, got_l, coef, 121)
    xf = h.float() @ w.float().t()
    onehot = (torch.arange(128)[None, :] == tgt.long()[:, None]).float()
    d32 = coef[:, None] * (onehot - torch.exp(xf - got_l[:, None]))
    d32[:, 121:] = 0.0
    assert passes("dlogits", d32.to(BF), val)["ratio"] <= 1.0
    fails("dlogits", trunc_bf16(d32), val)
