"""Per-element accuracy of every kernel output against float64 (tests/accuracy.py): table-driven like test_containment_gpu.py.

Each case computes ref64 - the header's formula in float64 on the same bf16-rounded or fp32 inputs - and E, the error the kernel's
documented arithmetic may have before its one round-to-nearest-even store, and asserts |got - ref64| <= 0.5 ulp_out(|ref64| + E) + E
element by element.  E is written with accuracy.Val objects: the kernel's formula line by line, every operation adding its own
term, so the derivation of a bound IS the code next to the case; terms that are not plain fp32 roundings are named in a comment with
the kernel line that justifies them.  Inputs are chosen so that the stabilising terms of the formulas matter (eps-dominated norm rows,
saturated logistic losses, gradients far below AdamW's eps, every finite bf16 pattern for the unary kernels).

    python -m pytest tests/test_accuracy_gpu.py -m gpu -q"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy as A  # noqa: E402
from accuracy import Val, U32  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def call(name, *args):
    from rlaif_v_amd import hip
    hip.call(name, *args)


def rnd(*shape, scale=1.0, seed=0, dev=None, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)


def f32r(x: float) -> float:
    """a python float as the ABI receives it (float argument)"""
    return float(torch.tensor(x, dtype=F32))


CASES = []


def case(*ids_kwargs):
    def deco(fn):
        for cid, kw in ids_kwargs:
            CASES.append(pytest.param(fn, kw, id=f"{fn.__name__[2:]}[{cid}]" if cid else fn.__name__[2:]))
        return fn
    return deco


def grid(**axes):
    import itertools
    keys = list(axes)
    out = []
    for vals in itertools.product(*[axes[k] for k in keys]):
        kw = dict(zip(keys, vals))
        out.append(("-".join(f"{k}={'x'.join(map(str, v)) if isinstance(v, tuple) else v}" for k, v in kw.items()), kw))
    return out


def _restore_knobs():
    call("rv_set_gemm_mi16", 1)
    call("rv_set_gemm_variant", -1)
    call("rv_set_attn_dkv_version", 0)
    call("rv_set_attn_fwd_version", 0)


def run_case(fn, **kw):
    dev = _dev()
    try:
        fn(dev, **kw)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):      # a faulted device: start nothing more on it
            pytest.exit(f"GPU fault in {fn.__name__} {kw}: {e}", returncode=3)
        raise
    finally:
        _restore_knobs()


def chk(got, val: Val, what, out_dtype=None, doc=None):
    return A.check(got, val.v, val.e, out_dtype or got.dtype, what, doc=doc)


def chk_doc(got, formula, what):
    """a formula with documented bf16 operand roundings (Val.bf16): their share of E stays out of the discrimination cap"""
    val = formula()
    with A.no_doc():
        plain = formula()
    return chk(got, val, what, doc=val.e - plain.e)


# =========================================================================================== dense GEMMs
def _act(z: Val, act: int) -> Val:
    """the epilogue's activation on the fp32 pre-activation (gemm.hpp EpiStore::apply_wide): 1 = z / (1 + __expf(-1.702f z)),
    2 = 0.5f z (1 + erff(z * 0.70710678f))"""
    if act == 1:
        return z / (1.0 + (-(Val.const(1.702) * z)).exp())
    if act == 2:
        return A.gelu(z)
    return z


def _epilogue(acc: Val, bias=None, res=None, act=0) -> Val:
    """act(alpha * acc + bias[n]) + residual[m][n] in the order of EpiStore: every operand exact, every step one fp32 rounding"""
    z = acc if bias is None else acc + bias.double()[None, :]
    y = _act(z, act)
    return y if res is None else y + res.double()


def _gemm_inputs(kind, dev, M, N, K):
    """(a [M][K], b [N][K], bias, residual, alpha, acts)"""
    if kind == "ragged":                              # N(0,1): the plain accumulation bound, edge tiles on both axes
        return rnd(M, K, seed=1, dev=dev), rnd(N, K, seed=2, dev=dev), None, None, 1.0, (0,)
    if kind == "epilogue":                            # K = 64, pre-activation alpha a.b + bias of standard deviation ~2.2: spans [-6, 6]
        return (rnd(M, K, seed=3, dev=dev, scale=0.7071), rnd(N, K, seed=4, dev=dev, scale=0.7071), rnd(N, seed=5, dev=dev),
                rnd(M, N, seed=6, dev=dev), 0.5, (0, 1, 2))
    a, b = A.cancelling_gemm(M, N, K, seed=7, device=dev)
    return a, b, None, None, 1.0, (0,)


GEMM_SHAPES = {"ragged": [(200, 132, 192), (7, 4, 64)], "epilogue": [(130, 136, 64)], "cancelling": [(130, 136, 256)]}


@case(*grid(variant=[0, 1, 2, 3], mi16=[1, 0], kind=["ragged", "epilogue", "cancelling"]))
def c_gemm_nt(dev, variant, mi16, kind):
    call("rv_set_gemm_mi16", mi16)
    for M, N, K in GEMM_SHAPES[kind]:
        a, b, bias, res, alpha, acts = _gemm_inputs(kind, dev, M, N, K)
        acc = A.matmul(a, b.t(), alpha)
        for act in acts:
            c = torch.empty(M, N, dtype=BF, device=dev)
            call("rv_gemm_nt_bf16", a, K, b, K, c, N, M, N, K, bias, res, N if res is not None else 0, act, alpha, variant)
            chk(c, _epilogue(acc, bias, res, act), f"rv_gemm_nt_bf16 C ({kind} {M}x{N}x{K} act={act} variant={variant} mi16={mi16})")


@case(*grid(entry=["f32out", "f32res"], variant=[-1, 0, 1, 2], kind=["ragged", "cancelling"]))
def c_gemm_nt_f32(dev, entry, variant, kind):
    for M, N, K in GEMM_SHAPES[kind]:
        a, b, _, _, _, _ = _gemm_inputs(kind, dev, M, N, K)
        acc = A.matmul(a, b.t())
        if entry == "f32out":
            c = torch.empty(M, N, dtype=F32, device=dev)
            call("rv_gemm_nt_bf16_f32out", a, K, b, K, c, N, M, N, K, variant)
            chk(c, acc, f"rv_gemm_nt_bf16_f32out C ({kind} {M}x{N}x{K} variant={variant})")
            continue
        bias, res = rnd(N, seed=8, dev=dev), rnd(M, N, seed=9, dev=dev, dtype=F32) * 3.0
        c = res.clone()                                   # C aliases the fp32 residual stream, as ops.gemm_nt_f32res calls it
        call("rv_gemm_nt_bf16_f32res", a, K, b, K, c, N, M, N, K, bias, c, N, variant)
        chk(c, _epilogue(acc, bias, res), f"rv_gemm_nt_bf16_f32res C ({kind} {M}x{N}x{K} variant={variant})")


NN_SHAPES = {"ragged": [(200, 136, 192), (7, 8, 64)], "epilogue": [(130, 136, 64)], "cancelling": [(130, 136, 256)]}


@case(*grid(mi16=[1, 0], kind=["ragged", "epilogue", "cancelling"]))
def c_gemm_nn(dev, mi16, kind):
    """rv_gemm_nn_bf16 (residual + alpha) and rv_gemm_nn_bias_act_bf16 (the NT epilogue); N % 8 == 0 for the NN forms"""
    call("rv_set_gemm_mi16", mi16)
    for M, N, K in NN_SHAPES[kind]:
        a, b, bias, res, alpha, acts = _gemm_inputs(kind, dev, M, N, K)
        bt = b.t().contiguous()                           # [K][N]
        acc = A.matmul(a, bt, alpha)
        c = torch.empty(M, N, dtype=BF, device=dev)
        call("rv_gemm_nn_bf16", a, K, bt, N, c, N, M, N, K, res, N if res is not None else 0, alpha)
        chk(c, _epilogue(acc, None, res), f"rv_gemm_nn_bf16 C ({kind} {M}x{N}x{K} mi16={mi16})")
        if kind == "epilogue":
            for act in acts:
                call("rv_gemm_nn_bias_act_bf16", a, K, bt, N, c, N, M, N, K, bias, res, N, act, alpha)
                chk(c, _epilogue(acc, bias, res, act), f"rv_gemm_nn_bias_act_bf16 C ({M}x{N}x{K} act={act} mi16={mi16})")


@case(*grid(mi16=[1, 0], kind=["ragged", "epilogue", "cancelling"]))
def c_gemm_tn(dev, mi16, kind):
    """C[i][j] = alpha sum_r P[r][i] Q[r][j] + residual: ragged R (the zero-row redirect), I, J; the split-K form at 3 chunks"""
    call("rv_set_gemm_mi16", mi16)
    shapes = {"ragged": [(190, 200, 136), (7, 8, 8)], "epilogue": [(64, 136, 128)], "cancelling": [(256, 136, 128)]}[kind]
    for R, I, J in shapes:
        q = rnd(R, J, seed=11, dev=dev)
        if kind == "cancelling":
            pa, qb = A.cancelling_gemm(I, J, R, seed=12, device=dev)
            p, q = pa.t().contiguous(), qb.t().contiguous()
        else:
            p = rnd(R, I, seed=10, dev=dev)
        res, alpha = (rnd(I, J, seed=13, dev=dev), 0.5) if kind == "epilogue" else (None, 1.0)
        acc = A.matmul(p.t(), q, alpha)
        c = torch.empty(I, J, dtype=BF, device=dev)
        call("rv_gemm_tn_bf16", p, I, q, J, c, J, R, I, J, res, J if res is not None else 0, alpha)
        chk(c, _epilogue(acc, None, res), f"rv_gemm_tn_bf16 C ({kind} {R}x{I}x{J} mi16={mi16})")
        if kind != "epilogue" and R >= 190:
            # splits fp32 slabs summed in a fixed order, then * alpha: (splits - 1) more additions, inside "any order" of gemm_E
            splits = 3
            ws = torch.empty(splits * I * J, dtype=F32, device=dev)
            call("rv_gemm_tn_bf16_splitk", p, I, q, J, c, J, R, I, J, 0.25, splits, ws)
            chk(c, A.matmul(p.t(), q, 0.25), f"rv_gemm_tn_bf16_splitk C ({kind} {R}x{I}x{J} mi16={mi16})")


# =========================================================================================== exhaustive unary kernels
def _all_bf16(dev):
    return A.all_finite_bf16(dev)                         # 65,280 = 255 rows x 256 columns


@case(("", {}))
def c_gelu(dev):
    from rlaif_v_amd import ops
    x = _all_bf16(dev)
    chk(ops.gelu_fwd(x), A.gelu(x), "rv_gelu_fwd y")
    for dyv in (1.0, -0.37):
        dy = torch.full_like(x, dyv)
        xv = Val(x)
        # elementwise.hip gelu_bwd_kernel: cdf = 0.5f (1 + erff(x c)); pdf = 0.39894228f __expf(-0.5f x x); dx = dy (cdf + x pdf)
        cdf = Val.const(0.5) * (1.0 + (xv * Val.const(math.sqrt(0.5))).erf())
        pdf = Val.const(0.3989422804014327) * ((Val.const(-0.5) * xv) * xv).exp()
        dx = Val(dy) * (cdf + xv * pdf)
        # the value from erfc: 1 + erf cancels in float64 as well for x << 0
        xd = x.double()
        ref = dy.double() * (0.5 * torch.special.erfc(-xd * math.sqrt(0.5)) + xd * torch.exp(-0.5 * xd * xd) / math.sqrt(2 * math.pi))
        chk(ops.gelu_bwd(dy, x), Val(ref, dx.e), f"rv_gelu_bwd dx (dy = {dyv})")


def _swiglu_gu(dev, upv, interleaved):
    g = _all_bf16(dev).view(255, 256)
    u = torch.full_like(g, upv)
    gu = torch.stack([g, u], dim=2).reshape(255, 512) if interleaved else torch.cat([g, u], dim=1)
    return g, u, gu.contiguous()


@case(*grid(interleaved=[0, 1], up=[1.0, -3.0, 2.0 ** -20]))
def c_swiglu(dev, interleaved, up):
    from rlaif_v_amd import ops
    g, u, gu = _swiglu_gu(dev, up, interleaved)
    gv, ud = Val(g), u.double()
    # swiglu_fwd_kernel: o = g / (1.f + __expf(-g)) * u.  For g < -88.72 exp(-g) passes the fp32 range and the quotient is 0: Val's
    # division takes the whole (tiny) value as the error there
    act = gv / (1.0 + (-gv).exp()) * ud
    chk(ops.swiglu_fwd(gu, interleaved=bool(interleaved)), act, f"rv_swiglu_fwd act (up = {up}, interleaved = {interleaved})")
    # swiglu_bwd_kernel: sg = 1.f / (1.f + __expf(-g)); dg = da u sg (1.f + g (1.f - sg)); du = da (g sg)
    da = torch.full_like(g, -0.37)
    sg = 1.0 / (1.0 + (-gv).exp())
    dg = Val(da) * ud * sg * (1.0 + gv * (1.0 - sg))
    du = Val(da) * (gv * sg)
    # 1 - sg and g (1 - sg) cancel in float64 too for large g: the values from the closed forms sigmoid(-g), g sigmoid(-g)
    gd, s64 = g.double(), torch.sigmoid(g.double())
    dg = Val(da.double() * ud * s64 * (1.0 + gd * torch.sigmoid(-gd)), dg.e)
    dgu = ops.swiglu_bwd(da, gu, interleaved=bool(interleaved))
    got_dg, got_du = (dgu[:, 0::2], dgu[:, 1::2]) if interleaved else (dgu[:, :256], dgu[:, 256:])
    chk(got_dg, dg, f"rv_swiglu_bwd d gate (up = {up}, interleaved = {interleaved})")
    chk(got_du, du, f"rv_swiglu_bwd d up (up = {up}, interleaved = {interleaved})")


def _dropout_ref(x, p, seed):
    """(mask, Val of the kept values): rv_dropout multiplies by inv_keep = 1.f / (1.f - p), computed in fp32 on the host
    (elementwise.hip rv_dropout): two roundings in inv_keep, one in the product"""
    from rlaif_v_amd import ops
    mask = ops.dropout(torch.ones_like(x), p, seed) != 0
    inv = 1.0 / (1.0 - Val(torch.tensor(f32r(p), dtype=F64, device=x.device)))
    return mask, Val(x) * inv


@case(*grid(up=[1.0, -3.0, 2.0 ** -20]))
def c_swiglu_dropout(dev, up):
    """rv_swiglu_fwd_dropout: act as rv_swiglu_fwd; actd = rv_dropout(act) - a documented second rounding, checked on the act
    the kernel stored (its bf16 values are the exact operand of the dropout)"""
    from rlaif_v_amd import ops
    g, u, gu = _swiglu_gu(dev, up, 0)
    gv = Val(g)
    act, actd = ops.swiglu_fwd_dropout(gu, 0.3, 77)
    chk(act, gv / (1.0 + (-gv).exp()) * u.double(), f"rv_swiglu_fwd_dropout act (up = {up})")
    fin = torch.isfinite(act)                           # up = -3 overflows at the largest gates: act = -inf there, and so is actd where kept
    mask, kept = _dropout_ref(torch.where(fin, act, torch.zeros_like(act)), 0.3, 77)
    chk(torch.where(fin, actd, torch.zeros_like(actd)), A.where(mask, kept, Val(torch.zeros_like(kept.v))),
        f"rv_swiglu_fwd_dropout actd (up = {up})")
    assert bool((actd[~fin] == torch.where(mask, act, torch.zeros_like(act))[~fin]).all()), "rv_swiglu_fwd_dropout actd: overflowed elements"


@case(*grid(p=[0.05, 0.3]))
def c_dropout(dev, p):
    from rlaif_v_amd import ops
    x = _all_bf16(dev)
    mask, kept = _dropout_ref(x, p, 4711)
    y = ops.dropout(x, p, 4711)
    chk(y, A.where(mask, kept, Val(torch.zeros_like(kept.v))), f"rv_dropout y (p = {p})")
    assert bool((y[~mask] == 0).all())
    drop = 1.0 - mask.double().mean().item()
    assert abs(drop - p) <= 4 * math.sqrt(p * (1 - p) / x.numel()) + 2.0 ** -16, f"rv_dropout: {drop:.4f} of the elements dropped at p = {p}"
    acc0 = rnd(x.numel(), seed=3, dev=dev)
    acc = acc0.clone()
    ops.dropout(x, p, 4711, out=None, accumulate_into=acc)
    # dropout_kernel: acc += f with the UNROUNDED fp32 product f = x inv_keep: one more fp32 addition, one store
    chk(acc, A.where(mask, kept, Val(torch.zeros_like(kept.v))) + acc0.double(), f"rv_dropout acc (p = {p})")


@case(("", {}))
def c_cast(dev):
    from rlaif_v_amd import ops
    x = _all_bf16(dev)
    A.check_bits(ops.cast_bf16_to_f32(x), x.view(torch.int16).to(torch.int32).bitwise_left_shift(16).view(F32), "rv_cast_bf16_to_f32 out")
    xin, want = A.bf16_midpoints(dev)
    got = ops.cast_f32_to_bf16(xin).view(torch.int16).to(torch.int32) & 0xFFFF
    bad = got != want
    assert not bool(bad.any()), (f"rv_cast_f32_to_bf16 out: {int(bad.sum())} of {want.numel()} midpoint inputs rounded wrongly, first input "
                                 f"bits {xin.view(torch.int32)[bad][0].item() & 0xFFFFFFFF:#010x}: want {want[bad][0].item():#06x}, got "
                                 f"{got[bad][0].item():#06x}")


@case(("", {}))
def c_add_f32_bf16(dev):
    from rlaif_v_amd import ops
    b = _all_bf16(dev)
    for scale in (1.0, 2.0 ** -30, 2.0 ** 40):
        x = rnd(b.numel(), seed=5, dev=dev, dtype=F32) * scale
        chk(ops.add_f32_bf16(x, b), Val(x) + b.double(), f"rv_add_f32_bf16 out (x scale {scale:g})")


@case(("", {}))
def c_grad_accum(dev):
    """mode 2: g = bf16((acc + g) * scale), scale = 1 / 3 as the ABI's float; modes 0 / 1 are exact copies / one fp32 addition"""
    from rlaif_v_amd import ops
    g0 = _all_bf16(dev)
    acc = torch.empty(g0.numel(), dtype=F32, device=dev)
    g = g0.clone()
    ops.grad_accum(acc, g, 0)
    A.check_bits(acc, g0.float(), "rv_grad_accum mode 0 acc")
    g1 = rnd(g0.numel(), seed=6, dev=dev)
    ops.grad_accum(acc, g1.clone(), 1)
    chk(acc, Val(g0) + g1.double(), "rv_grad_accum mode 1 acc")
    acc_in = acc.clone()
    g2 = rnd(g0.numel(), seed=7, dev=dev)
    g = g2.clone()
    ops.grad_accum(acc, g, 2, 1.0 / 3.0)
    chk(g, (Val(acc_in) + g2.double()) * f32r(1.0 / 3.0), "rv_grad_accum mode 2 g")


# =========================================================================================== norms
NORM_GRID = dict(d=[520, 4104], eps=[1e-5, 1e-6])
ROWS = 37


def _depth(d: int) -> int:
    """additions on the longest path of a row reduction of the norm kernels (elementwise.hip: 8 elements per thread and 2048-column
    pass, then common.hpp block_sum: 6 wave_sum steps and a serial sum over the 4 waves' partials)"""
    return 8 * ((d + 2047) // 2048) + 6 + 4


def _rms(x: Val, d: int, eps: float):
    """rmsnorm_fwd_kernel: ss = sum x x (any order); rs = rsqrtf(ss / d + eps)"""
    return ((x * x).sum(1, keepdim=True, depth=_depth(d)) / float(d) + f32r(eps)).rsqrt()


def _norm_w(d, dev, seed=2):
    return (1 + 0.1 * rnd(d, seed=seed, dev=dev).float()).to(BF)


def _check_zero_row(y, what):
    assert bool((y[1].float() == 0).all()), f"{what}: the all-zero row must give y = 0"


@case(*grid(kind=["bf16", "dropout", "f32", "f32add"], **NORM_GRID))
def c_rmsnorm_fwd(dev, kind, d, eps):
    from rlaif_v_amd import ops
    w = _norm_w(d, dev)
    what = f"({kind}, d = {d}, eps = {eps})"
    if kind in ("bf16", "dropout"):
        x = A.eps_rows(ROWS, d, seed=1, device=dev)
        xv = Val(x)
        if kind == "bf16":
            y, rstd = ops.rmsnorm_fwd(x, w, eps)
            name = "rv_rmsnorm_fwd"
        else:
            y, rstd, yd = ops.rmsnorm_fwd_dropout(x, w, eps, 0.3, 99)
            name = "rv_rmsnorm_fwd_dropout"
            # yd = rv_dropout(y), bit for bit (the header's contract): the second rounding is rv_dropout's, checked in c_dropout
            A.check_bits(yd, ops.dropout(y.contiguous(), 0.3, 99), f"{name} yd {what}")
    else:
        x = A.eps_rows(ROWS, d, seed=1, device=dev, dtype=F32) * (1 + 2.0 ** -12)       # genuinely fp32 values
        name = "rv_rmsnorm_fwd_f32"
        if kind == "f32":
            xv = Val(x)
            y, rstd = ops.rmsnorm_fwd(x, w, eps)
        else:
            add = A.eps_rows(ROWS, d, seed=3, device=dev)                                # the same small / zero / constant rows
            xout, y, rstd = ops.add_rmsnorm_fwd(x, add, w, eps)
            xv = Val(x) + add.double()                                                   # xout = x + add: one fp32 addition
            chk(xout, xv, f"{name} xout {what}")
    rs = _rms(xv, d, eps)
    chk(rstd, rs[:, 0], f"{name} rstd {what}")
    chk(y, xv * rs * w.double()[None, :], f"{name} y {what}")
    _check_zero_row(y, f"{name} y {what}")


@case(*grid(f32x=[False, True], **NORM_GRID))
def c_rmsnorm_bwd(dev, f32x, d, eps):
    """rmsnorm_bwd_kernel on the rstd the forward kernel stored (an exact fp32 input of this call): xh = x rs; dot = sum(dy w xh) / d;
    dx = rs (dy w - x rs dot) + dres; dw[c] = sum_r dy xh over fp32 partials in any order"""
    from rlaif_v_amd import ops
    name = "rv_rmsnorm_bwd_f32x" if f32x else "rv_rmsnorm_bwd"
    what = f"(d = {d}, eps = {eps})"
    x = A.eps_rows(ROWS, d, seed=1, device=dev, dtype=F32) * (1 + 2.0 ** -12) if f32x else A.eps_rows(ROWS, d, seed=1, device=dev)
    w, dy, dres = _norm_w(d, dev), rnd(ROWS, d, seed=4, dev=dev), rnd(ROWS, d, seed=5, dev=dev)
    _, rstd = ops.rmsnorm_fwd(x, w, eps)
    dw = torch.zeros(d, dtype=BF, device=dev)
    dx = ops.rmsnorm_bwd(dy, x, w, rstd, dw, dres=dres)
    xv, rs, dyd, wd = Val(x), rstd.double()[:, None], dy.double(), w.double()[None, :]
    xh = xv * rs
    dot = ((Val(dyd) * wd) * xh).sum(1, keepdim=True, depth=_depth(d)) / float(d)
    ref_dx = Val(rs) * (Val(dyd) * wd - (xv * rs) * dot) + dres.double()
    chk(dx, ref_dx, f"{name} dx {what}")
    assert bool(torch.isfinite(dx[1].float()).all()), f"{name}: dx of the all-zero row must be finite"
    chk(dw, (Val(dyd) * xh).sum(0), f"{name} dw {what}")


def _layernorm(x: Val, d: int, eps: float):
    """layernorm_fwd_kernel: mean = sum x / d; v = sum (x - mean)^2; rs = rsqrtf(v / d + eps): (x - mean, rs)"""
    mean = x.sum(1, keepdim=True, depth=_depth(d)) / float(d)
    xc = x - mean
    return xc, ((xc * xc).sum(1, keepdim=True, depth=_depth(d)) / float(d) + f32r(eps)).rsqrt()


@case(*grid(f32in=[False, True], **NORM_GRID))
def c_layernorm_fwd(dev, f32in, d, eps):
    """the constant row: the kernel's fp32 mean of d equal values is off by up to d 2^-24 |x|, x - mean is that error and rs =
    rsqrt(eps) amplifies it - all of it inside Val's propagated terms (first and second order)"""
    from rlaif_v_amd import ops
    x = A.eps_rows(ROWS, d, seed=1, device=dev, dtype=F32) * (1 + 2.0 ** -12) if f32in else A.eps_rows(ROWS, d, seed=1, device=dev)
    w, b = _norm_w(d, dev), rnd(d, seed=6, dev=dev, scale=0.1)
    y = ops.layernorm_fwd_f32in(x, w, b, eps) if f32in else ops.layernorm_fwd(x, w, b, eps)
    xc, rs = _layernorm(Val(x), d, eps)
    name = "rv_layernorm_fwd_f32in" if f32in else "rv_layernorm_fwd"
    chk(y, xc * rs * w.double()[None, :] + b.double()[None, :], f"{name} y (d = {d}, eps = {eps})")


@case(*grid(**NORM_GRID))
def c_layernorm_bwd(dev, d, eps):
    """layernorm_bwd_kernel: xh = (x - mean) rs; s1 = sum(dy w) / d; s2 = sum(dy w xh) / d; dx = rs (dy w - s1 - (x - mean) rs s2);
    dw = sum_r dy xh, db = sum_r dy"""
    from rlaif_v_amd import ops
    x = A.eps_rows(ROWS, d, seed=1, device=dev)
    w, dy = _norm_w(d, dev), rnd(ROWS, d, seed=4, dev=dev)
    dw, db = torch.zeros(d, dtype=BF, device=dev), torch.zeros(d, dtype=BF, device=dev)
    dx = ops.layernorm_bwd(dy, x, w, eps, dw, db)
    xc, rs = _layernorm(Val(x), d, eps)
    dyd, wd = dy.double(), w.double()[None, :]
    g = Val(dyd) * wd
    xh = xc * rs
    s1 = g.sum(1, keepdim=True, depth=_depth(d)) / float(d)
    s2 = (g * xh).sum(1, keepdim=True, depth=_depth(d)) / float(d)
    what = f"(d = {d}, eps = {eps})"
    chk(dx, rs * (g - s1 - (xc * rs) * s2), f"rv_layernorm_bwd dx {what}")
    chk(dw, (Val(dyd) * xh).sum(0), f"rv_layernorm_bwd dw {what}")
    chk(db, Val(dyd).sum(0), f"rv_layernorm_bwd db {what}")


# =========================================================================================== other elementwise / data movement
@case(*grid(backward=[0, 1]))
def c_rope_inplace(dev, backward):
    """rope_kernel: o1 = a c - b s, o2 = b c + a s (s negated for backward): E = 4 * 2^-24 (|x1 cos| + |x2 sin|) covers the two
    products and the sum (3 roundings); tables fp32 with positions up to 4095"""
    from rlaif_v_amd import ops
    n, heads, hd = 96, 3, 128
    cos, sin = ops.rope_tables(4096, hd, 10000.0, dev)
    pos = (torch.arange(n, dtype=I32) * 43 % 4096)
    pos[-1] = 4095
    pos = pos.to(dev)
    x = rnd(n, heads * hd, seed=8, dev=dev)
    got = ops.rope_inplace(x.clone(), cos, sin, 4096, heads, hd, backward=bool(backward), pos=pos)
    xr = x.double().view(n, heads, 2, hd // 2)
    c, s = cos[pos.long()].double()[:, None], sin[pos.long()].double()[:, None] * (-1.0 if backward else 1.0)
    x1, x2 = xr[:, :, 0], xr[:, :, 1]
    ref = torch.stack([x1 * c - x2 * s, x2 * c + x1 * s], 2).reshape(n, heads * hd)
    E = torch.stack([x1.abs() * c.abs() + x2.abs() * s.abs(), x2.abs() * c.abs() + x1.abs() * s.abs()], 2).reshape(n, heads * hd)
    A.check(got, ref, 4 * U32 * E, BF, f"rv_rope_inplace x (backward = {backward})")


@case(("", {}))
def c_row_sums(dev):
    """rv_add_rows (one addition), rv_sum_rows_periodic, rv_colsum, rv_embed_bwd, rv_feat_grad: fp32 sums in any order, one store"""
    from rlaif_v_amd import ops
    x, p = rnd(37 * 5, 72, seed=1, dev=dev), rnd(37, 72, seed=2, dev=dev, scale=2.0 ** -6)
    chk(ops.add_rows(x, p), Val(x) + p.double().repeat(5, 1), "rv_add_rows y")
    chk(ops.sum_rows_periodic(x, 37), Val(x.double().view(5, 37, 72)).sum(0), "rv_sum_rows_periodic y")
    dy = rnd(203, 136, seed=3, dev=dev)
    chk(ops.colsum(dy), Val(dy).sum(0), "rv_colsum db")
    dxr = rnd(60, 72, seed=4, dev=dev)
    uniq, seg_off = torch.tensor([5, 0, 9], dtype=I32, device=dev), torch.tensor([0, 1, 24, 60], dtype=I32, device=dev)
    order = torch.randperm(60, generator=torch.Generator().manual_seed(5)).to(I32).to(dev)
    dW = torch.zeros(12, 72, dtype=BF, device=dev)
    ops.embed_bwd(uniq, seg_off, order, dxr, dW)
    for k, (a, b) in enumerate(((0, 1), (1, 24), (24, 60))):
        chk(dW[int(uniq[k])], Val(dxr.double()[order[a:b].long()]).sum(0), f"rv_embed_bwd dW row {int(uniq[k])} ({b - a} rows)")
    assert bool((dW[[1, 2, 3, 4, 6, 7, 8, 10, 11]] == 0).all())
    sa = torch.tensor([3, -1, 7, -1, 59], dtype=I32, device=dev)
    sb = torch.tensor([4, 2, -1, -1, 0], dtype=I32, device=dev)
    d64 = dxr.double()
    zero = torch.zeros(1, 72, dtype=F64, device=dev)
    pick = lambda idx: torch.cat([d64[i:i + 1] if i >= 0 else zero for i in idx.tolist()])       # noqa: E731
    chk(ops.feat_grad(sa, sb, dxr, 72), Val(pick(sa)) + pick(sb), "rv_feat_grad dfeat")


@case(("", {}))
def c_data_movement(dev):
    """bit-exact: rv_splice_fwd, rv_gather_rows (both directions), rv_transpose; rv_clip_assemble is one addition"""
    from rlaif_v_amd import ops
    x = _all_bf16(dev).view(255, 256)                    # every finite pattern, -0 and the subnormals included
    idx = torch.randperm(255, generator=torch.Generator().manual_seed(1)).to(I32).to(dev)
    A.check_bits(ops.gather_rows(x, idx[:100]), x[idx[:100].long()], "rv_gather_rows out (gather)")
    out = torch.zeros_like(x)
    ops.scatter_rows(x, idx, out)
    want = torch.zeros_like(x)
    want[idx.long()] = x
    A.check_bits(out, want, "rv_gather_rows out (scatter)")
    t = ops.transpose(x[:130, :200].contiguous())
    A.check_bits(t[:, :130].contiguous(), x[:130, :200].t().contiguous(), "rv_transpose out")
    assert bool((t[:, 130:].view(torch.int16) == 0).all()), "rv_transpose out: the K padding must be +0"
    feats = rnd(9, 256, seed=2, dev=dev)
    src = torch.tensor([3, -1, -2, 254, -10, 0, -1], dtype=I32, device=dev)
    want = torch.stack([x[3], torch.zeros_like(x[0]), feats[0], x[254], feats[8], x[0], torch.zeros_like(x[0])])
    A.check_bits(ops.splice_fwd(src, x, feats, 256), want, "rv_splice_fwd out")
    B, P, d = 2, 5, 72
    patch, cls, pos = rnd(B * P, d, seed=3, dev=dev), rnd(d, seed=4, dev=dev), rnd(P + 1, d, seed=5, dev=dev, scale=2.0 ** -5)
    base = torch.cat([torch.cat([cls[None], patch[b * P:(b + 1) * P]]) for b in range(B)])
    chk(ops.clip_assemble(patch, cls, pos, B, P), Val(base) + pos.double().repeat(B, 1), "rv_clip_assemble x")


# =========================================================================================== fp32 scalar kernels at the extremes
BZ = [0.0, 1e-4, -1e-4, 1.0, -1.0, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 1000.0, -1000.0]


@case(*grid(use_average=[0, 1], sft=[0.0, 0.1]))
def c_dpo_loss(dev, use_average, sft):
    """dpo_loss_kernel, beta * margin from 0 to +-1000 (the saturated regime of BASELINE config 1): loss = fmaxf(-bz, 0) +
    log1pf(__expf(-|bz|)); sig = 1.f / (1.f + __expf(bz)); gw = (-dpo_w beta sig - sft_w) / B; gr = dpo_w beta sig / B (/ cnt with
    use_average).  At bz = +88 and above the loss and sig are below 2^-126: the flush rule of the helper; nothing may be NaN."""
    from rlaif_v_amd import ops
    B, beta, dpo_w = len(BZ), 0.1, 1.0
    cnt_w, cnt_r = torch.full((B,), 7.0), torch.full((B,), 5.0)
    ref_w, ref_r = rnd(B, seed=1, dtype=F32) - 40.0, rnd(B, seed=2, dtype=F32) - 45.0
    pol_r = rnd(B, seed=3, dtype=F32) - 44.0
    z = torch.tensor(BZ, dtype=F64) / beta
    pol_w = (z + (ref_w.double() - ref_r.double()) + pol_r.double()).float()          # the margin lands near z; ref64 uses what fp32 holds
    if use_average:
        pol_w, pol_r = pol_w * cnt_w, pol_r * cnt_r
    seq_sum, seq_cnt = torch.cat([pol_w, pol_r]).to(dev), torch.cat([cnt_w, cnt_r]).to(dev)
    ref_w, ref_r = ref_w.to(dev), ref_r.to(dev)
    per_pair, scalars, coef = ops.dpo_loss(seq_sum, seq_cnt, ref_w, ref_r, beta, bool(use_average), sft, dpo_w)
    b32, bf = f32r(beta), float(B)
    pw, pr = Val(seq_sum[:B]), Val(seq_sum[B:])
    if use_average:
        pw, pr = pw / seq_cnt[:B].double(), pr / seq_cnt[B:].double()
    bz = b32 * ((pw - pr) - (Val(ref_w) - ref_r.double()))
    loss = (-bz).maximum(0.0) + (-(bz.abs())).exp().log1p()
    sig = 1.0 / (1.0 + bz.exp())
    # the values from the stable closed forms (softplus, sigmoid) in float64
    loss = Val(torch.nn.functional.softplus(-bz.v), loss.e)
    sig = Val(torch.sigmoid(-bz.v), sig.e)
    sc = lambda x: Val(torch.tensor(x, dtype=F64, device=dev))                        # noqa: E731
    gw = ((sc(-f32r(dpo_w)) * b32) * sig - f32r(sft)) / bf
    gr = ((sc(f32r(dpo_w)) * b32) * sig) / bf
    if use_average:
        gw, gr = gw / seq_cnt[:B].double(), gr / seq_cnt[B:].double()
    what = f"(use_average = {use_average}, sft = {sft})"
    for t in (per_pair, scalars, coef):
        assert bool(torch.isfinite(t).all()), f"rv_dpo_loss {what}: a non-finite output"
    chk(per_pair[0], loss, f"rv_dpo_loss per_pair losses {what}")
    chk(per_pair[1], b32 * (pw - ref_w.double()), f"rv_dpo_loss per_pair chosen rewards {what}")
    cw, cr = b32 * (pw - ref_w.double()), b32 * (pr - ref_r.double())
    chk(per_pair[2], cr, f"rv_dpo_loss per_pair rejected rewards {what}")
    chk(per_pair[3], pw, f"rv_dpo_loss per_pair policy win logp {what}")
    chk(per_pair[4], pr, f"rv_dpo_loss per_pair policy rej logp {what}")
    chk(coef[:B], gw, f"rv_dpo_loss coef win {what}")
    chk(coef[B:], gr, f"rv_dpo_loss coef rej {what}")
    inv = 1.0 / sc(bf)                                   # scalars[0] = dpo_w * a_loss * inv - sft_w * a_pw * inv
    total = f32r(dpo_w) * loss.sum(0) * inv - f32r(sft) * pw.sum(0) * inv
    # scalars[0 .. 6], ONE output tensor and one check (the symmetric +-bz make the mean chosen reward and the margin cancel; the median
    # of the cap is taken over the tensor): block sums in any order over B terms, times inv; [3] counts cw > cr - the case keeps every
    # pair at bz = 0 has cw = cr up to rounding and may count either way (1 / B in E); [7] is 0
    clear = (cw.v - cr.v).abs() > 4.0 * (cw.e + cr.e)
    assert int((~clear).sum()) <= 1, "rv_dpo_loss: only the bz = 0 pair may have rewards too close to call"
    counted = Val(((cw.v > cr.v) & clear).double()).sum(0) * inv
    counted = Val(counted.v, counted.e + float((~clear).sum()) / bf)
    parts = [total, cw.sum(0) * inv, cr.sum(0) * inv, counted, (cw.sum(0) - cr.sum(0)) * inv,
             pw.sum(0) * inv, pr.sum(0) * inv]
    chk(scalars[:7], Val(torch.stack([x.v for x in parts]), torch.stack([x.e for x in parts])), f"rv_dpo_loss scalars {what}")
    assert float(scalars[7]) == 0.0


@case(*grid(step=[1, 100000], wd=[0.0, 0.01]))
def c_adamw(dev, step, wd):
    """adamw_kernel with gradients of 1e-12 .. 1e-9, where eps = 1e-8 dominates sqrt(v): w *= 1 - lr wd; m = b1 m + (1 - b1) g;
    v = b2 v + (1 - b2) g g; w -= (lr / bc1) (m / (sqrtf(v) / sqrt(bc2) + eps)); bc = 1 - powf(beta, step) on the host in fp32
    (rv_adamw_step: powf to 1 ulp, then the subtraction); lr, betas, eps, wd as the fp32 values the ABI receives; p = RNE(master)"""
    from rlaif_v_amd import ops
    n = 4096
    gen = torch.Generator().manual_seed(step)
    g = (torch.sign(torch.randn(n, generator=gen)) * 10.0 ** (-12 + 3 * torch.rand(n, generator=gen))).to(BF).to(dev)
    master = (torch.randn(n, generator=gen) * 0.02).to(dev)
    m0 = (torch.randn(n, generator=gen) * 1e-10).to(dev) if step > 1 else torch.zeros(n, device=dev)
    v0 = (torch.rand(n, generator=gen) * 1e-20).to(dev) if step > 1 else torch.zeros(n, device=dev)
    p = master.to(BF)
    w_in, m_in, v_in = master.clone(), m0.clone(), v0.clone()
    lr, b1, b2, eps = 1e-4, 0.9, 0.999, 1e-8
    ops.adamw_step(p, master, m0, v0, g, lr, b1, b2, eps, wd, step)
    lr32, b1_32, b2_32, eps32, wd32 = f32r(lr), f32r(b1), f32r(b2), f32r(eps), f32r(wd)
    sc = lambda x: torch.tensor(x, dtype=F64, device=dev)                             # noqa: E731
    bc1 = 1.0 - Val(sc(b1_32 ** step), 2 * U32 * b1_32 ** step)
    bc2 = 1.0 - Val(sc(b2_32 ** step), 2 * U32 * b2_32 ** step)
    gg = Val(g)
    w = Val(w_in) * (1.0 - Val(sc(lr32)) * wd32)
    mv = b1_32 * Val(m_in) + (1.0 - Val(sc(b1_32))) * gg
    vv = b2_32 * Val(v_in) + ((1.0 - Val(sc(b2_32))) * gg) * gg
    denom = vv.sqrt() / bc2.sqrt() + eps32
    w = w - (lr32 / bc1) * (mv / denom)
    what = f"(step = {step}, wd = {wd})"
    chk(m0, mv, f"rv_adamw_step m {what}")
    chk(v0, vv, f"rv_adamw_step v {what}")
    chk(master, w, f"rv_adamw_step master {what}")
    A.check_bits(p, master.to(BF), f"rv_adamw_step p {what}")


@case(("", {}))
def c_seq_sum_row_coef(dev):
    """seq_sum_kernel: sum logp w and sum w over each sequence's rows (one EMPTY sequence: 0, 0), with and without weights;
    row_coef_kernel: one product"""
    from rlaif_v_amd import ops
    off = torch.tensor([0, 300, 300, 301, 1000], dtype=I32, device=dev)
    logp = -(rnd(1000, seed=1, dev=dev, dtype=F32).abs() * 3.0 + 1e-6)
    logp[::7] = -60.0
    wt = rnd(1000, seed=2, dev=dev, dtype=F32).abs()
    for weight in (None, wt):
        s, c = ops.seq_sum(logp, off, 4, weight=weight)
        for k in range(4):
            a, b = int(off[k]), int(off[k + 1])
            lv = Val(logp[a:b]) * (weight[a:b].double() if weight is not None else 1.0)
            cv = Val(weight[a:b] if weight is not None else torch.ones(b - a, device=dev))
            tag = f"(sequence {k}, {b - a} rows, {'weighted' if weight is not None else 'plain'})"
            if b == a:
                assert float(s[k]) == 0.0 and float(c[k]) == 0.0, f"rv_seq_sum {tag}: an empty sequence sums to 0"
                continue
            chk(s[k], lv.sum(0), f"rv_seq_sum out_sum {tag}")
            chk(c[k], cv.sum(0), f"rv_seq_sum out_cnt {tag}")
    coef = rnd(4, seed=3, dev=dev, dtype=F32) * 1e-3
    seq_of_row = torch.bucketize(torch.arange(1000, device=dev), off[1:].long(), right=True).to(I32)
    chk(ops.row_coef(coef, seq_of_row, wt), Val(coef[seq_of_row.long()]) * wt.double(), "rv_row_coef out (weighted)")
    A.check_bits(ops.row_coef(coef, seq_of_row), coef[seq_of_row.long()], "rv_row_coef out (plain)")


# =========================================================================================== fused GEMMs
def _mask(dev, M, N, p, seed):
    """the mask rv_dropout(p, seed) draws for a contiguous [M][N] tensor, taken from rv_dropout on ones"""
    from rlaif_v_amd import ops
    return ops.dropout(torch.ones(M, N, dtype=BF, device=dev), p, seed) != 0


def _inv_keep(p, dev):
    """1.f / (1.f - p) as the host wrappers compute it in fp32"""
    return 1.0 / (1.0 - Val(torch.tensor(f32r(p), dtype=F64, device=dev)))


def _zero(v: Val) -> Val:
    return Val(torch.zeros_like(v.v))


def _sparse(t, every=4):
    """keep every 4th column: a contraction the kernel only takes at depth >= 512 then has 128 products that are not zero"""
    return t * (torch.arange(t.shape[1], device=t.device) % every == 0).to(t.dtype)[None, :]


def _swiglu_bwd(da: Val, gu):
    """the arithmetic of swiglu_bwd_kernel / EpiSwiGLUBwd on the stored (bf16) gate|up: (d gate, d up)"""
    g, u = gu.double()[:, 0::2], gu.double()[:, 1::2]
    gv = Val(g)
    sg = 1.0 / (1.0 + (-gv).exp())
    dg = da * u * sg * (1.0 + gv * (1.0 - sg))
    dg = Val(da.v * u * torch.sigmoid(g) * (1.0 + g * torch.sigmoid(-g)), dg.e)          # the value from the stable closed form
    return dg, da * (gv * sg)


@case(*grid(kind=["fwd", "bwd"]))
def c_gemm_nn_swiglu(dev, kind):
    """rv_gemm_nn_swiglu_bf16: GU = one rounding of the accumulators, ACT = silu(g) u FROM THE ACCUMULATORS (one rounding);
    rv_gemm_nn_swiglu_bwd_bf16: d act is rounded to bf16 first (gemm.hpp EpiSwiGLUBwd: epi_unpack8(epi_pack8(v), da) - a documented
    operand rounding), then swiglu_bwd_kernel's arithmetic on the stored gate|up"""
    from rlaif_v_amd import ops
    M, d, f = 300, 192, 512
    x, wgu = rnd(M, d, seed=71, dev=dev), rnd(d, 2 * f, seed=72, dev=dev, scale=0.08)
    if kind == "fwd":
        gu, act = ops.linear_swiglu(x, wgu)
        acc = A.matmul(x, wgu)
        chk(gu, acc, "rv_gemm_nn_swiglu_bf16 GU")
        g, u = acc[:, 0::2], acc[:, 1::2]
        chk(act, g / (1.0 + (-g).exp()) * u, "rv_gemm_nn_swiglu_bf16 ACT")
        return
    gu = ops.gemm_nn(x, wgu)
    dy, wd = rnd(M, d, seed=73, dev=dev, scale=0.5), rnd(d, f, seed=74, dev=dev, scale=0.08)
    dgu = ops.linear_swiglu_bwd(dy, wd, gu)
    chk_doc(dgu[:, 0::2], lambda: _swiglu_bwd(A.matmul(dy, wd).bf16(), gu)[0], "rv_gemm_nn_swiglu_bwd_bf16 DGU gate")
    chk_doc(dgu[:, 1::2], lambda: _swiglu_bwd(A.matmul(dy, wd).bf16(), gu)[1], "rv_gemm_nn_swiglu_bwd_bf16 DGU up")


@case(*grid(use_pos=[True, False]))
def c_gemm_nn_rope(dev, use_pos):
    """rv_gemm_nn_rope_bf16: y1 = x1 cos - x2 sin, y2 = x2 cos + x1 sin on the fp32 accumulators (EpiStoreRope), one rounding;
    the v columns behind rope_cols are the plain product.  q | k | v of 2 heads each (hd = 128); K = 512 is the entry point's minimum
    (64-deep-A kernel): x keeps every 4th column (_sparse)"""
    from rlaif_v_amd import ops
    M, K, N, rope_cols, hd, L = 130, 512, 768, 512, 128, 97
    x, w = _sparse(rnd(M, K, seed=81, dev=dev)), rnd(K, N, seed=82, dev=dev, scale=0.12)
    cos, sin = ops.rope_tables(4096, hd, 10000.0, dev)
    pos = ((torch.arange(M, dtype=I32) * 61) % 4096).to(dev) if use_pos else None
    c = ops.linear_rope(x, w, cos, sin, pos, L, rope_cols, hd)
    acc = A.matmul(x, w)
    pp = pos.long() if use_pos else torch.arange(M, device=dev) % L
    cc, ss = cos[pp].double()[:, None, :], sin[pp].double()[:, None, :]
    heads = rope_cols // hd
    v4, e4 = acc.v[:, :rope_cols].reshape(M, heads, 2, 64), acc.e[:, :rope_cols].reshape(M, heads, 2, 64)
    x1, x2 = Val(v4[:, :, 0], e4[:, :, 0]), Val(v4[:, :, 1], e4[:, :, 1])
    y1, y2 = x1 * cc - x2 * ss, x2 * cc + x1 * ss
    rot = Val(torch.stack([y1.v, y2.v], 2).reshape(M, rope_cols), torch.stack([y1.e, y2.e], 2).reshape(M, rope_cols))
    chk(c[:, :rope_cols], rot, f"rv_gemm_nn_rope_bf16 C rotated columns (pos = {use_pos})")
    chk(c[:, rope_cols:], acc[:, rope_cols:], f"rv_gemm_nn_rope_bf16 C plain columns (pos = {use_pos})")


def _lora_acc(a, bt, a2, b2t, gc, dev, alpha=1.0):
    """sum_k a b + sum_q a2[:, c0(n) + q] b2 as ONE fp32 accumulation (the adapter steps run in the same K loop): per column group
    the product of the concatenated operands"""
    N, K2 = bt.shape[1], b2t.shape[0]
    groups = N // gc if gc else 1
    parts = []
    for g in range(groups):
        cols = slice(g * gc, (g + 1) * gc) if gc else slice(0, N)
        parts.append(A.matmul(torch.cat([a, a2[:, g * K2:(g + 1) * K2]], 1), torch.cat([bt[:, cols], b2t[:, cols]], 0), alpha))
    return Val(torch.cat([p.v for p in parts], 1), torch.cat([p.e for p in parts], 1))


@case(*grid(shape=[(130, 256, 128, 128, 0), (300, 768, 256, 64, 256)], residual=[False, True]))
def c_gemm_nt_lora(dev, shape, residual):
    from rlaif_v_amd import ops
    M, N, K, K2, gc = shape
    groups = N // gc if gc else 1
    a, b = rnd(M, K, seed=31, dev=dev), rnd(N, K, seed=32, dev=dev)
    a2, b2, res = rnd(M, groups * K2, seed=33, dev=dev), rnd(N, K2, seed=34, dev=dev), rnd(M, N, seed=35, dev=dev)
    c = ops.gemm_nt_lora(a, b, a2, b2, group_cols=gc, residual=res if residual else None)
    acc = _lora_acc(a, b.t(), a2, b2.t(), gc, dev)
    chk(c, acc + res.double() if residual else acc, f"rv_gemm_nt_lora_bf16 C ({shape}, residual = {residual})")


@case(*grid(kind=["nn_lora", "nn_lora a64 mi16=0", "pre p=0", "pre p=0.3"]))
def c_gemm_nn_lora(dev, kind):
    """rv_gemm_nn_lora_bf16 (K = 128: the 32-deep kernel; K = 512 with rv_set_gemm_mi16(0): the 64-deep-A kernel's 32x32x16 loop with
    the second K segment, which no other test reaches) and rv_gemm_nn_lora_pre_bf16 (K >= 512 is its documented minimum: A sparse, see
    _sparse): pre with p > 0 masks the adapter segment's fp32 accumulators (times inv_keep), the main segment accumulates on top - one
    rounding"""
    from rlaif_v_amd import ops
    M, N, K2, gc = 300, 512, 64, 256
    K = 128 if kind == "nn_lora" else 512
    groups = N // gc
    a, b = rnd(M, K, seed=61, dev=dev), rnd(K, N, seed=62, dev=dev, scale=0.05)
    a2, b2, res = rnd(M, groups * K2, seed=63, dev=dev), rnd(K2, N, seed=64, dev=dev, scale=0.2), rnd(M, N, seed=65, dev=dev)
    if kind == "nn_lora":
        c = ops.gemm_nn_lora(a, b, a2, b2, group_cols=gc, residual=res)
        chk(c, _lora_acc(a, b, a2, b2, gc, dev) + res.double(), "rv_gemm_nn_lora_bf16 C")
        return
    a = _sparse(a)
    if kind.startswith("nn_lora"):
        call("rv_set_gemm_mi16", 0)
        c = ops.gemm_nn_lora(a, b, a2, b2, group_cols=gc, residual=res)
        chk(c, _lora_acc(a, b, a2, b2, gc, dev) + res.double(), "rv_gemm_nn_lora_bf16 C (K = 512, mi16 = 0)")
        return
    p, seed = (0.3, 4711) if kind.endswith("0.3") else (0.0, 0)
    c = ops.gemm_nn_lora_pre(a, b, a2, b2, p=p, seed=seed, group_cols=gc, residual=res)
    if p == 0.0:
        chk(c, _lora_acc(a, b, a2, b2, gc, dev) + res.double(), "rv_gemm_nn_lora_pre_bf16 C (p = 0)")
        return
    ad = torch.cat([A.matmul(a2[:, g * K2:(g + 1) * K2], b2[:, g * gc:(g + 1) * gc]).v for g in range(groups)], 1)
    ade = torch.cat([A.matmul(a2[:, g * K2:(g + 1) * K2], b2[:, g * gc:(g + 1) * gc]).e for g in range(groups)], 1)
    adapter = A.where(_mask(dev, M, N, p, seed), Val(ad, ade) * _inv_keep(p, dev), Val(torch.zeros_like(ad)))
    chk(c, adapter + A.matmul(a, b) + res.double(), "rv_gemm_nn_lora_pre_bf16 C (p = 0.3)")


@case(*grid(alias=[False, True]))
def c_gemm_nt_dropout(dev, alias):
    """C = dropout(alpha A B^T) + residual: the mask and inv_keep on the fp32 value (EpiStore), then the residual, one rounding"""
    from rlaif_v_amd import ops
    M, N, K, p, seed = 300, 264, 128, 0.3, 12345
    a, b, res = rnd(M, K, seed=1, dev=dev), rnd(N, K, seed=2, dev=dev), rnd(M, N, seed=3, dev=dev)
    c = res.clone() if alias else torch.empty(M, N, dtype=BF, device=dev)
    call("rv_gemm_nt_dropout_bf16", a, K, b, K, c, N, M, N, K, c if alias else None, N if alias else 0, 0.5, p, seed)
    acc = A.matmul(a, b.t(), 0.5)
    val = A.where(_mask(dev, M, N, p, seed), acc * _inv_keep(p, dev), _zero(acc))
    chk(c, val + res.double() if alias else val, f"rv_gemm_nt_dropout_bf16 C (alias = {alias})")


MASK_SEEDS = (1234567, 89, 2147480000)


@case(*grid(G=[1, 3], kind=["down", "dgrad", "wgrad"]))
def c_lora_masks(dev, G, kind):
    """the per-module-mask adapter kernels.  down / wgrad: the kept values of X are scaled by inv_keep and ROUNDED TO BF16 before the
    MFMA (rv_dropout's arithmetic; the header says so): one documented operand rounding.  dgrad: module g's term is added "with its
    own rounding to bf16": G - 1 documented roundings of the running sum before the final store."""
    M, K, p, alpha = 300, 128, 0.25, 0.25
    seeds = MASK_SEEDS[:G] + (0,) * (3 - G)
    x, Aw = rnd(M, K, seed=1, dev=dev), rnd(64 * G, K, seed=2, dev=dev, scale=0.05)
    dt, res = rnd(M, 64 * G, seed=3, dev=dev, scale=0.5), rnd(M, K, seed=4, dev=dev)
    masks = [_mask(dev, M, K, p, s_) for s_ in seeds[:G]]
    inv = _inv_keep(p, dev)
    xd = lambda g: A.where(masks[g], (Val(x) * inv).bf16(), Val(torch.zeros(M, K, dtype=F64, device=dev)))     # noqa: E731
    if kind == "down":
        t = torch.empty(M, 64 * G, dtype=BF, device=dev)
        call("rv_gemm_nt_lora_masks_bf16", x, K, Aw, K, t, 64 * G, M, K, G, alpha, p, *seeds)
        for g in range(G):
            chk_doc(t[:, 64 * g:64 * g + 64], lambda: A.matmul_val(xd(g), Aw[64 * g:64 * g + 64].double().t(), alpha),
                    f"rv_gemm_nt_lora_masks_bf16 T module {g} of {G}")
    elif kind == "dgrad":
        aT = Aw.t().contiguous()
        c = res.clone()
        call("rv_gemm_nt_dropout_masks_bf16", dt, 64 * G, aT, 64 * G, c, K, M, K, G, c, K, p, *seeds)

        def formula():
            acc = Val(res)
            for g in range(G):
                term = A.matmul(dt[:, 64 * g:64 * g + 64], Aw[64 * g:64 * g + 64])
                acc = acc + A.where(masks[g], term * inv, _zero(term))
                if g < G - 1:
                    acc = acc.bf16()
            return acc
        chk_doc(c, formula, f"rv_gemm_nt_dropout_masks_bf16 C (G = {G})")
    else:
        splits = 3
        dA, ws = torch.empty(64 * G, K, dtype=BF, device=dev), torch.empty(splits * 64 * G * K, dtype=F32, device=dev)
        call("rv_gemm_tn_lora_masks_bf16", dt, 64 * G, x, K, dA, K, M, K, G, p, *seeds, splits, ws)
        for g in range(G):
            def formula(g=g):
                xg = xd(g)
                r = A.matmul_val(Val(xg.v.t(), xg.e.t()), dt[:, 64 * g:64 * g + 64].double())          # dA_g^T = xd_g^T dT_g
                return Val(r.v.t(), r.e.t())
            chk_doc(dA[64 * g:64 * g + 64], formula, f"rv_gemm_tn_lora_masks_bf16 dA module {g} of {G}")


LSW = dict(M=257, f=12168, d=512, rp=64)          # the smallest shape the fused adapter SwiGLU GEMMs accept (test_containment_gpu.py)


@case(*grid(p=[0.0, 0.3]))
def c_gemm_nn_lora_swiglu(dev, p):
    """forward: GU = [A | A2] [B | B2] in one accumulation, ACT = silu(g) u from the accumulators, ACTD = rv_dropout(ACT) bit for bit;
    backward: d act = A B + mask(A2 B2) inv_keep (the mask on the adapter segment's accumulators, as rv_gemm_nn_lora_pre_bf16),
    rounded to bf16 (EpiSwiGLUBwd), then SwiGLU'.  d = 512 is the minimum depth: x and dy keep every 4th column (_sparse)"""
    from rlaif_v_amd import ops
    M, f, d, rp, seed = LSW["M"], LSW["f"], LSW["d"], LSW["rp"], 12345
    x, wgu, t = _sparse(rnd(M, d, seed=91, dev=dev)), rnd(d, 2 * f, seed=92, dev=dev, scale=0.12), rnd(M, 2 * rp, seed=93, dev=dev, scale=0.5)
    bexp = torch.zeros(2 * rp, 2 * f, dtype=BF, device=dev)
    bexp[:rp, 0::2] = rnd(rp, f, seed=94, dev=dev, scale=0.1)
    bexp[rp:, 1::2] = rnd(rp, f, seed=95, dev=dev, scale=0.1)
    gu, act, actd = ops.linear_lora_swiglu(x, wgu, t, bexp, p=p, seed=seed)
    acc = A.matmul(torch.cat([x, t], 1), torch.cat([wgu, bexp], 0))
    chk(gu, acc, f"rv_gemm_nn_lora_swiglu_bf16 GU (p = {p})")
    g, u = acc[:, 0::2], acc[:, 1::2]
    chk(act, g / (1.0 + (-g).exp()) * u, f"rv_gemm_nn_lora_swiglu_bf16 ACT (p = {p})")
    if p > 0:
        A.check_bits(actd, ops.dropout(act.contiguous(), p, seed), "rv_gemm_nn_lora_swiglu_bf16 ACTD")
    del acc, g, u
    dy, wd = _sparse(rnd(M, d, seed=96, dev=dev, scale=0.5)), rnd(d, f, seed=97, dev=dev, scale=0.12)
    dt, ad = rnd(M, rp, seed=98, dev=dev, scale=0.5), rnd(rp, f, seed=99, dev=dev, scale=0.1)
    dgu = ops.linear_lora_swiglu_bwd(dy, wd, dt, ad, gu, p=p, seed=seed)
    mask = _mask(dev, M, f, p, seed) if p > 0 else None

    def dact():
        adapter = A.matmul(dt, ad)
        if p > 0:
            adapter = A.where(mask, adapter * _inv_keep(p, dev), _zero(adapter))
            return (adapter + A.matmul(dy, wd)).bf16()
        return A.matmul(torch.cat([dy, dt], 1), torch.cat([wd, ad], 0)).bf16()
    chk_doc(dgu[:, 0::2], lambda: _swiglu_bwd(dact(), gu)[0], f"rv_gemm_nn_lora_swiglu_bwd_bf16 DGU gate (p = {p})")
    chk_doc(dgu[:, 1::2], lambda: _swiglu_bwd(dact(), gu)[1], f"rv_gemm_nn_lora_swiglu_bwd_bf16 DGU up (p = {p})")


@case(("", {}))
def c_gemm_tn_ws(dev):
    """rv_gemm_tn_bf16_ws at the smallest shape the library plans a tail split for (test_containment_gpu.py found (4096, 3080,
    4872)): every 16th contraction row is not zero, so each output is a sum of 256 products - the slabs of the split add exact
    zeros or a few more fp32 additions, inside "any order" """
    from rlaif_v_amd import hip
    R, I, J = 4096, 3080, 4872
    need = int(hip.lib().lib.rv_gemm_tn_workspace_floats(R, I, J))
    assert need > 0, "the library plans no tail split for the containment table's shape"
    gen = torch.Generator(device=dev).manual_seed(1)
    rows = (torch.arange(R, device=dev) % 16 == 5).to(BF)[:, None]
    p = (torch.randn(R, I, device=dev, generator=gen)).to(BF) * rows
    q = (torch.randn(R, J, device=dev, generator=gen)).to(BF) * rows
    c, ws = torch.empty(I, J, dtype=BF, device=dev), torch.empty(need, dtype=F32, device=dev)
    call("rv_gemm_tn_bf16_ws", p, I, q, J, c, J, R, I, J, ws, need)
    keep = rows[:, 0] != 0
    val = A.matmul(p[keep].t(), q[keep])                  # the zero rows contribute exact zeros
    chk(c, val, f"rv_gemm_tn_bf16_ws C ({R}x{I}x{J}, 256 rows not zero)")


# =========================================================================================== LM head
@case(*grid(variant=[-1, 3]))
def c_lmhead(dev, variant):
    """n 70, d 64, V 128 with V_valid 121, logits spanning +-40 (accuracy.lmhead_inputs / lmhead_bound): logp at the argmax (~ -1e-6),
    in the deep tail, at id 0 and V_valid - 1; the target -100 leaves the caller's fill: logp = 0 - lse"""
    from rlaif_v_amd import ops
    n, V, vv = 70, 128, 121
    h, w, tgt = A.lmhead_inputs(n, 64, V, vv, device=dev)
    pmax, psum = torch.empty(n, V // 64, dtype=F32, device=dev), torch.empty(n, V // 64, dtype=F32, device=dev)
    tl, lse, logp = torch.zeros(n, dtype=F32, device=dev), torch.empty(n, dtype=F32, device=dev), torch.empty(n, dtype=F32, device=dev)
    call("rv_lmhead_logp_fwd", h, 64, w, 64, tgt, n, V, vv, 64, pmax, psum, tl, variant)
    call("rv_logp_finish", pmax, psum, tl, V // 64, n, lse, logp)
    logp_b, lse_b, _, _ = A.lmhead_bound(h, w, tgt, vv)
    ok = tgt >= 0
    chk(lse, lse_b, f"rv_logp_finish lse (variant = {variant})")
    chk(logp[ok], logp_b[ok], f"rv_logp_finish logp (variant = {variant})")
    A.check_bits(logp[~ok], -lse[~ok], "rv_logp_finish logp of the rows without a vocabulary target")
    # finish + unpack: the same device code, bit-equal; row m to per_token[m + 3] and compact[n - 1 - m], every 5th row nowhere
    m = torch.arange(n, dtype=I32, device=dev)
    dst_a = torch.where(m % 5 == 0, torch.full_like(m, -1), m + 3)
    dst_b, dst_c = torch.full_like(m, -1), n - 1 - m
    per_token, compact = torch.full((n + 8,), 7.0, dtype=F32, device=dev), torch.full((n,), 7.0, dtype=F32, device=dev)
    call("rv_logp_finish_unpack", pmax, psum, tl, V // 64, n, dst_a, dst_b, dst_c, per_token, n + 8, compact, n)
    want = torch.full((n + 8,), 7.0, dtype=F32, device=dev)
    want[3:n + 3] = torch.where(m % 5 == 0, torch.full_like(logp, 7.0), logp)
    A.check_bits(per_token, want, "rv_logp_finish_unpack per_token")
    A.check_bits(compact, logp.flip(0), "rv_logp_finish_unpack compact")
    coef = rnd(n, seed=9, dev=dev, dtype=F32) * 0.1
    dl = ops.lmhead_logp_bwd(h, w, tgt, lse, coef, n, v_valid=vv)
    chk(dl, A.lmhead_bwd_bound(h, w, tgt, lse, coef, vv), f"rv_lmhead_logp_bwd dlogits (variant = {variant})")
    assert bool((dl[:, vv:] == 0).all())


@case(("", {}))
def c_next_token_scores(dev):
    """logits spanning +-1e4, repetition penalty on, tied maxima (the lowest index wins), one wanted id out of range.
    next_token_scores_kernel: a seen logit is l / penalty or l * penalty (one rounding: dl = 2^-24 |l'|, and d lse / d l_i = P_i); every
    exponent is a rounded difference whose distances telescope to mx - l_i over the online rescales (2^-24 (mx - l_i)); a term passes
    ceil(V / 256) + 8 rescale-and-add events (thread loop, 6 shuffle steps, 2 combine levels), each of them, in units of 2^-24:
    expf to 1 ulp (2) + the product sum * expf (1) + the addition (1) = 4; logf FEW; logp = l' - lse; probs = expf(logp)"""
    from rlaif_v_amd import ops
    M, V, ldl, pen = 6, 1000, 1024, 1.3
    gen = torch.Generator().manual_seed(3)
    logits = torch.clamp(torch.randn(M, ldl, generator=gen) * 3000.0, -1e4, 1e4)
    logits[0, 700], logits[0, 200] = 9500.0, 9500.0              # tied maxima, neither seen: argmax 200
    logits[1] = torch.randn(ldl, generator=gen) * 2.0             # an ordinary row: many terms in the sum
    logits[2] = torch.clamp(logits[2], -7000.0, 7000.0)
    logits[2, 17] = 1e4                                           # the maximum is a seen id: 1e4 / 1.3 still wins
    logits[3, :V] = -3.0                                          # all equal: argmax 0, lse = -3 pen + log V (all seen below)
    logits[:, V:] = 3e4                                           # vocabulary padding must not enter
    seen_rows = [[5, 700 + 1, 999], [3, 3, 8], [17, 1000, 5000, -4], list(range(V)), [], [0]]
    import itertools
    seen_off = torch.tensor([0] + list(itertools.accumulate(len(r) for r in seen_rows)), dtype=I32, device=dev)
    seen_ids = torch.tensor([i for r in seen_rows for i in r], dtype=I32, device=dev)
    want = torch.tensor([3, 200, 17, 999, 1000, 0], dtype=I32, device=dev)
    logits = logits.to(dev)
    probs, logp, argmax, lse = ops.next_token_scores(logits, M, V, want, seen=(seen_off, seen_ids), penalty=pen)
    pen32 = f32r(pen)
    seen = torch.zeros(M, V, dtype=torch.bool, device=dev)
    for r, ids in enumerate(seen_rows):
        for i in ids:
            if 0 <= i < V:
                seen[r, i] = True
    l64 = logits[:, :V].double()
    lp = torch.where(seen, torch.where(l64 > 0, l64 / pen32, l64 * pen32), l64)
    dl = torch.where(seen, U32 * lp.abs(), torch.zeros_like(lp))
    mx = lp.max(-1, keepdim=True).values
    P = torch.softmax(lp, -1)
    n_ev = (V + 255) // 256 + 8
    ref_lse = torch.logsumexp(lp, -1)
    E_lse = (P * (dl + U32 * (mx - lp) + 4 * U32 * n_ev)).sum(-1) + A.FEW * U32 * (ref_lse - mx[:, 0]).abs() + U32 * ref_lse.abs()
    chk(lse, Val(ref_lse, E_lse), "rv_next_token_scores lse")
    inr = (want >= 0) & (want < V)
    wi = want[inr].long()
    lpv = Val(lp[:, wi], dl[:, wi]) - Val(ref_lse, E_lse).v[:, None]
    lpv = Val(lpv.v, lpv.e + E_lse[:, None])
    chk(logp[:, inr], lpv, "rv_next_token_scores logp")
    chk(probs[:, inr], lpv.exp(fast=False), "rv_next_token_scores probs")
    assert bool((logp[:, ~inr] == -math.inf).all()) and bool((probs[:, ~inr] == 0).all()), "an id out of range: 0 / -inf"
    first_max = torch.where(lp == mx, torch.arange(V, device=dev)[None, :], V).min(-1).values
    gap = (mx[:, 0] - torch.where(lp == mx, torch.full_like(lp, -math.inf), lp).max(-1).values)
    assert bool((gap[[0, 1, 2, 4, 5]] > 1e-2).all()), "the case's maxima must be clear of the runner-up (ties aside)"
    assert torch.equal(argmax.long(), first_max), f"rv_next_token_scores argmax {argmax.tolist()} against {first_max.tolist()}"


# =========================================================================================== attention
ATTN_LAYOUTS = {"L1": dict(L=1), "L65": dict(L=65), "L200": dict(L=200), "packed-L200": dict(L=200, seg=([40, 0], [120, 64])),
                "pad-free-130-77": dict(L=130, lens=[130, 77])}
CAUSAL_LAYOUTS = list(ATTN_LAYOUTS)
# causal = 0 (attn_fwd2_kernel<64 / 128, false>, attn_fwd3_kernel<false>, attn_bwd_dq2 / dkv3 / dkv5_kernel<false>): one pass per
# workgroup, an unpaired grid, kv_end = L and t_begin = 0 - every query meets the ragged last key tile, the only masked one.  The
# smallest shapes that reach each path.  hds / G128: where the discrimination cap (accuracy.check) admits the layout - at L = 257 with
# head dim 128 and ONE kv head, and at L = 577 with head dim 128, median E / ulp of `out` passes 1/8 (tests/test_accuracy_helper.py
# runs every admitted combination through the CPU emulation and prints the figures).
FULL_LAYOUTS = {
    "full-L1": dict(L=1),                                         # a single key and a single query
    "full-L65": dict(L=65),                                       # one full key tile + a one-key tail, for every query
    "full-L200": dict(L=200),                                     # two 128-query blocks; the ragged fourth key tile is seen by all rows
    "full-L257": dict(L=257, G128=(1,)),                          # three 128-query blocks (odd, unpaired grid); 256 + 1 for fwd3's 256-query blocks
    "full-pad-free-130-77": dict(L=130, lens=[130, 77]),          # row_off / row_len with causal = 0 (varlen_done without pairing)
    "full-window-L200": dict(L=200, seg=([40, 0], [120, 64])),    # the window under causal = 0: queries >= e1 do not see [sh, e1)
    "full-L577": dict(L=577, hds=(64,)),                          # the CLIP tower's own length: 4 blocks + 65
    # the OmniLMM Resampler: nq live queries against all L keys; the query rows >= nq are zero and so is their dO.  Reference and
    # bound are built from the nq live queries only (Lq = 64, Lk = 200): a dead row may contribute NOTHING to dK / dV
    "resampler-L200-nq64": dict(L=200, nq=64, hds=(128,)),
}
for _c in FULL_LAYOUTS.values():
    _c["causal"] = False
ATTN_LAYOUTS.update(FULL_LAYOUTS)


def full_layout_cases(**axes):
    """grid(**axes, layout = the non-causal layouts) without the combinations the cap does not admit (FULL_LAYOUTS)"""
    out = []
    for cid, kw in grid(**axes, layout=list(FULL_LAYOUTS)):
        c, hd = FULL_LAYOUTS[kw["layout"]], kw.get("hd", 128)
        if hd in c.get("hds", (64, 128)) and (hd != 128 or kw["G"] in c.get("G128", (1, 2))):
            out.append((cid, kw))
    return out


def _attn_layout(dev, L, hd, G, lens=None, seed=0, nq=None):
    """S = 2, H = 2 (kv_group G: H / G key / value heads) with the input rows of accuracy.spiked_attention_rows, laid out as qkv
    [tokens][q heads | k heads | v heads].  lens: pad-free rows (sequence s has lens[s] <= L tokens, 3 / 5 token rows of gap in front
    of the sequences); nq: the query rows >= nq of every sequence are zero (the Resampler): returns (qkv, q, k, v, starts, lens)"""
    S, H, Hkv = 2, 2, 2 // G
    q, k, v = A.spiked_attention_rows(S, L, H, hd, seed=seed, device=dev, kv_heads=Hkv)
    lens = lens or [L, L]
    starts = [0, L] if lens == [L, L] else [3, 3 + lens[0] + 5]
    ntok = S * L if lens == [L, L] else starts[1] + lens[1] + 4
    qkv = rnd(ntok, (H + 2 * Hkv) * hd, seed=99, dev=dev)         # the gap rows hold ordinary values no result may depend on
    for s_ in range(S):
        n, a = lens[s_], starts[s_]
        qkv[a:a + n, :H * hd] = q[s_, :, :n].transpose(0, 1).reshape(n, H * hd)
        qkv[a:a + n, H * hd:(H + Hkv) * hd] = k[s_, :, :n].transpose(0, 1).reshape(n, Hkv * hd)
        qkv[a:a + n, (H + Hkv) * hd:] = v[s_, :, :n].transpose(0, 1).reshape(n, Hkv * hd)
        if nq is not None:
            qkv[a + nq:a + n, :H * hd] = 0
    return qkv, q, k, v, starts, lens


def _allowed(c, s_, n, dev, nq=None):
    """the mask of sequence s_ (n tokens) as the reference sees it: [nq or n queries][n keys]"""
    seg = (c["seg"][0][s_], c["seg"][1][s_]) if "seg" in c else None
    if c.get("causal", True):
        return A.causal_allowed(n, n, dev, seg=seg)
    return A.full_allowed(nq or n, n, dev, seg=seg)


def _attn_call_args(c, dev, starts, lens):
    seg = tuple(torch.tensor(t, dtype=I32, device=dev) for t in c["seg"]) if "seg" in c else None
    rows = (torch.tensor(starts, dtype=I32, device=dev), torch.tensor(lens, dtype=I32, device=dev)) if "lens" in c else None
    return seg, rows


def _check_attn_fwd(c, dev, hd, G, out, lse, q, k, v, starts, lens, what):
    """one check per output tensor: all sequences and heads of the case (the live queries of a Resampler layout)"""
    H, scale = 2, 1.0 / math.sqrt(hd)
    go, ro, eo, do_, gl, rl, el = [], [], [], [], [], [], []
    for s_ in range(2):
        n, a = lens[s_], starts[s_]
        nq = c.get("nq", n)
        ok = _allowed(c, s_, n, dev, nq)
        for h in range(H):
            ov, doc, lv = A.attn_fwd_bound(q[s_, h, :nq], k[s_, h // G, :n], v[s_, h // G, :n], ok, scale)
            go.append(out[a:a + nq, h * hd:(h + 1) * hd]), ro.append(ov.v), eo.append(ov.e), do_.append(doc)
            gl.append(lse[s_, h, :nq]), rl.append(lv.v), el.append(lv.e)
    return (chk(torch.cat(go), Val(torch.cat(ro), torch.cat(eo)), f"{what} out", doc=torch.cat(do_)),
            chk(torch.cat(gl), Val(torch.cat(rl), torch.cat(el)), f"{what} lse"))


@case(*grid(version=[2, 3], hd=[64, 128], G=[1, 2], layout=CAUSAL_LAYOUTS),
      *full_layout_cases(version=[2, 3], hd=[64, 128], G=[1, 2]))
def c_attn_fwd(dev, version, hd, G, layout):
    """rv_attn_fwd, both forward kernels of head dim 128 (rv_set_attn_fwd_version; at head dim 64 there is one kernel and the knob
    must not matter), causal and full: bounds and their derivation in accuracy.attn_fwd_bound, first passed by its CPU emulation
    (test_accuracy_helper.py)"""
    from rlaif_v_amd import ops
    c = ATTN_LAYOUTS[layout]
    L = c["L"]
    call("rv_set_attn_fwd_version", version)
    qkv, q, k, v, starts, lens = _attn_layout(dev, L, hd, G, c.get("lens"), nq=c.get("nq"))
    seg, rows = _attn_call_args(c, dev, starts, lens)
    H, Hkv = 2, 2 // G
    out, lse = ops.attn_fwd(qkv, 2, L, H, hd, c.get("causal", True), 0, H * hd, (H + Hkv) * hd, seg=seg, kv_group=G, rows=rows)
    _check_attn_fwd(c, dev, hd, G, out, lse, q, k, v, starts, lens, f"rv_attn_fwd (version {version}, hd {hd}, kv_group {G}, {layout})")


@case(*grid(hd=[64, 128], G=[1, 2]))
def c_attn_fwd_branches(dev, hd, G):
    """rv_attn_fwd_branches with two branches = the packed pair of rv_attn_fwd (seg_sh, seg_e1): the same bound"""
    from rlaif_v_amd import ops
    c = ATTN_LAYOUTS["packed-L200"]
    L, H, Hkv = 200, 2, 2 // G
    qkv, q, k, v, starts, lens = _attn_layout(dev, L, hd, G)
    seg_sh = torch.tensor(c["seg"][0], dtype=I32, device=dev)
    q_lo = torch.zeros(2 * L, dtype=I32, device=dev)
    for s_ in range(2):
        sh, e1 = c["seg"][0][s_], c["seg"][1][s_]
        i = torch.arange(L, device=dev)
        q_lo[s_ * L:(s_ + 1) * L] = torch.where(i >= e1, torch.full_like(i, e1), torch.full_like(i, sh)).to(I32)
    out, lse = ops.attn_fwd(qkv, 2, L, H, hd, True, 0, H * hd, (H + Hkv) * hd, kv_group=G, branches=(seg_sh, q_lo))
    _check_attn_fwd(c, dev, hd, G, out, lse, q, k, v, starts, lens, f"rv_attn_fwd_branches (hd {hd}, kv_group {G})")


def _attn_bwd_dO(c, dev, ntok, starts, lens, H=2, hd=128):
    """dO of a backward case; the rows of a Resampler layout's dead queries are zero"""
    dO = rnd(ntok, H * hd, seed=5, dev=dev, scale=0.5)
    if "nq" in c:
        for a, n in zip(starts, lens):
            dO[a + c["nq"]:a + n] = 0
    return dO


def _check_attn_bwd(c, dev, G, dqkv, dO, O, lse, q, k, v, starts, lens, what, rope=None):
    """one check per gradient: all sequences and heads of the case.  A key / value head sums the terms of its kv_group query heads in
    the same fp32 accumulators.  rope = (cos, sin, pos) of the fused inverse rotation.  A Resampler layout (nq): the reference has the nq
    live queries only, over all keys - no term from a dead row - and dQ of the dead rows must be +0 bit for bit (dS = P (dP - delta) with
    dO = 0 is P * (0 - 0) whatever P is)"""
    hd, H, Hkv = 128, 2, 2 // G
    scale = 1.0 / math.sqrt(hd)
    k0, v0 = H * hd, (H + Hkv) * hd
    acc = {n_: ([], [], [], []) for n_ in ("dQ", "dK", "dV")}

    def put(name, got, val, doc):
        for lst, x in zip(acc[name], (got, val.v, val.e, doc)):
            lst.append(x)
    for s_ in range(2):
        n, a = lens[s_], starts[s_]
        nq = c.get("nq", n)
        ok = _allowed(c, s_, n, dev, nq)
        cs = (rope[0][rope[2][a:a + n].long()].double(), rope[1][rope[2][a:a + n].long()].double()) if rope else None
        per_kv = {}
        for h in range(H):
            res = A.attn_bwd_bound(q[s_, h, :nq], k[s_, h // G, :n], v[s_, h // G, :n], dO[a:a + nq, h * hd:(h + 1) * hd],
                                   O[a:a + nq, h * hd:(h + 1) * hd], lse[s_, h, :nq], ok, scale)
            val, doc = res["dQ"]
            if rope:
                val, doc = A.rope_bwd_val(val, doc, *cs)
            put("dQ", dqkv[a:a + nq, h * hd:(h + 1) * hd], val, doc)
            for name in ("dK", "dV"):
                val, doc = res[name]
                if (h // G, name) in per_kv:
                    pv, pd = per_kv[(h // G, name)]
                    val, doc = Val(pv.v + val.v, pv.e + val.e + U32 * (pv.v + val.v).abs()), pd + doc
                per_kv[(h // G, name)] = (val, doc)
        for (hk, name), (val, doc) in per_kv.items():
            if rope and name == "dK":
                val, doc = A.rope_bwd_val(val, doc, *cs)
            c0 = (k0 if name == "dK" else v0) + hk * hd
            put(name, dqkv[a:a + n, c0:c0 + hd], val, doc)
        if nq < n:
            dead = dqkv[a + nq:a + n, :H * hd].contiguous()
            A.check_bits(dead, torch.zeros_like(dead), f"{what} dQ of the dead query rows")
    return {name: A.check(torch.cat(got), torch.cat(vv), torch.cat(ee), BF, f"{what} {name}", doc=torch.cat(doc), cap_unit="ulp+doc")
            for name, (got, vv, ee, doc) in acc.items()}


@case(*grid(dkv=[3, 5], rope=[False, True], G=[1, 2], layout=CAUSAL_LAYOUTS),
      *full_layout_cases(dkv=[3, 5], rope=[False], G=[1, 2]))
def c_attn_bwd(dev, dkv, rope, G, layout):
    """rv_attn_bwd (head dim 128), both dK/dV kernels, causal (with and without the fused inverse RoPE) and full, on the forward
    kernel's O and lse (exact operands of this call): accuracy.attn_bwd_bound / rope_bwd_val, first passed by their CPU emulation.
    The cap is measured against ulp + doc (accuracy.check)"""
    from rlaif_v_amd import ops
    c = ATTN_LAYOUTS[layout]
    L, hd, H, Hkv = c["L"], 128, 2, 2 // G
    causal = c.get("causal", True)
    call("rv_set_attn_dkv_version", dkv)
    qkv, q, k, v, starts, lens = _attn_layout(dev, L, hd, G, c.get("lens"), seed=1, nq=c.get("nq"))
    seg, rows = _attn_call_args(c, dev, starts, lens)
    k0, v0 = H * hd, (H + Hkv) * hd
    O, lse = ops.attn_fwd(qkv, 2, L, H, hd, causal, 0, k0, v0, seg=seg, kv_group=G, rows=rows)
    dO = _attn_bwd_dO(c, dev, qkv.shape[0], starts, lens)
    rp = None
    if rope:
        cos, sin = ops.rope_tables(4096, hd, 10000.0, dev)
        pos = ((torch.arange(qkv.shape[0], dtype=I32) * 53 + 7) % 4096).to(dev)
        rp = (cos, sin, pos)
    dqkv = ops.attn_bwd(qkv, O, dO, lse, 2, L, H, hd, causal, 0, k0, v0, seg=seg, kv_group=G, rope=rp, rows=rows)
    _check_attn_bwd(c, dev, G, dqkv, dO, O, lse, q, k, v, starts, lens, f"rv_attn_bwd (dkv {dkv}, rope {rope}, kv_group {G}, {layout})",
                    rope=rp)


@pytest.mark.parametrize("fn,kw", CASES)
def test_accuracy(fn, kw):
    run_case(fn, **kw)
