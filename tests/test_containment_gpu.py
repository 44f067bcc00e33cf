"""Guard-band and poison containment of the kernel entry points (include/rlaifv_hip.h).

Every case builds its operands through tests/guarded.py - windows of larger allocations whose surroundings hold a NaN sentinel -
launches the entry point on them through the C ABI (rlaif_v_amd.hip.call, so that no wrapper allocates an output, a statistic or a
workspace behind the test's back) and asserts three things:
  (a) the inside matches the reference (the reference and the bound of the entry point's own test where it has one);
  (b) every guard of every output, in/out operand and workspace is intact, every input is bit-unchanged, and the kernel wrote
      everything its contract says it writes;
  (c) the same call on the CLEAN layout - identical geometry, zeros instead of NaNs around and between the inputs - gives
      bit-identical outputs, and no output holds a NaN: nothing a result depends on lies outside what the caller must define.
Every launch is an ordinary in-bounds call on buffers the test owns.

    python -m pytest tests/test_containment_gpu.py -q -m gpu
"""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded as G  # noqa: E402
from test_kernels_gpu import _packed_mask, close  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
_LD_MULT = {BF: 8, F32: 4, I32: 4, torch.uint8: 16}        # rows of every operand stay 16-byte aligned


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rnd(*shape, scale=1.0, seed=0, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def i32(v):
    return torch.as_tensor(v, dtype=I32)


class Layout:
    """The operands of one call, all guarded; clean = the zero-surrounded twin of the poisoned layout."""

    def __init__(self, dev, clean):
        self.dev, self.clean = dev, clean
        self.items = []                 # (Guarded, kind, written, saved bits)
        self.finished = 0

    def _make(self, name, shape, dtype, fill, inner, kind, written):
        shape = tuple(shape)
        if len(shape) == 1:
            g = G.guarded_1d_obj(shape[0], dtype, self.dev, fill=fill, name=name, clean=self.clean, inner=inner, role=kind)
            t = g.flat
        else:
            g = G.Guarded(shape[0], shape[1], dtype, self.dev, fill=fill, name=name, clean=self.clean, inner=inner,
                          ld_multiple=_LD_MULT[dtype], role=kind)
            t = g.view
        self.items.append([g, kind, written, g.bits() if kind == "in" else None])
        return t

    def inp(self, name, t, inner=None):
        """read-only operand: poison (or zeros) around it and in its `inner` gaps; must come back bit-unchanged"""
        return self._make(name, t.shape, t.dtype, t, inner, "in", None)

    def io(self, name, t, inner=None):
        """in/out operand"""
        return self._make(name, t.shape, t.dtype, t, inner, "io", None)

    def out(self, name, shape, dtype=BF, written=True, inner=None):
        """pure output or workspace: sentinel inside; `written` = what the contract says the kernel writes (True: all of it)"""
        return self._make(name, shape, dtype, None, inner, "out", written)

    def finish(self):
        torch.cuda.synchronize()
        for g, kind, written, saved in self.items:
            g.check(written=written if kind == "out" else None)
            if kind == "in":
                assert torch.equal(g.bits(), saved), f"{g.name}: a read-only operand changed"
        self.finished += 1

    def results(self):
        out = {}
        for g, kind, _, _ in self.items:
            if kind != "in":
                bits, keep = g.bits(), ~g.inner if g.inner is not None else None
                sent = bits == g.sentinel
                if g.dtype.is_floating_point:
                    nan = torch.isnan(g.view) & ~sent
                    if keep is not None:
                        nan = nan & keep
                    assert not bool(nan.any()), f"{g.name}: NaN in an output ({int(nan.sum())} elements)"
                out[g.name] = bits if keep is None else torch.where(keep, bits, torch.zeros_like(bits))
        return out


def run_case(fn, **kw):
    """(a) + (b) inside fn on the poisoned layout and again on the clean one, then (c): bit-equal outputs"""
    dev = _dev()
    res = []
    for clean in (False, True):
        lay = Layout(dev, clean)
        try:
            fn(lay, **kw)
        except RuntimeError as e:
            if "HIP error" in str(e) or "illegal memory access" in str(e):      # a faulted device: start nothing more on it
                pytest.exit(f"GPU fault in {fn.__name__} {kw}: {e}", returncode=3)
            raise
        assert lay.finished, "the case never checked its guards"
        lay.finish()
        res.append(lay.results())
    assert res[0].keys() == res[1].keys()
    for name in res[0]:
        same = res[0][name] == res[1][name]
        assert bool(same.all()), (f"{name}: the result depends on memory outside the operands: {int((~same).sum())} element(s) differ "
                                  f"between NaN-surrounded and zero-surrounded inputs, first at {(~same).nonzero()[0].tolist()}")


def call(name, *args):
    from rlaif_v_amd import hip
    hip.call(name, *args)


def ld(t):
    return t.stride(0)


def yardstick(got, yard, ref64, what):
    """The kernel's error against the float64 result may be at most twice that of torch's own fp32 implementation rounded to the
    kernel's output type (max and mean): the factor covers another, equally legitimate fp32 summation order."""
    e_k, e_y = (got.double() - ref64).abs(), (yard.double() - ref64).abs()
    msg = (f"{what}: kernel max {e_k.max().item():.4e} mean {e_k.mean().item():.4e}; "
           f"fp32 torch yardstick max {e_y.max().item():.4e} mean {e_y.mean().item():.4e}")
    print(msg)
    assert torch.isfinite(got.float()).all(), msg
    assert e_k.max().item() <= 2 * e_y.max().item() and e_k.mean().item() <= 2 * e_y.mean().item(), msg


CASES = []


def case(*ids_kwargs):
    """register fn once per (id, kwargs) pair"""
    def deco(fn):
        for cid, kw in ids_kwargs:
            CASES.append(pytest.param(fn, kw, id=f"{fn.__name__[2:]}[{cid}]" if cid else fn.__name__[2:]))
        return fn
    return deco


def grid(**axes):
    """[(id, kwargs)] over the cross product of the axes"""
    import itertools
    keys = list(axes)
    out = []
    for vals in itertools.product(*[axes[k] for k in keys]):
        kw = dict(zip(keys, vals))
        out.append(("-".join(f"{k}={'x'.join(map(str, v)) if isinstance(v, tuple) else v}" for k, v in kw.items()), kw))
    return out


# =========================================================================================== norms
NORM_SHAPES = [(3, 40), (333, 520)]


def _row_idx(rows, use_idx):
    """(x rows, idx or None): with row_idx the x operand has more rows than the call names, in a shuffled order"""
    if not use_idx:
        return rows, None
    xrows = rows + max(2, rows // 5)
    return xrows, torch.randperm(xrows, generator=torch.Generator().manual_seed(rows))[:rows].to(I32)


def _unnamed(xrows, idx, d):
    if idx is None:
        return None
    m = torch.ones(xrows, dtype=torch.bool)
    m[idx.long()] = False
    return m[:, None].expand(xrows, d)


@case(*grid(shape=NORM_SHAPES, use_idx=[False, True], kind=["bf16", "f32", "f32add", "dropout"]))
def c_rmsnorm_fwd(lay, shape, use_idx, kind):
    (rows, d), eps = shape, 1e-5
    xrows, idx = _row_idx(rows, use_idx)
    hole = _unnamed(xrows, idx, d)
    w = (1 + 0.1 * rnd(d, seed=2).float()).to(BF)
    x32 = rnd(xrows, d, seed=1, dtype=F32) * 2.0
    xh = x32 if kind in ("f32", "f32add") else x32.to(BF)
    x = lay.inp("x", xh, inner=hole)
    wd = lay.inp("w", w)
    ix = lay.inp("row_idx", idx) if use_idx else None
    y = lay.out("y", (rows, d))
    rstd = lay.out("rstd", (rows,), F32)
    sel = idx.long() if use_idx else torch.arange(rows)
    xs = xh.float()[sel].to(lay.dev)
    if kind == "bf16":
        call("rv_rmsnorm_fwd", x, ld(x), ix, wd, y, ld(y), rstd, rows, d, eps)
    elif kind == "f32":
        call("rv_rmsnorm_fwd_f32", x, ld(x), ix, None, 0, None, 0, wd, y, ld(y), rstd, rows, d, eps)
    elif kind == "f32add":
        # add and xout are indexed like x (rows row_idx names); y and rstd by the call's own row number
        addh = rnd(xrows, d, seed=4, scale=0.2)
        add = lay.inp("add", addh, inner=hole)
        xout = lay.out("xout", (xrows, d), F32, inner=hole)
        call("rv_rmsnorm_fwd_f32", x, ld(x), ix, add, ld(add), xout, ld(xout), wd, y, ld(y), rstd, rows, d, eps)
        xs = xs + addh.float()[sel].to(lay.dev)
    else:
        yd = lay.out("yd", (rows * d,))                    # contiguous [rows][d]
        call("rv_rmsnorm_fwd_dropout", x, ld(x), ix, wd, y, ld(y), rstd, rows, d, eps, yd, 0.3, 77)
    lay.finish()
    if kind == "f32add":
        assert torch.equal(xout[sel.to(lay.dev)], xs)       # the fp32 sum is exact
    ref_rstd = torch.rsqrt(xs.pow(2).mean(-1) + eps)
    close(y, xs * ref_rstd[:, None] * w.float().to(lay.dev), rel=1e-2 if kind == "f32add" else 1.6e-2, what=f"rmsnorm fwd {kind}")
    torch.testing.assert_close(rstd, ref_rstd, rtol=1e-5, atol=1e-6)
    if kind == "dropout":
        from rlaif_v_amd import ops
        assert torch.equal(yd.view(rows, d), ops.dropout(y.contiguous(), 0.3, 77))


@case(*grid(shape=NORM_SHAPES, use_idx=[False, True], f32x=[False, True]))
def c_rmsnorm_bwd(lay, shape, use_idx, f32x):
    """dw written, then accumulated by a second call; dx / dres are indexed like x: rows row_idx does not name stay sentinel"""
    (rows, d), eps = shape, 1e-5
    xrows, idx = _row_idx(rows, use_idx)
    hole = _unnamed(xrows, idx, d)
    sel = idx.long() if use_idx else torch.arange(rows)
    xh = rnd(xrows, d, seed=1, dtype=F32) if f32x else rnd(xrows, d, seed=1)
    w, dyh, dresh = (1 + 0.1 * rnd(d, seed=2).float()).to(BF), rnd(rows, d, seed=3), rnd(xrows, d, seed=4)
    xs = xh.float()[sel]
    rstd_h = torch.rsqrt(xs.pow(2).mean(-1) + eps)
    x, wd, dy = lay.inp("x", xh, inner=hole), lay.inp("w", w), lay.inp("dy", dyh)
    dres, rstd = lay.inp("dres", dresh, inner=hole), lay.inp("rstd", rstd_h)
    ix = lay.inp("row_idx", idx) if use_idx else None
    dx = lay.out("dx", (xrows, d), inner=hole)
    from rlaif_v_amd import hip
    nb = hip.lib().lib.rv_rmsnorm_bwd_nblocks(rows)
    part = lay.out("dw_partial", (nb * d,), F32)
    dw = lay.out("dw", (d,))
    fn = "rv_rmsnorm_bwd_f32x" if f32x else "rv_rmsnorm_bwd"
    call(fn, dy, ld(dy), x, ld(x), ix, wd, rstd, dres, ld(dres), dx, ld(dx), part, dw, 0, rows, d)
    lay.finish()
    dw1, dx1 = dw.clone(), dx.clone()
    call(fn, dy, ld(dy), x, ld(x), ix, wd, rstd, None, 0, dx, ld(dx), part, dw, 1, rows, d)
    lay.finish()
    xf = xs.to(lay.dev).requires_grad_(True)
    wf = w.float().to(lay.dev).requires_grad_(True)
    (wf * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps))).backward(dyh.float().to(lay.dev))
    close(dx1[sel.to(lay.dev)], xf.grad + dresh.float()[sel].to(lay.dev), rel=2e-2 if f32x else 1.6e-2, what="rmsnorm dx + dres")
    close(dx[sel.to(lay.dev)], xf.grad, rel=2e-2 if f32x else 1.6e-2, what="rmsnorm dx (second call, no dres)")
    close(dw1, wf.grad, rel=2e-2, what="rmsnorm dw")
    close(dw, 2 * wf.grad, rel=3e-2, what="rmsnorm dw accumulate")


@case(*grid(shape=NORM_SHAPES, f32in=[False, True]))
def c_layernorm_fwd(lay, shape, f32in):
    (rows, d), eps = shape, 1e-5
    xh = rnd(rows, d, seed=1, dtype=F32) * 1.5 + 0.3 if f32in else rnd(rows, d, seed=1)
    wh, bh = rnd(d, seed=2, scale=0.3) + 1, rnd(d, seed=3, scale=0.1)
    x, w, b = lay.inp("x", xh), lay.inp("w", wh), lay.inp("b", bh)
    y = lay.out("y", (rows, d))
    call("rv_layernorm_fwd_f32in" if f32in else "rv_layernorm_fwd", x, ld(x), w, b, y, ld(y), rows, d, eps)
    lay.finish()
    close(y, F.layer_norm(xh.float(), (d,), wh.float(), bh.float(), eps).to(lay.dev), rel=1e-2 if f32in else 1.6e-2, what="layernorm fwd")


@case(*grid(shape=NORM_SHAPES, period=[False, True], want_dx=[True, False]))
def c_layernorm_bwd(lay, shape, period, want_dx):
    """dw and db live next to each other in ONE buffer with a sentinel gap between them (the trainer's flat gradient buffer holds
    them adjacent); first call writes, second accumulates.  float64 reference, fp32 torch autograd as the yardstick."""
    (rows, d), eps = shape, 1e-5
    per = {3: 2, 333: 37}[rows] if period else 0
    xh = rnd(per if per else rows, d, seed=1)
    wh, dyh, dy2h = rnd(d, seed=2, scale=0.3) + 1, rnd(rows, d, seed=3), rnd(rows, d, seed=4, scale=0.5)
    x, w, dy, dy2 = lay.inp("x", xh), lay.inp("w", wh), lay.inp("dy", dyh), lay.inp("dy of the accumulating call", dy2h)
    dx = lay.out("dx", (rows, d)) if want_dx else None
    from rlaif_v_amd import hip
    nb = hip.lib().lib.rv_rmsnorm_bwd_nblocks(rows)
    part = lay.out("partial", (nb * 2 * d,), F32)
    gap = 64
    hole = torch.zeros(2 * d + gap, dtype=torch.bool)
    hole[d:d + gap] = True
    dwdb = lay.out("dw|db", (2 * d + gap,), inner=hole)
    dw, db = dwdb[:d], dwdb[d + gap:]
    tail = (x, ld(x), per, w, dx, ld(dx) if want_dx else 0, part, dw, db)
    call("rv_layernorm_bwd", dy, ld(dy), *tail, 0, rows, d, eps)
    lay.finish()
    dw1, db1, dx1 = dw.clone(), db.clone(), dx.clone() if want_dx else None
    call("rv_layernorm_bwd", dy2, ld(dy2), *tail, 1, rows, d, eps)          # another dy: the sum is not just twice the first result
    lay.finish()
    rowsel = torch.arange(rows) % per if per else torch.arange(rows)

    def grads(dt, dyv):
        xf = xh.to(dt)[rowsel].to(lay.dev).requires_grad_(True)
        wf = wh.to(dt).to(lay.dev).requires_grad_(True)
        bf = torch.zeros(d, dtype=dt, device=lay.dev, requires_grad=True)
        F.layer_norm(xf, (d,), wf, bf, eps).backward(dyv.to(dt).to(lay.dev))
        return xf.grad, wf.grad, bf.grad
    (dx64, dw64, db64), (dx32, dw32, db32) = grads(torch.float64, dyh), grads(F32, dyh)
    (dx64b, dw64b, db64b), (dx32b, dw32b, db32b) = grads(torch.float64, dy2h), grads(F32, dy2h)
    what = f"{rows}x{d} period {per}"
    if want_dx:
        yardstick(dx1, dx32.to(BF), dx64, f"layernorm_bwd dx {what}")
        yardstick(dx, dx32b.to(BF), dx64b, f"layernorm_bwd dx (second call) {what}")
    yardstick(dw1, dw32.to(BF), dw64, f"layernorm_bwd dw {what}")
    yardstick(db1, db32.to(BF), db64, f"layernorm_bwd db {what}")
    yardstick(dw, (dw1.float() + dw32b).to(BF), dw1.double() + dw64b, f"layernorm_bwd dw accumulate {what}")
    yardstick(db, (db1.float() + db32b).to(BF), db1.double() + db64b, f"layernorm_bwd db accumulate {what}")


@case(*grid(backward=[0, 1], use_pos=[False, True]))
def c_rope_inplace(lay, backward, use_pos):
    """q | k heads rotate in place; the v columns to their right hold the sentinel and must come back bit-unchanged"""
    n, L, H, hd = 70, 37, 2, 128
    rc = 2 * H * hd
    hole = torch.zeros(n, rc + H * hd, dtype=torch.bool)
    hole[:, rc:] = True
    xh = rnd(n, rc + H * hd, seed=1)
    x = lay.io("qkv", xh, inner=hole)
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=F32) / hd))
    fr = torch.arange(64, dtype=F32)[:, None] * inv[None]
    cos, sin = lay.inp("cos", fr.cos().reshape(-1)), lay.inp("sin", fr.sin().reshape(-1))      # contiguous [positions][64] tables
    posh = torch.randint(0, 64, (n,), generator=torch.Generator().manual_seed(0)).to(I32) if use_pos else None
    pos = lay.inp("pos", posh) if use_pos else None
    call("rv_rope_inplace", x, ld(x), cos, sin, pos, n, L, 2 * H, hd, backward)
    lay.finish()
    p = posh.long() if use_pos else torch.arange(n) % L
    c, s = torch.cat([fr[p], fr[p]], -1).cos()[:, None], torch.cat([fr[p], fr[p]], -1).sin()[:, None]
    xf = xh[:, :rc].float().view(n, 2 * H, hd)
    rot = torch.cat([-xf[..., hd // 2:], xf[..., :hd // 2]], -1)
    ref = xf * c + rot * (-s if backward else s)
    close(x[:, :rc], ref.view(n, rc).to(lay.dev), what="rope in place")


@case(*grid(interleaved=[0, 1], kind=["fwd", "bwd"]), ("dropout", dict(interleaved=0, kind="dropout")))
def c_swiglu(lay, interleaved, kind):
    rows, f = 77, 264
    guh, dah = rnd(rows, 2 * f, seed=1), rnd(rows, f, seed=2)
    gu = lay.inp("gu", guh)
    g32, u32 = (guh.float()[:, 0::2], guh.float()[:, 1::2]) if interleaved else (guh.float()[:, :f], guh.float()[:, f:])
    g32, u32 = g32.to(lay.dev), u32.to(lay.dev)
    if kind == "bwd":
        da = lay.inp("dact", dah)
        dgu = lay.out("dgu", (rows, 2 * f))
        call("rv_swiglu_bwd", da, ld(da), gu, ld(gu), dgu, ld(dgu), rows, f, interleaved)
        lay.finish()
        sg, daf = torch.sigmoid(g32), dah.float().to(lay.dev)
        dg, du = (dgu[:, 0::2], dgu[:, 1::2]) if interleaved else (dgu[:, :f], dgu[:, f:])
        close(dg, daf * u32 * sg * (1 + g32 * (1 - sg)), what="swiglu d gate")
        close(du, daf * g32 * sg, what="swiglu d up")
        return
    act = lay.out("act", (rows, f))
    if kind == "dropout":
        actd = lay.out("actd", (rows * f,))
        call("rv_swiglu_fwd_dropout", gu, ld(gu), act, ld(act), rows, f, actd, 0.3, 99)
    else:
        call("rv_swiglu_fwd", gu, ld(gu), act, ld(act), rows, f, interleaved)
    lay.finish()
    close(act, F.silu(g32) * u32, what="swiglu fwd")
    if kind == "dropout":
        from rlaif_v_amd import ops
        assert torch.equal(actd.view(rows, f), ops.dropout(act.contiguous(), 0.3, 99))


@case(("", {}))
def c_gelu(lay):
    n = 40 * 256
    xh, dyh = rnd(n, seed=3), rnd(n, seed=4)
    x, dy = lay.inp("x", xh), lay.inp("dy", dyh)
    y, dx = lay.out("y", (n,)), lay.out("dx", (n,))
    call("rv_gelu_fwd", x, y, n)
    call("rv_gelu_bwd", dy, x, dx, n)
    lay.finish()
    xf = xh.float().to(lay.dev).requires_grad_(True)
    r = F.gelu(xf)
    r.backward(dyh.float().to(lay.dev))
    close(y, r.detach(), what="gelu fwd")
    close(dx, xf.grad, what="gelu bwd")


@case(*grid(n=[8, 8008], mode=["y", "acc", "y+acc", "inplace"]))
def c_dropout(lay, n, mode):
    from oracle import dropout_mask as DM
    p, seed = 0.3, 4711
    xh, acch = rnd(n, seed=5), rnd(n, seed=6)
    x = lay.io("x", xh) if mode == "inplace" else lay.inp("x", xh)
    y = x if mode == "inplace" else (lay.out("y", (n,)) if "y" in mode else None)
    acc = lay.io("acc", acch) if "acc" in mode else None
    call("rv_dropout", x, y, acc, n, p, seed)
    lay.finish()
    mult = DM.multiplier(1, n, p, seed)[0]                       # the host restatement of the device's counter hash
    inv_keep = torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))
    dropped = torch.where(mult != 0, xh.float() * inv_keep, torch.zeros(n))
    if y is not None:
        assert torch.equal(y.cpu(), dropped.to(BF))
    if acc is not None:
        assert torch.equal(acc.cpu(), (acch.float() + dropped).to(BF))      # accumulates the unrounded fp32 value


@case(("", {}))
def c_add_f32_bf16(lay):
    n = 8008
    xh, bh = rnd(n, seed=7, dtype=F32) * 3, rnd(n, seed=8)
    x, b = lay.inp("x", xh), lay.inp("b", bh)
    out = lay.out("out", (n,), F32)
    call("rv_add_f32_bf16", x, b, out, n)
    lay.finish()
    assert torch.equal(out.cpu(), xh + bh.float())


@case(("", {}))
def c_add_rows(lay):
    period, reps, d = 5, 3, 40
    xh, ph = rnd(period * reps, d, seed=1), rnd(period, d, seed=2)
    x, p = lay.inp("x", xh), lay.inp("p", ph)
    y = lay.out("y", (period * reps, d))
    call("rv_add_rows", x, ld(x), p, ld(p), period, y, ld(y), period * reps, d)
    lay.finish()
    assert torch.equal(y.cpu(), (xh.float() + ph.float().repeat(reps, 1)).to(BF))


@case(("", {}))
def c_sum_rows_periodic(lay):
    period, reps, d = 5, 3, 40
    xh = rnd(period * reps, d, seed=3)
    x = lay.inp("x", xh)
    y = lay.out("y", (period, d))
    call("rv_sum_rows_periodic", x, ld(x), period, reps, y, ld(y), d)
    lay.finish()
    ref64 = xh.double().view(reps, period, d).sum(0)
    yard = xh.float().view(reps, period, d).sum(0).to(BF)
    yardstick(y.cpu(), yard, ref64, "sum_rows_periodic")


# =========================================================================================== data movement, casts
@case(("", {}))
def c_transpose(lay):
    """the header: out is [C][ldo >= roundup(R, 64)], columns [R, roundup(R, 64)) are written as zeros - and nothing beyond"""
    R, C = 100, 136
    xh = rnd(R, C, seed=1)
    x = lay.inp("in", xh)
    out = lay.out("out", (C, 128))
    call("rv_transpose", x, ld(x), out, ld(out), R, C)
    lay.finish()
    assert torch.equal(out[:, :R].cpu(), xh.t()) and not bool(out[:, R:].cpu().view(torch.int16).any())


@case(("", {}))
def c_splice_gather_colsum(lay):
    """the row movers (contiguous [rows][d] operands) and rv_colsum at M = 100, N = 72"""
    d, V, nfeat = 256, 50, 12
    eh, fh, dxh = rnd(V, d, seed=1), rnd(nfeat, d, seed=2), rnd(10, d, seed=3)
    srch = i32([3, 3, -2, -3, -13, -1, 49, 0, -1, 3])
    def unused(n, used):                              # rows no index names are poison too
        m = torch.ones(n, d, dtype=torch.bool)
        m[used] = False
        return m
    embed, feats = lay.inp("embed", eh.view(-1), inner=unused(V, [0, 3, 49]).view(-1)), lay.inp("feats", fh.view(-1), inner=unused(nfeat, [0, 1, 11]).view(-1))
    dxc = lay.inp("dx", dxh.view(-1))
    src = lay.inp("src", srch)
    out = lay.out("splice out", (10 * d,))
    call("rv_splice_fwd", src, embed, feats, out, 10, d)
    # embedding backward: rows {0: [7], 3: [0, 1, 9], 49: [6]}; only the rows uniq_ids names are written
    uniq, seg, pos = lay.inp("uniq", i32([0, 3, 49])), lay.inp("seg_off", i32([0, 1, 4, 5])), lay.inp("pos", i32([7, 0, 1, 9, 6]))
    dW = lay.out("dW", (V * d,), inner=unused(V, [0, 3, 49]).view(-1))
    call("rv_embed_bwd", uniq, seg, pos, 3, dxc, dW, d)
    a, b = lay.inp("src_a", i32([2, -1, 4])), lay.inp("src_b", i32([3, -1, -1]))
    fg = lay.out("dfeat", (3 * d,))
    call("rv_feat_grad", a, b, dxc, fg, 3, d)
    # gather / scatter with ld > d on both sides; scatter writes only the rows idx names
    idxh = i32([9, 0, 4])
    dx2 = lay.inp("dx 2-D", dxh, inner=unused(10, idxh.long()))
    idx = lay.inp("idx", idxh)
    gth = lay.out("gathered", (3, d))
    call("rv_gather_rows", dx2, ld(dx2), idx, gth, ld(gth), 3, d, 0)
    sc = lay.out("scattered", (10, d), inner=unused(10, idxh.long()))
    call("rv_gather_rows", gth, ld(gth), idx, sc, ld(sc), 3, d, 1)
    M, N = 100, 72
    dyh = rnd(M, N, seed=9)
    dy = lay.inp("dy", dyh)
    db = lay.out("db", (N,))
    call("rv_colsum", dy, ld(dy), db, M, N)
    lay.finish()
    o = out.view(10, d).cpu()
    for i, s in enumerate(srch.tolist()):
        exp = eh[s] if s >= 0 else (torch.zeros(d, dtype=BF) if s == -1 else fh[-2 - s])
        assert torch.equal(o[i], exp), f"splice row {i}"
    ref = torch.zeros(V, d)
    ref.index_add_(0, torch.tensor([3, 3, 49, 0, 3]), dxh[[0, 1, 6, 7, 9]].float())
    close(dW.view(V, d)[[0, 3, 49]].cpu(), ref[[0, 3, 49]], rel=1e-2, what="embed bwd")
    f = fg.view(3, d).cpu()
    close(f[0], dxh[2].float() + dxh[3].float(), rel=1e-2, what="feat grad")
    assert f[1].abs().sum() == 0 and torch.equal(f[2], dxh[4])
    assert torch.equal(gth.cpu(), dxh[idxh.long()]) and torch.equal(sc.cpu()[idxh.long()], dxh[idxh.long()])
    close(db.cpu(), dyh.float().sum(0), rel=1e-2, what="colsum")


@case(("", {}))
def c_clip_front_end(lay):
    B, HW, ps, cd = 2, 56, 14, 128
    Kp, P = 640, 16
    pxh = torch.randn(B, 3, HW, HW, generator=torch.Generator().manual_seed(0))
    px = lay.inp("pixels", pxh.view(-1))
    cols = lay.out("patches", (B * P * Kp,))
    call("rv_im2col_patches", px, cols, B, HW, ps, Kp)
    peh, clsh, posh = rnd(B * P, cd, seed=1), rnd(cd, seed=2), rnd(P + 1, cd, seed=3)
    pe, cls, pos = lay.inp("patch emb", peh.view(-1)), lay.inp("cls", clsh), lay.inp("pos", posh.view(-1))
    x = lay.out("x", (B * (P + 1) * cd,))
    call("rv_clip_assemble", pe, cls, pos, x, B, P, cd)
    lay.finish()
    ref = F.unfold(pxh.to(BF).float(), ps, stride=ps).transpose(1, 2).reshape(B * P, 3 * ps * ps)
    c = cols.view(B * P, Kp).cpu()
    assert torch.equal(c[:, :588].float(), ref) and c[:, 588:].abs().sum() == 0
    refx = torch.cat([clsh.float().expand(B, 1, cd), peh.float().view(B, P, cd)], 1) + posh.float()[None]
    close(x.view(B * (P + 1), cd).cpu(), refx.reshape(B * (P + 1), cd), rel=1e-2, what="clip assemble")


def _special_f32():
    """±0, ±Inf, denormals, ties both ways (round to nearest even), the largest finite fp32, values that round up to Inf"""
    bits = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001,
            0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x00008000, 0x00018000]
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(F32)


@case(*grid(n=[8, 8008]))
def c_cast(lay, n):
    sp = _special_f32()
    xh = rnd(n, seed=n, dtype=F32) * 100
    k = min(n, sp.numel())
    xh[:k] = sp[:k]
    x = lay.inp("f32 in", xh)
    y = lay.out("bf16 out", (n,))
    call("rv_cast_f32_to_bf16", x, y, n)
    bh = xh.to(BF)
    b = lay.inp("bf16 in", bh)
    z = lay.out("f32 out", (n,), F32)
    call("rv_cast_bf16_to_f32", b, z, n)
    lay.finish()
    assert torch.equal(y.cpu().view(torch.int16), bh.view(torch.int16)), "f32 -> bf16 differs from torch's round-to-nearest-even"
    assert torch.equal(z.cpu().view(torch.int32), bh.float().view(torch.int32))


def test_cast_nan_gives_nan():
    """a NaN input gives a NaN (its payload is not pinned); kept apart from the table, whose outputs must be NaN-free"""
    dev = _dev()
    x, cx = G.guarded_1d(8, F32, dev, fill=torch.tensor([float("nan"), 1.0, -float("nan"), 2.0, 0, 0, 0, 0]))
    y, cy = G.guarded_1d(8, BF, dev)
    call("rv_cast_f32_to_bf16", x, y, 8)
    torch.cuda.synchronize()
    cx(), cy(written=True)
    assert torch.isnan(y).tolist() == [True, False, True, False, False, False, False, False]
    assert y[1].item() == 1.0 and y[3].item() == 2.0


# =========================================================================================== optimizer
OPT_N = [8, 8 * 1000 + 8]


@case(*grid(n=OPT_N, max_norm=[1.0, 0.0]))
def c_grad_norm_and_sumsq(lay, n, max_norm):
    """rv_grad_norm with pre_scale = 0.125; rv_grad_sumsq accumulate 0 then 1; rv_clip_from_sumsq == rv_grad_norm's out2 bit for bit"""
    from rlaif_v_amd import hip
    nbk = hip.lib().lib.rv_sumsq_nblocks()
    gh, g2h = rnd(n, seed=n, scale=3.0), rnd(n, seed=n + 1, scale=2.0)
    g, g2 = lay.inp("g", gh), lay.inp("g2", g2h)
    part = lay.out("partial", (nbk,), F32)
    out2 = lay.out("out2", (2,), F32)
    call("rv_grad_norm", g, n, part, max_norm, 0.125, out2)
    s_a, s_b, s_ab = lay.out("sumsq a", (1,), F32), lay.out("sumsq b", (1,), F32), lay.out("sumsq a+b", (1,), F32)
    call("rv_grad_sumsq", g, n, part, s_a, 0)
    call("rv_grad_sumsq", g2, n, part, s_b, 0)
    call("rv_grad_sumsq", g, n, part, s_ab, 0)
    call("rv_grad_sumsq", g2, n, part, s_ab, 1)
    clip2 = lay.out("clip out2", (2,), F32)
    call("rv_clip_from_sumsq", s_a, max_norm, 0.125, clip2)
    lay.finish()
    nrm = gh.float().norm().to(lay.dev) * 0.125
    torch.testing.assert_close(out2[0], nrm, rtol=1e-4, atol=1e-4)
    want = 0.125 * torch.clamp(max_norm / (nrm + 1e-6), max=1.0) if max_norm > 0 else torch.tensor(0.125, device=lay.dev)
    torch.testing.assert_close(out2[1], want, rtol=1e-4, atol=1e-6)
    assert torch.equal(clip2.view(I32), out2.view(I32)), "rv_clip_from_sumsq differs from rv_grad_norm on the same data"
    assert torch.equal(s_ab, s_a + s_b), "accumulate differs from the fp32 sum of the two plain results"
    ref64 = gh.double().pow(2).sum().view(1)
    yardstick(s_a.cpu(), gh.float().pow(2).sum().view(1), ref64, f"grad_sumsq n={n}")


@case(*grid(n=OPT_N))
def c_grad_accum(lay, n):
    g1h, g2h, g3h = rnd(n, seed=1), rnd(n, seed=2), rnd(n, seed=3)
    acc = lay.out("acc", (n,), F32)
    g1, g2 = lay.inp("g1", g1h), lay.inp("g2", g2h)
    g3 = lay.io("g3", g3h)
    call("rv_grad_accum", acc, g1, n, 0, 1.0)
    lay.finish()
    assert torch.equal(acc.cpu(), g1h.float())
    call("rv_grad_accum", acc, g2, n, 1, 1.0)
    lay.finish()
    s = g1h.float() + g2h.float()
    assert torch.equal(acc.cpu(), s)
    call("rv_grad_accum", acc, g3, n, 2, 1.0 / 3.0)
    lay.finish()
    scale = torch.tensor(1.0 / 3.0, dtype=F32)
    assert torch.equal(g3.cpu(), ((s + g3h.float()) * scale).to(BF)) and torch.equal(acc.cpu(), s)


def _f32(x):
    """the value the C ABI's `float` parameter carries"""
    return float(torch.tensor(x, dtype=F32))


def _torch_adamw(master, m, v, g, lr, b1, b2, eps, wd, step, gs, dt):
    """step number `step` of torch.optim.AdamW in dtype dt from the given state, on the hyper-parameters as the ABI rounds them"""
    prm = torch.nn.Parameter(master.to(dt))
    opt = torch.optim.AdamW([prm], lr=_f32(lr), betas=(_f32(b1), _f32(b2)), eps=_f32(eps), weight_decay=_f32(wd))
    opt.state[prm] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.to(dt), "exp_avg_sq": v.to(dt)}
    prm.grad = g.to(dt) * _f32(gs)
    opt.step()
    return prm.detach(), opt.state[prm]["exp_avg"], opt.state[prm]["exp_avg_sq"]


@case(*grid(n=OPT_N, use_clip=[True, False], wd=[0.0, 0.01]))
def c_adamw(lay, n, use_clip, wd):
    """steps 1..3 against torch.optim.AdamW (the bound of test_adamw_and_gradnorm), then step 1000 from that state against float64"""
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    gen = torch.Generator().manual_seed(n)
    mh = torch.randn(n, generator=gen)
    master, p = lay.io("master", mh), lay.io("p", mh.to(BF))
    m, v = lay.io("m", torch.zeros(n)), lay.io("v", torch.zeros(n))
    grads = [(torch.randn(n, generator=gen) * 3).to(BF) for _ in range(4)]
    g = lay.io("g", grads[0])                       # refilled between steps by the test; the kernel only reads it
    cliph = torch.tensor([5.0, 0.37])
    clip = lay.inp("clip", cliph) if use_clip else None
    gs = 0.37 if use_clip else 1.0
    ref = torch.nn.Parameter(mh.clone().to(lay.dev))
    opt = torch.optim.AdamW([ref], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for step in range(1, 4):
        g.copy_(grads[step - 1])
        before = g.clone()
        call("rv_adamw_step", p, master, m, v, g, n, lr, b1, b2, eps, wd, step, clip)
        lay.finish()
        assert torch.equal(g, before), "rv_adamw_step changed the gradient"
        ref.grad = grads[step - 1].float().to(lay.dev) * gs
        opt.step()
        torch.testing.assert_close(master, ref.detach(), rtol=2e-5, atol=2e-6)
        assert torch.equal(p, master.to(BF))
    g.copy_(grads[3])
    st = [t.clone().cpu() for t in (master, m, v)]
    call("rv_adamw_step", p, master, m, v, g, n, lr, b1, b2, eps, wd, 1000, clip)
    lay.finish()
    w64, m64, v64 = _torch_adamw(*st, grads[3], lr, b1, b2, eps, wd, 1000, gs, torch.float64)
    w32, m32, v32 = _torch_adamw(*st, grads[3], lr, b1, b2, eps, wd, 1000, gs, F32)
    yardstick(master.cpu(), w32, w64, f"adamw step 1000 master n={n}")
    yardstick(m.cpu(), m32, m64, f"adamw step 1000 m n={n}")
    yardstick(v.cpu(), v32, v64, f"adamw step 1000 v n={n}")
    assert torch.equal(p, master.to(BF))


@case(("", {}))
def c_reduce_copy_persistent(lay):
    n, n_wg = 8008, 4
    ah, bh = rnd(n, seed=1), rnd(n, seed=2)
    a, b = lay.inp("a", ah), lay.inp("b", bh)
    dst = lay.out("dst", (n,))
    call("rv_reduce_copy_persistent", a, b, dst, n, n_wg)
    lay.finish()
    assert torch.equal(dst.cpu(), (ah.float() + bh.float()).to(BF))


# =========================================================================================== GEMM family
def dv(t, lay):
    return t.to(lay.dev)


def mm(a, b, lay, dt=F32):
    """a @ b on the device in dtype dt (the reference of every GEMM case: the same bf16-rounded operands)"""
    return dv(a, lay).to(dt) @ dv(b, lay).to(dt)


def _act(z, act):
    return z * torch.sigmoid(1.702 * z) if act == 1 else (F.gelu(z) if act == 2 else z)


@case(*grid(variant=[0, 1, 2, 3], shape=[(200, 132, 192), (7, 4, 64)]))
def c_gemm_nt(lay, variant, shape):
    M, N, K = shape
    ah, bh = rnd(M, K, seed=1), rnd(N, K, seed=2)
    a, b = lay.inp("A", ah), lay.inp("B", bh)
    c = lay.out("C", (M, N))
    call("rv_gemm_nt_bf16", a, ld(a), b, ld(b), c, ld(c), M, N, K, None, None, 0, 0, 1.0, variant)
    lay.finish()
    close(c, mm(ah, bh.t(), lay), what=f"gemm_nt v{variant} {M}x{N}x{K}")


@case(*grid(variant=[0, 1, 2, 3], act=[0, 1, 2]))
def c_gemm_nt_epilogue(lay, variant, act):
    """bias + residual + activation, the residual being C itself"""
    M, N, K = 300, 256, 320
    ah, bh = rnd(M, K, seed=3, scale=0.5), rnd(N, K, seed=4, scale=0.5)
    biash, resh = rnd(N, seed=5), rnd(M, N, seed=6)
    a, b, bias = lay.inp("A", ah), lay.inp("B", bh), lay.inp("bias", biash)
    c = lay.io("C = residual", resh)
    call("rv_gemm_nt_bf16", a, ld(a), b, ld(b), c, ld(c), M, N, K, bias, c, ld(c), act, 0.5, variant)
    lay.finish()
    z = 0.5 * mm(ah, bh.t(), lay) + dv(biash, lay).float()
    close(c, _act(z, act) + dv(resh, lay).float(), what=f"gemm_nt epilogue act={act} v{variant}")


@case(("", {}))
def c_gemm_nt_skinny(lay):
    """>= 4096 rows, <= 256 columns, plain store: the streaming kernel; bit for bit the 128x128 kernel's result"""
    M, N, K = 4100, 64, 128
    ah, bh = rnd(M, K, seed=5), rnd(N, K, seed=6, scale=0.1)
    a, b = lay.inp("A", ah), lay.inp("B", bh)
    c, c1 = lay.out("C", (M, N)), lay.out("C variant 1", (M, N))
    call("rv_gemm_nt_bf16", a, ld(a), b, ld(b), c, ld(c), M, N, K, None, None, 0, 0, 0.25, -1)
    call("rv_gemm_nt_bf16", a, ld(a), b, ld(b), c1, ld(c1), M, N, K, None, None, 0, 0, 0.25, 1)
    lay.finish()
    close(c, 0.25 * mm(ah, bh.t(), lay), what="gemm_nt skinny")
    assert torch.equal(c, c1)


@case(*grid(kind=["f32out", "f32res", "f32res-nobias"], variant=[-1, 0, 1, 2]))
def c_gemm_nt_f32(lay, kind, variant):
    M, N, K = 300, 256, 128
    ah, wh, biash = rnd(M, K, seed=1, scale=0.5), rnd(N, K, seed=2, scale=0.05), rnd(N, seed=3)
    xh = rnd(M, N, seed=4, dtype=F32) * 3.0
    a, w = lay.inp("A", ah), lay.inp("B", wh)
    if kind == "f32out":
        c = lay.out("C", (M, N), F32)
        call("rv_gemm_nt_bf16_f32out", a, ld(a), w, ld(w), c, ld(c), M, N, K, variant)
        lay.finish()
        torch.testing.assert_close(c, mm(ah, wh.t(), lay), rtol=1e-4, atol=1e-3)
        return
    bias = lay.inp("bias", biash) if kind == "f32res" else None
    c = lay.io("C = residual", xh)
    call("rv_gemm_nt_bf16_f32res", a, ld(a), w, ld(w), c, ld(c), M, N, K, bias, c, ld(c), variant)
    lay.finish()
    ref = dv(xh, lay) + mm(ah, wh.t(), lay) + (dv(biash, lay).float() if bias is not None else 0)
    torch.testing.assert_close(c, ref, rtol=1e-4, atol=2e-3)


@case(*grid(alias=[False, True]))
def c_gemm_nt_dropout(lay, alias):
    from rlaif_v_amd import ops
    M, N, K, p, seed = 300, 264, 128, 0.3, 12345
    ah, bh, resh = rnd(M, K, seed=1), rnd(N, K, seed=2), rnd(M, N, seed=3)
    a, b = lay.inp("A", ah), lay.inp("B", bh)
    c = lay.io("C = residual", resh) if alias else lay.out("C", (M, N))
    call("rv_gemm_nt_dropout_bf16", a, ld(a), b, ld(b), c, ld(c), M, N, K, c if alias else None, ld(c) if alias else 0, 0.5, p, seed)
    lay.finish()
    mask = ops.dropout(torch.ones(M, N, dtype=BF, device=lay.dev), p, seed) != 0
    ref = 0.5 * mm(ah, bh.t(), lay) * mask / (1 - p)
    if alias:
        ref = ref + dv(resh, lay).float()
    else:
        assert torch.equal(c != 0, mask & (ops.gemm_nt(dv(ah, lay), dv(bh, lay), alpha=0.5) != 0))
    assert (c.float() - ref).abs().max() <= 1.6e-2 * ref.abs().max()


@case(*grid(kind=["plain", "residual", "bias_act"]))
def c_gemm_nn(lay, kind):
    M, N, K = 300, 264, 96
    ah, bh, resh, biash = rnd(M, K, seed=51), rnd(K, N, seed=52, scale=0.3), rnd(M, N, seed=53), rnd(N, seed=54, scale=0.5)
    a, b = lay.inp("A", ah), lay.inp("B", bh)
    c = lay.out("C", (M, N))
    if kind == "plain":
        call("rv_gemm_nn_bf16", a, ld(a), b, ld(b), c, ld(c), M, N, K, None, 0, 1.0)
        ref = mm(ah, bh, lay)
    elif kind == "residual":
        res = lay.inp("residual", resh)
        call("rv_gemm_nn_bf16", a, ld(a), b, ld(b), c, ld(c), M, N, K, res, ld(res), 0.5)
        ref = 0.5 * mm(ah, bh, lay) + dv(resh, lay).float()
    else:
        res, bias = lay.inp("residual", resh), lay.inp("bias", biash)
        call("rv_gemm_nn_bias_act_bf16", a, ld(a), b, ld(b), c, ld(c), M, N, K, bias, res, ld(res), 1, 1.0)
        ref = _act(mm(ah, bh, lay) + dv(biash, lay).float(), 1) + dv(resh, lay).float()
    lay.finish()
    close(c, ref, what=f"gemm_nn {kind}")


@case(*grid(use_pos=[True, False]))
def c_gemm_nn_rope(lay, use_pos):
    from rlaif_v_amd import ops
    M, d, kvd, hd, L = 300, 1024, 1024, 128, 977
    H, Hkv = d // hd, kvd // hd
    N, rope_cols = d + 2 * kvd, d + kvd
    xh, wh = rnd(M, d, seed=81), rnd(d, N, seed=82, scale=0.06)
    cos_d, sin_d = ops.rope_tables(2048, hd, 10000.0, lay.dev)
    posh = (torch.arange(M, dtype=I32) * 7 % 1500).contiguous()
    x, w = lay.inp("A", xh), lay.inp("B", wh)
    cos, sin = lay.inp("cos", cos_d.reshape(-1)), lay.inp("sin", sin_d.reshape(-1))
    pos = lay.inp("pos", posh) if use_pos else None
    c = lay.out("C", (M, N))
    call("rv_gemm_nn_rope_bf16", x, ld(x), w, ld(w), c, ld(c), M, N, d, cos, sin, pos, L, rope_cols, hd)
    lay.finish()
    plain = ops.gemm_nn(dv(xh, lay), dv(wh, lay))
    assert torch.equal(c[:, rope_cols:], plain[:, rope_cols:])
    unfused = ops.rope_inplace(plain.clone(), cos_d, sin_d, L, H + Hkv, hd, pos=dv(posh, lay) if use_pos else None)
    close(c, unfused, rel=1.6e-2, what="fused rope vs gemm + rope_inplace")
    y = mm(xh, wh, lay, torch.float64)
    pp = dv(posh, lay).long() if use_pos else torch.arange(M, device=lay.dev) % L
    cc, ss = cos_d[pp].double(), sin_d[pp].double()
    yr = y[:, :rope_cols].reshape(M, H + Hkv, 2, 64)
    x1, x2 = yr[:, :, 0], yr[:, :, 1]
    ex = torch.stack([x1 * cc[:, None] - x2 * ss[:, None], x2 * cc[:, None] + x1 * ss[:, None]], 2).reshape(M, rope_cols)
    close(c[:, :rope_cols], ex.float(), rel=8e-3, what="fused rope vs exact")


@case(*grid(kind=["fwd", "bwd"]))
def c_gemm_nn_swiglu(lay, kind):
    from rlaif_v_amd import ops
    M, d, f = 300, 256, 512
    xh, wguh = rnd(M, d, seed=71), rnd(d, 2 * f, seed=72, scale=0.08)
    gu_ref = ops.gemm_nn(dv(xh, lay), dv(wguh, lay))
    g32, u32 = gu_ref.float()[:, 0::2], gu_ref.float()[:, 1::2]
    if kind == "fwd":
        x, w = lay.inp("A", xh), lay.inp("B", wguh)
        gu, act = lay.out("GU", (M, 2 * f)), lay.out("ACT", (M, f))
        call("rv_gemm_nn_swiglu_bf16", x, ld(x), w, ld(w), gu, ld(gu), act, ld(act), M, 2 * f, d)
        lay.finish()
        assert torch.equal(gu, gu_ref)
        close(act, F.silu(g32) * u32, what="fused swiglu act")
        gu_f = mm(xh, wguh, lay, torch.float64)
        close(act, (F.silu(gu_f[:, 0::2]) * gu_f[:, 1::2]).float(), rel=6e-3, what="fused swiglu act vs exact")
        return
    dyh, wdh = rnd(M, d, seed=73, scale=0.5), rnd(d, f, seed=74, scale=0.08)
    dy, wd, gu = lay.inp("A", dyh), lay.inp("B", wdh), lay.inp("GU", gu_ref.cpu())
    dgu = lay.out("DGU", (M, 2 * f))
    call("rv_gemm_nn_swiglu_bwd_bf16", dy, ld(dy), wd, ld(wd), gu, ld(gu), dgu, ld(dgu), M, f, d)
    lay.finish()
    dact = ops.gemm_nn(dv(dyh, lay), dv(wdh, lay))
    assert torch.equal(dgu, ops.swiglu_bwd(dact, gu_ref, interleaved=True))
    da, sg = dact.float(), torch.sigmoid(g32)
    close(dgu[:, 0::2], da * u32 * sg * (1 + g32 * (1 - sg)), what="fused swiglu d gate")
    close(dgu[:, 1::2], da * g32 * sg, what="fused swiglu d up")


# the smallest shape ops.linear_lora_swiglu_ok accepts that still has a ragged second row tile: 2 x 96 tiles of 256 x 256
LSW = dict(M=257, f=12168, d=512, rp=64)


@case(*grid(p=[0.0, 0.3]))
def c_gemm_nn_lora_swiglu(lay, p):
    """forward (GU, ACT, ACTD) and backward (DGU) of the fused adapter SwiGLU GEMMs"""
    from rlaif_v_amd import ops
    M, f, d, rp, seed = LSW["M"], LSW["f"], LSW["d"], LSW["rp"], 12345
    assert ops.linear_lora_swiglu_ok(M, f, d, rp) and not ops.linear_lora_swiglu_ok(M - 1, f, d, rp) \
        and not ops.linear_lora_swiglu_ok(M, f - 8, d, rp) and not ops.linear_lora_swiglu_ok(M, f, d - 64, rp)
    xh, wguh, th = rnd(M, d, seed=91), rnd(d, 2 * f, seed=92, scale=0.06), rnd(M, 2 * rp, seed=93, scale=0.5)
    bexph = torch.zeros(2 * rp, 2 * f, dtype=BF)
    bexph[:rp, 0::2] = rnd(rp, f, seed=94, scale=0.1)
    bexph[rp:, 1::2] = rnd(rp, f, seed=95, scale=0.1)
    x, w, t, bexp = lay.inp("A", xh), lay.inp("B", wguh), lay.inp("A2", th), lay.inp("B2", bexph)
    gu = lay.out("GU", (M, 2 * f))
    if p > 0:                                  # ACTD needs a contiguous ACT (ldact == N / 2)
        act, actd, ldact = lay.out("ACT", (M * f,)), lay.out("ACTD", (M * f,)), f
    else:
        act, actd = lay.out("ACT", (M, f)), None
        ldact = ld(act)
    call("rv_gemm_nn_lora_swiglu_bf16", x, ld(x), w, ld(w), t, ld(t), bexp, ld(bexp), 2 * rp, gu, ld(gu), act, ldact, actd, p, seed,
         M, 2 * f, d)
    dyh, wdh = rnd(M, d, seed=96, scale=0.5), rnd(d, f, seed=97, scale=0.06)
    dth, adh = rnd(M, rp, seed=98, scale=0.5), rnd(rp, f, seed=99, scale=0.1)
    dy, wd, dt, ad = lay.inp("bwd A", dyh), lay.inp("bwd B", wdh), lay.inp("bwd A2", dth), lay.inp("bwd B2", adh)
    dgu = lay.out("DGU", (M, 2 * f))
    call("rv_gemm_nn_lora_swiglu_bwd_bf16", dy, ld(dy), wd, ld(wd), dt, ld(dt), ad, ld(ad), rp, p, seed, gu, ld(gu), dgu, ld(dgu),
         M, f, d)
    lay.finish()
    act2 = act.view(M, f)
    exact_gu = mm(xh, wguh, lay, torch.float64) + mm(th, bexph, lay, torch.float64)
    close(gu, exact_gu.float(), rel=6e-3, what="lora swiglu gate|up")
    close(act2, (F.silu(exact_gu[:, 0::2]) * exact_gu[:, 1::2]).float(), rel=6e-3, what="lora swiglu act")
    adm = mm(dth, adh, lay, torch.float64)
    if p > 0:
        assert torch.equal(actd.view(M, f), ops.dropout(act2.contiguous(), p, seed))
        adm = adm * (ops.dropout(torch.ones(M, f, dtype=BF, device=lay.dev), p, seed) != 0).double() / (1 - p)
    dact = (mm(dyh, wdh, lay, torch.float64) + adm).float().bfloat16()
    guc = gu.contiguous()
    close(dgu, ops.swiglu_bwd(dact, guc, interleaved=True).float(), rel=1.6e-2, what="lora swiglu d(gate|up)")
    g32, u32, da = guc.float()[:, 0::2], guc.float()[:, 1::2], dact.float()
    sg = torch.sigmoid(g32)
    close(dgu[:, 0::2], da * u32 * sg * (1 + g32 * (1 - sg)), rel=1.6e-2, what="lora swiglu d gate")
    close(dgu[:, 1::2], da * g32 * sg, rel=1.6e-2, what="lora swiglu d up")


def _lora_ref(lay, ah, bTh, a2h, b2Th, gc, resh=None, mult=None):
    """a @ bT + sum over column groups of a2_g @ b2T[:, group] (* mult) (+ res), fp32 on the device; bT [K][N], b2T [K2][N]"""
    N, K2 = bTh.shape[1], b2Th.shape[0]
    ref = mm(ah, bTh, lay)
    lo = torch.zeros_like(ref)
    for g in range(N // gc if gc else 1):
        cols = slice(g * gc, (g + 1) * gc) if gc else slice(0, N)
        lo[:, cols] = mm(a2h[:, g * K2:(g + 1) * K2], b2Th[:, cols], lay)
    ref = ref + (lo * mult if mult is not None else lo)
    return ref + dv(resh, lay).float() if resh is not None else ref


@case(*grid(shape=[(130, 256, 128, 128, 0), (300, 768, 256, 64, 256)], residual=[False, True]))
def c_gemm_nt_lora(lay, shape, residual):
    M, N, K, K2, gc = shape
    groups = N // gc if gc else 1
    ah, bh = rnd(M, K, seed=31), rnd(N, K, seed=32)
    a2h, b2h, resh = rnd(M, groups * K2, seed=33), rnd(N, K2, seed=34), rnd(M, N, seed=35)
    a, b, a2, b2 = lay.inp("A", ah), lay.inp("B", bh), lay.inp("A2", a2h), lay.inp("B2", b2h)
    res = lay.inp("residual", resh) if residual else None
    c = lay.out("C", (M, N))
    call("rv_gemm_nt_lora_bf16", a, ld(a), b, ld(b), a2, ld(a2), b2, ld(b2), K2, gc, 0, c, ld(c), M, N, K, res, ld(res) if residual else 0)
    lay.finish()
    close(c, _lora_ref(lay, ah, bh.t(), a2h, b2h.t(), gc, resh if residual else None), what=f"gemm_nt_lora {shape}")


@case(*grid(kind=["nn_lora", "pre p=0", "pre p=0.3"]))
def c_gemm_nn_lora(lay, kind):
    """the NN forms; K raised to rv_gemm_nn_lora_pre_bf16's documented minimum of 512 for that entry point"""
    from rlaif_v_amd import ops
    M, N, K2, gc = 300, 512, 64, 256
    K = 128 if kind == "nn_lora" else 512
    groups = N // gc
    ah, bh = rnd(M, K, seed=61), rnd(K, N, seed=62, scale=0.05)
    a2h, b2h, resh = rnd(M, groups * K2, seed=63), rnd(K2, N, seed=64, scale=0.2), rnd(M, N, seed=65)
    a, b, a2, b2, res = lay.inp("A", ah), lay.inp("B", bh), lay.inp("A2", a2h), lay.inp("B2", b2h), lay.inp("residual", resh)
    c = lay.out("C", (M, N))
    if kind == "nn_lora":
        call("rv_gemm_nn_lora_bf16", a, ld(a), b, ld(b), a2, ld(a2), b2, ld(b2), K2, gc, 0, c, ld(c), M, N, K, res, ld(res))
        lay.finish()
        close(c, _lora_ref(lay, ah, bh, a2h, b2h, gc, resh), what="gemm_nn_lora")
        nt = ops.gemm_nt_lora(dv(ah, lay), dv(bh.t().contiguous(), lay), dv(a2h, lay), dv(b2h.t().contiguous(), lay), group_cols=gc,
                              residual=dv(resh, lay))
        close(c, nt, rel=4e-3, what="gemm_nn_lora vs nt_lora (different tile kernels)")
        return
    p, seed = (0.3, 4711) if kind.endswith("0.3") else (0.0, 0)
    call("rv_gemm_nn_lora_pre_bf16", a, ld(a), b, ld(b), a2, ld(a2), b2, ld(b2), K2, gc, 0, p, seed, c, ld(c), M, N, K, res, ld(res))
    lay.finish()
    mult = (ops.dropout(torch.ones(M, N, dtype=BF, device=lay.dev), p, seed) != 0).float() / (1 - p) if p > 0 else None
    ref = _lora_ref(lay, ah, bh, a2h, b2h, gc, resh, mult)
    e = ((c.float() - ref).abs().max() / ref.abs().max()).item()
    assert e <= 6e-3, f"gemm_nn_lora_pre {kind}: max err {e:.3e} of the largest value"


@case(*grid(shape=[(100, 136, 520), (7, 8, 8)], residual=[False, True]))
def c_gemm_tn(lay, shape, residual):
    R, I, J = shape
    ph, qh, resh = rnd(R, I, seed=21, scale=0.5), rnd(R, J, seed=22, scale=0.5), rnd(I, J, seed=23)
    p, q = lay.inp("P", ph), lay.inp("Q", qh)
    res = lay.inp("residual", resh) if residual else None
    c = lay.out("C", (I, J))
    call("rv_gemm_tn_bf16", p, ld(p), q, ld(q), c, ld(c), R, I, J, res, ld(res) if residual else 0, 0.5 if residual else 1.0)
    lay.finish()
    ref = mm(ph.t(), qh, lay)
    close(c, 0.5 * ref + dv(resh, lay).float() if residual else ref, what=f"gemm_tn {shape}")


@case(("", {}))
def c_gemm_tn_splitk(lay):
    R, I, J, splits = 777, 64, 64, 7
    ph, qh = rnd(R, I, seed=41, scale=0.3), rnd(R, J, seed=42, scale=0.3)
    p, q = lay.inp("P", ph), lay.inp("Q", qh)
    c, ws = lay.out("C", (I, J)), lay.out("workspace", (splits * I * J,), F32)
    call("rv_gemm_tn_bf16_splitk", p, ld(p), q, ld(q), c, ld(c), R, I, J, 0.25, splits, ws)
    lay.finish()
    close(c, 0.25 * mm(ph.t(), qh, lay), what="gemm_tn_splitk")


def _smallest_tail_split_shape():
    """(R, I, J, workspace floats): the smallest operand footprint R (I + J) + I J for which the library plans a tail split,
    found by asking rv_gemm_tn_workspace_floats; ragged last tiles (8 columns) on both output axes"""
    from rlaif_v_amd import hip
    fn = hip.lib().lib.rv_gemm_tn_workspace_floats
    best = None
    for R in (4096, 4128):
        for ti in range(1, 40):
            for tj in range(ti, 300):
                I, J = (ti - 1) * 256 + 8, (tj - 1) * 256 + 8
                cost = R * (I + J) + I * J
                if best is not None and cost >= best[0]:
                    break
                need = fn(R, I, J)
                if need > 0:
                    best = (cost, R, I, J, need)
                    break
    assert best is not None, "no shape below 40 x 300 tiles plans a tail split"
    return best[1:]


@case(("", {}))
def c_gemm_tn_ws(lay):
    R, I, J, need = _smallest_tail_split_shape()
    g = torch.Generator(device=lay.dev).manual_seed(1)
    pd_ = (torch.randn(R, I, device=lay.dev, generator=g) * 0.5).to(BF)
    qd_ = (torch.randn(R, J, device=lay.dev, generator=g) * 0.5).to(BF)
    p, q = lay.inp("P", pd_), lay.inp("Q", qd_)
    c, ws = lay.out("C", (I, J)), lay.out("workspace", (need,), F32)
    call("rv_gemm_tn_bf16_ws", p, ld(p), q, ld(q), c, ld(c), R, I, J, ws, need)
    lay.finish()
    close(c, pd_.float().t() @ qd_.float(), what=f"gemm_tn tail split {R}x{I}x{J}")


MASK_SEEDS = (1234567, 89, 2147480000)


@case(*grid(G=[1, 3], kind=["down", "dgrad", "wgrad"]))
def c_lora_masks(lay, G, kind):
    """the three per-module-mask adapter kernels at M = R = 300, K = N = 128; masks from the host restatement of the counter hash"""
    from oracle import dropout_mask as DM
    M, K, p, alpha = 300, 128, 0.25, 0.25
    seeds = MASK_SEEDS[:G] + (0,) * (3 - G)
    xh, Ah = rnd(M, K, seed=1), rnd(64 * G, K, seed=2, scale=0.05)
    dth, resh = rnd(M, 64 * G, seed=3, scale=0.5), rnd(M, K, seed=4)
    mults = [DM.multiplier(M, K, p, s) for s in seeds[:G]]
    xds = [(xh.float() * m).to(BF).float() for m in mults]                   # the dropped operand as the MFMA sees it
    if kind == "down":
        x, A = lay.inp("X", xh), lay.inp("A", Ah)
        t = lay.out("T", (M, 64 * G))
        call("rv_gemm_nt_lora_masks_bf16", x, ld(x), A, ld(A), t, ld(t), M, K, G, alpha, p, *seeds)
        lay.finish()
        for g in range(G):
            close(t[:, 64 * g:64 * g + 64].cpu(), alpha * (xds[g] @ Ah[64 * g:64 * g + 64].float().t()), what=f"F module {g}")
    elif kind == "dgrad":
        dt, aT = lay.inp("dT", dth), lay.inp("AT", Ah.t().contiguous())
        c = lay.io("C = residual", resh)
        call("rv_gemm_nt_dropout_masks_bf16", dt, ld(dt), aT, ld(aT), c, ld(c), M, K, G, c, ld(c), p, *seeds)
        lay.finish()
        ref = resh.float()
        for g in range(G):
            ref = ref + mults[g] * (dth[:, 64 * g:64 * g + 64].float() @ Ah[64 * g:64 * g + 64].float())
        close(c.cpu(), ref, what="B1")
    else:
        splits = 3                                     # 128-row chunks: a ragged last one
        dt, x = lay.inp("dT", dth), lay.inp("X", xh)
        dA, ws = lay.out("dA", (64 * G, K)), lay.out("workspace", (splits * 64 * G * K,), F32)
        call("rv_gemm_tn_lora_masks_bf16", dt, ld(dt), x, ld(x), dA, ld(dA), M, K, G, p, *seeds, splits, ws)
        lay.finish()
        for g in range(G):
            close(dA[64 * g:64 * g + 64].cpu(), dth[:, 64 * g:64 * g + 64].float().t() @ xds[g], what=f"B2 module {g}")


# =========================================================================================== attention
ATTN = {"causal-L200": dict(hd=128, causal=True, L=200), "causal-L1": dict(hd=128, causal=True, L=1),
        "full-hd64-L130": dict(hd=64, causal=False, L=130), "packed-L200": dict(hd=128, causal=True, L=200, seg=([40, 0], [120, 64])),
        "pad-free-1-130": dict(hd=128, causal=True, L=130, rows=[1, 130]),
        # causal = 0 at head dim 128, forward and backward (one pass per workgroup, an unpaired grid, every query block on the ragged
        # last key tile); with pad-free rows of 1 and 130 tokens: the grid has two blocks per row, the one-token row uses one
        "full-L130": dict(hd=128, causal=False, L=130), "full-pad-free-1-130": dict(hd=128, causal=False, L=130, rows=[1, 130])}
GAP = 64          # sentinel columns between / behind the q, k, v ranges and behind out / dO's heads


def _attn_geometry(c, G, S=2, H=2):
    """token rows and columns of one attention case: q | gap | k | gap | v | gap columns; pad-free rows: 3 gap rows, sequence 0,
    5 gap rows, sequence 1, 7 gap rows (rectangular rows cannot have row gaps: row s * L + l is the layout)"""
    hd, L, Hkv = c["hd"], c["L"], H // G
    q0, k0 = 0, H * hd + GAP
    v0 = k0 + Hkv * hd + GAP
    width = v0 + Hkv * hd + GAP
    if "rows" in c:
        lens = list(c["rows"])
        starts = [3, 3 + lens[0] + 5]
        ntok = starts[1] + lens[1] + 7
    else:
        lens, starts, ntok = [L] * S, [s * L for s in range(S)], S * L
    rowgap = torch.ones(ntok, dtype=torch.bool)
    for a, n in zip(starts, lens):
        rowgap[a:a + n] = False
    colgap = torch.ones(width, dtype=torch.bool)
    for c0, n in ((q0, H * hd), (k0, Hkv * hd), (v0, Hkv * hd)):
        colgap[c0:c0 + n] = False
    ocolgap = torch.zeros(H * hd + GAP, dtype=torch.bool)
    ocolgap[H * hd:] = True
    lse_hole = torch.zeros(S, H, L, dtype=torch.bool)
    for s_, n in enumerate(lens):
        lse_hole[s_, :, n:] = True
    return dict(S=S, H=H, Hkv=Hkv, hd=hd, L=L, q0=q0, k0=k0, v0=v0, width=width, lens=lens, starts=starts, ntok=ntok, rowgap=rowgap,
                hole=rowgap[:, None] | colgap[None, :], ohole=rowgap[:, None] | ocolgap[None, :], lse_hole=lse_hole.view(-1))


def _rows_cat(t, g):
    return torch.cat([t[a:a + n] for a, n in zip(g["starts"], g["lens"])])


def _attn_reference(lay, g, qkvh, G, mask_of):
    """fp32 attention per sequence on the device: (leaf x [ntok, width], out [sum n, H hd], [lse [H, n] per sequence])"""
    H, Hkv, hd = g["H"], g["Hkv"], g["hd"]
    x = dv(qkvh, lay).float().requires_grad_(True)
    outs, lses = [], []
    for s_, (a, n) in enumerate(zip(g["starts"], g["lens"])):
        blk = x[a:a + n]
        q = blk[:, g["q0"]:g["q0"] + H * hd].view(n, H, hd).transpose(0, 1)
        k = blk[:, g["k0"]:g["k0"] + Hkv * hd].view(n, Hkv, hd).transpose(0, 1).repeat_interleave(G, 0)
        v = blk[:, g["v0"]:g["v0"] + Hkv * hd].view(n, Hkv, hd).transpose(0, 1).repeat_interleave(G, 0)
        sc = (q @ k.transpose(-1, -2)) / math.sqrt(hd) + mask_of(s_, n)
        outs.append((torch.softmax(sc, -1) @ v).transpose(0, 1).reshape(n, H * hd))
        lses.append(torch.logsumexp(sc, -1).detach())
    return x, torch.cat(outs), lses


def _check_fwd(g, out, lse, ro, lses, what):
    H, hd = g["H"], g["hd"]
    close(_rows_cat(out, g)[:, :H * hd], ro.detach(), rel=2e-2, what=f"{what}: out")
    lse3 = lse.view(g["S"], H, g["L"])
    for s_, n in enumerate(g["lens"]):
        torch.testing.assert_close(lse3[s_, :, :n], lses[s_], rtol=1e-3, atol=2e-3)


def _attn_cases():
    out = []
    for name, c in ATTN.items():
        for G in (1, 2):
            if c["hd"] != 128:                     # rv_attn_bwd: head dim 128 only
                out.append((f"{name}-G={G}-fwd", dict(name=name, G=G, bwd=False, rope=False, dkv=0)))
                continue
            for rope in (False, True):
                for dkv in (0, 3):
                    out.append((f"{name}-G={G}-rope={rope}-dkv={dkv or 'default'}", dict(name=name, G=G, bwd=True, rope=rope, dkv=dkv)))
    # head dim 128 has a second forward kernel (attn_fwd3_kernel, rv_set_attn_fwd_version(3)): the same cases on it
    out += [(f"{cid}-fwd=3", dict(kw, fwdv=3)) for cid, kw in out if ATTN[kw["name"]]["hd"] == 128]
    return out


@case(*_attn_cases())
def c_attn(lay, name, G, bwd, rope, dkv, fwdv=0):
    """rv_attn_fwd, then rv_attn_bwd on its out / lse: everything outside the owned q | k | v columns and outside the sequences' token
    rows is poison on the input side and guard on the output side; lse and the delta planes hold the sentinel at l >= row_len[s].
    fwdv: the forward kernel (rv_set_attn_fwd_version; 0 = the default)"""
    from rlaif_v_amd import hip, ops
    c = ATTN[name]
    g = _attn_geometry(c, G)
    S, H, hd, L, ntok, width = g["S"], g["H"], g["hd"], g["L"], g["ntok"], g["width"]
    scale = 1.0 / math.sqrt(hd)
    qkvh = rnd(ntok, width, seed=L + hd + G, scale=0.7)
    qkv = lay.inp("qkv", qkvh, inner=g["hole"])
    out = lay.out("out", (ntok, H * hd + GAP), inner=g["ohole"])
    lse = lay.out("lse", (S * H * L,), F32, inner=g["lse_hole"])
    sh = e1 = roff = rlen = None
    if "seg" in c:
        sh, e1 = lay.inp("seg_sh", i32(c["seg"][0])), lay.inp("seg_e1", i32(c["seg"][1]))
    if "rows" in c:
        roff, rlen = lay.inp("row_off", i32(g["starts"])), lay.inp("row_len", i32(g["lens"]))
    hip.lib().call("rv_set_attn_fwd_version", fwdv)
    try:
        call("rv_attn_fwd", qkv, ld(qkv), g["q0"], g["k0"], g["v0"], out, ld(out), lse, S, L, H, hd, int(c["causal"]), scale, sh, e1, G,
             roff, rlen)
    finally:
        hip.lib().call("rv_set_attn_fwd_version", 0)
    if bwd:
        doh = rnd(ntok, H * hd + GAP, seed=L + 1)
        do = lay.inp("dO", doh, inner=g["ohole"])
        nws = int(hip.lib().lib.rv_attn_bwd_workspace_floats(S, H, L))
        assert nws == 3 * S * H * L
        delta = lay.out("delta", (nws,), F32, inner=g["lse_hole"].repeat(3))
        dqkv = lay.out("dqkv", (ntok, width), inner=g["hole"])
        cos = sin = pos = posh = None
        if rope:
            cos_d, sin_d = ops.rope_tables(512, hd, 10000.0, lay.dev)
            cos, sin = lay.inp("rope_cos", cos_d.reshape(-1)), lay.inp("rope_sin", sin_d.reshape(-1))
            if "rows" in c or G == 2:              # a position per token row of the buffer (required under pad-free rows)
                posh = torch.randint(0, 512, (ntok,), generator=torch.Generator().manual_seed(1)).to(I32)
                pos = lay.inp("rope_pos", posh, inner=g["rowgap"])
        hip.lib().call("rv_set_attn_dkv_version", dkv)
        try:
            call("rv_attn_bwd", qkv, ld(qkv), g["q0"], g["k0"], g["v0"], do, ld(do), out, ld(out), lse, delta, dqkv, ld(dqkv), S, L, H,
                 hd, int(c["causal"]), scale, sh, e1, G, cos, sin, pos, roff, rlen)
        finally:
            hip.lib().call("rv_set_attn_dkv_version", 0)
    lay.finish()

    def mask_of(s_, n):
        if "seg" in c:
            return _packed_mask(n, c["seg"][0][s_], c["seg"][1][s_], lay.dev)
        return torch.full((n, n), float("-inf"), device=lay.dev).triu(1) if c["causal"] else torch.zeros(n, n, device=lay.dev)
    x, ro, lses = _attn_reference(lay, g, qkvh, G, mask_of)
    _check_fwd(g, out, lse, ro, lses, name)
    if not bwd:
        return
    ro.backward(_rows_cat(dv(doh, lay), g)[:, :H * hd].float())
    grad = _rows_cat(x.grad, g)
    got = _rows_cat(dqkv, g)
    if rope:                                       # dQ, dK rotated back: dx1 = dy1 cos + dy2 sin, dx2 = dy2 cos - dy1 sin
        if posh is not None:
            pp = _rows_cat(dv(posh, lay), g).long()
        else:
            pp = torch.cat([torch.arange(n, device=lay.dev) for n in g["lens"]])
        cc, ss = cos_d[pp][:, None], sin_d[pp][:, None]
        grad = grad.clone()
        for c0, nh in ((g["q0"], H), (g["k0"], g["Hkv"])):
            y = grad[:, c0:c0 + nh * hd].reshape(-1, nh, 2, 64)
            y1, y2 = y[:, :, 0], y[:, :, 1]
            grad[:, c0:c0 + nh * hd] = torch.stack([y1 * cc + y2 * ss, y2 * cc - y1 * ss], 2).reshape(-1, nh * hd)
    for nm, c0, nh in (("q", g["q0"], H), ("k", g["k0"], g["Hkv"]), ("v", g["v0"], g["Hkv"])):
        close(got[:, c0:c0 + nh * hd], grad[:, c0:c0 + nh * hd], rel=2.5e-2, what=f"{name}: d{nm} rope={rope} dkv={dkv}")
    # the delta workspace, first plane: rowsum(dO * O) of the forward output (what rv_attn_delta computes)
    d3 = delta.view(3, S, H, L)
    of, dof = _rows_cat(out, g)[:, :H * hd].float(), _rows_cat(dv(doh, lay), g)[:, :H * hd].float()
    rs = (of.double() * dof.double()).view(-1, H, hd).sum(-1)
    bound = hd * 2.0 ** -24 * (of.double() * dof.double()).abs().view(-1, H, hd).sum(-1) + 1e-30    # an hd-term fp32 sum, any order
    at = 0
    for s_, n in enumerate(g["lens"]):
        assert bool(((d3[0, s_, :, :n].double() - rs[at:at + n].t()).abs() <= bound[at:at + n].t()).all()), f"{name}: delta plane"
        assert torch.equal(d3[1, s_, :, :n], -d3[0, s_, :, :n])
        at += n


@case(("", {}))
def c_attn_fwd_branches(lay):
    """tests/test_attn_branches_gpu.py's rows (prefix 70 + six branches, prefix 0 + four branches), H = 2, pad-free with gap rows"""
    from test_attn_branches_gpu import ROWS, _q_lo
    lens = [sh + sum(br) for sh, br in ROWS]
    G = 1
    g = _attn_geometry(dict(hd=128, L=max(lens), rows=lens), G)
    S, H, hd, L, ntok = g["S"], g["H"], g["hd"], g["L"], g["ntok"]
    qkvh = rnd(ntok, g["width"], seed=17, scale=0.7)
    qloh = torch.zeros(ntok, dtype=I32)
    for (sh_, br), a in zip(ROWS, g["starts"]):
        ql = _q_lo(sh_, br)
        qloh[a:a + len(ql)] = i32(ql)
    qkv = lay.inp("qkv", qkvh, inner=g["hole"])
    sh, qlo = lay.inp("seg_sh", i32([r[0] for r in ROWS])), lay.inp("q_lo", qloh, inner=g["rowgap"])
    roff, rlen = lay.inp("row_off", i32(g["starts"])), lay.inp("row_len", i32(g["lens"]))
    out = lay.out("out", (ntok, H * hd + GAP), inner=g["ohole"])
    lse = lay.out("lse", (S * H * L,), F32, inner=g["lse_hole"])
    call("rv_attn_fwd_branches", qkv, ld(qkv), g["q0"], g["k0"], g["v0"], out, ld(out), lse, S, L, H, hd, 1.0 / math.sqrt(hd), sh, qlo,
         G, roff, rlen)
    lay.finish()

    def mask_of(s_, n):
        i, j = torch.arange(n, device=lay.dev)[:, None], torch.arange(n, device=lay.dev)[None, :]
        lo = dv(i32(_q_lo(*ROWS[s_])), lay)[:, None]
        return torch.where((j <= i) & ((j < ROWS[s_][0]) | (j >= lo)), 0.0, float("-inf"))
    _, ro, lses = _attn_reference(lay, g, qkvh, G, mask_of)
    _check_fwd(g, out, lse, ro, lses, "branches")


@case(*grid(hd=[128, 64]))
def c_attn_delta(lay, hd):
    S, L, H = 2, 5, 3
    doh, oh = rnd(S * L, H * hd, seed=1), rnd(S * L, H * hd, seed=2)
    do, o = lay.inp("dO", doh), lay.inp("O", oh)
    delta = lay.out("delta", (S * H * L,), F32)
    call("rv_attn_delta", do, ld(do), o, ld(o), delta, S, L, H, hd)
    lay.finish()

    def ref(dt):                                  # [S, H, L]
        return (doh.to(dt) * oh.to(dt)).view(S, L, H, hd).sum(-1).permute(0, 2, 1).contiguous()
    yardstick(delta.view(S, H, L).cpu(), ref(F32), ref(torch.float64), f"attn_delta hd={hd}")


# =========================================================================================== LM head and loss
@case(*grid(variant=[-1, 3]))
def c_lmhead(lay, variant):
    """M = 100 rows of a 128-row h whose rows 100..127 are poison; V = 512 stored, 449 valid: rows 449..511 of W are poison too
    (those columns are left out of the softmax and written as zeros).  dlogits has ldd > V; its rows >= M are not the kernel's.
    tgt_logit: the caller pre-fills it (ops.lmhead_logp_fwd: zeros) - a row whose target is no vocabulary id keeps the fill."""
    M, Mpad, K, V, Vv = 100, 128, 256, 512, 449
    nblk = V // 64
    hh, wh = rnd(Mpad, K, seed=1), rnd(V, K, seed=2, scale=0.2)
    tgth = torch.randint(0, Vv, (M,), generator=torch.Generator().manual_seed(3)).to(I32)
    tgth[0], tgth[1], tgth[2] = 0, Vv - 1, -100
    hrows = torch.zeros(Mpad, K, dtype=torch.bool)
    hrows[M:] = True
    wrows = torch.zeros(V, K, dtype=torch.bool)
    wrows[Vv:] = True
    h, w, tgt = lay.inp("h", hh, inner=hrows), lay.inp("W", wh, inner=wrows), lay.inp("tgt", tgth)
    pmax, psum = lay.out("pmax", (M * nblk,), F32), lay.out("psum", (M * nblk,), F32)
    tl = lay.io("tgt_logit", torch.zeros(M))
    call("rv_lmhead_logp_fwd", h, ld(h), w, ld(w), tgt, M, V, Vv, K, pmax, psum, tl, variant)
    lse, logp = lay.out("lse", (M,), F32), lay.out("logp", (M,), F32)
    call("rv_logp_finish", pmax, psum, tl, nblk, M, lse, logp)
    # finish + unpack: slots no row names keep the caller's fill; negative and out-of-range indices are skipped
    n_pt, n_c = 150, 90
    dst_a = torch.randperm(n_pt, generator=torch.Generator().manual_seed(5))[:M].to(I32)
    dst_a[3], dst_a[4] = -1, n_pt + 7
    dst_b = torch.full((M,), -1, dtype=I32)
    free = sorted(set(range(n_pt)) - set(dst_a.tolist()))
    dst_b[10], dst_b[11] = free[0], free[1]
    dst_c = torch.arange(M, dtype=I32)                              # rows 90..99 are out of range for compact[90]
    dst_c[5] = -1
    da, db, dc = lay.inp("dst_a", dst_a), lay.inp("dst_b", dst_b), lay.inp("dst_c", dst_c)
    per_token, compact = lay.io("per_token", torch.full((n_pt,), -7.0)), lay.io("compact", torch.full((n_c,), -9.0))
    call("rv_logp_finish_unpack", pmax, psum, tl, nblk, M, da, db, dc, per_token, n_pt, compact, n_c)
    coefh = torch.randn(M, generator=torch.Generator().manual_seed(4))
    coef = lay.inp("coef", coefh)
    drows = torch.zeros(Mpad, V, dtype=torch.bool)
    drows[M:] = True
    dlog = lay.out("dlogits", (Mpad, V), inner=drows)
    call("rv_lmhead_logp_bwd", h, ld(h), w, ld(w), tgt, lse, coef, dlog, ld(dlog), M, V, Vv, K, variant)
    lay.finish()
    logits = mm(hh[:M], wh[:Vv].t(), lay)
    ok = dv(tgth, lay) >= 0
    t_idx = dv(tgth, lay).clamp(min=0).long()
    ref_lse = torch.logsumexp(logits, -1)
    ref_lp = torch.where(ok, logits.gather(1, t_idx[:, None])[:, 0], torch.zeros_like(ref_lse)) - ref_lse
    torch.testing.assert_close(lse, ref_lse, rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(logp, ref_lp, rtol=1e-4, atol=1e-3)
    assert tl[2].item() == 0.0
    pt, cp, lp = per_token.cpu(), compact.cpu(), logp.cpu()
    exp_pt, exp_c = torch.full((n_pt,), -7.0), torch.full((n_c,), -9.0)
    for m in range(M):
        for d_ in (int(dst_a[m]), int(dst_b[m])):
            if 0 <= d_ < n_pt:
                exp_pt[d_] = lp[m]
        if 0 <= int(dst_c[m]) < n_c:
            exp_c[int(dst_c[m])] = lp[m]
    assert torch.equal(pt, exp_pt) and torch.equal(cp, exp_c)       # the same device code as rv_logp_finish: bit-equal
    onehot = F.one_hot(t_idx, Vv).float() * ok[:, None]
    close(dlog[:M, :Vv], dv(coefh, lay)[:, None] * (onehot - torch.softmax(logits, -1)), rel=1e-2, what="dlogits (valid columns)")
    assert not bool(dlog[:M, Vv:].cpu().view(torch.int16).any())


@case(("", {}))
def c_seq_sum_dpo_row_coef(lay):
    import itertools
    from oracle import dpo_oracle as O
    B = 5
    gen = torch.Generator().manual_seed(0)
    lens = [7, 1, 12, 3, 9, 4, 0, 6, 2, 11]
    n = sum(lens)
    offh = i32([0] + list(itertools.accumulate(lens)))
    logph, wth = -torch.rand(n, generator=gen) * 5, torch.rand(n, generator=gen)
    logp, wt, off = lay.inp("logp", logph), lay.inp("weight", wth), lay.inp("seq_off", offh)
    s, c = lay.out("seq_sum", (2 * B,), F32), lay.out("seq_cnt", (2 * B,), F32)
    sw, cw = lay.out("weighted sum", (2 * B,), F32), lay.out("weighted cnt", (2 * B,), F32)
    call("rv_seq_sum", logp, None, off, 2 * B, s, c)
    call("rv_seq_sum", logp, wt, off, 2 * B, sw, cw)
    rwh, rrh = -20 * torch.rand(B, generator=gen), -20 * torch.rand(B, generator=gen)
    rw, rr = lay.inp("ref_win", rwh), lay.inp("ref_rej", rrh)
    per_pair, scal, coef = lay.out("per_pair", (5 * B,), F32), lay.out("scalars", (8,), F32), lay.out("coef", (2 * B,), F32)
    call("rv_dpo_loss", s, c, rw, rr, B, 0.1, 0, 0.3, 0.7, per_pair, scal, coef)
    seq_of_row = torch.cat([torch.full((m,), i_, dtype=I32) for i_, m in enumerate(lens)])
    sor = lay.inp("seq_of_row", seq_of_row)
    rc, rcw = lay.out("row coef", (n,), F32), lay.out("weighted row coef", (n,), F32)
    call("rv_row_coef", coef, sor, None, rc, n)
    call("rv_row_coef", coef, sor, wt, rcw, n)
    lay.finish()
    sc_, cc_ = s.cpu(), c.cpu()
    seg = [slice(int(offh[i_]), int(offh[i_ + 1])) for i_ in range(2 * B)]
    torch.testing.assert_close(sc_, torch.stack([logph[r].sum() for r in seg]), rtol=1e-6, atol=1e-5)
    assert cc_.tolist() == [float(m) for m in lens]
    # (weighted: the unweighted test's bound - sums of at most 12 fp32 products of magnitude <= 5)
    torch.testing.assert_close(sw.cpu(), torch.stack([(logph[r] * wth[r]).sum() for r in seg]), rtol=1e-6, atol=1e-5)
    torch.testing.assert_close(cw.cpu(), torch.stack([wth[r].sum() for r in seg]), rtol=1e-6, atol=1e-5)
    sv = sc_.clone().requires_grad_(True)
    losses, cw_, cr_ = O.dpo_loss(sv[:B], sv[B:], rwh, rrh, 0.1)
    loss = 0.7 * losses.mean() - 0.3 * sv[:B].mean()
    loss.backward()
    pp = per_pair.view(5, B).cpu()
    torch.testing.assert_close(pp[0], losses.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(pp[1], cw_.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(pp[2], cr_.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(scal.cpu()[0], loss.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(coef.cpu(), sv.grad, rtol=1e-4, atol=1e-7)
    assert torch.equal(rc.cpu(), coef.cpu()[seq_of_row.long()]) and torch.equal(rcw.cpu(), coef.cpu()[seq_of_row.long()] * wth)


@case(*grid(penalty=[1.0, 1.1]))
def c_next_token_scores(lay, penalty):
    """logits columns [V_valid, ldl) and the rows behind M are poison"""
    import numpy as np
    from test_next_token_scores_gpu import _make, _reference
    M, Mrows, Vv = 3, 5, 32009
    logits, ldl, want, seen = _make(M, Vv, seed=M * 7 + Vv)
    logits[0, 100] = logits[0, 31000] = 40.0
    logits[1, Vv - 1] = 41.0
    full = np.zeros((Mrows, ldl), dtype=np.float32)
    full[:M] = logits
    hole = torch.zeros(Mrows, ldl, dtype=torch.bool)
    hole[:, Vv:] = True
    hole[M:] = True
    lg = lay.inp("logits", torch.from_numpy(full), inner=hole)
    off = np.zeros(M + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(x) for x in seen])
    seen_off, seen_ids = lay.inp("seen_off", torch.from_numpy(off)), lay.inp("seen_ids", i32(sum(seen, [])))
    K = len(want)
    want_t = lay.inp("want_ids", torch.from_numpy(want.astype(np.int32)))
    probs, logp = lay.out("probs", (M * K,), F32), lay.out("logp", (M * K,), F32)
    argmax, lse = lay.out("argmax", (M,), I32), lay.out("lse", (M,), F32)
    call("rv_next_token_scores", lg, ld(lg), M, Vv, seen_off, seen_ids, penalty, want_t, K, probs, logp, argmax, lse)
    lay.finish()
    r_logp, r_probs, r_arg, r_lse = _reference(logits, Vv, seen, penalty, want)
    assert np.abs(lse.cpu().numpy().astype(np.float64) - r_lse).max() <= 3e-5
    assert np.abs(logp.view(M, K).cpu().numpy().astype(np.float64) - r_logp).max() <= 3e-5
    np.testing.assert_allclose(probs.view(M, K).cpu().numpy().astype(np.float64), r_probs, rtol=1e-4, atol=1e-30)
    assert argmax.cpu().numpy().tolist() == r_arg.tolist()


# =========================================================================================== CLIP image preprocessing
@case(("", {}))
def c_resize(lay):
    """the two passes of the bicubic resize on the (97, 411) image of tests/test_image_preprocess.py: source rows and columns no
    tap reads are poison; bit-exact against the oracle of Pillow's fixed-point filter"""
    import numpy as np
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_image_golden as MG
    from oracle import clip_preprocess_oracle as P
    from rlaif_v_amd import image as im
    Hh, W, size = 97, 411, 336
    img = MG.make_image(Hh, W, 4)
    oh, ow = im.resize_output_size(Hh, W, size)
    top, left = (oh - size) // 2, (ow - size) // 2
    ks_h, b_h, k_h = im._taps(W, ow)
    ks_v, b_v, k_v = im._taps(Hh, oh)
    bv = b_v[top:top + size].copy()
    bh = b_h[left:left + size]
    y0, y1 = int(bv[0, 0]), int(bv[-1, 0] + bv[-1, 1])
    x0, x1 = int(bh[:, 0].min()), int((bh[:, 0] + bh[:, 1]).max())
    bv[:, 0] -= y0
    unread = torch.ones(Hh, W, 3, dtype=torch.bool)
    unread[y0:y1, x0:x1] = False
    src = lay.inp("src", torch.from_numpy(np.ascontiguousarray(img)).view(-1), inner=unread.view(-1))
    bh_d, kh_d = lay.inp("h bounds", torch.from_numpy(np.ascontiguousarray(bh)).view(-1)), lay.inp("h taps", torch.from_numpy(np.ascontiguousarray(k_h[left:left + size])).view(-1))
    bv_d, kv_d = lay.inp("v bounds", torch.from_numpy(bv).view(-1)), lay.inp("v taps", torch.from_numpy(np.ascontiguousarray(k_v[top:top + size])).view(-1))
    table = lay.inp("table", torch.from_numpy(im._norm_table(im.CLIP_MEAN, im.CLIP_STD, 1 / 255)).view(-1))
    # (a uint8 result can legitimately equal the sentinel byte: no "nothing left unwritten" check on tmp; out proves the pass ran)
    tmp = lay.out("tmp", ((y1 - y0) * size * 3,), torch.uint8, written=None)
    out = lay.out("out", (3 * size * size,), F32)
    call("rv_resize_h_u8", src, Hh, W, y0, y1 - y0, bh_d, kh_d, ks_h, size, tmp)
    call("rv_resize_v_norm_u8", tmp, y1 - y0, size, bv_d, kv_d, ks_v, size, table, out)
    lay.finish()
    assert np.array_equal(out.view(3, size, size).cpu().numpy(), P.clip_preprocess(img))


# =========================================================================================== the table
@pytest.mark.parametrize("fn,kw", CASES)
def test_containment(fn, kw):
    run_case(fn, **kw)
