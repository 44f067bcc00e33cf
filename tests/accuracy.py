"""Per-element float64 error bounds for kernel outputs (plain helper module, imported by putting the tests directory on sys.path like
guarded.py; works on CPU and GPU tensors alike).

check(got, ref64, E, out_dtype, what) asserts, element by element,

    |got - ref64| <= 0.5 * ulp_out(|ref64| + E) + E

ref64 is the operation in float64 on the same (bf16-rounded or fp32) inputs; ulp_out is the spacing of the OUTPUT type at that
magnitude (bf16: 2^(floor(log2 r) - 7), fp32: 2^(floor(log2 r) - 23), never below the spacing of the smallest normal binade); E is
a per-element float64 tensor that bounds the error the kernel's documented arithmetic may have BEFORE its one round-to-nearest-even
store.  The ulp is taken at |ref64| + E because the unrounded value may sit one binade above ref64.  Nothing in the bound comes from
`got`.

Edge rules: where RNE(ref64) overflows to +-inf, `got` must be that inf; where |ref64| < 2^-126, |got| <= 2^-126 is accepted as well
(flush to zero; signed zeros compare equal); a NaN in `got` always fails; no other element is left out.

Discrimination cap: median(E / ulp) over the elements held to the bound must be <= 1/8, or the case is refused (CapError): a case
cannot pass by inflating E.  Cancelling elements may have a large E, the median may not.  The ulp of the cap is the bf16 one for
fp32 outputs too: the E of an fp32 evaluation is a few fp32 ulps by construction (never an eighth of one), so an fp32 output is
held to the cap its bf16 rounding would be held to - no fp32 case may be looser than a bf16 case - and to its own, 2^16 times
finer, half ulp in the bound.  Documented bf16 operand roundings (`doc`) stay out of the capped share, and for outputs that cancel by
construction the share is measured against ulp + doc (check(cap_unit=...) says why).  The cap cannot be switched off.

How an E is built (the functions below; every caller writes its one-line derivation next to the case):
  * fp32 evaluation in any order (Higham): a sum of n terms carries n * 2^-24 * sum |terms|.  A GEMM: (K + c) * 2^-24 * |alpha| *
    (|A| |B|)[m][n] (gemm_E) plus 2^-24 times |bias|, |residual|, ...;
    exp(x) through __expf / exp2: (|x| + 2) * 2^-23 relative (the argument is scaled by log2 e in fp32: |x| * 2^-24 twice, v_exp_f32
    is good to 1 ulp); division, rsqrt and erff: FEW * 2^-24 relative; each propagated through the op's derivative;
    an fp32 intermediate below 2^-126 may flush: TINY absolute, propagated the same way;
  * one bf16 operand rounding inside the kernel where the header documents one: 2^-8 relative (the UNIT ROUNDOFF of bf16, not 2^-9);
  * nothing else.
MFMA_FACTOR multiplies the K * 2^-24 term of gemm_E: how a gfx950 MFMA rounds inside one instruction cannot be derived.  1 = IEEE;
a larger value is twice the ratio torch's own bf16 matmul reaches on the device through this same check, rounded up to a power of
two (CHANGELOG.md records the measurement) - never a figure taken from the library under test."""
import math
from typing import Optional

import torch

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
U32 = 2.0 ** -24             # unit roundoff of fp32
U16 = 2.0 ** -8              # unit roundoff of bf16
TINY = 2.0 ** -126           # smallest normal of bf16 and fp32
FEW = 8.0                    # "a few" 2^-24: correctly rounded division is 1, v_rsq_f32 / v_rcp_f32 are 1 ulp (2), OCML erff / logf / log1pf 4 ulp (8)
MFMA_FACTOR = 1.0            # see the module docstring
CAP = 0.125
_MANT = {BF: 7, F32: 23}
_MAXFIN = {BF: float(torch.finfo(BF).max), F32: float(torch.finfo(F32).max)}


class AccuracyError(AssertionError):
    pass


class CapError(AccuracyError):
    pass


def f64(t: torch.Tensor) -> torch.Tensor:
    return t.to(F64)


def ulp(r: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of `dtype` at magnitude r (float64, r >= 0): 2^(floor(log2 r) - mant), at least that of the smallest normal binade."""
    r = f64(r).abs()
    _, e = torch.frexp(torch.clamp(r, min=TINY))        # r = m * 2^e, m in [0.5, 1): floor(log2 r) = e - 1
    e = torch.clamp(e.to(F64) - 1.0, min=-126.0, max=1023.0 - _MANT[dtype] - 1)
    return torch.ldexp(torch.ones_like(r), (e - _MANT[dtype]).to(torch.int32))


def rne(ref64: torch.Tensor, dtype) -> torch.Tensor:
    """ref64 rounded to nearest even in `dtype`, as float64 (+-inf on overflow).  Exact: the scaling is by a power of two and
    torch.round rounds halves to even."""
    ref64 = f64(ref64)
    q = ulp(ref64, dtype)
    r = torch.round(ref64 / q) * q
    return torch.where(r.abs() > _MAXFIN[dtype], torch.sign(r) * math.inf, r)


def bound(ref64: torch.Tensor, E: torch.Tensor, dtype) -> torch.Tensor:
    ref64 = f64(ref64)
    return 0.5 * ulp(ref64.abs() + E, dtype) + E


def check(got: torch.Tensor, ref64: torch.Tensor, E, out_dtype=None, what: str = "output", cap=True, doc=None, cap_unit: str = "ulp"):
    """Raises AccuracyError naming `what`; returns the figures it prints (a dict: ratio, differs, mean_ulps, median_E_ulps).  E: float64 tensor broadcastable to ref64, or a python float.
    doc: the share of E that comes from documented bf16 operand roundings (see no_doc); the cap applies to E - doc.
    cap: True = CAP (1/8); it cannot be switched off.
    cap_unit: what the fp32 share E - doc is measured against.  "ulp" (default): the output ulp, the issue's cap.  "ulp+doc": the
    contract part of the bound, output ulp + documented roundings, for outputs that cancel by construction - the attention backward's
    dQ_i = scale sum_j dS_ij k_j has sum_j dS_ij = 0 (with equal keys dQ is exactly 0), so the output's ulp says nothing about the size
    of the terms; its documented 2^-8 sum |dS| |k| is 2 - 6 ulp (median) and the fp32 share, fed by two hd = 128-deep any-order sums per
    dS_ij, 0.1 - 0.8 ulp.  The cap then still says what it is for: the share of the bound a case could inflate stays below an eighth
    of the share the contract fixes (0.02 - 0.11 on the prescribed rows; tests/test_accuracy_helper.py prints the figures)."""
    out_dtype = out_dtype or got.dtype
    if cap is not True:
        raise ValueError(f"{what}: the discrimination cap cannot be switched off")
    if out_dtype not in _MANT:
        raise TypeError(f"{what}: outputs are bf16 or fp32, not {out_dtype}")
    ref64 = f64(ref64)
    if got.shape != ref64.shape:
        raise AccuracyError(f"{what}: shape {tuple(got.shape)} against the reference's {tuple(ref64.shape)}")
    g = f64(got)
    E = torch.as_tensor(E, dtype=F64, device=ref64.device).expand(ref64.shape)
    if not bool(torch.isfinite(ref64).all()) or not bool(torch.isfinite(E).all()) or bool((E < 0).any()):
        raise ValueError(f"{what}: the reference and E must be finite and E >= 0 (a broken case, not a kernel fault)")
    nan = torch.isnan(g)
    if bool(nan.any()):
        idx = tuple(nan.nonzero()[0].tolist())
        raise AccuracyError(f"{what}: NaN in the output, {int(nan.sum())} element(s), first at index {idx} (ref64 {ref64[idx].item():.9g})")
    r = rne(ref64, out_dtype)
    over = torch.isinf(r)
    tiny = ref64.abs() < TINY
    b = bound(ref64, E, out_dtype)
    err = (g - ref64).abs()
    ok = torch.where(over, g == r, err <= b)
    ok = ok | (tiny & (g.abs() <= TINY))
    held = ~over & ~tiny
    u = ulp(ref64, out_dtype)
    entry = {"what": what, "ratio": 0.0, "differs": 0.0, "mean_ulps": 0.0, "median_E_ulps": 0.0, "n": ref64.numel()}
    if bool(held.any()):
        ratio = torch.where(held, err / b, torch.zeros_like(err))
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
        entry["ratio"] = float(ratio.max())
        entry["differs"] = float((g != r)[held].double().mean())
        fin = held & torch.isfinite(g)
        entry["mean_ulps"] = float(((g - ref64) / u)[fin].mean()) if bool(fin.any()) else 0.0
        E_cap = E if doc is None else torch.clamp(E - torch.as_tensor(doc, dtype=F64, device=E.device), min=0.0)
        if cap_unit not in ("ulp", "ulp+doc") or (cap_unit == "ulp+doc" and doc is None):
            raise ValueError(f"{what}: cap_unit is 'ulp' or, with doc, 'ulp+doc'")
        unit = ulp(ref64, BF) + (torch.as_tensor(doc, dtype=F64, device=E.device) if cap_unit == "ulp+doc" else 0.0)
        entry["median_E_ulps"] = float((E_cap / unit)[held].median())
    stats = (f"max error / bound {entry['ratio']:.3f}; {100 * entry['differs']:.2f} % of the elements differ from RNE(ref64); "
             f"mean signed error {entry['mean_ulps']:+.4f} ulp; median E / bf16 ulp {entry['median_E_ulps']:.4f}")
    cap_at = CAP
    if entry["median_E_ulps"] > cap_at:
        raise CapError(f"{what}: median E / ulp is {entry['median_E_ulps']:.4f} > {cap_at}: the case cannot tell a wrong kernel from a "
                       f"right one - choose K and the input scales so that E stays below an eighth of an output ulp")
    print(f"[accuracy] {what}: {stats}")
    if not bool(ok.all()):
        bad = ~ok
        score = torch.where(bad, torch.where(over | ~torch.isfinite(err), torch.full_like(err, math.inf), err / b), torch.zeros_like(err))
        flat = int(score.argmax())
        idx = tuple(torch.unravel_index(torch.tensor(flat), ref64.shape)) if ref64.dim() else ()
        idx = tuple(int(i) for i in idx)
        rule = "must be that inf (RNE(ref64) overflows)" if bool(over[idx]) else f"bound {b[idx].item():.9g}"
        raise AccuracyError(f"{what}: {int(bad.sum())} of {ref64.numel()} element(s) outside the bound, worst at index {idx}: ref64 "
                            f"{ref64[idx].item():.9g}, got {g[idx].item():.9g}, {rule}; {stats}")
    return entry


def check_bits(got: torch.Tensor, want: torch.Tensor, what: str = "output"):
    """Bit-for-bit equality on the integer view (data movement, casts): NaN-safe, signed zeros differ."""
    iv = {BF: torch.int16, F32: torch.int32}[got.dtype]
    if got.shape != want.shape or got.dtype != want.dtype:
        raise AccuracyError(f"{what}: {tuple(got.shape)} {got.dtype} against {tuple(want.shape)} {want.dtype}")
    bad = got.contiguous().view(iv) != want.contiguous().view(iv)
    if bool(bad.any()):
        idx = tuple(bad.nonzero()[0].tolist())
        raise AccuracyError(f"{what}: {int(bad.sum())} of {got.numel()} element(s) differ bit for bit, first at index {idx}: want "
                            f"{want[idx].item()!r}, got {got[idx].item()!r}")


# ------------------------------------------------------------------------------------------------------------- error terms
def gemm_E(a64: torch.Tensor, bt64: torch.Tensor, K: int, alpha: float = 1.0, c: int = 2) -> torch.Tensor:
    """fp32 accumulation of K products in any order, then * alpha: (MFMA_FACTOR * K + c) * 2^-24 * |alpha| * (|A| |B|)[m][n];
    a64 [M][K], bt64 [K][N].  The products of bf16 operands are exact in fp32 (16 significant bits).  K counts, per output element,
    the products that are not zero (adding an exact zero is exact in any order): sparse operands let a case reach a kernel that only
    takes deep contractions and still keep E under the cap."""
    K = torch.clamp((a64 != 0).double() @ (bt64 != 0).double(), max=float(K))
    return (MFMA_FACTOR * K + c) * U32 * abs(alpha) * (a64.abs() @ bt64.abs())


def exp_rel(x64: torch.Tensor) -> torch.Tensor:
    """relative error of __expf(x) / exp2(x * log2 e) in fp32"""
    return (x64.abs() + 2.0) * 2.0 * U32


FLT_MAX = _MAXFIN[F32]
DENORM = 2.0 ** -149


class Val:
    """A float64 value `v` together with a bound `e` on the absolute error of its fp32 evaluation: the kernel's formula is written
    once with these objects, line by line as the kernel has it, and every operation adds its own term - one fp32 rounding (2^-24
    relative, 2^-149 where a product may be subnormal), the propagated errors of its operands INCLUDING the second-order product (a
    constant row's variance is all second order), the function's own accuracy (exp_rel for __expf, FEW for erff / logf / log1pf, 1 ulp
    for v_rsq_f32, correctly rounded division and sqrt) and TINY where v_exp_f32 / v_rcp_f32 / v_rsq_f32 flush a subnormal result.
    An operand that is not a Val is exact (a kernel input)."""

    def __init__(self, v, e=None):
        self.v = f64(torch.as_tensor(v))
        self.e = torch.zeros_like(self.v) if e is None else f64(torch.as_tensor(e)).to(self.v.device).expand(self.v.shape).clone()

    @staticmethod
    def of(x) -> "Val":
        return x if isinstance(x, Val) else Val(x)

    def _pair(self, o):
        """both operands on one device (python scalars and literals live on the CPU)"""
        o = Val.of(o)
        dev = self.v.device if self.v.device.type != "cpu" else o.v.device
        return Val(self.v.to(dev), self.e.to(dev)), Val(o.v.to(dev), o.e.to(dev))

    @staticmethod
    def const(x: float) -> "Val":
        """a literal of the source: rounded to fp32 by the compiler"""
        return Val(torch.tensor(float(x), dtype=F64), abs(float(x)) * U32)

    def _rounded(self, v, e, extra=0.0):
        return Val(v, e + U32 * (v.abs() + e) + extra)

    def __neg__(self):
        return Val(-self.v, self.e)

    def __add__(self, o):
        self, o = self._pair(o)
        return self._rounded(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-Val.of(o))

    def __rsub__(self, o):
        return Val.of(o) + (-self)

    def __mul__(self, o):
        self, o = self._pair(o)
        return self._rounded(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e, DENORM)

    __rmul__ = __mul__

    def __truediv__(self, o):
        self, o = self._pair(o)
        v = self.v / o.v
        lo = o.v.abs() - o.e
        over = torch.isinf(o.e)                          # the divisor overflowed fp32: the quotient is 0 or below |a| / FLT_MAX
        if bool(((lo <= 0) & ~over).any()):
            raise ValueError("Val: a divisor is not bounded away from zero")
        e = (self.v.abs() * o.e + o.v.abs() * self.e) / (o.v.abs() * lo)
        e = torch.where(over, (self.v.abs() + self.e) / FLT_MAX + v.abs(), e)
        return self._rounded(v, e, TINY)

    def __rtruediv__(self, o):
        return Val.of(o) / self

    def exp(self, fast: bool = True) -> "Val":
        """__expf (fast) or expf (1 ulp); a value past the fp32 range becomes inf: e = inf, which only a division absorbs"""
        v = torch.exp(self.v)
        rel = exp_rel(self.v) if fast else torch.full_like(v, 2.0 * U32)
        hi = torch.exp(self.v + self.e)
        e = (hi - v) + hi * rel + TINY
        return Val(v, torch.where(v > FLT_MAX, torch.full_like(v, math.inf), e))

    def erf(self) -> "Val":
        v = torch.erf(self.v)
        near = torch.clamp(self.v.abs() - self.e, min=0.0)
        return Val(v, self.e * (2.0 / math.sqrt(math.pi)) * torch.exp(-near * near) + FEW * U32 * v.abs())

    def rsqrt(self) -> "Val":
        lo = self.v - self.e
        if bool((lo <= 0).any()):
            raise ValueError("Val: rsqrt of a value not bounded away from zero")
        v = self.v.rsqrt()
        return Val(v, (lo.rsqrt() - v) + 2.0 * U32 * v + TINY)

    def sqrt(self) -> "Val":
        v = self.v.sqrt()
        return self._rounded(v, v - torch.clamp(self.v - self.e, min=0.0).sqrt())

    def log(self) -> "Val":
        lo = self.v - self.e
        if bool((lo <= 0).any()):
            raise ValueError("Val: log of a value not bounded away from zero")
        v = self.v.log()
        return Val(v, torch.log(self.v / lo) + FEW * U32 * v.abs())

    def log1p(self) -> "Val":
        v = torch.log1p(self.v)
        return Val(v, self.e / (1.0 + self.v - self.e) + FEW * U32 * v.abs())

    def sum(self, dim, keepdim: bool = False, depth: Optional[int] = None) -> "Val":
        """n terms in any order (Higham): (n - 1) * 2^-24 * sum |terms|.  `depth`: the kernel's summation tree is known and no term
        passes through more than `depth` additions - depth * 2^-24 * sum |terms| (the caller names the loop)."""
        n = self.v.shape[dim] if isinstance(dim, int) else math.prod(self.v.shape[d] for d in dim)
        mag = (self.v.abs() + self.e).sum(dim, keepdim)
        return Val(self.v.sum(dim, keepdim), self.e.sum(dim, keepdim) + (n - 1 if depth is None else min(depth, n - 1)) * U32 * mag)

    def maximum(self, o) -> "Val":
        self, o = self._pair(o)
        return Val(torch.maximum(self.v, o.v), torch.maximum(self.e, o.e))

    def abs(self) -> "Val":
        return Val(self.v.abs(), self.e)

    def bf16(self) -> "Val":
        """an operand rounding to bf16 inside the kernel (only where the header documents one); a no-op inside no_doc()"""
        return Val(self.v, self.e + (U16 * (self.v.abs() + self.e) if _DOC[0] else 0.0))

    def __getitem__(self, i) -> "Val":
        return Val(self.v[i], self.e[i])


_DOC = [True]


class no_doc:
    """with no_doc(): Val.bf16() adds nothing.  A case evaluates its formula twice; the difference of the two E is the share of the
    DOCUMENTED bf16 operand roundings, which check() keeps out of the discrimination cap (a 2^-8 term is of the size of an output
    ulp by nature: the cap guards the fp32 terms, the terms a case could inflate)."""

    def __enter__(self):
        _DOC[0] = False

    def __exit__(self, *exc):
        _DOC[0] = True


def where(cond, a, b) -> Val:
    a, b = Val.of(a)._pair(b)
    return Val(torch.where(cond, a.v, b.v), torch.where(cond, a.e, b.e))


def matmul(a64: torch.Tensor, bt64: torch.Tensor, alpha: float = 1.0) -> Val:
    """alpha * A B of exact bf16 operands through the MFMA pipeline (gemm_E)"""
    a64, bt64 = f64(a64), f64(bt64)
    return Val(alpha * (a64 @ bt64), gemm_E(a64, bt64, a64.shape[-1], alpha))


def matmul_val(a: Val, bt64: torch.Tensor, alpha: float = 1.0) -> Val:
    """the same with an inexact left operand (a documented operand rounding): its error rides through |B|"""
    bt64 = f64(bt64)
    return Val(alpha * (a.v @ bt64), gemm_E(a.v, bt64, a.v.shape[-1], alpha) + abs(alpha) * (a.e @ bt64.abs()))


def sigmoid(g, k: float = 1.0) -> Val:
    """1 / (1 + __expf(-k g)) as every kernel of the library writes it"""
    g = Val.of(g)
    return 1.0 / (1.0 + (-(g * Val.const(k) if k != 1.0 else g)).exp())


def gelu(z) -> Val:
    """0.5f * z * (1.f + erff(z * 0.70710678f)); the value is taken from erfc (1 + erf cancels in float64 too for z << 0)"""
    z = Val.of(z)
    r = Val.const(0.5) * z * (1.0 + (z * Val.const(math.sqrt(0.5))).erf())
    return Val(0.5 * z.v * torch.special.erfc(-z.v * math.sqrt(0.5)), r.e)


# ------------------------------------------------------------------------------------------------------------- input builders
def all_finite_bf16(device="cpu") -> torch.Tensor:
    """Every finite bf16 bit pattern (65,280 values, a multiple of 8), both zeros and all subnormals included."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    return bits.to(torch.int16).view(BF).to(device)


def bf16_midpoints(device="cpu"):
    """(fp32 inputs [3 n], expected bf16 bit patterns int32 [3 n]): for every pair of adjacent finite bf16 values of equal sign the
    fp32 midpoint (low half 0x8000) and its two fp32 neighbours (0x7FFF, 0x8001).  Expected values from integer arithmetic: below
    the midpoint the upper half stays, above it it grows by one, AT it it goes to the even neighbour.  A sum that passes the largest
    finite pattern is the infinity's (RNE overflow)."""
    hi = torch.arange(0, 1 << 16, dtype=torch.int64)
    hi = hi[(hi & 0x7F80) != 0x7F80]
    lo = torch.tensor([0x7FFF, 0x8000, 0x8001], dtype=torch.int64)
    bits = (hi[:, None] << 16) | lo[None, :]
    up = torch.stack([torch.zeros_like(hi), hi & 1, torch.ones_like(hi)], dim=1)
    want = hi[:, None] + up
    x = (bits.reshape(-1) & 0xFFFFFFFF)
    x = torch.where(x >= (1 << 31), x - (1 << 32), x).to(torch.int32).view(F32)
    return x.to(device), want.reshape(-1).to(torch.int32).to(device)


def randn_bf16(*shape, scale=1.0, seed=0, device="cpu") -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(device)


def eps_rows(rows: int, d: int, seed: int = 0, device="cpu", dtype=BF) -> torch.Tensor:
    """Norm inputs that enter the eps-dominated regime: N(0,1) rows, every fourth row scaled by 2^-10 (mean(x^2) ~ 1e-6, of the
    order of eps), row 1 all zero, row 2 constant (LayerNorm's variance is 0).  rows >= 5."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, d, generator=g)
    x[::4] *= 2.0 ** -10
    x[1] = 0.0
    x[2] = 0.8125
    return x.to(BF).to(dtype).to(device)


def cancelling_gemm(M: int, N: int, K: int, seed: int = 0, device="cpu"):
    """(a [M][K], b [N][K]) with cancelling outputs: a's paired columns hold (x, -x + small) and the rows n % 8 < 3 of b repeat
    their value over each pair, so those outputs are sums of small * b and sit below 2^-6 of sum |a b|; the other rows of b are N(0,1)
    and their outputs are ordinary.  (Three columns of eight, not every second one: the discrimination cap is a MEDIAN, and with
    exactly half of the elements cancelling it would sit on the seam between the two populations.)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K // 2, generator=g).to(BF).float()
    small = (torch.randn(M, K // 2, generator=g) * 2.0 ** -9)
    a = torch.stack([x, (-x + small * x.abs()).to(BF).float()], dim=2).reshape(M, K)
    b = torch.randn(N, K, generator=g)
    pair = torch.randn(N, K // 2, generator=g).repeat_interleave(2, dim=1)
    sel = (torch.arange(N) % 8) < 3
    b[sel] = pair[sel]
    return a.to(BF).to(device), b.to(BF).to(device)


def spiked_attention_rows(S: int, L: int, H: int, hd: int, seed: int = 0, device="cpu", kv_heads: Optional[int] = None):
    """q [S][H][L][hd], k, v [S][kv_heads][L][hd] (bf16) for the attention cases (S = 2; query head h reads kv head h * kv_heads // H):
    N(0,1) x 0.7 everywhere, and
      sequence 0, query head 0:     a LATE dominating key - the last key is 2 sign(q_last), so the last query's online softmax meets
                                    its maximum in the final tile and rescales at the end;
      sequence 0, query head H - 1: an EARLY dominating key - every query of the head carries a shared unit direction c (q += c) and
                                    key 0 of its kv head is (7.5 / sqrt(hd)) c (|c|^2 = hd): a scaled score of 7.5 for every query
                                    against scores of standard deviation ~ 0.9 elsewhere: P[:, 0] > 0.5 for (nearly) all queries, the
                                    maximum sits in the first tile, alpha = 1 and small p in every later tile;
      sequence 1, kv head 0:        the keys of the first quarter all equal: the queries there see a uniform softmax, out = mean v
                                    (the denominator);
      sequence 1, query head H - 1: q and the keys of its kv head at scale 3: nearly one-hot rows, raw q.k of about +-100.
    With kv_heads = 1 the rows of a sequence share the one kv head (late and early key at its two ends; the scale-3 keys keep their
    equal first quarter), so every row kind exists for kv_group = H as well.  tests/test_accuracy_helper.py asserts all of this."""
    kvh = kv_heads or H
    kv_of = lambda h: h * kvh // H                     # noqa: E731
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(S, H, L, hd, generator=g) * 0.7
    k = torch.randn(S, kvh, L, hd, generator=g) * 0.7
    v = torch.randn(S, kvh, L, hd, generator=g) * 0.7
    c = torch.sign(torch.randn(hd, generator=g))        # |c|^2 = hd
    q[0, H - 1] += c
    k[0, kv_of(H - 1), 0] = (7.5 / math.sqrt(hd)) * c   # (q_i . k_0) / sqrt(hd) = 7.5 + N(0, 0.5) for every query of head H - 1
    k[0, 0, L - 1] = 2.0 * torch.sign(q[0, 0, L - 1])
    if S > 1:
        q[1, H - 1] *= 3.0 / 0.7
        k[1, kv_of(H - 1)] *= 3.0 / 0.7
        k[1, 0, :max(1, L // 4)] = k[1, 0, 0]          # the queries of the first quarter see equal keys only
    return q.to(BF).to(device), k.to(BF).to(device), v.to(BF).to(device)


# ------------------------------------------------------------------------------------------------------------- attention bounds
def _score_terms(q, k, scale, allowed, extra_abs=0.0):
    """(s, P-independent relative error of exp(s - reference)): s = scale q.k^T in float64; the exponent t = fma(S, c, -m) with
    S from the MFMA over hd products (gemm_E), c = fl(scale * log2 e) (2 * 2^-24 |s|), the fma's rounding (2^-24 |s - m|, added
    by the caller who knows m) and v_exp_f32's 1 ulp (2 * 2^-24)"""
    hd = q.shape[-1]
    s = scale * (q @ k.transpose(-1, -2))
    ds = (MFMA_FACTOR * hd + 2) * U32 * scale * (q.abs() @ k.abs().transpose(-1, -2)) + 2.0 * U32 * s.abs() + 2.0 * U32 + extra_abs
    return torch.where(allowed, s, torch.full_like(s, -math.inf)), ds


def attn_fwd_bound(q, k, v, allowed, scale, tile: int = 64):
    """One head of rv_attn_fwd: q [Lq][hd], k, v [Lk][hd] (float64 copies of the bf16 operands), allowed bool [Lq][Lk] (every row
    sees at least one key).  Returns (out Val, doc, lse Val): out_i = sum_j bf16(p_ij) v_j / sum_j p_ij, lse_i = m_i + ln sum_j p_ij.
      doc  = 2^-8 sum_j P_ij |v_j|: P is rounded to bf16 for the PV MFMA (attention.hip pack_frag in the key loop; oracle/rounding.py
             point P); the row sum is taken from the UNROUNDED p (psum += p before the pack);
      score error rel_ij (see _score_terms) propagated: d out_i = sum_j P_ij (v_j - out_i) rel_ij, d lse_i = sum_j P_ij rel_ij.  The
             running maximum cancels (one fp32 number per row and tile serves numerator and denominator); each of the ceil(Lk / 64)
             tiles rescales o and l by the same alpha.  Per tile, in units of 2^-24: `out` sees the rounding of o * alpha (1) and of
             l * alpha (1) = 2; lse sees l * alpha (1) and alpha = exp2(m_old - m_new) itself, which does not cancel there: v_exp_f32's
             1 ulp (2) and the rounding of the difference, 2^-24 |m_old - m_new| weighted by the rescaled tile's share e^-|m_old - m_new|
             (x e^-x <= 1 / e: below 1) = 4.  rel carries 4 per tile for both;
      fp32 : the PV accumulation ((Lk + tiles) 2^-24 sum P |v|), the row sum (Lk 2^-24, relative), 1.f / l and the final product
             (2 * 2^-24 |out|), p below 2^-126 flushing (Lk * TINY * max |v|); lse: log2f FEW, the sum and the product by ln 2."""
    q, k, v = f64(q), f64(k), f64(v)
    Lk = k.shape[0]
    tiles = (Lk + tile - 1) // tile
    s, ds = _score_terms(q, k, scale, allowed)
    m = s.max(-1, keepdim=True).values
    rel = torch.where(allowed, ds + U32 * (s - m).abs() + 4.0 * U32 * tiles, torch.zeros_like(ds))
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    P = p / l
    out = P @ v
    Pv = P @ v.abs()
    doc = U16 * Pv
    # sum_j P_ij rel_ij |v_je - out_ie| for every column e: (P rel) @ |v| + ((P rel) 1) |out| bounds it without an [Lq][Lk][hd] tensor
    Pr = P * rel
    prop = (Pr @ v.abs() + Pr.sum(-1, keepdim=True) * out.abs()) * (1.0 + 2.0 * rel.max())
    E = doc + prop + (Lk + tiles) * U32 * Pv + (Lk + 2) * U32 * out.abs() + Lk * TINY * v.abs().max()
    lse = m + torch.log(l)
    E_lse = Pr.sum(-1, keepdim=True) + Lk * U32 + FEW * U32 * torch.log(l).abs() + 3.0 * U32 * lse.abs()
    return Val(out, E), doc, Val(lse[:, 0], E_lse[:, 0])


def attn_bwd_bound(q, k, v, dO, O, lse, allowed, scale):
    """One head of rv_attn_bwd (no RoPE): O and lse are the forward kernel's outputs, exact operands of this call.
      P_ij = exp2(S_ij c - lse_i log2 e): rel_ij of _score_terms plus the fma's 2^-24 |s - lse| plus, in the dQ kernel, 2 * 2^-24
             |lse_i| (lse * LOG2E in fp32), in the dK/dV kernel (hd + 4) 2^-24 |lse_i| (version 5 feeds -lse / scale, a workspace
             plane the dQ kernel writes next to delta, into the accumulator of the S MFMA: it rides through the hd-deep sum);
      dP_ij - delta_i: two hd-deep fp32 sums (the MFMA, and the fma chain of delta at the top of the dQ kernel): (hd + 2) 2^-24
             (|dO| |v|^T + sum |dO O|);  dS = P (dP - delta): 2 roundings;
      documented bf16 operand roundings, ONE per product (pack_frag of dS before the dQ / dK MFMAs, of P before the dV MFMA):
             dQ: 2^-8 scale sum_j |dS_ij| |k_j|;  dK: 2^-8 scale sum_i |dS_ij| |q_i|;  dV: 2^-8 sum_i P_ij |dO_i|;
      the MFMA accumulations over L terms and the final * scale.
    Returns {name: (Val, doc)} for dQ, dK, dV of this (query head, kv head) pair."""
    q, k, v, dO, O, lse = (f64(t) for t in (q, k, v, dO, O, lse))
    hd, Lq, Lk = q.shape[-1], q.shape[0], k.shape[0]
    s, ds = _score_terms(q, k, scale, allowed)
    lse = lse[:, None]
    rel_q = torch.where(allowed, ds + 2.0 * U32 * lse.abs() + U32 * (s - lse).abs(), torch.zeros_like(ds))       # the dQ kernel
    rel = torch.where(allowed, ds + (hd + 4) * U32 * lse.abs() + U32 * (s - lse).abs(), torch.zeros_like(ds))   # the dK / dV kernel
    P = torch.exp(s - lse)
    dP = dO @ v.transpose(-1, -2)
    delta = (dO * O).sum(-1, keepdim=True)
    E_dpd = (MFMA_FACTOR * hd + 2) * U32 * (dO.abs() @ v.abs().transpose(-1, -2) + (dO * O).abs().sum(-1, keepdim=True))
    dS = P * (dP - delta)
    E_dS = (P * rel * (dP - delta).abs() + P * E_dpd) * (1.0 + rel.max()) + 2.0 * U32 * dS.abs() + TINY
    E_dS_q = (P * rel_q * (dP - delta).abs() + P * E_dpd) * (1.0 + rel.max()) + 2.0 * U32 * dS.abs() + TINY
    E_P = P * rel + TINY
    res = {}
    aS, aP = dS.abs(), P
    doc = U16 * scale * (aS @ k.abs())
    res["dQ"] = (Val(scale * (dS @ k), doc + scale * (E_dS_q @ k.abs() + (Lk + 2) * U32 * (aS @ k.abs())) + U32 * scale * (dS @ k).abs()), doc)
    doc = U16 * scale * (aS.transpose(-1, -2) @ q.abs())
    res["dK"] = (Val(scale * (dS.transpose(-1, -2) @ q), doc + scale * (E_dS.transpose(-1, -2) @ q.abs() + (Lq + 2) * U32 *
                                                                   (aS.transpose(-1, -2) @ q.abs())) + U32 * scale * (dS.transpose(-1, -2) @ q).abs()), doc)
    doc = U16 * (aP.transpose(-1, -2) @ dO.abs())
    res["dV"] = (Val(P.transpose(-1, -2) @ dO, doc + E_P.transpose(-1, -2) @ dO.abs() + (Lq + 2) * U32 * (aP.transpose(-1, -2) @ dO.abs())), doc)
    return res


def rope_bwd_val(val: Val, doc: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor):
    """the inverse RoPE fused into the dQ / dK stores (attention.hip store_rope_bwd_pair): the values are FIRST ROUNDED TO BF16 (a
    documented operand rounding: what the separate rv_rope_inplace pass used to read back), then dx1 = a cos + b sin, dx2 = b cos - a
    sin in fp32 (two products and a sum: 3 * 2^-24 of |a cos| + |b sin|).  val [L][128], cos / sin [L][64] float64: (Val, doc)"""
    a, b = Val(val.v[:, :64], val.e[:, :64]).bf16(), Val(val.v[:, 64:], val.e[:, 64:]).bf16()
    da, db = doc[:, :64] + U16 * a.v.abs(), doc[:, 64:] + U16 * b.v.abs()
    ac, bs, bc, as_ = a.v * cos, b.v * sin, b.v * cos, a.v * sin
    e1 = a.e * cos.abs() + b.e * sin.abs() + 3.0 * U32 * (ac.abs() + bs.abs())
    e2 = b.e * cos.abs() + a.e * sin.abs() + 3.0 * U32 * (bc.abs() + as_.abs())
    d1, d2 = da * cos.abs() + db * sin.abs(), db * cos.abs() + da * sin.abs()
    return Val(torch.cat([ac + bs, bc - as_], 1), torch.cat([e1, e2], 1)), torch.cat([d1, d2], 1)


def emulate_attn_fwd(q, k, v, allowed, scale, online: bool = True, tile: int = 64, rescale_last: bool = True):
    """CPU emulation of the forward kernel's arithmetic: fp32 throughout, exp2 of fma(S, c, -m), P rounded to bf16 for the PV product,
    the row sum from the unrounded p; online (64-key tiles, running maximum, rescale) or plain (one pass).  Returns (out bf16, lse).
    rescale_last = False is a PLANTED DEFECT (tests/test_accuracy_helper.py): the last tile moves the maximum but o and l are not
    rescaled by alpha."""
    LOG2E, LN2 = torch.tensor(1.4426950408889634, dtype=F32), torch.tensor(0.6931471805599453, dtype=F32)
    qf, kf, vf = q.float(), k.float(), v.float()
    c = torch.tensor(scale, dtype=F32) * LOG2E
    S = qf @ kf.t()
    S = torch.where(allowed, S, torch.full_like(S, -math.inf))
    Lq, Lk = S.shape
    m = torch.full((Lq, 1), -math.inf)
    l = torch.zeros(Lq, 1)
    o = torch.zeros(Lq, v.shape[1])
    for k0 in (range(0, Lk, tile) if online else [0]):
        k1 = min(Lk, k0 + tile) if online else Lk
        St = S[:, k0:k1]
        m_new = torch.maximum(m, St.max(-1, keepdim=True).values * c)
        alpha = torch.where(torch.isinf(m_new), torch.ones_like(m), torch.exp2(m - m_new))
        if not rescale_last and k0 > 0 and k1 == Lk:
            alpha = torch.ones_like(m)
        neg_m = torch.where(torch.isinf(m_new), torch.zeros_like(m), -m_new)
        p = torch.exp2(St * c + neg_m)
        o = o * alpha + p.to(BF).float() @ vf[k0:k1]
        l = l * alpha + p.sum(-1, keepdim=True)
        m = m_new
    return (o * (1.0 / l)).to(BF), ((m + torch.log2(l)) * LN2)[:, 0]


def emulate_attn_bwd(q, k, v, dO, O, lse, allowed, scale):
    """CPU emulation of the backward kernels' arithmetic (fp32, dS and P rounded to bf16 for their MFMAs): (dQ, dK, dV) bf16"""
    LOG2E = torch.tensor(1.4426950408889634, dtype=F32)
    qf, kf, vf, dof = q.float(), k.float(), v.float(), dO.float()
    c = torch.tensor(scale, dtype=F32) * LOG2E
    S = torch.where(allowed, qf @ kf.t(), torch.tensor(-math.inf))
    P = torch.exp2(S * c - (lse.float() * LOG2E)[:, None])
    delta = (dof * O.float()).sum(-1, keepdim=True)
    dS = P * (dof @ vf.t() - delta)
    sc = torch.tensor(scale, dtype=F32)
    return (((dS.to(BF).float() @ kf) * sc).to(BF), ((dS.to(BF).float().t() @ qf) * sc).to(BF), (P.to(BF).float().t() @ dof).to(BF))


def causal_allowed(Lq: int, Lk: int, device="cpu", seg=None) -> torch.Tensor:
    """causal mask; seg = (sh, e1): queries at index >= e1 do not see the keys [sh, e1) (packed preference pairs)"""
    i, j = torch.arange(Lq, device=device)[:, None], torch.arange(Lk, device=device)[None, :]
    ok = j <= i
    if seg is not None:
        ok = ok & ~((i >= seg[1]) & (j >= seg[0]) & (j < seg[1]))
    return ok


def full_allowed(Lq: int, Lk: int, device="cpu", seg=None) -> torch.Tensor:
    """non-causal mask (rv_attn_fwd / rv_attn_bwd with causal = 0): every query sees every key; seg = (sh, e1): the window still
    applies - queries at index >= e1 do not see the keys [sh, e1).  Together with causal_allowed this is the kernels' documented
    predicate (attention.hip, "Element masks"): hidden(q, key) <=> key >= L || (CAUSAL && key > q) || (q >= e1 && sh <= key < e1).
    Lq != Lk: the first Lq queries of a row of Lk keys (the Resampler's live queries)."""
    i, j = torch.arange(Lq, device=device)[:, None], torch.arange(Lk, device=device)[None, :]
    ok = torch.ones(Lq, Lk, dtype=torch.bool, device=device)
    if seg is not None:
        ok = ok & ~((i >= seg[1]) & (j >= seg[0]) & (j < seg[1]))
    return ok


# ------------------------------------------------------------------------------------------------------------- LM head bounds
def lmhead_bound(h, w, tgt, v_valid: int):
    """rv_lmhead_logp_fwd + rv_logp_finish: logits x = h w^T over K products (dlogit = (K + 4) 2^-24 sum |h| |w|); per 64-column
    block mx_b, sum_n __expf(x_n - mx_b); finish: mx = max_b mx_b, s = sum_b psum_b __expf(mx_b - mx), lse = mx + logf(s), logp =
    x_tgt - lse.  Every exponent carries the rounding of its difference (2^-24 times the distance) and exp_rel; the maxima cancel
    (the same fp32 number on both sides); the sums run over 64 + V / 64 terms; logf FEW.  Per term, in units of 2^-24: the two
    differences x - mx_b and mx_b - mx round once each (1 * dist in total) and exp_rel of the two __expf is 2 (|arg| + 2) each = 2 *
    dist + 8: 3 * dist + 8; the product psum_b * __expf(mx_b - mx) rounds once: + 1 = 9.
    Returns (logp Val, lse Val, logits float64, dlogit) for the rows with 0 <= tgt < v_valid (the others: lse only is meaningful)."""
    h, w = f64(h), f64(w)
    K, V = h.shape[1], w.shape[0]
    x = h @ w.t()
    dlogit = (MFMA_FACTOR * K + 4) * U32 * (h.abs() @ w.abs().t())
    valid = torch.arange(V, device=x.device)[None, :] < v_valid
    xm = torch.where(valid, x, torch.full_like(x, -math.inf))
    mxb = xm.view(x.shape[0], V // 64, 64).max(-1, keepdim=True).values.expand(-1, -1, 64).reshape(x.shape)
    mx = xm.max(-1, keepdim=True).values
    dist = torch.where(valid, (xm - mxb).abs() + (mxb - mx).abs(), torch.zeros_like(x))
    rel = torch.where(valid, dlogit + 3.0 * U32 * dist + 9.0 * U32, torch.zeros_like(x))
    P = torch.softmax(xm, -1)
    lse = torch.logsumexp(xm, -1)
    E_lse = (P * rel).sum(-1) + (64 + V // 64) * U32 + FEW * U32 * (lse - mx[:, 0]).abs() + U32 * lse.abs()
    t = tgt.long().clamp(0, V - 1)
    xt, dt = x.gather(1, t[:, None])[:, 0], dlogit.gather(1, t[:, None])[:, 0]
    logp = xt - lse
    return Val(logp, dt + E_lse + U32 * logp.abs()), Val(lse, E_lse), x, dlogit


def lmhead_bwd_bound(h, w, tgt, lse, coef, v_valid: int) -> Val:
    """rv_lmhead_logp_bwd: dlogits = coef ((n == tgt) - __expf(x - lse)) with the forward's lse as an exact operand: p carries
    dlogit, the rounding of x - lse and exp_rel; then the subtraction (where 1 - p cancels as p -> 1) and the product"""
    h, w, lse, coef = f64(h), f64(w), f64(lse)[:, None], f64(coef)[:, None]
    K, V = h.shape[1], w.shape[0]
    x = Val(h @ w.t(), (MFMA_FACTOR * K + 4) * U32 * (h.abs() @ w.abs().t()))
    p = (x - lse).exp()
    onehot = (torch.arange(V, device=lse.device)[None, :] == tgt.long()[:, None]).double()
    d = coef * (onehot - p)
    valid = torch.arange(V, device=lse.device)[None, :] < v_valid
    return where(valid, d, Val(torch.zeros_like(d.v)))


def emulate_lmhead(h, w, tgt, v_valid: int):
    """CPU emulation of the LM-head forward + finish in fp32 (block partials, then the combine): (logp, lse)"""
    x = h.float() @ w.float().t()
    V = x.shape[1]
    x = torch.where(torch.arange(V)[None, :] < v_valid, x, torch.tensor(-math.inf))
    xb = x.view(x.shape[0], V // 64, 64)
    pmax = xb.max(-1).values
    psum = torch.exp(xb - pmax[..., None]).sum(-1)
    mx = pmax.max(-1, keepdim=True).values
    s = (psum * torch.exp(pmax - mx)).sum(-1)
    lse = mx[:, 0] + torch.log(s)
    return x.gather(1, tgt.long().clamp(0, V - 1)[:, None])[:, 0] - lse, lse


def lmhead_inputs(n: int = 70, d: int = 64, V: int = 128, v_valid: int = 121, seed: int = 0, device="cpu"):
    """(h [n][d], w [V][d], tgt int32 [n]): logits spanning about +-40 (h ~ N(0,1), w ~ 1.5 N(0,1) over d = 64: standard deviation
    12); targets: rows 0-9 the row's argmax, the row being 0.16 times one row of w (its logit ~ 24, the others ~ N(0, 3): logp ~ -1e-6
    and closer to 0: absolute accuracy), rows 10-19 the row's smallest logit (logp ~ -60), then id 0, id v_valid - 1, -100 (no
    vocabulary id), the rest random valid ids"""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(n, d, generator=g)
    w = torch.randn(V, d, generator=g) * 1.5
    h[:10] = 0.16 * w[torch.arange(10) * 11 + 3]
    h, w = h.to(BF), w.to(BF)
    x = h.double() @ w.double().t()
    x[:, v_valid:] = -math.inf
    tgt = torch.randint(0, v_valid, (n,), generator=g)
    tgt[:10] = x[:10].argmax(-1)
    x[:, v_valid:] = math.inf
    tgt[10:20] = x[10:20].argmin(-1)
    tgt[20], tgt[21], tgt[22] = 0, v_valid - 1, -100
    return h.to(device), w.to(device), tgt.to(torch.int32).to(device)
