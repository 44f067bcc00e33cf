"""Guard-band buffers for the containment tests (plain helper module, imported by putting the tests directory on sys.path like
autocheck_case.py and full_depth.py; works on CPU and GPU tensors alike).

guarded_2d(rows, cols, dtype, device) gives a [rows][cols] WINDOW of a larger allocation: GUARD rows above and below, GUARD elements
left and right (ld = cols + 2 * GUARD, rounded up to `ld_multiple`), the window itself starting on a 16-byte boundary.  GUARD = 256 is
one full tile of the largest kernel (256 x 256), so a one-tile overshoot lands in the band - inside the allocation - where check()
sees it.  Everything outside the window holds a sentinel bit pattern (a quiet NaN with a payload for bf16 / fp32, a fixed negative
value for int32); with fill=None the window holds it too (a pure output), else a copy of `fill` (input, in/out operand).
`inner` marks window elements that stay guard as well (the gap between q | k | v column ranges, token rows no sequence owns, rows
that row_idx does not name): they are sentinel from the start, whatever `fill` holds there, and check() wants them untouched.

The three roles have three different patterns - "in" (read-only operand; the default with a fill), "io" (in/out operand), "out" (pure
output or workspace; the default without a fill) - and no fp32 pattern turns into a bf16 one when a kernel truncates or rounds it:
an overshooting store whose VALUE is somebody's poison (a gather that copies an input's guard, a sum that ran into an fp32
workspace's guard) still changes the bits of the guard it lands in.

clean=True builds the same geometry (same ld, same alignment of the window, same `inner`) over ZEROS instead of the sentinel for the
operands a kernel reads ("in", "io"): the "clean layout" of a poisoned-input comparison.  A kernel whose outputs differ between the
two layouts, or hold a NaN in the poisoned one, reads memory it has no business reading.  Pure outputs keep their sentinel in both.

check() compares the whole guard region bit for bit (on an integer view) with what was put there and raises GuardError naming the
operand, the edge (above / below / left / right / inside), the first offending index relative to the window and the number of changed
elements.  check(written=...) also asserts that no sentinel is left where the contract says the kernel writes (True = the whole
window outside `inner`, or a boolean mask): the call was not a no-op."""
from typing import Callable, Optional, Tuple

import torch

GUARD = 256            # guard rows above / below and guard elements left / right of a 2-D window
GUARD_1D = 4096        # guard elements before / after a flat buffer

_INT_VIEW = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.int32: torch.int32, torch.uint8: torch.uint8}
# quiet NaNs with a payload (bf16: 0x7FC0 | payload, fp32: 0x7FC00000 | payload); the upper halves of the fp32 patterns, truncated
# (0x7FC7, 0x7FCD, 0x7FD1) or rounded up (0x7FC8, 0x7FCE, 0x7FD2), are none of the bf16 patterns, and no bf16 pattern widened to
# fp32 (low half zero) is an fp32 pattern.  No kernel of the library produces any of them.
SENTINELS = {"in": {torch.bfloat16: 0x7FE5, torch.float32: 0x7FC7A5A5, torch.int32: -0x5A5A5A5B, torch.uint8: 0xA5},
             "io": {torch.bfloat16: 0x7FD9, torch.float32: 0x7FCDA5A5, torch.int32: -0x3C3C3C3D, torch.uint8: 0x5A},
             "out": {torch.bfloat16: 0x7FF3, torch.float32: 0x7FD1A5A5, torch.int32: -0x69696969, torch.uint8: 0xC3}}


class GuardError(AssertionError):
    pass


class Guarded:
    """One guarded operand.  .view is the window (a strided view of the parent allocation in the operand's dtype)."""

    def __init__(self, rows: int, cols: int, dtype, device, fill=None, name: str = "buffer", clean: bool = False, inner=None,
                 ld_multiple: int = 1, guard_rows: int = GUARD, guard_cols: int = GUARD, role: Optional[str] = None):
        if dtype not in _INT_VIEW:
            raise TypeError(f"guarded buffers hold bf16, fp32, int32 or uint8, not {dtype}")
        role = role or ("out" if fill is None else "in")
        if role not in SENTINELS or (role == "out") != (fill is None):
            raise ValueError("role: 'in' / 'io' with a fill, 'out' without")
        self.name, self.rows, self.cols, self.dtype, self.role = name, rows, cols, dtype, role
        self.clean = clean = clean and role != "out"
        self.gr, self.gc = guard_rows, guard_cols
        self.ld = -(-(cols + 2 * guard_cols) // ld_multiple) * ld_multiple
        self.idtype = _INT_VIEW[dtype]
        self.sentinel = SENTINELS[role][dtype]
        self.background = 0 if clean else self.sentinel
        item = torch.empty(0, dtype=dtype).element_size()
        per16 = max(1, 16 // item)
        body = (rows + 2 * guard_rows) * self.ld
        self._flat = torch.full((body + per16,), self.background, dtype=self.idtype, device=device)
        # shift the body so that the WINDOW's first element sits on a 16-byte boundary
        win = guard_rows * self.ld + guard_cols
        self.off = next(o for o in range(per16) if ((self._flat.data_ptr() // item + o + win) % per16) == 0)
        self._body = self._flat[self.off:self.off + body].view(rows + 2 * guard_rows, self.ld)
        self._iwin = self._body[guard_rows:guard_rows + rows, guard_cols:guard_cols + cols]
        self.view = self._flat.view(dtype)[self.off:self.off + body].view(rows + 2 * guard_rows, self.ld)[
            guard_rows:guard_rows + rows, guard_cols:guard_cols + cols]
        assert self.view.data_ptr() % 16 == 0
        self.inner = None
        if fill is None:
            self._iwin.fill_(self.sentinel)
        else:
            self.view.copy_(torch.as_tensor(fill).to(device=device, dtype=dtype).reshape(rows, cols))
        if inner is not None:
            self.inner = torch.as_tensor(inner).to(device=device, dtype=torch.bool).expand(rows, cols).clone()
            self._iwin[self.inner] = self.background

    # ------------------------------------------------------------------ checks
    def _report(self, edge: str, bad: torch.Tensor, r0: int, c0: int):
        idx = bad.nonzero()
        first = idx[0].tolist()
        raise GuardError(f"{self.name}: guard {edge} the window changed: {idx.shape[0]} element(s), first at window index "
                         f"(row {first[0] + r0}, col {first[1] + c0}) of a [{self.rows}][{self.cols}] window (ld {self.ld})")

    def check(self, written=None) -> None:
        gr, gc, R, C, b = self.gr, self.gc, self.rows, self.cols, self._body
        regions = (("above", b[:gr], -gr, -gc), ("below", b[gr + R:], R, -gc),
                   ("left of", b[gr:gr + R, :gc], 0, -gc), ("right of", b[gr:gr + R, gc + C:], 0, C))
        for edge, reg, r0, c0 in regions:
            bad = reg != self.background
            if bool(bad.any()):
                self._report(edge, bad, r0, c0)
        head, tail = self._flat[:self.off], self._flat[self.off + b.numel():]
        if bool((head != self.background).any()):
            raise GuardError(f"{self.name}: guard above the window changed: alignment slack in front of the guard rows")
        if bool((tail != self.background).any()):
            raise GuardError(f"{self.name}: guard below the window changed: alignment slack behind the guard rows")
        if self.inner is not None:
            bad = (self._iwin != self.background) & self.inner
            if bool(bad.any()):
                self._report("inside", bad, 0, 0)
        if written is not None and written is not False:
            want = torch.ones(R, C, dtype=torch.bool, device=self._flat.device) if written is True else \
                torch.as_tensor(written).to(device=self._flat.device, dtype=torch.bool).expand(R, C)
            if self.inner is not None:
                want = want & ~self.inner
            left = (self._iwin == self.sentinel) & want
            if bool(left.any()):
                idx = left.nonzero()
                raise GuardError(f"{self.name}: {idx.shape[0]} element(s) the kernel must write still hold the sentinel, first at "
                                 f"window index (row {idx[0][0].item()}, col {idx[0][1].item()}): the call wrote nothing there")

    def untouched(self) -> torch.Tensor:
        """bool [rows][cols]: window elements that still hold the sentinel bit pattern."""
        return self._iwin == self.sentinel

    def bits(self) -> torch.Tensor:
        """A copy of the window on the integer view (for bit-for-bit comparisons, NaN-safe)."""
        return self._iwin.clone()


def guarded_2d(rows: int, cols: int, dtype, device, fill=None, **kw) -> Tuple[torch.Tensor, Callable]:
    g = Guarded(rows, cols, dtype, device, fill=fill, **kw)
    return g.view, g.check


def guarded_1d(n: int, dtype, device, fill=None, **kw) -> Tuple[torch.Tensor, Callable]:
    """The same for flat buffers (lse, delta, pmax / psum, workspaces, optimizer slices): n elements with GUARD_1D guard elements
    before ("left of") and after ("right of") them."""
    g = guarded_1d_obj(n, dtype, device, fill=fill, **kw)
    return g.flat, g.check


def guarded_1d_obj(n: int, dtype, device, fill=None, **kw) -> "Guarded":
    if fill is not None:
        fill = torch.as_tensor(fill).reshape(1, n)
    if kw.get("inner") is not None:
        kw["inner"] = torch.as_tensor(kw["inner"]).reshape(1, n)
    g = Guarded(1, n, dtype, device, fill=fill, guard_rows=0, guard_cols=GUARD_1D, **kw)
    g.flat = g.view[0]
    return g
