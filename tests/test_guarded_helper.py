"""Host tests of tests/guarded.py (CPU tensors): a planted one-element write one past each edge of the window, and one in the far
corner of the band, is reported with the operand's name and the edge; an untouched buffer passes; the "kernel wrote its output"
check fires on a window nothing wrote."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded as G  # noqa: E402

DTYPES = [torch.bfloat16, torch.float32, torch.int32]
ROWS, COLS = 5, 24


def _parent(g):
    """the whole allocation behind a Guarded as [rows + 2 GUARD][ld] in the operand's dtype (what a stray kernel write would hit)"""
    return g.view.as_strided((g.rows + 2 * g.gr, g.ld), (g.ld, 1), g.view.storage_offset() - g.gr * g.ld - g.gc)


def _poke(g, r, c):
    """one-element write at window-relative (r, c)"""
    _parent(g)[g.gr + r, g.gc + c] = 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("clean", [False, True])
def test_untouched_buffer_passes(dtype, clean):
    x = torch.arange(ROWS * COLS).reshape(ROWS, COLS).to(dtype)
    g = G.Guarded(ROWS, COLS, dtype, "cpu", fill=x, name="x", clean=clean)
    assert g.view.shape == (ROWS, COLS) and g.view.stride() == (COLS + 2 * G.GUARD, 1)
    assert g.view.data_ptr() % 16 == 0
    assert torch.equal(g.view, x)
    g.check()
    g.check(written=True)          # a filled window holds no sentinel
    view, check = G.guarded_2d(ROWS, COLS, dtype, "cpu", fill=x)
    assert torch.equal(view, x)
    check()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("role", ["in", "io"])
def test_guard_holds_the_sentinel_and_the_clean_layout_has_the_same_geometry(dtype, role):
    x = torch.ones(ROWS, COLS)
    p = G.Guarded(ROWS, COLS, dtype, "cpu", fill=x, name="p", role=role)
    c = G.Guarded(ROWS, COLS, dtype, "cpu", fill=x, name="c", role=role, clean=True)
    o = G.Guarded(ROWS, COLS, dtype, "cpu", name="o", clean=True)        # a pure output keeps its sentinel in the clean layout
    assert p.ld == c.ld == o.ld and p.view.stride() == c.view.stride() == o.view.stride()
    assert p.view.data_ptr() % 16 == c.view.data_ptr() % 16 == o.view.data_ptr() % 16 == 0
    for g in (p, c):
        outside = _parent(g).clone()
        assert bool((outside[g.gr:g.gr + ROWS, g.gc:g.gc + COLS] == 1).all())
        outside[g.gr:g.gr + ROWS, g.gc:g.gc + COLS] = 0 if g is c else outside[0, 0]
        if g is c:
            assert bool((outside == 0).all())
        elif dtype.is_floating_point:
            assert bool(torch.isnan(outside).all())
        else:
            assert bool((outside == G.SENTINELS[role][dtype]).all()) and G.SENTINELS[role][dtype] < 0
    po = _parent(o)
    assert bool(torch.isnan(po).all()) if dtype.is_floating_point else bool((po == G.SENTINELS["out"][dtype]).all())


def test_sentinel_patterns_do_not_turn_into_each_other():
    """A kernel that rounds or truncates an fp32 poison to bf16, or widens a bf16 poison to fp32, must not reproduce a guard."""
    bf = {r: G.SENTINELS[r][torch.bfloat16] for r in G.SENTINELS}
    f32 = {r: G.SENTINELS[r][torch.float32] for r in G.SENTINELS}
    assert len(set(bf.values())) == 3 and len(set(f32.values())) == 3
    for v in f32.values():
        t = torch.tensor([v], dtype=torch.int32).view(torch.float32)
        assert bool(torch.isnan(t).all())
        assert (v >> 16) not in bf.values() and ((v >> 16) + 1) not in bf.values()
        assert int(t.to(torch.bfloat16).view(torch.int16)) not in bf.values()
    for v in bf.values():
        t = torch.tensor([v], dtype=torch.int16).view(torch.bfloat16)
        assert bool(torch.isnan(t).all()) and (v << 16) not in f32.values()
        assert int(t.float().view(torch.int32)) not in f32.values()
    for dt in (torch.int32, torch.uint8):
        assert len({G.SENTINELS[r][dt] for r in G.SENTINELS}) == 3


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("clean", [False, True])
@pytest.mark.parametrize("edge,r,c", [("above", -1, 0), ("below", ROWS, COLS - 1), ("left of", 0, -1), ("right of", ROWS - 1, COLS),
                                      ("above", -G.GUARD, -G.GUARD), ("below", ROWS + G.GUARD - 1, COLS + G.GUARD - 1)])
def test_planted_write_is_reported_with_name_edge_index_and_count(dtype, clean, edge, r, c):
    g = G.Guarded(ROWS, COLS, dtype, "cpu", fill=torch.zeros(ROWS, COLS), name="operand_q", clean=clean)
    _poke(g, r, c)
    with pytest.raises(G.GuardError) as e:
        g.check()
    msg = str(e.value)
    assert "operand_q" in msg and f"guard {edge} the window" in msg
    assert f"(row {r}, col {c})" in msg and "1 element(s)" in msg


def test_count_and_first_index_of_a_wider_overshoot():
    g = G.Guarded(ROWS, COLS, torch.bfloat16, "cpu", name="c_out")
    for c in range(COLS, COLS + 8):               # an unmasked 8-wide vector store past the last column of rows 2 and 3
        _poke(g, 2, c)
        _poke(g, 3, c)
    with pytest.raises(G.GuardError, match=r"c_out: guard right of the window changed: 16 element\(s\), first at window index "
                                           rf"\(row 2, col {COLS}\)"):
        g.check()


def test_flat_buffer_edges():
    x = torch.arange(40, dtype=torch.float32)
    flat, check = G.guarded_1d(40, torch.float32, "cpu", fill=x)
    assert flat.shape == (40,) and flat.data_ptr() % 16 == 0 and torch.equal(flat, x)
    check()
    g = G.guarded_1d_obj(40, torch.float32, "cpu", fill=x, name="lse")
    g.flat.as_strided((1,), (1,), g.flat.storage_offset() + 40)[0] = 3.0
    with pytest.raises(G.GuardError, match=r"lse: guard right of the window.*\(row 0, col 40\)"):
        g.check()
    g = G.guarded_1d_obj(40, torch.float32, "cpu", fill=x, name="lse")
    g.flat.as_strided((1,), (1,), g.flat.storage_offset() - 1)[0] = 3.0
    with pytest.raises(G.GuardError, match=r"lse: guard left of the window.*\(row 0, col -1\)"):
        g.check()


def test_inner_guard_elements():
    """Gaps inside the window (between q | k | v, rows no sequence owns) start as guard whatever `fill` holds, and are checked."""
    inner = torch.zeros(ROWS, COLS, dtype=torch.bool)
    inner[:, 8:16] = True
    inner[3] = True
    x = torch.ones(ROWS, COLS)
    g = G.Guarded(ROWS, COLS, torch.bfloat16, "cpu", fill=x, name="qkv", inner=inner)
    assert bool(torch.isnan(g.view[inner]).all()) and bool((g.view[~inner] == 1).all())
    g.check()
    g.view[3, 20] = 0.5
    with pytest.raises(G.GuardError, match=r"qkv: guard inside the window changed: 1 element\(s\).*\(row 3, col 20\)"):
        g.check()
    z = G.Guarded(ROWS, COLS, torch.bfloat16, "cpu", fill=x, name="qkv", inner=inner, clean=True)
    assert bool((z.view[inner] == 0).all())
    z.check()
    o = G.Guarded(ROWS, COLS, torch.bfloat16, "cpu", name="dqkv", inner=inner)
    o.view[~inner] = 3.0
    o.check(written=True)                                       # the gaps are not the kernel's to write
    o.view[0, 9] = 3.0
    with pytest.raises(G.GuardError, match=r"dqkv: guard inside the window changed"):
        o.check(written=True)


def test_written_check_fires_on_a_window_never_written():
    g = G.Guarded(ROWS, COLS, torch.float32, "cpu", name="y")
    g.check()                                       # guards intact ...
    with pytest.raises(G.GuardError, match=rf"y: {ROWS * COLS} element\(s\) the kernel must write still hold the sentinel"):
        g.check(written=True)                       # ... but nothing was written
    g.view[:, :COLS - 1] = 2.0
    with pytest.raises(G.GuardError, match=rf"y: {ROWS} element\(s\).*\(row 0, col {COLS - 1}\)"):
        g.check(written=True)
    mask = torch.ones(ROWS, COLS, dtype=torch.bool)
    mask[:, COLS - 1] = False
    g.check(written=mask)                           # the contract leaves the last column alone: passes
    assert bool(g.untouched()[:, COLS - 1].all()) and not bool(g.untouched()[:, :COLS - 1].any())
    g.view[:, COLS - 1] = 2.0
    g.check(written=True)


def test_rejects_other_dtypes_and_roles():
    with pytest.raises(TypeError):
        G.Guarded(2, 8, torch.float64, "cpu")
    with pytest.raises(ValueError):
        G.Guarded(2, 8, torch.float32, "cpu", role="out", fill=torch.zeros(2, 8))
    with pytest.raises(ValueError):
        G.Guarded(2, 8, torch.float32, "cpu", role="io")
