"""rv_attn_fwd_branches: causal attention over rows [shared prefix | branch 0 | ... | branch N-1].

Shapes: row A = prefix 70 + branches [5, 17, 150, 40, 90, 33] (L = 405), row B = prefix 0 + branches [1, 64, 31, 130]
(L = 226) - the smallest that have a prefix that is no multiple of the 64-key tile, a 32-query wave over three branches
(queries 64..95 of row A: prefix, 5, 17, 150), a 128-query block inside one branch with a fully hidden key tile (row B,
queries 128..225 lie in the last branch, whose queries never see keys 0..95, so tile 0 is skipped by the block), a one-token
branch and seg_sh = 0.

  1. against dense fp32 masked attention on the same bf16 inputs, with the bound tests/test_kernels_gpu.py uses for the
     existing forward (``close(out, ref, rel=2e-2)``, ``assert_close(lse, ref, rtol=1e-3, atol=2e-3)``); a wrong mask is an
     error of order one;
  2. isolation, no tolerance: new q / k / v rows in branch j change nothing outside branch j;
  3. reduction, no tolerance: two branches = rv_attn_fwd(seg_sh, seg_e1), one branch = plain causal rv_attn_fwd, bit for bit
     (the same main loop visits the same key tiles in the same order; a tile one kernel skips and the other multiplies under
     a full mask adds exp2(-inf) = 0 and leaves the running maximum alone);
  4. no NaN / Inf in out or lse (the all-masked first tiles of row B meet a running maximum of -inf)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
HD = 128
ROWS = [(70, [5, 17, 150, 40, 90, 33]), (0, [1, 64, 31, 130])]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    _dev()
    from rlaif_v_amd import ops as o
    return o


def close(got, ref, rel, what):
    """tests/test_kernels_gpu.py ``close``: max error against rel * max |ref|, mean error against half of that."""
    got, ref = got.float(), ref.float()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err, mag = (got - ref).abs().max().item(), ref.abs().max().item()
    print(f"{what}: max err {err:.3e} of {mag:.3e}")
    assert err <= rel * mag + 1e-6, f"{what}: max err {err:.4e} vs max |ref| {mag:.4e}"
    merr, mmag = (got - ref).abs().mean().item(), ref.abs().mean().item()
    assert merr <= 0.5 * rel * mmag + 1e-7, f"{what}: mean err {merr:.4e} vs mean |ref| {mmag:.4e}"


def _q_lo(sh, branches, L=None):
    """q_lo of one row (pads behind the row continue its last branch, as the plan builder lays them out)."""
    out, n = [0] * sh, sh
    for b in branches:
        out += [n] * b
        n += b
    if L is not None:
        out += [out[-1]] * (L - len(out))
    return out


def _layout(pad_free):
    lens = [sh + sum(br) for sh, br in ROWS]
    L = max(lens)
    if pad_free:
        q_lo = sum((_q_lo(sh, br) for sh, br in ROWS), [])
        off = [0, lens[0]]
        return L, lens, off, q_lo, sum(lens)
    q_lo = sum((_q_lo(sh, br, L) for sh, br in ROWS), [])
    return L, [L, L], [0, L], q_lo, 2 * L


def _run(ops, qkv, H, G, pad_free, dev):
    L, lens, off, q_lo, _ = _layout(pad_free)
    Hkv = H // G
    sh = torch.tensor([r[0] for r in ROWS], dtype=torch.int32, device=dev)
    ql = torch.tensor(q_lo, dtype=torch.int32, device=dev)
    rows = (torch.tensor(off, dtype=torch.int32, device=dev), torch.tensor(lens, dtype=torch.int32, device=dev)) if pad_free else None
    return ops.attn_fwd(qkv, 2, L, H, HD, True, 0, H * HD, (H + Hkv) * HD, kv_group=G, rows=rows, branches=(sh, ql))


def _dense(qkv, H, G, pad_free):
    """fp32 masked attention per row on the CPU: (out [tokens, H*hd], lse list of [H, len])."""
    L, lens, off, q_lo, n_tok = _layout(pad_free)
    Hkv = H // G
    x = qkv.float().cpu()
    outs, lses = [], []
    for s, (sh, _) in enumerate(ROWS):
        n = lens[s]
        blk = x[off[s]:off[s] + n]
        q = blk[:, :H * HD].view(n, H, HD).transpose(0, 1)
        k = blk[:, H * HD:(H + Hkv) * HD].view(n, Hkv, HD).transpose(0, 1).repeat_interleave(G, 0)
        v = blk[:, (H + Hkv) * HD:].view(n, Hkv, HD).transpose(0, 1).repeat_interleave(G, 0)
        i = torch.arange(n)[:, None]
        j = torch.arange(n)[None, :]
        lo = torch.tensor(q_lo[off[s]:off[s] + n])[:, None]
        ok = (j <= i) & ((j < sh) | (j >= lo))
        sc = (q @ k.transpose(-1, -2)) / math.sqrt(HD) + torch.where(ok, 0.0, float("-inf"))
        outs.append((torch.softmax(sc, -1) @ v).transpose(0, 1).reshape(n, H * HD))
        lses.append(torch.logsumexp(sc, -1))
    return torch.cat(outs), lses


_CACHE = {}


def _case(ops, H, G, pad_free, dev):
    """(qkv, out, lse, dense out, dense lse) computed once per configuration and shared, never modified."""
    key = (H, G, pad_free)
    if key not in _CACHE:
        n_tok = _layout(pad_free)[4]
        g = torch.Generator().manual_seed(17 + H)
        qkv = (torch.randn(n_tok, (H + 2 * (H // G)) * HD, generator=g) * 0.7).to(BF).to(dev)
        out, lse = _run(ops, qkv, H, G, pad_free, dev)
        _CACHE[key] = (qkv, out, lse) + _dense(qkv, H, G, pad_free)
    return _CACHE[key]


@pytest.mark.parametrize("H,G,pad_free", [(2, 1, True), (2, 1, False), (4, 2, True)])
def test_against_dense_masked_attention(ops, H, G, pad_free):
    dev = _dev()
    qkv, out, lse, ro, rl = _case(ops, H, G, pad_free, dev)
    L, lens, off, _, _ = _layout(pad_free)
    assert torch.isfinite(out.float()).all()
    close(out.cpu(), ro, rel=2e-2, what=f"branches fwd H{H} G{G} pad_free={pad_free}")
    for s in range(2):
        got = lse[s, :, :lens[s]].cpu()
        assert torch.isfinite(got).all()
        torch.testing.assert_close(got, rl[s], rtol=1e-3, atol=2e-3)


@pytest.mark.parametrize("pad_free", [True, False])
def test_branch_isolation_is_exact(ops, pad_free):
    dev = _dev()
    H, G = 2, 1
    qkv, out, lse, _, _ = _case(ops, H, G, pad_free, dev)
    L, lens, off, _, _ = _layout(pad_free)
    g = torch.Generator().manual_seed(99)
    for s, (sh, branches) in enumerate(ROWS):
        real = sh + sum(branches)
        b0 = sh
        for j, b in enumerate(branches):
            mod = qkv.clone()
            mod[off[s] + b0:off[s] + b0 + b] = (torch.randn(b, qkv.shape[1], generator=g) * 0.7).to(BF).to(dev)
            o2, l2 = _run(ops, mod, H, G, pad_free, dev)
            keep = torch.ones(qkv.shape[0], dtype=torch.bool, device=dev)
            keep[off[s] + b0:off[s] + b0 + b] = False
            if not pad_free and j == len(branches) - 1:
                keep[off[s] + real:off[s] + L] = False                   # the pads behind a row continue its last branch
            assert torch.equal(o2[keep], out[keep]), f"row {s} branch {j}: out changed outside the branch"
            for r in range(2):
                n = lens[r] if pad_free else ROWS[r][0] + sum(ROWS[r][1])
                kr = torch.ones(n, dtype=torch.bool, device=dev)
                if r == s:
                    kr[b0:b0 + b] = False
                assert torch.equal(l2[r, :, :n][:, kr], lse[r, :, :n][:, kr]), f"row {s} branch {j}: lse changed outside the branch"
            assert torch.isfinite(o2.float()).all()
            b0 += b


@pytest.mark.parametrize("hd,L,segs", [(128, 333, [(130, 260), (129, 131)]), (128, 900, [(100, 500), (64, 448), (0, 256), (130, 131)]),
                                       (64, 300, [(0, 40), (0, 100)])])
def test_two_branches_equal_the_packed_pair_kernel(ops, hd, L, segs):
    """q_lo derived from seg_e1: the chosen branch starts at seg_sh, the rejected branch at seg_e1."""
    dev = _dev()
    S, H = len(segs), 2
    g = torch.Generator().manual_seed(L)
    qkv = (torch.randn(S * L, 3 * H * hd, generator=g) * 0.7).to(BF).to(dev)
    sh = torch.tensor([a for a, _ in segs], dtype=torch.int32, device=dev)
    e1 = torch.tensor([b for _, b in segs], dtype=torch.int32, device=dev)
    q_lo = torch.tensor(sum(([0] * a + [a] * (b - a) + [b] * (L - b) for a, b in segs), []), dtype=torch.int32, device=dev)
    ref_o, ref_l = ops.attn_fwd(qkv, S, L, H, hd, True, 0, H * hd, 2 * H * hd, seg=(sh, e1))
    out, lse = ops.attn_fwd(qkv, S, L, H, hd, True, 0, H * hd, 2 * H * hd, branches=(sh, q_lo))
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    assert torch.equal(out, ref_o) and torch.equal(lse, ref_l)


@pytest.mark.parametrize("hd,lens,sh", [(128, [405, 226, 1], [70, 0, 0]), (64, [200, 33], [0, 10])])
def test_one_branch_equals_plain_causal(ops, hd, lens, sh):
    """One branch behind any prefix hides nothing: pad-free rows against plain causal rv_attn_fwd on the same rows."""
    dev = _dev()
    S, H, L = len(lens), 2, max(lens)
    off = [sum(lens[:s]) for s in range(S)]
    g = torch.Generator().manual_seed(sum(lens))
    qkv = (torch.randn(sum(lens), 3 * H * hd, generator=g) * 0.7).to(BF).to(dev)
    rows = (torch.tensor(off, dtype=torch.int32, device=dev), torch.tensor(lens, dtype=torch.int32, device=dev))
    seg_sh = torch.tensor(sh, dtype=torch.int32, device=dev)
    q_lo = torch.tensor(sum(([0] * a + [a] * (n - a) for a, n in zip(sh, lens)), []), dtype=torch.int32, device=dev)
    ref_o, ref_l = ops.attn_fwd(qkv, S, L, H, hd, True, 0, H * hd, 2 * H * hd, rows=rows)
    out, lse = ops.attn_fwd(qkv, S, L, H, hd, True, 0, H * hd, 2 * H * hd, rows=rows, branches=(seg_sh, q_lo))
    assert torch.equal(out, ref_o)
    for s in range(S):
        assert torch.equal(lse[s, :, :lens[s]], ref_l[s, :, :lens[s]]) and torch.isfinite(lse[s, :, :lens[s]]).all()


def test_arguments_are_checked(ops):
    dev = _dev()
    qkv = torch.zeros(64, 3 * 128, dtype=BF, device=dev)
    sh = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="q_lo"):
        ops.attn_fwd(qkv, 1, 64, 1, 128, True, 0, 128, 256, branches=(sh, torch.zeros(63, dtype=torch.int32, device=dev)))
    with pytest.raises(ValueError, match="causal"):
        ops.attn_fwd(qkv, 1, 64, 1, 128, False, 0, 128, 256, branches=(sh, torch.zeros(64, dtype=torch.int32, device=dev)))
