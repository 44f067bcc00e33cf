"""rv_next_token_scores against a float64 numpy softmax.

Tolerance (derived, not measured): the kernel works in fp32 on logits of magnitude <= 41.  lse = max + log(sum): the
exponentials carry a relative error of a few ulp (2^-23 each), the 32 k-term sum is a 125-term chain per thread followed by an
11-level tree, so its relative error stays below ~150 * 2^-24 ~ 1e-5 in the worst case and log() turns that into an absolute
1e-5; the fp32 representation of lse itself (|lse| < 64) adds 2^-18 ~ 4e-6.  logp = logit - lse adds one rounding.  Bound:
|logp - ref| <= 3e-5, |lse - ref| <= 3e-5, probs relative 1e-4 (exp of a 3e-5 error) + 1e-30 absolute."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _reference(logits, v_valid, seen, penalty, want):
    """float64: HF RepetitionPenaltyLogitsProcessor (transformers logits_process.py: score < 0 -> score * penalty, else
    score / penalty, at the prompt's ids) and log-softmax over the valid columns."""
    x = logits[:, :v_valid].astype(np.float64).copy()
    if seen is not None and penalty != 1.0:
        for m, ids in enumerate(seen):
            ids = np.unique(np.asarray(ids, dtype=np.int64))
            # the kernel applies the penalty to the fp32 logit in fp32
            v = logits[m, ids].astype(np.float32)
            v = np.where(v < 0, v * np.float32(penalty), v / np.float32(penalty)).astype(np.float32)
            x[m, ids] = v.astype(np.float64)
    mx = x.max(1, keepdims=True)
    lse = (mx + np.log(np.exp(x - mx).sum(1, keepdims=True)))[:, 0]
    logp = x[:, want] - lse[:, None]
    return logp, np.exp(logp), x.argmax(1), lse


def _make(M, v_valid, seed):
    ldl = (v_valid + 63) // 64 * 64
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((M, ldl)) * 3.0).astype(np.float32)
    logits[:, v_valid:] = 1e30                                 # vocabulary padding must not matter
    want = np.array([3869, 8241, 694, 1939], dtype=np.int64)   # llama's yes / Yes / no / No
    seen = []
    for m in range(M):
        ids = rng.integers(0, v_valid, size=40 + m).tolist()
        ids += [int(want[m % 4])]                              # a wanted id among the prompt's ids
        neg = int(np.argmin(logits[m, :v_valid]))              # a strongly negative seen logit
        pos = int(np.argmax(logits[m, :v_valid]))              # and the row's maximum: the penalty can move the argmax
        seen.append(ids + [neg, pos])
    return logits, ldl, want, seen


@pytest.mark.parametrize("penalty", [1.0, 1.1])
@pytest.mark.parametrize("v_valid", [32000, 32009])
@pytest.mark.parametrize("M", [1, 3, 70])
def test_against_float64_softmax(M, v_valid, penalty):
    dev = _dev()
    from rlaif_v_amd import ops
    logits, ldl, want, seen = _make(M, v_valid, seed=M * 7 + v_valid)
    # tied maxima: the lowest index wins; a row whose maximum sits in the last valid column
    logits[0, 100] = logits[0, 31000] = 40.0
    if M > 1:
        logits[1, v_valid - 1] = 41.0
    if M > 2:
        logits[2, 5] = logits[2, 6] = logits[2, v_valid - 1] = 39.5
    lg = torch.from_numpy(logits).to(dev)
    before = lg.clone()
    off = np.zeros(M + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(s) for s in seen])
    seen_t = (torch.from_numpy(off).to(dev), torch.tensor(sum(seen, []), dtype=torch.int32, device=dev))
    want_t = torch.from_numpy(want.astype(np.int32)).to(dev)
    probs, logp, argmax, lse = ops.next_token_scores(lg, M, v_valid, want_t, seen=seen_t, penalty=penalty)
    again = ops.next_token_scores(lg, M, v_valid, want_t, seen=seen_t, penalty=penalty)
    torch.cuda.synchronize()
    assert torch.equal(lg, before), "logits were written"
    for a, b in zip((probs, logp, argmax, lse), again):
        assert torch.equal(a, b), "two calls differ"
    r_logp, r_probs, r_arg, r_lse = _reference(logits, v_valid, seen, penalty, want)
    e_lse = np.abs(lse.cpu().numpy().astype(np.float64) - r_lse).max()
    e_logp = np.abs(logp.cpu().numpy().astype(np.float64) - r_logp).max()
    print(f"M={M} V={v_valid} penalty={penalty}: max |lse err| {e_lse:.3e}, max |logp err| {e_logp:.3e}")
    assert e_lse <= 3e-5 and e_logp <= 3e-5
    np.testing.assert_allclose(probs.cpu().numpy().astype(np.float64), r_probs, rtol=1e-4, atol=1e-30)
    assert argmax.cpu().numpy().tolist() == r_arg.tolist()      # numpy's argmax is the first of equal maxima too
    if penalty == 1.0:
        assert int(argmax[0]) == 100
        if M > 1:
            assert int(argmax[1]) == v_valid - 1
        if M > 2:
            assert int(argmax[2]) == 5


def test_penalty_off_without_seen_table_and_padded_rows():
    """seen=None with a penalty, and penalty 1 with a table, are both the plain softmax; rows beyond n_rows are not read."""
    dev = _dev()
    from rlaif_v_amd import ops
    logits, ldl, want, seen = _make(3, 32000, seed=5)
    lg = torch.full((64, ldl), float("nan"), device=dev)
    lg[:3] = torch.from_numpy(logits).to(dev)
    want_t = torch.from_numpy(want.astype(np.int32)).to(dev)
    off = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device=dev)
    ids = torch.tensor([5, 6, 7], dtype=torch.int32, device=dev)
    a = ops.next_token_scores(lg, 3, 32000, want_t)
    b = ops.next_token_scores(lg, 3, 32000, want_t, seen=None, penalty=1.1)
    c = ops.next_token_scores(lg, 3, 32000, want_t, seen=(off, ids), penalty=1.0)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z) and x.shape[0] == 3
    r_logp, _, r_arg, _ = _reference(logits, 32000, None, 1.0, want)
    assert np.abs(a[1].cpu().numpy() - r_logp).max() <= 3e-5 and a[2].cpu().tolist() == r_arg.tolist()
    with pytest.raises(ValueError):
        ops.next_token_scores(lg, 3, ldl + 1, want_t)
    with pytest.raises(ValueError):
        ops.next_token_scores(lg, 3, 32000, want_t.long())
