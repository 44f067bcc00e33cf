"""Token-weighted DPO through the generic (OmniLMM) branch of get_beta_and_logps on the GPU, against the fixture the
REFERENCE'S OWN code produced (tests/golden/omnilmm_token_weighted.pt, tests/golden/make_token_weighted_golden.py):

  * the two weighted kernels on the hot path, ``rv_seq_sum`` and ``rv_row_coef``, against float64;
  * the training step (OmniLMMDPOTrainer.compute_loss + backward) at both ``dpo_use_average`` settings in the rectangular,
    packed and pad-free layouts: weighted policy / reference log-probs, loss, rewards, language-model and resampler gradients;
  * the precompute's generic branch (get_multimodal_sample_logps(is_llava15=False));
  * all-ones weights reproduce the unweighted generic step bit for bit (full fine-tune and LoRA with dropout 0);
  * OmniLMMDPOTrainer.training_step moves the parameters, logs the reference's metric names, and a NaN reference log-prob
    raises FloatingPointError before backward with parameters and optimizer state untouched.

Bars (those of test_omnilmm_gpu.py): log-probs / loss 1e-3 relative (the summed loss: 5e-3, reason at the assert); gradients
per-tensor norm within 3 %, cosine >= 0.995."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dpo_oracle as O  # noqa: E402
from oracle import omnilmm_oracle as OO  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden", "omnilmm_token_weighted.pt")
LAYOUTS = {"rect": (False, False), "packed": (True, False), "pad_free": (True, True)}     # (share_prefix, pad_free)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


def _gold():
    return torch.load(GOLD, weights_only=False)


def _cfg(meta):
    from rlaif_v_amd.omnilmm import OmniLMMConfig
    pt, st, en = meta["tokens"]
    return OmniLMMConfig(hidden=512, layers=2, heads=4, kv_heads=2, ffn=768, vocab=325, model_max_length=256,
                         num_query=meta["num_query"], vision_width=meta["kv_dim"], image_size=84,
                         im_patch_token=pt, im_start_token=st, im_end_token=en)


def _weights(meta):
    """The weight recipe of make_omnilmm_golden.py (lm_weights(seed=3) + make_resampler_weights)."""
    ocfg = O.LlavaCfg(hidden=512, layers=2, heads=4, kv_heads=2, ffn=768, vocab=325, model_max_length=256)
    W = {k: v for k, v in O.make_weights(ocfg, seed=3).items() if "vision_tower" not in k and "mm_projector" not in k}
    W.update(OO.make_resampler_weights(512, meta["kv_dim"], meta["num_query"]))
    return W


def _model(G, layout="rect", lora=None):
    from rlaif_v_amd.omnilmm import OmniLMMDPOModel
    model = OmniLMMDPOModel(_cfg(G["meta"]), lora=lora)
    model.share_prefix, model.pad_free = LAYOUTS[layout]
    model.load_state_dict(_weights(G["meta"]))
    return model


def _batch(G):
    b = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in G["batch"].items()}
    b["images"] = G["tower_features"].clone()                  # precomputed tower tokens [B, N, width]
    return b


def _check_grads(gold, mine, what):
    worst = 0.0
    for k, g in gold.items():
        m = mine[k].float().cpu()
        if "full" in g:
            ref = g["full"]
            if float(ref.norm()) < 1e-7:
                continue
            c = _cos(m, ref)
            rel = abs(float(m.norm()) - float(ref.norm())) / float(ref.norm())
        else:
            blk = m.reshape(m.shape[0], -1)[:8, :64]
            c = _cos(blk, g["block"])
            rel = abs(float(m.double().norm()) - g["norm"]) / g["norm"]
        worst = max(worst, rel)
        assert c >= 0.995, (what, k, c)
        assert rel <= 3e-2, (what, k, rel)
    print(f"[{what}] worst per-tensor grad-norm rel err {worst:.3e}")


# ------------------------------------------------------------------------------------------------ kernels
def test_weighted_seq_sum_and_row_coef_kernels():
    _need_gpu()
    from rlaif_v_amd import ops
    g = torch.Generator().manual_seed(3)
    lens = [0, 1, 255, 256, 257, 1000, 3, 0, 37]                  # empty and ragged segments, n = 1809 (not a multiple of 256)
    n, n_seq = sum(lens), len(lens)
    off = torch.zeros(n_seq + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(lens), 0)
    seq_of_row = torch.repeat_interleave(torch.arange(n_seq), torch.tensor(lens))
    logp = -6.0 * torch.rand(n, generator=g)
    w = torch.rand(n, generator=g) * 3.0
    w[torch.rand(n, generator=g) < 0.2] = 0.0                     # zeros among non-binary weights
    w[seq_of_row == 6] = 0.0                                      # a segment whose weights are all zero
    coef = torch.randn(n_seq, generator=g)
    dev = torch.device("cuda:0")
    d = lambda t, dt: t.to(dev, dt).contiguous()                  # noqa: E731
    s, c = ops.seq_sum(d(logp, torch.float32), d(off, torch.int32), n_seq, weight=d(w, torch.float32))
    rc = ops.row_coef(d(coef, torch.float32), d(seq_of_row, torch.int32), d(w, torch.float32))
    torch.cuda.synchronize()
    lw, ww = logp.double() * w.double(), w.double()
    s_ref = torch.stack([lw[off[i]:off[i + 1]].sum() for i in range(n_seq)])
    c_ref = torch.stack([ww[off[i]:off[i + 1]].sum() for i in range(n_seq)])
    scale = torch.stack([lw[off[i]:off[i + 1]].abs().sum() for i in range(n_seq)]) + 1e-30
    assert bool(((s.double().cpu() - s_ref).abs() <= 1e-5 * scale).all()), (s.cpu(), s_ref)
    assert bool(((c.double().cpu() - c_ref).abs() <= 1e-5 * (c_ref + 1e-30)).all()), (c.cpu(), c_ref)
    assert float(s[0]) == 0.0 and float(c[0]) == 0.0 and float(s[7]) == 0.0 and float(c[7]) == 0.0 and float(c[6]) == 0.0
    torch.testing.assert_close(rc.cpu().double(), coef.double()[seq_of_row] * ww, rtol=1e-6, atol=0.0)
    # weight 1.0 everywhere is bit-identical to no weight (w * 1.0 is exact, same reduction order)
    ones = torch.ones(n, dtype=torch.float32, device=dev)
    s1, c1 = ops.seq_sum(d(logp, torch.float32), d(off, torch.int32), n_seq, weight=ones)
    s0, c0 = ops.seq_sum(d(logp, torch.float32), d(off, torch.int32), n_seq)
    assert torch.equal(s1, s0) and torch.equal(c1, c0)
    assert torch.equal(ops.row_coef(d(coef, torch.float32), d(seq_of_row, torch.int32), ones),
                       ops.row_coef(d(coef, torch.float32), d(seq_of_row, torch.int32)))


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("avg", [False, True])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_token_weighted_step_matches_reference_golden(layout, avg, monkeypatch):
    _need_gpu()
    from rlaif_v_amd.trainer import OmniLMMDPOTrainer, TrainingArguments
    monkeypatch.setenv("SFT_weight", "0.0")
    monkeypatch.setenv("DPO_weight", "1.0")
    G = _gold()
    case = G[f"avg{int(avg)}"]
    model = _model(G, layout)
    tr = OmniLMMDPOTrainer(model=model, args=TrainingArguments(dpo_token_weighted=True, dpo_use_average=avg))
    loss = tr.compute_loss(model, _batch(G))
    out = model.last_out
    B = G["batch"]["win_input_ids"].shape[0]
    # the selected-row training path: weights ride on the plan, no all-rows evaluation
    labels = G["batch"]["concatenated_labels"]
    mask = labels[:, 1:] != -100
    assert out.plan.n_sel == int(mask.sum()) and out.ctx["w_rows"] is out.plan.w_sel
    assert torch.equal(out.plan.w_sel.cpu(), G["batch"]["concatenated_token_weight"][mask])
    pol = (out.seq_logp / out.seq_cnt if avg else out.seq_logp).cpu()
    ref_pol = torch.cat([case["policy_win_logp"], case["policy_rej_logp"]])
    err = (pol - ref_pol).abs()
    print(f"{layout} avg={avg}: policy logp err {err.tolist()} of {ref_pol.tolist()}; loss {float(loss):.6f} vs "
          f"{float(case['loss']):.6f}")
    assert bool((err <= 1e-3 * ref_pol.abs()).all())
    # weighted reference log-probs (compute_weighted_logp on the device, fp32) enter the loss and the rewards
    ref_w = torch.cat([case["ref_win_logp"], case["ref_rej_logp"]])
    z = (pol[:B] - pol[B:]).double() - (ref_w[:B] - ref_w[B:]).double()
    torch.testing.assert_close(loss.cpu().double(), torch.nn.functional.softplus(-G["batch"]["beta"] * z).mean(), rtol=1e-5, atol=0.0)
    # The loss bar.  With dpo_use_average the 1e-3 bar holds as is (measured 3e-5).  With sums, each log-prob has magnitude
    # 200-300 but the fixture's pairs sit near z = 0, where d(loss) / loss = beta sigmoid(-beta z) / softplus(-beta z) dz,
    # i.e. about 0.07 dz.  The measured log-prob errors are 0.003-0.026 (<= 1.2e-4 relative, 8x inside their 1e-3 bar) and
    # move the loss by up to 1.1e-3 relative.  That is the bf16 forward, not the weighting: all-ones weights are bit-identical
    # to the unweighted step (test below), and the averaged case, the same rows and weights, is 30x inside the bar.  The sums
    # get the loss bar of test_omnilmm_full_width_shallow_vs_oracle (5e-3, same reason); the log-probs carry the 1e-3 bar
    # above, and the line before this comment pins the loss as the DPO loss of the product's own log-probs.
    torch.testing.assert_close(loss.cpu(), case["loss"], rtol=1e-3 if avg else 5e-3, atol=0.0)
    torch.testing.assert_close(out.per_pair[3:5].flatten().cpu(), ref_pol, rtol=1e-3, atol=0.0)
    torch.testing.assert_close(out.per_pair[1].cpu(), case["chosen_rewards"], rtol=2e-3, atol=1e-2)
    torch.testing.assert_close(out.per_pair[2].cpu(), case["rejected_rewards"], rtol=2e-3, atol=1e-2)
    m = tr.pop_metrics()
    torch.testing.assert_close(torch.tensor([m["logps_train/ref_chosen"], m["logps_train/ref_rejected"]]),
                               torch.stack([ref_w[:B].mean(), ref_w[B:].mean()]).float(), rtol=1e-5, atol=0.0)
    model.backward(out, model.last_coef)
    _check_grads(case["grads"], model.grads_state_dict(), f"token-weighted {layout} avg={avg}")


def test_precompute_generic_branch_matches_reference_golden():
    _need_gpu()
    from rlaif_v_amd.inference_logp import get_multimodal_sample_logps
    G = _gold()
    model = _model(G)
    b = G["batch"]
    loader = [dict(win_input_ids=b["win_input_ids"], win_labels=b["win_labels"], rej_input_ids=b["rej_input_ids"],
                   rej_labels=b["rej_labels"], images=G["tower_features"])]
    wl, wa, wp, rl, ra, rp = get_multimodal_sample_logps(model, loader, is_llava15=False)
    gold = G["precompute"]["policy"]
    for key, (lp, av, pt) in (("win", (wl, wa, wp)), ("rej", (rl, ra, rp))):
        g = gold[key]
        ids = b[f"{key}_input_ids"]
        assert len(pt) == ids.shape[0] and all(len(row) == ids.shape[1] - 1 for row in pt)
        lp, av, pt = torch.tensor(lp), torch.tensor(av), torch.tensor(pt)
        print(f"precompute {key}: logp {lp.tolist()} vs {g['logp'].tolist()}; per-token max abs err "
              f"{float((pt - g['per_token']).abs().max()):.3e}")
        assert bool(((lp - g["logp"]).abs() <= 1e-3 * g["logp"].abs()).all())
        assert bool(((av - g["avg"]).abs() <= 1e-3 * g["avg"].abs()).all())
        assert _cos(pt, g["per_token"]) >= 0.9999
        assert float((pt - g["per_token"]).abs().max()) <= 5e-2


# ------------------------------------------------------------------------------------------------ unit weights
def _unit_weight_batches(G, dev):
    """The fixture batch with all-ones token weights, and the same batch for the unweighted step with reference log-probs
    computed by the same device reduction (so both steps feed rv_dpo_loss identical reference values)."""
    from rlaif_v_amd.trainer import compute_weighted_logp
    bw = _batch(G)
    for k in ("win_token_weight", "rej_token_weight", "concatenated_token_weight"):
        bw[k] = torch.ones_like(bw[k])
    bu = _batch(G)
    for key in ("win", "rej"):
        pt, lab, w = bw[f"ref_{key}_per_token_logp"], bw[f"{key}_labels"], bw[f"{key}_token_weight"]
        bu[f"ref_{key}_logp"] = compute_weighted_logp(pt.to(dev), lab, w, False).cpu()
        bu[f"ref_{key}_avg_logp"] = compute_weighted_logp(pt.to(dev), lab, w, True).cpu()
    return bw, bu


@pytest.mark.parametrize("lora", [False, True])
@pytest.mark.parametrize("avg", [False, True])
def test_unit_weights_equal_the_unweighted_step_bit_for_bit(avg, lora, monkeypatch):
    _need_gpu()
    from rlaif_v_amd.model import LoraConfig
    from rlaif_v_amd.trainer import OmniLMMDPOTrainer, TrainingArguments
    monkeypatch.setenv("SFT_weight", "0.0")
    monkeypatch.setenv("DPO_weight", "1.0")
    G = _gold()
    model = _model(G, "pad_free", lora=LoraConfig(r=16, lora_alpha=32, lora_dropout=0.0) if lora else None)
    if lora:
        model.reset_lora_parameters(seed=1, b_std=0.02)
    bw, bu = _unit_weight_batches(G, model.device)
    res = []
    for tw, batch in ((True, bw), (False, bu)):
        tr = OmniLMMDPOTrainer(model=model, args=TrainingArguments(dpo_token_weighted=tw, dpo_use_average=avg))
        loss = tr.compute_loss(model, batch)
        model.backward(model.last_out, model.last_coef)
        torch.cuda.synchronize()
        res.append((loss.clone(), tr.pop_metrics(), model.store.flat_g.clone(), model.last_out.seq_logp.clone(),
                    model.last_out.seq_cnt.clone()))
    (lw, mw, gw, sw, cw), (lu, mu, gu, su, cu) = res
    assert torch.equal(sw, su) and torch.equal(cw, cu)
    assert torch.equal(lw, lu), (float(lw), float(lu))
    assert mw == mu
    assert float(gw.float().abs().max()) > 0 and torch.equal(gw, gu)


# ------------------------------------------------------------------------------------------------ trainer
def test_omnilmm_trainer_trains_token_weighted_and_stops_on_nan(monkeypatch):
    _need_gpu()
    from rlaif_v_amd.trainer import OmniLMMDPOTrainer, TrainingArguments
    monkeypatch.setenv("SFT_weight", "0.0")
    monkeypatch.setenv("DPO_weight", "1.0")
    G = _gold()
    model = _model(G, "pad_free")
    tr = OmniLMMDPOTrainer(model=model, args=TrainingArguments(dpo_token_weighted=True, learning_rate=1e-4, max_steps=10,
                                                               warmup_ratio=0.0, lr_scheduler_type="constant"))
    st = model.store
    p0 = st.train_p.clone()
    names = {"rewards_train/chosen", "rewards_train/rejected", "logps_train/rejected", "logps_train/chosen",
             "logps_train/ref_rejected", "logps_train/ref_chosen", "rewards_train/accuracies", "rewards_train/margins"}
    losses = []
    for _ in range(2):
        losses.append(float(tr.training_step(_batch(G))))
        m = tr.pop_metrics()
        assert set(m) == names and all(v == v for v in m.values()), m
    assert tr.state["global_step"] == 2 and all(v == v for v in losses)
    assert not torch.equal(st.train_p, p0)
    print(f"token-weighted training losses {losses}")
    # a NaN reference log-prob stops the step before backward: nothing of the model or the optimizer moves
    bad = _batch(G)
    lab = bad["win_labels"]
    col = int(torch.nonzero(lab[0, 1:] != -100)[0])
    bad["ref_win_per_token_logp"][0, col] = float("nan")
    snap = [t.clone() for t in (st.train_p, st.flat_master, st.flat_m, st.flat_v)]
    with pytest.raises(FloatingPointError, match="ref_win_logp"):
        tr.training_step(bad)
    torch.cuda.synchronize()
    for a, b in zip(snap, (st.train_p, st.flat_master, st.flat_m, st.flat_v)):
        assert torch.equal(a, b)
    assert tr.state["global_step"] == 2
