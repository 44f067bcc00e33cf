"""RV_LORA_PEFT_MASKS=1 (peft's one nn.Dropout per wrapped nn.Linear: q / k / v and gate / up drop the same input with INDEPENDENT
masks) on the kernels that draw the masks themselves: a training step against the fp32 oracle with the seven per-module masks of
oracle/dropout_mask.py replayed, with and without the fused SwiGLU layout (RV_LORA_FUSE_SWIGLU=1, which used to be dropped silently
under per-module masks), what it launches, gradient checkpointing, and the untouched default.  Bars as in
test_lora_gpu.py::test_lora_peft_exact_per_module_dropout_masks."""
import collections
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dpo_oracle as O  # noqa: E402

F_, B1_, B2_ = "rv_gemm_nt_lora_masks_bf16", "rv_gemm_nt_dropout_masks_bf16", "rv_gemm_tn_lora_masks_bf16"


def _env(monkeypatch, peft_masks, fuse_swiglu):
    monkeypatch.setenv("SFT_weight", "0.0")
    monkeypatch.setenv("DPO_weight", "1.0")
    monkeypatch.setenv("RV_LORA_FUSE_SWIGLU", str(fuse_swiglu))
    if peft_masks:
        monkeypatch.setenv("RV_LORA_PEFT_MASKS", "1")
    else:
        monkeypatch.delenv("RV_LORA_PEFT_MASKS", raising=False)


def _full_width():
    if torch.cuda.get_device_properties(0).total_memory < 100 * 2**30:
        pytest.skip("needs the 288 GB part")
    cfg = O.LlavaCfg(layers=2, clip_layers=3, image_size=112, model_max_length=2048)      # 64 patches, 3-layer CLIP-L width
    return cfg, O.make_synthetic_batch(cfg, 2, 1000, 24, seed=17), 0.05, 17


def _tiny():
    cfg = O.tiny_cfg()
    return cfg, O.make_synthetic_batch(cfg, 2, 40, 12, seed=43), 0.25, 3


def _counted_step(monkeypatch, model, tr, batch, coef=None):
    """One training step (forward + backward) with every C-ABI call counted."""
    from rlaif_v_amd import hip
    calls = collections.Counter()
    orig_call = hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (calls.update([name]), orig_call(name, *a))[1])
    loss = tr.compute_loss(model, dict(batch))
    out = model.last_out
    if coef is None:
        model.backward(out, model.last_coef)
    monkeypatch.setattr(hip, "call", orig_call)
    return loss, out, calls


def _check_against_oracle(model, W, cfg, batch, p, loss, out, backward_on_oracle_coef):
    import test_lora_gpu as TL
    from oracle import dropout_mask as DM
    N = out.plan.S * out.plan.L
    masks, shared = {}, {}
    for i in range(cfg.layers):
        masks.update(DM.layer_masks(i, N, cfg.hidden, cfg.ffn, p, step=1, rank=0, per_module=True))
        shared.update(DM.layer_masks(i, N, cfg.hidden, cfg.ffn, p, step=1, rank=0))
    q, k = masks["model.layers.0.self_attn.q_proj"], masks["model.layers.0.self_attn.k_proj"]
    assert not torch.equal(q, k) and torch.equal(q, shared["model.layers.0.self_attn.q_proj"])
    torch.set_num_threads(min(64, os.cpu_count() or 8))
    ref, grads = TL._oracle_grads(batch, W, cfg, 16 / 64, masks)
    ref = {kk: (v.detach() if torch.is_tensor(v) else v) for kk, v in ref.items()}
    if backward_on_oracle_coef:
        # sums over 1,000 answer tokens: the forward's bf16 noise moves sigma(-beta z), hence every gradient norm, by several per
        # cent, so the backward runs on the oracle's loss coefficients (as test_lora_full_width_dropout_one_pass_paths_vs_oracle does)
        lp_ref = ref["log_prob"]
        beta, Bq = float(batch["beta"]), lp_ref.numel() // 2
        z_ref = (lp_ref[:Bq] - lp_ref[Bq:]) - (batch["ref_win_logp"].float() - batch["ref_rej_logp"].float())
        sig = torch.sigmoid(-beta * z_ref)
        coef_ref = torch.cat([-beta * sig / Bq, beta * sig / Bq])
        model.backward(out, coef_ref.to(model.last_coef.device, model.last_coef.dtype))
    loss_err = abs(float(loss) - float(ref["loss"]))
    lp_err = (out.seq_logp.cpu() - ref["log_prob"]).abs()
    got = model.grads_state_dict()
    worst = min((TL._cos(got[kk], gref), kk) for kk, gref in grads.items() if gref.norm() >= 1e-8)
    ref_shared = O.dpo_step_forward(batch, W, cfg, sft_weight=0.0, dpo_weight=1.0, lora_scale=16 / 64, lora_masks=shared)
    moved = (ref_shared["log_prob"].detach() - ref["log_prob"]).abs().max().item()
    print(f"per-module masks: loss {float(loss):.6f} vs oracle {float(ref['loss']):.6f} (|d| {loss_err:.3e}), sequence log-prob max "
          f"|d| {lp_err.max().item():.3e} of {ref['log_prob'].abs().max().item():.1f}, worst gradient cosine {worst[0]:.5f} ({worst[1]}), "
          f"shared masks move a log-prob by {moved:.3e}")
    assert loss_err <= 2e-3 * abs(float(ref["loss"])) + 7e-3
    assert bool((lp_err <= 1e-3 * ref["log_prob"].abs() + 5e-2).all())
    assert worst[0] >= 0.99, worst
    assert moved > 1e-3


@pytest.mark.parametrize("fuse_swiglu", [0, 1])
def test_tiny_step_matches_oracle_with_per_module_masks(monkeypatch, fuse_swiglu):
    """Tiny model, p = 0.25.  fuse_swiglu = 1 is honoured under per-module masks (interleaved gate|up layout, parity-split dB)."""
    import test_lora_gpu as TL
    TL._need_gpu()
    _env(monkeypatch, True, fuse_swiglu)
    cfg, batch, p, seed = _tiny()
    model, W = TL._build(cfg, 64, seed=seed, dropout=p, share_prefix=False)       # reference row layout: masks index [S L, in]
    assert model.lora_peft_masks and model.store.lora_il == bool(fuse_swiglu)
    tr = TL._trainer(model)
    model.train()
    loss, out, calls = _counted_step(monkeypatch, model, tr, batch)
    assert calls["rv_dropout"] == 0 and calls[F_] == 4 * cfg.layers
    _check_against_oracle(model, W, cfg, batch, p, loss, out, backward_on_oracle_coef=False)


@pytest.mark.parametrize("fuse_swiglu", [0, 1])
def test_full_width_step_matches_oracle_with_per_module_masks(monkeypatch, fuse_swiglu):
    """Two full-width layers, r = 64, p = 0.05, 4,256 rows (the model of test_lora_full_width_dropout_one_pass_paths_vs_oracle):
    the chip-filling kernels, with fuse_swiglu = 1 the fused-LoRA gate|up GEMM with the SwiGLU epilogue on t = [t_gate | t_up]
    whose halves were dropped with independent masks."""
    import test_lora_gpu as TL
    TL._need_gpu()
    _env(monkeypatch, True, fuse_swiglu)
    cfg, batch, p, seed = _full_width()
    model, W = TL._build(cfg, 64, seed=seed, dropout=p, share_prefix=False)
    assert model.lora_peft_masks and model.store.lora_il == bool(fuse_swiglu)
    tr = TL._trainer(model)
    model.train()
    loss, out, calls = _counted_step(monkeypatch, model, tr, batch, coef="oracle")
    assert out.plan.S * out.plan.L >= 4096
    assert calls["rv_dropout"] == 0 and calls[F_] == 4 * cfg.layers
    assert (calls["rv_gemm_nn_lora_swiglu_bf16"] == cfg.layers) == bool(fuse_swiglu), dict(calls)
    _check_against_oracle(model, W, cfg, batch, p, loss, out, backward_on_oracle_coef=True)


@pytest.mark.parametrize("fuse_swiglu", [0, 1])
@pytest.mark.parametrize("width", ["tiny", "full"])
def test_training_step_makes_no_dropped_copy(monkeypatch, width, fuse_swiglu):
    """One training step under per-module masks: no rv_dropout call at all, one F per fused projection per layer in forward, one
    B2 per fused projection in backward, one B1 per fused projection - except the down projection where its input gradient goes
    through the fused SwiGLU-backward kernel (interleaved layout at chip-filling shapes; down_proj is one module, that kernel's
    mask is already the module's)."""
    import test_lora_gpu as TL
    TL._need_gpu()
    _env(monkeypatch, True, fuse_swiglu)
    cfg, batch, p, seed = _tiny() if width == "tiny" else _full_width()
    model, _ = TL._build(cfg, 64, seed=seed, dropout=p, share_prefix=False)
    tr = TL._trainer(model)
    model.train()
    _, _, calls = _counted_step(monkeypatch, model, tr, batch)
    fused_down = calls["rv_gemm_nn_lora_swiglu_bwd_bf16"]
    assert fused_down == (cfg.layers if (fuse_swiglu and width == "full") else 0), dict(calls)
    assert calls["rv_dropout"] == 0, dict(calls)
    assert calls[F_] == 4 * cfg.layers, dict(calls)
    assert calls[B2_] == 4 * cfg.layers, dict(calls)
    assert calls[B1_] == 4 * cfg.layers - fused_down, dict(calls)
    assert calls["rv_rmsnorm_fwd_dropout"] == 0 and calls["rv_swiglu_fwd_dropout"] == 0 and calls["rv_gemm_nt_dropout_bf16"] == 0, dict(calls)
    if fuse_swiglu and width == "full":
        assert calls["rv_gemm_nn_lora_swiglu_bf16"] == cfg.layers, dict(calls)


@pytest.mark.parametrize("fuse_swiglu", [0, 1])
def test_gradient_checkpointing_is_bit_identical_under_per_module_masks(monkeypatch, fuse_swiglu):
    """Re-running a layer in backward regenerates the same masks (same step counter, deterministic kernels): gradients equal to
    the stored-activation run bit for bit, as test_model_parity_gpu.py::test_gradient_checkpointing_is_bit_identical asks of the
    base model."""
    import test_lora_gpu as TL
    TL._need_gpu()
    _env(monkeypatch, True, fuse_swiglu)
    cfg, batch, p, seed = _tiny()
    grads = []
    for ckpt in (False, True):
        model, _ = TL._build(cfg, 64, seed=seed, dropout=p, share_prefix=False)
        tr = TL._trainer(model, gradient_checkpointing=ckpt)
        assert model.gradient_checkpointing == ckpt and model.lora_peft_masks
        model.train()
        tr.compute_loss(model, dict(batch))
        model.backward(model.last_out, model.last_coef)
        grads.append(model.store.flat_g.clone())
    assert bool(grads[0].any()) and torch.equal(grads[0], grads[1])


@pytest.mark.parametrize("fuse_swiglu", [0, 1])
def test_default_masks_never_reach_the_per_module_kernels(monkeypatch, fuse_swiglu):
    """Without RV_LORA_PEFT_MASKS the step is what it was: one mask per fused projection, none of the three new entry points."""
    import test_lora_gpu as TL
    TL._need_gpu()
    _env(monkeypatch, False, fuse_swiglu)
    cfg, batch, p, seed = _tiny()
    model, _ = TL._build(cfg, 64, seed=seed, dropout=p, share_prefix=False)
    assert not model.lora_peft_masks
    tr = TL._trainer(model)
    model.train()
    _, _, calls = _counted_step(monkeypatch, model, tr, batch)
    assert calls[F_] == 0 and calls[B1_] == 0 and calls[B2_] == 0, dict(calls)
    assert calls["rv_dropout"] + calls["rv_rmsnorm_fwd_dropout"] > 0, dict(calls)
