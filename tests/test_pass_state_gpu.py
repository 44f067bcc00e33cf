"""The pass state of LlavaDPOModel (model._cur_drop, a LoraDrop written by _begin_pass): every surface draws its adapter-dropout
masks from the dropout step and mode of the pass it runs, also the reference-style ``forward()``, which before read a second
ambient attribute that only the other surfaces wrote.  Tiny adapter model, r = 16, lora_dropout 0.25; every comparison is
``torch.equal`` - the same kernels on the same inputs and seeds."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import dpo_oracle as O  # noqa: E402
from test_lora_gpu import _build, _need_gpu, _trainer  # noqa: E402


def _embeds(cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(2, 24, cfg.hidden, generator=g) * 0.5).to(torch.bfloat16)


def test_forward_on_a_fresh_adapter_model_in_training_mode():
    _need_gpu()
    cfg = O.tiny_cfg()
    model, _ = _build(cfg, 16, dropout=0.25)
    model.train()
    emb = _embeds(cfg)
    step0 = model._dropout_step
    a = model(inputs_embeds=emb).logits.clone()
    b = model(inputs_embeds=emb).logits.clone()
    assert a.shape == (2, 24, cfg.vocab)
    assert torch.equal(a, b)                            # forward() does not advance the step: the same masks again
    c = model.eval()(inputs_embeds=emb).logits
    assert not torch.equal(a, c)                        # and the masks were applied
    assert model._dropout_step == step0


def test_forward_masks_follow_the_dropout_step_not_the_last_pass(monkeypatch):
    _need_gpu()
    monkeypatch.setenv("SFT_weight", "0.0")
    monkeypatch.setenv("DPO_weight", "1.0")
    cfg = O.tiny_cfg()
    emb = _embeds(cfg, seed=1)
    used, _ = _build(cfg, 16, dropout=0.25)
    used.train()
    tr = _trainer(used)
    tr.compute_loss(used, dict(O.make_synthetic_batch(cfg, 2, 40, 12, seed=41)))
    used.backward(used.last_out, used.last_coef)        # restores the pass state of step 1 from the forward's context
    fresh, _ = _build(cfg, 16, dropout=0.25)
    fresh.train()
    used._dropout_step = fresh._dropout_step = 5
    assert torch.equal(used(inputs_embeds=emb).logits, fresh(inputs_embeds=emb).logits)


def test_pass_state_survives_a_pass(monkeypatch):
    _need_gpu()
    monkeypatch.setenv("SFT_weight", "0.0")
    monkeypatch.setenv("DPO_weight", "1.0")
    cfg = O.tiny_cfg()
    model, _ = _build(cfg, 16, dropout=0.25)
    model.train()
    batch = O.make_synthetic_batch(cfg, 2, 40, 12, seed=41)
    _trainer(model).compute_loss(model, dict(batch))
    assert model._dropout_step == 1
    assert model._cur_drop.p == 0.25 and model._cur_drop.step == model._dropout_step
    model.eval()
    ids = batch["concatenated_input_ids"]
    prompts = [[ids[k, :12].clone(), ids[k, :14].clone()] for k in range(2)]
    model.forward_next_token_scores(prompts, batch["images"], [3, 4])
    assert model._cur_drop.p == 0.0 and model._cur_drop.step == 1 and model._dropout_step == 1
