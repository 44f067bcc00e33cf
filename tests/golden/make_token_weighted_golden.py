"""Golden vectors for token-weighted DPO through the generic (OmniLMM) branch, produced by the REFERENCE'S OWN code on CPU:

    python tests/golden/make_token_weighted_golden.py          (build container only: needs /root/reference)

Same model, shims and weight recipe as make_omnilmm_golden.py (imported from it): ``OmniLMMForCausalLM`` with a stub tower,
4 query / 2 key-value heads, ``lm_weights(seed=3)`` + ``make_resampler_weights``.  What runs:

  1. the precompute's generic branch (muffin/eval/muffin_inference_logp.py:253-261): ``model(input_ids, labels, images)`` per
     key on the B distinct images, then ``get_batch_logps(return_all=True)``.  Once on a PERTURBED copy of the weights - the
     reference model of the DPO step, so that reference != policy - and once on the unperturbed weights (pins the product's
     precompute, ``get_multimodal_sample_logps(is_llava15=False)``);
  2. the reference collator ``DataCollatorForDPODataset`` (muffin/train/train_muffin.py:37-112, ``mod_token_weight`` 3.0):
     token weights from ``utils/diff_lib.get_diff_ids``; the rejected answers share runs of >= 3 tokens with the chosen
     ones, so only some tokens are marked and both weight values appear;
  3. ``get_beta_and_logps(is_llava15=False)`` with ``dpo_token_weighted=True`` for ``dpo_use_average`` False and True, then
     ``dpo_loss``, ``.mean()``, ``backward()``.

Stored: the batch (every key the reference pops), the tower features, the policy and weighted-reference log-probs, losses,
rewards and gradients (compressed like omnilmm_tiny.pt), and the precompute outputs.
"""
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_omnilmm_golden as M  # noqa: E402  (installs the timm / torchvision / cv2 / wandb shims on import)

from muffin.eval.muffin_inference_logp import get_batch_logps, preference_collator_fn  # noqa: E402
from muffin.train.train_muffin import DataCollatorForDPODataset  # noqa: E402
from muffin.train.trainers import dpo_loss, get_beta_and_logps  # noqa: E402
from omnilmm.model.omnilmm import OmniLMMConfig, OmniLMMForCausalLM  # noqa: E402
from oracle import omnilmm_oracle as OO  # noqa: E402

B, PROMPT_LEN, MOD_TOKEN_WEIGHT, BETA = 3, 8, 3.0, 0.1
PERTURB_STD = 0.3


def build_model(cfg, W):
    ocfg = OmniLMMConfig(hidden_size=cfg.hidden, intermediate_size=cfg.ffn, num_hidden_layers=cfg.layers,
                         num_attention_heads=cfg.heads, num_key_value_heads=cfg.n_kv_heads, vocab_size=cfg.vocab,
                         rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta, max_position_embeddings=4096,
                         sliding_window=None, pad_token_id=None, attn_implementation="eager",
                         mm_vision_tower="stub", num_query=M.NUM_QUERY, image_size=M.IMG)
    torch.manual_seed(0)
    model = OmniLMMForCausalLM(ocfg).float()
    missing, unexpected = model.load_state_dict(W, strict=False)
    assert not unexpected, unexpected
    assert all(("vision_tower" in m) or m.endswith("resampler.pos_embed") for m in missing), missing
    vc = model.model.vision_config
    vc.im_patch_token, vc.im_start_token, vc.im_end_token = M.TOKENS
    vc.use_im_start_end = True
    return model


def make_samples(cfg, g):
    """B (chosen, rejected) token sequences in the OmniLMM convention [bos, prompt, <im_start>, <im_patch> x nq, <im_end>,
    question, answer]; the rejected answer is the chosen one with a few short spans replaced / inserted / deleted."""
    im_patch, im_start, im_end = M.TOKENS
    lo, hi = 3, cfg.vocab - 4
    out = []
    for b in range(B):
        prompt = torch.randint(lo, hi, (PROMPT_LEN,), generator=g)
        img = torch.cat([torch.tensor([im_start]), torch.full((M.NUM_QUERY,), im_patch), torch.tensor([im_end])])
        head = torch.cat([torch.tensor([1]), prompt, img, torch.randint(lo, hi, (6,), generator=g)])
        ans = torch.randint(lo, hi, (30 + 4 * b,), generator=g)
        rej = torch.cat([ans[:6], torch.randint(lo, hi, (2,), generator=g),        # replace 2
                         ans[8:15], torch.randint(lo, hi, (3,), generator=g),      # insert 3
                         ans[15:22], ans[24:]])                                    # delete 2
        if b == 1:
            rej = torch.cat([rej, torch.randint(lo, hi, (5,), generator=g)])        # longer rejected answer
        pair = []
        for a in (ans, rej):
            ids = torch.cat([head, a])
            lab = torch.cat([torch.full((head.numel(),), -100), a])
            pair.append((ids, lab))
        out.append(pair)
    return out


@torch.no_grad()
def precompute(model, batch):
    """muffin_inference_logp.py:253-263, generic branch, on CPU."""
    res = {}
    for key in ("win", "rej"):
        output = model(input_ids=batch[f"{key}_input_ids"], labels=batch[f"{key}_labels"],
                       attention_mask=batch[f"{key}_attention_mask"], images=batch["images"])
        per_token, log_prob, avg = get_batch_logps(output.logits, batch[f"{key}_labels"], return_all=True)
        assert per_token.size(1) >= batch[f"{key}_input_ids"].size(1) - 1
        res[key] = dict(per_token=per_token.clone(), logp=log_prob.clone(), avg=avg.clone())
    return res


def main():
    cfg = M.tiny_cfg()
    W = M.lm_weights(cfg)
    W.update(OO.make_resampler_weights(cfg.hidden, M.KV_DIM, M.NUM_QUERY))
    model = build_model(cfg, W)
    gp = torch.Generator().manual_seed(21)
    W_ref = {k: v + PERTURB_STD * v.float().std() * torch.randn(v.shape, generator=gp) for k, v in W.items()}
    ref_model = build_model(cfg, W_ref)
    model.eval(), ref_model.eval()

    g = torch.Generator().manual_seed(17)
    samples = make_samples(cfg, g)
    images = torch.randn(B, 3, M.IMG, M.IMG, generator=g)
    raw = [(dict(input_ids=r[0], labels=r[1], image=images[b]), dict(input_ids=w[0], labels=w[1], image=images[b]))
           for b, (w, r) in enumerate(samples)]
    plain = preference_collator_fn(raw, 0)
    pre_ref = precompute(ref_model, plain)                       # the DPO step's reference model
    pre_pol = precompute(model, plain)                           # pins the product's precompute

    instances = []
    for b, (rej, win) in enumerate(raw):
        win = dict(win, ref_win_logp=float(pre_ref["win"]["logp"][b]), ref_win_avg_logp=float(pre_ref["win"]["avg"][b]),
                   ref_win_per_token_logp=pre_ref["win"]["per_token"][b].tolist())
        rej = dict(rej, ref_rej_logp=float(pre_ref["rej"]["logp"][b]), ref_rej_avg_logp=float(pre_ref["rej"]["avg"][b]),
                   ref_rej_per_token_logp=pre_ref["rej"]["per_token"][b].tolist())
        instances.append((rej, win))
    collator = DataCollatorForDPODataset(tokenizer=types.SimpleNamespace(pad_token_id=0), beta=BETA,
                                         mod_token_weight=MOD_TOKEN_WEIGHT)
    batch = collator(instances)
    for k in ("win_token_weight", "rej_token_weight"):
        vals = set(batch[k].unique().tolist())
        assert vals == {1.0, MOD_TOKEN_WEIGHT}, (k, vals)
    with torch.no_grad():
        tf = model.model.vision_tower.forward_features(images)[:, 1:]

    out = dict(batch={k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}, tower_features=tf,
               precompute=dict(policy=pre_pol, reference=pre_ref))
    model.train()
    for avg in (False, True):
        args = types.SimpleNamespace(dpo_use_average=avg, dpo_token_weighted=True, task="DPO")
        model.zero_grad()
        pw, pr, rw, rr, beta = get_beta_and_logps(dict(batch), model, args, is_llava15=False)
        losses, cw, cr = dpo_loss(pw, pr, rw, rr, beta=beta)
        loss = losses.mean()
        loss.backward()
        grads = M.compress_grads({k: v.grad for k, v in model.named_parameters() if v.grad is not None and "vision_tower" not in k})
        out[f"avg{int(avg)}"] = dict(policy_win_logp=pw.detach(), policy_rej_logp=pr.detach(), ref_win_logp=rw.detach(),
                                     ref_rej_logp=rr.detach(), loss=loss.detach(), losses=losses.detach(),
                                     chosen_rewards=cw.detach(), rejected_rewards=cr.detach(), grads=grads)
        print(f"dpo_use_average={avg}: loss {float(loss):.6f}  policy {pw.tolist()} {pr.tolist()}  ref {rw.tolist()} {rr.tolist()}")
    out["meta"] = dict(num_query=M.NUM_QUERY, kv_dim=M.KV_DIM, tokens=M.TOKENS, mod_token_weight=MOD_TOKEN_WEIGHT)
    path = os.path.join(M.REPO, "tests", "golden", "omnilmm_token_weighted.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
