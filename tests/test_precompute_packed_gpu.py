"""The packed reference log-prob precompute on the GPU (get_multimodal_sample_logps(packed=True)): one forward per batch on the
packed training layout, stored values bit-identical to what the packed training forward computes on the same weights.

  1. ``rv_logp_finish_unpack`` against ``rv_logp_finish`` + torch indexing: bit-equal, untouched slots keep their fill;
  2. step-0 consistency: packed precompute -> ``compute_loss`` on the same batch and weights gives delta = 0.0 for every row,
     rewards exactly 0, the loss of an all-zero logit, per-token values bit-equal at the target positions (pad-free and
     rectangular packed rows, MHA and GQA).  The un-packed precompute's deltas are printed and recorded, not asserted;
  3. batch independence: batch size 1 (three calls) and batch size 3 give bit-equal sums and per-token lists;
  4. the oracle bars of test_reference_logp_precompute (tests/test_model_parity_gpu.py) in packed mode, parquet included;
  5. OmniLMM (position-keeping splice, is_llava15=False): T - 1 entries per list, bit-equal to the packed token-weighted
     training forward at the target positions, compute_weighted_logp on them = the device's weighted sums.

Measured numbers go to the parity record of tests/test_zz_baseline_configs_gpu.py (``_record``)."""
import json
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dpo_oracle as O  # noqa: E402
from oracle import omnilmm_oracle as OO  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # tests/test_zz_baseline_configs_gpu.py (_record)
ANSWERS = [(70, 45), (33, 90), (2, 64)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _record(key, value):
    """The project's record of measured numbers (the parity_<round>.json of tests/test_zz_baseline_configs_gpu.py)."""
    from test_zz_baseline_configs_gpu import _record as record
    record(key, value)


def _build(cfg, seed=3):
    from rlaif_v_amd.model import LlavaConfig, LlavaDPOModel
    model = LlavaDPOModel(LlavaConfig(**O.asdict(cfg)))
    model.load_state_dict(O.make_weights(cfg, seed=seed))
    return model


def _instances(batch):
    """The batch as the precompute's dataset items: (rej_dict, win_dict) per pair, the collator's padding removed."""
    def trim(ids, lab):
        n = int((lab != -100).nonzero()[-1]) + 1
        return ids[:n], lab[:n]
    out = []
    for i in range(batch["win_input_ids"].shape[0]):
        wi, wl = trim(batch["win_input_ids"][i], batch["win_labels"][i])
        ri, rl = trim(batch["rej_input_ids"][i], batch["rej_labels"][i])
        out.append((dict(input_ids=ri, labels=rl, image=batch["images"][i]), dict(input_ids=wi, labels=wl, image=batch["images"][i])))
    return out


def _loader(batch, bs, pad_id=0):
    from rlaif_v_amd.data import preference_collator_fn
    inst = _instances(batch)
    return [preference_collator_fn(inst[i:i + bs], pad_id) for i in range(0, len(inst), bs)]


# ------------------------------------------------------------------------------------------------ 1. kernel
@pytest.mark.parametrize("M", [1, 63, 300])
def test_finish_unpack_kernel_is_finish_plus_indexing(M):
    _need_gpu()
    from rlaif_v_amd import hip
    dev = torch.device("cuda:0")
    nblk = 8                                                         # V = 512
    g = torch.Generator().manual_seed(M)
    pmax = (4.0 * torch.randn(M, nblk, generator=g)).to(dev)
    psum = (1.0 + 63.0 * torch.rand(M, nblk, generator=g)).to(dev)
    tl = (4.0 * torch.randn(M, generator=g)).to(dev)
    # slots: rows 0, 3, 6, .. have two per-token slots; rows 1, 4, .. no compact slot; the last row names no slot at all
    n_pt, n_c = 2 * M + 7, M + 3
    perm = torch.randperm(n_pt, generator=g)
    a, b, c = perm[:M].clone(), torch.full((M,), -1), torch.full((M,), -1)
    b[0::3] = perm[M:2 * M][0::3]
    keep = torch.ones(M, dtype=torch.bool)
    keep[1::3] = False
    c[keep] = torch.randperm(n_c, generator=g)[:int(keep.sum())]
    a[M - 1] = b[M - 1] = c[M - 1] = -1
    a, b, c = (t.to(dev, torch.int32).contiguous() for t in (a, b, c))
    lse = torch.empty(M, dtype=torch.float32, device=dev)
    logp = torch.empty(M, dtype=torch.float32, device=dev)
    hip.call("rv_logp_finish", pmax, psum, tl, nblk, M, lse, logp)
    FILL_PT, FILL_C = -7.5, 3.25
    want_pt = torch.full((n_pt,), FILL_PT, dtype=torch.float32, device=dev)
    want_c = torch.full((n_c,), FILL_C, dtype=torch.float32, device=dev)
    want_pt[a[a >= 0].long()] = logp[a >= 0]
    want_pt[b[b >= 0].long()] = logp[b >= 0]
    want_c[c[c >= 0].long()] = logp[c >= 0]
    got_pt, got_c = torch.full_like(want_pt, FILL_PT), torch.full_like(want_c, FILL_C)
    hip.call("rv_logp_finish_unpack", pmax, psum, tl, nblk, M, a, b, c, got_pt, n_pt, got_c, n_c)
    torch.cuda.synchronize()
    assert torch.equal(got_pt, want_pt) and torch.equal(got_c, want_c)
    written = int((a >= 0).sum() + (b >= 0).sum())
    assert int((got_pt != FILL_PT).sum()) == written and int((got_pt == FILL_PT).sum()) == n_pt - written
    # float64 check of the shared finish itself
    ref = tl.double() - torch.logsumexp(pmax.double() + psum.double().log(), 1)
    torch.testing.assert_close(logp.double(), ref, rtol=0, atol=1e-5)


# ------------------------------------------------------------------------------------------------ 2. bit-consistency
@pytest.mark.parametrize("cfg_name", ["tiny_cfg", "tiny_gqa_cfg"])
@pytest.mark.parametrize("pad_free", ["1", "0"])
def test_packed_precompute_is_the_training_forward_bit_for_bit(pad_free, cfg_name, monkeypatch):
    _need_gpu()
    from rlaif_v_amd import ops
    from rlaif_v_amd.inference_logp import get_multimodal_sample_logps
    from rlaif_v_amd.splice import build_splice_plan
    from rlaif_v_amd.trainer import LLaVA15DPOTrainer, TrainingArguments
    monkeypatch.setenv("RV_PAD_FREE", pad_free)
    monkeypatch.setenv("SFT_weight", "0.0")
    monkeypatch.setenv("DPO_weight", "1.0")
    cfg = getattr(O, cfg_name)()
    model = _build(cfg)
    assert model.share_prefix and model.pad_free == (pad_free == "1")
    batch = O.make_synthetic_batch(cfg, 3, 130, 40, seed=3, answer_lens=ANSWERS)
    B = 3
    wl, wa, wp, rl, ra, rp = get_multimodal_sample_logps(model, [dict(batch)], packed=True)
    u_wl, _, _, u_rl, _, _ = get_multimodal_sample_logps(model, _loader(batch, 1))       # the reference's setting: batch size 1
    tr = LLaVA15DPOTrainer(model=model, args=TrainingArguments())
    model.train(True)

    def step(ref_w, ref_r):
        b = dict(batch)
        b["ref_win_logp"], b["ref_rej_logp"] = torch.tensor(ref_w), torch.tensor(ref_r)
        loss = tr.compute_loss(model, b)
        return loss, model.last_out, tr.pop_metrics()

    loss_u, out_u, m_u = step(u_wl, u_rl)
    delta_u = (out_u.seq_logp.float().cpu() - torch.tensor(u_wl + u_rl)).tolist()
    loss, out, m = step(wl, rl)
    delta = out.seq_logp.float().cpu() - torch.tensor(wl + rl)
    rec = dict(cfg=cfg_name, pad_free=pad_free, packed=dict(delta_nats=delta.tolist(), loss=float(loss), metrics=m),
               unpacked=dict(delta_nats=delta_u, loss=float(loss_u), metrics=m_u), ln2=math.log(2.0))
    print("  " + json.dumps(rec))
    _record(f"step0_tiny_{cfg_name}_padfree{pad_free}", rec)
    assert out.plan.S == B and (out.plan.row_off is not None) == (pad_free == "1")        # really the packed training forward
    assert delta.tolist() == [0.0] * (2 * B)
    assert m["rewards_train/chosen"] == 0.0 and m["rewards_train/rejected"] == 0.0
    z = torch.zeros(B, dtype=torch.float32, device=model.device)
    _, scal0, _ = ops.dpo_loss(torch.zeros(2 * B, dtype=torch.float32, device=model.device),
                               torch.ones(2 * B, dtype=torch.float32, device=model.device), z, z, float(batch["beta"]), False, 0.0, 1.0)
    assert float(loss) == float(scal0[0]) and abs(float(loss) - math.log(2.0)) < 1e-6
    cnt = out.seq_cnt.cpu()
    torch.testing.assert_close(torch.tensor(wa + ra), torch.tensor(wl + rl) / cnt, rtol=1e-6, atol=0.0)   # the average is seq_logp / seq_cnt
    # per-token values at the target positions = the training forward's selected rows, in (sequence, position) order
    flat = build_splice_plan(batch["concatenated_input_ids"], batch["concatenated_labels"], model.cfg.n_image_tokens,
                             B, cfg.model_max_length)
    off = out.plan.seq_off.cpu().tolist()
    train_tok = out.per_token_logp.float().cpu()
    text_len = (batch["concatenated_input_ids"] != 0).sum(1)
    for s, lst in enumerate(wp + rp):
        assert len(lst) == int(text_len[s]) + model.cfg.n_image_tokens - 1 - 1                # n_s - 1
        t = torch.nonzero(flat.labels[s, 1:] != -100, as_tuple=True)[0]
        assert torch.equal(torch.tensor(lst)[t], train_tok[off[s]:off[s + 1]]), s


# ------------------------------------------------------------------------------------------------ 3. batch independence
def test_packed_precompute_does_not_depend_on_the_batch_size():
    _need_gpu()
    from rlaif_v_amd.inference_logp import get_multimodal_sample_logps
    cfg = O.tiny_cfg()
    model = _build(cfg)
    batch = O.make_synthetic_batch(cfg, 3, 130, 40, seed=3, answer_lens=ANSWERS)
    one = get_multimodal_sample_logps(model, _loader(batch, 1), packed=True)
    three = get_multimodal_sample_logps(model, _loader(batch, 3), packed=True)
    for a, b in zip(one, three):
        assert len(a) == len(b) == 3
    assert one[0] == three[0] and one[3] == three[3]                 # the six sums
    assert one[1] == three[1] and one[4] == three[4]
    assert one[2] == three[2] and one[5] == three[5]                 # every per-token list, entry for entry
    assert [len(x) for x in one[2]] == [124, 87, 56] and [len(x) for x in one[5]] == [99, 144, 118]


# ------------------------------------------------------------------------------------------------ 4. oracle parity
def test_packed_reference_logp_precompute_matches_oracle(tmp_path, golden_dir):
    _need_gpu()
    import pandas as pd
    from rlaif_v_amd.inference_logp import inference_logp
    g = torch.load(os.path.join(golden_dir, "tiny_b2.pt"), weights_only=False)
    cfg = O.LlavaCfg(**g["cfg"])
    model = _build(cfg, seed=g["seed"])
    batch = O.make_synthetic_batch(cfg, g["n_pairs"], g["text_len"], g["prompt_len"], seed=g["seed"])
    B = g["n_pairs"]
    inst = _instances(batch)

    class DS(torch.utils.data.Dataset):
        data = [dict(question=f"q{i}", chosen="c", rejected="r", idx=i) for i in range(B)]

        def __len__(self):
            return B

        def __getitem__(self, i):
            return inst[i]

    logps = inference_logp(model, None, DS(), str(tmp_path), batch_size=2, packed=True)
    with torch.no_grad():
        ref = O.dpo_step_forward(batch, O.make_weights(cfg, seed=g["seed"]), cfg, sft_weight=0.0, dpo_weight=1.0)
    worst = 0.0
    for i in range(B):
        win_lp, win_avg, win_tok, rej_lp, rej_avg, rej_tok = logps[i]
        for s, lp, avg, tok, (rej_d, win_d) in ((i, win_lp, win_avg, win_tok, inst[i]), (B + i, rej_lp, rej_avg, rej_tok, inst[i])):
            assert abs(lp - float(ref["log_prob"][s])) <= 1e-3 * abs(float(ref["log_prob"][s]))
            assert abs(avg - float(ref["average_log_prob"][s])) <= 5e-3
            n_text = (win_d if s < B else rej_d)["input_ids"].numel()
            n = len(tok)
            assert n == min(n_text + model.cfg.n_image_tokens - 1, cfg.model_max_length) - 1       # n_s - 1
            # every position, incl. masked ones (log-prob of token id 0 there), in the reference's per-token layout
            torch.testing.assert_close(torch.tensor(tok), ref["per_token_logps"][s, :n], rtol=0, atol=3e-2)
            worst = max(worst, float((torch.tensor(tok) - ref["per_token_logps"][s, :n]).abs().max()))
    print(f"packed precompute vs oracle: worst per-token |err| {worst:.3e}")
    files = sorted(os.listdir(tmp_path))
    assert files == [f"RLAIF-V-Dataset-withlogp_000-{B}.parquet"]
    df = pd.read_parquet(os.path.join(tmp_path, files[0]))
    rec = json.loads(df.iloc[0]["logps"])["logps"]
    assert len(rec) == 6 and abs(rec[0] - logps[0][0]) < 1e-6 and list(df.columns) == ["question", "chosen", "rejected", "idx", "logps"]


# ------------------------------------------------------------------------------------------------ 5. OmniLMM
def test_packed_precompute_generic_branch_omnilmm(monkeypatch):
    _need_gpu()
    from rlaif_v_amd.inference_logp import get_multimodal_sample_logps
    from rlaif_v_amd.omnilmm import OmniLMMConfig, OmniLMMDPOModel
    from rlaif_v_amd.trainer import OmniLMMDPOTrainer, TrainingArguments, compute_weighted_logp
    monkeypatch.setenv("SFT_weight", "0.0")
    monkeypatch.setenv("DPO_weight", "1.0")
    G = torch.load(os.path.join(REPO, "tests", "golden", "omnilmm_tiny.pt"), weights_only=False)
    meta, case = G["meta"], G["dpo"]
    pt, st, en = meta["tokens"]
    cfg = OmniLMMConfig(hidden=512, layers=2, heads=4, kv_heads=2, ffn=768, vocab=325, model_max_length=256,
                        num_query=meta["num_query"], vision_width=meta["kv_dim"], image_size=84,
                        im_patch_token=pt, im_start_token=st, im_end_token=en)
    ocfg = O.LlavaCfg(hidden=512, layers=2, heads=4, kv_heads=2, ffn=768, vocab=325, model_max_length=256)
    W = {k: v for k, v in O.make_weights(ocfg, seed=3).items() if "vision_tower" not in k and "mm_projector" not in k}
    W.update(OO.make_resampler_weights(512, meta["kv_dim"], meta["num_query"]))
    model = OmniLMMDPOModel(cfg)
    model.load_state_dict(W)
    assert model.share_prefix and model.splice_keeps_positions
    b = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in case["batch"].items()}
    ids, labels = b["concatenated_input_ids"], b["concatenated_labels"]
    S2, T = ids.shape
    B = S2 // 2
    loader = [dict(concatenated_input_ids=ids, concatenated_labels=labels, images=case["tower_features"])]
    with pytest.raises(ValueError, match="share_prefix"):
        get_multimodal_sample_logps(_NoShare(model), loader, is_llava15=False, packed=True)
    wl, wa, wp, rl, ra, rp = get_multimodal_sample_logps(model, loader, is_llava15=False, packed=True)
    assert all(len(x) == T - 1 for x in wp + rp) and len(wp) == len(rp) == B
    # the packed token-weighted training forward on the same weights, fed with these reference values
    gw = torch.Generator().manual_seed(7)
    tw = (0.25 + 2.0 * torch.rand(S2, T - 1, generator=gw)).float()
    b.update(win_token_weight=tw[:B], rej_token_weight=tw[B:], concatenated_token_weight=tw,
             ref_win_per_token_logp=torch.tensor(wp), ref_rej_per_token_logp=torch.tensor(rp), images=case["tower_features"])
    tr = OmniLMMDPOTrainer(model=model, args=TrainingArguments(dpo_token_weighted=True))
    model.train(True)
    tr.compute_loss(model, dict(b))
    out = model.last_out
    per = torch.tensor(wp + rp)
    mask = labels[:, 1:] != -100
    assert torch.equal(per[mask], out.per_token_logp.float().cpu())              # row-major = the plan's (sequence, position) order
    ref_w = compute_weighted_logp(per.to(model.device), labels, tw, False).cpu()
    torch.testing.assert_close(ref_w, out.seq_logp.float().cpu(), rtol=1e-6, atol=0.0)
    m = tr.pop_metrics()
    print(f"omnilmm packed precompute: weighted ref {ref_w.tolist()} policy {out.seq_logp.tolist()} rewards "
          f"{m['rewards_train/chosen']:.3e} {m['rewards_train/rejected']:.3e}")


class _NoShare:
    """A model whose share_prefix is off: the packed precompute must refuse it."""

    def __init__(self, model):
        self._m = model
        self.share_prefix = False

    def __getattr__(self, k):
        return getattr(self._m, k)
