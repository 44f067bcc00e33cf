"""Forward-only throughput of the reference log-prob precompute (inference_logp) at the 7B configuration on RLAIF-V-shaped
lengths, un-packed against packed, and the step-0 consistency of both modes at full depth.

    timeout -k 10 1100 python tools/bench_precompute.py [--pairs 24] [--layers 32] [--out profiles/r09_precompute_packed.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_precompute.py --no-step0 --reps 1

One process, nothing spawned.  Three cases over the same ``--pairs`` synthetic pairs (the length generator of ``bench.py
--ragged``: SyntheticPreferenceDataset(length_dist="rlaifv")), alternated ``--reps`` times after ``--warmup`` passes each:

    unpacked_bs1   one un-packed forward per branch, batch size 1 (the reference's setting)
    unpacked_bs8   the same at batch size 8 (rows right-padded to the batch maximum)
    packed_bs8     one forward per batch on the packed [shared prefix | chosen | rejected] layout (model.pad_free as configured)

Each case reports pairs/s (median and every repetition) and the token rows it pushes through the decoder per pair; the ratio of
those row counts is what the packed mode can be expected to gain.  The step-0 check then runs BASELINE config 1's batch (the
weights and batch of tests/full_depth.py, case cfg1_step) through the precompute in both modes and through the packed training
forward on the same weights, and records ``delta_nats`` = policy - reference per row beside the figures of
profiles/r06_parity_full_depth.json."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))          # tests/full_depth.py: the full-depth cases' weights and batches

import torch  # noqa: E402

CASES = (("unpacked_bs1", 1, False), ("unpacked_bs8", 8, False), ("packed_bs8", 8, True))


def token_rows(batches, model, packed):
    """Rows of the token-major activation buffers one pass over ``batches`` pushes through the decoder, and LM-head rows."""
    from rlaif_v_amd.splice import build_packed_plan, build_splice_plan
    cfg = model.cfg
    rows = head = 0
    for b in batches:
        B = len(b["images"])
        if packed:
            p = build_packed_plan(b["concatenated_input_ids"], b["concatenated_labels"], cfg.n_image_tokens, B, cfg.model_max_length,
                                  cfg.pad_token_id, pad_free=model.pad_free, all_rows=True)
            rows, head = rows + p.n_tokens, head + p.n_ev
        else:
            for key in ("win", "rej"):
                p = build_splice_plan(b[f"{key}_input_ids"], b[f"{key}_labels"], cfg.n_image_tokens, B, cfg.model_max_length)
                rows, head = rows + p.n_tokens, head + p.S * (p.L - 1)
    return rows, head


def step0(model, trainer, FD, ocfg):
    """cfg1's batch: reference values from the precompute (either mode), policy values from the packed training forward."""
    from rlaif_v_amd.inference_logp import get_multimodal_sample_logps
    batch = FD.make_batch("cfg1_step", ocfg)
    B = batch["win_input_ids"].shape[0]
    rows = [{k: (v[i:i + 1] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == B else v) for k, v in batch.items()}
            for i in range(B)]
    out = {}
    for mode in ("unpacked", "packed"):
        if mode == "packed":
            win_lp, _, _, rej_lp, _, _ = get_multimodal_sample_logps(model, [dict(batch)], packed=True)
        else:
            win_lp, _, _, rej_lp, _, _ = get_multimodal_sample_logps(model, rows)      # batch size 1, as the r06 record
        b = dict(batch)
        b["ref_win_logp"], b["ref_rej_logp"] = torch.tensor(win_lp), torch.tensor(rej_lp)
        model.train(True)
        loss = trainer.compute_loss(model, b)
        pol = model.last_out.seq_logp.float().cpu()
        model.last_out = None
        model.eval()
        delta = (pol - torch.tensor(win_lp + rej_lp)).tolist()
        m = trainer.pop_metrics()
        out[mode] = dict(delta_nats=delta, loss=float(loss), ln2=0.6931472, seq_logp=pol.tolist(),
                         rewards_chosen=m["rewards_train/chosen"], rewards_rejected=m["rewards_train/rejected"])
        print(f"[step0] {mode}: loss {float(loss):.7f} delta_nats {delta}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=24, help="pairs every case processes per pass (a multiple of 8)")
    ap.add_argument("--layers", type=int, default=32, help="debug only: anything but 32 is not the 7B configuration")
    ap.add_argument("--seq-len", type=int, default=2048, help="model_max_length (spliced)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-step0", action="store_true", help="throughput only, on random weights (no 27 GB of seeded host weights)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r09_precompute_packed.json"))
    args = ap.parse_args()
    if args.pairs % 8:
        raise SystemExit("--pairs must be a multiple of 8")

    import full_depth as FD
    from oracle import dpo_oracle as O
    from rlaif_v_amd.data import SyntheticPreferenceDataset, preference_collator_fn
    from rlaif_v_amd.inference_logp import get_multimodal_sample_logps
    from rlaif_v_amd.model import LlavaConfig, LlavaDPOModel
    from rlaif_v_amd.trainer import LLaVA15DPOTrainer, TrainingArguments

    dev = torch.device("cuda", 0)
    t0 = time.time()
    ocfg = O.LlavaCfg(layers=args.layers, model_max_length=args.seq_len)
    model = LlavaDPOModel(LlavaConfig(**O.asdict(ocfg)), device=dev, with_optimizer=False)
    if args.no_step0:
        model.init_random(seed=0)
    else:
        model.load_state_dict(O.make_weights(ocfg, seed=FD.WEIGHT_SEED))
    model.eval()
    trainer = LLaVA15DPOTrainer(model=model, args=TrainingArguments())
    print(f"[bench_precompute] model ready in {time.time() - t0:.0f} s (share_prefix={model.share_prefix}, pad_free={model.pad_free})",
          flush=True)
    if not model.share_prefix:
        raise SystemExit("the packed precompute needs share_prefix (RV_SHARE_PREFIX=0 is set)")

    cfg = model.cfg
    ds = SyntheticPreferenceDataset(n=args.pairs, vocab=cfg.vocab, text_len=args.seq_len - (cfg.n_patches - 1), prompt_len=64,
                                    image_size=cfg.image_size, seed=1234, length_dist="rlaifv")
    items = [ds[i] for i in range(args.pairs)]
    batches = {}
    for bs in (1, 8):
        batches[bs] = [preference_collator_fn(items[i:i + bs], cfg.pad_token_id) for i in range(0, args.pairs, bs)]
        for b in batches[bs]:
            b["images"] = b["images"].to(dev)            # inputs resident in HBM before the timed region

    def run(bs, packed):
        torch.cuda.synchronize()
        t = time.perf_counter()
        get_multimodal_sample_logps(model, batches[bs], packed=packed)      # ends with the one device -> host transfer
        torch.cuda.synchronize()
        return args.pairs / (time.perf_counter() - t)

    result = {name: dict(batch_size=bs, packed=packed, pairs_per_s_runs=[]) for name, bs, packed in CASES}
    for name, bs, packed in CASES:
        rows, head = token_rows(batches[bs], model, packed)
        result[name].update(token_rows_per_pair=rows / args.pairs, lm_head_rows_per_pair=head / args.pairs)
        for _ in range(args.warmup):
            run(bs, packed)
    for rep in range(args.reps):                          # alternate the cases: clock / thermal drift hits all three alike
        for name, bs, packed in CASES:
            v = run(bs, packed)
            result[name]["pairs_per_s_runs"].append(round(v, 3))
            print(f"[bench_precompute] rep {rep} {name}: {v:.2f} pairs/s", flush=True)
    for name in result:
        result[name]["pairs_per_s"] = round(statistics.median(result[name]["pairs_per_s_runs"]), 3)
    u8, p8 = result["unpacked_bs8"], result["packed_bs8"]
    line = dict(tool="tools/bench_precompute.py", device=torch.cuda.get_device_name(0), layers=args.layers, model_max_length=args.seq_len,
                pairs=args.pairs, warmup=args.warmup, reps=args.reps, pad_free=model.pad_free,
                length_dist="rlaifv (SyntheticPreferenceDataset, seed 1234: the generator of bench.py --ragged)",
                weights="random (init_random)" if args.no_step0 else f"seeded, tests/full_depth.py WEIGHT_SEED {FD.WEIGHT_SEED}",
                cases=result,
                row_ratio_unpacked_bs8_over_packed_bs8=round(u8["token_rows_per_pair"] / p8["token_rows_per_pair"], 4),
                row_ratio_unpacked_bs1_over_packed_bs8=round(result["unpacked_bs1"]["token_rows_per_pair"] / p8["token_rows_per_pair"], 4),
                speedup_packed_bs8_over_unpacked_bs8=round(p8["pairs_per_s"] / u8["pairs_per_s"], 4),
                speedup_packed_bs8_over_unpacked_bs1=round(p8["pairs_per_s"] / result["unpacked_bs1"]["pairs_per_s"], 4))
    if not args.no_step0:
        if args.layers != 32:
            print("[bench_precompute] step-0 check below is NOT at full depth", flush=True)
        s0 = step0(model, trainer, FD, ocfg)
        r06_path = os.path.join(REPO, "profiles", "r06_parity_full_depth.json")
        if os.path.exists(r06_path):
            r06 = json.load(open(r06_path)).get("step0_self_consistency_cfg1_step", {})
            s0["r06_unpacked_record"] = dict(delta_nats=r06.get("delta_nats"), loss=r06.get("loss"))
        line["step0_cfg1_full_depth" if args.layers == 32 else f"step0_cfg1_{args.layers}_layers"] = s0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(line, open(args.out, "w"), indent=1)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
