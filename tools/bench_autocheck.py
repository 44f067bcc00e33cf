"""Throughput of the yes / no feedback scoring (LlavaDPOModel.forward_next_token_scores) at the 7B LLaVA-1.5 shape: one
plain causal row per question (``packed=False``, what the reference's per-question generate costs in token rows) against
the N-branch rows that compute every image's shared prefix once (``packed=True``).

    timeout -k 10 900 python tools/bench_autocheck.py [--images 8] [--questions 16] [--layers 32] [--out bench_outputs/r10_autocheck.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_autocheck.py --only packed --reps 3 --out DIR/line.json

One process, nothing spawned.  Random weights (init_random), ``--images`` x ``--questions`` prompts
[bos, 34 system tokens, <image>, own tail] with tails drawn uniformly from [32, 64] tokens (mean 48) from a fixed seed.  The two
modes alternate ``--reps`` times after ``--warmup`` passes each and report questions/s (median and every repetition), the
token rows per question they push through the decoder, and the time of the decoder's attention launches per layer (HIP
events around ops.attn_fwd in one extra pass).  The expectation for the speed-up is the token-row ratio; the measured ratio
is written next to it.  The result is merged into ``--out`` under the key ``throughput`` (the parity figures of
tests/test_autocheck_gpu.py live in the same file)."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402


def make_prompts(n_images, n_questions, vocab, seed=1234, system_len=34, lo=32, hi=64):
    g = torch.Generator().manual_seed(seed)
    system = torch.cat([torch.tensor([1]), torch.randint(3, vocab, (system_len,), generator=g)])
    prompts = []
    for _ in range(n_images):
        tails = torch.randint(lo, hi + 1, (n_questions,), generator=g).tolist()
        prompts.append([torch.cat([system, torch.tensor([-200]), torch.randint(3, vocab, (t,), generator=g)]) for t in tails])
    return prompts


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--questions", type=int, default=16)
    ap.add_argument("--layers", type=int, default=32, help="debug only: anything but 32 is not the 7B configuration")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=("packed", "unpacked"), help="run one mode alone (a kernel trace of that mode)")
    ap.add_argument("--out", default=os.path.join(os.environ.get("RV_RECORD_DIR") or os.path.join(REPO, "bench_outputs"), "r10_autocheck.json"))
    args = ap.parse_args()

    from oracle import dpo_oracle as O
    from rlaif_v_amd import ops
    from rlaif_v_amd.model import LlavaConfig, LlavaDPOModel
    from rlaif_v_amd.splice import build_branch_plan

    dev = torch.device("cuda", 0)
    t0 = time.time()
    ocfg = O.LlavaCfg(layers=args.layers)
    model = LlavaDPOModel(LlavaConfig(**O.asdict(ocfg)), device=dev, with_optimizer=False)
    model.init_random(seed=0)
    model.eval()
    cfg = model.cfg
    print(f"[bench_autocheck] model ready in {time.time() - t0:.0f} s (pad_free={model.pad_free})", flush=True)
    prompts = make_prompts(args.images, args.questions, cfg.vocab)
    pixels = torch.randn(args.images, 3, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(5)).to(dev)
    want = [3869, 8241, 694, 1939]                       # yes / Yes / no / No of the llama tokenizer
    n_q = args.images * args.questions

    def run(packed):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = model.forward_next_token_scores(prompts, pixels, want, packed=packed)
        out[0].cpu()                                       # the one device -> host transfer the stage needs
        torch.cuda.synchronize()
        return n_q / (time.perf_counter() - t)

    def attention_ms(packed):
        """Time of the decoder's attention launches in one pass (HIP events around ops.attn_fwd), per layer."""
        real, events = ops.attn_fwd, []

        def timed(*a, **kw):
            if not a[5]:                                   # the vision tower's non-causal attention
                return real(*a, **kw)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = real(*a, **kw)
            e1.record()
            events.append((e0, e1))
            return r
        ops.attn_fwd = timed
        try:
            model.forward_next_token_scores(prompts, pixels, want, packed=packed)
            torch.cuda.synchronize()
        finally:
            ops.attn_fwd = real
        assert len(events) == cfg.layers
        return sum(a.elapsed_time(b) for a, b in events) / len(events)

    modes = [m for m in (("unpacked", False), ("packed", True)) if args.only in (None, m[0])]
    result = {}
    for name, packed in modes:
        plan = build_branch_plan(prompts, cfg.n_image_tokens, cfg.model_max_length, pad_free=True, packed=packed)
        result[name] = dict(packed=packed, token_rows_per_question=plan.n_tokens / n_q, rows=plan.S, longest_row=plan.L,
                            questions_per_s_runs=[])
        for _ in range(args.warmup):
            run(packed)
    for rep in range(args.reps):                           # alternate: clock / thermal drift hits both alike
        for name, packed in modes:
            v = run(packed)
            result[name]["questions_per_s_runs"].append(round(v, 2))
            print(f"[bench_autocheck] rep {rep} {name}: {v:.1f} questions/s", flush=True)
    for name, packed in modes:
        result[name]["questions_per_s"] = round(statistics.median(result[name]["questions_per_s_runs"]), 2)
        result[name]["attention_ms_per_layer"] = round(attention_ms(packed), 4)
    line = dict(tool="tools/bench_autocheck.py", device=torch.cuda.get_device_name(0), layers=args.layers, images=args.images,
                questions_per_image=args.questions, tails="uniform [32, 64] tokens, seed 1234", weights="random (init_random)",
                warmup=args.warmup, reps=args.reps, cases=result)
    if args.only is None:
        u, p = result["unpacked"], result["packed"]
        line.update(expected_speedup_token_row_ratio=round(u["token_rows_per_question"] / p["token_rows_per_question"], 4),
                    measured_speedup_packed_over_unpacked=round(p["questions_per_s"] / u["questions_per_s"], 4),
                    attention_time_ratio_unpacked_over_packed=round(u["attention_ms_per_layer"] / p["attention_ms_per_layer"], 4))
    blob = {}
    if os.path.exists(args.out):
        try:
            blob = json.load(open(args.out))
        except ValueError:
            blob = {}
    blob["throughput" if args.only is None else f"throughput_{args.only}_only"] = line
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(blob, open(args.out, "w"), indent=1)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
