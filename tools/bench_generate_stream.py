"""Continuous batching against fixed chunks at the 7B LLaVA-1.5 shape: 32 layers, prompts of 640 spliced tokens (bos + 34 system
tokens + 576 image tokens + a 29-token question), 48 items x 10 samples, temperature 0.7, at most 512 new tokens.

    python tools/bench_generate_stream.py [--out profiles/generate_stream.json]

A random-weight model never emits EOS, so every sample gets a budget from a seeded length table (schedule.length_table:
log-normal, median 90, sigma 0.6, clipped to [1, 512] - an ASSUMED distribution) that plays EOS's part:

  generate    LlavaDPOModel.generate on 6 items x 10 samples per call (the stage's --batch_size 6), each call decoding what it
              would with answers of these lengths: until its longest sample has ended and the flags are read, i.e.
              ceil(longest / 8) * 8 sampler rounds (at most 512);
  continuous  LlavaDPOModel.generate_continuous on the same items with 64 slots and the per-sample budgets.

The two run alternately in ONE process on the same items, ``--reps`` times after ``--warmup``.  Reported for both: useful
tokens/s (the budgets' sum over the wall time, prefills included), decode steps executed, ms per decode step (HIP events
around _decode_step, median) and wall ms per step, each with its spread over the repeats; and the scheduler's host count of
the continuous path's steps (schedule.simulate), which must match.

The driver starts the GPU part as a child process of its own under ``timeout -k 10`` and stops if it does not end with
status 0.  Random weights (init_random).  The result is written to ``--out``."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ITEMS, REPEAT, SLOTS, MAX_NEW, PER_CALL, POLL = 48, 10, 64, 512, 6, 8
SYSTEM, QUESTION = 34, 29


def _spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def part_stream(args):
    import torch
    from oracle import dpo_oracle as O
    from rlaif_v_amd import schedule
    from rlaif_v_amd.model import LlavaConfig, LlavaDPOModel
    dev = torch.device("cuda", 0)
    t0 = time.time()
    model = LlavaDPOModel(LlavaConfig(**O.asdict(O.LlavaCfg(layers=args.layers))), device=dev, with_optimizer=False)
    model.init_random(seed=0)
    model.eval()
    cfg = model.cfg
    print(f"[bench_generate_stream] model ready in {time.time() - t0:.0f} s", flush=True)
    g = torch.Generator().manual_seed(1234)
    n_items = args.items
    prompts = [torch.cat([torch.tensor([1]), torch.randint(3, cfg.vocab, (SYSTEM,), generator=g), torch.tensor([-200]),
                          torch.randint(3, cfg.vocab, (QUESTION,), generator=g)]) for _ in range(n_items)]
    pixels = torch.randn(n_items, 3, cfg.image_size, cfg.image_size, generator=g).to(dev)
    prompt_tokens = int(prompts[0].numel()) - 1 + cfg.n_image_tokens
    flat = schedule.length_table(n_items * REPEAT, args.length_seed, hi=MAX_NEW)
    lengths = [flat[i * REPEAT:(i + 1) * REPEAT] for i in range(n_items)]
    useful = sum(flat)
    host = schedule.simulate(lengths, SLOTS, REPEAT, poll_every=POLL, known=True)
    static_steps = schedule.static_decode_steps(lengths, PER_CALL, MAX_NEW, POLL)
    real_step = model._decode_step
    events = []

    def timed(*a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = real_step(*a, **kw)
        e1.record()
        events.append((e0, e1))
        return r

    def run_generate(rep):
        steps = 0
        for i0 in range(0, n_items, PER_CALL):
            longest = max(max(ls) for ls in lengths[i0:i0 + PER_CALL])
            rounds = min(MAX_NEW, -(-longest // POLL) * POLL)
            model.generate(prompts[i0:i0 + PER_CALL], pixels[i0:i0 + PER_CALL], rounds, repeat=REPEAT, temperature=0.7,
                           generator=torch.Generator().manual_seed(rep))
            steps += rounds - 1
        return steps

    def run_continuous(rep):
        sched = []
        reqs = ((prompts[i], pixels[i], lengths[i]) for i in range(n_items))
        got = dict(model.generate_continuous(reqs, MAX_NEW, slots=SLOTS, repeat=REPEAT, temperature=0.7, seed=rep,
                                             max_prompt_tokens=prompt_tokens, poll_every=POLL, _scheduler=sched))
        assert all([len(t) for t in got[i]] == lengths[i] for i in range(n_items)), "every sample used its budget"
        return sched[0].steps_executed

    runs = {"generate": [], "continuous": []}
    for rep in range(args.warmup + args.reps):
        for name, fn in (("generate", run_generate), ("continuous", run_continuous)):
            events.clear()
            model._decode_step = timed
            try:
                torch.cuda.synchronize()
                t = time.perf_counter()
                steps = fn(rep)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t
            finally:
                model._decode_step = real_step
            step_ms = statistics.median(a.elapsed_time(b) for a, b in events)
            print(f"[bench_generate_stream] rep {rep} {name}: {useful / wall:.1f} useful tokens/s, {steps} decode steps, "
                  f"decode step {step_ms:.3f} ms, wall {wall:.2f} s", flush=True)
            if rep >= args.warmup:
                runs[name].append(dict(wall_s=round(wall, 4), useful_tokens_per_s=round(useful / wall, 1), decode_steps=steps,
                                       decode_step_ms=round(step_ms, 4), wall_ms_per_step=round(wall / steps * 1e3, 4)))
    out = dict(device=torch.cuda.get_device_name(0), layers=cfg.layers, items=n_items, repeat=REPEAT, slots=SLOTS,
               prompt_tokens=prompt_tokens, max_new_tokens=MAX_NEW, poll_every=POLL, items_per_generate_call=PER_CALL,
               temperature=0.7, weights="random (init_random)", useful_tokens=useful, length_seed=args.length_seed,
               lengths="schedule.length_table: log-normal, median 90, sigma 0.6, clipped to [1, 512] - assumed, not measured",
               warmup=args.warmup, reps=args.reps, host_steps=dict(generate=static_steps, continuous=host.steps_executed))
    for name, rs in runs.items():
        out[name] = dict(runs=rs, decode_steps=rs[0]["decode_steps"],
                         useful_tokens_per_s=_spread([r["useful_tokens_per_s"] for r in rs]),
                         decode_step_ms=_spread([r["decode_step_ms"] for r in rs]),
                         wall_ms_per_step=_spread([r["wall_ms_per_step"] for r in rs]))
    out["steps_match_host_count"] = all(r["decode_steps"] == host.steps_executed for r in runs["continuous"]) and \
        all(r["decode_steps"] == static_steps for r in runs["generate"])
    out["note"] = ("decode_step_ms: HIP events around _decode_step (one chunk of <= 64 rows), median over the run's steps; "
                   "wall_ms_per_step: wall time / decode steps, prefills, sampler, bookkeeping and read-backs included; "
                   "useful tokens: the budgets' sum, the same for both paths")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(dict(part="stream", steps=out["host_steps"], match=out["steps_match_host_count"],
                          tokens_per_s={k: out[k]["useful_tokens_per_s"]["median"] for k in runs},
                          decode_step_ms={k: out[k]["decode_step_ms"]["median"] for k in runs})))
    if not out["steps_match_host_count"]:
        sys.exit(3)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=("stream",), help="run the GPU part in this process (what the driver starts)")
    ap.add_argument("--layers", type=int, default=32, help="debug only: anything but 32 is not the 7B configuration")
    ap.add_argument("--items", type=int, default=ITEMS, help="debug only: anything but 48 is not the stated workload")
    ap.add_argument("--length-seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=900, help="time limit of the GPU part, seconds")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "generate_stream.json"))
    args = ap.parse_args()
    if args.part == "stream":
        return part_stream(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--part", "stream", "--layers",
           str(args.layers), "--items", str(args.items), "--length-seed", str(args.length_seed), "--warmup", str(args.warmup),
           "--reps", str(args.reps), "--out", args.out]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"[bench_generate_stream] the GPU part ended with status {rc}: nothing more is started", file=sys.stderr)
        sys.exit(rc)
    print(open(args.out).read())


if __name__ == "__main__":
    main()
