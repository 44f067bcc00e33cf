"""Cost of OmniLMM candidate generation at the OmniLMM-12B decoder shape (d 4096, f 14336, 32 query / 8 key-value heads,
V 32009, 32 layers, 64 resampler queries over 1024 tower tokens of width 1792; random weights, precomputed tower tokens): a
prompt of 130 tokens (bos + 34 system tokens + <im_start> <im_patch> x 64 <im_end> + a 29-token question), 128 new tokens,
temperature 0.7, repetition_penalty 1.1 - the sampling call of omnilmm/omnilmm_gen_data.py - and of the kernel its beam branch
adds.

    python tools/bench_omni_generate.py [--out profiles/omni_generate.json]

The driver starts every GPU part as a child process of its own under ``timeout -k 10`` and stops at the first part that does
not end with status 0 (nothing more is started on a device after a fault, an abort or a time limit).  Parts:

  kernels     rv_beam_topk_penalty against rv_beam_topk at K = 3, V = 32009 (row stride 32064), G in {1, 6}, penalty 1.1,
              n_hist in {0, 64, 512, 1023} of a 1024-column history of random ids: the two kernels ALTERNATE in one process,
              one warm-up round, then ``--kreps`` rounds of 20 back-to-back calls each between HIP events; median and
              min - max of the rounds, microseconds per call (two launches: rows, merge).
  generate    ms per decode step (HIP events around ``_decode_step``) and tokens/s of generate() at 6 prompts x 10 samples.
  continuous  the same for generate_continuous() at 64 slots: 24 requests x 10 samples whose budgets run from 32 to 128 tokens,
              so that rows finish at different steps and are refilled.

No threshold is fixed in advance: the penalised kernel is reported against the plain one measured beside it, and as a share
of the decode step of the ``generate`` part.  A part that did not run is written "not measured".  The result goes to ``--out``."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NEW_TOKENS, SYSTEM, QUESTION, K, TOWER_TOKENS = 128, 34, 29, 3, 1024
PARTS = ("kernels", "generate", "continuous")


def _merge(path, key, value):
    blob = {}
    if os.path.exists(path):
        try:
            blob = json.load(open(path))
        except ValueError:
            blob = {}
    blob[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(blob, open(path, "w"), indent=1)


def _stats(v):
    return dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))


def part_kernels(args):
    import torch
    from rlaif_v_amd import ops
    dev = torch.device("cuda", 0)
    V, LD, T = 32009, 32064, 1024
    g = torch.Generator().manual_seed(0)
    rows = []
    for G in (1, 6):
        M = G * K
        logits = torch.zeros(M, LD, dtype=torch.float32)
        logits[:, :V] = torch.randn(M, V, generator=g) * 3
        logits = logits.to(dev)
        score = (-torch.rand(M, generator=g) * 4).to(dev)
        hist = torch.randint(0, V, (M, T), generator=g).to(torch.int32).to(dev)
        plain = lambda: ops.beam_topk(logits, score, G, K, V)                                         # noqa: E731
        for n_hist in (0, 64, 512, 1023):
            pen = lambda n=n_hist: ops.beam_topk(logits, score, G, K, V, hist=hist, n_hist=n, penalty=1.1)    # noqa: E731
            same = all(bool(torch.equal(a, b)) for a, b in zip(plain(), pen()))
            t = {"plain": [], "penalty": []}
            for rep in range(1 + args.kreps):                           # round 0 is the warm-up
                for key, fn in (("plain", plain), ("penalty", pen)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(20):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    if rep:
                        t[key].append(e0.elapsed_time(e1) / 20 * 1e3)
            row = dict(G=G, K=K, V=V, n_hist=n_hist, rv_beam_topk_us=_stats(t["plain"]), rv_beam_topk_penalty_us=_stats(t["penalty"]),
                       penalty_minus_plain_us=round(statistics.median(t["penalty"]) - statistics.median(t["plain"]), 2),
                       same_outputs_as_plain=same)
            rows.append(row)
            print(f"[bench_omni_generate] G {G} n_hist {n_hist}: plain {row['rv_beam_topk_us']}, penalty {row['rv_beam_topk_penalty_us']}", flush=True)
    _merge(args.out, "kernels", dict(device=torch.cuda.get_device_name(0), rounds=args.kreps, calls_per_round=20, penalty=1.1, rows=rows,
                                     note="microseconds per ops.beam_topk call: output allocation, the row kernel and the merge kernel, "
                                          "host launch time included where the device waits for it; n_hist 0 launches the plain kernel"))
    print(json.dumps(dict(part="kernels", rows=len(rows))))


def _model(args):
    import torch
    from rlaif_v_amd.omnilmm import OmniLMMConfig, OmniLMMDPOModel
    t0 = time.time()
    model = OmniLMMDPOModel(OmniLMMConfig(layers=args.layers), device=torch.device("cuda", 0), with_optimizer=False)
    model.init_random(seed=0)
    model.eval()
    print(f"[bench_omni_generate] model ready in {time.time() - t0:.0f} s", flush=True)
    return model


def _prompt(cfg, g):
    import torch
    return torch.cat([torch.tensor([1]), torch.randint(3, 32000, (SYSTEM,), generator=g),
                      torch.tensor([cfg.im_start_token] + [cfg.im_patch_token] * cfg.num_query + [cfg.im_end_token]),
                      torch.randint(3, 32000, (QUESTION,), generator=g)])


def _timed_steps(model, events):
    import torch
    real = model._decode_step

    def timed(*a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = real(*a, **kw)
        e1.record()
        events.append((e0, e1))
        return r
    return real, timed


def part_generate(args):
    import torch
    model = _model(args)
    cfg, dev = model.cfg, model.device
    g = torch.Generator().manual_seed(1234)
    n_prompts, repeat = 6, 10
    prompts = [_prompt(cfg, g) for _ in range(n_prompts)]
    tower = torch.randn(n_prompts, TOWER_TOKENS, cfg.vision_width, generator=g).bfloat16().to(dev)
    events, runs = [], []
    real, timed = _timed_steps(model, events)
    for rep in range(args.warmup + args.reps):
        events.clear()
        model._decode_step = timed
        try:
            torch.cuda.synchronize()
            t = time.perf_counter()
            toks = model.generate(prompts, tower, NEW_TOKENS, repeat=repeat, temperature=0.7, repetition_penalty=1.1,
                                  generator=torch.Generator().manual_seed(rep))
            torch.cuda.synchronize()
            wall = time.perf_counter() - t
        finally:
            model._decode_step = real
        n_tok = sum(len(s) for p in toks for s in p)
        step_ms = [a.elapsed_time(b) for a, b in events]
        if rep >= args.warmup:
            runs.append(dict(wall_s=round(wall, 4), tokens=n_tok, tokens_per_s=round(n_tok / wall, 1),
                             decode_step_ms=round(statistics.median(step_ms), 4), decode_step_ms_min=round(min(step_ms), 4),
                             decode_step_ms_max=round(max(step_ms), 4)))
        print(f"[bench_omni_generate] generate {n_prompts} x {repeat} rep {rep}: {n_tok / wall:.1f} tokens/s, decode step "
              f"{statistics.median(step_ms):.3f} ms", flush=True)
    med = statistics.median(r["decode_step_ms"] for r in runs)
    out = dict(device=torch.cuda.get_device_name(0), layers=cfg.layers, hidden=cfg.hidden, ffn=cfg.ffn, heads=cfg.heads, kv_heads=cfg.n_kv_heads,
               vocab=cfg.vocab, prompts=n_prompts, repeat=repeat, rows=n_prompts * repeat, prompt_tokens=int(prompts[0].numel()),
               new_tokens=NEW_TOKENS, temperature=0.7, repetition_penalty=1.1, weights="random (init_random)",
               images="precomputed tower tokens [1024, 1792] per prompt", runs=runs, decode_step_ms=med,
               tokens_per_s=statistics.median(r["tokens_per_s"] for r in runs),
               decode_tokens_per_s=round(n_prompts * repeat / med * 1e3, 1))
    _merge(args.out, "generate", out)
    print(json.dumps(dict(part="generate", decode_step_ms=med, tokens_per_s=out["tokens_per_s"])))


def part_continuous(args):
    import torch
    model = _model(args)
    cfg, dev = model.cfg, model.device
    g = torch.Generator().manual_seed(1234)
    n_req, repeat, slots = 24, 10, 64
    prompts = [_prompt(cfg, g) for _ in range(n_req)]
    tower = torch.randn(6, TOWER_TOKENS, cfg.vision_width, generator=g).bfloat16().to(dev)
    budgets = [32 + (96 * i) // (n_req - 1) for i in range(n_req)]
    budgets = [budgets[(7 * i) % n_req] for i in range(n_req)]          # a fixed shuffle: short and long requests interleaved
    reqs = [(prompts[i], tower[i % 6], budgets[i]) for i in range(n_req)]
    events, runs = [], []
    real, timed = _timed_steps(model, events)
    for rep in range(args.warmup + args.reps):
        events.clear()
        sched = []
        model._decode_step = timed
        try:
            torch.cuda.synchronize()
            t = time.perf_counter()
            got = dict(model.generate_continuous(reqs, NEW_TOKENS, slots=slots, repeat=repeat, temperature=0.7, repetition_penalty=1.1,
                                                 seed=rep, max_prompt_tokens=int(prompts[0].numel()), _scheduler=sched))
            torch.cuda.synchronize()
            wall = time.perf_counter() - t
        finally:
            model._decode_step = real
        n_tok = sum(len(s) for v in got.values() for s in v)
        step_ms = [a.elapsed_time(b) for a, b in events]
        if rep >= args.warmup:
            runs.append(dict(wall_s=round(wall, 4), tokens=n_tok, tokens_per_s=round(n_tok / wall, 1),
                             decode_step_ms=round(statistics.median(step_ms), 4), decode_step_ms_min=round(min(step_ms), 4),
                             decode_step_ms_max=round(max(step_ms), 4), decode_steps=sched[0].steps_executed, polls=sched[0].polls))
        print(f"[bench_omni_generate] continuous {n_req} x {repeat} in {slots} slots rep {rep}: {n_tok / wall:.1f} tokens/s, decode step "
              f"{statistics.median(step_ms):.3f} ms, {sched[0].steps_executed} steps", flush=True)
    out = dict(device=torch.cuda.get_device_name(0), layers=cfg.layers, requests=n_req, repeat=repeat, slots=slots, budgets=budgets,
               prompt_tokens=int(prompts[0].numel()), max_new_tokens=NEW_TOKENS, temperature=0.7, repetition_penalty=1.1,
               weights="random (init_random)", runs=runs, decode_step_ms=statistics.median(r["decode_step_ms"] for r in runs),
               tokens_per_s=statistics.median(r["tokens_per_s"] for r in runs),
               note="tokens_per_s counts prefills and polls (wall time of the whole call); 24 prompts are prefilled, 8 per call at most")
    _merge(args.out, "continuous", out)
    print(json.dumps(dict(part="continuous", decode_step_ms=out["decode_step_ms"], tokens_per_s=out["tokens_per_s"])))


def _summary(path):
    """the penalised kernel's extra cost as a share of the decode step measured beside it"""
    blob = json.load(open(path))
    for part in PARTS:
        blob.setdefault(part, "not measured")
    if isinstance(blob["kernels"], dict) and isinstance(blob["generate"], dict):
        step_us = blob["generate"]["decode_step_ms"] * 1e3
        worst = max(blob["kernels"]["rows"], key=lambda r: r["rv_beam_topk_penalty_us"]["median"])
        blob["summary"] = dict(decode_step_us=round(step_us, 1), slowest_penalised_call=dict(G=worst["G"], n_hist=worst["n_hist"],
                               us=worst["rv_beam_topk_penalty_us"]["median"], plain_us=worst["rv_beam_topk_us"]["median"]),
                               penalised_call_share_of_decode_step=round(worst["rv_beam_topk_penalty_us"]["median"] / step_us, 5),
                               penalty_extra_share_of_decode_step=round(max(r["penalty_minus_plain_us"] for r in blob["kernels"]["rows"]) / step_us, 5))
    else:
        blob["summary"] = "not measured"
    json.dump(blob, open(path, "w"), indent=1)
    return blob


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=PARTS, help="run one part in this process (what the driver starts)")
    ap.add_argument("--parts", nargs="+", choices=PARTS, default=list(PARTS), help="the parts the driver runs, in order")
    ap.add_argument("--layers", type=int, default=32, help="debug only: anything but 32 is not the 12B configuration's decoder")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kreps", type=int, default=15, help="timed rounds of the kernels part")
    ap.add_argument("--limits", type=int, nargs=3, default=[120, 300, 360], help="time limits of the three parts, seconds")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "omni_generate.json"))
    args = ap.parse_args()
    if args.part:
        return dict(kernels=part_kernels, generate=part_generate, continuous=part_continuous)[args.part](args)
    for part in args.parts:
        limit = args.limits[PARTS.index(part)]
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part, "--layers", str(args.layers),
               "--warmup", str(args.warmup), "--reps", str(args.reps), "--kreps", str(args.kreps), "--out", args.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"[bench_omni_generate] part {part} ended with status {rc}: nothing more is started", file=sys.stderr)
            if os.path.exists(args.out):
                _summary(args.out)
            sys.exit(rc)
    print(json.dumps(_summary(args.out), indent=1))


if __name__ == "__main__":
    main()
