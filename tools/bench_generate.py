"""Throughput of KV-cached candidate generation (LlavaDPOModel.generate) at the 7B LLaVA-1.5 shape: 32 layers, a prompt of about
640 spliced tokens (bos + 34 system tokens + 576 image tokens + a 29-token question), 128 new tokens, prompts x repeat in
{1 x 1, 1 x 10, 6 x 10}, temperature 0.7.

    python tools/bench_generate.py [--out bench_outputs/r11_generate.json]

The driver starts every GPU part as a child process of its own under ``timeout -k 10`` and stops at the first part that does
not end with status 0 (nothing more is started on a device after a fault, an abort or a time limit).  Parts:

  gemm      the five skinny shapes of a decode step (q|k|v, o, gate|up, down, LM head) at M in {1, 10, 60}:
            rv_gemm_nt_skinny_bf16 against rv_gemm_nt_bf16 (LM head: rv_gemm_nt_bf16_f32out) on the same operands, the two
            interleaved, median of ``--reps`` timings of 20 back-to-back launches each.
  generate  tokens/s and ms per decode step (HIP events around the steps 1..127) per case; the parent's only way to a next
            token for comparison - one no-cache prefill of prompt + tokens so far per token through the forward that
            forward_next_token_scores runs, timed at the prompt plus 64 tokens (the mean length of the 128 steps); and the
            weight-streaming floor: decoder + LM-head bytes every step must read, divided by the HBM streaming rate.  That rate
            (6.29 TB/s, a float4 copy) is the measuring guide's figure, not a measurement of this machine: the output says so.

  sampler   one rv_sample_token call at M = 60 rows of V = 32000 (6 prompts x 10 samples) on the LM head's own output of random
            weights, next to the LM-head skinny GEMM that writes those rows: temperature 0.7 (the stage's) and 0.2 with top-p 0.9,
            each without top-k and with top_k = 50 (rv_sample_token_topk: 32 block-wide counts for the select), the calls
            interleaved, median of ``--reps`` timings of 20 back-to-back launches each.
  launches  launches per decode step and chunk: the library's (through hip.call) and every device kernel (torch.profiler),
            from 2- and 3-layer models of the 7B widths.

Random weights (init_random).  The result is written to ``--out``."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_STREAM_TBS = 6.29
CASES = [(1, 1), (1, 10), (6, 10)]
NEW_TOKENS, SYSTEM, QUESTION = 128, 34, 29


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


def part_gemm(args):
    import torch
    from rlaif_v_amd import ops
    dev = torch.device("cuda", 0)
    d, f, V = 4096, 11008, 32000
    shapes = [("qkv", 3 * d, d), ("o", d, d), ("gate_up", 2 * f, d), ("down", d, f), ("lm_head", V, d)]
    g = torch.Generator().manual_seed(0)
    rows = []
    for name, N, K in shapes:
        w = (torch.randn(N, K, generator=g) * 0.02).bfloat16().to(dev)
        for M in (1, 10, 60):
            a = torch.randn(M, K, generator=g).bfloat16().to(dev)
            f32 = name == "lm_head"
            a64 = torch.zeros(64, K, dtype=torch.bfloat16, device=dev)       # the existing kernels' callers pad the rows to 64
            a64[:M] = a

            def old():
                return ops.gemm_nt_f32(a64, w) if f32 else ops.gemm_nt(a, w)

            def new():
                return ops.gemm_nt_skinny(a, w, out_f32=f32)
            ref, got = old()[:M].float(), new().float()
            err = float((ref - got).abs().max())
            t = {"old": [], "new": []}
            for fn in (old, new):
                fn()
            torch.cuda.synchronize()
            for _ in range(args.reps):
                for key, fn in (("old", old), ("new", new)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(20):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    t[key].append(e0.elapsed_time(e1) / 20 * 1e3)
            old_us, new_us = statistics.median(t["old"]), statistics.median(t["new"])
            rows.append(dict(shape=name, M=M, N=N, K=K, nt_us=round(old_us, 2), skinny_us=round(new_us, 2),
                             skinny_tbs=round(N * K * 2 / new_us / 1e6, 3), speedup=round(old_us / new_us, 3), max_abs_diff=err))
            print(f"[bench_generate] {name} M={M}: nt {old_us:.1f} us, skinny {new_us:.1f} us ({N * K * 2 / new_us / 1e6:.2f} TB/s)", flush=True)
    _merge(args.out, "skinny_gemm", dict(device=torch.cuda.get_device_name(0), reps=args.reps, rows=rows))
    print(json.dumps(dict(part="gemm", rows=len(rows))))


def part_sampler(args):
    import torch
    from rlaif_v_amd import ops
    dev = torch.device("cuda", 0)
    M, V, D = 60, 32000, 4096
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(V, D, generator=g) * 0.02).bfloat16().to(dev)
    h = (torch.randn(M, D, generator=g) * 1.5).bfloat16().to(dev)
    logits = torch.empty(M, V, dtype=torch.float32, device=dev)
    ops.gemm_nt_skinny(h, w, out=logits, out_f32=True)
    u = torch.rand(M, generator=g).to(dev)
    fns = {"lm_head_skinny_gemm": lambda: ops.gemm_nt_skinny(h, w, out=logits, out_f32=True)}
    for T, p in ((0.7, 1.0), (0.7, 0.9), (0.2, 0.9)):
        for k in (0, 50):
            fns[f"T{T}_p{p}_k{k}"] = lambda T=T, p=p, k=k: ops.sample_token(logits, M, V, u, T, p, top_k=k)
    fns["greedy"] = lambda: ops.sample_token(logits, M, V, None, 0.0, 1.0)
    t = {k: [] for k in fns}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for key, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t[key].append(e0.elapsed_time(e1) / 20 * 1e3)
    us = {k: round(statistics.median(v), 2) for k, v in t.items()}
    print(f"[bench_generate] sampler M={M} V={V}: {us}", flush=True)
    _merge(args.out, "sampler", dict(device=torch.cuda.get_device_name(0), reps=args.reps, M=M, V=V, K=D,
                                     logit_spread=round(float(logits.max() - logits.min()), 2), us=us,
                                     note="microseconds per call, HIP events around 20 back-to-back launches, median of reps"))
    print(json.dumps(dict(part="sampler", us=us)))


def part_launches(args):
    """Launches of one decode step of one chunk at the 7B widths.  Library launches are counted through hip.call, every device
    kernel (the library's and torch's own: slices made contiguous, fills, index writes) with torch.profiler; one step = the
    difference between generate() with 3 and with 2 new tokens, one layer = the difference between a 3- and a 2-layer model."""
    import torch
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    from oracle import dpo_oracle as O
    from rlaif_v_amd import hip, ops
    from rlaif_v_amd.model import LlavaConfig, LlavaDPOModel
    dev = torch.device("cuda", 0)
    V = 32000
    g = torch.Generator().manual_seed(0)
    px = torch.randn(1, 3, 336, 336, generator=g).to(dev)
    prompt = torch.cat([torch.tensor([1]), torch.randint(3, V, (8,), generator=g), torch.tensor([-200]), torch.randint(3, V, (4,), generator=g)])
    counts, real = [0], hip.call

    def counting(name, *a):
        counts[0] += 2 if name == "rv_attn_decode" else 1               # rv_attn_decode is two launches (splits, combine)
        return real(name, *a)
    lib, kern = {}, {}
    for layers in (2, 3):
        model = LlavaDPOModel(LlavaConfig(**O.asdict(O.LlavaCfg(layers=layers))), device=dev, with_optimizer=False)
        model.init_random(seed=0)
        model.generate([prompt], px, 2, temperature=0.7)                  # warm-up: lazy initialisation stays out of the counts
        for T in (2, 3):
            counts[0] = 0
            hip.call = ops.hip.call = counting
            try:
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    model.generate([prompt], px, T, temperature=0.7)
                    torch.cuda.synchronize()
            finally:
                hip.call = ops.hip.call = real
            lib[(layers, T)] = counts[0]
            kern[(layers, T)] = sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA and
                                    not e.name.lower().startswith(("memcpy", "memset")))
        del model
    out = {}
    for key, c in (("library_launches", lib), ("device_kernels", kern)):
        step2, step3 = c[(2, 3)] - c[(2, 2)], c[(3, 3)] - c[(3, 2)]
        per_layer = step3 - step2
        out[key] = dict(per_step_2_layers=step2, per_step_3_layers=step3, per_layer=per_layer,
                        per_step_32_layers=step2 + 30 * per_layer)
    out["note"] = ("library_launches: kernels launched by this library's entry points; device_kernels: every kernel torch.profiler "
                   "saw on the device, torch's own copies, fills and index writes included; one chunk of <= 64 sequences")
    _merge(args.out, "launches", out)
    print(json.dumps(dict(part="launches", **out)))


def part_generate(args):
    import torch
    from oracle import dpo_oracle as O
    from rlaif_v_amd.model import LlavaConfig, LlavaDPOModel
    dev = torch.device("cuda", 0)
    t0 = time.time()
    model = LlavaDPOModel(LlavaConfig(**O.asdict(O.LlavaCfg(layers=args.layers))), device=dev, with_optimizer=False)
    model.init_random(seed=0)
    model.eval()
    cfg = model.cfg
    print(f"[bench_generate] model ready in {time.time() - t0:.0f} s (resid_fp32={model.resid_fp32})", flush=True)
    g = torch.Generator().manual_seed(1234)

    def prompt(extra=0):
        return torch.cat([torch.tensor([1]), torch.randint(3, cfg.vocab, (SYSTEM,), generator=g), torch.tensor([-200]),
                          torch.randint(3, cfg.vocab, (QUESTION + extra,), generator=g)])
    d, f, kvd = cfg.hidden, cfg.ffn, cfg.kv_dim
    step_bytes = 2 * (cfg.layers * ((d + 2 * kvd) * d + d * d + 2 * f * d + d * f) + cfg.vocab_padded * d)
    floor_ms = step_bytes / (HBM_STREAM_TBS * 1e12) * 1e3
    out = dict(device=torch.cuda.get_device_name(0), layers=cfg.layers, new_tokens=NEW_TOKENS, temperature=0.7,
               prompt_tokens=1 + SYSTEM + cfg.n_image_tokens + QUESTION, weights="random (init_random)",
               weight_bytes_per_step=step_bytes, hbm_stream_tbs=HBM_STREAM_TBS,
               hbm_stream_source="the measuring guide's float4-copy figure for MI355X, NOT measured on this machine",
               weight_streaming_floor_ms_per_step=round(floor_ms, 4), cases=[])
    real_step = model._decode_step
    for n_prompts, repeat in CASES:
        prompts = [prompt() for _ in range(n_prompts)]
        pixels = torch.randn(n_prompts, 3, cfg.image_size, cfg.image_size, generator=g).to(dev)
        events = []

        def timed(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = real_step(*a, **kw)
            e1.record()
            events.append((e0, e1))
            return r
        runs = []
        for rep in range(args.warmup + args.reps):
            events.clear()
            model._decode_step = timed
            try:
                torch.cuda.synchronize()
                t = time.perf_counter()
                toks = model.generate(prompts, pixels, NEW_TOKENS, repeat=repeat, temperature=0.7,
                                      generator=torch.Generator().manual_seed(rep))
                torch.cuda.synchronize()
                wall = time.perf_counter() - t
            finally:
                model._decode_step = real_step
            n_tok = sum(len(s) for p in toks for s in p)
            step_ms = statistics.median(a.elapsed_time(b) for a, b in events)
            if rep >= args.warmup:
                runs.append(dict(wall_s=round(wall, 4), tokens=n_tok, tokens_per_s=round(n_tok / wall, 1), decode_step_ms=round(step_ms, 4)))
            print(f"[bench_generate] {n_prompts} x {repeat} rep {rep}: {n_tok / wall:.1f} tokens/s, decode step {step_ms:.3f} ms", flush=True)
        med = statistics.median(r["decode_step_ms"] for r in runs)
        out["cases"].append(dict(prompts=n_prompts, repeat=repeat, rows=n_prompts * repeat, runs=runs,
                                 tokens_per_s=statistics.median(r["tokens_per_s"] for r in runs), decode_step_ms=med,
                                 decode_tokens_per_s=round(n_prompts * repeat / med * 1e3, 1),
                                 step_over_weight_floor=round(med / floor_ms, 3)))
    # the parent's way to a next token: a no-cache prefill of prompt + tokens so far, per token and sequence
    ext = [prompt(extra=NEW_TOKENS // 2)]
    px = torch.randn(1, 3, cfg.image_size, cfg.image_size, generator=g).to(dev)
    ts = []
    for rep in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        model.forward_next_token_scores([ext], px, [3, 4], packed=False)[2].cpu()
        torch.cuda.synchronize()
        if rep >= args.warmup:
            ts.append((time.perf_counter() - t) * 1e3)
    out["no_cache_prefill_per_token"] = dict(tokens_in_row=int(ext[0].numel()) - 1 + cfg.n_image_tokens, ms_per_token=round(statistics.median(ts), 3),
                                             tokens_per_s=round(1e3 / statistics.median(ts), 2),
                                             note="one sequence, tower included as forward_next_token_scores runs it; the parent has no other "
                                                  "way to a next token")
    _merge(args.out, "generate", out)
    print(json.dumps(dict(part="generate", cases=[(c["rows"], c["tokens_per_s"], c["decode_step_ms"]) for c in out["cases"]],
                          floor_ms=out["weight_streaming_floor_ms_per_step"], no_cache=out["no_cache_prefill_per_token"]["ms_per_token"])))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=("gemm", "generate", "launches", "sampler"), help="run one part in this process (what the driver starts)")
    ap.add_argument("--layers", type=int, default=32, help="debug only: anything but 32 is not the 7B configuration")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limits", type=int, nargs=3, default=[240, 600, 240], help="time limits of the gemm, generate and launches parts, seconds")
    ap.add_argument("--sampler-limit", type=int, default=120, help="time limit of the sampler part, seconds")
    ap.add_argument("--out", default=os.path.join(os.environ.get("RV_RECORD_DIR") or os.path.join(REPO, "bench_outputs"), "r11_generate.json"))
    args = ap.parse_args()
    if args.part == "gemm":
        return part_gemm(args)
    if args.part == "generate":
        return part_generate(args)
    if args.part == "launches":
        return part_launches(args)
    if args.part == "sampler":
        return part_sampler(args)
    for part, limit in zip(("gemm", "generate", "launches", "sampler"), list(args.limits) + [args.sampler_limit]):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part, "--layers", str(args.layers),
               "--warmup", str(args.warmup), "--reps", str(args.reps), "--out", args.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"[bench_generate] part {part} ended with status {rc}: nothing more is started", file=sys.stderr)
            sys.exit(rc)
    print(open(args.out).read())


if __name__ == "__main__":
    main()
