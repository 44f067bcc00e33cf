"""Throughput of the claim-splitting stage's decoding (rlaif_v_amd.divide: TextLMModel.generate) at the Llama-3-8B shape: hidden
4096, 32 layers, 32 / 8 heads, ffn 14336, vocabulary 128256; batches of 4 and 8 prompts of about 300 tokens, 256 new tokens,
temperature 0.2, top-p 0.9 (the stage's settings).  Random weights (init_random).

    python tools/bench_divide.py [--out profiles/divide.json]

The driver starts every GPU part as a child process of its own under ``timeout -k 10`` and stops at the first part that does
not end with status 0 (nothing more is started on a device after a fault, an abort or a time limit).  Parts:

  sampler   one rv_sample_token_wide call at M = 8 and M = 64 rows of V = 128256 next to the LM-head skinny GEMM that writes
            those rows (rv_gemm_nt_skinny_bf16, N = 128256, K = 4096, fp32 out), interleaved, median of ``--reps`` timings of 20
            back-to-back launches each.  Rows: the LM head's own output of random weights scaled to a spread of several units
            (at temperature 0.2 a peaked distribution: the candidate lists stay in LDS), greedy on the same rows, and the worst
            case - temperature 1, top-p 0.9 on a flat row, every token a candidate, every wave spills to the workspace.  Next to
            the stage's row and the flat row the same call with top_k = 50 (rv_sample_token_wide_topk: two more passes over
            the row for the radix select, then at most 50 + ties candidates).
  generate  ms per decode step (HIP events around every _decode_step) and tokens/s per batch, the sampler and the LM head per
            step (HIP events around ops.sample_token_wide; the LM head from a skinny GEMM of the batch's rows timed alone), and the
            weight-streaming floor: decoder + LM-head bytes every step must read, divided by the HBM streaming rate.  That rate
            (6.29 TB/s, a float4 copy) is the measuring guide's figure, not a measurement of this machine: the output says so.

The result is one JSON, written to ``--out``."""
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
V, D = 128256, 4096
BATCHES = (4, 8)
PROMPT_TOKENS, NEW_TOKENS = 300, 256
TEMPERATURE, TOP_P, TOP_K = 0.2, 0.9, 50


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


def _time(fns, reps, inner=20):
    """median microseconds per call of every function in ``fns`` (name -> callable), the functions interleaved"""
    import torch
    t = {k: [] for k in fns}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for key, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t[key].append(e0.elapsed_time(e1) / inner * 1e3)
    return {k: round(statistics.median(v), 2) for k, v in t.items()}


def part_sampler(args):
    import torch
    from rlaif_v_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(V, D, generator=g) * 0.02).bfloat16().to(dev)
    rows = []
    for M in (8, 64):
        h = (torch.randn(M, D, generator=g) * 1.5).bfloat16().to(dev)
        logits = torch.empty(M, V, dtype=torch.float32, device=dev)
        ops.gemm_nt_skinny(h, w, out=logits, out_f32=True)
        flat = (torch.randn(M, V, generator=g) * 1.5).to(dev)
        u = torch.rand(M, generator=g).to(dev)
        ws = torch.empty(ops.sample_token_wide_workspace_floats(M, V), dtype=torch.float32, device=dev)
        spread = float(logits.max() - logits.min())
        fns = {"lm_head_skinny_gemm": lambda: ops.gemm_nt_skinny(h, w, out=logits, out_f32=True),
               "wide_T0.2_p0.9_lm_head_rows": lambda: ops.sample_token_wide(logits, M, V, u, TEMPERATURE, TOP_P, workspace=ws),
               "wide_T0.2_p0.9_k50_lm_head_rows": lambda: ops.sample_token_wide(logits, M, V, u, TEMPERATURE, TOP_P, workspace=ws,
                                                                                  top_k=TOP_K),
               "wide_greedy_lm_head_rows": lambda: ops.sample_token_wide(logits, M, V, None, 0.0, 1.0, workspace=ws),
               "wide_T1_p1_lm_head_rows": lambda: ops.sample_token_wide(logits, M, V, u, 1.0, 1.0, workspace=ws),
               "wide_T1_p0.9_flat_rows_spill": lambda: ops.sample_token_wide(flat, M, V, u, 1.0, TOP_P, workspace=ws),
               "wide_T1_p0.9_k50_flat_rows": lambda: ops.sample_token_wide(flat, M, V, u, 1.0, TOP_P, workspace=ws, top_k=TOP_K)}
        us = _time(fns, args.reps)
        rows.append(dict(M=M, V=V, K=D, logit_spread=round(spread, 2), us=us,
                         lm_head_tbs=round(V * D * 2 / us["lm_head_skinny_gemm"] / 1e6, 3)))
        print(f"[bench_divide] M={M}: {us}", flush=True)
    _merge(args.out, "sampler", dict(device=torch.cuda.get_device_name(0), reps=args.reps, rows=rows,
                                     note="microseconds per call, HIP events around 20 back-to-back launches, median of reps"))
    print(json.dumps(dict(part="sampler", rows=len(rows))))


def part_generate(args):
    import torch
    from rlaif_v_amd import ops
    from rlaif_v_amd.textlm import TextLMConfig, TextLMModel
    dev = torch.device("cuda", 0)
    t0 = time.time()
    model = TextLMModel(TextLMConfig(layers=args.layers), device=dev)
    model.init_random(seed=0)
    cfg = model.cfg
    print(f"[bench_divide] model ready in {time.time() - t0:.0f} s (resid_fp32={model.resid_fp32})", flush=True)
    g = torch.Generator().manual_seed(1234)
    d, f, kvd = cfg.hidden, cfg.ffn, cfg.kv_dim
    step_bytes = 2 * (cfg.layers * ((d + 2 * kvd) * d + d * d + 2 * f * d + d * f) + cfg.vocab_padded * d)
    floor_ms = step_bytes / (HBM_STREAM_TBS * 1e12) * 1e3
    out = dict(device=torch.cuda.get_device_name(0), layers=cfg.layers, hidden=d, heads=cfg.heads, kv_heads=cfg.n_kv_heads, ffn=f,
               vocab=cfg.vocab, prompt_tokens=PROMPT_TOKENS, new_tokens=NEW_TOKENS, temperature=TEMPERATURE, top_p=TOP_P,
               weights="random (init_random)", weight_bytes_per_step=step_bytes, hbm_stream_tbs=HBM_STREAM_TBS,
               hbm_stream_source="the measuring guide's float4-copy figure for MI355X, NOT measured on this machine",
               weight_streaming_floor_ms_per_step=round(floor_ms, 4), cases=[])
    real_step, real_sample = model._decode_step, ops.sample_token_wide
    for n in BATCHES:
        prompts = [torch.cat([torch.tensor([1]), torch.randint(3, cfg.vocab, (PROMPT_TOKENS - 1 + 7 * k,), generator=g)]) for k in range(n)]
        steps, samples = [], []

        def timed(real, sink):
            def run(*a, **kw):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = real(*a, **kw)
                e1.record()
                sink.append((e0, e1))
                return r
            return run
        runs = []
        for rep in range(args.warmup + args.reps):
            del steps[:], samples[:]
            model._decode_step, ops.sample_token_wide = timed(real_step, steps), timed(real_sample, samples)
            try:
                torch.cuda.synchronize()
                t = time.perf_counter()
                toks = model.generate(prompts, None, NEW_TOKENS, temperature=TEMPERATURE, top_p=TOP_P,
                                      generator=torch.Generator().manual_seed(rep))
                torch.cuda.synchronize()
                wall = time.perf_counter() - t
            finally:
                model._decode_step, ops.sample_token_wide = real_step, real_sample
            n_tok = sum(len(s) for p in toks for s in p)
            step_ms = statistics.median(a.elapsed_time(b) for a, b in steps)
            samp_us = statistics.median(a.elapsed_time(b) for a, b in samples) * 1e3
            if rep >= args.warmup:
                runs.append(dict(wall_s=round(wall, 4), tokens=n_tok, tokens_per_s=round(n_tok / wall, 1), decode_step_ms=round(step_ms, 4),
                                 sampler_us=round(samp_us, 2)))
            print(f"[bench_divide] batch {n} rep {rep}: {n_tok / wall:.1f} tokens/s, decode step {step_ms:.3f} ms, sampler {samp_us:.1f} us",
                  flush=True)
        h = torch.randn(n, d, generator=g).bfloat16().to(dev)
        lg = torch.empty(n, cfg.vocab_padded, dtype=torch.float32, device=dev)
        head_us = _time({"lm_head": lambda: ops.gemm_nt_skinny(h, model.store.p("lm_head.weight"), out=lg, out_f32=True)}, args.reps)["lm_head"]
        med = statistics.median(r["decode_step_ms"] for r in runs)
        out["cases"].append(dict(prompts=n, runs=runs, tokens_per_s=statistics.median(r["tokens_per_s"] for r in runs),
                                 decode_step_ms=med, decode_tokens_per_s=round(n / med * 1e3, 1),
                                 sampler_us_per_step=statistics.median(r["sampler_us"] for r in runs), lm_head_us_per_step=head_us,
                                 step_over_weight_floor=round(med / floor_ms, 3)))
    _merge(args.out, "generate", out)
    print(json.dumps(dict(part="generate", floor_ms=out["weight_streaming_floor_ms_per_step"],
                          cases=[(c["prompts"], c["tokens_per_s"], c["decode_step_ms"], c["sampler_us_per_step"], c["lm_head_us_per_step"])
                                 for c in out["cases"]])))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=("sampler", "generate"), help="run one part in this process (what the driver starts)")
    ap.add_argument("--layers", type=int, default=32, help="debug only: anything but 32 is not the Llama-3-8B configuration")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limits", type=int, nargs=2, default=[180, 420], help="time limits of the two parts, seconds")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "divide.json"))
    args = ap.parse_args()
    if args.part == "sampler":
        return part_sampler(args)
    if args.part == "generate":
        return part_generate(args)
    for part, limit in zip(("sampler", "generate"), args.limits):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part, "--layers", str(args.layers),
               "--warmup", str(args.warmup), "--reps", str(args.reps), "--out", args.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"[bench_divide] part {part} ended with status {rc}: nothing more is started", file=sys.stderr)
            sys.exit(rc)
    print(open(args.out).read())


if __name__ == "__main__":
    main()
