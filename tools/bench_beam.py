"""Cost of beam-search decoding (LlavaDPOModel.beam_search) at the 7B LLaVA-1.5 shape: 32 layers, a prompt of about 640 spliced
tokens (bos + 34 system tokens + 576 image tokens + a 29-token question), 128 new tokens, one prompt, K = 3 beams - against
``generate(repeat=3)`` at the same prompt and answer lengths, the existing path with the same three decode rows.

    python tools/bench_beam.py [--out profiles/beam_search.json]

The driver starts every GPU part as a child process of its own under ``timeout -k 10`` and stops at the first part that does
not end with status 0 (nothing more is started on a device after a fault, an abort or a time limit).  Parts:

  kernels   rv_attn_decode_indexed with the identity table against rv_attn_decode on the same cache (M = 3 sequences, 32 heads,
            640 prompt + 64 own keys, the model's n_split), and rv_beam_topk + rv_beam_step per step at V = 32000, G = 1,
            K = 3: the two interleaved, median of ``--reps`` timings of 20 back-to-back calls each.
  search    ms per decode step (HIP events around ``_decode_step``, steps 1..127) of beam_search(num_beams=3) and of
            generate(repeat=3, temperature=0), wall time of both, and the ms per step of beam_topk + beam_step inside the search
            (wall time between the decode steps, which includes their launches' host time).

Random weights (init_random); no EOS id, so both run all 128 steps.  No pass bar: nobody has measured this before.  The result
is written to ``--out``."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NEW_TOKENS, SYSTEM, QUESTION, K = 128, 34, 29, 3


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


def _interleaved(fns, reps):
    import torch
    t = {k: [] for k in fns}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for key, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t[key].append(e0.elapsed_time(e1) / 20 * 1e3)
    return {k: round(statistics.median(v), 2) for k, v in t.items()}


def part_kernels(args):
    import torch
    from rlaif_v_amd import ops
    dev = torch.device("cuda", 0)
    H, hd, pre, own, M, V, T = 32, 128, 640, 64, K, 32000, NEW_TOKENS
    g = torch.Generator().manual_seed(0)
    rows = pre + M * T
    kv = torch.randn(rows, 2 * H * hd, generator=g).bfloat16().to(dev)
    q = torch.randn(M, H * hd, generator=g).bfloat16().to(dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)          # noqa: E731
    pre_off, pre_len, own_len = i32([0] * M), i32([pre] * M), i32([own] * M)
    own_off = i32([pre + m * T for m in range(M)])
    table = (own_off[:, None] + torch.arange(T, dtype=torch.int32, device=dev)[None]).contiguous()
    n_split = min(8, max(1, (pre + T) // 256))
    plain = lambda: ops.attn_decode(q, kv, H, hd, 0, H * hd, (pre_off, pre_len, own_off, own_len), n_split=n_split)[0]     # noqa: E731
    indexed = lambda: ops.attn_decode_indexed(q, kv, H, hd, 0, H * hd, (pre_off, pre_len, own_len), table, own, n_split=n_split)[0]     # noqa: E731
    same = bool(torch.equal(plain(), indexed()))
    attn = _interleaved(dict(attn_decode_us=plain, attn_decode_indexed_us=indexed), args.reps)
    logits = (torch.randn(K, V, generator=g) * 3).to(dev)
    state = ops.BeamState(1, K, T, pre, dev)

    def select():
        cand = ops.beam_topk(logits, state.run_score, 1, K, V)[:3]
        state.run_score.copy_(torch.tensor([0.0, -1.0, -2.0], device=dev))
        ops.beam_step(state, cand, T // 2)
    sel = _interleaved(dict(beam_topk_plus_step_us=select, beam_topk_us=lambda: ops.beam_topk(logits, state.run_score, 1, K, V)), args.reps)
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, attention=dict(M=M, H=H, pre_len=pre, own_len=own, n_split=n_split,
               identity_table_same_bits=same, **attn), selection=dict(G=1, K=K, V=V, step=T // 2, **sel,
               note="beam_topk_plus_step includes one 3-element host-to-device copy that resets the scores"))
    _merge(args.out, "kernels", out)
    print(json.dumps(dict(part="kernels", **out)))


def part_search(args):
    import torch
    from oracle import dpo_oracle as O
    from rlaif_v_amd.model import LlavaConfig, LlavaDPOModel
    dev = torch.device("cuda", 0)
    model = LlavaDPOModel(LlavaConfig(**O.asdict(O.LlavaCfg(layers=args.layers))), device=dev, with_optimizer=False)
    model.init_random(seed=0)
    model.eval()
    cfg = model.cfg
    g = torch.Generator().manual_seed(1234)
    prompt = torch.cat([torch.tensor([1]), torch.randint(3, cfg.vocab, (SYSTEM,), generator=g), torch.tensor([-200]),
                        torch.randint(3, cfg.vocab, (QUESTION,), generator=g)])
    pixels = torch.randn(1, 3, cfg.image_size, cfg.image_size, generator=g).to(dev)
    real_step = model._decode_step
    modes = dict(generate_repeat3=lambda: model.generate([prompt], pixels, NEW_TOKENS, repeat=K, temperature=0.0),
                 beam_search_k3=lambda: model.beam_search([prompt], pixels, NEW_TOKENS, num_beams=K))
    out = dict(device=torch.cuda.get_device_name(0), layers=cfg.layers, new_tokens=NEW_TOKENS, num_beams=K,
               prompt_tokens=1 + SYSTEM + cfg.n_image_tokens + QUESTION, weights="random (init_random)", modes={})
    for name, fn in modes.items():
        runs = []
        for rep in range(args.warmup + args.reps):
            events = []

            def timed(*a, **kw):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = real_step(*a, **kw)
                e1.record()
                events.append((e0, e1))
                return r
            model._decode_step = timed
            try:
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                wall = time.perf_counter() - t
            finally:
                model._decode_step = real_step
            step_ms = statistics.median(a.elapsed_time(b) for a, b in events)
            between = statistics.median(events[i][1].elapsed_time(events[i + 1][0]) for i in range(len(events) - 1))
            if rep >= args.warmup:
                runs.append(dict(wall_s=round(wall, 4), decode_step_ms=round(step_ms, 4), between_steps_ms=round(between, 4)))
            print(f"[bench_beam] {name} rep {rep}: wall {wall:.3f} s, decode step {step_ms:.3f} ms, between steps {between:.3f} ms", flush=True)
        out["modes"][name] = dict(runs=runs, decode_step_ms=statistics.median(r["decode_step_ms"] for r in runs),
                                  between_steps_ms=statistics.median(r["between_steps_ms"] for r in runs),
                                  wall_s=statistics.median(r["wall_s"] for r in runs))
    b, s = out["modes"]["beam_search_k3"], out["modes"]["generate_repeat3"]
    out["beam_over_generate_decode_step"] = round(b["decode_step_ms"] / s["decode_step_ms"], 4)
    out["beam_over_generate_wall"] = round(b["wall_s"] / s["wall_s"], 4)
    out["note"] = ("between_steps_ms: device time from the end of one decode step to the start of the next - rv_sample_token for "
                   "generate, rv_beam_topk + rv_beam_step for beam_search, with whatever host time the device waited for")
    _merge(args.out, "search", out)
    print(json.dumps(dict(part="search", beam_step_ms=b["decode_step_ms"], generate_step_ms=s["decode_step_ms"],
                          beam_between_ms=b["between_steps_ms"], generate_between_ms=s["between_steps_ms"])))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=("kernels", "search"), help="run one part in this process (what the driver starts)")
    ap.add_argument("--layers", type=int, default=32, help="debug only: anything but 32 is not the 7B configuration")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limits", type=int, nargs=2, default=[180, 420], help="time limits of the two parts, seconds")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "beam_search.json"))
    args = ap.parse_args()
    if args.part == "kernels":
        return part_kernels(args)
    if args.part == "search":
        return part_search(args)
    for part, limit in zip(("kernels", "search"), args.limits):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part, "--layers", str(args.layers),
               "--warmup", str(args.warmup), "--reps", str(args.reps), "--out", args.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"[bench_beam] part {part} ended with status {rc}: nothing more is started", file=sys.stderr)
            sys.exit(rc)
    print(open(args.out).read())


if __name__ == "__main__":
    main()
