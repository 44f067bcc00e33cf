"""Per-launch time of the three per-module-mask adapter kernels (RV_LORA_PEFT_MASKS) at BASELINE config 5's four adapter shapes,
beside their streaming floor (every byte read and written once, over the HBM rate measured for this part) and beside the
composition they replace (rv_dropout + one skinny GEMM / one masked-epilogue GEMM / one split-K GEMM per module).

    python tools/bench_lora_module_masks.py [--rows 29000] [--reps 5] [--csv OUT.csv]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_lora_module_masks.py --reps 5 --new-only
    python tools/bench_lora_module_masks.py --from-trace DIR/.../*_kernel_trace.csv --reps 5 --csv OUT.csv      (no GPU needed)

Event timing brackets `reps` launches; the trace form attributes the kernel durations of a --new-only run to (shape, kernel) by
launch order (the run issues one warm-up plus `reps` launches per entry, in the order of SHAPES x KERNELS)."""
import argparse
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBPS = 6.29          # measured float4-copy rate of the part (8.0 spec)
SHAPES = (("qkv", 4096, 3), ("o", 4096, 1), ("gate|up", 4096, 2), ("down", 11008, 1))      # (projection, adapter input width, modules)
KERNELS = ("F", "B1", "B2")
P, SEEDS = 0.05, (11, 22, 33)


def floor_bytes(kern, M, K, G):
    """Bytes moved if every operand is read once and every result written once (bf16; the fp32 split-K slabs are not counted)."""
    big, thin, adapter = 2 * M * K, 2 * M * 64 * G, 2 * 64 * G * K
    return {"F": big + adapter + thin, "B1": 2 * big + adapter + thin, "B2": big + thin + adapter}[kern]


def from_trace(path, rows, reps, out):
    import collections
    launches = []
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Kernel_Name", "")
            if "lora_masks" in name or "splitk_reduce" in name or "gemm_nt_256_kernel<EpiStore" in name or "gemm_nt_kernel<1, EpiStore" in name:
                launches.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), name))
    launches.sort()
    it = iter(launches)
    table = []
    for proj, K, G in SHAPES:
        for kern in KERNELS:
            per = 2 if kern == "B2" else 1                     # B2 = first pass + the fixed-order reduce
            us = collections.defaultdict(list)
            for rep in range(reps + 1):
                for _ in range(per):
                    _, dur, name = next(it)
                    if rep:
                        us[name.split("(")[0]].append(dur / 1e3)
            tot = sum(sorted(v)[len(v) // 2] for v in us.values())
            fl = floor_bytes(kern, rows, K, G) / (HBM_TBPS * 1e6)
            table.append((proj, kern, rows, K, G, round(tot, 1), round(fl, 1), round(tot / fl, 2), " + ".join(us)))
    write(table, out, "median kernel time from the trace, us")


def write(table, out, what):
    head = ("projection", "kernel", "rows", "width", "modules", what, "streaming floor us", "x floor", "note")
    fh = open(out, "w", newline="") if out else sys.stdout
    w = csv.writer(fh)
    w.writerow(head)
    w.writerows(table)
    if out:
        fh.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=29000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--csv", default=None)
    ap.add_argument("--new-only", action="store_true", help="only the new kernels (the form to run under a kernel trace)")
    ap.add_argument("--from-trace", default=None)
    a = ap.parse_args()
    if a.from_trace:
        return from_trace(a.from_trace, a.rows, a.reps, a.csv)
    import torch
    from rlaif_v_amd import ops
    dev, BF, M = torch.device("cuda:0"), torch.bfloat16, a.rows
    g = torch.Generator(device=dev).manual_seed(1)

    def timed(fn):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.reps

    table = []
    for proj, K, G in SHAPES:
        seeds = SEEDS[:G]
        x = torch.randn(M, K, device=dev, generator=g).to(BF)
        A = (torch.randn(64 * G, K, device=dev, generator=g) * 0.05).to(BF)
        aT = A.t().contiguous()
        dt = torch.randn(M, 64 * G, device=dev, generator=g).to(BF)
        dx = torch.randn(M, K, device=dev, generator=g).to(BF)
        t, dA = torch.empty(M, 64 * G, dtype=BF, device=dev), torch.empty(64 * G, K, dtype=BF, device=dev)

        def old_f():
            for i, s in enumerate(seeds):
                ops.gemm_nt(ops.dropout(x, P, s), A[64 * i:64 * i + 64], out=t[:, 64 * i:64 * i + 64])

        def old_b1():
            for i, s in enumerate(seeds):
                ops.gemm_nt_dropout(dt[:, 64 * i:64 * i + 64], aT[:, 64 * i:64 * i + 64], P, s, out=dx, residual=dx)

        def old_b2():
            for i, s in enumerate(seeds):
                ops.gemm_tn_skinny(dt[:, 64 * i:64 * i + 64], ops.dropout(x, P, s), out=dA[64 * i:64 * i + 64])

        new = {"F": lambda: ops.lora_down_module_masks(x, A, P, seeds, out=t),
               "B1": lambda: ops.lora_dgrad_module_masks(dt, aT, P, seeds, out=dx, residual=dx),
               "B2": lambda: ops.lora_wgrad_module_masks(dt, x, P, seeds, out=dA)}
        old = {"F": old_f, "B1": old_b1, "B2": old_b2}
        for kern in KERNELS:
            us = timed(new[kern])
            fl = floor_bytes(kern, M, K, G) / (HBM_TBPS * 1e6)
            note = "" if a.new_only else f"composition it replaces: {timed(old[kern]):.1f} us"
            table.append((proj, kern, M, K, G, round(us, 1), round(fl, 1), round(us / fl, 2), note))
    write(table, a.csv, "us per call (events)")


if __name__ == "__main__":
    main()
