"""Power / clock probe of the GEMMs: socket power + shader clock while our gate_up GEMM / hipBLASLt loop runs.

    python tools/exp_gemm_variants.py power
"""
import json
import os
import subprocess
import sys
import threading
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def sample_smi(stop, rows):
    while not stop.is_set():
        try:
            out = subprocess.run(["rocm-smi", "--showpower", "--showclocks", "--json"], capture_output=True, text=True, timeout=10).stdout
            d = json.loads(out)
            c = d.get("card0", {})
            rows.append({k: v for k, v in c.items() if "ower" in k or "sclk" in k or "mclk" in k or "fclk" in k})
        except Exception as e:       # noqa: BLE001
            rows.append({"error": repr(e)[:100]})
        time.sleep(0.05)


def power():
    import torch
    from rlaif_v_amd import ops
    BF = torch.bfloat16
    R, N, K = 27664, 22016, 4096
    x = torch.randn(R, K, device="cuda").to(BF)
    w = (torch.randn(N, K, device="cuda") * 0.02).to(BF)
    wT = w.t().contiguous()
    out = torch.empty(R, N, device="cuda", dtype=BF)
    p = torch.randn(R, N, device="cuda").to(BF)
    gw = torch.empty(N, K, device="cuda", dtype=BF)
    cases = [("ours nn gate_up", lambda: ops.gemm_nn(x, wT, out=out)), ("hipBLASLt x @ w.T", lambda: torch.matmul(x, w.t(), out=out)),
             ("ours tn wgu", lambda: ops.gemm_tn(p, x, out=gw)), ("idle", None)]
    for name, fn in cases:
        rows, stop = [], threading.Event()
        th = threading.Thread(target=sample_smi, args=(stop, rows))
        t0 = time.time()
        n = 0
        th.start()
        if fn is None:
            time.sleep(3)
        else:
            while time.time() - t0 < 4.0:
                for _ in range(20):
                    fn()
                torch.cuda.synchronize()
                n += 20
        dt = time.time() - t0
        stop.set()
        th.join()
        tf = 2.0 * R * N * K * n / dt / 1e12 if fn else 0.0
        print(f"== {name}: {tf:.0f} TF/s sustained over {dt:.1f} s; samples:")
        for r in rows[1:6]:
            print("   ", json.dumps(r))


if __name__ == "__main__":
    {"power": power}[sys.argv[1]]()
