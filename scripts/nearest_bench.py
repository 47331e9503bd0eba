#!/usr/bin/env python
"""cg_nearest_update against the bandwidth a kernel can have: D = 3072 (32 x 32 rgb), pools of 4096 and 65 536 rows, 1 / 16 / 64 queries,
device events around `reps` back-to-back calls after a warm-up, and a device-to-device copy of the same pool in the same process as the
yardstick.  The copy reads the pool and writes it: its memory traffic is 2 bytes per pool byte, and that traffic rate is what a read-only
kernel competes for - the search's pool bytes per second are reported as a share of it.  The 4096-row pool (50 MB, 100 MB with the
copy's destination) stays in the 256 MB Infinity Cache over the repetitions: its rows are cache figures, only the 65 536-row pool
(805 MB) measures HBM.  The measurements run in ONE child process under a time limit; the parent never touches the GPU.

    python scripts/nearest_bench.py [--out FILE.json] [--timeout 300] [--end-to-end DIR]

--end-to-end DIR: a directory of *.jpg images and a checkpoint DIR/logs/adversarial.net (train.py --save DIR/logs); times
sample.py --neighbours against --neighboursHost on it, one child process each, and adds both wall times."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 3072
SHAPES = [(N, Q) for N in (4096, 65536) for Q in (1, 16, 64)]


def child(reps, warmup):
    import importlib
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    cg = importlib.import_module("cat-generator_amd")
    U, L = cg.nn_utils, cg.lib()
    rs = np.random.RandomState(0)
    rows = []

    def timed(fn):
        for _ in range(warmup):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / reps      # us per call

    for N in sorted({n for n, _ in SHAPES}):
        pool = cg.Tensor.from_numpy(rs.rand(N, D).astype(np.float32))
        other = cg.Tensor.empty((N, D))
        nbytes = N * D * 4
        us = timed(lambda: L.memcpy_d2d(cg.tensor.stream(), other.ptr, pool.ptr, nbytes))
        rows.append(dict(what="memcpy_d2d", N=N, D=D, us=us, pool_bytes_per_s=nbytes / us * 1e6))
        for Q in sorted({q for n, q in SHAPES if n == N}):
            s = U.NearestSearch(rs.rand(Q, D).astype(np.float32))
            us = timed(lambda: s.update(pool, 0))
            idx, _ = s.result()
            assert (idx >= 0).all()
            rows.append(dict(what="cg_nearest_update", N=N, D=D, Q=Q, us=us, pool_bytes_per_s=nbytes / us * 1e6,
                             gflops=3.0 * N * D * Q / us * 1e-3))
    print("NEAREST_BENCH " + json.dumps(dict(device=torch.cuda.get_device_name(0), reps=reps, warmup=warmup, rows=rows)))


def derive(res):
    """Memory traffic per second of every row (the copy moves 2 bytes per pool byte, the search 1) and its share of the copy's."""
    copy = {x["N"]: x for x in res["rows"] if x["what"] == "memcpy_d2d"}
    for x in res["rows"]:
        x["traffic_bytes_per_s"] = x["pool_bytes_per_s"] * (2 if x["what"] == "memcpy_d2d" else 1)
        x["share_of_copy_traffic"] = x["traffic_bytes_per_s"] / (2 * copy[x["N"]]["pool_bytes_per_s"])
        x.pop("share_of_copy_rate", None)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--timeout", type=int, default=300); ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5); ap.add_argument("--end-to-end"); ap.add_argument("--child", action="store_true")
    o = ap.parse_args()
    if o.child:
        return child(o.reps, o.warmup)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(o.reps), "--warmup", str(o.warmup)],
                       capture_output=True, text=True, timeout=o.timeout)
    if r.returncode != 0:
        sys.exit(f"the measuring process failed ({r.returncode}):\n{r.stderr[-3000:]}")
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("NEAREST_BENCH ")][-1][len("NEAREST_BENCH "):])
    for x in derive(res)["rows"]:
        print("%-18s N=%6d Q=%2s %9.1f us  %7.1f GB/s of memory traffic  %5.2f of the copy's traffic rate" % (
            x["what"], x["N"], x.get("Q", "-"), x["us"], x["traffic_bytes_per_s"] * 1e-9, x["share_of_copy_traffic"]))
    if o.end_to_end:
        base = [sys.executable, os.path.join(ROOT, "sample.py"), "--save", os.path.join(o.end_to_end, "logs"), "--dataDir", o.end_to_end,
                "--batchSize", "64", "--neighbours"]
        res["end_to_end"] = {}
        for name, extra in (("device", []), ("host", ["--neighboursHost"]), ("no_neighbours", None)):
            cmd = base[:-1] if extra is None else base + extra
            t0 = time.perf_counter()
            e = subprocess.run(cmd + ["--writeto", os.path.join(o.end_to_end, "samples_" + name)], capture_output=True, text=True, timeout=o.timeout)
            if e.returncode != 0:
                sys.exit(f"sample.py ({name}) failed:\n{e.stderr[-3000:]}")
            res["end_to_end"][name + "_wall_s"] = time.perf_counter() - t0
            print(f"sample.py [{name}]: {res['end_to_end'][name + '_wall_s']:.2f} s wall")
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        json.dump(res, open(o.out, "w"), indent=1)


if __name__ == "__main__":
    main()
