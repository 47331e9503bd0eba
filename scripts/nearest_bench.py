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
import os
import subprocess
import sys
import time

import devbench

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

    for N in sorted({n for n, _ in SHAPES}):
        pool = cg.Tensor.from_numpy(rs.rand(N, D).astype(np.float32))
        other = cg.Tensor.empty((N, D))
        nbytes = N * D * 4
        us = devbench.timed(lambda: L.memcpy_d2d(cg.tensor.stream(), other.ptr, pool.ptr, nbytes), reps, warmup)
        rows.append(dict(what="memcpy_d2d", N=N, D=D, us=us, pool_bytes_per_s=nbytes / us * 1e6))
        for Q in sorted({q for n, q in SHAPES if n == N}):
            s = U.NearestSearch(rs.rand(Q, D).astype(np.float32))
            us = devbench.timed(lambda: s.update(pool, 0), reps, warmup)
            idx, _ = s.result()
            assert (idx >= 0).all()
            rows.append(dict(what="cg_nearest_update", N=N, D=D, Q=Q, us=us, pool_bytes_per_s=nbytes / us * 1e6,
                             gflops=3.0 * N * D * Q / us * 1e-3))
    return dict(device=torch.cuda.get_device_name(0), reps=reps, warmup=warmup, rows=rows)


def derive(res):
    """Memory traffic per second of every row (the copy moves 2 bytes per pool byte, the search 1) and its share of the copy's."""
    copy = {x["N"]: x for x in res["rows"] if x["what"] == "memcpy_d2d"}
    for x in res["rows"]:
        x["traffic_bytes_per_s"] = x["pool_bytes_per_s"] * (2 if x["what"] == "memcpy_d2d" else 1)
        x["share_of_copy_traffic"] = x["traffic_bytes_per_s"] / (2 * copy[x["N"]]["pool_bytes_per_s"])
        x.pop("share_of_copy_rate", None)
    return res


def main():
    o, res = devbench.run(__file__, "NEAREST_BENCH", child, dict(reps=50, warmup=5), extra=["--end-to-end"])
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
    devbench.write(o.out, res)


if __name__ == "__main__":
    main()
