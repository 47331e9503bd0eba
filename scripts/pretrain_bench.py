#!/usr/bin/env python
"""cg_mse_forward / cg_mse_backward and the auto-encoder iteration of pretrain_g.py, by device events.

The criterion kernels at n = 16 x 3 x 32 x 32 (the script's default batch) and n = 128 x 3 x 64 x 64, `reps` back-to-back calls after a
warm-up, against a device-to-device copy of ONE operand's bytes in the same process.  Memory traffic per call: the copy 2 n floats
(read + write), the forward 2 n (two reads), the backward 3 n (two reads, one write); each kernel's traffic rate is reported as a share
of the copy's.  Both sizes stay in the caches over the repetitions (0.2 MB and 6.3 MB per operand): the figures are launch and cache
figures, not HBM ones.  Then ms per GPretrainer.step at batch 16 and batch 128 (32 x 32 rgb).  The measurements run in ONE child process
under a time limit; the parent never touches the GPU.

    python scripts/pretrain_bench.py [--out FILE.json] [--timeout 300]"""
import os
import sys

import devbench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [16 * 3 * 32 * 32, 128 * 3 * 64 * 64]
BATCHES = [16, 128]


def child(reps, warmup, iters):
    import importlib
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    cg = importlib.import_module("cat-generator_amd")
    pg = importlib.import_module("pretrain_g")
    L = cg.lib()
    rs = np.random.RandomState(0)
    rows = []

    for n in SIZES:
        x, t = cg.Tensor.from_numpy(rs.rand(n).astype(np.float32)), cg.Tensor.from_numpy(rs.rand(n).astype(np.float32))
        dx, loss = cg.Tensor.empty((n,)), cg.Tensor.zeros((1,))
        s = cg.tensor.stream()
        for what, floats, fn in (("memcpy_d2d", 2, lambda: L.memcpy_d2d(s, dx.ptr, x.ptr, 4 * n)),
                                 ("cg_mse_forward", 2, lambda: L.mse_forward(s, x.ptr, t.ptr, loss.ptr, n)),
                                 ("cg_mse_backward", 3, lambda: L.mse_backward(s, x.ptr, t.ptr, dx.ptr, n))):
            us = devbench.timed(fn, reps, warmup)
            rows.append(dict(what=what, n=n, us=us, traffic_bytes_per_s=4.0 * floats * n / us * 1e6))
        ref_loss, _ = cg.nn_utils.mse_np(x.numpy(), t.numpy())
        assert abs(float(loss.numpy()[0]) - float(ref_loss)) <= np.spacing(ref_loss)
    for N in BATCHES:
        cg.manual_seed(1)
        T = pg.GPretrainer(cg, (3, 32, 32), dict(batchSize=N, N_epoch=N, noiseDim=100))
        batch = cg.nn.as_nhwc(cg.nn.to_device(rs.rand(N, 3, 32, 32).astype(np.float32)))
        us = devbench.timed(lambda: T.step(batch), iters, 5)
        rows.append(dict(what="autoencoder_step", batch=N, ms=us * 1e-3, ms_per_sample=us * 1e-3 / N))
    return dict(device=torch.cuda.get_device_name(0), reps=reps, warmup=warmup, iters=iters, rows=rows)


def derive(res):
    copy = {x["n"]: x for x in res["rows"] if x["what"] == "memcpy_d2d"}
    for x in res["rows"]:
        if "n" in x:
            x["share_of_copy_traffic"] = x["traffic_bytes_per_s"] / copy[x["n"]]["traffic_bytes_per_s"]
    return res


def main():
    o, res = devbench.run(__file__, "PRETRAIN_BENCH", child, dict(reps=200, warmup=10, iters=30))
    for x in derive(res)["rows"]:
        if "n" in x:
            print("%-16s n=%8d %8.2f us  %7.1f GB/s of memory traffic  %5.2f of the copy's traffic rate" % (
                x["what"], x["n"], x["us"], x["traffic_bytes_per_s"] * 1e-9, x["share_of_copy_traffic"]))
        else:
            print("%-16s batch %3d  %8.3f ms per iteration  %7.4f ms per sample" % (x["what"], x["batch"], x["ms"], x["ms_per_sample"]))
    devbench.write(o.out, res)


if __name__ == "__main__":
    main()
