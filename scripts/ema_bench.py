#!/usr/bin/env python
"""What --G_ema costs: the optimiser kernels at G's size and the batch-128 training step, by device events.  No thresholds: every
figure is the median of its blocks with the fastest and the slowest one.

  kernels  n = 5 191 687 (G32up-c's flat vector), G's own settings (no penalty, clamp 5, gradient written back).  One process, --blocks
           alternating blocks of --reps back-to-back calls each: cg_adam_step, cg_adam_step_ema, cg_adam_step followed by cg_ema_update,
           and - with --parent-lib, the parent commit's libcatgan_hip.so, loaded beside this one - the parent's cg_adam_step, whose
           p, g, m, v after one step are first compared bit for bit with this commit's.  Traffic per call: Adam reads p, g, m, v and
           writes all four (8 n floats); the fused form adds e read and written (10 n); the two launches read p' once more (11 n).
  step     adversarial.iteration at batch 128, 3 x 32 x 32, synthetic pool: two States in one process, G_ema off and 0.999, alternating
           blocks of --iters iterations.

Each stage is a child process of its own under `timeout -k 10`; the script stops at the first non-zero status and never touches the
GPU itself.

    python scripts/ema_bench.py [--stages kernels,step] [--parent-lib FILE.so] [--out profiles/ema_bench.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_G = 5191687


def _setup():
    import importlib
    sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]
    import devbench
    return importlib.import_module("cat-generator_amd"), devbench


def _report(us, unit=("us", 1.0)):
    return ["  %-58s median %9.2f %s  (%.2f - %.2f)" % (name, statistics.median(v) * unit[1], unit[0], min(v) * unit[1], max(v) * unit[1])
            for name, v in us.items()]


def kernels_stage(o):
    import ctypes
    import numpy as np
    import torch
    cg, devbench = _setup()
    L, st, n = cg.lib(), cg.tensor.stream(), N_G
    rs = np.random.RandomState(0)
    host = dict(p=rs.randn(n) * 0.05, g=rs.randn(n) * 0.01, m=rs.randn(n) * 0.001, v=rs.rand(n) * 1e-4, e=rs.randn(n) * 0.05)
    fresh = lambda: {k: torch.from_numpy(a.astype(np.float32)).cuda() for k, a in host.items()}
    hp = (1e-3, 0.9, 0.999, 1e-8)
    tail = (0.0, 0.0, 5.0, 1)
    d = cg.optim.ema_decay(0.999, 10 ** 6)

    def adam(fn, b):
        return fn(st, b["p"].data_ptr(), b["g"].data_ptr(), b["m"].data_ptr(), b["v"].data_ptr(), n, *hp, 1, *tail)

    lines = [torch.cuda.get_device_name(0)]
    B = fresh()
    sides = {
        "cg_adam_step": lambda: adam(L.adam_step, B),
        "cg_adam_step_ema": lambda: L.adam_step_ema(st, B["p"].data_ptr(), B["g"].data_ptr(), B["m"].data_ptr(), B["v"].data_ptr(),
                                                    B["e"].data_ptr(), n, *hp, 1, *tail, d),
        "cg_adam_step, then cg_ema_update": lambda: (adam(L.adam_step, B), L.ema_update(st, B["e"].data_ptr(), B["p"].data_ptr(), n, d)),
    }
    if o.parent_lib:
        P = ctypes.CDLL(os.path.abspath(o.parent_lib))
        pf = P.cg_adam_step
        pf.restype = ctypes.c_int
        pf.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_long] + [ctypes.c_float] * 4 + [ctypes.c_int] + [ctypes.c_float] * 3 + [ctypes.c_int]
        mine, theirs = fresh(), fresh()
        adam(L.adam_step, mine)
        assert adam(pf, theirs) == 0
        for k in "pgmv":
            assert torch.equal(mine[k].view(torch.int32), theirs[k].view(torch.int32)), k
        lines.append("cg_adam_step: p, g, m, v after one step equal the parent library's bit for bit")
        sides = dict([("the parent commit's cg_adam_step", lambda: adam(pf, B))] + list(sides.items()))
    us = {name: [] for name in sides}
    for _ in range(o.blocks):
        for name, fn in sides.items():
            us[name].append(devbench.timed(fn, o.reps, 3))
    lines.append(f"n = {n}; {o.blocks} alternating blocks of {o.reps} calls, us per call:")
    lines += _report(us)
    a, f, two = (statistics.median(us[k]) for k in ("cg_adam_step", "cg_adam_step_ema", "cg_adam_step, then cg_ema_update"))
    lines.append("  the average costs %.2f us inside Adam's pass, %.2f us as a launch of its own" % (f - a, two - a))
    print("\n".join(lines))


def step_stage(o):
    import numpy as np
    import torch
    cg, devbench = _setup()
    N = 128
    data = cg.adversarial.TrainData(np.random.RandomState(5).rand(1000, 3, 32, 32).astype(np.float32))
    states = {}
    for name, opt in (("G_ema off", {}), ("G_ema 0.999", dict(G_ema=0.999))):
        cg.manual_seed(1)
        states[name] = cg.adversarial.State(dict(batchSize=N, **opt), cg.models.create_G((3, 32, 32), 100), cg.models.create_D((3, 32, 32)))
    sides = {name: (lambda S=S: cg.adversarial.iteration(S, data, N)) for name, S in states.items()}
    for fn in sides.values():
        devbench.timed(fn, 3, 3)
    us = {name: [] for name in sides}
    for _ in range(o.blocks):
        for name, fn in sides.items():
            us[name].append(devbench.timed(fn, o.iters, 1))
    off, on = (statistics.median(us[k]) for k in sides)
    print("\n".join([f"adversarial.iteration, batch {N}, 3 x 32 x 32; {o.blocks} alternating blocks of {o.iters} iterations, ms per iteration:"]
                    + _report(us, ("ms", 1e-3)) + ["  the flag costs %.1f us per iteration (%+.2f %%)" % (on - off, 100.0 * (on - off) / off)]))
    assert states["G_ema 0.999"].ema_n() == states["G_ema off"].OPTSTATE["adam"]["G"]["t"]


STAGES = {"kernels": kernels_stage, "step": step_stage}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stages", default="kernels,step")
    ap.add_argument("--parent-lib", default=None, help="kernels stage: the parent commit's libcatgan_hip.so")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per stage")
    ap.add_argument("--child", default=None, choices=list(STAGES))
    o = ap.parse_args()
    if o.child:
        return STAGES[o.child](o)
    lines = []
    for stage in o.stages.split(","):
        cmd = ["timeout", "-k", "10", str(o.timeout), sys.executable, os.path.abspath(__file__), "--child", stage] + sys.argv[1:]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:       # a failed or hung stage ends the run: nothing more is started on the device
            sys.exit(f"stage {stage} ended with status {r.returncode}:\n{r.stdout[-3000:]}{r.stderr[-3000:]}")
        lines += r.stdout.splitlines()
    report = "\n".join(lines)
    print(report)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
