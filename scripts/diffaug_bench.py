#!/usr/bin/env python
"""What --D_diffaug costs: the two kernels alone and the batch-128 training step, by device events.  No thresholds: every figure is
the median of its blocks with the fastest and the slowest one.

  kernels  cg_diffaug_forward (draw = 1, out of place) and cg_diffaug_backward at 128 x 32 x 32 x 3 (the batch-128 step's call: 1.5 MB
           read, 1.5 MB written, 128 workgroups of 12 KB LDS) and at 64 x 64 x 64 x 3 (3 MB each way, 64 workgroups of 48 KB), policy
           color,translation,cutout and, for the cost of the colour stage's pixel pass and sum, translation,cutout.  One process,
           --blocks alternating blocks of --reps back-to-back calls each.
  step     adversarial.iteration at batch 128, 3 x 32 x 32, synthetic pool: two States in one process, D_diffaug off and
           color,translation,cutout (three more launches per iteration), alternating blocks of --iters iterations.

Each stage is a child process of its own under `timeout -k 10`; the script stops at the first non-zero status and never touches the
GPU itself.

    python scripts/diffaug_bench.py [--stages kernels,step] [--out profiles/diffaug_bench.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLICY = "color,translation,cutout"


def _setup():
    import importlib
    sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]
    import devbench
    return importlib.import_module("cat-generator_amd"), devbench


def _report(us, unit=("us", 1.0)):
    return ["  %-58s median %9.2f %s  (%.2f - %.2f)" % (name, statistics.median(v) * unit[1], unit[0], min(v) * unit[1], max(v) * unit[1])
            for name, v in us.items()]


def kernels_stage(o):
    import numpy as np
    import torch
    cg, devbench = _setup()
    L, st = cg.lib(), cg.tensor.stream()
    lines = [torch.cuda.get_device_name(0)]
    for N, H, W, C in ((128, 32, 32, 3), (64, 64, 64, 3)):
        rs = np.random.RandomState(0)
        x, g = (torch.from_numpy(rs.randn(N, H, W, C).astype(np.float32)).cuda() for _ in range(2))
        y, gx = torch.empty_like(x), torch.empty_like(g)
        desc = torch.zeros(N * 8, dtype=torch.float32, device="cuda")
        sides = {}
        for name, policy in ((POLICY, 7), ("translation,cutout", 6)):
            sides[f"cg_diffaug_forward  {name}"] = lambda p=policy: L.diffaug_forward(st, x.data_ptr(), y.data_ptr(), desc.data_ptr(), N, H, W, C, p, 1, 1, 0, None)
            sides[f"cg_diffaug_backward {name}"] = lambda p=policy: L.diffaug_backward(st, g.data_ptr(), gx.data_ptr(), desc.data_ptr(), N, H, W, C, p)
        us = {name: [] for name in sides}
        for _ in range(o.blocks):
            for name, fn in sides.items():
                us[name].append(devbench.timed(fn, o.reps, 3))
        lines.append(f"{N} x {H} x {W} x {C} ({N * H * W * C * 4 / 1e6:.2f} MB read, as much written); {o.blocks} alternating blocks of {o.reps} calls, "
                     "us per call:")
        lines += _report(us)
    print("\n".join(lines))


def step_stage(o):
    import numpy as np
    cg, devbench = _setup()
    N = 128
    data = cg.adversarial.TrainData(np.random.RandomState(5).rand(1000, 3, 32, 32).astype(np.float32))
    states = {}
    for name, opt in (("D_diffaug off", {}), ("D_diffaug " + POLICY, dict(D_diffaug=POLICY))):
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
    spread = max(max(v) - min(v) for v in us.values())
    print("\n".join([f"adversarial.iteration, batch {N}, 3 x 32 x 32; {o.blocks} alternating blocks of {o.iters} iterations, ms per iteration:"]
                    + _report(us, ("ms", 1e-3))
                    + ["  the flag costs %.1f us per iteration (%+.2f %%); the blocks of one side spread over %.1f us" % (on - off, 100.0 * (on - off) / off, spread)]))


STAGES = {"kernels": kernels_stage, "step": step_stage}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stages", default="kernels,step")
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
