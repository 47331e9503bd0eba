"""The harness of the device-event measurement scripts (pretrain_bench.py, nearest_bench.py): timed() for the process that measures, and
run() for the command line of both sides.  The parent never touches the GPU: torch is imported inside timed() only."""
import argparse
import json
import os
import subprocess
import sys


def timed(fn, reps, warmup):
    """us per call of fn over `reps` back-to-back calls after `warmup`, by device events."""
    import torch
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def run(script, tag, child, flags, extra=()):
    """--out, --timeout, the int `flags` {name: default} that child(**flags) takes and the parent-only flags `extra`.  With --child: the
    measurement, its result printed as the line `tag JSON`.  Otherwise that child in ONE process under --timeout: (options, its result)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--timeout", type=int, default=300); ap.add_argument("--child", action="store_true")
    for k, v in flags.items():
        ap.add_argument("--" + k, type=int, default=v)
    for k in extra:
        ap.add_argument(k)
    o = ap.parse_args()
    given = {k: getattr(o, k) for k in flags}
    if o.child:
        print(tag + " " + json.dumps(child(**given)))
        sys.exit(0)
    cmd = [sys.executable, os.path.abspath(script), "--child"] + [x for k, v in given.items() for x in ("--" + k, str(v))]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=o.timeout)
    if r.returncode != 0:
        sys.exit(f"the measuring process failed ({r.returncode}):\n{r.stderr[-3000:]}")
    return o, json.loads([l for l in r.stdout.splitlines() if l.startswith(tag + " ")][-1][len(tag) + 1:])


def write(out, res):
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(res, open(out, "w"), indent=1)
