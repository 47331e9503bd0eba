#!/usr/bin/env python
"""--scale 16: what the fused localisation launch of the three branch transformers (csrc/locnet.hip at S 4, Cin 64) buys.  Two copies of
the G16up / D32_st3 pair live in one process - D planned with fuse_locnet 1 (every localisation branch as one launch) and with
fuse_locnet 2 (only the first transformer's: the plan without the S = 4 kernels) - and are timed in alternating blocks, each between two
device synchronisations on the host clock: D's forward + backward alone, and the whole training step.  The spread between the blocks of
one setting is printed beside the difference between the settings, at batch 128 and at the reference's default 32.
python scripts/scale16_probe.py [blocks=6] [D passes per block=1500] [steps per block=400]"""
import importlib, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
cg = importlib.import_module("cat-generator_amd")
BLOCKS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
KD = int(sys.argv[2]) if len(sys.argv) > 2 else 1500
KS = int(sys.argv[3]) if len(sys.argv) > 3 else 400
dims = (3, 16, 16)


def build(NB, fuse):
    cg.manual_seed(1)
    G, D = cg.models.create_G(dims, 100), cg.models.create_D(dims)
    S = cg.adversarial.State(dict(batchSize=NB, seed=1), G, D)
    cg.lib().net_set_option(D._planned_net().h, b"fuse_locnet", fuse)
    rs = np.random.RandomState(100)
    data = cg.adversarial.TrainData(rs.rand(512, *dims).astype(np.float32))
    x = cg.Tensor.from_numpy(rs.rand(NB, *dims).astype(np.float32))
    dy = cg.Tensor.from_numpy(rs.randn(NB, 1).astype(np.float32))
    return dict(S=S, D=D, data=data, x=x, dy=dy, NB=NB)


def d_pass(c, k):
    for _ in range(k):
        c["D"].forward(c["x"])
        c["D"].backward(c["x"], c["dy"])


def steps(c, k):
    for _ in range(k):
        cg.adversarial.iteration(c["S"], c["data"], c["NB"])


def timed(fn, c, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(c, k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / k, time.perf_counter() - t0


for NB in (128, 32):
    cfg = {1: build(NB, 1), 2: build(NB, 2)}
    for c in cfg.values():           # warm up every shape the timed blocks use
        d_pass(c, 20); steps(c, 20)
        st = c["D"]._pnet[1].stats()
        c["ops"] = (st["launches_forward"], st["launches_backward"])
    print(f"batch {NB}: launch ops of D forward / backward  fuse_locnet 1: {cfg[1]['ops']}  fuse_locnet 2: {cfg[2]['ops']}")
    for what, fn, k in (("D forward + backward", d_pass, KD), ("training step", steps, KS)):
        ms = {1: [], 2: []}
        secs = []
        for b in range(BLOCKS):
            for f in ((1, 2) if b % 2 == 0 else (2, 1)):
                t, s = timed(fn, cfg[f], k)
                ms[f].append(t); secs.append(s)
        a, o = np.array(ms[1]), np.array(ms[2])
        spread = max(a.max() - a.min(), o.max() - o.min())
        print(f"batch {NB} {what}: blocks of {k} ({min(secs):.2f}-{max(secs):.2f} s each)")
        print("   fuse_locnet 1 ms :", " ".join(f"{v:.4f}" for v in a), f"| mean {a.mean():.4f}")
        print("   fuse_locnet 2 ms :", " ".join(f"{v:.4f}" for v in o), f"| mean {o.mean():.4f}")
        print(f"   fused - unfused = {a.mean() - o.mean():+.4f} ms ({100 * (a.mean() / o.mean() - 1):+.1f} %), spread between blocks of one setting {spread:.4f} ms"
              f" -> {'faster by more than the spread' if o.mean() - a.mean() > spread else 'NOT faster by more than the spread'}")
