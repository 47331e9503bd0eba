#!/usr/bin/env python
"""What the resident training set (dataset.ResidentSet / ResidentLoader, pack_dataset.py) costs and saves, on one box.  No thresholds:
every figure is printed with its repetitions' spread (median, min - max) and written to --out.

    python scripts/resident_bench.py --data DIR [--images 8000] [--out FILE.json] [--stages builder,pools,end-to-end]
                                     [--parent TREE] [--rounds 2] [--timeout 600]

--data DIR is filled with --images synthetic 64 x 64 JPEGs (uniform noise, quality 95) when it holds none.  Stages:
  builder     wall time and images/s of dataset.buildPack (what pack_dataset.py runs) at 1, 8 and 16 threads, in this process;
  pools       one child process: a 1000-image pool, 64 x 64 -> 32 x 32 rgb, plain and augmented - ResidentLoader.next() by device events
              around the call (the host work of the call included: the device waits for it), the host time of the call, and its one gather
              kernel alone, back to back; the wall time per pool of AsyncLoader.next() with nothing else to wait for (decode-bound) and of
              loadRandomImages;
  end-to-end  the front-ends' own "time to learn 1 sample" lines and wall times, one process per line: train.py --batchSize 128
              --N_epoch 1000 --epochs 6 --noplot, pretrain_g.py --N_epoch 10000 --epochs 3 --noplot, train_v.py --epochs 3 --noplot,
              sample.py --neighbours (wall) - on this tree without and with a pack in DIR and, with --parent TREE (a built checkout of
              the parent commit), on that tree, in turn, --rounds times;
  stall       (not in the default list) one child process: train.py's loop for 12 epochs with AsyncLoader, then with ResidentLoader, and
              per epoch the time the training thread spends inside loader.next() - the wait the per-sample lines cannot show;
  augment     (not in the default list) the end-to-end stage for train.py ... --augment alone.
The parent process never touches the GPU."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = "RESIDENT_BENCH"
COMMANDS = [("train.py", ["--batchSize", "128", "--N_epoch", "1000", "--epochs", "6", "--noplot"]),
            ("pretrain_g.py", ["--N_epoch", "10000", "--epochs", "3", "--noplot"]),
            ("train_v.py", ["--epochs", "3", "--noplot"]),
            ("sample.py", ["--neighbours", "--batchSize", "64"])]
AUGMENTED = [("train.py", COMMANDS[0][1] + ["--augment"])]


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def fmt(s, unit):
    return "%.3f %s (%.3f - %.3f, %d repetitions)" % (s["median"], unit, s["min"], s["max"], s["n"])


def dataset():
    sys.path.insert(0, ROOT)
    ds = importlib.import_module("cat-generator_amd.dataset")
    ds.setFileExtension("jpg")
    return ds


def make_images(d, n):
    import numpy as np
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    if any(f.endswith(".jpg") for f in os.listdir(d)):
        return
    rs = np.random.RandomState(0)
    for i in range(n):
        Image.fromarray((rs.rand(64, 64, 3) * 255).astype(np.uint8)).save(os.path.join(d, "cat_%05d.jpg" % i), quality=95)


def builder(data):
    ds = dataset()
    rows = []
    for threads in (1, 8, 16):
        t0 = time.perf_counter()
        _, M = ds.buildPack(data, threads)
        dt = time.perf_counter() - t0
        rows.append(dict(threads=threads, images=M, wall_s=dt, images_per_s=M / dt))
        print("buildPack, %2d thread(s): %d images in %.2f s = %.0f images/s" % (threads, M, dt, M / dt))
    return rows


def pools_child(data, reps):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import devbench
    ds = dataset()
    cg = importlib.import_module("cat-generator_amd")
    ds.setDirs([data]); ds.setHeight(32); ds.setWidth(32); ds.colorSpace = "rgb"; ds.seed(1)
    pack = ds.openPack(data)
    assert pack is not None
    t0 = time.perf_counter()
    rset = ds.ResidentSet(pack)
    torch.cuda.synchronize()
    res = dict(device=torch.cuda.get_device_name(0), images=rset.M, set_bytes=rset.nbytes, upload_s=time.perf_counter() - t0, pool=1000, rows=[])
    for aug in (False, True):
        ds.setAugmentation(aug)
        row = dict(augmented=aug)
        ld = ds.ResidentLoader(1000, rset)
        for _ in range(3):
            ld.next()
        ev_ms, host_ms = [], []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            t0 = time.perf_counter()
            ld.next()
            host_ms.append((time.perf_counter() - t0) * 1e3)
            b.record()
            torch.cuda.synchronize()
            ev_ms.append(a.elapsed_time(b))
        row["resident_next_events_ms"], row["resident_next_host_ms"] = spread(ev_ms), spread(host_ms)
        # the one kernel of next() alone, on the buffers the last next() left
        L, s, st, n = ld.L, rset, cg.tensor.stream(), 1000
        out = ld.pools[0].ptr
        if aug:
            draw = ds.augment_draw(n)
            fn = lambda: L.images_u8_gather_augment_to_f32(st, s.ptr, s.M, ld.dev.value, out, n, 64, 64, 32, 32, 0, ld.dev.value + n * 4,
                                                           draw["noise_std"], draw["seed"], 0)
        else:
            fn = lambda: L.images_u8_gather_scale_to_f32(st, s.ptr, s.M, ld.dev.value, out, n, 64, 64, 32, 32, 0)
        row["gather_kernel_us"] = spread([devbench.timed(fn, 20, 5) for _ in range(5)])
        ld.close()
        al = ds.AsyncLoader(1000)
        for _ in range(2):
            al.next()
        wall = []
        for _ in range(max(3, reps // 4)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            al.next()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        al.close()
        row["async_next_wall_ms"] = spread(wall)
        wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            cg.adversarial.TrainData(ds.loadRandomImages(1000).scaled)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        row["blocking_wall_ms"] = spread(wall)
        res["rows"].append(row)
    ds.setAugmentation(False)
    rset.close()
    return res


def stall_child(data, epochs):
    """train.py's own loop at batch 128, --N_epoch 1000 (its set-up through its parse() and the front-end module), with the time the
    training thread spends inside loader.next() taken per epoch: with AsyncLoader that is the wait for the decode worker, which the
    scripts' per-sample lines leave out (they start their clock after the pool is there)."""
    import torch
    sys.path.insert(0, ROOT)
    train = importlib.import_module("train")
    fe = train.fe
    cg = importlib.import_module("cat-generator_amd")
    res = {}
    for name in ("AsyncLoader", "ResidentLoader"):
        o = train.parse(["--batchSize", "128", "--N_epoch", "1000", "--noplot", "--dataDir", data])
        cg.manual_seed(o.seed)
        dims = fe.img_dimensions(o)
        S = cg.adversarial.State(vars(o), cg.models.create_G(dims, o.noiseDim), cg.models.create_D(dims))
        ds = fe.configure_dataset(o)
        loader = ds.AsyncLoader(1000) if name == "AsyncLoader" else fe.resident_loader(o, 1000)
        assert type(loader).__name__ == name
        next_ms, epoch_ms = [], []
        for _ in range(epochs):
            t0 = time.perf_counter()
            pool = loader.next()
            t1 = time.perf_counter()
            cg.adversarial.train(S, cg.adversarial.TrainData(pool), o.D_maxAcc, 20, verbose=False)
            torch.cuda.synchronize()
            next_ms.append((t1 - t0) * 1e3); epoch_ms.append((time.perf_counter() - t1) * 1e3)
        loader.close()
        res[name] = dict(next_ms=next_ms, epoch_ms=epoch_ms)
    return res


def stall(data, timeout):
    dataset().buildPack(data, 8)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-stall", "--data", data], capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.exit(f"the measuring process failed ({r.returncode}):\n{r.stderr[-3000:]}")
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith(TAG + " ")][-1][len(TAG) + 1:])
    for name, x in res.items():
        print("train.py's loop, batch 128, --N_epoch 1000, %s, per epoch [ms]:" % name)
        print("  inside loader.next():  " + " ".join("%7.2f" % v for v in x["next_ms"]))
        print("  the epoch after it:    " + " ".join("%7.2f" % v for v in x["epoch_ms"]))
    return res


def pools(data, reps, timeout):
    ds = dataset()
    ds.buildPack(data, 8)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--data", data, "--reps", str(reps)], capture_output=True, text=True,
                       timeout=timeout)
    if r.returncode != 0:
        sys.exit(f"the measuring process failed ({r.returncode}):\n{r.stderr[-3000:]}")
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith(TAG + " ")][-1][len(TAG) + 1:])
    print("%s: %d images, %.1f MB resident, uploaded in %.2f s" % (res["device"], res["images"], res["set_bytes"] / 1e6, res["upload_s"]))
    for row in res["rows"]:
        print("pool of 1000, 64x64 -> 32x32 rgb, %s:" % ("augmented" if row["augmented"] else "plain"))
        print("  ResidentLoader.next(), device events around the call: " + fmt(row["resident_next_events_ms"], "ms"))
        print("  ResidentLoader.next(), host time of the call:         " + fmt(row["resident_next_host_ms"], "ms"))
        print("  its gather kernel alone, back to back:                " + fmt(row["gather_kernel_us"], "us"))
        print("  AsyncLoader.next(), wall, nothing else to wait for:   " + fmt(row["async_next_wall_ms"], "ms"))
        print("  loadRandomImages + upload, wall:                      " + fmt(row["blocking_wall_ms"], "ms"))
    return res


def end_to_end(data, parent, rounds, timeout, commands=COMMANDS):
    ds = dataset()
    logs = os.path.join(data, "logs")

    def run(tree, script, args, save=os.path.join(data, "scratch_logs")):
        cmd = [sys.executable, os.path.join(tree, script)] + args + ["--dataDir", data]
        cmd += ["--save", logs, "--writeto", os.path.join(data, "samples")] if script == "sample.py" else ["--save", save]
        t0 = time.perf_counter()
        r = subprocess.run(["timeout", "-k", "10", str(timeout)] + cmd, capture_output=True, text=True, cwd=data)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            sys.exit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stderr[-3000:]}")
        ms = [float(l.split("=")[1].split()[0]) for l in r.stdout.splitlines() if "time to learn 1 sample" in l]
        return dict(wall_s=wall, ms_per_sample=ms, resident="<dataset>" in r.stdout)

    if os.path.exists(ds.packPath(data)):
        os.remove(ds.packPath(data))
    run(ROOT, "train.py", ["--batchSize", "128", "--N_epoch", "1000", "--epochs", "1", "--noplot", "--saveFreq", "1"], save=logs)   # sample.py's checkpoint
    configs = ([("parent, files", parent, False)] if parent else []) + [("this commit, files", ROOT, False), ("this commit, pack", ROOT, True)]
    rows = []
    for rnd in range(rounds):
        for name, tree, packed in configs:
            if packed:
                ds.buildPack(data, 8)
            elif os.path.exists(ds.packPath(data)):
                os.remove(ds.packPath(data))
            for script, args in commands:
                x = run(tree, script, args)
                assert x["resident"] == packed, (name, script)
                rows.append(dict(round=rnd, config=name, script=script, args=" ".join(args), **x))
                print("round %d  %-20s %-14s wall %6.2f s   time to learn 1 sample, per epoch [ms]: %s" % (
                    rnd, name, script, x["wall_s"], " ".join("%.4f" % m for m in x["ms_per_sample"]) or "-"))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", required=True); ap.add_argument("--images", type=int, default=8000); ap.add_argument("--out")
    ap.add_argument("--stages", default="builder,pools,end-to-end"); ap.add_argument("--parent"); ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20); ap.add_argument("--timeout", type=int, default=600); ap.add_argument("--child", action="store_true")
    ap.add_argument("--child-stall", action="store_true")
    o = ap.parse_args()
    o.data = os.path.abspath(o.data)
    if o.child:
        print(TAG + " " + json.dumps(pools_child(o.data, o.reps)))
        return
    if o.child_stall:
        print(TAG + " " + json.dumps(stall_child(o.data, 12)))
        return
    make_images(o.data, o.images)
    res = {}
    stages = o.stages.split(",")
    if "builder" in stages:
        res["builder"] = builder(o.data)
    if "pools" in stages:
        res["pools"] = pools(o.data, o.reps, o.timeout)
    if "end-to-end" in stages:
        res["end_to_end"] = end_to_end(o.data, o.parent and os.path.abspath(o.parent), o.rounds, o.timeout)
    if "stall" in stages:
        res["stall"] = stall(o.data, o.timeout)
    if "augment" in stages:
        res["end_to_end_augment"] = end_to_end(o.data, o.parent and os.path.abspath(o.parent), o.rounds, o.timeout, AUGMENTED)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        json.dump(res, open(o.out, "w"), indent=1)


if __name__ == "__main__":
    main()
