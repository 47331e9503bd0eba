#!/usr/bin/env python
"""What augmenting out of padded faces costs (dataset.margin, cg_images_u8_gather_augment_window_to_f32, generate_dataset.py --margin).
No thresholds: every figure is printed with the spread of its blocks or runs.

  kernel   the augmented 1000-image pool by gather, -> 32 x 32 rgb, noise on, out of a resident set of --set images: 64 x 64 sources
           through cg_images_u8_gather_augment_to_f32 (margin 0) against 88 x 88 sources at margin 12 through the window form, and - with
           --parent-lib, the parent commit's libcatgan_hip.so, loaded beside this one - the parent's kernel on the 64 x 64 set.  One
           process, --blocks alternating blocks of --reps back-to-back launches each between device events; per side the median block
           and the fastest and slowest one.  The first pool of the two forms of this commit is compared with the host restatement.
  tool     generate_dataset.py --augmentations 0 end to end on the device path over faces_bench.py's synthetic tree (--images files of
           375 x 500), without --margin and with --margin 12, and - with --parent-tree, a checkout of the parent commit with its
           library built - the parent's library and front end with --margin 12, whose files are then compared with this commit's;
           alternating, --repeats times each.  Then padded_face_np alone over the same files on the tool's threads, and one
           cg_faces_u8_extract_padded call over the front end's first device call, between device events (--reps calls).  Its
           kernels are not separable with events from outside the call; their durations come from a kernel trace, taken in a run of
           its own, of    python scripts/augment_margin_bench.py --worker --do call --images 400 --reps 5

The kernel stage runs in ONE child process, the tool stage in one worker process per tree that the parent feeds commands; all under a
time limit, and the parent never touches the GPU.

    python scripts/augment_margin_bench.py [--stages kernel,tool] [--parent-lib FILE.so] [--parent-tree DIR] [--out FILE.txt] [--timeout 900]"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_stage(o, lines):
    import ctypes
    import importlib
    import numpy as np
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]
    import devbench
    cg = importlib.import_module("cat-generator_amd")
    ds = importlib.import_module("cat-generator_amd.dataset")
    L, st, n, M = cg.lib(), cg.tensor.stream(), 1000, o.set
    rs = np.random.RandomState(0)
    sets = {side: torch.from_numpy(rs.randint(0, 256, size=(M, side, side, 3)).astype(np.uint8)).cuda() for side in (64, 88)}
    ds.seed(1)
    ds.setAugmentation(True)
    idx_h = ds._rs.permutation(M)[:n].astype(np.int32)
    draw = ds.augment_draw(n)
    ds.setAugmentation(False)
    desc_h = {side: ds.augment_descriptors(n, side, side, draw) for side in (64, 88)}
    idx = torch.from_numpy(idx_h).cuda()
    desc = {side: torch.from_numpy(d).cuda() for side, d in desc_h.items()}
    out = cg.Tensor.empty((n, 3, 32, 32), "nhwc")
    sigma, seed = draw["noise_std"], draw["seed"]
    sides = {
        "this commit, 64 x 64, margin 0 (cg_images_u8_gather_augment_to_f32)": lambda: L.images_u8_gather_augment_to_f32(
            st, sets[64].data_ptr(), M, idx.data_ptr(), out.ptr, n, 64, 64, 32, 32, 0, desc[64].data_ptr(), sigma, seed, 0),
        "this commit, 88 x 88, margin 12 (the window form)": lambda: L.images_u8_gather_augment_window_to_f32(
            st, sets[88].data_ptr(), M, idx.data_ptr(), out.ptr, n, 88, 88, 12, 32, 32, 0, desc[88].data_ptr(), sigma, seed, 0),
    }
    # what the two forms compute, against the host restatement (the first 8 images of the pool)
    for name, fn, side, m in zip(sides, sides.values(), (64, 88), (0, 12)):
        fn()
        got = out.numpy()[:8]
        u8 = sets[side].cpu().numpy()[idx_h[:8]]
        w = ds.augment_images(u8, desc_h[side][:8], sigma, seed, 0, margin=m)
        assert np.array_equal(got, np.stack([ds.image_scale(im, 32, 32) for im in w])), name
    lines.append("the first 8 images of both forms' pools equal the host restatement's")
    if o.parent_lib:
        P = ctypes.CDLL(os.path.abspath(o.parent_lib))
        pf = P.cg_images_u8_gather_augment_to_f32
        pf.restype = ctypes.c_int
        pf.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 6 + [
            ctypes.c_void_p, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64]
        first = {}
        sides = dict([("parent commit, 64 x 64 (its cg_images_u8_gather_augment_to_f32)", lambda: pf(
            st, sets[64].data_ptr(), M, idx.data_ptr(), out.ptr, n, 64, 64, 32, 32, 0, desc[64].data_ptr(), sigma, seed, 0))] + list(sides.items()))
        for name in list(sides)[:2]:
            assert sides[name]() in (0, None)
            first[name] = out.numpy().copy()
        a, b = first.values()
        assert np.array_equal(a, b)
        lines.append("the parent's pool and this commit's at margin 0 are equal bit for bit")
    us = {name: [] for name in sides}
    for _ in range(o.blocks):
        for name, fn in sides.items():
            us[name].append(devbench.timed(fn, o.reps, 3))
    lines.append(f"augmented pool of {n} by gather out of {M} resident images -> 32 x 32 rgb, noise on; {o.blocks} alternating blocks of {o.reps} launches, us per launch:")
    for name, v in us.items():
        lines.append(f"  {name:72s} median {statistics.median(v):8.2f}  ({min(v):.2f} - {max(v):.2f})")


def padded_call(o, F, G, files, reply):
    """cg_faces_u8_extract_padded over the front end's first device call at --margin 12 (what fits PADDED_BYTES of sources, crops and
    passes): device events around the whole call - the descriptors' round trip, the head's upload and the four or five kernels."""
    import importlib
    import numpy as np
    import torch
    cg = importlib.import_module("cat-generator_amd")
    M, S, side = 12, 64, 88
    batch, nb = [], 0
    for fp in files:
        _, img, g = G._load(fp)
        pad = F.margin_pad(g["rect"][2], M, S)
        cost = img.nbytes + F.padded_bytes(g["rect"], pad, side)
        if batch and nb + cost > G.PADDED_BYTES:
            break
        batch.append((img, g, pad))
        nb += cost
    imgs, geoms, pads = [b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch]
    d = F.pack_padded_descriptors([im.shape[:2] for im in imgs], geoms, pads, side)
    N, dev = len(imgs), cg.tensor.device()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    src = up(np.concatenate([im.reshape(-1) for im in imgs]))
    arrs = [up(d[k]) for k in ("src_off", "geom", "inv", "taps", "tap_off", "pads")]
    wsb = F.padded_workspace_bytes([g["rect"] for g in geoms], pads, side)
    ws, dst = torch.empty(wsb, dtype=torch.uint8, device=dev), torch.empty((N, side, side, 3), dtype=torch.uint8, device=dev)
    call = lambda: cg.lib().faces_u8_extract_padded(cg.tensor.stream(), src.data_ptr(), src.numel(), arrs[0].data_ptr(), arrs[1].data_ptr(),
                                                    arrs[2].data_ptr(), arrs[3].data_ptr(), d["taps"].size, arrs[4].data_ptr(), arrs[5].data_ptr(),
                                                    dst.data_ptr(), N, side, ws.data_ptr(), wsb)
    ms = []
    for k in range(3 + o.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        if k >= 3:
            ms.append(a.elapsed_time(b))
    want = np.stack([F.padded_face_np(im, g["inv"], g["rect"], M, S) for im, g in zip(imgs[:8], geoms[:8])])
    assert np.array_equal(dst[:8].cpu().numpy(), want), "the timed call's padded faces differ from the host restatement's"
    filled = sum(max(F.crop_pads(im.shape[0], im.shape[1], g["rect"], p)) > 0 for im, g, p in zip(imgs, geoms, pads))
    reply.update(N=N, src_mb=src.numel() / 1e6, ws_mb=wsb / 1e6, pads=[min(pads), max(pads)], filled=int(filled), med=statistics.median(ms),
                 lo=min(ms), hi=max(ms), reps=o.reps)


def worker(o):
    """One process that serves one tree (this one, or --tree: a checkout of another commit with its library built): a JSON command per
    line of stdin - or the one command of --do - answered by a line `@ {...}`."""
    import importlib
    import json
    from concurrent.futures import ThreadPoolExecutor
    import torch
    sys.path.insert(0, os.path.abspath(o.tree or ROOT))
    F = importlib.import_module("cat-generator_amd.faces")
    G = importlib.import_module("generate_dataset")
    files = []
    for line in ([json.dumps(dict(cmd=o.do, path=None))] if o.do else sys.stdin):
        c = json.loads(line)
        reply = {}
        with tempfile.TemporaryDirectory() as own:
            if c["cmd"] == "tree":                                 # the synthetic raw trees; no GPU work
                F.write_raw_tree(os.path.join(c["path"], "raw"), [(375, 500)] * o.images, folders=tuple(f"CAT_{k:02d}" for k in range(7)))
                F.write_raw_tree(os.path.join(c["path"], "small"), [(375, 500)] * 12)
            elif c["cmd"] == "run":                                # generate_dataset.py end to end
                t0 = time.time()
                n, _ = G.main(c["argv"])
                torch.cuda.synchronize()
                reply.update(dt=time.time() - t0, n=n, device=torch.cuda.get_device_name(0))
            else:
                raw = os.path.join(c["path"] or own, "raw")
                files = G.list_raw(raw) if c["path"] else F.write_raw_tree(raw, [(375, 500)] * o.images)
                if c["cmd"] == "padded_np":                        # the host form alone, on the tool's threads
                    loaded = [G._load(fp) for fp in files[:200]]
                    t0 = time.time()
                    with ThreadPoolExecutor(max_workers=o.threads) as ex:
                        list(ex.map(lambda x: F.padded_face_np(x[1], x[2]["inv"], x[2]["rect"], 12, 64), loaded))
                    reply.update(dt=time.time() - t0)
                elif c["cmd"] == "call":
                    padded_call(o, F, G, files, reply)
        print("@ " + json.dumps(reply), flush=True)


class Worker:
    def __init__(self, o, tree):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--images", str(o.images), "--threads", str(o.threads), "--reps", str(o.reps)]
        self.p = subprocess.Popen(cmd + (["--tree", tree] if tree else []), stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(self, **c):
        import json
        self.p.stdin.write(json.dumps(c) + "\n")
        self.p.stdin.flush()
        for line in self.p.stdout:
            if line.startswith("@ "):
                return json.loads(line[2:])
        sys.exit(f"augment_margin_bench: a worker ended (or ran into the time limit) during {c}")

    def close(self):
        self.p.stdin.close()
        self.p.wait()


def tool_stage(o, lines):
    """Runs in the parent process, which never touches the GPU: every measurement is made by a worker process, one per tree, and the
    configurations alternate between them within one run."""
    import filecmp
    import threading
    here, old = Worker(o, None), (Worker(o, os.path.abspath(o.parent_tree)) if o.parent_tree else None)
    workers = [w for w in (here, old) if w]
    limit = threading.Timer(o.timeout, lambda: [w.p.kill() for w in workers])
    limit.start()
    try:
        with tempfile.TemporaryDirectory() as tmp:
            here.ask(cmd="tree", path=tmp)
            argv = lambda tree, out, extra: ["--path", os.path.join(tmp, tree), "--out", os.path.join(tmp, out), "--augmentations", "0",
                                             "--threads", str(o.threads)] + extra
            configs = [("without --margin", here, []), ("--margin 12", here, ["--margin", "12"])]
            if old:
                configs.append(("--margin 12, parent", old, ["--margin", "12"]))
            for k, w in enumerate(workers):                        # code objects, allocator
                dev = w.ask(cmd="run", argv=argv("small", f"warm{k}", ["--margin", "12"]))["device"]
            lines.append(f"device {dev}")
            lines.append(f"generate_dataset.py --augmentations 0 on the device path; {o.images} images of 375 x 500; {o.threads} threads; faces of 64 x 64"
                         + ("; `parent`: the parent commit's library and front end, alternating with this commit's in the same run" if old else ""))
            for r in range(o.repeats):
                for k, (name, w, extra) in enumerate(configs):
                    a = w.ask(cmd="run", argv=argv("raw", f"o{r}_{k}", extra))
                    lines.append(f"  {name:20s} end to end {a['dt']:8.2f} s   {a['n'] / a['dt']:8.0f} faces/s   (run {r})")
            if old:
                for d in ("out_padded_64x64_m12", "out_unaug_64x64"):
                    a, b = os.path.join(tmp, "o0_1", d), os.path.join(tmp, "o0_2", d)
                    names = sorted(os.listdir(a))
                    _, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
                    assert names == sorted(os.listdir(b)) and not mismatch and not errors, f"{d}: this commit's files differ from the parent's"
                lines.append(f"  this commit's out_padded_64x64_m12 and out_unaug_64x64 ({len(names)} faces each) are the parent's byte for byte")
            dt = here.ask(cmd="padded_np", path=tmp)["dt"]
            lines.append(f"  padded_face_np alone, 200 decoded images on {o.threads} threads: {dt:.2f} s   {200 / dt:.0f} faces/s")
            c = here.ask(cmd="call", path=tmp)
            lines.append(f"  cg_faces_u8_extract_padded over the first device call at --margin 12: {c['N']} faces, {c['src_mb']:.0f} MB of sources, pads "
                         f"{c['pads'][0]}..{c['pads'][1]}, {c['filled']} of them median-filled, {c['ws_mb']:.1f} MB workspace")
            lines.append(f"    call (read-back + its kernels)  median {c['med']:8.3f} ms of {c['reps']}  ({c['lo']:.3f} - {c['hi']:.3f})   "
                         f"{c['N'] / c['med'] * 1e3:10.0f} faces/s; its first 8 padded faces equal the host restatement's")
    finally:
        limit.cancel()
        for w in workers:
            w.close()


def child(o):
    import torch
    lines = [f"device {torch.cuda.get_device_name(0)}"]
    kernel_stage(o, lines)
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stages", default="kernel,tool")
    ap.add_argument("--parent-lib", default=None, help="kernel stage: the parent commit's libcatgan_hip.so")
    ap.add_argument("--parent-tree", default=None, help="tool stage: a checkout of the parent commit with its library built")
    ap.add_argument("--set", type=int, default=8000)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=None)
    ap.add_argument("--do", default=None, help="with --worker: one command (call, padded_np) over a tree of its own, e.g. under a kernel trace")
    o = ap.parse_args()
    if o.child:
        return child(o)
    if o.worker:
        return worker(o)
    stages, lines = o.stages.split(","), []
    if "kernel" in stages:
        cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=o.timeout)
        if out.returncode != 0:
            sys.exit(out.stdout[-4000:] + out.stderr[-4000:])
        lines += [ln for ln in out.stdout.splitlines() if not ln.startswith("<dataset>")]
    if "tool" in stages:
        tool_stage(o, lines)
    report = "\n".join(lines)
    print(report)
    if o.out:
        with open(o.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
