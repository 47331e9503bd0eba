#!/usr/bin/env python
"""What augmenting out of padded faces costs (dataset.margin, cg_images_u8_gather_augment_window_to_f32, generate_dataset.py --margin).
No thresholds: every figure is printed with the spread of its blocks or runs.

  kernel   the augmented 1000-image pool by gather, -> 32 x 32 rgb, noise on, out of a resident set of --set images: 64 x 64 sources
           through cg_images_u8_gather_augment_to_f32 (margin 0) against 88 x 88 sources at margin 12 through the window form, and - with
           --parent-lib, the parent commit's libcatgan_hip.so, loaded beside this one - the parent's kernel on the 64 x 64 set.  One
           process, --blocks alternating blocks of --reps back-to-back launches each between device events; per side the median block
           and the fastest and slowest one.  The first pool of the two forms of this commit is compared with the host restatement.
  tool     generate_dataset.py --augmentations 0 end to end on the device path over faces_bench.py's synthetic tree (--images files of
           375 x 500), without --margin and with --margin 12, alternating, --repeats times each; padded_face_np alone over the same
           files on the tool's threads.

The measurements run in ONE child process under a time limit; the parent never touches the GPU.

    python scripts/augment_margin_bench.py [--stages kernel,tool] [--parent-lib FILE.so] [--out FILE.txt] [--timeout 900]"""
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


def tool_stage(o, lines):
    import importlib
    from concurrent.futures import ThreadPoolExecutor
    import torch
    sys.path.insert(0, ROOT)
    F = importlib.import_module("cat-generator_amd.faces")
    G = importlib.import_module("generate_dataset")
    with tempfile.TemporaryDirectory() as tmp:
        files = F.write_raw_tree(os.path.join(tmp, "raw"), [(375, 500)] * o.images, folders=tuple(f"CAT_{k:02d}" for k in range(7)))
        F.write_raw_tree(os.path.join(tmp, "small"), [(375, 500)] * 12)
        lines.append(f"generate_dataset.py --augmentations 0 on the device path; {o.images} images of 375 x 500; {o.threads} threads; faces of 64 x 64")
        G.main(["--path", os.path.join(tmp, "small"), "--out", os.path.join(tmp, "warm"), "--augmentations", "0"])      # code objects, allocator
        for r in range(o.repeats):
            for name, extra in (("without --margin", []), ("--margin 12", ["--margin", "12"])):
                t0 = time.time()
                n, _ = G.main(["--path", os.path.join(tmp, "raw"), "--out", os.path.join(tmp, f"o{r}{len(extra)}"), "--augmentations", "0",
                               "--threads", str(o.threads)] + extra)
                torch.cuda.synchronize()
                dt = time.time() - t0
                lines.append(f"  {name:17s} end to end {dt:8.2f} s   {n / dt:8.0f} faces/s   (run {r})")
        loaded = [G._load(fp) for fp in files[:200]]
        t0 = time.time()
        with ThreadPoolExecutor(max_workers=o.threads) as ex:
            list(ex.map(lambda x: F.padded_face_np(x[1], x[2]["inv"], x[2]["rect"], 12, 64), loaded))
        dt = time.time() - t0
        lines.append(f"  padded_face_np alone, 200 decoded images on {o.threads} threads: {dt:.2f} s   {200 / dt:.0f} faces/s")


def child(o):
    import torch
    lines = [f"device {torch.cuda.get_device_name(0)}"]
    for stage in o.stages.split(","):
        {"kernel": kernel_stage, "tool": tool_stage}[stage](o, lines)
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stages", default="kernel,tool")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--set", type=int, default=8000)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--child", action="store_true")
    o = ap.parse_args()
    if o.child:
        return child(o)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=o.timeout)
    if out.returncode != 0:
        sys.exit(out.stdout[-4000:] + out.stderr[-4000:])
    report = "\n".join(ln for ln in out.stdout.splitlines() if not ln.startswith("<dataset>"))
    print(report)
    if o.out:
        with open(o.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
