#!/usr/bin/env python
"""generate_dataset.py timed end to end, device path against --host, on a synthetic raw tree (faces.write_raw_tree: --images files of
375 x 500, the 10k-cats' commonest size), and where the time goes:

  decode        Pillow on the front end's threads alone - every path pays it
  host          generate_dataset.py --host --augmentations 0, wall clock
  device        the same without --host, wall clock (the library and a small tree are warmed first; each side runs --repeats times,
                alternating, and every run is listed)
  call          cg_faces_u8_extract over the front end's first batch (what fits 256 MB of decoded sources): device events around the
                whole call - it reads its descriptors back and checks them before it launches, so this is the descriptors' round trip
                plus both kernels; the median of 20 calls after 3 warm-ups, and the fastest and slowest of them
  upload        the host-to-device copy of that batch's sources, the same way: what the device path pays in front of the call

With --variants the end-to-end runs write --augmentations 9 variants per face instead and compare three paths, alternating:
--variantsFrom crop on the device, --variantsFrom crop --host, and --variantsFrom face on the device; the timed calls are then
cg_faces_u8_extract and cg_faces_u8_extract_variants (A = 9, pad 30, noise on) over the front end's first device call of the crop mode
(what fits its byte bounds), checked against the host restatement.

The kernels on their own (faces_warp_hpass_k, faces_vpass_k; faces_crop_k, faces_median_k, faces_variant_hpass_k) are not separable with events from outside the call; their durations
come from a kernel trace of this script's --call-only mode, taken in a run of its own.  The measurements run in ONE child process under
a time limit; the parent never touches the GPU.

    python scripts/faces_bench.py [--images 2000] [--threads 16] [--repeats 2] [--out FILE.txt] [--timeout 900] [--call-only] [--variants]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(o):
    import importlib
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    cg = importlib.import_module("cat-generator_amd")
    F = importlib.import_module("cat-generator_amd.faces")
    ds = importlib.import_module("cat-generator_amd.dataset")
    G = importlib.import_module("generate_dataset")
    lines = [f"device {torch.cuda.get_device_name(0)}; {o.images} images of 375 x 500; {o.threads} threads; faces of 64 x 64"]
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.time()
        files = F.write_raw_tree(os.path.join(tmp, "raw"), [(375, 500)] * o.images, folders=tuple(f"CAT_{k:02d}" for k in range(7)))
        F.write_raw_tree(os.path.join(tmp, "small"), [(375, 500)] * 12)
        lines.append(f"tree written in {time.time() - t0:.1f} s")
        A = 9 if o.variants else 0
        run = lambda name, extra: G.main(["--path", os.path.join(tmp, "raw"), "--out", os.path.join(tmp, name), "--augmentations", str(A),
                                          "--threads", str(o.threads)] + extra)
        paths = (("host", ["--host"]), ("device", []))
        if o.variants:
            lines[0] += "; 9 variants per face"
            paths = (("crop device", ["--variantsFrom", "crop"]), ("crop host", ["--variantsFrom", "crop", "--host"]), ("face device", []))
        if not o.call_only:
            t0 = time.time()
            with ThreadPoolExecutor(max_workers=o.threads) as ex:
                nbytes = sum(im.nbytes for im in ex.map(ds._decode, files))
            dt = time.time() - t0
            lines.append(f"decode alone      {dt:8.2f} s   {o.images / dt:8.0f} images/s   ({nbytes / 1e6:.0f} MB decoded)")
            for k, (name, extra) in enumerate(paths):                        # code objects, allocator
                if "--host" not in extra:
                    G.main(["--path", os.path.join(tmp, "small"), "--out", os.path.join(tmp, f"warm{k}"), "--augmentations", str(A)] + extra)
            for r in range(o.repeats):
                for name, extra in paths:
                    t0 = time.time()
                    n, _ = run(f"{name.replace(' ', '_')}{r}", extra)
                    torch.cuda.synchronize()
                    dt = time.time() - t0
                    lines.append(f"{name:11s} end to end {dt:8.2f} s   {n / dt:8.0f} faces/s   (run {r})")
        # the front end's first batch
        batch, nb, nvb = [], 0, 0
        for fp in files:
            _, img, g = G._load(fp)
            vb = F.variant_bytes(g["rect"], 30, 9, 64) if o.variants else 0
            if nb + img.nbytes > G.BATCH_BYTES or (batch and nvb + img.nbytes + vb > G.VARIANT_BYTES):
                break
            batch.append((img, g))
            nb += img.nbytes
            nvb += img.nbytes + vb
        imgs, geoms = [b[0] for b in batch], [b[1] for b in batch]
        d = F.pack_descriptors([im.shape[:2] for im in imgs], geoms, 64)
        N, dev = len(imgs), cg.tensor.device()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
        host_src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).pin_memory()
        src = host_src.to(dev)
        arrs = [up(d[k]) for k in ("src_off", "geom", "inv", "taps", "tap_off")]
        wsb = F.workspace_bytes(N, 64, d["rows"])
        ws, dst = torch.empty(wsb, dtype=torch.uint8, device=dev), torch.empty((N, 64, 64, 3), dtype=torch.uint8, device=dev)
        call = lambda: cg.lib().faces_u8_extract(cg.tensor.stream(), src.data_ptr(), src.numel(), arrs[0].data_ptr(), arrs[1].data_ptr(),
                                                 arrs[2].data_ptr(), arrs[3].data_ptr(), d["taps"].size, arrs[4].data_ptr(), dst.data_ptr(), N, 64,
                                                 ws.data_ptr(), wsb)

        def events(fn, reps=20, warmup=3):
            ms = []
            for k in range(warmup + reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                if k >= warmup:
                    ms.append(a.elapsed_time(b))
            ms.sort()
            return ms[len(ms) // 2], ms[0], ms[-1]

        sides = sorted({g["rect"][2] for g in geoms})
        lines.append(f"first batch: {N} faces, {nb / 1e6:.0f} MB of sources, rectangle sides {sides[0]}..{sides[-1]}, {d['rows']} rows, "
                     f"{wsb / 1e6:.1f} MB workspace")
        med, lo, hi = events(call)
        lines.append(f"call (read-back + 2 kernels)  median {med:8.3f} ms  ({lo:.3f} - {hi:.3f})   {N / med * 1e3:10.0f} faces/s")
        if not o.call_only:
            med, lo, hi = events(lambda: src.copy_(host_src, non_blocking=True))
            lines.append(f"upload of the sources (pinned) median {med:8.3f} ms  ({lo:.3f} - {hi:.3f})   {nb / med / 1e6:8.1f} GB/s")
        if o.variants:
            ds.seed(42)
            ds.setAugmentation(True)
            desc = np.stack([ds.augment_descriptors(9, g["rect"][2] + 60, g["rect"][3] + 60) for g in geoms])
            ds.setAugmentation(False)
            bases = np.arange(N * 9, dtype=np.uint64).reshape(N, 9) << np.uint64(32)
            scale, seed = F.noise_scale(0.02), 12345
            vwsb = F.variants_workspace_bytes([g["rect"] for g in geoms], 30, 9, 64)
            vws, vdst = torch.empty(vwsb, dtype=torch.uint8, device=dev), torch.empty((N, 9, 64, 64, 3), dtype=torch.uint8, device=dev)
            ddesc, dbases = up(desc), up(bases)
            vcall = lambda: cg.lib().faces_u8_extract_variants(cg.tensor.stream(), src.data_ptr(), src.numel(), arrs[0].data_ptr(), arrs[1].data_ptr(),
                                                               arrs[2].data_ptr(), arrs[3].data_ptr(), d["taps"].size, arrs[4].data_ptr(), 30, 9,
                                                               ddesc.data_ptr(), dbases.data_ptr(), float(scale), seed, vdst.data_ptr(), N, 64,
                                                               vws.data_ptr(), vwsb)
            med, lo, hi = events(vcall)
            lines.append(f"variants call (read-back + its kernels, A = 9, {vwsb / 1e6:.1f} MB workspace)  median {med:8.3f} ms  ({lo:.3f} - {hi:.3f})   "
                         f"{N * 9 / med * 1e3:10.0f} variants/s")
            vwant = np.stack([F.variants_np(im, g["inv"], g["rect"], 30, desc[n], bases[n], scale, seed, 64)
                              for n, (im, g) in enumerate(zip(imgs[:4], geoms[:4]))])
            assert np.array_equal(vdst[:4].cpu().numpy(), vwant), "the timed call's variants differ from the host restatement's"
            lines.append("the timed call's first 36 variants equal the host restatement's")
        want = np.stack([F.resize_np(F.warp_rect_np(im, g["inv"], g["rect"]), 64) for im, g in zip(imgs[:16], geoms[:16])])
        assert np.array_equal(dst[:16].cpu().numpy(), want), "the timed call's faces differ from the host restatement's"
        lines.append("the timed call's first 16 faces equal the host restatement's")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--call-only", action="store_true")
    ap.add_argument("--variants", action="store_true")
    ap.add_argument("--child", action="store_true")
    o = ap.parse_args()
    if o.child:
        return child(o)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--images", str(o.images), "--threads", str(o.threads), "--repeats", str(o.repeats)]
    out = subprocess.run(cmd + (["--call-only"] if o.call_only else []) + (["--variants"] if o.variants else []), capture_output=True, text=True, timeout=o.timeout)
    if out.returncode != 0:
        sys.exit(out.stdout[-4000:] + out.stderr[-4000:])
    report = "\n".join(ln for ln in out.stdout.splitlines() if not ln.startswith("<dataset>"))
    print(report)
    if o.out:
        with open(o.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
