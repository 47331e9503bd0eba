#!/usr/bin/env python
"""Build the face set from the raw 10k-cats download (dataset/generate_dataset.py of the reference): every x.jpg of --path's CAT_*
folders that has its x.jpg.cat keypoints becomes the S x S face NNNNNN_000.jpg in <out>/out_unaug_SxS and <out>/out_aug_SxS - eye line
levelled, face rectangle of method 4, Pillow's bilinear resize, Pillow's default JPEG settings; cat-generator_amd/faces.py holds the
semantics.  The pixel work runs on the device (cg_faces_u8_extract); --host runs its numpy restatement instead, which writes the same
bytes and needs neither a GPU nor the library.

Files are taken in sorted order (folder by folder, then by name; the reference's os.listdir order is unspecified).  An image is skipped
with one warning line - and consumes no index - when it has no .cat file, its .cat line has fewer than nine points, both eyes are on one
pixel, or its rectangle is degenerate (no rectangle the reference would accept, or a side under 8 pixels).  Two runs over the same input
write byte-identical files.

out_aug_SxS also gets --augmentations variants NNNNNN_001 ... per face, their draws seeded by --seed, made in one of two ways:
  --variantsFrom face (the default)  the project's own augmentation of the finished face (dataset.augment_descriptors and
      cg_images_u8_augment_to_f32 at equal source and target size, colour space rgb, re-quantised by (u8)(v 255 + 0.5)): warped from
      the S x S face with edge replication, so rotated and shifted borders show smeared edge pixels; refused where S S 12 bytes
      exceed the augmentation kernel's LDS (S of about 117 and up);
  --variantsFrom crop  the reference's way (faces.py, stages a-d; cg_faces_u8_extract_variants): the rectangle is cut out with
      --padding (30) pixels of real image around it, median-filled where that leaves the image, the pixel stage and the warp run at
      full resolution, then the padding comes off and the result is resized - the borders show real fur and background.  Every
      --scale works.  The draws are dataset.augment_draw's, not the reference's `random` stream.
The _000 faces and out_unaug_SxS do not depend on the mode.

--margin M (default 0: nothing new is written) adds a third directory, <out>/out_padded_SxS_mM: NNNNNN_000.jpg of side S + 2 M for
every accepted face - the face with M pixels of real image around it (faces.padded_face_np: the rectangle enlarged by
faces.margin_pad(Hr, M, S) full-resolution pixels, median-filled where that leaves the image, then the same resize) - and margin.json,
{"margin": M, "side": S}.  The trainers' --augment, pointed at it (--dataDir <out>/out_padded_SxS_mM), warps every epoch pool's fresh
variants out of the padded faces, so their borders show real image, and everything un-augmented sees the S x S centre window
(dataset.setDirs reads margin.json).  With the default ranges and S = 64 a margin of 12 is never left.  An M whose padded face does not
fit the augmentation kernel's LDS is refused.  The padded faces are pixel work like the faces and run on the device
(cg_faces_u8_extract_padded, a pad per face; faces.extract_padded_device), in calls bounded by PADDED_BYTES that share the faces'
upload; with --variantsFrom crop the variants' calls have made the faces already and the padded faces take a second upload of the
sources.  A face whose padded side or pad exceeds the entry point's limits (faces.padded_fits_device) is computed by
faces.padded_face_np instead - rare, and the bytes are the same.  With --host the numpy form runs on the decoding threads
(profiles/augment_margin_bench.txt has what either costs).  --augmentations 0 --margin 12 together with --augment is the cheapest
use that has real borders.

    python generate_dataset.py --path /data/10k_cats --augmentations 0 --margin 12 --pack
"""
import argparse
import glob
import importlib
import json
import math
import os
import sys
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BATCH_BYTES = 256 << 20      # decoded source bytes per device call: batches are bounded by bytes, the images differ in size
MAX_THREADS = 16
LOOKAHEAD = 64               # files being decoded, or decoded and waiting for their batch
VARIANT_BYTES = 256 << 20    # sources, crops, horizontal passes and variants per device call with --variantsFrom crop: all but the first grow with --augmentations
PADDED_BYTES = 256 << 20     # sources, padded crops, horizontal passes and padded faces per device call with --margin
MIN_SIDE = 8                 # cg_faces_u8_extract's smallest rectangle side


def parse(argv=None):
    ap = argparse.ArgumentParser(description="Normalise (and augment) the 10k cats dataset.")
    ap.add_argument("--path", required=True, help="the directory that holds the CAT_* folders")
    ap.add_argument("--out", default="dataset", help="where out_unaug_SxS and out_aug_SxS are written")
    ap.add_argument("--scale", type=int, default=64, help="S, the side of the faces")
    ap.add_argument("--augmentations", type=int, default=9, help="variants per face in out_aug_SxS, beside _000")
    ap.add_argument("--threads", type=int, default=8, help="decoding threads (at most 16); the files do not depend on their number")
    ap.add_argument("--seed", type=int, default=42, help="seed of the variants' draws")
    ap.add_argument("--variantsFrom", choices=("face", "crop"), default="face",
                    help="what the variants are warped from: the finished face (edge replication) or the padded full-resolution crop (the reference's way)")
    ap.add_argument("--padding", type=int, default=30, help="pixels kept around the face rectangle for --variantsFrom crop (0..64)")
    ap.add_argument("--margin", type=int, default=0,
                    help="M: also write out_padded_SxS_mM, the faces with M pixels of real image around them, for the trainers' --augment (0 = off)")
    ap.add_argument("--host", action="store_true", help="compute the faces with the numpy restatement: no GPU, no library")
    ap.add_argument("--pack", action="store_true", help="finish with dataset.buildPack on out_aug_SxS, and on the --margin directory (pack_dataset.py)")
    o = ap.parse_args(argv)
    if o.threads < 1 or not 8 <= o.scale <= 128 or not 0 <= o.augmentations <= 999:
        ap.error("--threads must be positive, --scale in 8..128, --augmentations in 0..999")
    if not 0 <= o.padding <= 64:
        ap.error("--padding must be in 0..64")
    if o.margin < 0:
        ap.error("--margin must not be negative")
    return o


def list_raw(path):
    """The .jpg files of path's CAT_* folders: folder by folder, then by name."""
    files = []
    for d in sorted(glob.glob(os.path.join(path, "CAT_*"))):
        if os.path.isdir(d):
            files += sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith(".jpg") and os.path.isfile(os.path.join(d, f)))
    return files


def _load(fp, margin=0, S=64, host=False):
    """One raw file -> (fp, decoded image, geometry) or (fp, None, why it is skipped); with a margin and --host the geometry also carries
    the padded face, g["padded"] (without --host the flush makes it on the device).  Runs on the decoding threads."""
    F = importlib.import_module("cat-generator_amd.faces")
    ds = importlib.import_module("cat-generator_amd.dataset")
    if not os.path.isfile(fp + ".cat"):
        return fp, None, "it has no .cat file"
    img = ds._decode(fp)
    with open(fp + ".cat") as f:
        kp = F.parse_cat(f.read(), img.shape[0], img.shape[1])
    if kp is None:
        return fp, None, "its .cat line has fewer than nine points"
    g = F.face_geometry(kp, img.shape[0], img.shape[1])
    if not isinstance(g, str) and min(g["rect"][2:]) < MIN_SIDE:
        g = "its face rectangle is degenerate"
    if isinstance(g, str):
        return fp, None, g
    if margin and host:
        g["padded"] = F.padded_face_np(img, g["inv"], g["rect"], margin, S)
    return fp, img, g


def _loaded(ex, files, margin=0, S=64, host=False):
    """_load over the files, in their order whatever the threads do, with a bounded look-ahead: decoded sources wait here, never the
    whole set."""
    ahead = deque()
    for fp in files:
        ahead.append(ex.submit(_load, fp, margin, S, host))
        if len(ahead) >= LOOKAHEAD:
            yield ahead.popleft().result()
    while ahead:
        yield ahead.popleft().result()


def _variants(face, index, n, noise_seed, host):
    """The n augmented variants of one finished face, uint8 [n, S, S, 3]; `index` numbers the face among the accepted ones and with it
    the noise counters, so the variants do not depend on how the faces were batched."""
    ds = importlib.import_module("cat-generator_amd.dataset")
    S = face.shape[0]
    draw = ds.augment_draw(n)
    desc = ds.augment_descriptors(n, S, S, draw)
    u8 = np.ascontiguousarray(np.broadcast_to(face, (n, S, S, 3)))
    if host:
        v = ds.augment_images(u8, desc, draw["noise_std"], noise_seed, 0, index0=index * n).transpose(0, 2, 3, 1)
    else:
        import torch
        cg = importlib.import_module("cat-generator_amd")
        src, dsc = torch.from_numpy(u8).to(cg.tensor.device()), torch.from_numpy(desc).to(cg.tensor.device())
        dst = torch.empty((n, S, S, 3), dtype=torch.float32, device=cg.tensor.device())
        cg.lib().images_u8_augment_to_f32(cg.tensor.stream(), src.data_ptr(), dst.data_ptr(), n, S, S, S, S, 0, dsc.data_ptr(),
                                          draw["noise_std"], noise_seed, 3 * index * n * S * S * 3)
        v = dst.cpu().numpy()
    return (v * np.float32(255.0) + np.float32(0.5)).astype(np.int32).astype(np.uint8)


def _runs(cost, limit):
    """The device calls of one flush as runs (lo, hi) over its items' byte costs: a run takes items until the next one would pass
    `limit`, and one at least."""
    lo = 0
    while lo < len(cost):
        hi, nbytes = lo + 1, cost[lo]
        while hi < len(cost) and nbytes + cost[hi] <= limit:
            nbytes += cost[hi]
            hi += 1
        yield lo, hi
        lo = hi


def _crop_variants(batch, index0, A, pad, S, noise_seed, host):
    """--variantsFrom crop for the faces of one flush, (fp, image, geometry) each, the first of them face `index0` of the set:
    (faces [n, S, S, 3] or None on the host, variants [n, A, S, S, 3]).  Every face draws as _variants draws; the counter base of
    variant a of face i is (i A + a) 2^32, so nothing depends on how the faces were batched.  The device calls are bounded by
    VARIANT_BYTES."""
    F = importlib.import_module("cat-generator_amd.faces")
    ds = importlib.import_module("cat-generator_amd.dataset")
    n = len(batch)
    desc, bases = np.empty((n, A, 8), np.float32), np.empty((n, A), np.uint64)
    scale = None
    for i, (_, _, g) in enumerate(batch):
        draw = ds.augment_draw(A)
        desc[i] = ds.augment_descriptors(A, g["rect"][2] + 2 * pad, g["rect"][3] + 2 * pad, draw)
        bases[i] = [((index0 + i) * A + a) << 32 for a in range(A)]
        scale = F.noise_scale(draw["noise_std"])
    if host:
        return None, np.stack([F.variants_np(im, g["inv"], g["rect"], pad, desc[i], bases[i], scale, noise_seed, S)
                               for i, (_, im, g) in enumerate(batch)])
    cost = [im.nbytes + F.variant_bytes(g["rect"], pad, A, S) for _, im, g in batch]
    got = [F.extract_variants_device([b[1] for b in batch[lo:hi]], [b[2] for b in batch[lo:hi]], pad, desc[lo:hi], bases[lo:hi], scale,
                                     noise_seed, S, with_faces=True) for lo, hi in _runs(cost, VARIANT_BYTES)]
    return np.concatenate([f for f, _ in got]), np.concatenate([v for _, v in got])


def _padded_faces(batch, margin, S, with_faces):
    """--margin on the device for the faces of one flush, (fp, image, geometry) each: (faces [n, S, S, 3] or None, the padded faces
    [n, S + 2 margin, S + 2 margin, 3]).  The device calls are bounded by PADDED_BYTES; with_faces makes them return the S x S faces
    over the same upload.  A face that cg_faces_u8_extract_padded would refuse for its size goes through faces.padded_face_np (and,
    with_faces, a call of cg_faces_u8_extract of its own), which writes the same bytes."""
    F = importlib.import_module("cat-generator_amd.faces")
    n, side = len(batch), S + 2 * margin
    padded = np.empty((n, side, side, 3), np.uint8)
    faces = np.empty((n, S, S, 3), np.uint8) if with_faces else None
    dev, cost = [], []
    for i, (_, im, g) in enumerate(batch):
        pad = F.margin_pad(g["rect"][2], margin, S)
        if F.padded_fits_device(g["rect"], pad):
            dev.append(i)
            cost.append(im.nbytes + F.padded_bytes(g["rect"], pad, side) + (3 * S * (g["rect"][2] + S) if with_faces else 0))
            continue
        padded[i] = F.padded_face_np(im, g["inv"], g["rect"], margin, S)
        if with_faces:
            faces[i] = F.extract_faces_device([im], [g], S)[0]
    for lo, hi in _runs(cost, PADDED_BYTES):
        ix = dev[lo:hi]
        got = F.extract_padded_device([batch[i][1] for i in ix], [batch[i][2] for i in ix], margin, S, with_faces=with_faces)
        if with_faces:
            faces[ix], padded[ix] = got
        else:
            padded[ix] = got
    return faces, padded


def main(argv=None):
    o = parse(argv)
    from PIL import Image
    F = importlib.import_module("cat-generator_amd.faces")
    ds = importlib.import_module("cat-generator_amd.dataset")
    S, A = o.scale, o.augmentations
    crop = A > 0 and o.variantsFrom == "crop"
    if A and not crop and S * S * 12 > ds.AUG_LDS_BYTES:
        raise SystemExit(f"generate_dataset: variants of {S} x {S} faces do not fit the augmentation kernel's LDS; use --variantsFrom crop or --augmentations 0")
    if o.margin and (S + 2 * o.margin) ** 2 * 12 > ds.AUG_LDS_BYTES:
        most = (math.isqrt(ds.AUG_LDS_BYTES // 12) - S) // 2
        raise SystemExit(f"generate_dataset: --margin {o.margin}: {S + 2 * o.margin} x {S + 2 * o.margin} padded faces do not fit the augmentation "
                         f"kernel's LDS; " + (f"the largest margin that fits {S} x {S} faces is {most}" if most >= 0 else f"no {S} x {S} face fits at all"))
    files = list_raw(o.path)
    if not files:
        raise SystemExit(f"generate_dataset: no CAT_*/*.jpg under {o.path}")
    unaug, aug = (os.path.join(o.out, f"out_{k}_{S}x{S}") for k in ("unaug", "aug"))
    os.makedirs(unaug, exist_ok=True)
    os.makedirs(aug, exist_ok=True)
    padded = os.path.join(o.out, f"out_padded_{S}x{S}_m{o.margin}") if o.margin else None
    if padded:
        os.makedirs(padded, exist_ok=True)
        with open(os.path.join(padded, ds.MARGIN_NAME), "w") as f:
            json.dump({"margin": o.margin, "side": S}, f)
    ds.seed(o.seed)
    ds.setAugmentation(True)
    noise_seed = int(ds.augment_draw(1)["seed"])
    written = skipped = 0

    def flush(batch):
        nonlocal written
        if not batch:
            return
        imgs, geoms = [b[1] for b in batch], [b[2] for b in batch]
        faces = variants = pfaces = None
        if crop:
            faces, variants = _crop_variants(batch, written, A, o.padding, S, noise_seed, o.host)
        if padded and o.host:
            pfaces = [g["padded"] for g in geoms]
        elif padded:
            f, pfaces = _padded_faces(batch, o.margin, S, with_faces=faces is None)
            faces = f if faces is None else faces
        if faces is None and o.host:
            faces = np.stack([F.resize_np(F.warp_rect_np(im, g["inv"], g["rect"]), S) for im, g in zip(imgs, geoms)])
        elif faces is None:
            faces = F.extract_faces_device(imgs, geoms, S)
        for i, face in enumerate(faces):
            name = "{:0>6}_{:0>3}.jpg".format(written, 0)
            Image.fromarray(face).save(os.path.join(unaug, name))
            Image.fromarray(face).save(os.path.join(aug, name))
            if padded:
                Image.fromarray(pfaces[i]).save(os.path.join(padded, name))
            if A:
                for a, v in enumerate(variants[i] if crop else _variants(face, written, A, noise_seed, o.host)):
                    Image.fromarray(v).save(os.path.join(aug, "{:0>6}_{:0>3}.jpg".format(written, a + 1)))
            written += 1

    batch, nbytes = [], 0
    with ThreadPoolExecutor(max_workers=min(o.threads, MAX_THREADS)) as ex:
        for fp, img, g in _loaded(ex, files, o.margin, S, o.host):
            if img is None:
                print(f"<dataset> warning: {fp} skipped: {g}")
                skipped += 1
                continue
            if batch and nbytes + img.nbytes > BATCH_BYTES:
                flush(batch)
                batch, nbytes = [], 0
            batch.append((fp, img, g))
            nbytes += img.nbytes
        flush(batch)
    ds.setAugmentation(False)
    print(f"<dataset> {written} faces of {S}x{S} ({skipped} images skipped) -> {unaug}, {aug} (+{A} variants each)"
          + (f", {padded} (margin {o.margin})" if padded else ""))
    if o.pack:
        ds.setFileExtension("jpg")
        for d in (aug, padded) if padded else (aug,):
            path, M = ds.buildPack(d, o.threads)
            print(f"<dataset> {M} images -> {path}")
    return written, skipped


if __name__ == "__main__":
    main()
