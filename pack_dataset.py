#!/usr/bin/env python
"""Decode a dataset directory once: every *.jpg of --dataDir, in the loaders' sorted order, as 8-bit RGB into <dataDir>/images_u8.cgpack
(dataset.buildPack; the layout is documented at the top of cat-generator_amd/dataset.py).  train.py, train_v.py, pretrain_g.py and
sample.py --neighbours pick a pack up by themselves while it matches the directory (dataset.openPack): the set then stays in device
memory and every epoch pool is a gather out of it, bit-equal to what the file loaders give.  A directory whose files change needs the
pack rebuilt; a stale pack is ignored with a warning, never used.

    python pack_dataset.py --dataDir dataset/out_aug_64x64
"""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataDir", default="dataset/out_aug_64x64")
    ap.add_argument("--threads", type=int, default=8, help="decoding threads (at most 16); the file does not depend on their number")
    o = ap.parse_args(argv)
    if o.threads < 1:
        ap.error("--threads must be positive")
    ds = importlib.import_module("cat-generator_amd.dataset")
    ds.setFileExtension("jpg")
    t0 = time.time()
    path, M = ds.buildPack(o.dataDir, o.threads)
    dt = time.time() - t0
    print("<dataset> %d images -> %s (%d bytes) in %.2f s, %.0f images/s with %d thread(s)"
          % (M, path, os.path.getsize(path), dt, M / max(dt, 1e-9), min(o.threads, ds.PACK_MAX_THREADS)))


if __name__ == "__main__":
    main()
