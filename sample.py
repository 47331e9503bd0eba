#!/usr/bin/env python
"""sample.lua on the engine: load G and D from a checkpoint (torch.save format `adversarial.net`, or the
engine's .npz), switch both to evaluate mode, and per run write the grids sample.lua:69-128 writes: 64 training images, 256 and
1024 of 1024 fresh samples, the 64 best / worst (by D) / random ones, optionally the nearest training-set neighbours of the 16
best (--neighbours: searched on the device while the set streams through it; --neighboursHost keeps the reference's host loop).  Same
flags as sample.lua:11-25, plus --neighboursOf / --neighbourChunk, and --G_ema: sample from the averaged generator a `train.py --G_ema D`
run saved (the G_ema field of a .net, PARAMETERS_G_ema of an .npz) instead of the generator of its last mini-batch.  The flag is parsed
but, like train.py's, not listed by --help: the recorded command lines (tests/golden/cli_flags.json) pin the help text and the defaults.

    python sample.py --save logs --writeto samples --runs 1 --dataDir dataset/out_aug_64x64
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
fe = importlib.import_module("cat-generator_amd.frontend")


def parse():
    ap = argparse.ArgumentParser()
    a = ap.add_argument
    a("--save", default="logs"); a("--G_base", default="adversarial.net"); a("--D_base", default="adversarial.net")
    a("--neighbours", action="store_true"); a("--scale", type=int, default=32)
    a("--colorSpace", default="rgb", choices=fe.COLOR_SPACES); a("--writeto", default="samples"); a("--seed", type=int, default=1)
    a("--gpu", type=int, default=0); a("--runs", type=int, default=1); a("--noiseDim", type=int, default=100)
    a("--batchSize", type=int, default=16); a("--dataDir", default="dataset/out_aug_64x64")
    a("--nSamples", type=int, default=1024, help="images sampled per run (sample.lua: 1024)")
    a("--neighboursHost", action="store_true", help="--neighbours (implied) with the reference's host loop over the whole set held in memory")
    a("--neighboursOf", type=int, default=16, help="how many of the best images are searched (1..64; sample.lua: 16)")
    a("--neighbourChunk", type=int, default=4096, help="training images per device pool of the search")
    a("--G_ema", action="store_true", default=argparse.SUPPRESS, help=argparse.SUPPRESS)     # see the module docstring
    o = ap.parse_args()
    if not 1 <= o.neighboursOf <= 64:
        ap.error("--neighboursOf must be in 1..64")
    if o.neighboursHost:
        o.neighbours = True      # the host path of the same check: implies it
    if o.neighbourChunk < 1:
        ap.error("--neighbourChunk must be positive")
    return o


NO_G_EMA = "%s holds no averaged generator: --G_ema needs a checkpoint of a `train.py --G_ema D` run"


def load_models(cg, o, dims):
    """sample.lua:213-227: G from --G_base, D from --D_base, both in evaluate mode.  With --G_ema, G is the averaged generator of the file
    (its weights the running average, its batch-norm statistics the live G's at the time of the save); ValueError(NO_G_EMA) without one."""
    nets = {}
    ema = bool(getattr(o, "G_ema", False))
    for key, name in (("G", o.G_base), ("D", o.D_base)):
        path = os.path.join(o.save, name)
        if path.endswith(".npz"):
            G, D = cg.models.create_G(dims, o.noiseDim), cg.models.create_D(dims)
            S = cg.adversarial.State(dict(batchSize=o.batchSize, noiseDim=o.noiseDim), G, D)
            cg.checkpoint.load(path, S)
            if key == "G" and ema:
                z = np.load(path, allow_pickle=False)
                if "PARAMETERS_G_ema" not in z.files:
                    raise ValueError(NO_G_EMA % path)
                S.PARAMETERS_G.copy(z["PARAMETERS_G_ema"])
            nets[key] = {"G": G, "D": D}[key]
        elif key == "G" and ema:
            nets[key] = cg.checkpoint.import_t7(path).get("G_ema")
            if nets[key] is None:
                raise ValueError(NO_G_EMA % path)
        else:
            nets[key] = cg.checkpoint.import_t7(path)[key]
        nets[key].evaluate()
    return nets["G"], nets["D"]


def main():
    o = parse()
    import torch
    from PIL import Image
    cg = importlib.import_module("cat-generator_amd")
    U = cg.nn_utils
    torch.cuda.set_device(o.gpu)
    cg.manual_seed(o.seed)
    rs = np.random.RandomState(o.seed)                       # torch.manualSeed: the generator behind torch.randperm
    dims = fe.img_dimensions(o)
    ds = fe.configure_dataset(o)                             # sample.py has no --augment: the augmentation stays off
    try:
        G, D = load_models(cg, o, dims)
    except ValueError as e:
        sys.exit(str(e))
    S = cg.adversarial.State(dict(batchSize=o.batchSize, noiseDim=o.noiseDim, colorSpace=o.colorSpace), G, D)
    G.evaluate(); D.evaluate()
    os.makedirs(o.writeto, exist_ok=True)

    def save(name, images, nrow):
        grid = U.toDisplayTensor(U.toRgb(images, o.colorSpace), nrow)
        px = np.clip(np.rint(grid * 255.0), 0, 255).astype(np.uint8).transpose(1, 2, 0)
        Image.fromarray(px).save(os.path.join(o.writeto, name))

    print("Sampling...")
    for run in range(1, o.runs + 1):
        save("trainset_s1_%04d_base.jpg" % run, ds.loadRandomImages(64).scaled, 8)
        images = cg.nn.as_nhwc(U.createImages(S, o.nSamples)).numpy()
        if images.shape[1:] != dims:
            print("[WARNING] dimension mismatch between images generated by base G and command line parameters")
        save("random256_%04d_base.jpg" % run, U.selectRandomImagesFrom(images, 256, rs), 16)
        save("random1024_%04d_base.jpg" % run, images, 32)
        best, _ = U.sortImagesByPrediction(S, images, False, 64)
        worst, _ = U.sortImagesByPrediction(S, images, True, 64)
        save("best_%04d_base.jpg" % run, best, 8)
        save("worst_%04d_base.jpg" % run, worst, 8)
        save("random_%04d_base.jpg" % run, U.selectRandomImagesFrom(images, 64, rs), 8)
        if o.neighbours:
            if o.neighboursHost:
                pairs = U.findClosestNeighboursOf(best[:o.neighboursOf], ds.loadRandomImages(10 ** 9).scaled)
            else:      # the same single draw and file order as loadRandomImages(10 ** 9); the set streams through the device
                files = ds.pickFiles(10 ** 9)
                # with a fresh pack in --dataDir nothing is decoded: the search walks the resident set (in its sorted order)
                loader = fe.resident_chunks(o, o.neighbourChunk) or ds.SequentialLoader(files, o.neighbourChunk)
                try:
                    pairs, _ = U.findClosestNeighboursOnDevice(best[:o.neighboursOf], loader)
                finally:
                    loader.close()
            inter = np.stack([x for img, nb, _ in pairs for x in (img, nb)])
            save("best_%04d_neighbours_base.jpg" % run, inter, len(pairs))
        print("run %d / %d" % (run, o.runs))
    print("Finished.")


if __name__ == "__main__":
    main()
