#!/usr/bin/env python
"""train.lua on the engine: same flags (train.lua:15-49), same set-up order (:115-220: D, G,
criterion, flat parameters, optimiser state) and the same endless epoch loop (:223-248) around adversarial.train.
Per epoch (unless --noplot): the image grids of NN_UTILS.visualizeProgress (PNG files; no display server).  The validator V is
trained by train_v.py; when <V_dir>/v_CxHxW.net exists (train.lua:19,119-123) it is loaded in evaluate mode and every epoch's
visualisation prints V's ratings of the random, best and worst samples (nn_utils.lua:177-179,686-711).  Without the file the run
is what it was before.  The recalled upstream behaviour V relies on is tabulated in train_v.py.  Likewise G: when --network is empty
and <G_pretrained_dir>/g_pretrained_CxHxW_ndN.net exists (train.lua:20,152-158; pretrain_g.py writes it) G starts from that decoder
instead of create_G; without the file nothing changes.

Not in the reference: --G_ema D (0 < D < 1; off without it) keeps a running average of G's weights inside G's optimiser step, with the
warm-up d_n = min(D, (1 + n) / (10 + n)) over the applied updates n; every epoch's visualisation also writes images_ema/ from the
averaged generator and the checkpoints carry it (sample.py --G_ema samples from it).  The flag is parsed but not listed by --help and
absent from the parsed options unless given: the recorded command lines (tests/golden/cli_flags.json) pin both, and a run without it
stores the OPT it always stored.

Not in the reference either: --D_diffaug POLICY (a comma list out of color, translation, cutout; off without it, or with an empty value
or `none`) applies the same random differentiable augmentation T to every image D sees, real and fake, in the D-step and in the G-step,
and takes G's gradient through T (Zhao et al. 2020; cat-generator_amd/diffaug.py): D never sees an un-augmented image and
cannot memorise the set, while G's own samples stay un-augmented.  Three more launches per iteration; the draws come from the engine's
counter stream, so checkpoints resume bit for bit.  `color` needs channels that are colours: with --colorSpace yuv or hsl it is an
argument error (with y, saturation has nothing to do and is skipped).  Parsed like --G_ema: not listed by --help, absent unless given.

    python train.py --batchSize 128 --N_epoch 1000 --epochs 3 --synthetic          # no dataset needed
    python train.py --batchSize 128 --synthetic --epochs 30 --G_ema 0.999
    python train.py --batchSize 128 --synthetic --epochs 30 --D_diffaug color,translation,cutout
    python train.py --dataDir dataset/out_aug_64x64 --colorSpace y --saveFreq 30
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
fe = importlib.import_module("cat-generator_amd.frontend")


def parse(argv=None):
    ap = argparse.ArgumentParser()
    a = ap.add_argument
    a("--save", default="logs"); a("--saveFreq", type=int, default=30); a("--network", default="")
    a("--batchSize", type=int, default=32); a("--N_epoch", type=int, default=1000)
    a("--G_L1", type=float, default=0.0); a("--G_L2", type=float, default=0.0)
    a("--D_L1", type=float, default=0.0); a("--D_L2", type=float, default=1e-4)
    a("--D_iterations", type=int, default=1); a("--G_iterations", type=int, default=1)
    a("--D_maxAcc", type=float, default=1.01); a("--D_clamp", type=float, default=1.0); a("--G_clamp", type=float, default=5.0)
    a("--D_optmethod", default="adam"); a("--G_optmethod", default="adam")
    a("--D_sgd_lr", type=float, default=0.02); a("--G_sgd_lr", type=float, default=0.02)
    a("--D_sgd_momentum", type=float, default=0.0); a("--G_sgd_momentum", type=float, default=0.0)
    a("--gpu", type=int, default=0); a("--noiseDim", type=int, default=100); a("--scale", type=int, default=32)
    a("--seed", type=int, default=1); a("--colorSpace", default="rgb", choices=fe.COLOR_SPACES)
    fe.data_flags(ap, "train.lua")
    fe.augment_flags(ap)
    a("--noplot", action="store_true", help="train.lua:33 - skip the per-epoch image grids (logs/images*/<start>_<epoch>.png)")
    a("--blockingLoader", action="store_true", help="decode + upload each epoch's images on the training thread (dataset.loadRandomImages)")
    a("--V_dir", default="logs", help="train.lua:19 - directory of the validator network v_CxHxW.net that train_v.py writes")
    a("--G_pretrained_dir", default="logs", help="train.lua:20 - directory of the pre-trained generator g_pretrained_CxHxW_ndN.net that "
      "pretrain_g.py writes")
    a("--G_ema", type=float, default=argparse.SUPPRESS, help=argparse.SUPPRESS)     # see the module docstring
    a("--D_diffaug", default=argparse.SUPPRESS, help=argparse.SUPPRESS)             # likewise
    o = ap.parse_args(argv)
    if hasattr(o, "G_ema"):
        if not 0 <= o.G_ema < 1:
            ap.error("--G_ema must be in [0, 1): the decay of the generator's running average (0 = off)")
        if o.G_ema == 0:
            del o.G_ema          # off: the options are those of a run without the flag
    if hasattr(o, "D_diffaug"):
        if o.D_diffaug.strip().lower() in ("", "none"):
            del o.D_diffaug      # off, likewise
        else:
            diffaug = importlib.import_module("cat-generator_amd.diffaug")
            try:
                policy = diffaug.parse_policy(o.D_diffaug)
            except ValueError as e:
                ap.error(f"--D_diffaug: {e}")
            if policy & diffaug.COLOR and o.colorSpace in ("yuv", "hsl"):
                ap.error(f"--D_diffaug color with --colorSpace {o.colorSpace}: a per-pixel channel mean means nothing there (rgb and y are fine)")
    return o


def load_pretrained_G(cg, G_pretrained_dir, dims, noiseDim):
    """train.lua:152-158: G from <G_pretrained_dir>/g_pretrained_CxHxW_ndN.net (the decoder pretrain_g.py saved) when the file exists,
    else None - the caller then builds a fresh one (:160-161), and the run is what it is without the flag."""
    G = fe.load_net(fe.net_path("g_pretrained", G_pretrained_dir, dims, noiseDim), "G")   # the streams stay where D left them
    if G is not None:
        print("<trainer> loading pretrained G...")
        G.training()
    return G


def load_V(cg, S, V_dir, dims):
    """train.lua:119-123: V from <V_dir>/v_CxHxW.net, in evaluate mode, as S.MODEL_V (nn_utils.rateWithV reads it)."""
    fn = fe.net_path("v", V_dir, dims)
    V = fe.load_net(fn, "V")                                       # leaves the training streams where they were
    if V is None:
        print(f"<trainer> no validator network at {fn}: V ratings are off (train_v.py trains one)")
        return None
    V.evaluate()
    S.MODEL_V = V
    print(f"<trainer> loaded validator network {fn}")
    return V


def main(argv=None):
    o = parse(argv)
    import torch
    cg = importlib.import_module("cat-generator_amd")
    torch.cuda.set_device(o.gpu)                                   # cutorch.setDevice(OPT.gpu + 1), train.lua:109
    cg.manual_seed(o.seed)                                         # train.lua:61-62,110
    IMG_DIMENSIONS = fe.img_dimensions(o)                          # train.lua:74-78
    MODEL_D = cg.models.create_D(IMG_DIMENSIONS)                   # train.lua:147
    MODEL_G = None if o.network else load_pretrained_G(cg, o.G_pretrained_dir, IMG_DIMENSIONS, o.noiseDim)   # train.lua:152-158
    if MODEL_G is None:
        MODEL_G = cg.models.create_G(IMG_DIMENSIONS, o.noiseDim)   # train.lua:161
    print(MODEL_G); print(MODEL_D)
    print("Number of free parameters in D: %d" % cg.nn_utils.getNumberOfParameters(MODEL_D))
    print("Number of free parameters in G: %d" % cg.nn_utils.getNumberOfParameters(MODEL_G))
    S = cg.adversarial.State(vars(o), MODEL_G, MODEL_D)            # criterion, getParameters, OPTSTATE: :181-207
    ds = fe.configure_dataset(o)
    if o.network:   # after every generator was seeded: the checkpoint puts each of them back where the run stopped
        print(f"<trainer> reloading previously trained network: {o.network}")
        (cg.checkpoint.load_t7 if o.network.endswith(".net") else cg.checkpoint.load)(o.network, S)
    load_V(cg, S, o.V_dir, IMG_DIMENSIONS)
    n_pool = o.N_epoch if o.N_epoch > 0 else 10000
    import time
    START_TIME = int(time.time())                                  # train.lua:58
    PLOT_DATA = []
    # train.lua:216: the same 100 noise vectors every epoch (a generator of their own: the training streams do not move)
    VIS_NOISE_INPUTS = np.random.RandomState(o.seed).uniform(-1, 1, (100, o.noiseDim)).astype(np.float32)
    # the next epoch's pool loads while this one trains - or, with a fresh pack in --dataDir, is gathered out of the resident set
    loader = None if (o.synthetic or o.blockingLoader) else (fe.resident_loader(o, n_pool) or ds.AsyncLoader(n_pool))
    while True:                                                    # train.lua:223
        print("Loading new training data...")
        if o.synthetic:
            pool = fe.synthetic_pool(S.EPOCH, n_pool, IMG_DIMENSIONS)
        elif loader is not None:
            pool = loader.next()
        else:
            pool = ds.loadRandomImages(n_pool).scaled              # train.lua:225
        TRAIN_DATA = cg.adversarial.TrainData(pool)
        if not o.noplot:                                           # train.lua:228-236
            first = cg.nn.as_nhwc(TRAIN_DATA.pool.rows(1, min(50, TRAIN_DATA.size()))).numpy()
            cg.nn_utils.visualizeProgress(S, VIS_NOISE_INPUTS, first, o.save, START_TIME, PLOT_DATA, verbose=True)
        cg.adversarial.train(S, TRAIN_DATA, o.D_maxAcc, max(20, min(1000 // o.batchSize, 250)))   # train.lua:238
        if (S.EPOCH - 1) % o.saveFreq == 0:                        # train.lua:241-244 (EPOCH was already advanced)
            os.makedirs(o.save, exist_ok=True)
            fn = os.path.join(o.save, "adversarial.npz")
            if os.path.exists(fn):
                os.replace(fn, fn + ".old")
            print(f"<trainer> saving network to {fn}")
            cg.checkpoint.save(fn, S)
            cg.checkpoint.export_t7(os.path.join(o.save, "adversarial.net"), S, PLOT_DATA)   # torch.save's format, train.lua:252-261
        if o.epochs and S.EPOCH > o.epochs:
            break


if __name__ == "__main__":
    main()
