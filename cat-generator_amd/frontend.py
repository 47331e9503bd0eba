"""What the front-end scripts (train.py, train_v.py, pretrain_g.py, sample.py) share: the flag groups more than one of them has, the image
dimensions, the dataset set-up, the synthetic pool, the .net files, and the one class behind train_v.VTrainer and pretrain_g.GPretrainer."""
import contextlib
import os
import time

import numpy as np

from . import dataset as ds, t7, t7_nn
from .tensor import rng

COLOR_SPACES = ["rgb", "yuv", "hsl", "y"]


def run_flags(ap, batchSize, noplot_help, window, saveFreq):
    """The flags train_v.lua:12-28 and pretrain_g.lua:12-29 both start with, in their order."""
    a = ap.add_argument
    a("--save", default="logs"); a("--batchSize", type=int, default=batchSize); a("--noplot", action="store_true", help=noplot_help)
    a("--window", type=int, default=window); a("--seed", type=int, default=1); a("--aws", action="store_true")
    a("--saveFreq", type=int, default=saveFreq); a("--gpu", type=int, default=0); a("--threads", type=int, default=8)
    a("--colorSpace", default="rgb", choices=COLOR_SPACES); a("--scale", type=int, default=32)


def data_flags(ap, lua):
    """Where the images come from and when the run ends (not Lua flags: the reference hard-codes the directory and runs forever)."""
    ap.add_argument("--dataDir", default="dataset/out_aug_64x64"); ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--epochs", type=int, default=0, help=f"stop after this many epochs (0 = run forever, as {lua} does)")


def augment_flags(ap):
    a = ap.add_argument
    a("--augment", action="store_true", help="augment every epoch's images on the fly (dataset.setAugmentation: flip, brightness, noise, "
      "affine warp; on the device with the asynchronous loader) - point --dataDir at the UN-augmented faces, e.g. dataset/out_unaug_64x64")
    a("--augNoFlip", action="store_true", help="--augment without the left-right flips")
    a("--augScale", type=float, nargs=2, default=[0.93, 1.08], metavar=("LO", "HI"), help="--augment: zoom range")
    a("--augRotation", type=int, default=8, help="--augment: rotation of up to this many whole degrees either way")
    a("--augTranslation", type=int, default=4, help="--augment: shift of up to this many pixels on each axis")
    a("--augBrightness", type=float, default=0.15, help="--augment: brightness factor in [1 - this, 1 + this]")
    a("--augNoise", type=float, default=0.02, help="--augment: standard deviation of the noise added to the [0, 1] pixels")


def img_dimensions(o):
    """IMG_DIMENSIONS (train.lua:74-78, train_v.lua:44-48, pretrain_g.lua:42-46): one channel for "y", else three."""
    return (1 if o.colorSpace == "y" else 3, o.scale, o.scale)


def configure_dataset(o):
    """The dataset module set up from the flags (train.lua:85-94, train_v.lua:75-84, pretrain_g.lua:69-78, sample.lua:57-66)."""
    ds.colorSpace = o.colorSpace; ds.setFileExtension("jpg"); ds.setHeight(o.scale); ds.setWidth(o.scale)
    ds.setDirs([o.dataDir]); ds.seed(o.seed)
    if getattr(o, "augment", False):       # sample.py has no such flag
        ds.setAugmentation(True, hflip=not o.augNoFlip, scale=tuple(o.augScale), rotation=o.augRotation, translation=o.augTranslation,
                           brightness=o.augBrightness, noise_std=o.augNoise)
    return ds


def _resident_set(o):
    """The training set of o.dataDir in device memory when the directory holds a pack that still describes it (dataset.openPack warns
    and returns None otherwise) and the device has room; None without a pack file, with --synthetic, or when either refuses."""
    import warnings
    from ._abi import CatganError
    if getattr(o, "synthetic", False) or not os.path.isfile(ds.packPath(o.dataDir)):
        return None
    pack = ds.openPack(o.dataDir)
    if pack is None:
        return None
    try:
        return ds.ResidentSet(pack)
    except CatganError as e:
        warnings.warn(f"{pack.path}: the set does not fit the device ({e}): loading from the files")
        return None


def _resident_line(rset):
    print("<dataset> %d images resident on the device (%s)" % (rset.M, ds.PACK_NAME))


def resident_loader(o, count):
    """The epoch-pool loader over a pack the directory holds, found as train.lua finds g_pretrained_*.net - by the file being there and
    valid, with no flag: a dataset.ResidentLoader, or None when the file loaders have to do what they always did (no fresh pack,
    --synthetic, --blockingLoader, a set the gather kernels cannot serve)."""
    import warnings
    if getattr(o, "blockingLoader", False):
        return None
    rset = _resident_set(o)
    if rset is None:
        return None
    try:
        loader = ds.ResidentLoader(count, rset)
    except ValueError as e:
        warnings.warn(f"{e}: loading from the files")
        rset.close()
        return None
    _resident_line(rset)
    return loader


def resident_chunks(o, chunk):
    """Likewise for one pass over the whole set (sample.py --neighbours): ResidentSet.chunks, or None."""
    import warnings
    rset = _resident_set(o)
    if rset is None:
        return None
    try:
        chunks = rset.chunks(chunk)
    except ValueError as e:
        warnings.warn(f"{e}: loading from the files")
        rset.close()
        return None
    _resident_line(rset)
    return chunks


def synthetic_pool(epoch, n, dims):
    """--synthetic: n uniform-noise images, the same for the same epoch number."""
    return np.random.RandomState(epoch).rand(n, *dims).astype(np.float32)


def net_path(kind, save_dir, dims, noiseDim=None):
    """v_CxHxW.net (kind "v": train_v.lua:204, train.lua:119) or g_pretrained_CxHxW_ndN.net (kind "g_pretrained": pretrain_g.lua:203,
    train.lua:152)."""
    tail = "" if noiseDim is None else "_nd%d" % noiseDim
    return os.path.join(save_dir, "%s_%dx%dx%d%s.net" % ((kind,) + tuple(dims) + (tail,)))


def load_net(path, key):
    """The net saved under `key` of a torch.save file, rebuilt as engine modules, or None without the file.  Rebuilding the modules
    draws initial weights, torch.load does not: the counter stream is left where it was."""
    if not os.path.isfile(path):
        return None
    r, off = rng(), rng().offset
    net = t7_nn.from_t7(t7.load(path)[key])
    r.offset = off
    return net


def save_net(path, nets, opt, epoch):
    """{KEY = net ..., opt, EPOCH = epoch + 1} in torch.save's format (train_v.lua:203-210, pretrain_g.lua:199-214); opt's scalars only."""
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    opt = {k: v for k, v in opt.items() if isinstance(v, (int, float, str, bool))}
    return t7.save(path, {**{k: t7_nn.to_t7(net) for k, net in nets.items()}, "opt": opt, "EPOCH": epoch + 1})


class AdamFitter:
    """The state train_v.lua and pretrain_g.lua keep in globals (a net, CRITERION, flat parameters and gradients, OPTSTATE, EPOCH) and what
    both do with it.  A subclass names them as its Lua source does, has epoch() and sets KEY (the net's name in the saved file and in
    the KEY_L1 / KEY_L2 / KEY_clamp flags) and L2 (that flag's default)."""

    def __init__(self, cg, dims, opt, net, criterion):
        import torch
        self.cg, self.dims, self.opt = cg, tuple(dims), dict(opt)
        self.net, self.saved, self.CRITERION = net, net, criterion             # saved: what save() writes under KEY
        self.params, self.grads = net.getParameters()
        self.OPTSTATE, self.EPOCH = {"adam": {}}, 1
        self._torch = torch

    def adam_step(self, inputs, targets, forwarded=None, after=None):
        """optim.adam(feval, PARAMETERS, OPTSTATE.adam): the feval closure of both scripts, the penalty and the clamp in the fused update.
        forwarded(), when given, runs right after the forward pass; after(outputs, df_do) ends the closure."""
        def feval(x):
            if x is not self.params:
                self.params.copy(x)
            self.grads.zero()
            outputs = self.net.forward(inputs)
            if forwarded is not None:
                forwarded()
            f = self.CRITERION.forward(outputs, targets)
            df_do = self.CRITERION.backward(outputs, targets)
            self.net.backward(inputs, df_do)
            self._last = dict(outputs=outputs, f=f)
            if after is not None:
                after(outputs, df_do)
            return f, self.grads                                               # penalty + clamp: in the fused update below

        o, K = self.opt, self.KEY
        fused = dict(l1=o.get(K + "_L1", 0.0), l2=o.get(K + "_L2", self.L2), clamp=o.get(K + "_clamp", 5.0))
        self.cg.optim.adam(feval, self.params, self.OPTSTATE["adam"], fused=fused)
        return self._last

    def run_epoch(self, N_epoch, train, verbose):
        """train(trained, left) -> the samples it trained on (0 ends the epoch) until N_epoch are done, then both scripts' timing lines."""
        t0, trained = time.time(), 0
        while trained < N_epoch:
            N = train(trained, N_epoch - trained)
            if not N:
                break
            trained += N
        self._torch.cuda.synchronize()
        dt = time.time() - t0
        if verbose:
            print("<trainer> time required for this epoch = %d s" % dt)
            print("<trainer> time to learn 1 sample = %f ms" % (1000 * dt / N_epoch))

    @contextlib.contextmanager
    def evaluating(self):
        self.net.evaluate()
        try:
            yield self.net
        finally:
            self.net.training()

    def save(self, path):
        return save_net(path, {self.KEY: self.saved}, self.opt, self.EPOCH)

    def run(self, o, ds, path, plot):
        """The endless loop of train_v.lua:101-110 / pretrain_g.lua:113-127: per epoch a fresh pool (DATASET.loadRandomImages(OPT.N_epoch)),
        the save to `path` (train_v.lua:203-210, pretrain_g.lua:199-214), plot(trainData, epoch()'s result) unless --noplot; --epochs ends it."""
        loader = resident_loader(o, o.N_epoch)      # a fresh pack in --dataDir: the pools are gathered on the device, the same pools
        while True:
            print("<trainer> Epoch %d" % self.EPOCH)
            if loader is not None:
                pool = loader.next()
            else:
                pool = synthetic_pool(self.EPOCH, o.N_epoch, self.dims) if o.synthetic else ds.loadRandomImages(o.N_epoch).scaled
            trainData = self.cg.adversarial.TrainData(pool)
            result = self.epoch(trainData)
            if self.EPOCH % o.saveFreq == 0:
                print("<trainer> saving network to %s" % path)
                self.save(path)
            if not o.noplot:
                plot(trainData, result)
            self.EPOCH += 1
            if o.epochs and self.EPOCH > o.epochs:
                return self
