#!/usr/bin/env python
"""pretrain_g.lua on the engine: trains G as an auto-encoder - models.create_G_autoencoder: the encoder of models.lua:50-83 in front
of the decoder create_G returns - to reproduce its input images under nn.MSECriterion, and saves the DECODER alone as
<save>/g_pretrained_CxHxW_ndN.net ({G, opt, EPOCH}, pretrain_g.lua:199-214) - the file train.py --G_pretrained_dir picks up instead
of a freshly initialised G (train.lua:20,152-162).

Same flags as pretrain_g.lua:12-29, plus --epochs, --synthetic, --dataDir and the --augment set as in train_v.py.  Each batch
(pretrain_g.lua:131-190) feeds the same images as inputs and targets; fevalG is the auto-encoder forward, the criterion forward and
backward (cg_mse_forward / cg_mse_backward: a deterministic fp64 reduction on the device, read back only for the epoch's print) and
the auto-encoder backward, with the G_L2 / G_L1 penalty, the clamp and optim.adam in the fused update.  The auto-encoder holds
modules the planned executor has no entry for, so it runs module by module (nn.Sequential's walk), the encoder on the gradient the
decoder's first nn.Linear hands back.  Unless --noplot, every epoch writes the originals and their reconstructions (evaluate mode,
100 images) as PNG grids under <save>/g_pretrain_original, g_pretrain_decoded and appends "epoch loss" to
<save>/g_pretrain_loss.txt (visualizeProgress, :219-256, without the display server).

One departure: pretrain_g.lua:142-145 copies TRAIN_DATA[1 .. batchSize] in EVERY batch of an epoch, so the reference trains on the first
16 images of each epoch's draw only; here batch k takes the k-th slice of the pool, which is what its loop over N_epoch says it means.

    python pretrain_g.py --synthetic --N_epoch 1000 --epochs 3
    python train.py --G_pretrained_dir logs ...

Recalled upstream behaviour this script relies on (the Torch7 rocks are not vendored); each row names the test that holds it:

  | behaviour                                                                         | test                                                   |
  |-----------------------------------------------------------------------------------|--------------------------------------------------------|
  | nn.MSECriterion: sizeAverage - loss = sum (x - t)^2 / n, gradInput = 2 (x - t) / n | test_pretrain_host.py::test_mse_np_known_answers,      |
  |   over ALL elements of the batch, fp32 difference                                 |   test_gpu_pretrain.py::test_mse_kernel_vs_numpy       |
  | nn.BatchNormalization on 2-D input: per-column batch statistics, unbiased running  | test_gpu_validator.py::test_batchnorm_1d_training,     |
  |   variance, eval on running statistics                                            |   test_gpu_pretrain.py::test_autoencoder_vs_torch      |
  | nn.SpatialMaxPooling(2, 2): the stride defaults to the kernel size                | test_gpu_pretrain.py::test_autoencoder_vs_torch        |
  | nn.Sequential:backward hands every child its predecessor's output and returns the  | test_gpu_pretrain.py::test_autoencoder_vs_torch        |
  |   first child's gradInput: nested containers chain (encoder <- decoder)           |   (the encoder's output gradient)                      |
  | optim.adam: eps added to sqrt(v) outside the bias correction                      | test_gpu_pretrain.py::test_fevalG_adam_step_vs_torch   |
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    a = ap.add_argument
    a("--save", default="logs"); a("--batchSize", type=int, default=16)
    a("--noplot", action="store_true", help="skip the per-epoch grids of originals / reconstructions and the loss log")
    a("--window", type=int, default=23); a("--seed", type=int, default=1); a("--aws", action="store_true")
    a("--saveFreq", type=int, default=1); a("--gpu", type=int, default=0); a("--threads", type=int, default=8)
    a("--colorSpace", default="rgb", choices=["rgb", "yuv", "hsl", "y"]); a("--scale", type=int, default=32)
    a("--G_clamp", type=float, default=5.0); a("--G_L1", type=float, default=0.0); a("--G_L2", type=float, default=0.0)
    a("--N_epoch", type=int, default=10000); a("--noiseDim", type=int, default=100)
    a("--dataDir", default="dataset/out_aug_64x64"); a("--synthetic", action="store_true")
    a("--epochs", type=int, default=0, help="stop after this many epochs (0 = run forever, as pretrain_g.lua does)")
    a("--augment", action="store_true", help="augment every epoch's images on the fly (dataset.setAugmentation: flip, brightness, noise, "
      "affine warp; on the device with the asynchronous loader) - point --dataDir at the UN-augmented faces, e.g. dataset/out_unaug_64x64")
    a("--augNoFlip", action="store_true", help="--augment without the left-right flips")
    a("--augScale", type=float, nargs=2, default=[0.93, 1.08], metavar=("LO", "HI"), help="--augment: zoom range")
    a("--augRotation", type=int, default=8, help="--augment: rotation of up to this many whole degrees either way")
    a("--augTranslation", type=int, default=4, help="--augment: shift of up to this many pixels on each axis")
    a("--augBrightness", type=float, default=0.15, help="--augment: brightness factor in [1 - this, 1 + this]")
    a("--augNoise", type=float, default=0.02, help="--augment: standard deviation of the noise added to the [0, 1] pixels")
    return ap.parse_args(argv)


def pretrained_filename(save_dir, dims, noiseDim):
    """pretrain_g.lua:203 / train.lua:152: g_pretrained_CHANNELSxHEIGHTxWIDTH_ndNOISEDIM.net."""
    return os.path.join(save_dir, "g_pretrained_%dx%dx%d_nd%d.net" % (tuple(dims) + (noiseDim,)))


class GPretrainer:
    """The state pretrain_g.lua keeps in globals (G_AUTOENCODER, CRITERION, PARAMETERS_G_AUTOENCODER, OPTSTATE, EPOCH; :88-111) and
    its epoch loop."""

    def __init__(self, cg, dims, opt):
        import torch
        self.cg, self.dims, self.opt = cg, tuple(dims), dict(opt)
        self.noiseDim = int(self.opt.get("noiseDim", 100))
        self.G_AUTOENCODER = cg.models.create_G_autoencoder(self.dims, self.noiseDim)
        self.CRITERION = cg.nn.MSECriterion()
        self.PARAMETERS_G_AUTOENCODER, self.GRAD_PARAMETERS_G_AUTOENCODER = self.G_AUTOENCODER.getParameters()
        self.OPTSTATE = {"adam": {}}
        self.EPOCH = 1
        self._torch = torch

    @property
    def encoder(self):
        return self.G_AUTOENCODER.get(1)

    @property
    def decoder(self):
        return self.G_AUTOENCODER.get(2)

    def step(self, inputs):
        """One iteration of :131-190 on a batch [N,C,H,W] (inputs == targets): optim.adam(fevalG, PARAMETERS_G_AUTOENCODER, OPTSTATE.adam)."""
        cg, o, AE = self.cg, self.opt, self.G_AUTOENCODER
        inputs = cg.nn.as_nhwc(cg.nn.to_device(inputs))
        targets = inputs                                                       # :142-145: both the same image(s)

        def fevalG(x):                                                         # :148-181
            if x is not self.PARAMETERS_G_AUTOENCODER:
                self.PARAMETERS_G_AUTOENCODER.copy(x)
            self.GRAD_PARAMETERS_G_AUTOENCODER.zero()
            outputs = AE.forward(inputs)
            # the encoder trains on the gradInput the decoder's first nn.Linear hands back: the module-by-module walk computes it
            assert not AE._planned_last, "the auto-encoder runs on the per-module walk"
            f = self.CRITERION.forward(outputs, targets)
            df_do = self.CRITERION.backward(outputs, targets)
            AE.backward(inputs, df_do)
            self._last = dict(outputs=outputs, f=f, df_do=df_do)
            return f, self.GRAD_PARAMETERS_G_AUTOENCODER                       # penalty + clamp: in the fused update below

        fused = dict(l1=o.get("G_L1", 0.0), l2=o.get("G_L2", 0.0), clamp=o.get("G_clamp", 5.0))
        cg.optim.adam(fevalG, self.PARAMETERS_G_AUTOENCODER, self.OPTSTATE["adam"], fused=fused)
        return self._last

    def epoch(self, trainData, verbose=True):
        """epoch() (:120-216) without the saving, which main() does.  Returns the last batch's loss."""
        N_epoch = min(self.opt["N_epoch"], trainData.size())
        t0 = time.time()
        trained = 0
        while trained < N_epoch:
            N = min(self.opt["batchSize"], N_epoch - trained)
            self.step(trainData.pool.rows(trained + 1, trained + N))
            trained += N
        self._torch.cuda.synchronize()
        dt = time.time() - t0
        loss = float(self.CRITERION.output)
        if verbose:
            print("<trainer> time required for this epoch = %d s" % dt)
            print("<trainer> time to learn 1 sample = %f ms" % (1000 * dt / N_epoch))
            print("<trainer> last batch loss: %.4f" % loss)
        return loss

    def reconstruct(self, images):
        """G_AUTOENCODER:forward in evaluate mode (:221,241,255)."""
        self.G_AUTOENCODER.evaluate()
        try:
            return self.cg.nn.as_plain(self.G_AUTOENCODER.forward(self.cg.nn.as_nhwc(self.cg.nn.to_device(images)))).numpy()
        finally:
            self.G_AUTOENCODER.training()

    def save(self, path):
        """:199-214: {G = the decoder only, opt, EPOCH = EPOCH + 1} in torch.save's format."""
        t7 = importlib.import_module("cat-generator_amd.t7")
        t7_nn = importlib.import_module("cat-generator_amd.t7_nn")
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        opt = {k: v for k, v in self.opt.items() if isinstance(v, (int, float, str, bool))}
        return t7.save(path, {"G": t7_nn.to_t7(self.decoder), "opt": opt, "EPOCH": self.EPOCH + 1})


def visualize(T, images, loss, save_dir):
    """visualizeProgress (:219-256) without the display server: the images before and after the auto-encoder as 10 x 10 PNG grids, and
    (epoch, last batch loss) appended to the loss log."""
    cg = T.cg
    images = cg.nn.to_device(images).numpy()[:100]                             # host, logical [N,C,H,W]
    after = T.reconstruct(images)
    cs = T.opt.get("colorSpace", "rgb")
    for sub, im in (("g_pretrain_original", images), ("g_pretrain_decoded", after)):
        cg.nn_utils.saveImagesAsGrid(os.path.join(save_dir, sub, "%05d.png" % T.EPOCH), cg.nn_utils.toRgb(im, cs), 10, 10, T.EPOCH)
    os.makedirs(save_dir, exist_ok=True)
    with open(os.path.join(save_dir, "g_pretrain_loss.txt"), "a") as f:
        f.write("%d %.6f\n" % (T.EPOCH, loss))


def main(argv=None):
    o = parse(argv)
    import torch
    cg = importlib.import_module("cat-generator_amd")
    torch.cuda.set_device(o.gpu)
    cg.manual_seed(o.seed)                                                     # torch.manualSeed(OPT.seed), :39
    C = 1 if o.colorSpace == "y" else 3
    dims = (C, o.scale, o.scale)                                               # :42-46
    T = GPretrainer(cg, dims, vars(o))
    print("G autoencoder:")
    print(T.G_AUTOENCODER)
    print("Number of free parameters in G (total): %d" % cg.nn_utils.getNumberOfParameters(T.G_AUTOENCODER))
    print("... encoder: %d" % cg.nn_utils.getNumberOfParameters(T.encoder))
    print("... decoder: %d" % cg.nn_utils.getNumberOfParameters(T.decoder))
    ds = importlib.import_module("cat-generator_amd.dataset")
    ds.colorSpace = o.colorSpace; ds.setFileExtension("jpg"); ds.setHeight(o.scale); ds.setWidth(o.scale)
    ds.setDirs([o.dataDir]); ds.seed(o.seed)
    if o.augment:
        ds.setAugmentation(True, hflip=not o.augNoFlip, scale=tuple(o.augScale), rotation=o.augRotation, translation=o.augTranslation,
                           brightness=o.augBrightness, noise_std=o.augNoise)
    while True:                                                                # :113-127
        print("<trainer> Epoch %d" % T.EPOCH)
        if o.synthetic:
            pool = np.random.RandomState(T.EPOCH).rand(o.N_epoch, C, o.scale, o.scale).astype(np.float32)
        else:
            pool = ds.loadRandomImages(o.N_epoch).scaled                       # TRAIN_DATA = DATASET.loadRandomImages(OPT.N_epoch)
        trainData = cg.adversarial.TrainData(pool)
        loss = T.epoch(trainData)
        if T.EPOCH % o.saveFreq == 0:                                          # :199-214
            fn = pretrained_filename(o.save, dims, o.noiseDim)
            print("<trainer> saving network to %s" % fn)
            T.save(fn)
        if not o.noplot:
            images = trainData.pool.rows(1, min(100, trainData.size())) if o.synthetic else ds.loadRandomImages(100).scaled   # :229
            visualize(T, images, loss, o.save)
        T.EPOCH += 1
        if o.epochs and T.EPOCH > o.epochs:
            break
    return T


if __name__ == "__main__":
    main()
