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

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
fe = importlib.import_module("cat-generator_amd.frontend")


def parse(argv=None):
    ap = argparse.ArgumentParser()
    a = ap.add_argument
    fe.run_flags(ap, batchSize=16, noplot_help="skip the per-epoch grids of originals / reconstructions and the loss log", window=23, saveFreq=1)
    a("--G_clamp", type=float, default=5.0); a("--G_L1", type=float, default=0.0); a("--G_L2", type=float, default=0.0)
    a("--N_epoch", type=int, default=10000); a("--noiseDim", type=int, default=100)
    fe.data_flags(ap, "pretrain_g.lua")
    fe.augment_flags(ap)
    return ap.parse_args(argv)


def pretrained_filename(save_dir, dims, noiseDim):
    """pretrain_g.lua:203 / train.lua:152: g_pretrained_CHANNELSxHEIGHTxWIDTH_ndNOISEDIM.net."""
    return fe.net_path("g_pretrained", save_dir, dims, noiseDim)


class GPretrainer(fe.AdamFitter):
    """The state pretrain_g.lua keeps in globals (G_AUTOENCODER, CRITERION, PARAMETERS_G_AUTOENCODER, OPTSTATE, EPOCH; :88-111) and
    its epoch loop."""
    KEY, L2 = "G", 0.0

    def __init__(self, cg, dims, opt):
        self.noiseDim = int(opt.get("noiseDim", 100))
        super().__init__(cg, dims, opt, cg.models.create_G_autoencoder(tuple(dims), self.noiseDim), cg.nn.MSECriterion())
        self.G_AUTOENCODER, self.PARAMETERS_G_AUTOENCODER, self.GRAD_PARAMETERS_G_AUTOENCODER = self.net, self.params, self.grads
        self.saved = self.decoder                        # :199-214: {G = the decoder only, opt, EPOCH = EPOCH + 1} in torch.save's format

    @property
    def encoder(self):
        return self.G_AUTOENCODER.get(1)

    @property
    def decoder(self):
        return self.G_AUTOENCODER.get(2)

    def step(self, inputs):
        """One iteration of :131-190 on a batch [N,C,H,W] (inputs == targets): optim.adam(fevalG, PARAMETERS_G_AUTOENCODER, OPTSTATE.adam);
        fevalG (:148-181) is the shared closure, which here keeps df_do as well."""
        inputs = self.cg.nn.as_nhwc(self.cg.nn.to_device(inputs))
        targets = inputs                                                       # :142-145: both the same image(s)

        def walked():
            # the encoder trains on the gradInput the decoder's first nn.Linear hands back: the module-by-module walk computes it
            assert not self.G_AUTOENCODER._planned_last, "the auto-encoder runs on the per-module walk"

        return self.adam_step(inputs, targets, forwarded=walked, after=lambda outputs, df_do: self._last.update(df_do=df_do))

    def epoch(self, trainData, verbose=True):
        """epoch() (:120-216) without the saving, which run() does.  Returns the last batch's loss."""
        def train(trained, left):
            N = min(self.opt["batchSize"], left)
            self.step(trainData.pool.rows(trained + 1, trained + N))
            return N
        self.run_epoch(min(self.opt["N_epoch"], trainData.size()), train, verbose)
        loss = float(self.CRITERION.output)
        if verbose:
            print("<trainer> last batch loss: %.4f" % loss)
        return loss

    def reconstruct(self, images):
        """G_AUTOENCODER:forward in evaluate mode (:221,241,255)."""
        with self.evaluating() as AE:
            return self.cg.nn.as_plain(AE.forward(self.cg.nn.as_nhwc(self.cg.nn.to_device(images)))).numpy()


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
    dims = fe.img_dimensions(o)                                                # :42-46
    T = GPretrainer(cg, dims, vars(o))
    print("G autoencoder:")
    print(T.G_AUTOENCODER)
    print("Number of free parameters in G (total): %d" % cg.nn_utils.getNumberOfParameters(T.G_AUTOENCODER))
    print("... encoder: %d" % cg.nn_utils.getNumberOfParameters(T.encoder))
    print("... decoder: %d" % cg.nn_utils.getNumberOfParameters(T.decoder))
    ds = fe.configure_dataset(o)

    def plot(trainData, loss):
        images = trainData.pool.rows(1, min(100, trainData.size())) if o.synthetic else ds.loadRandomImages(100).scaled   # :229
        visualize(T, images, loss, o.save)

    return T.run(o, ds, pretrained_filename(o.save, dims, o.noiseDim), plot)   # :113-127


if __name__ == "__main__":
    main()
