"""What several test modules share (a plain module, imported as tests/plan_trace.py is): the two measures of the parity tests, the
`options` context that forces dispatch tunables, `counter` that reads a launch counter, the per-tensor gradient rule, the JPEG directory
of the loader tests, and the torch fp64 twin of an engine nn.Sequential."""
import ctypes
import os

import numpy as np
import torch
import torch.nn.functional as F


def close(a, b, K=1024, tol=2e-5, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    s = max(1.0, np.sqrt(K / 1024.0)) * max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert np.isfinite(a).all(), f"{what}: non-finite values"
    assert err <= tol * s, f"{what}: max|d|={err:.3e} > {tol * s:.3e} (K={K})"
    return err


class options:
    """with options(cg, CG_NN_TILE=128064, ...): force dispatch tunables through the C ABI, restore afterwards."""

    def __init__(self, cg, **kv):
        self.cg, self.kv = cg, kv

    def __enter__(self):
        for k, v in self.kv.items():
            self.cg.lib().set_option(k.encode(), int(v))

    def __exit__(self, *exc):
        for k in self.kv:
            self.cg.lib().set_option(k.encode(), -1)


def counter(cg, name):
    """A launch counter kept among the options (CG_WINO3_LAUNCHES, CG_WINO_DGRAD_FUSE_LAUNCHES): how a test tells which kernel ran."""
    v = ctypes.c_long(-1)
    assert cg.lib().get_option(name.encode(), ctypes.byref(v)) == 0
    return v.value


def bulk_close(a, b, max_rel=3e-2, mean_rel=2e-3, what=""):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    scale = max(float(np.abs(b).max()), 1e-12)
    d = np.abs(a - b)
    assert d.max() <= max_rel * scale, f"{what}: max|d|={d.max():.3e} vs scale {scale:.3e}"
    if a.size > 1:
        assert d.mean() <= mean_rel * scale, f"{what}: mean|d|={d.mean():.3e} vs scale {scale:.3e}"


def check_grads(g, params):
    """The flat gradient g against the twin's leaves: bulk_close over all of it, then every tensor on its own.  Returns the twin's."""
    gref = torch.cat([p.grad.reshape(-1) for p in params]).numpy()
    bulk_close(g, gref, what="gradParameters")
    off = 0
    for p in params:     # per tensor, with a floor: a convolution bias in front of a batch norm has an exactly-zero gradient
        k = p.numel()
        a, b = g[off:off + k].astype(np.float64), p.grad.numpy().ravel()
        scale = max(float(np.abs(b).max()), 1e-4 * float(np.abs(gref).max()))
        d = np.abs(a - b)
        print(f"gradParameters [{off}:{off + k}]: max|d| {d.max():.3e} against {3e-2 * scale:.3e}")
        assert d.max() <= 3e-2 * scale, f"gradParameters [{off}:{off + k}]"
        off += k
    assert off == g.size
    return gref


def make_jpgs(d, n=6, size=64, odd=None):
    """n random size x size JPEGs cat_000.jpg ... in directory d; image number `odd`, if any, is 48 x 80."""
    from PIL import Image
    rs = np.random.RandomState(0)
    for i in range(n):
        shape = (48, 80, 3) if i == odd else (size, size, 3)
        Image.fromarray((rs.rand(*shape) * 255).astype(np.uint8)).save(os.path.join(d, f"cat_{i:03d}.jpg"), quality=95)


# ------------------------------------------------------------------------------ an engine net restated in torch fp64
def snapshot(net):
    """Parameters and running statistics of every module, as host arrays taken now (depth first, as getParameters orders them)."""
    snap = {}
    for m in net.listModules():
        d = {k: getattr(m, k).numpy().copy() for k in ("weight", "bias", "running_mean", "running_var") if getattr(m, k, None) is not None}
        if d:
            snap[id(m)] = d
    return snap


KINK = 1e-4        # relative to max|h|: inside it the side of PReLU's kink is the last bit's, not the net's (test_autoencoder_vs_torch)


def torch_twin(net, snap, h, params, taps, masks=None, sides=None):
    """nn.Sequential `net` restated in torch fp64 on the snapshot's values.  params collects the leaves in getParameters' order; taps
    records every child container's output (retain_grad), the torch running statistics per batch-norm module and the output per
    nn.Linear.  masks: {id(an nn.Dropout / nn.SpatialDropout): the mask the device was given}.  sides: {id(an nn.PReLU): the device's
    input to it} - where the twin's own input lies within KINK max|h| of zero the twin takes the device's side of the kink
    (teacher-forced, as the dropout masks are); taps counts those elements."""
    for m in net.modules:
        t = m.typename
        s = snap.get(id(m), {})
        leaf = lambda k: torch.tensor(s[k], dtype=torch.float64, requires_grad=True)
        if t == "nn.Sequential":
            h = torch_twin(m, snap, h, params, taps, masks, sides)
            h.retain_grad()
            taps[id(m)] = h
        elif t in ("nn.SpatialConvolution", "cudnn.SpatialConvolution", "nn.Linear"):
            w, b = leaf("weight"), leaf("bias")
            params += [w, b]
            h = F.conv2d(h, w, b, padding=m.padH) if "Convolution" in t else F.linear(h, w, b)
            if t == "nn.Linear":
                taps[id(m)] = h
        elif t in ("nn.SpatialBatchNormalization", "nn.BatchNormalization"):
            w, b = leaf("weight"), leaf("bias")
            params += [w, b]
            rm, rv = torch.tensor(s["running_mean"], dtype=torch.float64), torch.tensor(s["running_var"], dtype=torch.float64)
            taps[id(m)] = (rm, rv)
            h = F.batch_norm(h, rm, rv, w, b, training=True, momentum=0.1, eps=1e-5)
        elif t == "nn.LeakyReLU":
            h = torch.where(h >= 0, h, h * m.negative_scale)
        elif t == "nn.PReLU":
            w = leaf("weight")
            params.append(w)
            pos = h > 0
            if sides and id(m) in sides:
                a = h.detach().abs()
                near = a <= KINK * a.max()
                pos = torch.where(near, torch.from_numpy(sides[id(m)].reshape(tuple(h.shape)) > 0), pos)
                taps["forced", id(m)] = (int(near.sum()), int((pos != (h > 0)).sum()))
            h = torch.where(pos, h, h * w)
        elif t == "nn.SpatialMaxPooling":
            h = F.max_pool2d(h, 2)
        elif t == "nn.SpatialUpSamplingNearest":
            h = F.interpolate(h, scale_factor=2, mode="nearest")
        elif t in ("nn.Dropout", "nn.SpatialDropout"):
            h = h * masks[id(m)]
        elif t == "nn.View":
            h = h.reshape(h.shape[0], *m.sizes)        # V's View(feat) flattens: the same as reshape(N, -1), and an error if feat is not all
        elif t == "nn.Sigmoid":
            h = torch.sigmoid(h)
        elif t == "nn.SoftMax":
            h = torch.softmax(h, 1)
        else:
            raise AssertionError(t)
    return h
