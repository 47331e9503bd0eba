"""What several test modules share (a plain module, imported as tests/plan_trace.py is): the two measures of the parity tests, the
`options` context that forces dispatch tunables, `counter` that reads a launch counter, the per-tensor gradient rule, the JPEG directory
of the loader tests, the torch fp64 twin of an engine nn.Sequential, and the measures, launch arithmetic, inputs and guarded device
buffers of the memory-bound edge sweeps."""
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
    """A launch counter kept among the options (CG_WINO3_LAUNCHES, CG_WINO_DGRAD_FUSE_LAUNCHES, CG_SAMPLER_ATOMIC_LAUNCHES): how a test tells which kernel ran."""
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


# ------------------------------------------------------------------------------ memory-bound edge sweeps (test_gpu_membound_edges.py)
U24 = 2.0 ** -24          # unit roundoff of fp32: one rounding moves a value by at most U24 of its magnitude
TINY = 2.0 ** -149        # ... or, where it underflows, by the smallest fp32 denormal


def bits_equal(a, b, what=""):
    """fp32 arrays equal bit for bit (so -0.0 != +0.0), and finite."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape, f"{what}: {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
    assert np.isfinite(a).all(), f"{what}: non-finite values"
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=what)


def rounding_close(a, ref, terms, r, what="", slack=0.0):
    """|a - ref| <= r (U24 terms + TINY) + slack per element (per column for a reduction): ref the fp64 value, terms the sum of the
    magnitudes of the addends of that element, r the number of fp32 roundings on the longest chain of the kernel's expression plus 2
    (a number, or an array that broadcasts against ref where the chain's length depends on the element), slack an error propagated from
    an input that is checked on its own.  Nothing here is scaled by a tensor's maximum."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, f"{what}: shape {a.shape} vs {ref.shape}"
    assert np.isfinite(a).all(), f"{what}: non-finite values"
    rr = np.broadcast_to(np.asarray(r, dtype=np.float64), ref.shape)
    bound = rr * (U24 * np.broadcast_to(np.abs(terms), ref.shape) + TINY) + slack
    d = np.abs(a - ref)
    worst = float((d / bound).max()) if d.size else 0.0
    rs = f"{r}" if np.ndim(r) == 0 else f"{int(rr.min())}..{int(rr.max())}"
    print(f"{what}: worst |d| / bound = {worst:.3f} (r = {rs})")
    k = int(np.argmax(d / bound)) if d.size else 0
    assert worst <= 1.0, f"{what}: |d| = {worst:.3f} x the bound of {rr.ravel()[k] if d.size else r:g} roundings at flat index {k}"
    return worst


def ew_grid(n, cap):
    """common.h ew_grid(): workgroups of 256 lanes for n items, capped."""
    return int(max(1, min((n + 255) // 256, cap)))


def fixed_channel_grid(n4, C4, cap):
    """fused.hip fixed_channel_grid(): ew_grid rounded down to a multiple of C4 / gcd(C4, 256), at least that multiple."""
    import math
    b = min((n4 + 255) // 256, cap)
    if 256 % C4:
        m = C4 // math.gcd(C4, 256)
        b = max(m, b // m * m)
    return int(max(1, b))


def col_launch(M, C, v4, wgs):
    """ops.hip colreduce_launch() / fused.hip cg_bn_act_backward_stats(): channel blocks, row chunks and rows per chunk of a column
    reduction over [M][C]; v4: the float4 kernels (C % 4 == 0, aligned), wgs: kNumCU * kColReduceWgsPerCU."""
    qb = 32 if C >= 128 else 16
    cblocks = -(-(C // 4) // qb) if v4 else -(-C // 64)
    chunks = max(1, min((M + 63) // 64, wgs // cblocks))
    rows = (-(-M // chunks) + 3) // 4 * 4
    chunks = -(-M // rows)
    return dict(qb=qb, RL=256 // qb if v4 else 4, cblocks=cblocks, chunks=chunks, rows=rows)


def col_tree(chunks):
    """common.h col_tree_layout(): chunks per group, groups, size of the last group."""
    G = max(16, -(-chunks // 32))
    ngroups = -(-chunks // G)
    return dict(G=G, ngroups=ngroups, last=chunks - (ngroups - 1) * G)


def edge_normal(rng, shape, plant=True):
    """Seeded fp32 normal data, channels last, |mean| <= std per channel (well conditioned), with +0.0, -0.0 and +-1e-30 planted at the
    first and last element and at random places.  rng: a numpy Generator."""
    C = shape[-1]
    std = rng.uniform(0.5, 2.0, C).astype(np.float32)
    mean = (rng.uniform(-1.0, 1.0, C) * std).astype(np.float32)
    x = rng.standard_normal(shape, dtype=np.float32) * std + mean
    if plant:
        flat = x.reshape(-1)
        vals = np.array([0.0, -0.0, 1e-30, -1e-30], np.float32)
        k = int(min(64, max(1, flat.size // 8)))
        pos = rng.integers(0, flat.size, 4 * k)
        pos[:4] = [0, flat.size - 1, flat.size // 2, flat.size // 3]
        flat[pos] = np.tile(vals, k)
    return x


def duplicate_in_windows(rng, x, frac=0.2):
    """x: [N][H][W][C].  In a fraction of the 2x2 windows copy one element over one, two or all three of the others (ties for a max)."""
    N, H, W, C = x.shape
    w = x.reshape(N, H // 2, 2, W // 2, 2, C)
    pick = rng.random((N, H // 2, W // 2, C)) < frac
    src = w[:, :, 1, :, 0, :].copy()                      # the third element in scan order: a tie must still go to an earlier one
    for iy, ix in ((0, 0), (0, 1), (1, 1)):
        sel = pick & (rng.random(pick.shape) < 0.6)
        w[:, :, iy, :, ix, :] = np.where(sel, src, w[:, :, iy, :, ix, :])
    return x


# ------------------------------------------------------------------------------ guarded device buffers of the edge sweeps
def dev(a, misaligned=False):
    """A flat device copy of a; misaligned: a view one float into a larger tensor (4 bytes off a 16-byte boundary).  The tensor it
    lives in has four guard floats on either side, which host() checks."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return torch.from_numpy(a.reshape(-1)).cuda()
    big = torch.full((a.size + 9,), 777.0, dtype=torch.float32, device="cuda")
    o = 5 if misaligned else 4
    v = big[o:o + a.size]
    v.copy_(torch.from_numpy(a.reshape(-1)))
    assert v.data_ptr() % 16 == (4 if misaligned else 0)
    v.guard = (big, o, a.size)
    return v


def out_like(n, misaligned=False, fill=555.0):
    """A guarded output buffer of n floats, prefilled (with NaN an element the kernel leaves unwritten fails every measure here)."""
    return dev(np.full(int(n), fill, np.float32), misaligned)


def host(t, shape=None):
    big, o, n = t.guard
    g = big.cpu().numpy()
    assert (g[:o] == 777.0).all() and (g[o + n:] == 777.0).all(), "a kernel wrote outside its tensor"
    a = g[o:o + n].copy()
    return a if shape is None else a.reshape(shape)
