"""Differentiable augmentation of D's input (train.py --D_diffaug POLICY; Zhao et al. 2020, "DiffAugment"; not in the reference).

The same random colour / translation / cutout transform T goes over every image D sees, real and fake, in the D-step and in the
G-step, and G's gradient is taken through T (cg_diffaug_forward / cg_diffaug_backward, include/catgan.h; csrc/diffaug.hip).  This
module holds the host side: the policy's names, the host twin of the descriptor draws (the fp32 operations of the kernel in its
order, on tensor.SplitMix.u01's arithmetic), the fp64 restatement of T and of its adjoint, and the DiffAugment object
adversarial.iteration calls, whose descriptor buffers are persistent (nothing allocates inside a captured iteration).

Arrays here are channels last, [N][H][W][C], as the kernels see them; desc is [N][8] = (b, s, c, tx, ty, cy, cx, 0) per image.
"""
import numpy as np
import torch

from .tensor import SplitMix, Tensor, device, lib, rng, stream

COLOR, TRANSLATION, CUTOUT = 1, 2, 4
NAMES = {"color": COLOR, "translation": TRANSLATION, "cutout": CUTOUT}
DRAWS = 8          # counters per image, whatever the policy
f32, f64 = np.float32, np.float64


def parse_policy(text):
    """"color,translation,cutout" -> 7.  An integer 1..7 passes through; an unknown name, an empty policy or a number outside 1..7 raises."""
    if isinstance(text, (int, np.integer)) and not isinstance(text, bool):
        p = int(text)
    else:
        p = 0
        for name in str(text).split(","):
            name = name.strip()
            if name not in NAMES:
                raise ValueError(f"D_diffaug: unknown augmentation {name!r} (known: {', '.join(NAMES)})")
            p |= NAMES[name]
    if not 1 <= p <= 7:
        raise ValueError(f"D_diffaug: policy {p} outside 1..7")
    return p


def policy_names(policy):
    return ",".join(n for n, bit in NAMES.items() if policy & bit)


def _round_of(L, f):
    return int(f32(f32(L) * f32(f)) + f32(0.5))


def geometry(H, W):
    """(Rh, Rw, ch, cw): the largest shift per axis and the cutout's size."""
    return _round_of(H, 0.125), _round_of(W, 0.125), _round_of(H, 0.5), _round_of(W, 0.5)


def draw_np(seed, offset, N, H, W):
    """desc[N][8] as the kernel draws it at counters offset + 8n + k: the same fp32 operations in the same order."""
    g = SplitMix(seed)
    g.offset = int(offset)
    u = g.u01(DRAWS * N).reshape(N, DRAWS)
    Rh, Rw, ch, cw = geometry(H, W)
    d = np.zeros((N, DRAWS), f32)
    d[:, 0] = u[:, 0] - f32(0.5)
    d[:, 1] = f32(2.0) * u[:, 1]
    d[:, 2] = u[:, 2] + f32(0.5)
    d[:, 3] = np.floor(u[:, 3] * f32(2 * Rw + 1)) - f32(Rw)
    d[:, 4] = np.floor(u[:, 4] * f32(2 * Rh + 1)) - f32(Rh)
    d[:, 5] = np.floor(u[:, 5] * f32(H + 1 - ch % 2))
    d[:, 6] = np.floor(u[:, 6] * f32(W + 1 - cw % 2))
    assert d.dtype == f32
    return d


def _mix(v, m, k):
    return (v - m) * k + m


def _cutout_mask(desc_n, H, W):
    """True where image n's cutout rectangle covers the image."""
    _, _, ch, cw = geometry(H, W)
    r0, c0 = int(desc_n[5]) - ch // 2, int(desc_n[6]) - cw // 2
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy >= r0) & (yy < r0 + ch) & (xx >= c0) & (xx < c0 + cw)


def _shift(a, ty, tx):
    """out[y][x] = a[y - ty][x - tx] where that lies in the image, else 0 (a: [H][W][C])."""
    H, W = a.shape[:2]
    out = np.zeros_like(a)
    ys, xs = slice(max(0, ty), min(H, H + ty)), slice(max(0, tx), min(W, W + tx))
    yd, xd = slice(max(0, -ty), min(H, H - ty)), slice(max(0, -tx), min(W, W - tx))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[ys, xs] = a[yd, xd]
    return out


def forward_np(x, desc, policy):
    """T in fp64 (x: [N][H][W][C], any float type; desc: [N][8]); with a policy without colour the values are moved, never changed."""
    x = np.asarray(x)
    N, H, W, C = x.shape
    out = np.zeros(x.shape, f64)
    for n in range(N):
        b, s, c = (f64(v) for v in desc[n][:3])
        v = x[n].astype(f64)
        if policy & COLOR:
            v = v + b
            if C > 1:
                v = _mix(v, v.sum(axis=2, keepdims=True) / C, s)
            v = _mix(v, v.mean(), c)
        if policy & TRANSLATION:
            v = _shift(v, int(desc[n][4]), int(desc[n][3]))
        if policy & CUTOUT:
            v = np.where(_cutout_mask(desc[n], H, W)[:, :, None], 0.0, v)
        out[n] = v
    return out


def backward_np(g, desc, policy):
    """T's adjoint in fp64: g the gradient with respect to T's output, the result the gradient with respect to its input."""
    g = np.asarray(g)
    N, H, W, C = g.shape
    out = np.zeros(g.shape, f64)
    for n in range(N):
        _, s, c = (f64(v) for v in desc[n][:3])
        v = g[n].astype(f64)
        if policy & CUTOUT:
            v = np.where(_cutout_mask(desc[n], H, W)[:, :, None], 0.0, v)
        if policy & TRANSLATION:
            v = _shift(v, -int(desc[n][4]), -int(desc[n][3]))
        if policy & COLOR:
            v = _mix(v, v.mean(), c)
            if C > 1:
                v = _mix(v, v.sum(axis=2, keepdims=True) / C, s)
        out[n] = v
    return out


class DiffAugment:
    """The policy and one persistent descriptor buffer per (role, batch size): role "D" for the D-step's batch, "G" for the G-step's,
    whose backward reuses the forward's draws.  Draws come from the process's counter stream (the rank's, under data parallelism),
    8 N counters per call; forward(..., offset=) applies draws reserved earlier with reserve()."""

    def __init__(self, policy):
        self.policy = parse_policy(policy)
        self._desc = {}

    def desc(self, role, N):
        d = self._desc.get((role, N))
        if d is None:
            d = self._desc[(role, N)] = torch.zeros(N * DRAWS, dtype=torch.float32, device=device())
        return d

    def desc_np(self, role, N):
        return self.desc(role, N).cpu().numpy().reshape(N, DRAWS)

    @staticmethod
    def reserve(N):
        """Take image 0..N-1's counters from the stream now; -> the offset to hand to forward()."""
        return rng().take(DRAWS * N)

    @staticmethod
    def _dims(x):
        assert isinstance(x, Tensor) and x.fmt == "nhwc" and x.ups == 0 and x.dim() == 4, f"DiffAugment: an NHWC batch, not {x}"
        N, C, H, W = x.shape
        return N, H, W, C

    def forward(self, x, y, role, offset=None):
        """y = T(x) with fresh draws, stored for (role, N).  y may be x."""
        N, H, W, C = self._dims(x)
        assert self._dims(y) == (N, H, W, C)
        r = rng()
        if offset is None:
            offset = self.reserve(N)
        lib().diffaug_forward(stream(), x.ptr, y.ptr, self.desc(role, N).data_ptr(), N, H, W, C, self.policy, 1, r.seed, offset, r.base_ptr())
        y.epoch.bump()
        return y

    def backward(self, gy, gx, role):
        """gx = T^T gy with the draws the last forward of (role, N) stored.  gx may be gy."""
        N, H, W, C = self._dims(gy)
        assert self._dims(gx) == (N, H, W, C)
        lib().diffaug_backward(stream(), gy.ptr, gx.ptr, self.desc(role, N).data_ptr(), N, H, W, C, self.policy)
        gx.epoch.bump()
        return gx
