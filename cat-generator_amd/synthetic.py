"""train_v.lua's synthetic fakes (train_v.lua:294-668): V's training input, made on the device.

The reference builds every fake with per-pixel Lua loops.  Here the host only draws the random choices - kind, pool rows, bank
overlays, shift direction, warp length, offsets, base values - from a seeded numpy RandomState (as adversarial.State.random
stands in for math.random; Lua's own stream is not reproduced), packs them into the int32 / float descriptor arrays of
include/catgan.h, and two launches per batch do the work: cg_synth_overlays (getGaussianOverlay) and cg_synth_images (the four
kinds, the optional second-level mix, the per-image normalisation), written straight into a NHWC batch.

Two pieces are sequential per overlay and stay on the host, in numpy: the random-walk bank (createGaussianOverlay,
:573-637; 1000 walks, vectorised across the walks, built once per run) and createPixelwiseOverlay (:645-668, once per batch
that needs one).  `compose_overlays_np` / `synth_images_np` are the numpy twin of the two kernels (the tests hold them together).
"""
import numpy as np
import torch

from .tensor import Tensor, device, lib, stream

MIX, STAMP, WARP, RANDOM = 0, 1, 2, 3
KINDS = (MIX, STAMP, WARP, RANDOM)
DI, DF, DO = 18, 8, 5          # ints / floats per image descriptor, ints per overlay descriptor (catgan.h)
_DIRECTIONS = np.array([[-1, 0], [-1, 1], [0, 1], [1, 1], [1, 0], [1, -1], [0, -1], [-1, -1]], np.int64)   # :585-594


def within_image_coords(y, x, maxY, maxX):
    """withinImageCoords (train_v.lua:450-467), 1-based and literal: Lua's % is the floored modulo."""
    y = y % maxY
    if y < 1:
        y = maxY - (-y)
    x = x % maxX
    if x < 1:
        x = maxX - (-x)
    return y, x


def gaussian(size, sigma=0.25):
    """image.gaussian(size) with its defaults [upstream, recalled]: amplitude 1, not normalised, centre 0.5*size + 0.5 (1-based
    taps), g = exp(-((j-c)/(sigma*size))^2/2 - ((i-c)/(sigma*size))^2/2); computed in double, stored as float (:555 `:float()`)."""
    c = 0.5 * size + 0.5
    i = np.arange(1, size + 1, dtype=np.float64)
    u = ((i - c) / (sigma * size)) ** 2 / 2.0
    return np.exp(-(u[:, None] + u[None, :])).astype(np.float32)


def convolve_same(img, ker):
    """image.convolve(img, ker, "same") [upstream, recalled]: the full 2-D convolution cropped from row / column ceil(k/2)
    (1-based), i.e. out[y,x] = sum_uv img[y+s-u, x+s-v] ker[u,v] with s = ceil(k/2) - 1, zero outside; accumulated in double."""
    H, W = img.shape
    k = ker.shape[0]
    s = (k + 1) // 2 - 1
    pad = np.zeros((H + 2 * k, W + 2 * k), np.float64)
    pad[k:k + H, k:k + W] = img
    out = np.zeros((H, W), np.float64)
    for u in range(k):
        for v in range(k):
            out += pad[k + s - u:k + s - u + H, k + s - v:k + s - v + W] * np.float64(ker[u, v])
    return out.astype(np.float32)


def create_overlay_bank(H, W, rs, n=1000, n_points=10000):
    """OVERLAYS (train_v.lua:536-541): n x createGaussianOverlay(H, W, n_points, 0) (:573-637), the n random walks stepped
    together.  Each walk: 2 % of the steps jump to a random pixel (remembering the last one), 10 % of the rest go back to the last
    pixel, the others move to one of the 8 neighbours that stays inside; every visit adds 1; divided by the maximum."""
    cy, cx = rs.randint(0, H, n), rs.randint(0, W, n)
    ly, lx = rs.randint(0, H, n), rs.randint(0, W, n)
    counts = np.zeros(n * H * W, np.int64)
    base = np.arange(n, dtype=np.int64) * (H * W)
    for _ in range(n_points):
        p, q = rs.rand(n), rs.rand(n)
        jump = p < 0.02
        back = ~jump & (q < 0.10)
        move = ~jump & ~back
        jy, jx = rs.randint(0, H, n), rs.randint(0, W, n)
        ny, nx = cy.copy(), cx.copy()
        ny[jump], nx[jump] = jy[jump], jx[jump]
        ny[back], nx[back] = ly[back], lx[back]
        ly = np.where(jump | move, cy, ly)
        lx = np.where(jump | move, cx, lx)
        todo = np.nonzero(move)[0]
        while todo.size:                                    # `while not found`: draw directions until the step stays inside
            d = _DIRECTIONS[rs.randint(0, 8, todo.size)]
            ty, tx = cy[todo] + d[:, 0], cx[todo] + d[:, 1]
            ok = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
            ny[todo[ok]], nx[todo[ok]] = ty[ok], tx[ok]
            todo = todo[~ok]
        cy, cx = ny, nx
        np.add.at(counts, base + cy * W + cx, 1)
    bank = counts.reshape(n, H, W).astype(np.float32)
    bank /= bank.reshape(n, -1).max(axis=1)[:, None, None]
    return bank


def create_pixelwise_overlay(H, W, rs):
    """createPixelwiseOverlay (train_v.lua:645-668): row by row, a pixel is min(2u, 1) with probability 1 - p, else 0; p drifts
    by +-pChange after every pixel."""
    p, pchange = rs.rand(), rs.rand() / 10
    keep, val, up = rs.rand(H * W), rs.rand(H * W), rs.rand(H * W)
    out = np.zeros(H * W, np.float32)
    for i in range(H * W):
        if keep[i] > p:
            out[i] = min(2 * val[i], 1.0)
        p = max(p - pchange, 0.0) if up[i] > 0.5 else min(p + pchange, 1.0)
    return out.reshape(H, W)


class Plan:
    """The random choices of one createSyntheticImages(N) call: overlay descriptors, the pixelwise overlays (stored after the
    composed ones), and the per-image descriptors."""

    def __init__(self, ovl, pix, idesc, fdesc):
        self.ovl, self.pix, self.idesc, self.fdesc = ovl, pix, idesc, fdesc

    @property
    def n_overlays(self):
        return len(self.ovl) + len(self.pix)


class Generator:
    """createSyntheticImages (train_v.lua:294-316) over a resident NHWC pool [P,H,W,C] (adversarial.TrainData.pool)."""

    def __init__(self, dims, rs, bank=None, bank_size=1000):
        self.C, self.H, self.W = (int(d) for d in dims)
        self.rs = rs
        self.bank = bank if bank is not None else create_overlay_bank(self.H, self.W, rs, bank_size)
        self._dev = {}

    # ---------------------------------------------------------------- host: the random choices
    def draw(self, N, npool, kind=None, second=None):
        """One createSyntheticImages(N) call.  kind / second force the branch (tests); by default they are drawn as :300-313 do."""
        rs, nb = self.rs, self.bank.shape[0]
        ovl, pix = [], []

        def gauss(blur=4):
            ovl.append(list(rs.randint(0, nb, 4)) + [blur])
            return len(ovl) - 1

        def pixelwise():
            pix.append(create_pixelwise_overlay(self.H, self.W, rs))
            return -len(pix)                                    # resolved once the number of composed overlays is known

        def mix_overlay():                                      # mixImageLists (:343-348)
            return gauss() if rs.rand() < 0.5 else pixelwise()

        def level(k):
            I, F = np.zeros((N, 8), np.int64), np.zeros((N, 4), np.float32)
            I[:, 0] = k
            if k == MIX:                                        # :376-382
                I[:, 1], I[:, 2] = rs.randint(0, npool, N), rs.randint(0, npool, N)
                I[:, 3] = mix_overlay()
            elif k == STAMP:                                    # :388-444 (the unused `p` of :398 is not drawn)
                I[:, 3] = gauss()
                I[:, 1] = rs.randint(0, npool, N)
                I[:, 6], I[:, 7] = rs.randint(1, 11, N), rs.randint(1, 11, N)
            elif k == WARP:                                     # :450-484: length = 1 + math.random(4)
                I[:, 3], I[:, 4] = gauss(), gauss()
                I[:, 1] = rs.randint(0, npool, N)
                F[:, 0] = 1 + rs.randint(1, 5, N)
            else:                                               # :490-528
                I[:, 3], I[:, 4] = gauss(10), gauss(10)
                for i in range(N):
                    I[i, 5] = gauss(4)
                I[:, 6], I[:, 7] = rs.randint(1, 11, N) - 5, rs.randint(1, 11, N) - 5
                F[:, :3] = rs.rand(N, 3)
            return I, F

        def pick():
            p = rs.rand()
            return MIX if p < 0.25 else (WARP if p < 0.5 else (STAMP if p < 0.75 else RANDOM))   # :300-308

        k1 = pick() if kind is None else kind
        I1, F1 = level(k1)
        sub = (rs.rand() < 0.33) if second is None else bool(second)
        idesc = np.zeros((N, DI), np.int64)
        fdesc = np.zeros((N, DF), np.float32)
        idesc[:, 0:8], fdesc[:, 0:4] = I1, F1
        idesc[:, 8] = -1
        if sub:                                                 # :310-313: a second call without sub-calls, mixed in
            I2, F2 = level(pick())
            idesc[:, 8:16], fdesc[:, 4:8] = I2, F2
            idesc[:, 16] = mix_overlay()
        for cols in ((3, 4, 5, 11, 12, 13, 16),):              # pixelwise placeholders -> their slots behind the composed overlays
            blk = idesc[:, cols]
            blk[blk < 0] = len(ovl) + (-blk[blk < 0] - 1)
            idesc[:, cols] = blk
        # the overlay fields a kind does not use point at slot 0 (the kernel clamps anyway)
        return Plan(np.asarray(ovl, np.int32).reshape(-1, DO), pix, idesc.astype(np.int32), fdesc)

    # ---------------------------------------------------------------- device: two launches
    def _buffers(self, plan):
        H, W = self.H, self.W
        if "bank" not in self._dev:
            self._dev["bank"] = torch.from_numpy(np.ascontiguousarray(self.bank)).to(device())
        k = max(plan.n_overlays, 1)
        ov = self._dev.get("ovl")
        if ov is None or ov.numel() < k * H * W:
            self._dev["ovl"] = ov = torch.empty(k * H * W, dtype=torch.float32, device=device())
        return self._dev["bank"], ov

    def run(self, plan, pool, dst):
        """Write the plan's N images into dst (a device pointer to [N,H,W,C] floats) from pool ([P,C,H,W] Tensor, NHWC).
        One host->device copy of the packed descriptors, no host synchronisation."""
        assert pool.fmt == "nhwc" and tuple(pool.shape[1:]) == (self.C, self.H, self.W)
        bank, ov = self._buffers(plan)
        H, W = self.H, self.W
        N = plan.idesc.shape[0]
        parts = [plan.ovl.reshape(-1), plan.idesc.reshape(-1), plan.fdesc.reshape(-1).view(np.int32)]
        parts += [p.astype(np.float32).reshape(-1).view(np.int32) for p in plan.pix]
        blob = np.concatenate(parts).astype(np.int32)
        d = self._dev.get("desc")
        if d is None or d.numel() < blob.size:
            self._dev["desc"] = d = torch.empty(max(blob.size, 4096), dtype=torch.int32, device=device())
        d[:blob.size].copy_(torch.from_numpy(blob), non_blocking=True)
        base = d.data_ptr()
        o_i = base + 4 * plan.ovl.size
        o_f = o_i + 4 * plan.idesc.size
        o_p = o_f + 4 * plan.fdesc.size
        nc = len(plan.ovl)
        if plan.pix:
            lib().memcpy_d2d(stream(), ov.data_ptr() + 4 * nc * H * W, o_p, 4 * len(plan.pix) * H * W)
        lib().synth_overlays(stream(), bank.data_ptr(), bank.shape[0], base, ov.data_ptr(), nc, H, W)
        lib().synth_images(stream(), pool.ptr, pool.shape[0], ov.data_ptr(), max(plan.n_overlays, 1), o_i, o_f, dst, N,
                           self.C, H, W)

    def images(self, N, pool, **kw):
        """createSyntheticImages(N) as a device Tensor [N,C,H,W] (NHWC)."""
        plan = self.draw(N, pool.shape[0], **kw)
        out = Tensor.empty((N, self.C, self.H, self.W), "nhwc")
        self.run(plan, pool, out.ptr)
        return out


# -------------------------------------------------------------------- the numpy twin of the two kernels
def compose_overlays_np(bank, ovl):
    """cg_synth_overlays on the host: getGaussianOverlay (train_v.lua:543-561) per descriptor row."""
    out = []
    for o1, o2, o3, o4, blur in np.asarray(ovl).reshape(-1, DO):
        r = np.clip(bank[o1] * np.float32(2) - bank[o2], 0, 1).astype(np.float32)
        r = np.clip(r + (bank[o3] * bank[o4]) * np.float32(2), 0, 1).astype(np.float32)
        if blur > 0:
            r = convolve_same(r, gaussian(int(blur)))
            m = r.max()
            r = r / (m if m > 0 else np.float32(1))
        out.append(r.astype(np.float32))
    return np.asarray(out, np.float32).reshape(-1, bank.shape[1], bank.shape[2])


def _wrap(v, m):
    return np.mod(v, m)


def _level_np(I, F, pool, ov, C, H, W):
    kind = int(I[0])
    A, B = pool[I[1]], pool[I[2]]                              # [C,H,W]
    OA, OB, OC = ov[I[3]], ov[I[4]], ov[I[5]]
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if kind == MIX:
        v = OA[None] * A + (np.float32(1) - OA[None]) * B
    elif kind == STAMP:
        yy, xx = _wrap(y + I[6], H), _wrap(x + I[7], W)
        v = (np.float32(1) - OA[None]) * A + OA[None] * A[:, yy, xx]
    elif kind == WARP:
        ln = np.float32(F[0])
        iy = np.clip(y.astype(np.float32) + (OA * np.float32(2) - np.float32(1)) * ln, 0, H - 1).astype(np.float32)
        ix = np.clip(x.astype(np.float32) + (OB * np.float32(2) - np.float32(1)) * ln, 0, W - 1).astype(np.float32)
        y0, x0 = np.floor(iy).astype(np.int64), np.floor(ix).astype(np.int64)
        y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
        wy, wx = (iy - y0).astype(np.float32), (ix - x0).astype(np.float32)
        top = (1 - wx) * A[:, y0, x0] + wx * A[:, y0, x1]
        bot = (1 - wx) * A[:, y1, x0] + wx * A[:, y1, x1]
        v = (1 - wy) * top + wy * bot
    else:
        v = np.empty((C, H, W), np.float32)
        for c in range(C):
            yy, xx = _wrap(y + (c + 1) * I[6], H), _wrap(x + (c + 1) * I[7], W)
            v[c] = np.float32(F[c]) + OA * OB[yy, xx] - OC[yy, xx]
    v = v.astype(np.float32)
    if kind == RANDOM:
        a = np.float32(abs(v.min()))
        v = (v + a).astype(np.float32)
    return (v / v.max()).astype(np.float32)


def synth_images_np(pool, overlays, idesc, fdesc):
    """cg_synth_images on the host.  pool [P,C,H,W] (logical layout), overlays [K,H,W]; returns [N,C,H,W]."""
    pool = np.asarray(pool, np.float32)
    C, H, W = pool.shape[1:]
    out = []
    for I, F in zip(np.asarray(idesc), np.asarray(fdesc)):
        a = _level_np(I[0:8], F[0:4], pool, overlays, C, H, W)
        if I[8] >= 0:
            b = _level_np(I[8:16], F[4:8], pool, overlays, C, H, W)
            o = overlays[I[16]][None]
            a = (o * a + (np.float32(1) - o) * b).astype(np.float32)
            a = (a / a.max()).astype(np.float32)
        out.append(a)
    return np.asarray(out, np.float32)


def plan_overlays_np(gen, plan):
    """All overlays of a plan on the host: the composed ones, then the pixelwise ones."""
    comp = compose_overlays_np(gen.bank, plan.ovl) if len(plan.ovl) else np.zeros((0, gen.H, gen.W), np.float32)
    if plan.pix:
        comp = np.concatenate([comp, np.asarray(plan.pix, np.float32)])
    return comp
