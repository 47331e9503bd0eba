"""utils/nn_utils.lua — what the training step uses: createNoiseInputs :35-39,
createImagesFromNoise :45-69, createImages :75-77, getNumberOfParameters :453-462, activateCuda :620-680 — and the
consumer side of the trained nets: sortImagesByPrediction :89-117, visualizeProgress :130-186 (without
the display server), toRgb :188-220, imagesToGridTensor / saveImagesAsGrid :526-583, rateWithV :686-711; and sample.lua's
nearest-neighbour check (:131-151) both as the reference's host loop (findClosestNeighboursOf) and on the device
(findClosestNeighboursOnDevice: cg_nearest_update over the pools of a dataset.SequentialLoader)."""
import os
import struct
import zlib

import numpy as np

from . import nn
from .dataset import COLOR_SPACES
from .tensor import Tensor, lib, rng, stream


def createNoiseInputs(S, N):
    """U(-1,1) noise [N, noiseDim] (utils/nn_utils.lua:35-39), generated on the device from the engine's counter stream.  A FRESH
    tensor per call, as upstream: callers keep what they get (train.lua:220 holds VIS_NOISE_INPUTS for the whole run)."""
    return _fill_noise(Tensor.empty((N, S.OPT["noiseDim"])))


def stepNoiseInputs(S, N):
    """The training iteration's private form of createNoiseInputs: one persistent buffer per N (the D-step's half batch and the
    G-step's full batch never share one).  A captured iteration (cg_graph_*) must find its noise at the same address on every
    replay, and the step itself never keeps a noise tensor across two calls; nothing outside adversarial.iteration may use this."""
    cache = S.__dict__.setdefault("_noise_bufs", {})
    t = cache.get(N)
    if t is None:
        t = cache[N] = Tensor.empty((N, S.OPT["noiseDim"]))
    return _fill_noise(t)


def _fill_noise(t, offset=None):
    """offset: an explicit position of the counter stream (the caller reserves it and advances the generator itself)."""
    r = rng()
    lib().rng_uniform_dev(stream(), t.ptr, t.nElement(), -1.0, 1.0, r.seed, r.take(t.nElement()) if offset is None else int(offset), r.base_ptr())
    return t


def stepNoiseInputsAt(S, N, offset):
    """stepNoiseInputs with the draws taken from `offset` of the counter stream instead of its current position: the G-step's noise
    drawn ahead of time (adversarial.iteration runs both generator forwards side by side) at the position it has in the reference's
    order - behind the D-step's dropout masks."""
    cache = S.__dict__.setdefault("_noise_bufs", {})
    t = cache.get(N)
    if t is None:
        t = cache[N] = Tensor.empty((N, S.OPT["noiseDim"]))
    return _fill_noise(t, offset)


def createImagesFromNoise(S, noiseInputs, outputAsList=False, *_, model=None):
    """G forward in chunks of OPT.batchSize (nn_utils.lua:48-58).  Note MODEL_G stays in training mode
    (train-mode BN on the chunk), exactly as upstream.  The reference's :clone() of each chunk is kept only when
    there is more than one chunk (the G output buffer is reused by the next forward).  `model`: another generator than
    S.MODEL_G (the averaged one of --G_ema)."""
    G = model if model is not None else S.MODEL_G
    noiseInputs = nn.to_device(noiseInputs)
    N = noiseInputs.size(1)
    bs = S.OPT["batchSize"]
    nBatches = -(-N // bs)
    if nBatches == 1:
        images = G.forward(noiseInputs)
    else:
        images = None
        for i in range(1, nBatches + 1):
            a, b = 1 + (i - 1) * bs, min(i * bs, N)
            generated = nn.as_nhwc(G.forward(noiseInputs.rows(a, b)))
            if images is None:
                images = Tensor.empty((N,) + generated.shape[1:], "nhwc")
            images.rows(a, b).copy(generated)
    if outputAsList:
        arr = images.numpy()
        return [arr[i] for i in range(arr.shape[0])]
    return images


def createImages(S, N, outputAsList=False):
    return createImagesFromNoise(S, createNoiseInputs(S, N), outputAsList)


def switchToEvaluationMode(S):
    """nn_utils.lua:334-340: dropout off, batch-norm on running statistics."""
    S.MODEL_G.evaluate()
    S.MODEL_D.evaluate()


def switchToTrainingMode(S):
    """nn_utils.lua:343-349."""
    S.MODEL_G.training()
    S.MODEL_D.training()


def sortImagesByPrediction(S, images, ascending=False, nbMaxOut=None):
    """nn_utils.lua:89-117: rate images with D (in chunks of OPT.batchSize) and sort them by D's certainty that they
    are real; returns (images as a host array [n,C,H,W], predictions [n]).  Used by sample.lua:104-105 and the
    epoch visualisation (nn_utils.lua:138-147)."""
    imgs = nn.as_nhwc(nn.to_device(images))
    N, bs = imgs.shape[0], S.OPT["batchSize"]
    preds = []
    for a in range(1, N + 1, bs):
        b = min(a + bs - 1, N)
        preds.append(nn.as_plain(S.MODEL_D.forward(imgs.rows(a, b))).numpy().reshape(-1))
    preds = np.concatenate(preds)
    order = np.argsort(preds, kind="stable")
    if not ascending:
        order = order[::-1]
    if nbMaxOut is not None:
        order = order[:nbMaxOut]
    return imgs.numpy()[order], preds[order]


def getNumberOfParameters(net):
    """nn_utils.lua:453-462: sums weight and bias sizes over listModules()."""
    n = 0
    for m in net.listModules():
        for name in ("weight", "bias"):
            t = getattr(m, name, None)
            if t is not None:
                n += t.nElement()
    return n


MSE_CHUNK = 4096           # elements of one chunk of cg_mse_forward's summation order (csrc/criterion.hip)
MSE_MAX_PARTIALS = 1024    # workgroup partials of one launch: beyond MSE_CHUNK * MSE_MAX_PARTIALS elements a workgroup walks several chunks


def mse_np(x, t):
    """nn.MSECriterion (cg_mse_forward / cg_mse_backward, include/catgan.h) stated in numpy: (loss float32, gradient float32 of x's
    shape).  The difference is taken in fp32, as Torch7 does; the squares are summed in fp64 (the device adds the same fp64 squares in
    another, fixed order: the two sums agree to n 2^-53 relative, so the rounded results are equal or neighbours) and the mean is
    rounded to fp32 once.  The gradient is norm * (x - t) with norm = float32(2) / float32(n): two fp32 operations, bit for bit."""
    f32 = np.float32
    x, t = np.asarray(x, dtype=f32), np.asarray(t, dtype=f32)
    assert x.shape == t.shape and x.size > 0
    n = x.size
    d = (x - t).astype(f32)
    loss = f32(np.sum(d.astype(np.float64) ** 2) / n)
    norm = f32(2.0) / f32(n)
    return loss, (norm * d).astype(f32)


def activateCuda(net):
    """nn_utils.lua:620-680: wrap the net in Copy layers unless it already contains some."""
    if any(isinstance(m, nn.Copy) for m in net.listModules()):
        return net
    tmp = nn.Sequential()
    tmp.add(nn.Copy("torch.FloatTensor", "torch.CudaTensor"))
    tmp.add(net)
    tmp.add(nn.Copy("torch.CudaTensor", "torch.FloatTensor"))
    return tmp


# ------------------------------------------------------------------ visual grids
def yuv2rgb(im):
    """image.yuv2rgb [upstream, recalled: the constants and the order of lua/image.lua:156-158] for a float32 [3, H, W] image, every
    operation a single fp32 one (the device form is colorspace_to_rgb in csrc/images.hip, same sequence).  The two matrices are five-digit
    constants, no exact inverses: a round trip leaves the unit cube by a few 1e-5, which _png_bytes clamps as image.save does."""
    f = np.float32
    y, u, v = (np.asarray(im[k], dtype=f) for k in range(3))
    return np.stack([y + f(1.13983) * v, (y - f(0.39465) * u) - f(0.58060) * v, y + f(2.03211) * u]).astype(f)


def _hue(p, q, t):
    """image.hsl2rgb's helper (lua/image.lua:171-178); 1/6 and 2/3 rounded to fp32 first."""
    f = np.float32
    sixth, two_thirds = f(1 / 6), f(2 / 3)
    t = np.where(t < f(0), t + f(1), t)
    t = np.where(t > f(1), t - f(1), t)
    return np.where(t < sixth, p + ((q - p) * f(6)) * t,
                    np.where(t < f(0.5), q, np.where(t < two_thirds, p + ((q - p) * (two_thirds - t)) * f(6), p)))


def hsl2rgb(im):
    """image.hsl2rgb [upstream, recalled: lua/image.lua:179-186] for a float32 [3, H, W] image with planes h, s, l; fp32 step by step
    (colorspace_to_rgb in csrc/images.hip is the same sequence)."""
    f = np.float32
    h, s, l = (np.asarray(im[k], dtype=f) for k in range(3))
    q = np.where(l < f(0.5), l * (f(1) + s), (l + s) - l * s)
    p = f(2) * l - q
    third = f(1 / 3)
    rgb = np.stack([_hue(p, q, h + third), _hue(p, q, h), _hue(p, q, h - third)])
    return np.where(s == f(0), l, rgb).astype(f)


def toRgb(images, colorSpace):
    """nn_utils.lua:188-220: 'rgb' as is, 'y' repeated over three channels, 'yuv' / 'hsl' through image.yuv2rgb / image.hsl2rgb.
    Returns a host array [n, 3, H, W].  Host arrays (what the grids hold) are converted in numpy; an engine tensor is converted on
    the device (cg_colorspace_convert, the same arithmetic) before it is copied back."""
    if colorSpace not in COLOR_SPACES:
        raise NotImplementedError(f"unknown colour space '{colorSpace}' (rgb | yuv | hsl | y)")
    if isinstance(images, Tensor):
        images = nn.as_nhwc(images)
        if colorSpace in ("yuv", "hsl"):
            out = Tensor.empty(images.shape, "nhwc")
            N, _, H, W = images.shape
            lib().colorspace_convert(stream(), images.ptr, out.ptr, N * H * W, COLOR_SPACES[colorSpace], COLOR_SPACES["rgb"])
            return out.numpy()
        images = images.numpy()
    images = np.asarray(images, dtype=np.float32)
    if images.ndim == 3:
        images = images[None]
    if colorSpace == "rgb":
        return images
    if colorSpace == "y":
        return np.tile(images, (1, 3, 1, 1))
    return np.stack([(yuv2rgb if colorSpace == "yuv" else hsl2rgb)(im) for im in images])


# the 3 x 5 digit glyphs the reference draws the epoch number with (CHAR_TENSORS, nn_utils.lua:465-515), one 15-bit row-major
# mask per digit
_DIGITS = (0b111101101101111, 0b001001001001001, 0b111001111100111, 0b111001011001111, 0b101101111001001,
           0b111100111001111, 0b111100111101111, 0b111001001001001, 0b111101111101111, 0b111101111001111)


def _glyph(d):
    bits = _DIGITS[d]
    return np.array([[(bits >> (14 - (r * 3 + c))) & 1 for c in range(3)] for r in range(5)], dtype=np.float32)


def imagesToGridTensor(images, height, width, epoch, dims=None):
    """nn_utils.lua:526-569: the first height*width images row by row on a black canvas of height*H + 7 rows, the epoch
    number in 3 x 5 digits at the bottom right (last digit rightmost).  images [n,C,H,W] in [0,1]; returns [C,Hpx,Wpx]."""
    images = np.asarray(images, dtype=np.float32)
    C = images.shape[1]
    H, W = (dims[1], dims[2]) if dims is not None else images.shape[2:]
    Hpx, Wpx = height * H + (1 + 5 + 1), width * W
    grid = np.zeros((C, Hpx, Wpx), np.float32)
    for i in range(min(images.shape[0], height * width)):
        y, x = divmod(i, width)
        grid[:, y * H:(y + 1) * H, x * W:(x + 1) * W] = images[i]
    for pos, ch in enumerate(reversed(str(int(epoch))), start=1):
        y0 = Hpx - 1 - 5 - 1                 # 0-based form of yStart = heightPx - 1 - 5
        x0 = Wpx - 1 - pos * 5 - pos - 1     # ... and of xStart = widthPx - 1 - pos*5 - pos
        if x0 < 0:
            break
        grid[:, y0:y0 + 5, x0:x0 + 3] = _glyph(int(ch))
    return grid


def _png_bytes(img):
    """[C,H,W] floats in [0,1] (C = 1 or 3) as an 8-bit PNG (what image.save writes): clamp, x255, round to nearest."""
    C, H, W = img.shape
    assert C in (1, 3)
    px = np.clip(np.rint(np.clip(img, 0.0, 1.0) * 255.0), 0, 255).astype(np.uint8).transpose(1, 2, 0)
    raw = b"".join(b"\x00" + px[y].tobytes() for y in range(H))   # filter type 0 per scan line

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 2 if C == 3 else 0, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b"")


def saveImagesAsGrid(filepath, images, height, width, epoch, dims=None):
    """nn_utils.lua:579-583."""
    grid = imagesToGridTensor(images, height, width, epoch, dims)
    d = os.path.dirname(filepath)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(filepath, "wb") as f:
        f.write(_png_bytes(grid))
    return grid


def rateWithV(S, images):
    """nn_utils.lua:686-711: 1 - mean of V's first output (1 = fake) over the images; V is any module with forward()."""
    V = getattr(S, "MODEL_V", None)
    if V is None:
        return None
    imgs = nn.to_device(np.asarray(images, dtype=np.float32))
    N, bs = imgs.shape[0], S.OPT["batchSize"]
    sm = 0.0
    for a in range(1, N + 1, bs):
        b = min(a + bs - 1, N)
        p = nn.as_plain(V.forward(imgs.rows(a, b))).numpy().reshape(b - a + 1, -1)
        sm += float(p[:, 0].sum())
    return 1.0 - sm / N


def visualizeProgress(S, noiseInputs, trainImages, save_dir, start_time=0, plot_data=None, verbose=False):
    """nn_utils.lua:130-186 without the display server: evaluation mode, the fixed-noise images, the best / worst 50 of them
    according to D (with one real image and one synthetic non-image planted as sanity checks, :133-146), the three PNG
    grids (10x10, 7x7, 7x7) under save_dir/images{,_good,_bad}/<start>_<epoch>.png, V's ratings when S.MODEL_V is set."""
    switchToEvaluationMode(S)
    try:
        train = np.asarray(trainImages, dtype=np.float32)[:50]
        C, H, W = train.shape[1:]
        sanity = np.random.RandomState(S.EPOCH).uniform(0.0, 0.5, size=(C, H, W)).astype(np.float32)   # not S.random: it draws the batches
        for i in range(1, H + 1):               # the reference walks OPT.scale (= the image side) in both directions
            for j in range(1, W + 1):
                if i == j:
                    sanity[0, i - 1, j - 1] = 1.0
                elif i % 4 == 0 and j % 4 == 0:
                    sanity[0, i - 1, j - 1] = 0.5
        rnd = nn.as_nhwc(createImagesFromNoise(S, noiseInputs)).numpy()
        clone = rnd.copy()
        clone[-2] = train[0]
        clone[-1] = sanity
        good, _ = sortImagesByPrediction(S, clone, False, 50)
        bad, _ = sortImagesByPrediction(S, clone, True, 50)
        if np.isnan(rnd).any():
            print("[nn_utils vizProgress] Generated images contain NaNs")
        cs, ep = S.OPT["colorSpace"], S.EPOCH
        out = {}
        for sub, imgs, side in (("images", rnd, 10), ("images_good", good, 7), ("images_bad", bad, 7)):
            path = os.path.join(save_dir, sub, "%d_%05d.png" % (start_time, ep))
            saveImagesAsGrid(path, toRgb(imgs, cs), side, side, ep)
            out[sub] = path
        ratings = [rateWithV(S, x) for x in (rnd, good, bad)]
        if ratings[0] is not None:
            if plot_data is not None:
                plot_data.append([ep] + ratings)
            if verbose:
                print("<nnutils viz> [V] semiRandom: %.4f, goodImages: %.4f, badImages: %.4f" % tuple(ratings))
        out["ratings"] = ratings
        if getattr(S, "EMA", None) is not None:
            # --G_ema: the same fixed noise through the averaged generator (evaluate mode, the live G's running statistics), after
            # everything above so that the three grids and every draw are what they are without the flag
            ema = nn.as_nhwc(createImagesFromNoise(S, noiseInputs, model=S.sync_ema_stats())).numpy()
            path = os.path.join(save_dir, "images_ema", "%d_%05d.png" % (start_time, ep))
            saveImagesAsGrid(path, toRgb(ema, cs), 10, 10, ep)
            out["images_ema"] = path
            out["rating_ema"] = rateWithV(S, ema)
            if out["rating_ema"] is not None and verbose:
                print("<nnutils viz> [V] averaged G (--G_ema): %.4f" % out["rating_ema"])
        return out
    finally:
        switchToTrainingMode(S)


# ------------------------------------------------------------------ sample.lua's helpers
def toDisplayTensor(images, nrow, padding=0):
    """image.toDisplayTensor{input=images, nrow=nrow} as sample.lua:166-168 uses it: `nrow` images PER ROW on a black canvas,
    the whole grid rescaled to [0,1] by its global minimum / maximum (the package's default min-max normalisation; recalled
    upstream behaviour - the image rock is not vendored).  images [n,C,H,W]; returns [C, rows*H, nrow*W]."""
    images = np.asarray(images, dtype=np.float32)
    n, C, H, W = images.shape
    rows = -(-n // nrow)
    grid = np.zeros((C, rows * (H + padding), nrow * (W + padding)), np.float32)
    for i in range(n):
        y, x = divmod(i, nrow)
        grid[:, y * (H + padding):y * (H + padding) + H, x * (W + padding):x * (W + padding) + W] = images[i]
    lo, hi = float(grid.min()), float(grid.max())
    return (grid - lo) / (hi - lo) if hi > lo else np.zeros_like(grid)


def selectRandomImagesFrom(images, n, rs):
    """sample.lua:199-207: the first n entries of a random permutation (torch.randperm -> the given generator)."""
    images = np.asarray(images)
    shuffle = rs.permutation(images.shape[0])
    return images[shuffle[:min(n, images.shape[0])]]


def findClosestNeighboursOf(images, trainingSet):
    """sample.lua:131-151: for every image its nearest training image in the 2-norm; [(image, neighbour, distance)]."""
    train = np.asarray(trainingSet, dtype=np.float32)
    flat = train.reshape(train.shape[0], -1)
    out = []
    for img in np.asarray(images, dtype=np.float32):
        d = np.sqrt(((flat - img.reshape(1, -1)) ** 2).sum(axis=1))
        j = int(np.argmin(d))
        out.append((img, train[j].copy(), float(d[j])))
    return out


# ------------------------------------------------------------------ the same search on the device (cg_nearest_update)
NEAREST_LANES = 64       # partial sums per tile
NEAREST_PER_LANE = 8     # elements each partial adds up, one after the other
NEAREST_TILE = NEAREST_LANES * NEAREST_PER_LANE      # 512 elements of D per tile
NEAREST_TREE = 6         # levels of the binary tree over a tile's 64 partials
NEAREST_MAX_Q = 64


def nearest_chain_length(D):
    """The longest chain of dependent additions in cg_nearest_update's summation order for rows of D elements: the eight of a partial,
    the six levels of the tree, one per tile."""
    return NEAREST_PER_LANE + NEAREST_TREE + -(-int(D) // NEAREST_TILE)


def nearest_d2_np(pool, queries):
    """cg_nearest_update's arithmetic in numpy, bit for bit (include/catgan.h states the order): pool [N][D], queries [Q][D] ->
    float32 [Q][N] of sum_e (pool[n][e] - q[e])^2, every subtraction, multiplication and addition a single fp32 operation.  D is cut into
    tiles of 512 (the last one filled up with zeros on both sides, which contribute +0); partial l of a tile adds the squares of its
    elements l, 64 + l, ... 448 + l in that order; the 64 partials go through a binary tree over adjacent pairs; the tile sums are added
    in tile order."""
    f32 = np.float32
    pool, queries = np.asarray(pool, dtype=f32), np.asarray(queries, dtype=f32)
    pool, queries = pool.reshape(pool.shape[0], -1), queries.reshape(queries.shape[0], -1)
    (N, D), Q = pool.shape, queries.shape[0]
    assert queries.shape[1] == D and D >= 1
    T = -(-D // NEAREST_TILE)
    pad = T * NEAREST_TILE - D
    if pad:
        pool, queries = np.pad(pool, ((0, 0), (0, pad))), np.pad(queries, ((0, 0), (0, pad)))
    out = np.zeros((Q, N), f32)
    for t in range(T):
        sl = slice(t * NEAREST_TILE, (t + 1) * NEAREST_TILE)
        x = pool[:, sl].reshape(N, NEAREST_PER_LANE, NEAREST_LANES)
        for q in range(Q):
            d = x - queries[q, sl].reshape(1, NEAREST_PER_LANE, NEAREST_LANES)
            sq = d * d
            s = np.zeros((N, NEAREST_LANES), f32)
            for j in range(NEAREST_PER_LANE):
                s = s + sq[:, j]
            for _ in range(NEAREST_TREE):
                s = s[:, 0::2] + s[:, 1::2]
            out[q] = out[q] + s[:, 0]
    return out


def nearest_merge_np(best_d2, best_idx, d2, index0):
    """cg_nearest_update's merge rule for one chunk: d2 [Q][N] are the distances to rows index0 .. index0 + N - 1; a candidate replaces
    (best_d2[q], best_idx[q]) if its d2 is smaller, or equal with a smaller index.  Returns the new (best_d2 float32 [Q], best_idx int32
    [Q]); start from nearest_reset_np(Q)."""
    best_d2, best_idx = np.array(best_d2, dtype=np.float32), np.array(best_idx, dtype=np.int32)
    d2 = np.asarray(d2, dtype=np.float32)
    if d2.shape[1] == 0:
        return best_d2, best_idx
    for q in range(d2.shape[0]):
        j = int(np.argmin(d2[q]))      # the first of equal minima = the smallest index of the chunk
        d, i = d2[q, j], int(index0) + j
        if d < best_d2[q] or (d == best_d2[q] and i < best_idx[q]):
            best_d2[q], best_idx[q] = d, i
    return best_d2, best_idx


def nearest_reset_np(Q):
    return np.full(Q, np.inf, np.float32), np.full(Q, -1, np.int32)


class NearestSearch:
    """The running nearest-neighbour search of up to 64 queries on the device.  queries: a host array [Q,C,H,W] (uploaded permuted to
    the pools' NHWC element order) or [Q,D] (taken as it is).  update(pool, index0) merges a chunk of the training set - an engine tensor
    [n,C,H,W] in NHWC memory or a plain [n,D] one, whose first row has the index index0 - on the engine stream without any host
    synchronisation; result() returns (indices int32 [Q], distances float32 [Q] = the fp32 square roots of the best d2)."""

    def __init__(self, queries):
        import torch
        from .tensor import device
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim not in (2, 4) or not 1 <= q.shape[0] <= NEAREST_MAX_Q:
            raise ValueError(f"NearestSearch: queries of shape {q.shape} (1..{NEAREST_MAX_Q} rows, [Q,C,H,W] or [Q,D])")
        self.Q, self.D = q.shape[0], int(np.prod(q.shape[1:]))
        self.queries = Tensor.from_numpy(q)      # 4-D: NHWC memory, as the pools
        self.best_d2 = torch.empty(self.Q, dtype=torch.float32, device=device())
        self.best_idx = torch.empty(self.Q, dtype=torch.int32, device=device())
        self.workspace = None
        self.fresh = True

    def update(self, pool, index0, n=None):
        import torch
        from .tensor import device
        n = pool.shape[0] if n is None else int(n)
        if n > pool.shape[0] or (pool.shape[0] and pool.nElement() // pool.shape[0] != self.D) or pool.ups or \
                (pool.dim() == 4) != (self.queries.dim() == 4) or pool.fmt != self.queries.fmt:
            raise ValueError(f"NearestSearch.update: {n} rows of {pool} against queries {self.queries}")
        need = lib().nearest_workspace_bytes(n, self.Q, self.D)
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.uint8, device=device())
        lib().nearest_update(stream(), pool.ptr, n, self.D, self.queries.ptr, self.Q, int(index0), 1 if self.fresh else 0,
                             self.best_d2.data_ptr(), self.best_idx.data_ptr(), self.workspace.data_ptr())
        self.fresh = False
        return self

    def reset(self):
        self.fresh = True
        return self

    def result(self):
        if self.fresh:      # nothing searched: (+inf, -1)
            self.update(Tensor.empty((0,) + self.queries.shape[1:], self.queries.fmt), 0)
        return self.best_idx.cpu().numpy(), np.sqrt(self.best_d2.cpu().numpy())


def findClosestNeighboursOnDevice(images, loader):
    """findClosestNeighboursOf over a training set that is never held: the pools of a dataset.SequentialLoader pass through
    cg_nearest_update while the next one is decoded and uploaded.  Returns ([(image, neighbour, distance)], indices into loader.files);
    the <= Q winning files are decoded once more on the host (dataset.loadImageFile) instead of keeping pools alive."""
    from . import dataset
    images = np.asarray(images, dtype=np.float32)
    search = NearestSearch(images)
    for pool, index0, n in loader:
        search.update(pool, index0, n)
    idx, dist = search.result()
    if (idx < 0).any():
        raise ValueError("findClosestNeighboursOnDevice: no training row is at a finite distance")
    return [(img, dataset.loadImageFile(loader.files[j]), float(d)) for img, j, d in zip(images, idx, dist)], idx
