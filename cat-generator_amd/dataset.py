"""dataset.lua restated: list + sort the image files of the configured directories
(dataset.lua:57-83), load `count` random ones (torch.randperm, :158-168), image.load them as floats in [0,1] (:166), scale the
FLOAT image to width x height (image.scale, :129-131) and convert the colour space (NN_UTILS.rgbToColorSpace,
nn_utils.lua:223-278: 'rgb', 'y' with weights 0.21/0.72/0.07, 'yuv' and 'hsl' through image.rgb2yuv / image.rgb2hsl [upstream,
recalled: the `image` rock's formulas and constants as lua/image.lua:152-186 restates them]).  PIL only decodes; the scaling is
`image_scale` below - the `image` rock's default separable 'bilinear' [upstream, recalled: box averaging when shrinking, linear
interpolation when enlarging] in fp32, the arithmetic cg_images_u8_scale_to_f32 performs on the device (oracle/oracle.py holds the
independent restatement the tests compare both with; for 'yuv' / 'hsl' the yardstick is fp64 and colorsys,
tests/test_colorspace_host.py).  The result is a float array (in [0,1] except yuv's signed U and V planes) that
adversarial.TrainData uploads to HBM once per epoch (the reference reloads N_epoch images per epoch, train.lua:225).

AsyncLoader is the production form of the same thing: the NEXT epoch's images are decoded by a worker
thread straight into a page-locked buffer as 8-bit RGB at their own size (a quarter of the fp32 bytes over PCIe), copied on a copy
stream while the current epoch trains, scaled and converted on the device (cg_images_u8_scale_to_f32: /255, image.scale, colour
space) into the second of two HBM pools, and handed to the compute stream through an event - no host synchronisation on the
training path.

SequentialLoader is the same pipeline over a given file list, in order, in chunks: one pass over the whole set for the nearest-neighbour
search of sample.py --neighbours (nn_utils.findClosestNeighboursOnDevice), which never holds the set.

setAugmentation turns on the augmentation the reference only has as an offline tool (dataset/generate_dataset.py): both loaders then
draw fresh variants for every epoch pool (augment_images on the host, cg_images_u8_augment_to_f32 on the device, bit-equal).

A directory of PADDED faces (generate_dataset.py --margin M: files of side S + 2 M, and a margin.json that says so) keeps M pixels of
real image around every face.  setDirs reads the margin (dataset.margin; setMargin sets it by hand); every loader then shows the centre
window of a file - the S x S face, byte for byte what a directory of the cropped windows gives - and the augmentation warps it out of the
whole padded file, so that rotated, shifted and zoomed-out variants show real neighbours at their borders instead of replicated edge
pixels (cg_images_u8_augment_window_to_f32 and its gather form serve augmented and un-augmented pools alike).  Margin 0, the default,
changes nothing anywhere.

A pack (buildPack / openPack, written by pack_dataset.py) holds a directory's files decoded once, as 8-bit RGB.  ResidentSet keeps a
pack's pixels in device memory for the whole run and ResidentLoader makes every epoch pool a gather out of it
(cg_images_u8_gather_scale_to_f32 / cg_images_u8_gather_augment_to_f32) on the training stream: the generator's draws and the pixel
arithmetic are loadRandomImages', so the pools are too, and no file is decoded after the pack was built.

The pack file images_u8.cgpack, all integers little endian:
    offset 0   8 bytes   the magic b"CGPACK01" (the last two bytes are the layout's version)
           8   uint64    M, the number of images
          16   uint32    Hs      20  uint32  Ws      24  uint32  3 (channels)      28  uint32  0
          32   uint64    the byte length of the freshness table
          40   uint64    the offset of the pixel block, a multiple of 4096 (so that the block can be memory-mapped)
          48   the freshness table: per file, in loadPaths()' sorted order, uint16 length of the base name, the base name (UTF-8), uint64
               size of the file in bytes, int64 st_mtime_ns - what openPack compares with the directory as it is now
          ...  zeros up to the pixel block: uint8 [M][Hs][Ws][3], image i = _decode(paths[i]); the file ends with it"""
import json
import os
import struct
import threading
import warnings

import numpy as np

dirs = []
fileExtension = ""
height = 32
width = 32
colorSpace = "rgb"
paths = None
_rs = np.random.RandomState(1)
_prefetch_state = None   # AsyncLoader: the generator's state BEFORE the pick of the prefetch that has not been consumed yet
# On-the-fly augmentation (setAugmentation below): off unless asked for; the ranges are generate_dataset.py:68-73's
AUG_DEFAULTS = dict(hflip=True, scale=(0.93, 1.08), rotation=8, translation=4, brightness=0.15, noise_std=0.02)
augmentation = None      # None = off, else a dict with AUG_DEFAULTS' keys
AUG_LDS_BYTES = 160 * 1024   # gfx950's LDS per workgroup: cg_images_u8_augment_to_f32 keeps one source image there as fp32
MARGIN_NAME = "margin.json"  # {"margin": M, "side": S} in a directory of padded faces (generate_dataset.py --margin)
margin = 0                   # pixels of real image around the window that every file of the directories carries


def _read_margin(d):
    """The margin directory d declares in its margin.json; 0 without the file."""
    path = os.path.join(d, MARGIN_NAME)
    if not os.path.isfile(path):
        return 0
    try:
        with open(path) as f:
            m = json.load(f)["margin"]
    except (ValueError, KeyError, TypeError) as e:
        raise ValueError(f"{path}: not a margin file ({type(e).__name__}: {e})") from e
    if isinstance(m, bool) or not isinstance(m, int) or m < 0:
        raise ValueError(f"{path}: margin = {m!r}, expected a whole number >= 0")
    return m


def setDirs(d):
    """The directories of the set; their margin.json files (absent = 0) must agree and give dataset.margin."""
    global dirs, paths, margin
    d = list(d)
    found = {x: _read_margin(x) for x in d}
    if len(set(found.values())) > 1:
        raise ValueError(f"setDirs: the directories disagree about the margin: {found}")
    dirs, paths, margin = d, None, (next(iter(found.values())) if found else 0)


def setMargin(m):
    """The margin by hand (library users whose padded files come without a margin.json); setDirs overwrites it."""
    global margin
    if int(m) < 0:
        raise ValueError(f"setMargin: {m}")
    margin = int(m)


def _window(Hp, Wp, m=None):
    """The window's size inside an Hp x Wp padded image for the margin m (the module's unless given)."""
    m = margin if m is None else int(m)
    if m < 0 or 2 * m >= min(Hp, Wp):
        raise ValueError(f"a margin of {m} leaves no window in a {Wp}x{Hp} image")
    return Hp - 2 * m, Wp - 2 * m


def setFileExtension(ext):
    global fileExtension
    fileExtension = ext


def setHeight(h):
    global height
    height = int(h)


def setWidth(w):
    global width
    width = int(w)


def seed(s):
    global _rs, _prefetch_state
    _rs = np.random.RandomState(s)
    _prefetch_state = None


def checkpoint_state():
    """What a checkpoint must store so that a resumed run loads the pools an uninterrupted one would: AsyncLoader has already
    drawn the NEXT epoch's permutation when an epoch ends, and a resumed loader draws again on construction - so the state to
    restore is the one from before that not-yet-consumed pick (the blocking loader has no pick in flight)."""
    return _prefetch_state if _prefetch_state is not None else _rs.get_state()


def restore_state(state):
    global _prefetch_state
    _rs.set_state(state)
    _prefetch_state = None


def _list(ds_):
    files = []
    for d in ds_:
        for f in os.listdir(d):
            if f.lower().endswith("." + fileExtension.lower()):
                files.append(os.path.join(d, f))
    files.sort()
    return files


def loadPaths():
    """dataset.lua:57-83: every file with the extension in every directory, sorted."""
    global paths
    paths = _list(dirs)
    return paths


COLOR_SPACES = {"rgb": 0, "y": 1, "yuv": 2, "hsl": 3}      # --colorSpace -> the `colorspace` code of include/catgan.h


def rgb2y(im):
    """nn_utils.lua:253-277."""
    return (np.float32(0.21) * im[0] + np.float32(0.72) * im[1] + np.float32(0.07) * im[2])[None].astype(np.float32)


def rgb2yuv(im):
    """image.rgb2yuv [upstream, recalled: the constants and the order of lua/image.lua:152-155] for a float32 [3, H, W] image, every
    operation a single fp32 one (the device form is store_colorspace in csrc/images.hip, same sequence).  U and V are signed."""
    f = np.float32
    r, g, b = (np.asarray(im[k], dtype=f) for k in range(3))
    return np.stack([(f(0.299) * r + f(0.587) * g) + f(0.114) * b,
                     (f(-0.14713) * r - f(0.28886) * g) + f(0.436) * b,
                     (f(0.615) * r - f(0.51499) * g) - f(0.10001) * b]).astype(f)


def rgb2hsl(im):
    """image.rgb2hsl [upstream, recalled: lua/image.lua:159-170] for a float32 [3, H, W] image -> planes h, s, l with h in [0, 1);
    fp32 step by step, the quotients correctly rounded (store_colorspace in csrc/images.hip is the same sequence)."""
    f = np.float32
    r, g, b = (np.asarray(im[k], dtype=f) for k in range(3))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    sm = mx + mn
    l = sm / f(2)
    d = mx - mn
    with np.errstate(divide="ignore", invalid="ignore"):      # the grey pixels (d == 0) are replaced below
        s = np.where(l > f(0.5), d / ((f(2) - mx) - mn), d / sm)
        h = np.where(mx == r, (g - b) / d + np.where(g < b, f(6), f(0)),
                     np.where(mx == g, (b - r) / d + f(2), (r - g) / d + f(4))) / f(6)
    grey = mx == mn
    return np.stack([np.where(grey, f(0), h), np.where(grey, f(0), s), l]).astype(f)


def rgbToColorSpace(images, cs):
    """nn_utils.lua:223-249: 'rgb' as is, 'y' with the reference's own weights, 'yuv' / 'hsl' through image.rgb2yuv / image.rgb2hsl."""
    if cs == "rgb":
        return images
    if cs in ("y", "yuv", "hsl"):
        convert = {"y": rgb2y, "yuv": rgb2yuv, "hsl": rgb2hsl}[cs]
        return np.stack([convert(im) for im in images])
    raise NotImplementedError(f"unknown colour space '{cs}' (rgb | yuv | hsl | y)")


class _Data:
    def __init__(self, scaled):
        self.scaled = scaled

    def size(self):
        return self.scaled.shape[0]

    def __len__(self):
        return self.scaled.shape[0]

    def __getitem__(self, i):
        return self.scaled[i]


def _pick_indices(count):
    """The files of one load as indices into the sorted paths: a fresh permutation, its first `count` entries (dataset.lua:158-163)."""
    if paths is None:
        loadPaths()
    if not paths:
        raise FileNotFoundError(f"no *.{fileExtension} images under {dirs}")
    return _rs.permutation(len(paths))[:min(len(paths), count)]


def _pick(count):
    """The files of one load (the same single draw as _pick_indices)."""
    return [paths[i] for i in _pick_indices(count)]


def pickFiles(count):
    """The files loadRandomImages(count) would load, in its order, consuming the same single draw of the generator: for callers that
    walk the files themselves (sample.py --neighbours streams them through a SequentialLoader)."""
    return _pick(count)


def _prefetch_pick(count):
    """_pick for a load that is consumed one epoch later (AsyncLoader): remembers the generator's state from before the pick,
    which is what a checkpoint taken in between must restore (checkpoint_state)."""
    global _prefetch_state
    _prefetch_state = _rs.get_state()
    return _pick(count)


def _decode(path):
    """One file as 8-bit RGB [H, W, 3] at its own size (what image.load reads before it divides by 255)."""
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)


def _scale_axis(a, Ld):
    """image.scale along the LAST axis of a float32 array [upstream, recalled: generic/image.c scaleLinear_rowcol]: every operation a
    single fp32 one in the loop's order (the device kernel images_u8_scale_k does the same sequence)."""
    f32 = np.float32
    Ls = a.shape[-1]
    if Ld == Ls:
        return a.copy()
    out = np.empty(a.shape[:-1] + (Ld,), f32)
    if Ld > Ls:      # linear interpolation, corner aligned; the last sample is copied
        scale = f32(Ls - 1) / f32(Ld - 1) if Ld > 1 else f32(0)
        for d in range(Ld - 1):
            sf = f32(d) * scale
            si = int(sf)
            sf = f32(sf - f32(si))
            out[..., d] = a[..., 0] if Ls == 1 else (f32(1) - sf) * a[..., si] + sf * a[..., si + 1]
        out[..., Ld - 1] = a[..., Ls - 1]
        return out
    scale = f32(Ls) / f32(Ld)      # box average, fractional ends weighted
    i0, f0 = 0, f32(0)
    for d in range(Ld):
        f1 = f32(d + 1) * scale
        i1 = int(f1)
        f1 = f32(f1 - f32(i1))
        acc = (f32(1) - f0) * a[..., i0]
        n = f32(1) - f0
        for si in range(i0 + 1, i1):
            acc = acc + a[..., si]
            n = f32(n + f32(1))
        if i1 < Ls:
            acc = acc + f1 * a[..., i1]
            n = f32(n + f1)
        out[..., d] = acc / n
        i0, f0 = i1, f1
    return out


def image_scale(img, w, h):
    """image.scale(img, w, h) for a float32 [C, H, W] image: rows to the target width first, then columns to the target height."""
    t = _scale_axis(np.ascontiguousarray(img, dtype=np.float32), w)
    return np.ascontiguousarray(_scale_axis(np.ascontiguousarray(t.transpose(0, 2, 1)), h).transpose(0, 2, 1))


# ---------------------------------------------------------------- augmentation
def setAugmentation(on=True, **ranges):
    """On-the-fly augmentation for both loaders: what the reference ships as an offline tool (dataset/generate_dataset.py:68-73 ->
    Image.augment, dataset/dataset.py:284-306, with the matrices of dataset/ImageAugmenter.py:160-190) that writes nine fixed variants of
    every face to disk, drawn afresh for every epoch pool instead - so --dataDir points at the UN-augmented faces.  Per image: a
    left-right flip with probability 1/2 (`hflip`), a brightness factor ~ U(1-B, 1+B) (`brightness`), noise of deviation `noise_std`,
    clipping to [0, 1], then an affine warp about the image centre (bilinear, edges replicated): zoom ~ U(`scale`) equal on both
    axes, a whole number of degrees in [-`rotation`, `rotation`], whole pixels in [-`translation`, `translation`] on each axis.
    Ranges not named keep AUG_DEFAULTS' values; setAugmentation(False) turns it off again (the default: the loaders then consume the
    generator and compute exactly what they always did).  augment_images holds the arithmetic, cg_images_u8_augment_to_f32 is its
    device form.

    Deliberate differences from the offline tool: no re-quantisation to 8 bits between the stages; the warp acts on the dataset's
    files at the dataset's resolution, not on the full-resolution crop; numpy's seeded generator (dataset.seed) instead of Python's
    `random`; the noise is a bit-reproducible Irwin-Hall normal (augment_noise), not numpy's.  What the warp finds beyond the face
    depends on the set: plain S x S files (margin 0) have none of the tool's padding left, so rotated / shifted borders show replicated
    edge pixels; a padded set (generate_dataset.py --margin M, dataset.margin) keeps M pixels of real image around every face, resized
    with it, and the warp reads those - with AUG_DEFAULTS and S = 64 a margin of 12 is never left (tests/test_augment_margin_host.py),
    a smaller one clamps at its own edge.  The tool's own variants - warped from the padded full-resolution crop and re-quantised
    between the stages - are written offline by generate_dataset.py --variantsFrom crop (faces.variants_np)."""
    global augmentation
    if not on:
        augmentation = None
        return
    unknown = set(ranges) - set(AUG_DEFAULTS)
    if unknown:
        raise TypeError(f"setAugmentation: unknown range(s) {sorted(unknown)} ({' | '.join(AUG_DEFAULTS)})")
    a = dict(AUG_DEFAULTS)
    a.update({k: v for k, v in ranges.items() if v is not None})
    a["scale"] = (float(a["scale"][0]), float(a["scale"][1]))
    a["rotation"], a["translation"] = int(a["rotation"]), int(a["translation"])
    if not (0 < a["scale"][0] <= a["scale"][1] and a["rotation"] >= 0 and a["translation"] >= 0 and 0 <= a["brightness"] < 1 and a["noise_std"] >= 0):
        raise ValueError(f"setAugmentation: bad ranges {a}")
    augmentation = a


def augment_draw(n):
    """The random choices of one pool of n images (create_aug_matrices' and Image.augment's draws, ImageAugmenter.py:160-172,
    dataset.py:284-293) from the loader's own generator: flip [n] 0/1, scale [n], rotation [n] whole degrees, tx / ty [n] whole pixels,
    brightness [n], one 63-bit seed for the pool's noise, and the noise deviation in force (no draw)."""
    a = augmentation if augmentation is not None else AUG_DEFAULTS
    R, T, B = a["rotation"], a["translation"], a["brightness"]
    return dict(flip=_rs.randint(0, 2, size=n) if a["hflip"] else np.zeros(n, np.int64),
                scale=_rs.uniform(a["scale"][0], a["scale"][1], size=n),
                rotation=_rs.randint(-R, R + 1, size=n), tx=_rs.randint(-T, T + 1, size=n), ty=_rs.randint(-T, T + 1, size=n),
                brightness=_rs.uniform(1.0 - B, 1.0 + B, size=n),
                seed=int(_rs.randint(0, 2 ** 63 - 1, dtype=np.int64)), noise_std=float(a["noise_std"]))


def augment_matrix(scale, rotation_deg, tx, ty, Hs, Ws):
    """The 3 x 3 forward matrix of ImageAugmenter.py:174-187 in fp64: to_center . A . to_topleft with the shift int(W/2), int(H/2) and
    A = [[s cos r, -s sin r, tx], [s sin r, s cos r, ty], [0, 0, 1]] (skimage's AffineTransform without shear).  The warp reads the
    source at the INVERSE of it (:190)."""
    r = np.deg2rad(float(rotation_deg))
    sx, sy = int(Ws / 2.0), int(Hs / 2.0)
    A = np.array([[scale * np.cos(r), -scale * np.sin(r), tx], [scale * np.sin(r), scale * np.cos(r), ty], [0, 0, 1]], np.float64)
    to_topleft = np.array([[1, 0, -sx], [0, 1, -sy], [0, 0, 1]], np.float64)
    to_center = np.array([[1, 0, sx], [0, 1, sy], [0, 0, 1]], np.float64)
    return to_center @ A @ to_topleft


def augment_descriptors(n, Hs=64, Ws=64, draw=None):
    """float32 [n, 8], per image (m00 m01 m02 m10 m11 m12 brightness flip): the first two rows of the inverse of augment_matrix (fp64,
    rounded once), the brightness factor and the flip - what cg_images_u8_augment_to_f32 and augment_images read.  draw = an
    augment_draw(n) made earlier (the loaders draw when they pick the files and build the matrix once an image's size is known);
    None draws now."""
    d = augment_draw(n) if draw is None else draw
    desc = np.empty((n, 8), np.float32)
    for i in range(n):
        desc[i] = augment_descriptor(d, i, Hs, Ws)
    return desc


def augment_descriptor(draw, i, Hs, Ws):
    """Row i of augment_descriptors for an image of Hs x Ws pixels."""
    inv = np.linalg.inv(augment_matrix(draw["scale"][i], draw["rotation"][i], draw["tx"][i], draw["ty"][i], Hs, Ws))
    return np.array([inv[0, 0], inv[0, 1], inv[0, 2], inv[1, 0], inv[1, 1], inv[1, 2], draw["brightness"][i], draw["flip"][i]], np.float32)


def augment_noise(seed, offset, j):
    """z for the sample indices j (any integer array): the engine's counter generator (splitmix64 of (seed, counter), tensor.SplitMix)
    at the counters offset + 3 j + {0, 1, 2}; S = the sum of the twelve 16-bit fields of the three outputs; z = (S - 393210) / 65536 as
    fp32.  Irwin-Hall of twelve: the sum of twelve uniform integers on 0..65535 has mean 393210 and deviation 65536 sqrt(1 - 2^-32),
    support +-6; S - 393210 and the division by 2^16 are exact in fp32, so host and device agree bit for bit (a Box-Muller normal would
    need logf / cosf, which are not correctly rounded on the device)."""
    u = np.uint64
    with np.errstate(over="ignore"):
        ctr = u(int(offset) & (2 ** 64 - 1)) + u(3) * np.asarray(j).astype(np.uint64)
        S = np.zeros(ctr.shape, np.int64)
        for k in (1, 2, 3):      # counter + 1: the generator's own convention (SplitMix.u01)
            z = u(int(seed) & (2 ** 64 - 1)) + (ctr + u(k)) * u(0x9E3779B97F4A7C15)
            z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
            z = z ^ (z >> u(31))
            for sh in (0, 16, 32, 48):
                S += ((z >> u(sh)) & u(0xFFFF)).astype(np.int64)
    return (S - 393210).astype(np.float32) / np.float32(65536.0)


def _warp_taps(s, L):
    """One axis of the warp's source positions: clamped to [0, L-1] (NaN -> 0) -> lower tap, upper tap, fraction."""
    f32 = np.float32
    with np.errstate(invalid="ignore"):
        s = np.where(~(s >= f32(0)), f32(0), np.where(s > f32(L - 1), f32(L - 1), s)).astype(f32)
    i0 = s.astype(np.int64)
    return i0, np.minimum(i0 + 1, L - 1), (s - i0.astype(f32)).astype(f32)


def augment_images(u8_batch, desc, noise_std, seed, offset, index0=0, margin=0):
    """The pixel stage and the warp for 8-bit RGB images [N, Hs, Ws, 3] with their descriptors [N, 8] -> float32 [N, 3, Hs, Ws], still
    on the source grid, ready for image_scale / rgbToColorSpace.  Every step is one fp32 operation in this order (the device kernel
    images_u8_augment_k performs the same sequence, so the two agree bit for bit):
      p[y][x][c] = min(max((u8[y][flip ? Ws-1-x : x][c] / 255) * brightness + noise_std * z, 0), 1), z = augment_noise at
                   j = (((index0 + n) Hs + y) Ws + x) 3 + c - index0 + n is the image's index in its pool;
      sx = (m00 x + m01 y) + m02, sy = (m10 x + m11 y) + m12, clamped to the image (edge replication); x0 = floor(sx), fx = sx - x0,
      x1 = min(x0 + 1, Ws-1), likewise y; top = (1-fx) p[y0][x0] + fx p[y0][x1], bot likewise on y1; w[y][x] = (1-fy) top + fy bot.
    An image of another size than its pool's (the loaders' host path) is passed on its own with index0 = its pool index and so
    evaluates j with its OWN Hs, Ws: its counters may overlap a neighbour's, which is accepted - the pool is what either loader gives.
    With margin > 0 the batch holds PADDED images [N, Hp, Wp, 3] and everything above runs on them with Hp, Wp in place of Hs, Ws (the
    flip, the counters j, the clamp, the descriptors' matrix) - but w is evaluated on the window only, at x = margin .. Wp-1-margin,
    y = margin .. Hp-1-margin: float32 [N, 3, Hp - 2 margin, Wp - 2 margin], whose borders show the padding where the warp reaches it."""
    f32 = np.float32
    u8_batch, desc = np.asarray(u8_batch), np.asarray(desc, dtype=f32)
    N, Hs, Ws, _ = u8_batch.shape      # the size the pixel stage and the taps see: the padded one
    Hw, Ww = _window(Hs, Ws, margin)
    sigma = f32(noise_std)
    out = np.empty((N, 3, Hw, Ww), f32)
    xs, ys = np.arange(margin, margin + Ww, dtype=f32)[None, :], np.arange(margin, margin + Hw, dtype=f32)[:, None]
    per = Hs * Ws * 3
    for n in range(N):
        m00, m01, m02, m10, m11, m12, bright, flip = desc[n]
        im = u8_batch[n, :, ::-1] if flip != 0 else u8_batch[n]
        p = (im.astype(f32) / f32(255.0)) * bright
        if sigma != 0:
            j = np.arange(per, dtype=np.uint64).reshape(Hs, Ws, 3) + np.uint64((int(index0) + n) * per)
            p = p + sigma * augment_noise(seed, offset, j)
        p = np.where(p < f32(0), f32(0), p)
        p = np.where(p > f32(1), f32(1), p).astype(f32)
        x0, x1, fx = _warp_taps((m00 * xs + m01 * ys) + m02, Ws)
        y0, y1, fy = _warp_taps((m10 * xs + m11 * ys) + m12, Hs)
        fx, fy = fx[..., None], fy[..., None]
        gx, gy = f32(1) - fx, f32(1) - fy
        top = gx * p[y0, x0] + fx * p[y0, x1]
        bot = gx * p[y1, x0] + fx * p[y1, x1]
        out[n] = (gy * top + fy * bot).transpose(2, 0, 1)
    return out


def _load_scaled(u8, draw=None, i=0):
    """One decoded image -> float32 [3, height, width] in rgb: image.load's floats (or, with a draw, image i of the pool augmented),
    image.scale.  Of a padded image (dataset.margin) it is the window that is loaded, or warped out of the whole."""
    if draw is None:
        if margin:
            Hw, Ww = _window(u8.shape[0], u8.shape[1])
            u8 = u8[margin:margin + Hw, margin:margin + Ww]
        img = u8.astype(np.float32).transpose(2, 0, 1) / np.float32(255.0)      # image.load(path, 3, 'float')
    else:
        desc = augment_descriptor(draw, i, u8.shape[0], u8.shape[1])
        img = augment_images(u8[None], desc[None], draw["noise_std"], draw["seed"], 0, index0=i, margin=margin)[0]
    return image_scale(img, width, height)


def loadImageFile(path):
    """One file through the blocking loader's per-image path (decode, image.load's floats, image.scale, colour space), never augmented:
    float32 [C, height, width], the bits loadRandomImages gives for it."""
    return rgbToColorSpace(_load_scaled(_decode(path))[None], colorSpace)[0]


def loadRandomImages(count):
    """dataset.lua:123-170; with setAugmentation on, every image goes through augment_images first."""
    files = _pick(count)
    draw = augment_draw(len(files)) if augmentation is not None else None
    data = np.empty((len(files), 3, height, width), np.float32)
    for i, f in enumerate(files):
        data[i] = _load_scaled(_decode(f), draw, i)
    return _Data(rgbToColorSpace(data, colorSpace))


def _kernel_limit(Hs, Ws, aug):
    """Why the device kernels cannot serve sources of Hs x Ws pixels (padded ones, with dataset.margin) - (the reason, what the host does
    in their place, a note for those who cannot fall back) - or None: they shrink a window at most 6x (images_u8_scale_k's box loop), and
    the augmentation kernel, which a margin goes through too, keeps one whole source image in the LDS."""
    Hw, Ww = _window(Hs, Ws)
    if Hw > 6 * height or Ww > 6 * width:
        return f"{Ww}x{Hw} sources are more than 6x the {width}x{height} target", "scaling on the host", " (the kernels' limit)"
    if (aug or margin) and Hs * Ws * 12 > AUG_LDS_BYTES:
        return f"{Ws}x{Hs} sources do not fit the augmentation kernel's LDS", "augmenting on the host", ""
    return None


def _pools(count, k):
    """What a loader's pools have in common: the colour space's code (include/catgan.h), its planes C, and k engine tensors
    [count, C, height, width] in NHWC memory."""
    from .tensor import Tensor
    C = 1 if colorSpace == "y" else 3
    return COLOR_SPACES[colorSpace], C, [Tensor.empty((count, C, height, width), "nhwc") for _ in range(k)]


def _to_pool(L, st, src, pool, n, Hs, Ws, m, cs_code, gather=(), desc=None, draw=None):
    """8-bit images on the device -> the first n images of the fp32 pool at `pool`, queued on stream st: the n Hs x Ws images at src or,
    with gather = (M, idx), those of the M at src that the n int32 indices at idx name.  One of the six cg_images_u8_* entry points: with
    a margin m the window form, whose descriptor is null unless augmenting; with a draw (augment_draw's, its descriptors [n][8] at desc)
    alone the augment form; else the scale form."""
    noise_std, nseed = (draw["noise_std"], draw["seed"]) if draw is not None else (0.0, 0)
    form = "gather_" if gather else ""
    if m:
        getattr(L, f"images_u8_{form}augment_window_to_f32")(st, src, *gather, pool, n, Hs, Ws, m, height, width, cs_code,
                                                             desc if draw is not None else None, noise_std, nseed, 0)
    elif draw is not None:
        getattr(L, f"images_u8_{form}augment_to_f32")(st, src, *gather, pool, n, Hs, Ws, height, width, cs_code, desc, noise_std, nseed, 0)
    else:
        getattr(L, f"images_u8_{form}scale_to_f32")(st, src, *gather, pool, n, Hs, Ws, height, width, cs_code)


class _Chunks:
    """Iterating a chunk loader: its next() gives (pool, index0, n), and None once the list is exhausted."""

    def __iter__(self):
        return self

    def __next__(self):
        item = self.next()
        if item is None:
            raise StopIteration
        return item


class AsyncLoader:
    """Double-buffered epoch pools in HBM.  next() returns the pool (an engine tensor [n,C,H,W], NHWC memory) whose upload
    was started one call earlier and immediately starts on the following one: decode (worker thread) -> pinned u8 buffer ->
    cg_memcpy_h2d on the copy stream -> cg_images_u8_to_f32 -> event.  The image choice and the pixel values are exactly
    loadRandomImages' (same generator, same decode, same fp32 operations), so switching loaders does not change a run.  With
    setAugmentation on (read when the loader is built) the pool's draws follow its pick on the caller's thread, the descriptors travel
    with the 8-bit images and cg_images_u8_augment_to_f32 takes the place of the scaling kernel.  With dataset.margin > 0 (read when the
    loader is built, too) the staged images are the padded ones and cg_images_u8_augment_window_to_f32 serves every pool, augmented
    (the descriptors are built for the padded size) or not (no descriptors: its identity form, the scaling kernel's bits for the
    windows)."""

    def __init__(self, count, depth=2):
        if paths is None:
            loadPaths()
        if not paths:
            raise FileNotFoundError(f"no *.{fileExtension} images under {dirs}")
        self._setup(count, depth, paths[0], augmentation is not None)

    def _next_files(self, slot):
        """The files of the pool after the last one started; on the caller's thread: the generator's draws stay in program order."""
        return _prefetch_pick(self.count)

    def _setup(self, count, depth, probe, aug):
        import ctypes
        from .tensor import Tensor, lib
        self._ct, self._T, self.L = ctypes, Tensor, lib()
        self.count, self.depth = int(count), int(depth)
        self.cs_code, self.C, pools = _pools(self.count, self.depth)
        self.Hs, self.Ws = _decode(probe).shape[:2]      # the dataset is written at one size (generate_dataset.py: 64 x 64)
        # The device kernel scales a batch of ONE source size, within _kernel_limit.  The reference (dataset.lua:129-131) scales every
        # image on its own: an image of another size - or all of them, beyond that limit - takes the blocking loader's host path
        # (image_scale, same arithmetic) and is patched into the pool.  With a margin, Hs x Ws is the padded size.
        self.margin, self.aug = margin, aug
        limit = _kernel_limit(self.Hs, self.Ws, aug)
        self.host_all = limit is not None
        if limit:
            warnings.warn(f"{type(self).__name__}: {limit[0]}: {limit[1]}")
        # host_all: nothing is scaled on the device, so no 8-bit staging / device buffer of the (large) SOURCE size exists at all - the
        # worker writes the finished fp32 NHWC rows into a pinned buffer of the POOL's size and one asynchronous copy moves them
        # (the u8 path would pin count x Hs x Ws x 3 bytes per slot for images it never uploads).  Otherwise: the u8
        # staging, plus a pinned fp32 side buffer of the pool's size for the odd-sized images that take the host path.
        self.row = height * width * self.C * 4
        self.nbytes = self.count * self.row if self.host_all else self.count * self.Hs * self.Ws * 3
        self.copy_stream = ctypes.c_void_p()
        self.L.stream_create(ctypes.byref(self.copy_stream))
        self.slots = []
        f32p = ctypes.POINTER(ctypes.c_float)
        for pool in pools:
            host, dev_u8, ev_ready, ev_free, side = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
            host_desc, dev_desc, desc = ctypes.c_void_p(), ctypes.c_void_p(), None
            self.L.host_alloc(ctypes.byref(host), self.nbytes)
            self.L.event_create(ctypes.byref(ev_ready)); self.L.event_create(ctypes.byref(ev_free))
            if self.host_all:
                staging = np.ctypeslib.as_array(ctypes.cast(host, f32p), shape=(self.count, height, width, self.C))
                patch = None
            else:
                self.L.malloc(ctypes.byref(dev_u8), self.nbytes)
                staging = np.ctypeslib.as_array(ctypes.cast(host, ctypes.POINTER(ctypes.c_uint8)), shape=(self.count, self.Hs, self.Ws, 3))
                self.L.host_alloc(ctypes.byref(side), self.count * self.row)
                patch = np.ctypeslib.as_array(ctypes.cast(side, f32p), shape=(self.count, height, width, self.C))
                if self.aug:      # the descriptors ride with the 8-bit batch: pinned on the host, eight floats per image on the device
                    self.L.host_alloc(ctypes.byref(host_desc), self.count * 32)
                    self.L.malloc(ctypes.byref(dev_desc), self.count * 32)
                    desc = np.ctypeslib.as_array(ctypes.cast(host_desc, f32p), shape=(self.count, 8))
            self.slots.append(dict(host=host, staging=staging, dev_u8=dev_u8, side=side, patch=patch, ready=ev_ready, free=ev_free, pool=pool,
                                   host_desc=host_desc, dev_desc=dev_desc, desc=desc, n=0, used=False))
        self.k = 0
        self._thread = None
        self._err = None
        self._start(self.slots[0])

    def _start(self, slot):
        files = self._next_files(slot)
        slot["n"] = len(files)
        draw = slot["draw"] = augment_draw(len(files)) if self.aug else None      # likewise, right after the pick (as loadRandomImages)
        if slot["used"]:
            self.L.event_sync(slot["ready"])   # its previous upload has left the pinned buffers (long ago; costs nothing)

        slot["patches"] = []

        def work():
            try:
                for i, f in enumerate(files):
                    im = _decode(f)
                    if self.host_all or im.shape[:2] != (self.Hs, self.Ws):
                        # loadRandomImages' arithmetic for this one image: /255 (or its augmentation, with the matrix of its own
                        # size) -> image.scale -> colour space, as NHWC rows
                        img = rgbToColorSpace(_load_scaled(im, draw, i)[None], colorSpace)[0].transpose(1, 2, 0)
                        if self.host_all:
                            slot["staging"][i] = img
                        else:
                            slot["patch"][i] = img         # pinned: the copy below needs no synchronisation
                            slot["patches"].append(i)
                            slot["staging"][i] = 0
                            if draw is not None:
                                slot["desc"][i] = (1, 0, 0, 0, 1, 0, 1, 0)      # the kernel's output for this row is overwritten
                    else:
                        slot["staging"][i] = im
                        if draw is not None:
                            slot["desc"][i] = augment_descriptor(draw, i, self.Hs, self.Ws)
            except Exception as e:   # surfaced by next()
                self._err = e
        self._thread = threading.Thread(target=work, daemon=True)
        self._thread.start()

    def _upload(self, slot):
        L, cs, n = self.L, self.copy_stream, slot["n"]
        if slot["used"]:
            L.stream_wait_event(cs, slot["free"])      # the training stream has finished reading this pool
        if self.host_all:
            L.memcpy_h2d(cs, slot["pool"].ptr, slot["host"], n * self.row)
        else:
            L.memcpy_h2d(cs, slot["dev_u8"], slot["host"], n * self.Hs * self.Ws * 3)
            if self.aug:
                L.memcpy_h2d(cs, slot["dev_desc"], slot["host_desc"], n * 32)
            _to_pool(L, cs, slot["dev_u8"], slot["pool"].ptr, n, self.Hs, self.Ws, self.margin, self.cs_code, desc=slot["dev_desc"], draw=slot["draw"])
            for i in slot["patches"]:     # images scaled on the host (another source size): over the rows the kernel produced from zeros
                L.memcpy_h2d(cs, slot["pool"].ptr + i * self.row, slot["side"].value + i * self.row, self.row)
            slot["patches"] = []
        L.event_record(slot["ready"], cs)

    def next(self):
        from .tensor import stream
        slot = self.slots[self.k]
        self._thread.join()
        if self._err is not None:
            raise self._err
        self._upload(slot)
        prev = self.slots[(self.k - 1) % self.depth]
        if prev["used"]:
            self.L.event_record(prev["free"], stream())   # everything queued so far on the training stream may still read `prev`
        self.L.stream_wait_event(stream(), slot["ready"])
        slot["used"] = True
        self.k = (self.k + 1) % self.depth
        self._start(self.slots[self.k])                     # decode the following epoch while this one trains
        pool = slot["pool"]
        return pool if slot["n"] == self.count else pool.rows(1, slot["n"])

    def close(self):
        global _prefetch_state
        _prefetch_state = None             # the pending pick dies with the loader
        self._release()

    def _release(self):
        if self._thread is not None:
            self._thread.join()
        self.L.stream_sync(self.copy_stream)
        for s_ in self.slots:
            self.L.host_free(s_["host"])
            if s_["dev_u8"]:
                self.L.free(s_["dev_u8"])
            if s_["side"]:
                self.L.host_free(s_["side"])
            if s_["host_desc"]:
                self.L.host_free(s_["host_desc"]); self.L.free(s_["dev_desc"])
            self.L.event_destroy(s_["ready"]); self.L.event_destroy(s_["free"])
        self.L.stream_destroy(self.copy_stream)
        self.slots = []


class SequentialLoader(_Chunks, AsyncLoader):
    """AsyncLoader's pipeline (worker decode -> pinned 8-bit buffer -> copy stream -> cg_images_u8_scale_to_f32 -> event, two pools) over
    a GIVEN file list, in that order, `chunk` files at a time: what a pass over the whole training set needs (sample.py --neighbours,
    nn_utils.findClosestNeighboursOnDevice) without ever holding the set.  next() returns (pool, index0, n) - the engine tensor
    [n,C,H,W] (NHWC memory) of files[index0 : index0 + n] - and None once the list is exhausted; iterating the loader does the same.  A
    pool stays valid until the next-but-one next().  The generator is never touched and augmentation never applied: the search is over
    the set as it is on disk, pixel for pixel what loadRandomImages gives for the same files (odd-sized sources and the more-than-6x
    shrink case take AsyncLoader's host path)."""

    def __init__(self, files, chunk, depth=2):
        self.files = list(files)
        if not self.files:
            raise FileNotFoundError("SequentialLoader: an empty file list")
        if int(chunk) < 1:
            raise ValueError(f"SequentialLoader: chunk = {chunk}")
        self._pos = 0
        self._setup(min(int(chunk), len(self.files)), depth, self.files[0], False)

    def _next_files(self, slot):
        slot["index0"] = self._pos
        files = self.files[self._pos:self._pos + self.count]
        self._pos += len(files)
        return files

    def next(self):
        slot = self.slots[self.k]
        if slot["n"] == 0:      # the list is exhausted (its worker had nothing to do)
            return None
        index0, n = slot["index0"], slot["n"]
        return AsyncLoader.next(self), index0, n

    def close(self):
        self._release()


# ---------------------------------------------------------------- the decoded set, packed on disk and resident on the device
PACK_NAME = "images_u8.cgpack"
PACK_MAGIC = b"CGPACK01"
_PACK_HEAD = struct.Struct("<8sQIIIIQQ")      # magic, M, Hs, Ws, channels, 0, table bytes, pixel offset
PACK_MAX_THREADS = 16


def packPath(d):
    return os.path.join(d, PACK_NAME)


def _freshness(files):
    """The table of the pack's header for these files as they are on disk now."""
    out = []
    for f in files:
        st = os.stat(f)
        name = os.path.basename(f).encode("utf-8")
        out.append(struct.pack("<H", len(name)) + name + struct.pack("<Qq", st.st_size, st.st_mtime_ns))
    return b"".join(out)


def buildPack(d, threads=8):
    """Decode every file loadPaths() lists for directory d (sorted; _decode) into d/images_u8.cgpack, image i = paths[i].  `threads`
    workers (at most PACK_MAX_THREADS) each write the slots of their own images, so the file does not depend on their number; it appears
    under its name only once it is complete (os.replace).  Every file must have the first one's size: a directory of mixed sizes stays
    with the file loaders, and the error names the files that differ.  Returns (path, M)."""
    files = _list([d])
    if not files:
        raise FileNotFoundError(f"no *.{fileExtension} images under {d}")
    threads = max(1, min(int(threads), PACK_MAX_THREADS))
    table = _freshness(files)
    first = _decode(files[0])
    Hs, Ws = first.shape[:2]
    M = len(files)
    offset = -(-(_PACK_HEAD.size + len(table)) // 4096) * 4096
    tmp = packPath(d) + ".tmp%d" % os.getpid()
    try:
        with open(tmp, "wb") as f:
            f.write(_PACK_HEAD.pack(PACK_MAGIC, M, Hs, Ws, 3, 0, len(table), offset))
            f.write(table)
            f.truncate(offset + M * Hs * Ws * 3)
        px = np.memmap(tmp, dtype=np.uint8, mode="r+", offset=offset, shape=(M, Hs, Ws, 3))
        odd = []

        def work(a):      # a run of consecutive images per task: a 64 x 64 decode is too short to be a task of its own
            for i in range(a, min(a + 64, M)):
                im = first if i == 0 else _decode(files[i])
                if im.shape != (Hs, Ws, 3):
                    odd.append((i, "%s (%dx%d)" % (files[i], im.shape[1], im.shape[0])))
                else:
                    px[i] = im
        if threads == 1:
            for a in range(0, M, 64):
                work(a)
        else:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=threads) as ex:
                list(ex.map(work, range(0, M, 64)))
        if odd:
            names = ", ".join(n for _, n in sorted(odd)[:8]) + (" ..." if len(odd) > 8 else "")
            raise ValueError(f"buildPack: {len(odd)} file(s) are not {Ws}x{Hs} like {files[0]}: {names} - a pack holds one source size")
        px.flush()
        del px
        os.replace(tmp, packPath(d))
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return packPath(d), M


class Pack:
    """An open pack: M images of Hs x Ws, `pixels` the memory-mapped uint8 [M][Hs][Ws][3] block, `paths` the files they were decoded from
    (paths[i] -> pixels[i])."""

    def __init__(self, path, files, pixels):
        self.path, self.paths, self.pixels = path, files, pixels
        self.M, self.Hs, self.Ws = pixels.shape[:3]


def openPack(d):
    """The pack of directory d, mapped, if it describes the directory as it is now - else None after one warning that says why (no pack
    file; a foreign magic; a truncated file; the files listed now differ from the freshness table in name, size or modification time).
    A stale or damaged pack is never an error and never used: the file loaders serve the directory as before."""
    path = packPath(d)

    def refuse(why):
        warnings.warn(f"{path}: {why} - not used (pack_dataset.py --dataDir {d} writes a fresh one)")
        return None
    if not os.path.isfile(path):
        return refuse("no such file")
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(_PACK_HEAD.size)
        if len(head) < _PACK_HEAD.size or head[:8] != PACK_MAGIC:
            return refuse("not a pack of this version (magic %r)" % head[:8])
        _, M, Hs, Ws, C, _, tbytes, offset = _PACK_HEAD.unpack(head)
        if C != 3 or M < 1 or Hs < 1 or Ws < 1 or offset % 4096 or offset < _PACK_HEAD.size + tbytes:
            return refuse("a damaged header")
        if size != offset + M * Hs * Ws * 3:
            return refuse("truncated (%d bytes, the header promises %d)" % (size, offset + M * Hs * Ws * 3))
        table = f.read(tbytes)
    files = _list([d])
    if len(files) != M:
        return refuse("stale: it holds %d images, the directory %d" % (M, len(files)))
    if table != _freshness(files):
        return refuse("stale: a file was renamed, rewritten or touched since it was built")
    return Pack(path, files, np.memmap(path, dtype=np.uint8, mode="r", offset=offset, shape=(M, Hs, Ws, 3)))


def _check_resident(who, Hs, Ws, aug):
    """A resident set has no host path: what _kernel_limit names is an error."""
    limit = _kernel_limit(Hs, Ws, aug)
    if limit:
        raise ValueError(f"{who}: {limit[0]}{limit[2]}")


class ResidentSet:
    """A pack's pixel block in device memory, uploaded once: uint8 [M][Hs][Ws][3] at `ptr`.  The buffer belongs to this object (close(), or
    its collection, frees it).  An allocation that fails raises (CatganError) before anything is kept: the caller falls back."""

    UPLOAD_BYTES = 64 << 20

    def __init__(self, pack):
        import ctypes
        from .tensor import lib, stream
        self.L, self.paths = lib(), list(pack.paths)
        self.M, self.Hs, self.Ws = int(pack.M), int(pack.Hs), int(pack.Ws)
        self.per = self.Hs * self.Ws * 3
        self.nbytes = self.M * self.per
        dev = ctypes.c_void_p()
        self.ptr = None
        self.L.malloc(ctypes.byref(dev), self.nbytes)
        self.ptr = dev.value
        step = max(1, self.UPLOAD_BYTES // self.per)
        try:
            for a in range(0, self.M, step):      # pageable memory: each piece has left the host when its copy is synchronised
                part = np.ascontiguousarray(pack.pixels[a:a + step])
                self.L.memcpy_h2d(stream(), self.ptr + a * self.per, part.ctypes.data, part.nbytes)
                self.L.stream_sync(stream())
        except Exception:
            self.close()
            raise

    def chunks(self, chunk):
        """SequentialLoader's contract over the resident set, in the set's (sorted-file) order: an iterable of (pool, index0, n) whose
        `files` are the set's paths.  Never augmented, the generator never touched."""
        return _ResidentChunks(self, chunk)

    def close(self):
        if self.ptr is not None:
            self.L.free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _ResidentChunks(_Chunks):
    """cg_images_u8_scale_to_f32 (of a padded set, dataset.margin: cg_images_u8_augment_window_to_f32's identity form) on consecutive
    slices of a ResidentSet, on the caller's stream, alternating two pools: a pool stays valid until the next-but-one next()."""

    def __init__(self, rset, chunk):
        if int(chunk) < 1:
            raise ValueError(f"ResidentSet.chunks: chunk = {chunk}")
        _check_resident("ResidentSet.chunks", rset.Hs, rset.Ws, False)
        self.set, self.files, self.count, self.margin = rset, rset.paths, min(int(chunk), rset.M), margin
        self.cs_code, self.C, self.pools = _pools(self.count, 2)
        self._pos, self.k = 0, 0

    def next(self):
        from .tensor import stream
        s = self.set
        if self._pos >= s.M:
            return None
        index0, n = self._pos, min(self.count, s.M - self._pos)
        pool = self.pools[self.k]
        _to_pool(s.L, stream(), s.ptr + index0 * s.per, pool.ptr, n, s.Hs, s.Ws, self.margin, self.cs_code)
        self._pos += n
        self.k ^= 1
        return (pool if n == self.count else pool.rows(1, n)), index0, n

    def close(self):
        self.pools = []


class ResidentLoader:
    """Epoch pools gathered out of a ResidentSet.  next() draws what loadRandomImages(count) draws from the module's generator, in its
    order (the permutation, then - with setAugmentation on when the loader was built - the pool's augment_draw), stages the indices and
    the descriptors in page-locked memory, and queues their copies and ONE gather kernel on the training stream: the pool (an engine
    tensor [n,C,H,W], NHWC memory, as AsyncLoader.next() returns) is ready wherever that stream reads it, and stream order is the only
    synchronisation - no copy stream, no thread, no prefetch.  So there is never a pick in flight and checkpoint_state() is the blocking
    loader's.  The staging is rewritten one epoch later, after the event recorded behind its copies; two pools alternate, each valid
    until the next-but-one next().  A set the kernels cannot serve (more than 6x larger than the target; with augmentation, beyond the
    LDS) is a ValueError here, and the paths of the set must be the module's.  A padded set (dataset.margin when the loader is built; the
    pack stores the padded size as it always stored the files') goes through cg_images_u8_gather_augment_window_to_f32, augmented or
    not."""

    def __init__(self, count, resident_set):
        import ctypes
        from .tensor import lib
        s = self.set = resident_set
        self.aug, self.margin = augmentation is not None, margin
        _check_resident(type(self).__name__, s.Hs, s.Ws, self.aug)
        if (paths if paths is not None else loadPaths()) != s.paths:
            raise ValueError(f"{type(self).__name__}: the resident set does not hold the files of {dirs}")
        self.L, self.count = lib(), int(count)
        n = min(self.count, s.M)
        self.cs_code, self.C, self.pools = _pools(n, 2)
        self.k, self.used = 0, False
        # indices [n] int32, then descriptors [n][8] float32: one page-locked block, one device block
        self.host, self.dev, self.staged = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self.L.host_alloc(ctypes.byref(self.host), n * 36)
        self.L.malloc(ctypes.byref(self.dev), n * 36)
        self.L.event_create(ctypes.byref(self.staged))
        self.idx = np.ctypeslib.as_array(ctypes.cast(self.host, ctypes.POINTER(ctypes.c_int32)), shape=(n,))
        self.desc = np.ctypeslib.as_array(ctypes.cast(ctypes.c_void_p(self.host.value + n * 4), ctypes.POINTER(ctypes.c_float)), shape=(n, 8))

    def next(self):
        from .tensor import stream
        L, s, st = self.L, self.set, stream()
        pick = _pick_indices(self.count)
        n = len(pick)
        draw = augment_draw(n) if self.aug else None      # right after the pick, as loadRandomImages
        if self.used:
            L.event_sync(self.staged)      # last epoch's copies have left the staging (long ago)
        self.idx[:n] = pick
        if self.aug:
            for i in range(n):
                self.desc[i] = augment_descriptor(draw, i, s.Hs, s.Ws)
        L.memcpy_h2d(st, self.dev.value, self.host.value, n * 4)
        if self.aug:
            L.memcpy_h2d(st, self.dev.value + len(self.idx) * 4, self.host.value + len(self.idx) * 4, n * 32)
        L.event_record(self.staged, st)
        self.used = True
        pool = self.pools[self.k]
        self.k ^= 1
        _to_pool(L, st, s.ptr, pool.ptr, n, s.Hs, s.Ws, self.margin, self.cs_code, gather=(s.M, self.dev.value),
                 desc=self.dev.value + len(self.idx) * 4, draw=draw)
        return pool if n == pool.shape[0] else pool.rows(1, n)

    def close(self):
        if self.host:
            if self.used:
                self.L.event_sync(self.staged)
            self.L.host_free(self.host); self.L.free(self.dev); self.L.event_destroy(self.staged)
            self.host = self.dev = self.staged = None
            self.pools = []
