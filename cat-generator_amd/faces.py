"""The reference's offline dataset tool restated for its un-augmented face (dataset/generate_dataset.py:53-91 over
dataset/dataset.py): from a decoded cat image and the nine keypoints of its .cat file to the out x out 8-bit face.  Four stages:

  1. keypoints (dataset.py:84-92): the first field of the .cat line is the count, then nine (x, y) pairs read as abs(int) and
     clipped into the image, kept as (y, x)                                                                     parse_cat
  2. rotation removal (:152-181): the angle of the eye line against the x axis (:489-508, :943-967); the forward map
     F(p) = R(-angle)(p - eyes_centre) + image_centre with both centres int()-truncated; the image is
     tf.warp(image, F^-1, mode="nearest") at the source size (order 1, edge replication), re-quantised by truncation (:174); every
     keypoint is drawn as one white pixel, warped with order 1 and constant mode, and moved to the arg-max (:777-796)
                                                                                     eye_angle, rotation_maps, move_keypoints, warp_rect_np
  3. face rectangle, method 4 (:602-676, Rectangle.square :853-910): the bounding box of the nine points, shifted half-way to the
     face centre (eyes and mouth, truncated thirds), the bounding box of both clipped to the image, squared by removing rows or
     columns (the extra one off the top / left); the crop is inclusive, (br - tl + 1)^2 pixels (:217)                       face_rectangle
  4. resize (:127-139): misc.imresize(face, (out, out)) = Pillow's Image.resize(..., BILINEAR)                   resize_taps, resize_np

extract_face(pad=30)'s padding (the median np.pad, :191-230) and unpad(30) (:145-150) cancel exactly for this variant - the margin is
`pad` on every side in every case of extract_rectangle - so neither appears here.  face_geometry chains 1-3's host decisions,
extract_faces_np the whole pipeline: it is the yardstick of the device form, cg_faces_u8_extract (csrc/faces.hip), which
extract_faces_device calls.  Host decisions are fp64 (Python floats); only pixels are computed in fp32 and integers.

For the tool's AUGMENTED variants (generate_dataset.py:62-73, Image.augment, dataset.py:284-308) the padding does not cancel: the
reference keeps `pad` pixels of real image around the rectangle "for the augmentation" (:62-64), warps at full resolution and only
then unpads and resizes, so its rotated, shifted and zoomed-out variants show fur and background at their borders.  Four stages
between 3 and 4, per accepted face (generate_dataset.py --variantsFrom crop; the default, face, warps the finished face instead):

  a. padded crop P, [Hr + 2 pad, Wr + 2 pad, 3] (extract_rectangle, :191-230): the rectangle enlarged by `pad` and clipped to the image
     (:196-204) out of stage 2's warp, then np.pad(mode="median") for the sides that left it (:206-228)        padded_crop_np, median_pad_np
  b. pixel stage on the flipped crop (:284-304): brightness, noise, clip - and the re-quantisation to 8 bits that the tool performs
     between its stages and that the on-the-fly form (dataset.augment_images) deliberately leaves out             variant_pixels_np
  c. warp (:306-307) by the inverse of ImageAugmenter's matrix (ImageAugmenter.py:111-112, 179-190) with the shifts int(Wp / 2),
     int(Hp / 2) of the PADDED crop, clamped to the padded crop, re-quantised by truncation; evaluated on the window
     [pad, pad + Hr) x [pad, pad + Wr) only - the warp is pointwise, so this equals warping all of it and unpad(pad) (:145-150)
                                                                                                                  variant_warp_np
  d. resize, stage 4 unchanged.
variants_np chains a-d and is the yardstick of cg_faces_u8_extract_variants, which extract_variants_device calls.  The draws are
dataset.augment_draw's (numpy's seeded generator, not the reference's `random` stream), the noise dataset.augment_noise at the counters
base + 3 j, j = (y Wp + x) 3 + c on the array the warp reads, `base` one 64-bit number per (face, variant) that the caller passes as
data.  Three exact consequences (tests/test_faces_variants_host.py): the identity draw returns the _000 rectangle; a whole-pixel shift
alone returns stage 2's warp of the rectangle shifted the other way - real neighbouring pixels; a flip alone returns the mirror.

The PADDED face of generate_dataset.py --margin is stage a with a pad of the face's own (margin_pad) through stage 4 as a whole, with
nothing in between: padded_face_np, the yardstick of cg_faces_u8_extract_padded, which extract_padded_device calls.

The keypoint move is written as a closed search instead of a warp of a whole image per point: a white pixel at p reaches output pixel q
with the weight max(0, 1 - |sx - px|) max(0, 1 - |sy - py|), (sx, sy) = F^-1(q), which is zero outside the rotated unit square around
F(p); that square lies within 1.92 pixels per axis of round(F(p)), so a 5 x 5 window holds every non-zero weight.  The first maximum
in raster order wins, and the reference's rule for "not found" is kept (:789: the arg-max is pixel 0 with less than 0.5 there - which
every weight being zero implies - leaves the keypoint unchanged).

Era- and library-dependent assumptions (in the sense of the table at the top of oracle/oracle.py), with the tests that hold our form:
  * skimage's warp computes in double; ours is the project's fp32 restatement of tf.warp (p = u8 / 255,
    sx = (m00 x + m01 y) + m02 with the six inverse entries rounded to fp32, clamp with NaN -> 0, taps x0 = (int)sx and
    x1 = min(x0 + 1, W - 1), the four-term blend of dataset.augment_images, q = (u8)(w 255) truncated), every operation a single
    correctly rounded fp32 one.  Held by tests/test_faces_host.py::test_level_eyes_chain_equals_shift_crop_and_pillow (where the two
    agree exactly) and tests/test_gpu_faces.py::test_kernel_equals_the_host_restatement_bit_for_bit.
  * the resize is the 8-bit resampling of the Pillow that is installed today (Resample.c: coefficients normalised in double, taps
    int(0.5 + w 2^22), a horizontal pass into 8 bits and then a vertical one, each clip8((2^21 + sum pixel k) >> 22)); the reference's
    Pillow of 2016 may have rounded differently.  Held by tests/test_faces_host.py::test_resize_stage_equals_pillow_bit_for_bit.
  * np.pad(mode="median") is written out (median_pad_np): axis 0 first, then axis 1 over all rows, the median of an even number of bytes
    being the mean of the two middle ones rounded half to even.  That is the numpy installed today (2.2: np.median's mean in double,
    then ndarray.round); the numpy of 2016 is recalled to behave the same.  Held by
    tests/test_faces_variants_host.py::test_median_fill_equals_numpy_pad.
"""
import math

import numpy as np

KSEARCH = 2   # the keypoint move looks at round(F(p)) +- 2


# ---------------------------------------------------------------- 1. keypoints
def parse_cat(text, H, W):
    """The first line of a .cat file -> int array [9, 2] of (y, x) (dataset.py:84-92), or None when it holds fewer than nine points."""
    lines = text.splitlines()
    raw = lines[0].split() if lines else []
    try:
        vals = [abs(int(v)) for v in raw]
    except ValueError:
        return None
    if len(vals) < 19:
        return None
    kp = np.empty((9, 2), np.int64)
    for i in range(9):
        kp[i, 0] = min(max(vals[2 + 2 * i], 0), H - 1)
        kp[i, 1] = min(max(vals[1 + 2 * i], 0), W - 1)
    return kp


# ---------------------------------------------------------------- 2. rotation removal
def eye_angle(kp):
    """Radians between the x axis and the line from the left eye (point 0) to the right eye (point 1), negative when the right eye is
    higher (dataset.py:489-508 through angle_between, :943-967); None when both eyes are on one pixel (the reference divides by zero)."""
    ey, ex = int(kp[1, 0]) - int(kp[0, 0]), int(kp[1, 1]) - int(kp[0, 1])
    n = math.hypot(ex, ey)
    if n == 0:
        return None
    v = math.acos(min(1.0, max(-1.0, ex / n)))
    return -v if ey < 0 else v


def rotation_maps(kp, H, W):
    """(F, F^-1) as 3 x 3 fp64 matrices in (x, y) coordinates (dataset.py:154-170): to the eyes' centre, rotate by -angle, to the image
    centre; the warp reads the source at F^-1 of an output position."""
    a = eye_angle(kp)
    ecx, ecy = int((int(kp[0, 1]) + int(kp[1, 1])) / 2), int((int(kp[0, 0]) + int(kp[1, 0])) / 2)
    icx, icy = int(W / 2), int(H / 2)
    c, s = math.cos(-a), math.sin(-a)
    to_topleft = np.array([[1, 0, -ecx], [0, 1, -ecy], [0, 0, 1]], np.float64)
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)
    to_center = np.array([[1, 0, icx], [0, 1, icy], [0, 0, 1]], np.float64)
    F = to_center @ rot @ to_topleft
    return F, np.linalg.inv(F)


def move_keypoints(kp, F, Finv, H, W):
    """Every keypoint to the arg-max of its warped white pixel (dataset.py:769-796), by the closed search of the module docstring."""
    out = np.array(kp, np.int64)
    for i in range(len(kp)):
        py, px = int(kp[i, 0]), int(kp[i, 1])
        cx = int(math.floor(F[0, 0] * px + F[0, 1] * py + F[0, 2] + 0.5))
        cy = int(math.floor(F[1, 0] * px + F[1, 1] * py + F[1, 2] + 0.5))
        best, by, bx = 0.0, -1, -1
        for y in range(max(cy - KSEARCH, 0), min(cy + KSEARCH, H - 1) + 1):         # raster order: the first maximum wins
            for x in range(max(cx - KSEARCH, 0), min(cx + KSEARCH, W - 1) + 1):
                sx = Finv[0, 0] * x + Finv[0, 1] * y + Finv[0, 2]
                sy = Finv[1, 0] * x + Finv[1, 1] * y + Finv[1, 2]
                w = max(0.0, 1.0 - abs(sx - px)) * max(0.0, 1.0 - abs(sy - py))
                if w > best:
                    best, by, bx = w, y, x
        if by < 0 or (by == 0 and bx == 0 and best < 0.5):
            continue
        out[i] = (by, bx)
    return out


# ---------------------------------------------------------------- 3. rectangle
def _rect(tl_y, tl_x, br_y, br_x):
    """Rectangle.__init__'s assertions (dataset.py:823-824) as a value: None where the reference stops."""
    if min(tl_y, tl_x, br_y, br_x) < 0 or not (tl_y < br_y and tl_x < br_x):
        return None
    return [int(tl_y), int(tl_x), int(br_y), int(br_x)]


def face_rectangle(kp, H, W):
    """Method 4 (dataset.py:602-676) -> (tl_y, tl_x, br_y, br_x), corners inclusive, or None when one of the rectangles on the way is
    degenerate.  Divisions are true divisions truncated by int(), as the reference's `from __future__ import division` makes them."""
    ys, xs = [int(v) for v in kp[:, 0]], [int(v) for v in kp[:, 1]]
    r0 = _rect(min(ys), min(xs), max(ys), max(xs))
    if r0 is None:
        return None
    fcy, fcx = int((ys[0] + ys[1] + ys[2]) / 3), int((xs[0] + xs[1] + xs[2]) / 3)             # eyes and mouth (:476-481)
    rcy, rcx = int(r0[0] + (r0[2] - r0[0]) / 2), int(r0[1] + (r0[3] - r0[1]) / 2)             # Rectangle.get_center (:844-851)
    dy, dx = fcy - rcy, fcx - rcx
    r2 = _rect(int(max(0, r0[0] + dy / 2)), int(max(0, r0[1] + dx / 2)), int(min(H - 1, r0[2] + dy / 2)), int(min(W - 1, r0[3] + dx / 2)))
    if r2 is None:
        return None
    r3 = _rect(max(0, min(r0[0], r2[0])), max(0, min(r0[1], r2[1])), min(H - 1, max(r0[2], r2[2])), min(W - 1, max(r0[3], r2[3])))
    if r3 is None:
        return None
    tl_y, tl_x, br_y, br_x = r3
    h, w = br_y - tl_y, br_x - tl_x
    if h > w:                                  # Rectangle.square (:895-910): the odd row comes off the top
        d = h - w
        tl_y += d // 2 + d % 2
        br_y -= d // 2
    elif w > h:
        d = w - h
        tl_x += d // 2 + d % 2
        br_x -= d // 2
    return tl_y, tl_x, br_y, br_x


def face_geometry(kp, H, W):
    """Stages 2 and 3's host decisions for one image -> dict(inv: float32 [6], the first two rows of F^-1; rect: (y0, x0, Hr, Wr);
    keypoints: the moved points), or a string naming why the image is skipped."""
    if eye_angle(kp) is None:
        return "both eyes are on one pixel"
    F, Finv = rotation_maps(kp, H, W)
    moved = move_keypoints(kp, F, Finv, H, W)
    r = face_rectangle(moved, H, W)
    if r is None:
        return "its face rectangle is degenerate"
    tl_y, tl_x, br_y, br_x = r
    return dict(inv=Finv[:2].reshape(6).astype(np.float32), rect=(tl_y, tl_x, br_y - tl_y + 1, br_x - tl_x + 1), keypoints=moved)


def warp_rect_np(img, inv, rect):
    """The rectangle (y0, x0, Hr, Wr) of tf.warp(img, F^-1, mode="nearest") re-quantised as dataset.py:174 does, uint8 [Hr, Wr, 3]: the
    fp32 sequence of dataset.augment_images' warp on p = u8 / 255, then (u8)(w 255) truncated.  Only the rectangle's pixels are
    computed - the warp is pointwise."""
    from .dataset import _warp_taps
    f32 = np.float32
    img = np.asarray(img)
    Hs, Ws, _ = img.shape
    y0, x0, Hr, Wr = rect
    m00, m01, m02, m10, m11, m12 = np.asarray(inv, f32)
    xs, ys = np.arange(x0, x0 + Wr, dtype=f32)[None, :], np.arange(y0, y0 + Hr, dtype=f32)[:, None]
    p = img.astype(f32) / f32(255.0)
    tx0, tx1, fx = _warp_taps((m00 * xs + m01 * ys) + m02, Ws)
    ty0, ty1, fy = _warp_taps((m10 * xs + m11 * ys) + m12, Hs)
    fx, fy = fx[..., None], fy[..., None]
    gx, gy = f32(1) - fx, f32(1) - fy
    top = gx * p[ty0, tx0] + fx * p[ty0, tx1]
    bot = gx * p[ty1, tx0] + fx * p[ty1, tx1]
    w = gy * top + fy * bot
    return (w * f32(255.0)).astype(np.int32).astype(np.uint8)


# ---------------------------------------------------------------- 4. resize
def resample_ksize(n_in, n_out):
    """Pillow's ksize of one axis for the bilinear filter (support 1): 2 ceil(max(in / out, 1)) + 1."""
    return 2 * ((max(n_in, n_out) + n_out - 1) // n_out) + 1


def resize_taps(n_in, n_out):
    """One axis of Pillow's 8-bit bilinear resampling (Resample.c precompute_coeffs + normalize_coeffs_8bpc) -> (bounds int32 [out, 2]
    of (first source sample, count), taps int32 [out, ksize]), computed in double exactly as the C does."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds, taps = np.zeros((n_out, 2), np.int32), np.zeros((n_out, ksize), np.int32)
    ss = 1.0 / fs
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = []
        for x in range(xmax):
            t = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - t if t < 1.0 else 0.0)
        ww = 0.0
        for v in w:
            ww += v
        bounds[i] = (xmin, xmax)
        for x in range(xmax):
            k = w[x] / ww if ww != 0.0 else w[x]
            taps[i, x] = int(-0.5 + k * 4194304.0) if k < 0 else int(0.5 + k * 4194304.0)
    assert ksize == resample_ksize(n_in, n_out)
    return bounds, taps


_taps_cache = {}


def _cached_taps(n_in, n_out):
    key = (int(n_in), int(n_out))
    if key not in _taps_cache:
        if len(_taps_cache) > 4096:
            _taps_cache.clear()
        _taps_cache[key] = resize_taps(*key)
    return _taps_cache[key]


def _resample_axis1(a, n_out):
    """One pass along axis 1 of an 8-bit [A, n_in, C] array: clip8((2^21 + sum pixel k) >> 22) per output sample, in int32."""
    bounds, taps = _cached_taps(a.shape[1], n_out)
    out = np.empty((a.shape[0], n_out, a.shape[2]), np.uint8)
    a32 = a.astype(np.int32)
    for i in range(n_out):
        lo, cnt = int(bounds[i, 0]), int(bounds[i, 1])
        ss = np.int32(1 << 21) + np.tensordot(a32[:, lo:lo + cnt], taps[i, :cnt], axes=([1], [0]))
        out[:, i] = np.clip(ss >> 22, 0, 255)
    return out


def resize_np(u8, out_h, out_w=None):
    """Image.fromarray(u8).resize((out_w, out_h), BILINEAR) for an 8-bit [H, W, C] image: the horizontal pass into 8 bits, then the
    vertical one (an axis already at its target size is multiplied by the identity taps, which changes nothing)."""
    out_w = out_h if out_w is None else out_w
    h = _resample_axis1(np.ascontiguousarray(u8), out_w)                           # [H, out_w, C]
    return np.ascontiguousarray(_resample_axis1(np.ascontiguousarray(h.transpose(1, 0, 2)), out_h).transpose(1, 0, 2))


# ---------------------------------------------------------------- the chain
def extract_faces_np(images, keypoints, out=64):
    """The faces of `images` (8-bit RGB arrays [H, W, 3], any sizes) with their parsed keypoints ([9, 2] of (y, x) each), uint8
    [N, out, out, 3]: the yardstick of cg_faces_u8_extract.  An image the front end would skip (face_geometry gives a reason) is an
    error here."""
    res = np.empty((len(images), out, out, 3), np.uint8)
    for n, (img, kp) in enumerate(zip(images, keypoints)):
        g = face_geometry(np.asarray(kp), img.shape[0], img.shape[1])
        if isinstance(g, str):
            raise ValueError(f"extract_faces_np: image {n}: {g}")
        res[n] = resize_np(warp_rect_np(img, g["inv"], g["rect"]), out)
    return res


def pack_padded_descriptors(shapes, geoms, pads, out):
    """The arrays cg_faces_u8_extract_padded reads (catgan.h) for faces with the source sizes `shapes` [(Hs, Ws)], the geometries
    `geoms` (dict(inv, rect), as face_geometry's) and the pads `pads` -> dict(src_off uint64 [N], geom int32 [N, 8], inv float32
    [N, 6], taps int32 [ntaps], tap_off uint64 [N, 2], pads int32 [N], rows = sum of Hr + 2 pad).  geom keeps the un-padded rectangle;
    its two ksizes and the tap tables belong to the padded sides, and faces of one padded side share a table.  Source f is expected at
    src_off[f] of the concatenated bytes."""
    N = len(shapes)
    src_off, geom = np.zeros(N, np.uint64), np.zeros((N, 8), np.int32)
    inv, tap_off = np.zeros((N, 6), np.float32), np.zeros((N, 2), np.uint64)
    pads = np.asarray(pads, np.int32).reshape(N)
    tables, where, ntaps, off = [], {}, 0, 0
    for f, ((Hs, Ws), g) in enumerate(zip(shapes, geoms)):
        y0, x0, Hr, Wr = g["rect"]
        Hp, Wp = Hr + 2 * int(pads[f]), Wr + 2 * int(pads[f])
        src_off[f] = off
        off += Hs * Ws * 3
        geom[f] = (Hs, Ws, y0, x0, Hr, Wr, resample_ksize(Wp, out), resample_ksize(Hp, out))
        inv[f] = g["inv"]
        for a, side in enumerate((Wp, Hp)):
            if side not in where:
                b, k = _cached_taps(side, out)
                where[side] = ntaps
                tables += [b.reshape(-1), k.reshape(-1)]
                ntaps += b.size + k.size
            tap_off[f, a] = where[side]
    return dict(src_off=src_off, geom=geom, inv=inv, taps=np.concatenate(tables).astype(np.int32), tap_off=tap_off, pads=pads,
                rows=int((geom[:, 4].astype(np.int64) + 2 * pads.astype(np.int64)).sum()))


def pack_descriptors(shapes, geoms, out):
    """The arrays cg_faces_u8_extract reads (catgan.h) for faces with the source sizes `shapes` [(Hs, Ws)] and the geometries `geoms`
    (dict(inv, rect), as face_geometry's) -> dict(src_off uint64 [N], geom int32 [N, 8], inv float32 [N, 6], taps int32 [ntaps],
    tap_off uint64 [N, 2], rows = sum of Hr).  Faces of one side share a tap table; source f is expected at src_off[f] of the
    concatenated bytes.  It is pack_padded_descriptors without a pad."""
    d = pack_padded_descriptors(shapes, geoms, np.zeros(len(shapes), np.int32), out)
    del d["pads"]
    return d


def workspace_bytes(N, out, rows):
    """cg_faces_u8_extract's workspace for N faces whose rectangles have `rows` rows in all (catgan.h)."""
    return 16 * N + 48 + 3 * out * rows


class _DeviceBatch:
    """One batch held on the device for the three entry points: the concatenated sources and the arrays of the descriptors `d`
    (pack_descriptors' or pack_padded_descriptors'), uploaded once each, and one workspace of `wsb` bytes that every call of the batch
    shares."""

    def __init__(self, images, d, wsb):
        import torch
        from . import tensor
        self.torch, self.dev, self.lib, self.N = torch, tensor.device(), tensor.lib(), len(images)
        self.src = self.up(np.concatenate([np.ascontiguousarray(im, dtype=np.uint8).reshape(-1) for im in images]))
        self.d = {k: self.up(v) for k, v in d.items() if k != "rows"}
        self.ws = torch.empty(wsb, dtype=torch.uint8, device=self.dev)

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(self.dev)   # bytes: torch has no uint64 arithmetic to need

    def call(self, fn, d, shape, *own):
        """fn(the stream, the nine leading arguments out of the uploaded arrays d, *own, dst, N, side, the workspace) -> dst, uint8
        [N, *shape, 3] with side = shape[-1], on the host."""
        from . import tensor
        dst = self.torch.empty((self.N,) + shape + (3,), dtype=self.torch.uint8, device=self.dev)
        fn(tensor.stream(), self.src.data_ptr(), self.src.numel(), d["src_off"].data_ptr(), d["geom"].data_ptr(), d["inv"].data_ptr(),
           d["taps"].data_ptr(), d["taps"].numel() // 4, d["tap_off"].data_ptr(), *own, dst.data_ptr(), self.N, shape[-1], self.ws.data_ptr(),
           self.ws.numel())
        return dst.cpu().numpy()

    def faces(self, out, own=None):
        """cg_faces_u8_extract over the batch; `own`: uploaded geom, taps and tap_off of the faces where the batch's are another form's."""
        return self.call(self.lib.faces_u8_extract, {**self.d, **(own or {})}, (out, out))


def extract_faces_device(images, geoms, out=64):
    """cg_faces_u8_extract over one batch: `images` 8-bit RGB arrays, `geoms` their face_geometry results -> uint8 [N, out, out, 3] on
    the host.  One upload of the concatenated sources and of the descriptors, one call, one download."""
    d = pack_descriptors([im.shape[:2] for im in images], geoms, out)
    return _DeviceBatch(images, d, workspace_bytes(len(images), out, d["rows"])).faces(out)


# ---------------------------------------------------------------- the variants out of the padded crop
def _median_u8(a, axis):
    """The median of 8-bit samples along `axis`, kept as a dimension of 1: the middle one, or the mean of the two middle ones rounded
    half to even, in integers."""
    srt = np.sort(np.asarray(a, np.uint8), axis=axis).astype(np.int32)
    L = srt.shape[axis]
    t = np.take(srt, [(L - 1) // 2], axis=axis) + np.take(srt, [L // 2], axis=axis)
    m = t >> 1
    return (m + ((t & 1) & (m & 1))).astype(np.uint8)


def median_pad_np(win, top, left, bottom, right):
    """np.pad(win, ((top, bottom), (left, right), (0, 0)), mode="median") for an 8-bit [H, W, 3] array, written out (dataset.py:228):
    axis 0 first - every column gets, per channel, the median of that column over win's rows - then axis 1 over ALL rows of the
    result, the rows just filled included, which is how the corners get their values."""
    win = np.asarray(win, np.uint8)
    H, W, _ = win.shape
    P = np.empty((H + top + bottom, W + left + right, 3), np.uint8)
    P[top:top + H, left:left + W] = win
    if top or bottom:
        m = _median_u8(win, 0)                                          # [1, W, 3]
        P[:top, left:left + W] = m
        P[top + H:, left:left + W] = m
    if left or right:
        m = _median_u8(P[:, left:left + W], 1)                          # [Hp, 1, 3]
        P[:, :left] = m
        P[:, left + W:] = m
    return P


def crop_pads(Hs, Ws, rect, pad):
    """(top, left, bottom, right): how far the rectangle enlarged by `pad` leaves its Hs x Ws image on each side (dataset.py:206-226)."""
    y0, x0, Hr, Wr = rect
    return (max(0, pad - y0), max(0, pad - x0), max(0, y0 + Hr - 1 + pad - (Hs - 1)), max(0, x0 + Wr - 1 + pad - (Ws - 1)))


def padded_crop_np(img, inv, rect, pad):
    """Stage a: extract_rectangle(pad) (dataset.py:191-230) out of the de-rotated image, uint8 [Hr + 2 pad, Wr + 2 pad, 3] - warp_rect_np
    over the enlarged rectangle clipped to the image, then the median fill of the sides that left it."""
    Hs, Ws = np.asarray(img).shape[:2]
    y0, x0, Hr, Wr = rect
    top, left, bottom, right = crop_pads(Hs, Ws, rect, pad)
    win = warp_rect_np(img, inv, (y0 - pad + top, x0 - pad + left, Hr + 2 * pad - top - bottom, Wr + 2 * pad - left - right))
    return median_pad_np(win, top, left, bottom, right)


def margin_pad(Hr, margin, out):
    """The full-resolution pad of a face whose rectangle has the side Hr and whose out x out form keeps `margin` pixels around it:
    margin Hr / out rounded half up, in integers.  Rectangles are square, so one value serves both axes."""
    return (2 * margin * Hr + out) // (2 * out)


def padded_face_np(img, inv, rect, margin, out=64):
    """The padded face of generate_dataset.py --margin, uint8 [out + 2 margin, out + 2 margin, 3]: stage a with the pad
    margin_pad(Hr, margin, out) - real image around the rectangle, median-filled where that leaves the image - through stage 4's
    unchanged resize.  The pad is rounded to whole source pixels, so the centre window is the _000 face exactly only at unit scale
    (Hr == out); elsewhere the two differ by that rounding's fraction of a face pixel."""
    return resize_np(padded_crop_np(img, inv, rect, margin_pad(rect[2], margin, out)), out + 2 * margin)


def noise_scale(noise_std):
    """s of the pixel stage: 255 noise_std, rounded to fp32 once."""
    return np.float32(255.0 * float(noise_std))


def variant_pixels_np(P, brightness, flip, scale, seed, base):
    """Stage b on the whole padded crop: q = (u8) clip(fl(fl(P[y][flip ? Wp-1-x : x][c] brightness) + fl(scale z)), 0, 255) truncated
    (NaN -> 0), z = dataset.augment_noise(seed, base, j), j = (y Wp + x) 3 + c on the flipped array; the noise term is left out for
    scale == 0."""
    from .dataset import augment_noise
    f32 = np.float32
    P = np.asarray(P, np.uint8)
    v = (P[:, ::-1] if flip != 0 else P).astype(f32) * f32(brightness)
    if f32(scale) != 0:
        v = v + f32(scale) * augment_noise(seed, base, np.arange(P.size, dtype=np.uint64).reshape(P.shape))
    with np.errstate(invalid="ignore"):
        v = np.where(~(v >= f32(0)), f32(0), np.where(v > f32(255), f32(255), v)).astype(f32)
    return v.astype(np.int32).astype(np.uint8)


def variant_warp_np(q, m, pad):
    """Stage c: warp_rect_np's arithmetic on the pixel stage q [Hp, Wp, 3] with the inverse entries m [6], over the window
    [pad, pad + Hr) x [pad, pad + Wr): uint8 [Hr, Wr, 3]."""
    Hp, Wp, _ = q.shape
    return warp_rect_np(q, m, (pad, pad, Hp - 2 * pad, Wp - 2 * pad))


def variants_np(img, inv, rect, pad, desc, bases, scale, seed, out=64):
    """The variants of one face, uint8 [A, out, out, 3]: stages a-d for the descriptors desc [A, 8] (m00 .. m12 of the inverse for the
    PADDED crop's size, brightness, flip: dataset.augment_descriptors(A, Hp, Wp, draw)) and the counter bases [A].  The yardstick of
    cg_faces_u8_extract_variants."""
    P = padded_crop_np(img, inv, rect, pad)
    desc = np.asarray(desc, np.float32)
    res = np.empty((len(desc), out, out, 3), np.uint8)
    for a, d in enumerate(desc):
        q = variant_pixels_np(P, d[6], d[7], scale, seed, int(bases[a]))
        res[a] = resize_np(variant_warp_np(q, d[:6], pad), out)
    return res


def variant_bytes(rect, pad, A, out):
    """Device bytes that one face's variants take beside its source: the padded crop, the horizontal passes' results and the output."""
    _, _, Hr, Wr = rect
    return -(-(3 * (Hr + 2 * pad) * (Wr + 2 * pad)) // 16) * 16 + 3 * A * out * (Hr + out)


def variants_workspace_bytes(rects, pad, A, out):
    """cg_faces_u8_extract_variants' workspace for faces with the rectangles `rects` (catgan.h)."""
    return 48 * len(rects) + 256 + sum(variant_bytes(r, pad, A, out) - 3 * A * out * out for r in rects)


def extract_variants_device(images, geoms, pad, desc, bases, scale, seed, out=64, with_faces=False):
    """cg_faces_u8_extract_variants over one batch: desc float32 [N, A, 8], bases uint64 [N, A] -> uint8 [N, A, out, out, 3] on the
    host.  with_faces also runs cg_faces_u8_extract over the same upload and returns (faces [N, out, out, 3], variants)."""
    d = pack_descriptors([im.shape[:2] for im in images], geoms, out)
    desc, bases = np.ascontiguousarray(desc, np.float32), np.ascontiguousarray(bases, np.uint64)
    N, A = bases.shape
    assert N == len(images) and desc.shape == (N, A, 8)
    b = _DeviceBatch(images, d, max(variants_workspace_bytes([g["rect"] for g in geoms], pad, A, out), workspace_bytes(N, out, d["rows"])))
    ddesc, dbases = b.up(desc), b.up(bases)
    faces = b.faces(out) if with_faces else None
    v = b.call(b.lib.faces_u8_extract_variants, b.d, (A, out, out), pad, A, ddesc.data_ptr(), dbases.data_ptr(), float(scale), int(seed))
    return (faces, v) if with_faces else v


# ---------------------------------------------------------------- the padded faces on the device
PADDED_SIDE_MAX = 8192   # cg_faces_u8_extract_padded's largest padded side, Hr + 2 pad: one row of it still fits a band of the horizontal pass
PADDED_PAD_MAX = 2048    # and its largest pad


def padded_fits_device(rect, pad):
    """Whether cg_faces_u8_extract_padded takes a face with this rectangle and pad; padded_face_np takes every one."""
    return 0 <= pad <= PADDED_PAD_MAX and max(rect[2], rect[3]) + 2 * pad <= PADDED_SIDE_MAX


def padded_bytes(rect, pad, out):
    """Device bytes that one padded face takes beside its source: the padded crop, the horizontal pass' result and the out x out face."""
    _, _, Hr, Wr = rect
    return -(-(3 * (Hr + 2 * pad) * (Wr + 2 * pad)) // 16) * 16 + 3 * out * (Hr + 2 * pad + out)


def padded_workspace_bytes(rects, pads, out):
    """cg_faces_u8_extract_padded's workspace for faces with the rectangles `rects` and the pads `pads` (catgan.h)."""
    return 80 * len(rects) + 256 + sum(padded_bytes(r, int(p), out) - 3 * out * out for r, p in zip(rects, pads))


def extract_padded_device(images, geoms, margin, out=64, with_faces=False):
    """cg_faces_u8_extract_padded over one batch: the padded faces of generate_dataset.py --margin, uint8
    [N, out + 2 margin, out + 2 margin, 3] on the host - padded_face_np's bytes, face f's pad being margin_pad(Hr, margin, out).  One
    upload of the concatenated sources and of the descriptors.  with_faces also runs cg_faces_u8_extract over the same upload (its
    own geometry and tap tables beside the padded ones) and returns (faces [N, out, out, 3], padded)."""
    shapes, rects, N, side = [im.shape[:2] for im in images], [g["rect"] for g in geoms], len(images), out + 2 * margin
    pads = [margin_pad(r[2], margin, out) for r in rects]
    d = pack_padded_descriptors(shapes, geoms, pads, side)
    fd = pack_descriptors(shapes, geoms, out) if with_faces else None
    b = _DeviceBatch(images, d, max(padded_workspace_bytes(rects, pads, side), workspace_bytes(N, out, fd["rows"]) if with_faces else 0))
    faces = b.faces(out, {k: b.up(fd[k]) for k in ("geom", "taps", "tap_off")}) if with_faces else None
    p = b.call(b.lib.faces_u8_extract_padded, b.d, (side, side), b.d["pads"].data_ptr())
    return (faces, p) if with_faces else p


# ---------------------------------------------------------------- a synthetic raw tree (tests, scripts/faces_bench.py)
TEMPLATE = np.array([[-1.0, -0.5], [1.0, -0.5], [0.0, 1.0], [-2.2, -1.2], [-1.8, -2.6], [-0.8, -1.8], [0.8, -1.8], [1.8, -2.6], [2.2, -1.2]])
TILTS = (0.0, 9.0, -14.0, 25.0)


def template_keypoints(H, W, tilt_deg, cy=None, cx=None):
    """Nine (x, y) keypoints in the .cat order (left eye, right eye, mouth, three per ear): TEMPLATE scaled by 0.12 min(H, W), tilted
    about (cx, cy) - the image centre unless given - and rounded."""
    s, r = 0.12 * min(H, W), math.radians(tilt_deg)
    cy, cx = (H // 2 if cy is None else cy), (W // 2 if cx is None else cx)
    x = cx + s * (TEMPLATE[:, 0] * math.cos(r) - TEMPLATE[:, 1] * math.sin(r))
    y = cy + s * (TEMPLATE[:, 0] * math.sin(r) + TEMPLATE[:, 1] * math.cos(r))
    return np.stack([np.rint(x), np.rint(y)], 1).astype(np.int64)


def cat_line(xy):
    """The line of a .cat file for nine (x, y) points."""
    return "9 " + " ".join(f"{int(x)} {int(y)}" for x, y in xy) + " \n"


def write_raw_tree(path, sizes, folders=("CAT_00", "CAT_01"), seed=0, quality=90):
    """A stand-in for the 10k-cats download under `path`: image i (smooth random colours, sizes[i] = (H, W)) goes to folder
    i % len(folders) as NNNNNNNN_000.jpg with its .cat file, its face tilted by TILTS[i % 4].  Returns the files in the front end's
    order (folder by folder, then by name)."""
    import os
    from PIL import Image
    rs = np.random.RandomState(seed)
    files = []
    for d in folders:
        os.makedirs(os.path.join(path, d), exist_ok=True)
    for i, (H, W) in enumerate(sizes):
        small = rs.randint(0, 256, size=(max(H // 8, 2), max(W // 8, 2), 3)).astype(np.uint8)
        img = Image.fromarray(small).resize((W, H), Image.BICUBIC)
        fp = os.path.join(path, folders[i % len(folders)], f"{i:08d}_000.jpg")
        img.save(fp, quality=quality)
        with open(fp + ".cat", "w") as f:
            f.write(cat_line(template_keypoints(H, W, TILTS[i % len(TILTS)])))
        files.append(fp)
    return sorted(files)
