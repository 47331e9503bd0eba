"""The variants out of the padded crop on the MI355X: cg_faces_u8_extract_variants bit-equal to faces.variants_np's stages (whose own
yardsticks are in tests/test_faces_variants_host.py) over a mixed batch whose padded rectangles leave their images in every way, the
clamp at the padded crop's border, independence of batch order and split, its argument checks, and generate_dataset.py
--variantsFrom crop on the device against --host, file by file.  Every comparison is exact."""
import filecmp
import importlib
import os

import numpy as np
import pytest
import torch

import test_faces_host as H
import test_faces_variants_host as V
from test_gpu_faces import tilted

pytestmark = pytest.mark.gpu
PAD, AMAX, SEED = 30, 9, 0x1234567887654321 >> 1
SCALE = np.float32(255.0 * 0.02)


@pytest.fixture(scope="module")
def cg():
    assert torch.cuda.is_available()
    return importlib.import_module("cat-generator_amd")


@pytest.fixture(scope="module")
def F():
    return importlib.import_module("cat-generator_amd.faces")


@pytest.fixture(scope="module")
def ds():
    return importlib.import_module("cat-generator_amd.dataset")


def draws(ds, rs, rect, pad, A):
    """desc [A, 8] for one face: the two extreme draws first (8 degrees, both zoom limits, +-4 pixels, both flips, both brightness
    limits), then draws from the default ranges"""
    d = dict(flip=rs.randint(0, 2, A), scale=rs.uniform(0.93, 1.08, A), rotation=rs.randint(-8, 9, A), tx=rs.randint(-4, 5, A),
             ty=rs.randint(-4, 5, A), brightness=rs.uniform(0.85, 1.15, A))
    for k, v in dict(flip=(1, 0), scale=(0.93, 1.08), rotation=(8, -8), tx=(4, -4), ty=(-4, 4), brightness=(1.15, 0.85)).items():
        d[k][:min(2, A)] = v[:min(2, A)]
    return np.stack([ds.augment_descriptor(d, a, rect[2] + 2 * pad, rect[3] + 2 * pad) for a in range(A)])


def reference(F, images, geoms, pad, desc, bases, scale):
    """the warped windows of the restatement before the resize, [face][variant] -> uint8 [Hr, Wr, 3]"""
    res = []
    for im, g, dd, bb in zip(images, geoms, desc, bases):
        P = F.padded_crop_np(im, g["inv"], g["rect"], pad)
        res.append([F.variant_warp_np(F.variant_pixels_np(P, d[6], d[7], scale, SEED, int(b)), d[:6], pad) for d, b in zip(dd, bb)])
    return res


@pytest.fixture(scope="module")
def batch(F, ds):
    """A dozen faces, their nine descriptors and counter bases each, and the restatement's warped windows: computed once, read by every
    (A, out)."""
    rs = np.random.RandomState(21)
    pic = lambda h, w: rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    images, geoms = [], []
    for (Hs, Ws), tilt in (((61, 83), 9.0), ((97, 131), -14.0), ((61, 61), 25.0), ((97, 97), 0.0), ((375, 500), 9.0)):
        img = pic(Hs, Ws)                                        # centred template faces: rectangles of about half the short side
        images.append(img)
        geoms.append(F.face_geometry(H.yx(F, Hs, Ws, tilt), Hs, Ws))
    big = images[-1]
    extra = [(pic(97, 131), dict(inv=tilted(9.0, 48, 65), rect=(3, 5, 40, 40))),            # a corner: pads top and left only
             (pic(97, 131), dict(inv=tilted(-14.0, 48, 65), rect=(50, 84, 47, 47))),        # the other corner: bottom and right
             (pic(61, 83), dict(inv=tilted(25.0, 30, 41), rect=(20, 40, 8, 8))),            # the smallest rectangle
             (pic(200, 160), dict(inv=tilted(9.0, 100, 80), rect=(10, 60, 150, 90))),       # not square, the top leaves the image
             (big, dict(inv=tilted(0.0, 0, 0), rect=(100, 0, 203, 120))),                   # not square, at the left border
             (big, dict(inv=tilted(-14.0, 187, 250), rect=(31, 34, 64, 64))),               # the margin just inside
             (pic(64, 97), dict(inv=tilted(0.0, 0, 0), rect=(0, 0, 64, 97)))]               # the whole image: every side pads by PAD
    images += [e[0] for e in extra]
    geoms += [e[1] for e in extra]
    pads = [F.crop_pads(im.shape[0], im.shape[1], g["rect"], PAD) for im, g in zip(images, geoms)]
    assert min(pads[2]) > 0 and min(pads[3]) > 0 and pads[0][0] > 0 and pads[0][2] > 0 and pads[1][0] > 0      # all four sides / top and bottom
    assert pads[4] == (0, 0, 0, 0) and pads[10] == (0, 0, 0, 0)
    assert pads[5][0] > 0 and pads[5][1] > 0 and pads[5][2:] == (0, 0) and pads[6][:2] == (0, 0) and min(pads[6][2:]) > 0
    assert pads[11] == (PAD,) * 4
    N = len(images)
    desc = np.stack([draws(ds, rs, g["rect"], PAD, AMAX) for g in geoms]).astype(np.float32)
    bases = (np.arange(N * AMAX, dtype=np.uint64).reshape(N, AMAX) << np.uint64(32)) + np.uint64(7)
    return images, geoms, desc, bases, reference(F, images, geoms, PAD, desc, bases, SCALE)


# ---------------------------------------------------------------- device against the restatement
@pytest.mark.parametrize("out", [64, 16])
@pytest.mark.parametrize("A", [1, 3, 9])
def test_kernels_equal_the_host_restatement_bit_for_bit(cg, F, batch, A, out):
    images, geoms, desc, bases, warped = batch
    got = F.extract_variants_device(images, geoms, PAD, desc[:, :A], bases[:, :A], SCALE, SEED, out)
    assert got.shape == (len(images), A, out, out, 3) and got.dtype == np.uint8
    for n in range(len(images)):
        for a in range(A):
            np.testing.assert_array_equal(got[n, a], F.resize_np(warped[n][a], out), err_msg=f"face {n} variant {a}: {geoms[n]['rect']} of {images[n].shape}")


def test_padded_crop_without_noise_and_without_padding(cg, F, batch):
    """noise_scale 0 leaves the noise term out, pad 0 has no margin at all: the identity draw then returns the _000 faces"""
    images, geoms, desc, bases, _ = batch
    images, geoms = images[:6], geoms[:6]
    ident = np.tile(np.array([1, 0, 0, 0, 1, 0, 1, 0], np.float32), (len(images), 1, 1))
    got = F.extract_variants_device(images, geoms, 0, ident, bases[:6, :1], 0.0, SEED, 64)
    for n, (im, g) in enumerate(zip(images, geoms)):
        np.testing.assert_array_equal(got[n, 0], F.resize_np(F.warp_rect_np(im, g["inv"], g["rect"]), 64))
    faces, got2 = F.extract_variants_device(images, geoms, PAD, desc[:6, :2], bases[:6, :2], 0.0, SEED, 64, with_faces=True)
    want = reference(F, images, geoms, PAD, desc[:6, :2], bases[:6, :2], 0.0)
    for n, (im, g) in enumerate(zip(images, geoms)):
        np.testing.assert_array_equal(faces[n], F.resize_np(F.warp_rect_np(im, g["inv"], g["rect"]), 64))
        for a in range(2):
            np.testing.assert_array_equal(got2[n, a], F.resize_np(want[n][a], 64))


def test_large_rectangles(cg, F, ds):
    """641 pixels: ksize 23, sixteen rows per band (the cap), a crop many workgroups wide, padding at the top and the right; the whole
    700 x 700 image: fifteen rows per band, a last band of ten, every side padded by PAD"""
    rs = np.random.RandomState(33)
    img = rs.randint(0, 256, (700, 700, 3)).astype(np.uint8)
    geoms = [dict(inv=tilted(9.0, 350, 350), rect=(20, 40, 641, 641)), dict(inv=tilted(-14.0, 350, 350), rect=(0, 0, 700, 700))]
    assert F.crop_pads(700, 700, geoms[0]["rect"], PAD) == (10, 0, 0, 11) and F.resample_ksize(641, 64) == 23
    desc = np.stack([draws(ds, rs, g["rect"], PAD, 1) for g in geoms]).astype(np.float32)
    bases = np.array([[5 << 32], [6 << 32]], np.uint64)
    got = F.extract_variants_device([img, img], geoms, PAD, desc, bases, SCALE, SEED, 64)
    want = reference(F, [img, img], geoms, PAD, desc, bases, SCALE)
    for n in range(2):
        np.testing.assert_array_equal(got[n, 0], F.resize_np(want[n][0], 64), err_msg=f"face {n}")


# ---------------------------------------------------------------- the clamp at the padded crop's border
def test_positions_beyond_the_padded_crop_replicate_its_edge(cg, F):
    img, geom, pad, desc, want = V.clamp_case(F)
    got = F.extract_variants_device([img], [geom], pad, desc[None], np.zeros((1, 1), np.uint64), 0.0, SEED, 16)
    np.testing.assert_array_equal(got[0, 0], F.resize_np(want, 16))


# ---------------------------------------------------------------- batch order and split
def test_variants_do_not_depend_on_batch_order_or_split(cg, F, batch):
    images, geoms, desc, bases, _ = batch
    A, out = 3, 32
    call = lambda ix: F.extract_variants_device([images[i] for i in ix], [geoms[i] for i in ix], PAD, desc[ix, :A], bases[ix, :A], SCALE, SEED, out)
    order = list(range(len(images)))
    whole = call(order)
    mixed = order[::-1][3:] + order[::-1][:3]
    for part in (mixed[:1], mixed[1:6], mixed[6:]):
        got = call(part)
        for k, i in enumerate(part):
            np.testing.assert_array_equal(got[k], whole[i], err_msg=f"face {i}")


# ---------------------------------------------------------------- argument checks
def test_bad_arguments_are_refused_before_any_launch(cg, F):
    shapes = [(97, 131), (61, 83)]
    geoms = [dict(inv=tilted(9.0, 48, 65), rect=(10, 20, 64, 64)), dict(inv=tilted(0.0, 0, 0), rect=(5, 5, 33, 40))]
    d = F.pack_descriptors(shapes, geoms, 64)
    N, out, A, pad = 2, 64, 2, 30
    d["desc"] = np.tile(np.array([1, 0, 0, 0, 1, 0, 1, 0], np.float32), (N, A, 1))
    d["bases"] = np.zeros((N, A), np.uint64)
    nsrc = sum(h * w * 3 for h, w in shapes)
    wsb = F.variants_workspace_bytes([g["rect"] for g in geoms], pad, A, out)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    src, ws = torch.zeros(nsrc, dtype=torch.uint8).cuda(), torch.zeros(wsb, dtype=torch.uint8).cuda()
    dst = torch.full((N, A, out, out, 3), 7, dtype=torch.uint8).cuda()
    call, s = cg.lib().faces_u8_extract_variants, cg.tensor.stream()
    arrays = ("src_off", "geom", "inv", "taps", "tap_off", "desc", "bases")

    def args(**kw):
        """the valid call with some descriptor arrays / scalars replaced"""
        a = dict(d, src=src.data_ptr(), src_bytes=nsrc, dst=dst.data_ptr(), N=N, out=out, ws=ws.data_ptr(), wsb=wsb, ntaps=d["taps"].size,
                 pad=pad, A=A, scale=0.0)
        a.update(kw)
        keep = [up(a[k]) if isinstance(a[k], np.ndarray) else None for k in arrays]
        p = {k: (t.data_ptr() if t is not None else a[k]) for k, t in zip(arrays, keep)}
        return keep, (s, a["src"], a["src_bytes"], p["src_off"], p["geom"], p["inv"], p["taps"], a["ntaps"], p["tap_off"], a["pad"], a["A"],
                      p["desc"], p["bases"], a["scale"], SEED, a["dst"], a["N"], a["out"], a["ws"], a["wsb"])

    def geom(f, col, v):
        g = d["geom"].copy()
        g[f, col] = v
        return g

    bad_bounds = d["taps"].copy()
    bad_bounds[int(d["tap_off"][0, 0]) + 2 * 63] = 64          # the last horizontal sample of face 0 would read past its side
    cases = [(dict(src=None), "null pointer"), (dict(src_off=None), "null pointer"), (dict(geom=None), "null pointer"),
             (dict(inv=None), "null pointer"), (dict(taps=None), "null pointer"), (dict(tap_off=None), "null pointer"),
             (dict(desc=None), "null pointer"), (dict(bases=None), "null pointer"),
             (dict(dst=None), "null pointer"), (dict(ws=None), "null pointer"),
             (dict(N=0), "N = 0"), (dict(N=-3), "N = -3"), (dict(out=7), "out = 7"), (dict(out=129), "out = 129"),
             (dict(pad=-1), "pad = -1"), (dict(pad=65), "pad = 65"), (dict(A=0), "A = 0"), (dict(A=1000), "A = 1000"),
             (dict(scale=-0.5), "noise_scale"), (dict(scale=float("inf")), "noise_scale"), (dict(scale=float("nan")), "noise_scale"),
             (dict(geom=geom(0, 0, 7)), "source is outside"), (dict(geom=geom(1, 1, 8193)), "source is outside"),
             (dict(geom=geom(0, 4, 7)), "rectangle is outside"), (dict(geom=geom(1, 5, 4097)), "rectangle is outside"),
             (dict(geom=geom(0, 2, 34)), "not inside its"), (dict(geom=geom(1, 3, 44)), "not inside its"), (dict(geom=geom(0, 2, -1)), "not inside its"),
             (dict(geom=geom(0, 6, 5)), "ksize"), (dict(geom=geom(1, 7, 5)), "ksize"),
             (dict(src_bytes=nsrc - 1), "does not fit the"), (dict(ntaps=d["taps"].size - 1), "does not fit the"),
             (dict(taps=bad_bounds), "reads \\["), (dict(wsb=wsb - 48 * N - 256 - 1), "workspace"), (dict(wsb=0), "workspace")]
    for kw, message in cases:
        keep, a = args(**kw)
        with pytest.raises(cg.CatganError, match="cg_faces_u8_extract_variants: .*" + message):
            call(*a)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 7).all()                     # nothing was launched
    keep, a = args()
    call(*a)                                                  # and the unmodified call is accepted
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0).all()                     # a black source


# ---------------------------------------------------------------- the front end
def test_generate_dataset_crop_mode_on_the_device_equals_host(cg, F, tmp_path, monkeypatch):
    H.make_tree(F, str(tmp_path / "raw"))
    argv = ["--path", str(tmp_path / "raw"), "--augmentations", "2", "--variantsFrom", "crop"]
    assert H.run_front_end(argv + ["--out", str(tmp_path / "host"), "--host"]) == (10, 2)
    assert H.run_front_end(argv + ["--out", str(tmp_path / "dev")]) == (10, 2)
    G = importlib.import_module("generate_dataset")
    monkeypatch.setattr(G, "VARIANT_BYTES", 600000)           # the device calls of one flush split: one to three faces each
    assert H.run_front_end(argv + ["--out", str(tmp_path / "split")]) == (10, 2)
    for d in ("out_aug_64x64", "out_unaug_64x64"):
        names = sorted(os.listdir(tmp_path / "host" / d))
        assert names == sorted(os.listdir(tmp_path / "dev" / d)) and len(names) == (30 if "_aug" in d else 10)
        for n in names:
            for dev in ("dev", "split"):
                assert filecmp.cmp(tmp_path / "host" / d / n, tmp_path / dev / d / n, shallow=False), f"{dev}: {d}/{n}"


def test_generate_dataset_crop_mode_at_128_pixels(cg, F, tmp_path):
    """--scale 128: the default mode refuses its variants (the augmentation kernel's LDS), the crop mode writes them"""
    H.make_tree(F, str(tmp_path / "raw"))
    argv = ["--path", str(tmp_path / "raw"), "--scale", "128", "--augmentations", "1", "--out", str(tmp_path / "o")]
    with pytest.raises(SystemExit, match="LDS"):
        H.run_front_end(argv)
    assert H.run_front_end(argv + ["--variantsFrom", "crop"]) == (10, 2)
    assert sorted(os.listdir(tmp_path / "o" / "out_aug_128x128")) == [f"{i:06d}_{a:03d}.jpg" for i in range(10) for a in range(2)]
    from PIL import Image
    assert Image.open(tmp_path / "o" / "out_aug_128x128" / "000004_001.jpg").size == (128, 128)
