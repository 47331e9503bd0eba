"""CPU checks of the variants warped from the padded full-resolution crop (cat-generator_amd/faces.py stages a-d, generate_dataset.py
--host --variantsFrom crop): the written-out median fill against np.pad, the padded crop where nothing leaves the image, the three
exact consequences of the semantics (identity, whole-pixel shifts, flip), the behaviour the mode adds (real pixels where the face mode
replicates an edge), the clamp at the padded crop's own border, and the front end over a synthetic raw tree.  Every comparison is exact."""
import filecmp
import importlib
import os
import sys

import numpy as np
import pytest

import test_faces_host as H

ROOT = H.ROOT
NEUTRAL = dict(scale=1.0, rotation=0, tx=0, ty=0, brightness=1.0, flip=0)


@pytest.fixture(scope="module")
def F():
    return importlib.import_module("cat-generator_amd.faces")


@pytest.fixture(scope="module")
def ds():
    return importlib.import_module("cat-generator_amd.dataset")


def one_draw(**kw):
    """an augment_draw(1) chosen by the test: neutral but for the entries named"""
    d = dict(NEUTRAL, **kw)
    return dict({k: np.array([v]) for k, v in d.items()}, seed=0, noise_std=0.0)


def descriptor(ds, Hp, Wp, **kw):
    return ds.augment_descriptors(1, Hp, Wp, one_draw(**kw))


def tilted_face(F, Hs, Ws, tilt, seed=0):
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (Hs, Ws, 3)).astype(np.uint8)
    g = F.face_geometry(H.yx(F, Hs, Ws, tilt), Hs, Ws)
    assert not isinstance(g, str)
    return img, g


def crop_variant(F, ds, img, g, pad, **kw):
    """the warped window (before the resize) of the variant with the draw `kw`, no noise"""
    _, _, Hr, Wr = g["rect"]
    d = descriptor(ds, Hr + 2 * pad, Wr + 2 * pad, **kw)[0]
    q = F.variant_pixels_np(F.padded_crop_np(img, g["inv"], g["rect"], pad), d[6], d[7], 0.0, 1, 0)
    return F.variant_warp_np(q, d[:6], pad)


# ---------------------------------------------------------------- a. the median fill
def test_median_fill_equals_numpy_pad(F):
    rs = np.random.RandomState(3)
    wins = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((7, 9), (8, 10), (7, 10), (8, 9), (2, 2), (1, 5), (31, 12))]
    # even lengths whose two middle bytes have an odd sum: .5 means that round down (to an even m) and up (from an odd m)
    halves = np.zeros((4, 4, 3), np.uint8)
    halves[:, :, 0] = [[10, 10, 11, 11]] * 4                  # 10.5 -> 10
    halves[:, :, 1] = [[11, 11, 12, 12]] * 4                  # 11.5 -> 12
    halves[:, :, 2] = np.array([[10, 10, 11, 11]] * 4).T
    wins.append(halves)
    assert F.median_pad_np(halves, 0, 1, 0, 0)[0, 0].tolist() == [10, 12, 10]
    assert F.median_pad_np(halves, 1, 0, 0, 0)[0, 0].tolist()[2] == 10
    pads = [(0, 0, 0, 0), (3, 0, 0, 0), (0, 4, 0, 0), (0, 0, 5, 0), (0, 0, 0, 2), (3, 4, 5, 2), (1, 1, 1, 1), (30, 30, 30, 30)]
    for w in wins:
        for top, left, bottom, right in pads:
            want = np.pad(w, ((top, bottom), (left, right), (0, 0)), mode="median")
            np.testing.assert_array_equal(F.median_pad_np(w, top, left, bottom, right), want, err_msg=f"{w.shape} {(top, left, bottom, right)}")


def test_padded_crop_with_its_margin_inside_is_the_enlarged_rectangle(F):
    img, g = tilted_face(F, 375, 500, 9.0)
    y0, x0, Hr, Wr = g["rect"]
    pad = 30
    assert F.crop_pads(375, 500, g["rect"], pad) == (0, 0, 0, 0)
    np.testing.assert_array_equal(F.padded_crop_np(img, g["inv"], g["rect"], pad),
                                  F.warp_rect_np(img, g["inv"], (y0 - pad, x0 - pad, Hr + 2 * pad, Wr + 2 * pad)))
    np.testing.assert_array_equal(F.padded_crop_np(img, g["inv"], g["rect"], 0), F.warp_rect_np(img, g["inv"], g["rect"]))


def test_padded_crop_that_leaves_the_image_is_numpy_pad_of_the_window(F):
    for Hs, Ws, sides in ((61, 83, 2), (97, 131, 2), (61, 61, 4), (64, 97, 2)):
        img, g = tilted_face(F, Hs, Ws, -14.0)
        y0, x0, Hr, Wr = g["rect"]
        top, left, bottom, right = F.crop_pads(Hs, Ws, g["rect"], 30)
        assert sum(v > 0 for v in (top, left, bottom, right)) >= sides, (top, left, bottom, right)
        wy0, wx0, wy1, wx1 = y0 - 30 + top, x0 - 30 + left, y0 + Hr + 30 - bottom, x0 + Wr + 30 - right
        assert wy0 >= 0 and wx0 >= 0 and wy1 <= Hs and wx1 <= Ws and (wy0 == 0) == (top > 0) and (wy1 == Hs) == (bottom > 0)
        win = F.warp_rect_np(img, g["inv"], (wy0, wx0, wy1 - wy0, wx1 - wx0))
        want = np.pad(win, ((top, bottom), (left, right), (0, 0)), mode="median")
        np.testing.assert_array_equal(F.padded_crop_np(img, g["inv"], g["rect"], 30), want)


# ---------------------------------------------------------------- the three exact consequences
def test_identity_shifts_and_flip_on_a_tilted_face(F, ds):
    Hs, Ws, pad = 200, 260, 30
    img, g = tilted_face(F, Hs, Ws, 9.0)
    y0, x0, Hr, Wr = g["rect"]
    assert F.crop_pads(Hs, Ws, (y0 - 4, x0 - 4, Hr + 8, Wr + 8), pad) == (0, 0, 0, 0)      # the margin and the shifts stay inside
    rect = lambda dy, dx: F.warp_rect_np(img, g["inv"], (y0 + dy, x0 + dx, Hr, Wr))
    np.testing.assert_array_equal(crop_variant(F, ds, img, g, pad), rect(0, 0))                      # the _000 rectangle
    np.testing.assert_array_equal(crop_variant(F, ds, img, g, pad, tx=4), rect(0, -4))               # real neighbouring pixels
    np.testing.assert_array_equal(crop_variant(F, ds, img, g, pad, tx=-3), rect(0, 3))
    np.testing.assert_array_equal(crop_variant(F, ds, img, g, pad, ty=4), rect(-4, 0))
    np.testing.assert_array_equal(crop_variant(F, ds, img, g, pad, ty=-4, tx=2), rect(4, -2))
    np.testing.assert_array_equal(crop_variant(F, ds, img, g, pad, flip=1), rect(0, 0)[:, ::-1])
    assert not np.array_equal(rect(0, -4), rect(0, 0))
    # and through the resize, by the chain
    d = descriptor(ds, Hr + 2 * pad, Wr + 2 * pad)
    got = F.variants_np(img, g["inv"], g["rect"], pad, d, [0], F.noise_scale(0.0), 1, 64)
    np.testing.assert_array_equal(got[0], F.resize_np(rect(0, 0), 64))


def test_a_shift_differs_from_the_face_modes_where_the_padding_leaves_the_image(F, ds):
    """What the feature adds.  The shifted variant of the crop mode holds the rectangle's real neighbours; the face mode's, of the same
    draw, replicates the finished face's edge."""
    Hs, Ws, pad, S = 61, 83, 30, 32
    img, g = tilted_face(F, Hs, Ws, 9.0)
    y0, x0, Hr, Wr = g["rect"]
    assert max(F.crop_pads(Hs, Ws, g["rect"], pad)) > 0 and x0 >= 4
    draw = one_draw(tx=4)
    crop = F.variants_np(img, g["inv"], g["rect"], pad, ds.augment_descriptors(1, Hr + 2 * pad, Wr + 2 * pad, draw), [0], F.noise_scale(0.0), 1, S)[0]
    np.testing.assert_array_equal(crop, F.resize_np(F.warp_rect_np(img, g["inv"], (y0, x0 - 4, Hr, Wr)), S))
    face = F.resize_np(F.warp_rect_np(img, g["inv"], g["rect"]), S)
    v = ds.augment_images(face[None], ds.augment_descriptors(1, S, S, draw), 0.0, 1, 0).transpose(0, 2, 3, 1)[0]
    face_mode = (v * np.float32(255.0) + np.float32(0.5)).astype(np.int32).astype(np.uint8)
    np.testing.assert_array_equal(face_mode[:, :4], np.repeat(face[:, :1], 4, axis=1))       # the smeared edge
    assert not np.array_equal(crop[:, :4], face_mode[:, :4])


def clamp_case(F):
    """A 97 x 131 source, a 40 x 36 rectangle, pad 2, and a descriptor chosen by the test: the inverse of a zoom to one half about the
    padded crop's centre with tx = ty = 4, x = 2 x' - (c + 8) per axis - whole source positions that leave the padded crop below 0 and
    above its last sample on both axes."""
    rs = np.random.RandomState(12)
    img = rs.randint(0, 256, (97, 131, 3)).astype(np.uint8)
    geom = dict(inv=np.array([1, 0, 0, 0, 1, 0], np.float32), rect=(20, 30, 40, 36))
    pad, Hp, Wp = 2, 44, 40
    desc = np.array([[2, 0, -(Wp // 2 + 8), 0, 2, -(Hp // 2 + 8), 1, 0]], np.float32)
    m = desc[0].astype(np.float64)
    ys, xs = np.mgrid[pad:pad + 40, pad:pad + 36]
    sx, sy = m[0] * xs + m[1] * ys + m[2], m[3] * xs + m[4] * ys + m[5]
    assert sx.min() < 0 and sx.max() > Wp - 1 and sy.min() < 0 and sy.max() > Hp - 1
    P = F.padded_crop_np(img, geom["inv"], geom["rect"], pad)
    np.testing.assert_array_equal(P, img[18:62, 28:68])
    want = P[np.clip(sy, 0, Hp - 1).astype(int), np.clip(sx, 0, Wp - 1).astype(int)]       # edge replication of the crop
    return img, geom, pad, desc, want


def test_positions_beyond_the_padded_crop_replicate_its_edge(F):
    img, geom, pad, desc, want = clamp_case(F)
    q = F.variant_pixels_np(F.padded_crop_np(img, geom["inv"], geom["rect"], pad), 1.0, 0, 0.0, 1, 0)
    np.testing.assert_array_equal(F.variant_warp_np(q, desc[0, :6], pad), want)
    got = F.variants_np(img, geom["inv"], geom["rect"], pad, desc, [0], F.noise_scale(0.0), 1, 16)
    np.testing.assert_array_equal(got[0], F.resize_np(want, 16))


def test_pixel_stage_keys_the_noise_by_position_and_base(F, ds):
    rs = np.random.RandomState(5)
    P = rs.randint(0, 256, (9, 7, 3)).astype(np.uint8)
    s = F.noise_scale(0.02)
    assert s.dtype == np.float32 and s == np.float32(5.1)
    q = F.variant_pixels_np(P, 1.1, 1, s, 77, 5 << 32)
    j = np.arange(P.size).reshape(P.shape)
    v = P[:, ::-1].astype(np.float32) * np.float32(1.1) + s * ds.augment_noise(77, 5 << 32, j)
    np.testing.assert_array_equal(q, np.clip(v, 0, 255).astype(np.uint8))
    assert not np.array_equal(q, F.variant_pixels_np(P, 1.1, 1, s, 77, 6 << 32))
    assert (F.variant_pixels_np(P, np.nan, 0, 0.0, 1, 0) == 0).all() and (F.variant_pixels_np(np.maximum(P, 1), 300.0, 0, 0.0, 1, 0) == 255).all()


# ---------------------------------------------------------------- the front end
def test_generate_dataset_host_variants_from_the_crop(F, tmp_path, monkeypatch):
    H.make_tree(F, str(tmp_path / "raw"))
    argv = ["--path", str(tmp_path / "raw"), "--host", "--augmentations", "2"]
    crop = argv + ["--variantsFrom", "crop"]
    assert H.run_front_end(crop + ["--out", str(tmp_path / "a")]) == (10, 2)
    assert H.run_front_end(crop + ["--out", str(tmp_path / "b"), "--threads", "3"]) == (10, 2)
    assert H.run_front_end(argv + ["--out", str(tmp_path / "f")]) == (10, 2)
    G = importlib.import_module("generate_dataset")
    monkeypatch.setattr(G, "BATCH_BYTES", 1)                   # every face is its own batch
    monkeypatch.setattr(G, "VARIANT_BYTES", 1)
    assert H.run_front_end(crop + ["--out", str(tmp_path / "c")]) == (10, 2)
    names = {"out_unaug_64x64": [f"{i:06d}_000.jpg" for i in range(10)],
             "out_aug_64x64": [f"{i:06d}_{a:03d}.jpg" for i in range(10) for a in range(3)]}
    same = lambda x, y, d, n: filecmp.cmp(tmp_path / x / d / n, tmp_path / y / d / n, shallow=False)
    for d, want in names.items():
        assert sorted(os.listdir(tmp_path / "a" / d)) == want
        for n in want:
            assert same("a", "b", d, n) and same("a", "c", d, n), f"{d}/{n}"
            if n.endswith("_000.jpg"):
                assert same("a", "f", d, n), f"{d}/{n}"          # _000 and out_unaug do not depend on the mode
    assert sum(not same("a", "f", "out_aug_64x64", n) for n in names["out_aug_64x64"]) == 20      # every variant does


def test_generate_dataset_new_flags(tmp_path):
    sys.path.insert(0, ROOT)
    G = importlib.import_module("generate_dataset")
    o = G.parse(["--path", "x"])
    assert (o.variantsFrom, o.padding) == ("face", 30)
    o = G.parse(["--path", "x", "--variantsFrom", "crop", "--padding", "0"])
    assert (o.variantsFrom, o.padding) == ("crop", 0) and G.parse(["--path", "x", "--padding", "64"]).padding == 64
    for bad in (["--padding", "-1"], ["--padding", "65"], ["--variantsFrom", "image"]):
        with pytest.raises(SystemExit):
            G.parse(["--path", "x"] + bad)
