"""CPU checks of the padded face set and of the augmentation out of it (dataset.margin): augment_images(margin=0) against a frozen copy
of the arithmetic it had before it took a margin; whole-pixel shifts, the identity and the flip as exact consequences (real neighbours,
the window, the mirrored window); the margin that AUG_DEFAULTS needs at 64 x 64; faces.padded_face_np against the _000 face and numpy's
median pad; generate_dataset.py --margin over a synthetic raw tree; setDirs / margin.json and the blocking loader over a padded
directory.  Every comparison is exact."""
import filecmp
import importlib
import json
import os
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 1, 0], np.float32)


@pytest.fixture()
def ds():
    d = importlib.import_module("cat-generator_amd.dataset")
    yield d
    d.setAugmentation(False)
    d.setDirs([])
    d.colorSpace = "rgb"
    d.setHeight(32); d.setWidth(32)
    d.seed(1)


@pytest.fixture(scope="module")
def F():
    return importlib.import_module("cat-generator_amd.faces")


def draw_of(ds, rows, noise_std=0.0, seed=7):
    """A draw dict from rows of (scale, rotation, tx, ty, brightness, flip)."""
    cols = list(zip(*rows))
    return dict(scale=cols[0], rotation=cols[1], tx=cols[2], ty=cols[3], brightness=cols[4], flip=cols[5], noise_std=noise_std, seed=seed)


# ---------------------------------------------------------------- 1. margin 0 is the arithmetic as it was
def augment_images_before(ds, u8_batch, desc, noise_std, seed, offset, index0=0):
    """dataset.augment_images as it stood before it took a margin, frozen here line by line."""
    f32 = np.float32
    u8_batch, desc = np.asarray(u8_batch), np.asarray(desc, dtype=f32)
    N, Hs, Ws, _ = u8_batch.shape
    sigma = f32(noise_std)
    out = np.empty((N, 3, Hs, Ws), f32)
    xs, ys = np.arange(Ws, dtype=f32)[None, :], np.arange(Hs, dtype=f32)[:, None]
    per = Hs * Ws * 3
    for n in range(N):
        m00, m01, m02, m10, m11, m12, bright, flip = desc[n]
        im = u8_batch[n, :, ::-1] if flip != 0 else u8_batch[n]
        p = (im.astype(f32) / f32(255.0)) * bright
        if sigma != 0:
            j = np.arange(per, dtype=np.uint64).reshape(Hs, Ws, 3) + np.uint64((int(index0) + n) * per)
            p = p + sigma * ds.augment_noise(seed, offset, j)
        p = np.where(p < f32(0), f32(0), p)
        p = np.where(p > f32(1), f32(1), p).astype(f32)
        x0, x1, fx = ds._warp_taps((m00 * xs + m01 * ys) + m02, Ws)
        y0, y1, fy = ds._warp_taps((m10 * xs + m11 * ys) + m12, Hs)
        fx, fy = fx[..., None], fy[..., None]
        gx, gy = f32(1) - fx, f32(1) - fy
        top = gx * p[y0, x0] + fx * p[y0, x1]
        bot = gx * p[y1, x0] + fx * p[y1, x1]
        out[n] = (gy * top + fy * bot).transpose(2, 0, 1)
    return out


@pytest.mark.parametrize("Hs,Ws,N", [(64, 64, 3), (17, 23, 5), (9, 40, 2)])
def test_margin_0_is_the_arithmetic_as_it_was(ds, Hs, Ws, N):
    rs = np.random.RandomState(Hs)
    u8 = rs.randint(0, 256, size=(N, Hs, Ws, 3)).astype(np.uint8)
    ds.seed(Hs)
    ds.setAugmentation(True)
    desc = ds.augment_descriptors(N, Hs, Ws)
    for sigma in (0.0, 0.02):
        want = augment_images_before(ds, u8, desc, sigma, 99, 12345, index0=4)
        np.testing.assert_array_equal(ds.augment_images(u8, desc, sigma, 99, 12345, index0=4), want)
        np.testing.assert_array_equal(ds.augment_images(u8, desc, sigma, 99, 12345, index0=4, margin=0), want)


# ---------------------------------------------------------------- 2. exact consequences
@pytest.mark.parametrize("Hp,Wp,m", [(24, 24, 4), (21, 30, 3)])
def test_whole_pixel_shifts_show_real_neighbours(ds, Hp, Wp, m):
    """A pure shift reads source (X - tx, Y - ty) with every fraction exactly 0: the padded image's own pixels / 255, and as long as
    |t| <= margin none of them is a clamped one.  The same draw on the cropped window repeats its edge instead."""
    P = np.random.RandomState(Hp).randint(0, 256, size=(Hp, Wp, 3)).astype(np.uint8)
    Hs, Ws = Hp - 2 * m, Wp - 2 * m
    win = P[m:m + Hs, m:m + Ws]
    f = lambda a: a.astype(np.float32).transpose(2, 0, 1) / np.float32(255.0)
    shifts = [(m, 0), (-m, 0), (0, m), (0, -m), (m, -m), (-m, m), (1, 2), (-2, 1)]
    draw = draw_of(ds, [(1.0, 0, tx, ty, 1.0, 0) for tx, ty in shifts])
    for i, (tx, ty) in enumerate(shifts):
        got = ds.augment_images(P[None], ds.augment_descriptor(draw, i, Hp, Wp)[None], 0.0, 7, 0, margin=m)[0]
        assert got.shape == (3, Hs, Ws)
        np.testing.assert_array_equal(got, f(P[m - ty:m - ty + Hs, m - tx:m - tx + Ws]), err_msg=f"shift {tx},{ty}")
        plain = ds.augment_images(win[None], ds.augment_descriptor(draw, i, Hs, Ws)[None], 0.0, 7, 0)[0]
        ys, xs = np.clip(np.arange(Hs) - ty, 0, Hs - 1), np.clip(np.arange(Ws) - tx, 0, Ws - 1)
        np.testing.assert_array_equal(plain, f(win[ys][:, xs]), err_msg=f"shift {tx},{ty}, no margin")      # replicated edges
        assert not np.array_equal(got, plain)
        inner = (slice(None), slice(abs(ty), Hs - abs(ty)), slice(abs(tx), Ws - abs(tx)))
        np.testing.assert_array_equal(got[inner], plain[inner])
    ident = ds.augment_images(P[None], IDENTITY[None], 0.0, 7, 0, margin=m)[0]
    np.testing.assert_array_equal(ident, f(win))
    flip = IDENTITY.copy()
    flip[7] = 1
    np.testing.assert_array_equal(ds.augment_images(P[None], flip[None], 0.0, 7, 0, margin=m)[0], f(win[:, ::-1]))


def test_a_margin_without_a_window_is_refused(ds):
    P = np.zeros((1, 8, 10, 3), np.uint8)
    for m in (4, 5, -1):
        with pytest.raises(ValueError, match="margin"):
            ds.augment_images(P, IDENTITY[None], 0.0, 1, 0, margin=m)
    assert ds.augment_images(P, IDENTITY[None], 0.0, 1, 0, margin=3).shape == (1, 3, 2, 4)


# ---------------------------------------------------------------- 3. the margin the default ranges need
def tap_range(ds, S, m):
    """The smallest and largest source coordinate, as the kernel computes it in fp32 before the clamp, that a window pixel of an
    S x S face with margin m reads over AUG_DEFAULTS' ranges.  The coordinate is affine in the pixel position and in the shift, so the
    four window corners and tx, ty = +-T bound it; it falls with the zoom at a corner, so the zoom's two ends do; every whole degree
    of the rotation range is tried."""
    a, f32 = ds.AUG_DEFAULTS, np.float32
    R, T = a["rotation"], a["translation"]
    rows = [(s, r, tx, ty, 1.0, 0) for s in a["scale"] for r in range(-R, R + 1) for tx in (-T, T) for ty in (-T, T)]
    draw = draw_of(ds, rows)
    L = S + 2 * m
    lo, hi = np.inf, -np.inf
    for i in range(len(rows)):
        m00, m01, m02, m10, m11, m12 = ds.augment_descriptor(draw, i, L, L)[:6]
        for X in (f32(m), f32(m + S - 1)):
            for Y in (f32(m), f32(m + S - 1)):
                for v in ((m00 * X + m01 * Y) + m02, (m10 * X + m11 * Y) + m12):
                    lo, hi = min(lo, float(v)), max(hi, float(v))
    return lo, hi, L - 1


def test_the_default_ranges_stay_inside_a_margin_of_12_at_64(ds):
    lo, hi, last = tap_range(ds, 64, 12)
    print(f"margin 12: source coordinates in [{lo:.2f}, {hi:.2f}] of [0, {last}]")
    assert 0.0 <= lo and hi <= last
    lo, hi, last = tap_range(ds, 64, 11)
    print(f"margin 11: source coordinates in [{lo:.2f}, {hi:.2f}] of [0, {last}]")
    assert lo < 0.0 or hi > last
    assert (64 + 2 * 12) ** 2 * 12 <= ds.AUG_LDS_BYTES


# ---------------------------------------------------------------- 4. padded_face_np
def test_margin_pad(F):
    assert [F.margin_pad(Hr, 12, 64) for Hr in (64, 128, 100, 8, 65, 67)] == [12, 24, 19, 2, 12, 13]      # 18.75, 1.5, 12.19, 12.56 rounded
    assert F.margin_pad(40, 4, 16) == 10 and F.margin_pad(64, 0, 64) == 0


def test_padded_face_at_unit_scale_holds_the_face_in_its_window(F):
    rs = np.random.RandomState(5)
    img = rs.randint(0, 256, (90, 120, 3)).astype(np.uint8)
    c, s = np.cos(0.2), np.sin(0.2)
    inv = np.array([c, -s, 8.0, s, c, -6.0], np.float32)
    for out, m, rect in ((32, 6, (30, 40, 32, 32)), (16, 4, (0, 0, 16, 16)), (24, 5, (66, 96, 24, 24))):      # inside, top-left corner, bottom-right corner
        Pf = F.padded_face_np(img, inv, rect, m, out)
        assert Pf.shape == (out + 2 * m, out + 2 * m, 3) and Pf.dtype == np.uint8
        face = F.resize_np(F.warp_rect_np(img, inv, rect), out)
        np.testing.assert_array_equal(Pf[m:m + out, m:m + out], face)


def test_padded_face_at_the_image_corner_gets_the_median_fill(F):
    rs = np.random.RandomState(6)
    img = rs.randint(0, 256, (90, 120, 3)).astype(np.uint8)
    inv = np.array([1, 0, 0, 0, 1, 0], np.float32)
    out, m, rect = 16, 4, (0, 0, 40, 40)
    pad = F.margin_pad(40, m, out)
    assert pad == 10
    clipped = F.warp_rect_np(img, inv, (0, 0, 40 + pad, 40 + pad))
    want = F.resize_np(np.pad(clipped, ((pad, 0), (pad, 0), (0, 0)), mode="median"), out + 2 * m)
    np.testing.assert_array_equal(F.padded_face_np(img, inv, rect, m, out), want)
    rect = (50, 80, 40, 40)      # the other corner: bottom and right
    clipped = F.warp_rect_np(img, inv, (40, 70, 50, 50))
    want = F.resize_np(np.pad(clipped, ((0, pad), (0, pad), (0, 0)), mode="median"), out + 2 * m)
    np.testing.assert_array_equal(F.padded_face_np(img, inv, rect, m, out), want)


# ---------------------------------------------------------------- 5. the front end
TREE_SIZES = [(61, 83), (97, 131), (200, 160), (97, 131), (131, 97), (120, 90)]


def run_front_end(argv):
    sys.path.insert(0, ROOT)
    G = importlib.import_module("generate_dataset")
    d = importlib.import_module("cat-generator_amd.dataset")
    try:
        return G.main(argv)
    finally:
        d.setAugmentation(False)
        d.setDirs([])
        d.seed(1)


def test_generate_dataset_margin_over_a_synthetic_tree(F, tmp_path):
    files = F.write_raw_tree(str(tmp_path / "raw"), TREE_SIZES)
    argv = ["--path", str(tmp_path / "raw"), "--host", "--scale", "16", "--augmentations", "1"]
    n = len(files)
    assert run_front_end(argv + ["--margin", "4", "--out", str(tmp_path / "a")]) == (n, 0)
    assert run_front_end(argv + ["--margin", "4", "--out", str(tmp_path / "b"), "--threads", "3"]) == (n, 0)
    assert run_front_end(argv + ["--out", str(tmp_path / "c")]) == (n, 0)
    name = "out_padded_16x16_m4"
    assert sorted(os.listdir(tmp_path / "a")) == ["out_aug_16x16", name, "out_unaug_16x16"]
    assert sorted(os.listdir(tmp_path / "c")) == ["out_aug_16x16", "out_unaug_16x16"]
    assert sorted(os.listdir(tmp_path / "a" / name)) == [f"{i:06d}_000.jpg" for i in range(n)] + ["margin.json"]
    with open(tmp_path / "a" / name / "margin.json") as f:
        assert json.load(f) == {"margin": 4, "side": 16}
    for i, fp in enumerate(files):
        assert Image.open(tmp_path / "a" / name / f"{i:06d}_000.jpg").size == (24, 24)
    for d in (name, "out_aug_16x16", "out_unaug_16x16"):      # two runs: the same bytes; and the margin changes nothing else
        for f in os.listdir(tmp_path / "a" / d):
            assert filecmp.cmp(tmp_path / "a" / d / f, tmp_path / "b" / d / f, shallow=False), (d, f)
            if d != name:
                assert filecmp.cmp(tmp_path / "a" / d / f, tmp_path / "c" / d / f, shallow=False), (d, f)
        if d != name:
            assert sorted(os.listdir(tmp_path / "a" / d)) == sorted(os.listdir(tmp_path / "c" / d))
    # a file is padded_face_np through Pillow's default JPEG settings
    import io
    img = np.asarray(Image.open(files[1]).convert("RGB"))
    with open(files[1] + ".cat") as f:
        g = F.face_geometry(F.parse_cat(f.read(), img.shape[0], img.shape[1]), img.shape[0], img.shape[1])
    buf = io.BytesIO()
    Image.fromarray(F.padded_face_np(img, g["inv"], g["rect"], 4, 16)).save(buf, format="JPEG")
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "a" / name / "000001_000.jpg")), np.asarray(Image.open(io.BytesIO(buf.getvalue()))))


def test_generate_dataset_refuses_a_margin_beyond_the_lds(tmp_path):
    os.makedirs(tmp_path / "CAT_00")
    sys.path.insert(0, ROOT)
    G = importlib.import_module("generate_dataset")
    assert G.parse(["--path", "x"]).margin == 0
    with pytest.raises(SystemExit):
        G.parse(["--path", "x", "--margin", "-1"])
    with pytest.raises(SystemExit, match="largest margin that fits 64 x 64 faces is 26"):      # 116 x 116 x 12 = 161472 <= 163840 < 118 x 118 x 12
        run_front_end(["--path", str(tmp_path), "--host", "--margin", "27", "--out", str(tmp_path / "o")])
    with pytest.raises(SystemExit, match="no CAT"):      # 26 passes the check
        run_front_end(["--path", str(tmp_path), "--host", "--margin", "26", "--out", str(tmp_path / "o")])
    with pytest.raises(SystemExit, match="no CAT"):      # without a margin the check does not apply: every --scale works as before
        run_front_end(["--path", str(tmp_path), "--host", "--scale", "128", "--augmentations", "0", "--out", str(tmp_path / "o")])
    with pytest.raises(SystemExit, match="no 128 x 128 face fits"):
        run_front_end(["--path", str(tmp_path), "--host", "--scale", "128", "--augmentations", "0", "--margin", "1", "--out", str(tmp_path / "o")])


# ---------------------------------------------------------------- 6. setDirs and the blocking loader
def padded_dirs(tmp_path, n=6, side=24, m=4):
    """A directory of n padded PNGs with its margin.json, and one of their cropped windows under the same names."""
    rs = np.random.RandomState(21)
    pad, win = tmp_path / "padded", tmp_path / "windows"
    os.makedirs(pad); os.makedirs(win)
    for i in range(n):
        P = rs.randint(0, 256, size=(side, side, 3)).astype(np.uint8)
        Image.fromarray(P).save(str(pad / f"{i:03d}.png"))
        Image.fromarray(P[m:side - m, m:side - m]).save(str(win / f"{i:03d}.png"))
    with open(pad / "margin.json", "w") as f:
        json.dump({"margin": m, "side": side - 2 * m}, f)
    return str(pad), str(win)


def test_setdirs_reads_the_margin_and_the_loader_shows_the_window(ds, tmp_path):
    pad, win = padded_dirs(tmp_path)
    ds.setFileExtension("png"); ds.setHeight(8); ds.setWidth(8)
    assert ds.margin == 0
    ds.setDirs([win])
    assert ds.margin == 0
    ds.seed(3)
    want = ds.loadRandomImages(6).scaled
    ds.setDirs([pad])
    assert ds.margin == 4
    assert len(ds.loadPaths()) == 6      # margin.json is not an image
    ds.seed(3)
    np.testing.assert_array_equal(ds.loadRandomImages(6).scaled, want)
    one = ds.loadImageFile(ds.paths[2])      # the un-augmented single-file path: the window too
    ds.setDirs([win])
    np.testing.assert_array_equal(one, ds.loadImageFile(ds.loadPaths()[2]))
    ds.setDirs([pad])
    # augmented: the window warped out of the padded file, not the cropped window warped
    ds.setAugmentation(True, noise_std=0.0)
    ds.seed(3)
    aug_pad = ds.loadRandomImages(6).scaled
    ds.seed(3)
    files = ds._pick(6)
    draw = ds.augment_draw(6)
    for i, fp in enumerate(files):
        u8 = ds._decode(fp)
        d = ds.augment_descriptor(draw, i, 24, 24)
        w = ds.augment_images(u8[None], d[None], 0.0, draw["seed"], 0, index0=i, margin=4)[0]
        np.testing.assert_array_equal(aug_pad[i], ds.image_scale(w, 8, 8))
    ds.setDirs([win])
    ds.seed(3)
    assert not np.array_equal(ds.loadRandomImages(6).scaled, aug_pad)
    # setMargin by hand, and setDirs overwrites it
    ds.setMargin(2)
    assert ds.margin == 2
    ds.setDirs([win])
    assert ds.margin == 0
    with pytest.raises(ValueError):
        ds.setMargin(-1)


def test_setdirs_refuses_disagreeing_or_malformed_margins(ds, tmp_path):
    pad, win = padded_dirs(tmp_path)
    with pytest.raises(ValueError, match="disagree"):
        ds.setDirs([pad, win])
    other = tmp_path / "other"
    os.makedirs(other)
    for text in ("{", "[4]", '{"side": 16}', '{"margin": "4"}', '{"margin": -1}', '{"margin": 1.5}', '{"margin": true}'):
        with open(other / "margin.json", "w") as f:
            f.write(text)
        with pytest.raises(ValueError, match="margin"):
            ds.setDirs([str(other)])
    with open(other / "margin.json", "w") as f:
        f.write('{"margin": 4}')
    ds.setDirs([pad, str(other)])
    assert ds.margin == 4
