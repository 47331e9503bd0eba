"""CPU checks of the face extraction (cat-generator_amd/faces.py, generate_dataset.py --host): the resize stage against Pillow, the
keypoint move against the brute-force white-pixel warp it replaces, the .cat parser, rectangle method 4 against hand-worked answers,
the whole chain against an independent yardstick (level eyes: shift, crop, Pillow), and the front end over a synthetic raw tree.
Every comparison is exact."""
import filecmp
import importlib
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(61, 83), (97, 131), (200, 160), (375, 500)]          # H, W
RESIZE_SIDES = [(17, 17), (40, 40), (63, 63), (64, 64), (65, 65), (97, 97), (128, 128), (131, 131), (200, 200), (301, 301), (513, 513),
                (90, 70), (64, 100)]
TREE_SIZES = [(61, 83), (97, 131), (200, 160), (375, 500), (97, 131), (61, 83), (200, 160), (375, 500), (131, 97), (300, 300), (97, 131),
              (120, 90)]


@pytest.fixture(scope="module")
def F():
    return importlib.import_module("cat-generator_amd.faces")


def image_kinds(rs, h, w):
    """random, binary and ramp images of h x w"""
    ramp = np.broadcast_to((np.arange(w) * 255 // max(w - 1, 1)).astype(np.uint8)[None, :, None], (h, w, 3)).copy()
    return [rs.randint(0, 256, (h, w, 3)).astype(np.uint8), (rs.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8), ramp]


def yx(F, H, W, tilt, **kw):
    """template keypoints as the parser stores them, (y, x)"""
    return F.template_keypoints(H, W, tilt, **kw)[:, ::-1].copy()


def make_tree(F, path):
    """The synthetic raw tree of the front-end tests: twelve images in two CAT_* folders, tilts 0, 9, -14, 25; then image 3 loses its .cat
    file and image 6 gets coincident eyes.  Returns (all files in the front end's order, the files it must accept)."""
    files = F.write_raw_tree(path, TREE_SIZES)
    by_index = {int(os.path.basename(f)[:8]): f for f in files}
    os.remove(by_index[3] + ".cat")
    xy = F.template_keypoints(200, 160, F.TILTS[6 % 4])
    xy[1] = xy[0]
    with open(by_index[6] + ".cat", "w") as f:
        f.write(F.cat_line(xy))
    return files, [f for f in files if f not in (by_index[3], by_index[6])]


def run_front_end(argv):
    sys.path.insert(0, ROOT)
    G = importlib.import_module("generate_dataset")
    ds = importlib.import_module("cat-generator_amd.dataset")
    try:
        return G.main(argv)
    finally:
        ds.setAugmentation(False)
        ds.seed(1)


# ---------------------------------------------------------------- resize
@pytest.mark.parametrize("out", [64, 32, 16])
def test_resize_stage_equals_pillow_bit_for_bit(F, out):
    rs = np.random.RandomState(out)
    for h, w in RESIZE_SIDES:
        for a in image_kinds(rs, h, w):
            want = np.asarray(Image.fromarray(a).resize((out, out), Image.BILINEAR))
            np.testing.assert_array_equal(F.resize_np(a, out), want, err_msg=f"{h}x{w} -> {out}")


def test_tap_tables_have_pillows_shape(F):
    for n_in, n_out, ksize in ((33, 64, 3), (64, 64, 3), (203, 64, 9), (640, 64, 21), (641, 64, 23), (64, 16, 9)):
        bounds, taps = F.resize_taps(n_in, n_out)
        assert taps.shape == (n_out, ksize) == (n_out, F.resample_ksize(n_in, n_out)) and bounds.shape == (n_out, 2)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all() and (bounds[:, 1] <= ksize).all()
        assert (np.abs(taps.sum(1) - (1 << 22)) <= ksize).all()          # each tap is rounded on its own
    bounds, taps = F.resize_taps(64, 64)                                 # equal sizes: the identity
    assert (taps[:, 0] == 1 << 22).all() and (taps[:, 1:] == 0).all() and (bounds[:, 0] == np.arange(64)).all()


# ---------------------------------------------------------------- keypoint move
def brute_force_move(kp, Finv, H, W):
    """Point2D.warp (dataset.py:769-796) as written: a white pixel on a black H x W image, warped with order 1 and constant mode 0 (the
    sample at (sx, sy) blends the four neighbours, those outside the image being 0), arg-max of the result; unchanged when the arg-max
    is pixel 0 with less than 0.5 there."""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    sx = Finv[0, 0] * xs + Finv[0, 1] * ys + Finv[0, 2]
    sy = Finv[1, 0] * xs + Finv[1, 1] * ys + Finv[1, 2]
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    out = np.array(kp, np.int64)
    for i, (py, px) in enumerate(kp):
        img = np.zeros((H + 2, W + 2))                      # one pixel of cval around the image
        img[py + 1, px + 1] = 1.0
        get = lambda yy, xx: np.where((yy >= -1) & (yy <= H) & (xx >= -1) & (xx <= W),
                                      img[np.clip(yy + 1, 0, H + 1).astype(int), np.clip(xx + 1, 0, W + 1).astype(int)], 0.0)
        top = (1 - fx) * get(y0, x0) + fx * get(y0, x0 + 1)
        bot = (1 - fx) * get(y0 + 1, x0) + fx * get(y0 + 1, x0 + 1)
        w = (1 - fy) * top + fy * bot
        k = int(np.argmax(w))
        if not (k == 0 and w[0, 0] < 0.5):
            out[i] = np.unravel_index(k, w.shape)
    return out


@pytest.mark.parametrize("H,W", GEOMETRIES)
def test_keypoint_move_equals_the_white_pixel_warp(F, H, W):
    for tilt in F.TILTS:
        kp = yx(F, H, W, tilt)
        Fm, Finv = F.rotation_maps(kp, H, W)
        np.testing.assert_array_equal(F.move_keypoints(kp, Fm, Finv, H, W), brute_force_move(kp, Finv, H, W), err_msg=f"tilt {tilt}")


def test_a_keypoint_that_leaves_the_image_stays(F):
    H, W = 97, 131
    kp = yx(F, H, W, 25.0)
    kp[8] = (0, W - 1)                                       # the top right corner turns out of the picture
    Fm, Finv = F.rotation_maps(kp, H, W)
    want = brute_force_move(kp, Finv, H, W)
    got = F.move_keypoints(kp, Fm, Finv, H, W)
    np.testing.assert_array_equal(got, want)
    assert tuple(got[8]) == (0, W - 1) and not np.array_equal(got[:8], kp[:8])
    moved = Fm @ np.array([W - 1, 0, 1.0])
    assert not (0 <= moved[0] <= W - 1 and 0 <= moved[1] <= H - 1)


def test_moved_eyes_are_level(F):
    for (H, W) in GEOMETRIES:
        for tilt in F.TILTS:
            g = F.face_geometry(yx(F, H, W, tilt), H, W)
            assert abs(int(g["keypoints"][0, 0]) - int(g["keypoints"][1, 0])) <= 1, (H, W, tilt)


# ---------------------------------------------------------------- parser
def test_parser(F):
    line = "9 10 20 -30 40 500 60 70 900 1 2 3 4 5 6 7 8 9 10 \n"
    kp = F.parse_cat(line, 100, 200)
    assert kp.shape == (9, 2)
    assert tuple(kp[0]) == (20, 10)                          # stored as (y, x)
    assert tuple(kp[1]) == (40, 30)                          # a negative coordinate: abs()
    assert tuple(kp[2]) == (60, 199) and tuple(kp[3]) == (99, 70)      # beyond the image: clipped to W - 1, H - 1
    assert F.parse_cat("9 1 2 3 4 5 6 7 8 9 10 11 12 13 14 15 16 17\n", 100, 200) is None      # a short line: eight and a half points
    assert F.parse_cat("", 100, 200) is None and F.parse_cat("9 a b\n", 100, 200) is None


# ---------------------------------------------------------------- rectangle
def test_rectangle_method_4_known_answers(F):
    """Two answers worked by hand from dataset.py:602-676 and :853-910, in a 100 (H) x 120 (W) image.

    A. eyes (y 30, x 40), (30, 60), mouth (50, 50), the other six points spanning y 20..50, x 30..70.
       rect 0 = y 20..50, x 30..70; its centre (35, 50); face centre (int(110/3), int(150/3)) = (36, 50); diff (1, 0), half (0.5, 0).
       rect 2 = (int(20.5), 30, int(50.5), 70) = (20, 30, 50, 70) = rect 3.  height 30, width 40: ten columns go, five from each side.
       -> (20, 35, 50, 65), 31 x 31 pixels.
    B. eyes (40, 40), (40, 60), mouth (70, 50), the others spanning y 10..70 (a point at y 10), x 35..66.
       rect 0 = y 10..70, x 35..66; centre (40, int(50.5)) = (40, 50); face centre (50, 50); diff (10, 0), half (5, 0).
       rect 2 = (15, 35, 75, 66); rect 3 = (10, 35, 75, 66): height 65, width 31, so 34 rows go - 17 from each end; with the mouth at
       y 71 instead rect 3 = (10, 35, 76, 66), height 66, 35 rows go: 17 from the bottom and 17 + the odd one from the top.
       -> (27, 35, 58, 66) and (28, 35, 59, 66), 32 x 32 pixels each."""
    H, W = 100, 120
    a = np.array([[30, 40], [30, 60], [50, 50], [20, 30], [25, 35], [40, 30], [40, 70], [25, 65], [20, 70]])
    assert F.face_rectangle(a, H, W) == (20, 35, 50, 65)
    b = np.array([[40, 40], [40, 60], [70, 50], [10, 35], [30, 36], [50, 35], [50, 66], [30, 66], [12, 60]])
    assert F.face_rectangle(b, H, W) == (27, 35, 58, 66)
    b[2] = (71, 50)                                           # face centre int(151 / 3) = 50 as before; rect 0 one row taller
    assert F.face_rectangle(b, H, W) == (28, 35, 59, 66)
    assert F.face_rectangle(np.tile([[5, 7]], (9, 1)), H, W) is None           # all points on one pixel: no rectangle


def test_rectangles_are_square_inside_and_inclusive(F):
    rs = np.random.RandomState(4)
    for (H, W) in GEOMETRIES:
        for tilt in F.TILTS:
            for _ in range(4):
                kp = yx(F, H, W, tilt, cy=int(rs.randint(H // 3, 2 * H // 3)), cx=int(rs.randint(W // 3, 2 * W // 3)))
                kp[:, 0], kp[:, 1] = np.clip(kp[:, 0], 0, H - 1), np.clip(kp[:, 1], 0, W - 1)
                g = F.face_geometry(kp, H, W)
                y0, x0, Hr, Wr = g["rect"]
                tl_y, tl_x, br_y, br_x = F.face_rectangle(g["keypoints"], H, W)
                assert Hr == Wr == br_y - tl_y + 1 == br_x - tl_x + 1 and (y0, x0) == (tl_y, tl_x)
                assert 0 <= y0 and 0 <= x0 and y0 + Hr <= H and x0 + Wr <= W
                assert F.warp_rect_np(np.zeros((H, W, 3), np.uint8), g["inv"], g["rect"]).shape == (Hr, Wr, 3)


# ---------------------------------------------------------------- the whole chain, independently
def level_eyes_case(F, H, W):
    """An image whose face has level eyes, its keypoints, and the face rectangle cut out WITHOUT any warp: with level eyes the warp is
    the integer shift image_centre - eyes_centre with edge replication (every fraction is exactly 0, and (u8 / 255) 255 truncates back
    to u8 in fp32), so shifting and cropping is all there is to do before the resize."""
    rs = np.random.RandomState(H)
    img = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    kp = yx(F, H, W, 0.0, cy=H // 2 - 7, cx=W // 2 + 5)
    assert kp[0, 0] == kp[1, 0]
    ecy, ecx = (int(kp[0, 0]) + int(kp[1, 0])) // 2, (int(kp[0, 1]) + int(kp[1, 1])) // 2
    dy, dx = H // 2 - ecy, W // 2 - ecx
    assert dy != 0 and dx != 0
    shifted = img[np.clip(np.arange(H) - dy, 0, H - 1)][:, np.clip(np.arange(W) - dx, 0, W - 1)]
    moved = kp + (dy, dx)                                     # every point stays inside: the move is the shift
    assert (moved >= 0).all() and (moved[:, 0] < H).all() and (moved[:, 1] < W).all()
    tl_y, tl_x, br_y, br_x = F.face_rectangle(moved, H, W)
    return img, kp, shifted[tl_y:br_y + 1, tl_x:br_x + 1]


@pytest.mark.parametrize("H,W", [(97, 131), (61, 83)])
def test_level_eyes_chain_equals_shift_crop_and_pillow(F, H, W):
    """The chain against a yardstick that shares none of its code: shift, crop the rectangle, Pillow-resize (level_eyes_case)."""
    img, kp, crop = level_eyes_case(F, H, W)
    for out in (64, 32):
        want = np.asarray(Image.fromarray(crop).resize((out, out), Image.BILINEAR))
        np.testing.assert_array_equal(F.extract_faces_np([img], [kp], out)[0], want)


def test_extract_refuses_what_the_front_end_skips(F):
    kp = yx(F, 97, 131, 0.0)
    kp[1] = kp[0]
    with pytest.raises(ValueError, match="both eyes"):
        F.extract_faces_np([np.zeros((97, 131, 3), np.uint8)], [kp])


# ---------------------------------------------------------------- the front end
def test_generate_dataset_host_over_a_synthetic_tree(F, tmp_path, capsys):
    files, accepted = make_tree(F, str(tmp_path / "raw"))
    argv = ["--path", str(tmp_path / "raw"), "--host", "--augmentations", "2"]
    assert run_front_end(argv + ["--out", str(tmp_path / "a")]) == (10, 2)
    out = capsys.readouterr().out
    assert out.count("warning") == 2 and "it has no .cat file" in out and "both eyes are on one pixel" in out
    assert run_front_end(argv + ["--out", str(tmp_path / "b"), "--threads", "3"]) == (10, 2)
    aug, unaug = tmp_path / "a" / "out_aug_64x64", tmp_path / "a" / "out_unaug_64x64"
    assert sorted(os.listdir(unaug)) == [f"{i:06d}_000.jpg" for i in range(10)]          # the skips consume no index
    assert sorted(os.listdir(aug)) == [f"{i:06d}_{a:03d}.jpg" for i in range(10) for a in range(3)]
    for d in ("out_aug_64x64", "out_unaug_64x64"):                                       # two runs: the same bytes
        for n in os.listdir(tmp_path / "a" / d):
            assert filecmp.cmp(tmp_path / "a" / d / n, tmp_path / "b" / d / n, shallow=False), n
    for i, fp in enumerate(accepted):                        # _000 = the restatement's face through Pillow's default JPEG settings
        img = np.asarray(Image.open(fp).convert("RGB"))
        with open(fp + ".cat") as f:
            kp = F.parse_cat(f.read(), img.shape[0], img.shape[1])
        buf = io.BytesIO()
        Image.fromarray(F.extract_faces_np([img], [kp], 64)[0]).save(buf, format="JPEG")
        want = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
        for d in (aug, unaug):
            np.testing.assert_array_equal(np.asarray(Image.open(d / f"{i:06d}_000.jpg")), want, err_msg=fp)
    variants = [np.asarray(Image.open(aug / f"000000_{a:03d}.jpg")).astype(int) for a in range(3)]
    assert np.abs(variants[1] - variants[0]).mean() > 1 and np.abs(variants[2] - variants[1]).mean() > 1


def test_generate_dataset_command_line(tmp_path):
    sys.path.insert(0, ROOT)
    G = importlib.import_module("generate_dataset")
    o = G.parse(["--path", "x"])
    assert (o.out, o.scale, o.augmentations, o.threads, o.seed, o.host, o.pack) == ("dataset", 64, 9, 8, 42, False, False)
    for bad in (["--scale", "7"], ["--scale", "129"], ["--threads", "0"], ["--augmentations", "-1"], []):
        with pytest.raises(SystemExit):
            G.parse((["--path", "x"] if bad else []) + bad)
    os.makedirs(tmp_path / "CAT_00")
    with pytest.raises(SystemExit, match="no CAT"):
        G.main(["--path", str(tmp_path), "--host", "--out", str(tmp_path / "o")])
