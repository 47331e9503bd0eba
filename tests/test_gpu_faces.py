"""The face extraction on the MI355X: cg_faces_u8_extract bit-equal to faces.extract_faces_np's pixel stages (whose own yardsticks are
in tests/test_faces_host.py) over mixed batches, its edge cases, the level-eyes face against Pillow directly, its argument checks, and
generate_dataset.py on the device against --host, file by file.  Every comparison is exact."""
import filecmp
import importlib
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

import test_faces_host as H

pytestmark = pytest.mark.gpu
SOURCES = [(61, 83), (97, 131), (200, 160), (375, 500)]      # Hs, Ws; one 700 x 700 joins every batch of five or more
# per source: the rectangles (Hr, Wr) cut out of it.  33 -> 64 enlarges, 64 -> 64 has the identity taps, 203 -> 64 is a non-integer
# shrink (ksize 9), 641 -> 64 a large one (ksize 23); two are not square, which the entry point allows though the front end makes none
RECTS = {(61, 83): [(33, 33), (40, 61)], (97, 131): [(64, 64), (50, 90)], (200, 160): [(64, 64), (150, 128)],
         (375, 500): [(203, 203), (203, 120)], (700, 700): [(641, 641)]}


@pytest.fixture(scope="module")
def cg():
    assert torch.cuda.is_available()
    return importlib.import_module("cat-generator_amd")


@pytest.fixture(scope="module")
def F():
    return importlib.import_module("cat-generator_amd.faces")


def tilted(deg, cy, cx, ty=0.0, tx=0.0):
    """the six fp32 inverse entries of a rotation by deg about (cx, cy) followed by a shift"""
    r = math.radians(deg)
    c, s = math.cos(r), math.sin(r)
    fwd = np.array([[c, -s, cx - c * cx + s * cy + tx], [s, c, cy - s * cx - c * cy + ty], [0, 0, 1]])
    return np.linalg.inv(fwd)[:2].reshape(6).astype(np.float32)


@pytest.fixture(scope="module")
def batches(F):
    """N -> (images, geometries, the warped rectangles of the host restatement): computed once, read by every target size"""
    out = {}
    for N in (1, 5, 300):
        rs = np.random.RandomState(N)
        pics = {s: rs.randint(0, 256, s + (3,)).astype(np.uint8) for s in SOURCES + [(700, 700)]}
        images, geoms = [], []
        for n in range(N):
            size = (700, 700) if (n == 4 and N >= 5) else SOURCES[n % 4] if N > 1 else (375, 500)
            Hs, Ws = size
            Hr, Wr = RECTS[size][(n // 4) % len(RECTS[size])]
            y0, x0 = int(rs.randint(0, Hs - Hr + 1)), int(rs.randint(0, Ws - Wr + 1))
            inv = tilted((0.0, 9.0, -14.0, 25.0)[(n // 2) % 4], Hs // 2, Ws // 2, ty=rs.randint(-5, 6), tx=rs.randint(-5, 6))
            images.append(pics[size])
            geoms.append(dict(inv=inv, rect=(y0, x0, Hr, Wr)))
        out[N] = (images, geoms, [F.warp_rect_np(im, g["inv"], g["rect"]) for im, g in zip(images, geoms)])
    return out


# ---------------------------------------------------------------- kernel against the host restatement
@pytest.mark.parametrize("out", [64, 32, 16])
@pytest.mark.parametrize("N", [1, 5, 300])
def test_kernel_equals_the_host_restatement_bit_for_bit(cg, F, batches, N, out):
    images, geoms, warped = batches[N]
    got = F.extract_faces_device(images, geoms, out)
    assert got.shape == (N, out, out, 3) and got.dtype == np.uint8
    for n in range(N):
        np.testing.assert_array_equal(got[n], F.resize_np(warped[n], out, out), err_msg=f"face {n}: {geoms[n]['rect']} of {images[n].shape}")


# ---------------------------------------------------------------- edges
def test_borders_corner_tilt_and_nan(cg, F):
    rs = np.random.RandomState(9)
    Hs, Ws = 97, 131
    img = rs.randint(0, 256, (Hs, Ws, 3)).astype(np.uint8)
    ident = tilted(0.0, 0, 0)
    geoms = [dict(inv=ident, rect=r) for r in ((0, 20, 40, 40), (57, 20, 40, 40), (20, 0, 40, 40), (20, 91, 40, 40), (0, 0, 97, 131))]
    # 45 degrees about a point near the top left corner, and near the bottom right one: source positions leave the image on both axes,
    # below 0 and above the last sample, so both clamps of both axes run
    geoms += [dict(inv=tilted(45.0, 6, 8), rect=(0, 0, 48, 48)), dict(inv=tilted(45.0, 90, 122), rect=(49, 83, 48, 48))]
    for g, low in zip(geoms[-2:], (True, False)):
        m = g["inv"].astype(np.float64)
        y0, x0, Hr, Wr = g["rect"]
        ys, xs = np.mgrid[y0:y0 + Hr, x0:x0 + Wr]
        sx, sy = m[0] * xs + m[1] * ys + m[2], m[3] * xs + m[4] * ys + m[5]
        assert ((sx < 0).any() and (sy < 0).any()) if low else ((sx > Ws - 1).any() and (sy > Hs - 1).any())
    for k in (0, 2, 4):                                       # a NaN entry: that axis reads sample 0 everywhere, by the clamp
        m = tilted(9.0, 48, 65).copy()
        m[k] = np.nan
        geoms.append(dict(inv=m, rect=(10, 10, 40, 40)))
    got = F.extract_faces_device([img] * len(geoms), geoms, 64)
    for n, g in enumerate(geoms):
        np.testing.assert_array_equal(got[n], F.resize_np(F.warp_rect_np(img, g["inv"], g["rect"]), 64, 64), err_msg=f"case {n}")
    np.testing.assert_array_equal(got[4], np.asarray(Image.fromarray(img).resize((64, 64), Image.BILINEAR)))      # identity warp, whole image


# ---------------------------------------------------------------- level eyes, against Pillow directly
@pytest.mark.parametrize("Hs,Ws", [(97, 131), (61, 83)])
def test_level_eyes_face_equals_shift_crop_and_pillow(cg, F, Hs, Ws):
    img, kp, crop = H.level_eyes_case(F, Hs, Ws)
    g = F.face_geometry(kp, Hs, Ws)
    for out in (64, 32):
        want = np.asarray(Image.fromarray(crop).resize((out, out), Image.BILINEAR))
        np.testing.assert_array_equal(F.extract_faces_device([img], [g], out)[0], want)


# ---------------------------------------------------------------- argument checks
def test_bad_arguments_are_refused_before_any_launch(cg, F):
    shapes = [(97, 131), (61, 83)]
    geoms = [dict(inv=tilted(9.0, 48, 65), rect=(10, 20, 64, 64)), dict(inv=tilted(0.0, 0, 0), rect=(5, 5, 33, 40))]
    d = F.pack_descriptors(shapes, geoms, 64)
    N, out = 2, 64
    nsrc = sum(h * w * 3 for h, w in shapes)
    wsb = F.workspace_bytes(N, out, d["rows"])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    src, ws = torch.zeros(nsrc, dtype=torch.uint8).cuda(), torch.zeros(wsb, dtype=torch.uint8).cuda()
    dst = torch.full((N, out, out, 3), 7, dtype=torch.uint8).cuda()
    call, s = cg.lib().faces_u8_extract, cg.tensor.stream()

    def args(**kw):
        """the valid call with some descriptor arrays / scalars replaced"""
        a = dict(d, src=src.data_ptr(), src_bytes=nsrc, dst=dst.data_ptr(), N=N, out=out, ws=ws.data_ptr(), wsb=wsb, ntaps=d["taps"].size)
        a.update(kw)
        keep = [up(a[k]) if isinstance(a[k], np.ndarray) else None for k in ("src_off", "geom", "inv", "taps", "tap_off")]
        ptr = lambda k, t: t.data_ptr() if t is not None else a[k]
        p = [ptr(k, t) for k, t in zip(("src_off", "geom", "inv", "taps", "tap_off"), keep)]
        return keep, (s, a["src"], a["src_bytes"], p[0], p[1], p[2], p[3], a["ntaps"], p[4], a["dst"], a["N"], a["out"], a["ws"], a["wsb"])

    def geom(f, col, v):
        g = d["geom"].copy()
        g[f, col] = v
        return g

    bad_bounds = d["taps"].copy()
    bad_bounds[int(d["tap_off"][0, 0]) + 2 * 63] = 64          # the last horizontal sample of face 0 would read past its side
    cases = [(dict(src=None), "null pointer"), (dict(src_off=None), "null pointer"), (dict(geom=None), "null pointer"),
             (dict(inv=None), "null pointer"), (dict(taps=None), "null pointer"), (dict(tap_off=None), "null pointer"),
             (dict(dst=None), "null pointer"), (dict(ws=None), "null pointer"),
             (dict(N=0), "N = 0"), (dict(N=-3), "N = -3"), (dict(out=7), "out = 7"), (dict(out=129), "out = 129"),
             (dict(geom=geom(0, 0, 7)), "source is outside"), (dict(geom=geom(1, 1, 8193)), "source is outside"),
             (dict(geom=geom(0, 4, 7)), "rectangle is outside"), (dict(geom=geom(1, 5, 4097)), "rectangle is outside"),
             (dict(geom=geom(0, 2, 34)), "not inside its"), (dict(geom=geom(1, 3, 44)), "not inside its"), (dict(geom=geom(0, 2, -1)), "not inside its"),
             (dict(geom=geom(0, 6, 5)), "ksize"), (dict(geom=geom(1, 7, 5)), "ksize"),
             (dict(src_bytes=nsrc - 1), "does not fit the"), (dict(ntaps=d["taps"].size - 1), "does not fit the"),
             (dict(taps=bad_bounds), "reads \\["), (dict(wsb=wsb - 16 * N - 48 - 1), "workspace")]
    for kw, message in cases:
        keep, a = args(**kw)
        with pytest.raises(cg.CatganError, match="cg_faces_u8_extract: .*" + message):
            call(*a)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 7).all()                     # nothing was launched
    keep, a = args()
    call(*a)                                                  # and the unmodified call is accepted
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0).all()                     # a black source


# ---------------------------------------------------------------- the front end
def test_generate_dataset_on_the_device_equals_host(cg, F, tmp_path):
    H.make_tree(F, str(tmp_path / "raw"))
    argv = ["--path", str(tmp_path / "raw"), "--augmentations", "2"]
    assert H.run_front_end(argv + ["--out", str(tmp_path / "host"), "--host"]) == (10, 2)
    assert H.run_front_end(argv + ["--out", str(tmp_path / "dev")]) == (10, 2)
    for d in ("out_aug_64x64", "out_unaug_64x64"):
        names = sorted(os.listdir(tmp_path / "host" / d))
        assert names == sorted(os.listdir(tmp_path / "dev" / d)) and len(names) == (30 if "_aug" in d else 10)
        for n in names:
            assert filecmp.cmp(tmp_path / "host" / d / n, tmp_path / "dev" / d / n, shallow=False), f"{d}/{n}"


def test_generate_dataset_pack_feeds_the_loaders(cg, F, tmp_path):
    """--scale 32 --pack: dataset.openPack accepts the directory, and the pools of the resident loader over it are the file loader's."""
    ds = importlib.import_module("cat-generator_amd.dataset")
    H.make_tree(F, str(tmp_path / "raw"))
    assert H.run_front_end(["--path", str(tmp_path / "raw"), "--out", str(tmp_path / "o"), "--scale", "32", "--augmentations", "0", "--pack"]) == (10, 2)
    d = str(tmp_path / "o" / "out_aug_32x32")
    try:
        ds.setDirs([d]); ds.setFileExtension("jpg"); ds.setHeight(32); ds.setWidth(32)
        ds.colorSpace = "rgb"
        pack = ds.openPack(d)
        assert pack is not None
        rset = ds.ResidentSet(pack)
        assert (rset.M, rset.Hs, rset.Ws) == (10, 32, 32)
        ds.seed(5)
        want = ds.loadRandomImages(8).scaled
        ds.seed(5)
        ld = ds.ResidentLoader(8, rset)
        np.testing.assert_array_equal(cg.nn.as_nhwc(ld.next()).numpy(), want)
        ld.close()
        rset.close()
    finally:
        ds.seed(1)
