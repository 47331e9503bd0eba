"""The padded faces on the MI355X: cg_faces_u8_extract_padded bit-equal to faces.padded_face_np (whose own yardsticks are in
tests/test_augment_margin_host.py and tests/test_faces_variants_host.py) over the variants' mixed batch, whose pads leave their images
in every way; pads of the caller's choice through the raw entry point, beyond what the tool derives from a margin; independence of
batch order and split; its argument checks; and generate_dataset.py --margin on the device against --host, file by file.  Every
comparison is exact."""
import filecmp
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

import test_faces_host as H
from test_gpu_faces import tilted
from test_gpu_faces_variants import batch   # noqa: F401 - the fixture: a dozen faces whose padded rectangles leave their images in every way

pytestmark = pytest.mark.gpu
CONFIGS = [(4, 16), (12, 64), (26, 64), (0, 64)]             # (margin, out)
TREE_SIZES = [(61, 83), (97, 131), (200, 160), (97, 131), (131, 97), (120, 90)]


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


def raw_call(cg, F, images, geoms, pads, out):
    """cg_faces_u8_extract_padded with pads of the caller's choice -> uint8 [N, out, out, 3]"""
    d = F.pack_padded_descriptors([im.shape[:2] for im in images], geoms, pads, out)
    N = len(images)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    src_off, src, seen = [], [], {}
    for im in images:                                          # faces may share a source
        if id(im) not in seen:
            seen[id(im)] = sum(a.size for a in src)
            src.append(np.ascontiguousarray(im).reshape(-1))
        src_off.append(seen[id(im)])
    src = up(np.concatenate(src))
    arrs = [up(a) for a in (np.array(src_off, np.uint64), d["geom"], d["inv"], d["taps"], d["tap_off"], d["pads"])]
    wsb = F.padded_workspace_bytes([g["rect"] for g in geoms], pads, out)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    dst = torch.empty((N, out, out, 3), dtype=torch.uint8, device="cuda")
    cg.lib().faces_u8_extract_padded(cg.tensor.stream(), src.data_ptr(), src.numel(), arrs[0].data_ptr(), arrs[1].data_ptr(), arrs[2].data_ptr(),
                                     arrs[3].data_ptr(), d["taps"].size, arrs[4].data_ptr(), arrs[5].data_ptr(), dst.data_ptr(), N, out,
                                     ws.data_ptr(), wsb)
    return dst.cpu().numpy()


# ---------------------------------------------------------------- 1. device against the restatement
def kinds(F, images, geoms, margin, out):
    """how each face's padded rectangle leaves its image: crop_pads (top, left, bottom, right) with the face's own pad"""
    return [F.crop_pads(im.shape[0], im.shape[1], g["rect"], F.margin_pad(g["rect"][2], margin, out)) for im, g in zip(images, geoms)]


@pytest.mark.parametrize("margin,out", CONFIGS)
def test_kernels_equal_the_host_restatement_bit_for_bit(cg, F, batch, margin, out):
    images, geoms = batch[0], batch[1]
    assert len(images) == 12
    if margin:
        k = kinds(F, images, geoms, margin, out)
        assert min(k[5][:2]) > 0 and k[5][2:] == (0, 0)                      # top and left only
        assert k[6][:2] == (0, 0) and min(k[6][2:]) > 0                      # bottom and right only
        assert min(k[11]) > 0 and geoms[11]["rect"] == (0, 0) + images[11].shape[:2]      # the whole image: all four sides
        assert k[10] == (0, 0, 0, 0)                                         # none
        assert geoms[7]["rect"][2:] == (8, 8)                                # the smallest rectangle
        assert geoms[8]["rect"][2] != geoms[8]["rect"][3] and geoms[9]["rect"][2] != geoms[9]["rect"][3]      # the two that are not square
        assert len({F.margin_pad(g["rect"][2], margin, out) for g in geoms}) >= 6          # and the pads differ from face to face
    faces, got = F.extract_padded_device(images, geoms, margin, out, with_faces=True)
    side = out + 2 * margin
    assert got.shape == (12, side, side, 3) and got.dtype == np.uint8 and faces.shape == (12, out, out, 3)
    for n, (im, g) in enumerate(zip(images, geoms)):
        np.testing.assert_array_equal(got[n], F.padded_face_np(im, g["inv"], g["rect"], margin, out), err_msg=f"face {n}: {g['rect']} of {im.shape}")
    np.testing.assert_array_equal(F.extract_padded_device(images, geoms, margin, out), got)           # without the faces: the same
    np.testing.assert_array_equal(faces, F.extract_faces_device(images, geoms, out))
    if margin == 0:
        np.testing.assert_array_equal(got, faces)                                                     # no margin: cg_faces_u8_extract's output


# ---------------------------------------------------------------- 2. pads of the caller's choice
def test_caller_given_pads_through_the_raw_entry(cg, F):
    rs = np.random.RandomState(44)
    img = rs.randint(0, 256, (97, 131, 3)).astype(np.uint8)
    pads = [0, 1, 7, 64, 65]                                   # 65: beyond cg_faces_u8_extract_variants' limit
    geoms = [dict(inv=tilted(9.0, 48, 65), rect=(10, 20, 64, 64))] * len(pads)
    assert F.crop_pads(97, 131, geoms[0]["rect"], 7) == (0, 0, 0, 0) and min(F.crop_pads(97, 131, geoms[0]["rect"], 64)) > 0
    got = raw_call(cg, F, [img] * len(pads), geoms, pads, 48)
    for n, p in enumerate(pads):
        np.testing.assert_array_equal(got[n], F.resize_np(F.padded_crop_np(img, geoms[0]["inv"], geoms[0]["rect"], p), 48), err_msg=f"pad {p}")
    np.testing.assert_array_equal(got[0], F.extract_faces_device([img], geoms[:1], 48)[0])


def test_a_wide_rectangle_that_is_mostly_fill(cg, F):
    """4096 x 8 (width x height) in a 12 x 4100 source with pad 700: padded rows of 5496 pixels, one per band of the horizontal pass,
    and a crop of 1408 rows of which twelve are image"""
    rs = np.random.RandomState(45)
    img = rs.randint(0, 256, (12, 4100, 3)).astype(np.uint8)
    g = dict(inv=tilted(2.0, 6, 2050), rect=(2, 2, 8, 4096))
    assert F.crop_pads(12, 4100, g["rect"], 700) == (698, 698, 698, 698) and 32768 // (3 * 5496) == 1
    got = raw_call(cg, F, [img], [g], [700], 64)
    np.testing.assert_array_equal(got[0], F.resize_np(F.padded_crop_np(img, g["inv"], g["rect"], 700), 64))


def test_a_large_rectangle_at_margin_12(cg, F):
    """the 641-pixel rectangle of test_gpu_faces_variants.test_large_rectangles: pad 120, padded rows of 881 pixels - twelve per band,
    below the cap of sixteen - and ksize 29"""
    rs = np.random.RandomState(33)
    img = rs.randint(0, 256, (700, 700, 3)).astype(np.uint8)
    g = dict(inv=tilted(9.0, 350, 350), rect=(20, 40, 641, 641))
    pad = F.margin_pad(641, 12, 64)
    assert pad == 120 and 32768 // (3 * 881) == 12 and F.resample_ksize(881, 64) == 29 and min(F.crop_pads(700, 700, g["rect"], pad)) > 0
    got = raw_call(cg, F, [img], [g], [pad], 64)
    np.testing.assert_array_equal(got[0], F.resize_np(F.padded_crop_np(img, g["inv"], g["rect"], pad), 64))


# ---------------------------------------------------------------- 3. batch order and split
def test_padded_faces_do_not_depend_on_batch_order_or_split(cg, F, batch):
    images, geoms = batch[0], batch[1]
    call = lambda ix: F.extract_padded_device([images[i] for i in ix], [geoms[i] for i in ix], 12, 32)
    order = list(range(len(images)))
    whole = call(order)
    mixed = order[::-1][3:] + order[::-1][:3]
    for part in (mixed[:1], mixed[1:6], mixed[6:]):
        got = call(part)
        for k, i in enumerate(part):
            np.testing.assert_array_equal(got[k], whole[i], err_msg=f"face {i}")


# ---------------------------------------------------------------- 4. argument checks
def test_bad_arguments_are_refused_before_any_launch(cg, F):
    shapes = [(97, 131), (61, 83)]
    geoms = [dict(inv=tilted(9.0, 48, 65), rect=(10, 20, 64, 64)), dict(inv=tilted(0.0, 0, 0), rect=(5, 5, 33, 40))]
    N, out, pads = 2, 40, [12, 3]                             # 64 -> 40 needs ksize 5, the padded 88 -> 40 needs 7
    d = F.pack_padded_descriptors(shapes, geoms, pads, out)
    plain = F.pack_descriptors(shapes, geoms, out)
    nsrc = sum(h * w * 3 for h, w in shapes)
    wsb = F.padded_workspace_bytes([g["rect"] for g in geoms], pads, out)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    src, ws = torch.zeros(nsrc, dtype=torch.uint8).cuda(), torch.zeros(wsb, dtype=torch.uint8).cuda()
    dst = torch.full((N, out, out, 3), 7, dtype=torch.uint8).cuda()
    call, s = cg.lib().faces_u8_extract_padded, cg.tensor.stream()
    arrays = ("src_off", "geom", "inv", "taps", "tap_off", "pads")

    def args(**kw):
        """the valid call with some descriptor arrays / scalars replaced"""
        a = dict(d, src=src.data_ptr(), src_bytes=nsrc, dst=dst.data_ptr(), N=N, out=out, ws=ws.data_ptr(), wsb=wsb, ntaps=d["taps"].size)
        a.update(kw)
        keep = [up(a[k]) if isinstance(a[k], np.ndarray) else None for k in arrays]
        p = {k: (t.data_ptr() if t is not None else a[k]) for k, t in zip(arrays, keep)}
        return keep, (s, a["src"], a["src_bytes"], p["src_off"], p["geom"], p["inv"], p["taps"], a["ntaps"], p["tap_off"], p["pads"], a["dst"],
                      a["N"], a["out"], a["ws"], a["wsb"])

    def geom(f, col, v):
        g = d["geom"].copy()
        g[f, col] = v
        return g

    i32 = lambda *v: np.array(v, np.int32)
    bad_bounds = d["taps"].copy()
    bad_bounds[int(d["tap_off"][0, 0]) + 2 * (out - 1)] = 88   # the last horizontal sample of face 0 would read past its padded side
    cases = [(dict(src=None), "null pointer"), (dict(src_off=None), "null pointer"), (dict(geom=None), "null pointer"),
             (dict(inv=None), "null pointer"), (dict(taps=None), "null pointer"), (dict(tap_off=None), "null pointer"),
             (dict(pads=None), "null pointer"), (dict(dst=None), "null pointer"), (dict(ws=None), "null pointer"),
             (dict(N=0), "N = 0"), (dict(N=-3), "N = -3"), (dict(out=7), "out = 7"), (dict(out=129), "out = 129"),
             (dict(pads=i32(-1, 3)), "pad = -1"), (dict(pads=i32(12, 2049)), "pad = 2049"),
             (dict(geom=geom(1, 5, 4097), pads=i32(12, 2048)), "padded crop of 8193 x 4129 is beyond 8192"),
             (dict(geom=geom(0, 0, 7)), "source is outside"), (dict(geom=geom(1, 1, 8193)), "source is outside"),
             (dict(geom=geom(0, 4, 7)), "rectangle is outside"), (dict(geom=geom(1, 5, 4097)), "rectangle is outside"),
             (dict(geom=geom(0, 2, 34)), "not inside its"), (dict(geom=geom(1, 3, 44)), "not inside its"), (dict(geom=geom(0, 2, -1)), "not inside its"),
             (dict(geom=geom(0, 6, 5)), "ksize"), (dict(geom=geom(1, 7, 5)), "ksize"),
             (dict(geom=plain["geom"], taps=plain["taps"], tap_off=plain["tap_off"], ntaps=plain["taps"].size), "reads \\[|ksize"),      # the un-padded sides' tables
             (dict(src_bytes=nsrc - 1), "does not fit the"), (dict(ntaps=d["taps"].size - 1), "does not fit the"),
             (dict(taps=bad_bounds), "reads \\["), (dict(wsb=wsb - 80 * N - 256 - 1), "workspace"), (dict(wsb=0), "workspace")]
    assert tuple(plain["geom"][0, 6:8]) == (5, 5) and tuple(d["geom"][0, 6:8]) == (7, 7)
    for kw, message in cases:
        keep, a = args(**kw)
        with pytest.raises(cg.CatganError, match="cg_faces_u8_extract_padded: .*(" + message + ")"):
            call(*a)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 7).all()                     # nothing was launched
    keep, a = args()
    call(*a)                                                  # and the unmodified call is accepted
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0).all()                     # a black source


# ---------------------------------------------------------------- 5. the front end
def margin_tree(F, path):
    """TREE_SIZES through write_raw_tree, and a seventh image whose face is larger than the tree's own - the template at 0.2 min(H, W),
    tilted by 14 degrees - so that its padded rectangle leaves the image by more than a few pixels"""
    files = F.write_raw_tree(path, TREE_SIZES + [(97, 131)])
    big = [f for f in files if os.path.basename(f).startswith("00000006")][0]
    s, r, cy, cx = 0.2 * 97, math.radians(14.0), 97 // 2 + 12, 131 // 2
    x = cx + s * (F.TEMPLATE[:, 0] * math.cos(r) - F.TEMPLATE[:, 1] * math.sin(r))
    y = cy + s * (F.TEMPLATE[:, 0] * math.sin(r) + F.TEMPLATE[:, 1] * math.cos(r))
    assert x.min() >= 0 and y.min() >= 0 and x.max() <= 130 and y.max() <= 96
    with open(big + ".cat", "w") as f:
        f.write(F.cat_line(np.stack([np.rint(x), np.rint(y)], 1)))
    return files, big


def same_trees(a, b, dirs, counts):
    for d, n in zip(dirs, counts):
        names = sorted(os.listdir(a / d))
        assert names == sorted(os.listdir(b / d)) and len(names) == n, d
        for name in names:
            assert filecmp.cmp(a / d / name, b / d / name, shallow=False), f"{b.name}: {d}/{name}"


def test_generate_dataset_margin_on_the_device_equals_host(cg, F, tmp_path, monkeypatch):
    sys.path.insert(0, H.ROOT)
    G = importlib.import_module("generate_dataset")
    files, big = margin_tree(F, str(tmp_path / "raw"))
    n = len(files)
    fills = {}
    for fp in files:                                          # on the CPU: how far each padded rectangle leaves its image
        _, img, g = G._load(fp)
        fills[fp] = F.crop_pads(img.shape[0], img.shape[1], g["rect"], F.margin_pad(g["rect"][2], 8, 16))
    assert sum(max(v) > 0 for fp, v in fills.items() if fp != big) >= 2, fills      # the median path is there without the seventh image
    assert max(fills[big]) > 4, fills[big]                                           # and there it fills more than a few pixels
    argv = ["--path", str(tmp_path / "raw"), "--scale", "16", "--margin", "8", "--augmentations", "1"]
    dirs, counts = ("out_aug_16x16", "out_unaug_16x16", "out_padded_16x16_m8"), (2 * n, n, n + 1)
    assert H.run_front_end(argv + ["--out", str(tmp_path / "host"), "--host"]) == (n, 0)
    assert H.run_front_end(argv + ["--out", str(tmp_path / "dev")]) == (n, 0)
    same_trees(tmp_path / "host", tmp_path / "dev", dirs, counts)
    calls, device = [], F.extract_padded_device
    monkeypatch.setattr(F, "extract_padded_device", lambda images, *a, **kw: calls.append(len(images)) or device(images, *a, **kw))
    monkeypatch.setattr(G, "PADDED_BYTES", 250000)            # the padded calls of the one flush split
    assert H.run_front_end(argv + ["--out", str(tmp_path / "split")]) == (n, 0)
    assert len(calls) >= 3 and sum(calls) == n and 1 <= min(calls) and max(calls) <= 3, calls
    same_trees(tmp_path / "host", tmp_path / "split", dirs, counts)


def test_generate_dataset_margin_with_the_variants_from_the_crop(cg, F, tmp_path):
    files, _ = margin_tree(F, str(tmp_path / "raw"))
    n = len(files)
    argv = ["--path", str(tmp_path / "raw"), "--scale", "16", "--margin", "8", "--augmentations", "1", "--variantsFrom", "crop"]
    assert H.run_front_end(argv + ["--out", str(tmp_path / "host"), "--host"]) == (n, 0)
    assert H.run_front_end(argv + ["--out", str(tmp_path / "dev")]) == (n, 0)
    same_trees(tmp_path / "host", tmp_path / "dev", ("out_aug_16x16", "out_unaug_16x16", "out_padded_16x16_m8"), (2 * n, n, n + 1))
