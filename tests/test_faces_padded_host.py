"""CPU checks of the padded faces' device path (cg_faces_u8_extract_padded, faces.extract_padded_device, generate_dataset.py --margin
without --host), as far as it goes without a GPU: the entry point is declared and exported, the descriptors it reads (the un-padded
rectangle beside the ksizes and tap tables of the PADDED sides), the workspace formula against the layout the header documents, and the
front end's choice of who computes a padded face.  Every comparison is exact."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

import test_faces_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(97, 131), (61, 83), (375, 500), (97, 131), (61, 83)]
RECTS = [(10, 20, 64, 64), (5, 5, 33, 40), (100, 0, 203, 120), (3, 5, 40, 40), (20, 40, 8, 8)]


@pytest.fixture(scope="module")
def F():
    return importlib.import_module("cat-generator_amd.faces")


@pytest.fixture(scope="module")
def G():
    sys.path.insert(0, ROOT)
    return importlib.import_module("generate_dataset")


def geoms_of(rects):
    return [dict(inv=np.arange(6, dtype=np.float32) + i, rect=r) for i, r in enumerate(rects)]


# ---------------------------------------------------------------- the entry point
def test_the_header_declares_the_entry_point_and_the_library_exports_it():
    abi = importlib.import_module("cat-generator_amd._abi")
    protos = abi.parse_header()
    assert "cg_faces_u8_extract_padded" in protos and hasattr(ctypes.CDLL(abi.LIB_PATH), "cg_faces_u8_extract_padded")
    ret, args = protos["cg_faces_u8_extract_padded"]
    assert ret == "int" and [n for _, n in args] == ["stream", "src", "src_bytes", "src_off", "geom", "inv", "taps", "ntaps", "tap_off", "pads",
                                                     "dst", "N", "out", "workspace", "workspace_bytes"]
    assert dict((n, t) for t, n in args)["pads"] == "const int32_t*"
    sib = [n for _, n in protos["cg_faces_u8_extract"][1]]      # cg_faces_u8_extract's arguments with pads in front of dst
    assert [n for _, n in args if n != "pads"] == sib


# ---------------------------------------------------------------- descriptors
@pytest.mark.parametrize("out", [64, 16, 88])
def test_zero_pads_pack_what_pack_descriptors_packs(F, out):
    a = F.pack_padded_descriptors(SHAPES, geoms_of(RECTS), [0] * len(RECTS), out)
    b = F.pack_descriptors(SHAPES, geoms_of(RECTS), out)
    assert a["pads"].dtype == np.int32 and (a["pads"] == 0).all()
    assert set(a) == set(b) | {"pads"}
    for k in b:
        if isinstance(b[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("out", [24, 88])
def test_tap_tables_and_ksizes_belong_to_the_padded_sides(F, out):
    pads = [12, 0, 38, 24, 2]
    d = F.pack_padded_descriptors(SHAPES, geoms_of(RECTS), pads, out)
    np.testing.assert_array_equal(d["pads"], pads)
    off = 0
    for f, ((Hs, Ws), (y0, x0, Hr, Wr), p) in enumerate(zip(SHAPES, RECTS, pads)):
        assert tuple(d["geom"][f, :6]) == (Hs, Ws, y0, x0, Hr, Wr)       # the rectangle stays un-padded
        assert tuple(d["geom"][f, 6:8]) == (F.resample_ksize(Wr + 2 * p, out), F.resample_ksize(Hr + 2 * p, out))
        assert int(d["src_off"][f]) == off
        off += Hs * Ws * 3
        np.testing.assert_array_equal(d["inv"][f], np.arange(6, dtype=np.float32) + f)
        for a, side in enumerate((Wr + 2 * p, Hr + 2 * p)):
            bounds, taps = F._cached_taps(side, out)
            at = int(d["tap_off"][f, a])
            np.testing.assert_array_equal(d["taps"][at:at + bounds.size], bounds.reshape(-1))
            np.testing.assert_array_equal(d["taps"][at + bounds.size:at + bounds.size + taps.size], taps.reshape(-1))
    assert d["rows"] == sum(r[2] + 2 * p for r, p in zip(RECTS, pads))
    # faces 0 (64 + 24) and 3 (40 + 48) have the same padded side: one table serves them, on both axes
    assert len({int(v) for v in d["tap_off"][[0, 3]].reshape(-1)}) == 1
    sides = {r[2 + a] + 2 * p for r, p in zip(RECTS, pads) for a in (0, 1)}
    assert d["taps"].size == sum(out * (2 + F.resample_ksize(s, out)) for s in sides)      # every padded side once


# ---------------------------------------------------------------- workspace
def header_layout_bytes(rects, pads, out):
    """The layout under cg_faces_u8_extract_padded in catgan.h, piece by piece, each from a multiple of 16."""
    N, at = len(rects), 0
    for n in [4 * (N + 1)] * 2 + [4 * (N + 1)] * 2 + [4 * N] * 2 + [8 * N] * 2 + [32 * N]:
        at = -(-(at + n) // 16) * 16
    for (_, _, Hr, Wr), p in zip(rects, pads):
        at += -(-(3 * (Hr + 2 * p) * (Wr + 2 * p)) // 16) * 16
    return at + sum(3 * out * (r[2] + 2 * p) for r, p in zip(rects, pads))


def test_workspace_formula_covers_the_documented_layout_and_grows_with_the_pad(F):
    for rects in (RECTS, RECTS[:1], RECTS * 40):
        last = 0
        for pad in (0, 1, 2, 7, 30, 64, 65, 700, 2048):
            pads = [pad] * len(rects)
            for out in (16, 88):
                got = F.padded_workspace_bytes(rects, pads, out)
                exact = header_layout_bytes(rects, pads, out)
                assert exact <= got <= exact + 80 * len(rects) + 256, (pad, out)
                assert got == 80 * len(rects) + 256 + sum(F.padded_bytes(r, pad, out) - 3 * out * out for r in rects)
            assert got > last
            last = got
    assert F.padded_bytes((0, 0, 64, 64), 12, 88) == 3 * 88 * 88 + 3 * 88 * 88 + 3 * 88 * 88      # crop, horizontal pass, padded face
    assert F.padded_bytes((0, 0, 33, 40), 1, 16) == -(-(3 * 35 * 42) // 16) * 16 + 3 * 16 * 35 + 3 * 16 * 16
    assert F.PADDED_SIDE_MAX == 8192


# ---------------------------------------------------------------- the front end: who computes a padded face
def test_load_computes_no_padded_face_unless_host(F, G, tmp_path, monkeypatch):
    files = F.write_raw_tree(str(tmp_path / "raw"), [(61, 83), (97, 131)])
    fp, img, g = G._load(files[0], 4, 16, True)
    np.testing.assert_array_equal(g["padded"], F.padded_face_np(img, g["inv"], g["rect"], 4, 16))

    def boom(*a, **kw):
        raise AssertionError("padded_face_np ran on a decoding thread of the device mode")
    monkeypatch.setattr(F, "padded_face_np", boom)
    for args in ((4, 16), (4, 16, False), (0, 16, True), ()):
        fp, img, g = G._load(files[1], *args)
        assert img is not None and "padded" not in g
    with pytest.raises(AssertionError, match="decoding thread"):
        G._load(files[1], 4, 16, True)


def test_a_face_beyond_the_device_limits_takes_the_host_form(F, G, monkeypatch):
    """The selection alone: the device calls are stubs that return recognisable bytes."""
    assert F.padded_fits_device((0, 0, 4096, 4096), 2048) and not F.padded_fits_device((0, 0, 4096, 4096), 2049)
    assert F.padded_fits_device((0, 0, 5000, 5000), 1596) and not F.padded_fits_device((0, 0, 5000, 5000), 1597)      # 8192 and 8194
    assert not F.padded_fits_device((0, 0, 700, 700), 2188)
    S, margin = 16, 50                                         # pad = 3.125 Hr: beyond 2048 from Hr = 656 on
    side = S + 2 * margin
    rects = [(0, 0, 64, 64), (0, 0, 700, 700), (0, 0, 100, 100), (0, 0, 655, 655), (0, 0, 656, 656)]
    fits = [F.padded_fits_device(r, F.margin_pad(r[2], margin, S)) for r in rects]
    assert fits == [True, False, True, True, False]
    batch = [(f"f{i}", np.zeros((8, 8, 3), np.uint8), dict(inv=None, rect=r, tag=i)) for i, r in enumerate(rects)]
    calls = []

    def dev(images, geoms, m, out, with_faces=False):
        assert (m, out) == (margin, S)
        calls.append([g["tag"] for g in geoms])
        p = np.stack([np.full((side, side, 3), 100 + g["tag"], np.uint8) for g in geoms])
        return (np.stack([np.full((S, S, 3), 10 + g["tag"], np.uint8) for g in geoms]), p) if with_faces else p

    monkeypatch.setattr(F, "extract_padded_device", dev)
    monkeypatch.setattr(F, "padded_face_np", lambda im, inv, rect, m, out=64: np.full((out + 2 * m, out + 2 * m, 3), 200 + rect[2] % 50, np.uint8))
    monkeypatch.setattr(F, "extract_faces_device", lambda ims, gs, out=64: np.stack([np.full((out, out, 3), 50 + g["tag"], np.uint8) for g in gs]))
    faces, padded = G._padded_faces(batch, margin, S, with_faces=True)
    assert calls == [[0, 2, 3]]                                # one device call for the faces that fit, in their order
    assert padded.shape == (5, side, side, 3) and faces.shape == (5, S, S, 3)
    assert [int(p[0, 0, 0]) for p in padded] == [100, 200, 102, 103, 206]
    assert [int(f[0, 0, 0]) for f in faces] == [10, 51, 12, 13, 54]
    calls.clear()
    monkeypatch.setattr(G, "PADDED_BYTES", 1)                  # every device call takes one face
    faces, padded2 = G._padded_faces(batch, margin, S, with_faces=False)
    assert faces is None and calls == [[0], [2], [3]]
    np.testing.assert_array_equal(padded2, padded)
