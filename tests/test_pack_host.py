"""The decoded-set pack on the host (dataset.buildPack / openPack, pack_dataset.py): the round trip against _decode, independence of the
thread count, every way a pack goes stale or is damaged, the one-source-size rule, _pick_indices as the index form of _pick, and the
two gather entry points in the header and the library."""
import ctypes
import importlib
import os
import warnings

import numpy as np
import pytest

from helpers import make_jpgs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATHER = ("cg_images_u8_gather_scale_to_f32", "cg_images_u8_gather_augment_to_f32")


@pytest.fixture()
def ds():
    d = importlib.import_module("cat-generator_amd.dataset")
    d.setFileExtension("jpg")
    yield d
    d.setDirs([])
    d.seed(1)


def _refused(ds, d):
    """openPack(d) is None after exactly one warning; returns its text."""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert ds.openPack(d) is None
    assert len(w) == 1, [str(x.message) for x in w]
    return str(w[0].message)


def _opened(ds, d):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pack = ds.openPack(d)
    assert pack is not None
    return pack


def test_round_trip_equals_decode_in_load_paths_order(ds, tmp_path):
    d = str(tmp_path)
    make_jpgs(d, n=7)
    path, M = ds.buildPack(d, threads=3)
    assert path == os.path.join(d, "images_u8.cgpack") and M == 7
    assert sorted(os.listdir(d))[-1] == "images_u8.cgpack" and len(os.listdir(d)) == 8      # no temporary file is left
    ds.setDirs([d])
    files = ds.loadPaths()
    pack = _opened(ds, d)
    assert (pack.M, pack.Hs, pack.Ws) == (7, 64, 64) and pack.paths == files
    assert pack.pixels.dtype == np.uint8 and pack.pixels.shape == (7, 64, 64, 3)
    for i, f in enumerate(files):
        np.testing.assert_array_equal(pack.pixels[i], ds._decode(f), err_msg=f)
    raw = open(path, "rb").read()
    assert raw[:6] == b"CGPACK" and pack.pixels.offset % 4096 == 0
    assert raw[pack.pixels.offset:] == np.stack([ds._decode(f) for f in files]).tobytes()


def test_thread_count_does_not_change_the_file(ds, tmp_path):
    d = str(tmp_path)
    make_jpgs(d, n=9)
    ds.buildPack(d, threads=1)
    one = open(ds.packPath(d), "rb").read()
    ds.buildPack(d, threads=4)
    assert open(ds.packPath(d), "rb").read() == one
    ds.buildPack(d, threads=1000)      # capped, not an error
    assert open(ds.packPath(d), "rb").read() == one


def test_stale_and_damaged_packs_are_refused_with_a_warning(ds, tmp_path):
    from PIL import Image
    d = str(tmp_path)
    make_jpgs(d, n=5)
    assert "no such file" in _refused(ds, d)
    path, _ = ds.buildPack(d)
    good = open(path, "rb").read()
    _opened(ds, d)
    # truncated: by one byte, and down to less than a header
    for keep in (len(good) - 1, 20):
        open(path, "wb").write(good[:keep])
        _refused(ds, d)
    # a foreign magic, and this magic in another version
    for magic in (b"NOTAPACK", b"CGPACK02"):
        open(path, "wb").write(magic + good[8:])
        assert "magic" in _refused(ds, d)
    open(path, "wb").write(good)
    _opened(ds, d)
    # a file added
    extra = os.path.join(d, "cat_999.jpg")
    Image.fromarray(np.zeros((64, 64, 3), np.uint8)).save(extra, quality=95)
    assert "stale" in _refused(ds, d)
    os.remove(extra)
    _opened(ds, d)
    # a file touched (same bytes, another modification time)
    victim = os.path.join(d, "cat_002.jpg")
    st = os.stat(victim)
    os.utime(victim, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))
    assert "stale" in _refused(ds, d)
    os.utime(victim, ns=(st.st_atime_ns, st.st_mtime_ns))
    _opened(ds, d)
    # a file rewritten with other content (another size), the old modification time put back
    Image.fromarray(np.full((64, 64, 3), 200, np.uint8)).save(victim, quality=95)
    os.utime(victim, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert os.path.getsize(victim) != st.st_size
    assert "stale" in _refused(ds, d)
    # a file removed; and removed with another of the same name count put in its place
    ds.buildPack(d)
    _opened(ds, d)
    os.rename(victim, os.path.join(d, "cat_777.jpg"))
    assert "stale" in _refused(ds, d)
    os.remove(os.path.join(d, "cat_777.jpg"))
    assert "stale" in _refused(ds, d)


def test_builder_fails_on_an_odd_sized_file_and_names_it(ds, tmp_path):
    d = str(tmp_path)
    make_jpgs(d, n=6, odd=4)
    with pytest.raises(ValueError, match=r"cat_004\.jpg \(80x48\)"):
        ds.buildPack(d, threads=2)
    assert sorted(os.listdir(d)) == ["cat_%03d.jpg" % i for i in range(6)]      # neither a pack nor a temporary file


def test_pack_cli_writes_the_pack(ds, tmp_path, capsys):
    import sys
    sys.path.insert(0, ROOT)
    d = str(tmp_path)
    make_jpgs(d, n=4)
    importlib.import_module("pack_dataset").main(["--dataDir", d, "--threads", "2"])
    assert "4 images" in capsys.readouterr().out
    assert _opened(ds, d).M == 4


def test_pick_indices_is_the_index_form_of_pick(ds, tmp_path):
    d = str(tmp_path)
    make_jpgs(d, n=11)
    ds.setDirs([d])
    files = ds.loadPaths()
    for count in (1, 7, 11, 20, 10 ** 9):      # 20, 10 ** 9: more than the directory holds
        ds.seed(3)
        want = [ds._pick(count) for _ in range(2)]
        state = ds._rs.get_state()
        ds.seed(3)
        got = [ds._pick_indices(count) for _ in range(2)]
        for w, g in zip(want, got):
            assert len(g) == min(count, 11) and [files[i] for i in g] == w
        after = ds._rs.get_state()
        assert after[0] == state[0] and after[2:] == state[2:]
        np.testing.assert_array_equal(after[1], state[1])


def test_gather_entry_points_are_declared_and_exported():
    abi = importlib.import_module("cat-generator_amd._abi")
    protos = abi.parse_header()
    dll = ctypes.CDLL(abi.LIB_PATH)
    for name in GATHER:
        assert name in protos, f"{name} is not declared in include/catgan.h"
        assert hasattr(dll, name), f"{name} is not exported by the library"
    ret, args = protos[GATHER[0]]
    assert ret == "int" and [t for t, _ in args] == ["void*", "const unsigned char*", "long", "const int32_t*", "float*"] + ["int"] * 6
    ret, args = protos[GATHER[1]]
    assert [t for t, _ in args] == (["void*", "const unsigned char*", "long", "const int32_t*", "float*"] + ["int"] * 6 +
                                    ["const float*", "float", "uint64_t", "uint64_t"])
