"""The window form of the augmentation on the MI355X: cg_images_u8_augment_window_to_f32 and its gather form bit-equal to
dataset.augment_images(margin) -> image_scale -> rgbToColorSpace (whose own yardsticks are in tests/test_augment_margin_host.py); with
margin 0 to the entry points without a margin; with the identity draw to cg_images_u8_scale_to_f32 of the cropped windows; their
refusals; and the three loaders over a padded directory against the blocking loader."""
import importlib
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
CODE = {"rgb": 0, "y": 1, "yuv": 2, "hsl": 3}
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 1, 0], np.float32)
SEED, OFFSET = 0x5DEECE66D1234567, 987654321
# Hp, Wp, margin, Hd, Wd, N: equal sizes, a shrink by 2, a non-integer shrink of a window that is not square, an enlargement, and the
# padded 64 x 64 face (93 KB of LDS: the dynamic size has to be asked for); a 13 x 4 window shrunk down its height and stretched along its width
SHAPES = [(12, 12, 2, 8, 8, None), (20, 20, 2, 8, 8, None), (17, 19, 2, 8, 8, None), (12, 12, 2, 12, 12, None), (88, 88, 12, 32, 32, 2),
          (17, 8, 2, 5, 9, None)]


@pytest.fixture(scope="module")
def cg():
    assert torch.cuda.is_available()
    return importlib.import_module("cat-generator_amd")


@pytest.fixture()
def ds():
    d = importlib.import_module("cat-generator_amd.dataset")
    yield d
    d.setAugmentation(False)
    d.setDirs([])
    d.colorSpace = "rgb"
    d.setHeight(32); d.setWidth(32)
    d.seed(1)


def descriptors(ds, Hp, Wp, m):
    """The descriptors of the issue's list for a padded size: identity; shifts up to +-margin; 8 degrees with zoom 0.93 and a shift of 4;
    a shift beyond the margin (it clamps); a NaN entry; both flips (of the identity and of the rotated draw)."""
    rows = [(1.0, 0, 0, 0, 1.0, 0), (1.0, 0, m, -m, 0.9, 0), (1.0, 0, -m, m, 1.1, 0), (1.0, 0, 1, 0, 1.0, 0), (0.93, 8, 4, -4, 1.15, 0),
            (1.0, 0, m + 3, -(m + 2), 1.0, 0), (1.08, -8, 0, 0, 0.85, 0), (1.0, 0, 0, 0, 1.0, 1), (0.93, 8, -4, 4, 1.05, 1)]
    cols = list(zip(*rows))
    draw = dict(scale=cols[0], rotation=cols[1], tx=cols[2], ty=cols[3], brightness=cols[4], flip=cols[5])
    desc = ds.augment_descriptors(len(rows), Hp, Wp, draw)
    np.testing.assert_array_equal(desc[0], IDENTITY)
    desc[6, 2] = np.nan
    return desc


def _window(cg, u8, desc, m, h, w, cs, sigma, seed=SEED, offset=OFFSET):
    N, Hp, Wp, _ = u8.shape
    src = torch.from_numpy(u8).cuda()
    dsc = None if desc is None else torch.from_numpy(np.ascontiguousarray(desc, dtype=np.float32)).cuda()
    dst = cg.Tensor.empty((N, 1 if cs == "y" else 3, h, w), "nhwc")
    cg.lib().images_u8_augment_window_to_f32(cg.tensor.stream(), src.data_ptr(), dst.ptr, N, Hp, Wp, m, h, w, CODE[cs],
                                             None if dsc is None else dsc.data_ptr(), sigma, seed, offset)
    return dst.numpy()


def _gather(cg, u8set, idx, desc, m, h, w, cs, sigma, seed=SEED, offset=OFFSET):
    M, Hp, Wp, _ = u8set.shape
    N = len(idx)
    src, ix = torch.from_numpy(u8set).cuda(), torch.from_numpy(np.asarray(idx, np.int32)).cuda()
    dsc = None if desc is None else torch.from_numpy(np.ascontiguousarray(desc, dtype=np.float32)).cuda()
    dst = cg.Tensor.empty((N, 1 if cs == "y" else 3, h, w), "nhwc")
    cg.lib().images_u8_gather_augment_window_to_f32(cg.tensor.stream(), src.data_ptr(), M, ix.data_ptr(), dst.ptr, N, Hp, Wp, m, h, w, CODE[cs],
                                                    None if dsc is None else dsc.data_ptr(), sigma, seed, offset)
    return dst.numpy()


def _host(ds, u8, desc, m, h, w, cs, sigma, seed=SEED, offset=OFFSET):
    warped = ds.augment_images(u8, desc, sigma, seed, offset, margin=m)
    return ds.rgbToColorSpace(np.stack([ds.image_scale(im, w, h) for im in warped]), cs)


def _scaled(cg, u8, h, w, cs):
    """cg_images_u8_scale_to_f32 of a batch."""
    N, Hs, Ws, _ = u8.shape
    src = torch.from_numpy(np.ascontiguousarray(u8)).cuda()
    dst = cg.Tensor.empty((N, 1 if cs == "y" else 3, h, w), "nhwc")
    cg.lib().images_u8_scale_to_f32(cg.tensor.stream(), src.data_ptr(), dst.ptr, N, Hs, Ws, h, w, CODE[cs])
    return dst.numpy()


def _images(rs, N, Hp, Wp, grey=False):
    u8 = rs.randint(0, 256, size=(N, Hp, Wp, 3)).astype(np.uint8)
    if grey:      # hsl: grey pixels and ties between channels
        u8[0, : Hp // 3] = u8[0, : Hp // 3, :, :1]
    return u8


# ---------------------------------------------------------------- 1. kernel against the host restatement
@pytest.mark.parametrize("sigma", [0.0, 0.02])
@pytest.mark.parametrize("Hp,Wp,m,h,w,N", SHAPES)
def test_window_kernel_equals_the_host_restatement_bit_for_bit(cg, ds, Hp, Wp, m, h, w, N, sigma):
    desc = descriptors(ds, Hp, Wp, m)
    if N is not None:      # the large shape: two images, the rotated draw and the flipped one
        desc = desc[[4, 8]]
    u8 = _images(np.random.RandomState(Hp + h), len(desc), Hp, Wp)
    np.testing.assert_array_equal(_window(cg, u8, desc, m, h, w, "rgb", sigma), _host(ds, u8, desc, m, h, w, "rgb", sigma))


@pytest.mark.parametrize("cs", ["y", "yuv", "hsl"])
def test_window_kernel_in_the_other_colour_spaces(cg, ds, cs):
    Hp, Wp, m, h, w = 17, 19, 2, 8, 8
    desc = descriptors(ds, Hp, Wp, m)
    u8 = _images(np.random.RandomState(3), len(desc), Hp, Wp, grey=cs == "hsl")
    np.testing.assert_array_equal(_window(cg, u8, desc, m, h, w, cs, 0.02), _host(ds, u8, desc, m, h, w, cs, 0.02))


def test_window_kernel_with_three_images_and_drawn_descriptors(cg, ds):
    Hp, Wp, m, h, w = 20, 20, 2, 8, 8
    ds.seed(11)
    ds.setAugmentation(True)
    desc = ds.augment_descriptors(3, Hp, Wp)
    u8 = _images(np.random.RandomState(4), 3, Hp, Wp)
    np.testing.assert_array_equal(_window(cg, u8, desc, m, h, w, "rgb", 0.02), _host(ds, u8, desc, m, h, w, "rgb", 0.02))


# ---------------------------------------------------------------- 2. the gather form
@pytest.mark.parametrize("Hp,Wp,m,h,w", [(17, 19, 2, 8, 8), (88, 88, 12, 32, 32)])
def test_gather_form_equals_the_host_restatement_and_zeroes_bad_indices(cg, ds, Hp, Wp, m, h, w):
    M, idx = 5, [3, 1, 3, -1, 5, 0]
    u8set = _images(np.random.RandomState(Hp), M, Hp, Wp)
    desc = descriptors(ds, Hp, Wp, m)[[4, 1, 8, 0, 0, 5]]
    got = _gather(cg, u8set, idx, desc, m, h, w, "rgb", 0.02)
    # image n of the pool: the source set[idx[n]] with descriptor n and the noise counters of position n
    want = _host(ds, u8set[np.clip(idx, 0, M - 1)], desc, m, h, w, "rgb", 0.02)
    want[3] = 0
    want[4] = 0
    np.testing.assert_array_equal(got, want)
    assert not np.array_equal(got[0], got[2])      # the repeated index: the same source, another draw and other noise
    plain = _window(cg, u8set[np.clip(idx, 0, M - 1)], desc, m, h, w, "rgb", 0.02)      # and the form without a gather on set[idx]
    plain[3:5] = 0
    np.testing.assert_array_equal(got, plain)


# ---------------------------------------------------------------- 3. margin 0 = the entry points without a margin
@pytest.mark.parametrize("cs", ["rgb", "hsl"])
def test_margin_0_equals_the_entry_points_without_a_margin(cg, ds, cs):
    for Hs, Ws, h, w in ((64, 64, 32, 32), (17, 19, 8, 8), (12, 12, 16, 16)):
        N = 5
        ds.seed(Hs)
        ds.setAugmentation(True)
        desc = ds.augment_descriptors(N, Hs, Ws)
        u8 = _images(np.random.RandomState(Hs), N, Hs, Ws, grey=cs == "hsl")
        src, dsc = torch.from_numpy(u8).cuda(), torch.from_numpy(desc).cuda()
        ix = torch.from_numpy(np.array([4, 0, 2, 2, 1], np.int32)).cuda()
        a, b = (cg.Tensor.empty((N, 3, h, w), "nhwc") for _ in range(2))
        cg.lib().images_u8_augment_to_f32(cg.tensor.stream(), src.data_ptr(), a.ptr, N, Hs, Ws, h, w, CODE[cs], dsc.data_ptr(), 0.02, SEED, OFFSET)
        np.testing.assert_array_equal(_window(cg, u8, desc, 0, h, w, cs, 0.02), a.numpy())
        cg.lib().images_u8_gather_augment_to_f32(cg.tensor.stream(), src.data_ptr(), N, ix.data_ptr(), b.ptr, N, Hs, Ws, h, w, CODE[cs],
                                                 dsc.data_ptr(), 0.02, SEED, OFFSET)
        np.testing.assert_array_equal(_gather(cg, u8, [4, 0, 2, 2, 1], desc, 0, h, w, cs, 0.02), b.numpy())


# ---------------------------------------------------------------- 4. identity = the scaling kernel on the cropped windows
@pytest.mark.parametrize("cs", ["rgb", "y", "yuv", "hsl"])
def test_identity_equals_the_scaling_kernel_on_the_cropped_windows(cg, ds, cs):
    for Hp, Wp, m, h, w, N in SHAPES:
        N = N or 4
        u8 = _images(np.random.RandomState(Hp + w), N, Hp, Wp, grey=cs == "hsl")
        want = _scaled(cg, u8[:, m:Hp - m, m:Wp - m], h, w, cs)
        what = f"{Hp}x{Wp} margin {m} -> {h}x{w}"
        np.testing.assert_array_equal(_window(cg, u8, None, m, h, w, cs, 0.0), want, err_msg=what + ", no descriptors")
        np.testing.assert_array_equal(_window(cg, u8, np.tile(IDENTITY, (N, 1)), m, h, w, cs, 0.0), want, err_msg=what)
        idx = list(range(N))[::-1]
        np.testing.assert_array_equal(_gather(cg, u8, idx, None, m, h, w, cs, 0.0), want[idx], err_msg=what + ", gathered")


# ---------------------------------------------------------------- 5. refusals
def test_bad_windows_are_refused_before_any_launch(cg):
    big = torch.zeros((1, 118, 118, 3), dtype=torch.uint8).cuda()
    u8 = torch.zeros((2, 12, 12, 3), dtype=torch.uint8).cuda()
    ix = torch.zeros(2, dtype=torch.int32).cuda()
    desc = torch.from_numpy(np.tile(IDENTITY, (2, 1))).cuda()
    dst = cg.Tensor.from_numpy(np.full((2, 3, 32, 32), -1.0, np.float32))
    s, L = cg.tensor.stream(), cg.lib()
    plain = lambda src, *a: L.images_u8_augment_window_to_f32(s, src.data_ptr(), dst.ptr, *a)
    gather = lambda src, *a: L.images_u8_gather_augment_window_to_f32(s, src.data_ptr(), 1, ix.data_ptr(), dst.ptr, *a)
    for f in (plain, gather):
        with pytest.raises(cg.CatganError, match="LDS"):      # 118 x 118 x 12 = 167088 bytes > 160 KB; the 94 x 94 window is within 6x of 32
            f(big, 1, 118, 118, 12, 32, 32, 0, desc.data_ptr(), 0.02, 1, 0)
        for m in (6, 7, -1):                                  # 2 margin >= Hp; a negative margin
            with pytest.raises(cg.CatganError, match="margin"):
                f(u8, 2, 12, 12, m, 8, 8, 0, desc.data_ptr(), 0.02, 1, 0)
        with pytest.raises(cg.CatganError, match="margin"):   # ... or >= Wp alone
            f(u8, 1, 24, 6, 3, 8, 8, 0, desc.data_ptr(), 0.02, 1, 0)
        with pytest.raises(cg.CatganError, match="more than 6"):      # the window's factor: 100 / 8 with margin 2, while 12 / 2 = 6 passes below
            f(big, 1, 104, 104, 2, 8, 8, 0, desc.data_ptr(), 0.02, 1, 0)
        with pytest.raises(cg.CatganError, match="bad arguments"):
            f(u8, 2, 12, 12, 2, 8, 8, 0, desc.data_ptr(), -0.5, 1, 0)
    with pytest.raises(cg.CatganError, match="bad arguments"):
        L.images_u8_augment_window_to_f32(s, None, dst.ptr, 2, 12, 12, 2, 8, 8, 0, desc.data_ptr(), 0.02, 1, 0)
    torch.cuda.synchronize()
    assert np.all(dst.numpy() == -1.0)
    small = cg.Tensor.from_numpy(np.full((2, 3, 2, 2), -1.0, np.float32))      # the limit is the window's: 16 x 16 padded, 12 x 12 shown, 2 x 2 target
    wide = torch.zeros((2, 16, 16, 3), dtype=torch.uint8).cuda()
    L.images_u8_augment_window_to_f32(s, wide.data_ptr(), small.ptr, 2, 16, 16, 2, 2, 2, 0, None, 0.0, 0, 0)
    assert np.all(small.numpy() == 0.0)


# ---------------------------------------------------------------- 6. the loaders over a padded directory
@pytest.fixture()
def padded_dir(tmp_path):
    rs = np.random.RandomState(31)
    for i in range(12):
        Image.fromarray(rs.randint(0, 256, size=(24, 24, 3)).astype(np.uint8)).save(str(tmp_path / f"{i:03d}.png"))
    with open(tmp_path / "margin.json", "w") as f:
        json.dump({"margin": 4, "side": 16}, f)
    return str(tmp_path)


def _setup(ds, d, aug):
    ds.setDirs([d]); ds.setFileExtension("png"); ds.setHeight(8); ds.setWidth(8)
    assert ds.margin == 4
    ds.setAugmentation(aug)
    ds.seed(5)
    ref = [ds.loadRandomImages(7).scaled for _ in range(3)]
    ds.seed(5)
    return ref


@pytest.mark.parametrize("aug", [False, True])
def test_async_loader_pools_of_a_padded_directory_equal_the_blocking_loader(cg, ds, padded_dir, aug):
    ref = _setup(ds, padded_dir, aug)
    ld = ds.AsyncLoader(7)
    assert ld.aug == aug and ld.margin == 4 and not ld.host_all and (ld.Hs, ld.Ws) == (24, 24)
    for e in range(3):
        np.testing.assert_array_equal(cg.nn.as_nhwc(ld.next()).numpy(), ref[e], err_msg=f"pool {e}")
    torch.cuda.synchronize()
    ld.close()
    assert np.array_equal(ref[0], ref[1]) is False


@pytest.mark.parametrize("aug", [False, True])
def test_resident_loader_pools_of_a_padded_directory_equal_the_blocking_loader(cg, ds, padded_dir, aug):
    ref = _setup(ds, padded_dir, aug)
    ds.buildPack(padded_dir, threads=2)
    pack = ds.openPack(padded_dir)      # margin.json does not disturb the freshness check
    assert pack is not None and (pack.M, pack.Hs, pack.Ws) == (12, 24, 24)
    rset = ds.ResidentSet(pack)
    ld = ds.ResidentLoader(7, rset)
    assert ld.aug == aug and ld.margin == 4
    for e in range(3):
        np.testing.assert_array_equal(cg.nn.as_nhwc(ld.next()).numpy(), ref[e], err_msg=f"pool {e}")
    torch.cuda.synchronize()
    ld.close()
    ds.setAugmentation(True)      # the chunks are never augmented: the windows as loadImageFile gives them
    want = np.stack([ds.loadImageFile(p) for p in rset.paths])
    got = np.concatenate([cg.nn.as_nhwc(pool).numpy()[:n] for pool, _, n in rset.chunks(5)])
    np.testing.assert_array_equal(got, want)
    torch.cuda.synchronize()
    rset.close()


def test_sequential_loader_over_a_padded_directory_equals_load_image_file(cg, ds, padded_dir):
    _setup(ds, padded_dir, True)
    files = ds.loadPaths()
    want = np.stack([ds.loadImageFile(p) for p in files])
    ld = ds.SequentialLoader(files, 5)
    assert ld.margin == 4 and not ld.aug
    got = np.concatenate([cg.nn.as_nhwc(pool).numpy()[:n] for pool, _, n in ld])
    ld.close()
    np.testing.assert_array_equal(got, want)


def test_resident_chunks_over_a_padded_directory_equal_load_image_file(cg, ds, padded_dir):
    """ResidentSet.chunks with a margin: the window form's identity draw on consecutive slices, 12 files in chunks of 5."""
    _setup(ds, padded_dir, True)
    ds.buildPack(padded_dir, threads=2)
    rset = ds.ResidentSet(ds.openPack(padded_dir))
    ch = rset.chunks(5)
    assert ch.margin == 4 and ch.files == rset.paths
    seen = []
    for pool, index0, n in ch:
        seen.append((index0, n))
        for i in range(n):
            np.testing.assert_array_equal(cg.nn.as_nhwc(pool).numpy()[i], ds.loadImageFile(rset.paths[index0 + i]), err_msg=rset.paths[index0 + i])
    assert seen == [(0, 5), (5, 5), (10, 2)] and ch.next() is None
    torch.cuda.synchronize()
    ch.close()
    rset.close()


@pytest.mark.parametrize("aug", [False, True])
def test_async_loader_host_paths_follow_the_margin(cg, ds, padded_dir, aug):
    """An image of another size is scaled on the host and patched into the pool; a window more than 6x the target sends all of them
    there.  Both go through _load_scaled, which knows the margin."""
    Image.fromarray(np.random.RandomState(32).randint(0, 256, size=(20, 30, 3)).astype(np.uint8)).save(os.path.join(padded_dir, "odd.png"))
    _setup(ds, padded_dir, aug)
    ref = [ds.loadRandomImages(13).scaled for _ in range(2)]
    ds.seed(5)
    ld = ds.AsyncLoader(13)
    assert not ld.host_all
    for e in range(2):
        np.testing.assert_array_equal(cg.nn.as_nhwc(ld.next()).numpy(), ref[e], err_msg=f"pool {e}")
    torch.cuda.synchronize()
    ld.close()
    ds.setHeight(2); ds.setWidth(2)      # 16 / 2 = 8: beyond the kernel's 6, by the window's size (24 / 2 = 12 would be, too)
    ds.seed(5)
    ref = [ds.loadRandomImages(13).scaled for _ in range(2)]
    ds.seed(5)
    with pytest.warns(UserWarning, match="16x16 sources are more than 6x"):
        ld = ds.AsyncLoader(13)
    assert ld.host_all
    for e in range(2):
        np.testing.assert_array_equal(cg.nn.as_nhwc(ld.next()).numpy(), ref[e], err_msg=f"host pool {e}")
    torch.cuda.synchronize()
    ld.close()
