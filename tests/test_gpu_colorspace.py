"""The 'yuv' and 'hsl' colour spaces on the MI355X: the loader kernels (cg_images_u8_scale_to_f32, cg_images_u8_to_f32) in modes 2 / 3
and cg_colorspace_convert, bit-equal to the numpy functions of dataset.py / nn_utils.py (whose distance to fp64 and colorsys
tests/test_colorspace_host.py bounds); AsyncLoader's pools against the blocking loader; train.py -> sample.py end to end."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import make_jpgs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = {"rgb": 0, "y": 1, "yuv": 2, "hsl": 3}


@pytest.fixture(scope="module")
def cg():
    assert torch.cuda.is_available()
    return importlib.import_module("cat-generator_amd")


@pytest.fixture(scope="module")
def ds():
    return importlib.import_module("cat-generator_amd.dataset")


# ---------------------------------------------------------------- 6. the loader kernels
@pytest.mark.parametrize("cs", ["rgb", "y", "yuv", "hsl"])
def test_loader_kernels_equal_the_host_loader_bit_for_bit(cg, ds, cs):
    """image.load -> image.scale -> colour space from the decoded bytes, over the geometries of test_dataset_cli.py: 'yuv' / 'hsl'
    against dataset.rgbToColorSpace of the host-scaled rgb image, 'rgb' / 'y' (which must not have moved) against the oracle."""
    from oracle import oracle as O
    C = 1 if cs == "y" else 3
    rs = np.random.RandomState(3)
    for (Hs, Ws, h, w) in ((64, 64, 32, 32), (64, 64, 64, 64), (32, 32, 64, 64), (96, 60, 32, 24), (80, 80, 32, 32),
                           (13, 4, 5, 9), (7, 11, 7, 4), (5, 11, 13, 11)):      # the two axes in different branches of the footprint rule
        u8 = rs.randint(0, 256, size=(2, Hs, Ws, 3)).astype(np.uint8)
        if cs == "hsl":      # grey pixels and ties between channels inside a scaled image too
            u8[0, : Hs // 4] = u8[0, : Hs // 4, :, :1]
            u8[1, : Hs // 4, :, 1] = u8[1, : Hs // 4, :, 0]
        src = torch.from_numpy(u8).cuda()
        dst = cg.Tensor.empty((2, C, h, w), "nhwc")
        cg.lib().images_u8_scale_to_f32(cg.tensor.stream(), src.data_ptr(), dst.ptr, 2, Hs, Ws, h, w, CODE[cs])
        if cs in ("rgb", "y"):
            want = np.stack([O.load_image(u8[i], w, h, cs) for i in range(2)])
        else:
            scaled = np.stack([ds.image_scale(u8[i].astype(np.float32).transpose(2, 0, 1) / np.float32(255.0), w, h) for i in range(2)])
            want = ds.rgbToColorSpace(scaled, cs)
        np.testing.assert_array_equal(dst.numpy(), want, err_msg=f"{Hs}x{Ws} -> {h}x{w} {cs}")
    # the flat form (no resize): every pixel of the 8-bit grid's corners plus random ones, a count that is no multiple of the block
    u8 = rs.randint(0, 256, size=(3, 37, 41, 3)).astype(np.uint8)
    u8[0, 0, :12] = [(0, 0, 0), (255, 255, 255), (128, 128, 128), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255),
                     (255, 0, 255), (200, 10, 90), (200, 200, 10), (10, 200, 200)]
    src = torch.from_numpy(u8).cuda()
    dst = cg.Tensor.empty((3, C, 37, 41), "nhwc")
    cg.lib().images_u8_to_f32(cg.tensor.stream(), src.data_ptr(), dst.ptr, 3 * 37 * 41, CODE[cs])
    rgb = u8.astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255.0)
    want = np.stack([O.load_image(u8[i], 41, 37, cs) for i in range(3)]) if cs in ("rgb", "y") else ds.rgbToColorSpace(rgb, cs)
    np.testing.assert_array_equal(dst.numpy(), want, err_msg=f"flat {cs}")
    for bad in (-1, 4):
        with pytest.raises(cg.CatganError, match="bad arguments"):
            cg.lib().images_u8_to_f32(cg.tensor.stream(), src.data_ptr(), dst.ptr, 3 * 37 * 41, bad)
        with pytest.raises(cg.CatganError, match="bad arguments"):
            cg.lib().images_u8_scale_to_f32(cg.tensor.stream(), src.data_ptr(), dst.ptr, 3, 37, 41, 37, 41, bad)


# ---------------------------------------------------------------- 7. cg_colorspace_convert
def _inputs(cs, shape, seed):
    """Pixels of space `cs` as [N, 3, H, W]: half of them what the loader makes of 8-bit images, half arbitrary floats in (0, 1) on
    all three planes - what G's Sigmoid hands to toRgb."""
    ds = importlib.import_module("cat-generator_amd.dataset")
    rs = np.random.RandomState(seed)
    N = shape[0]
    x = rs.rand(*shape).astype(np.float32)
    grid = rs.randint(0, 256, size=(N // 2,) + shape[1:]).astype(np.float32) / np.float32(255)
    grid[0, :, 0, :6] = np.array([(0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 0, 1), (1, 1, 0), (0.5, 0.5, 0.5)], np.float32).T
    x[: N // 2] = ds.rgbToColorSpace(grid, cs)
    if cs == "hsl":
        x[-1, 1, 0, :8] = 0.0                                                     # s == 0 on arbitrary h, l
        x[-1, 2, 1, :8] = [0.5, 0.25, 0.75, 0.0, 1.0, 0.5, 0.4999, 0.5001]       # l around 0.5
        x[-1, 0, 2, :4] = [0.0, np.nextafter(np.float32(1), np.float32(0)), 1 / 3, 2 / 3]
    return x


@pytest.mark.parametrize("shape", [(4, 3, 37, 41), (70, 3, 64, 64)])     # 6 068 pixels (23.7 blocks); 286 720 pixels: more than one grid pass
@pytest.mark.parametrize("frm,to", [("rgb", "y"), ("rgb", "yuv"), ("rgb", "hsl"), ("yuv", "rgb"), ("hsl", "rgb")])
def test_colorspace_convert_equals_numpy_bit_for_bit(cg, ds, frm, to, shape):
    U = cg.nn_utils
    x = _inputs(frm, shape, seed=shape[0] + CODE[frm])
    want = ds.rgbToColorSpace(x, to) if frm == "rgb" else U.toRgb(x, frm)
    N, _, H, W = shape
    src = cg.Tensor.from_numpy(x)
    dst = cg.Tensor.empty(want.shape, "nhwc")
    cg.lib().colorspace_convert(cg.tensor.stream(), src.ptr, dst.ptr, N * H * W, CODE[frm], CODE[to])
    np.testing.assert_array_equal(dst.numpy(), want, err_msg=f"{frm} -> {to} out of place")
    np.testing.assert_array_equal(src.numpy(), x)
    if to != "y":
        cg.lib().colorspace_convert(cg.tensor.stream(), src.ptr, src.ptr, N * H * W, CODE[frm], CODE[to])
        np.testing.assert_array_equal(src.numpy(), want, err_msg=f"{frm} -> {to} in place")
    if to == "rgb":      # nn_utils.toRgb handed an engine tensor converts on the device and returns the host array
        np.testing.assert_array_equal(U.toRgb(cg.Tensor.from_numpy(x), frm), want)


def test_colorspace_convert_refuses_what_it_cannot_do(cg):
    x = cg.Tensor.from_numpy(np.full((1, 3, 4, 4), 0.25, np.float32))
    y = cg.Tensor.from_numpy(np.full((1, 3, 4, 4), -1.0, np.float32))
    s = cg.tensor.stream()
    for frm, to in ((0, 0), (1, 0), (2, 3), (3, 2), (2, 1), (0, 4), (4, 0), (-1, 0), (2, 2)):
        with pytest.raises(cg.CatganError, match="unsupported pair"):
            cg.lib().colorspace_convert(s, x.ptr, y.ptr, 16, frm, to)
    with pytest.raises(cg.CatganError, match="in place"):
        cg.lib().colorspace_convert(s, x.ptr, x.ptr, 16, 0, 1)
    with pytest.raises(cg.CatganError, match="bad arguments"):
        cg.lib().colorspace_convert(s, x.ptr, y.ptr, 0, 0, 2)
    with pytest.raises(cg.CatganError, match="bad arguments"):
        cg.lib().colorspace_convert(s, None, y.ptr, 16, 0, 2)
    torch.cuda.synchronize()
    assert np.all(y.numpy() == -1.0) and np.all(x.numpy() == 0.25)        # nothing was launched
    assert cg.nn_utils.toRgb(cg.Tensor.from_numpy(np.full((2, 1, 4, 4), 0.5, np.float32)), "y").shape == (2, 3, 4, 4)


# ---------------------------------------------------------------- 8. AsyncLoader
@pytest.mark.parametrize("cs", ["yuv", "hsl"])
def test_async_loader_pools_equal_the_blocking_loader(cg, ds, tmp_path, cs):
    """The shape of test_dataset_cli.py's test of the same name for the two new spaces: four epochs over both pools, fewer files than
    asked for, and files of another source size that take the host path inside the loader."""
    from PIL import Image
    make_jpgs(str(tmp_path), n=9)
    ds.setDirs([str(tmp_path)]); ds.setFileExtension("jpg"); ds.setHeight(32); ds.setWidth(32)
    ds.colorSpace = cs
    try:
        ds.seed(5)
        ref = [ds.loadRandomImages(6).scaled for _ in range(4)]
        ds.seed(5)
        ld = ds.AsyncLoader(6)
        assert ld.C == 3
        keep = []
        for e in range(4):
            pool = ld.next()
            assert cg.adversarial.TrainData(pool).size() == 6 and pool.shape == (6, 3, 32, 32)
            np.testing.assert_array_equal(cg.nn.as_nhwc(pool).numpy(), ref[e])
            keep.append(pool.t.sum())            # work on the training stream that reads this pool while the next one loads
        torch.cuda.synchronize()
        ld.close()
        ds.seed(7)
        few_ref = ds.loadRandomImages(20).scaled
        ds.seed(7)
        ld = ds.AsyncLoader(20)
        few = ld.next()
        assert few.shape[0] == 9
        np.testing.assert_array_equal(cg.nn.as_nhwc(few).numpy(), few_ref)
        ld.close()
        rs = np.random.RandomState(11)
        for k, (hh, ww) in enumerate(((48, 80), (64, 40), (100, 100))):
            Image.fromarray(rs.randint(0, 256, size=(hh, ww, 3)).astype(np.uint8)).save(os.path.join(str(tmp_path), f"odd{k}.jpg"), quality=95)
        ds.setDirs([str(tmp_path)])
        ds.seed(9)
        mixed_ref = [ds.loadRandomImages(12).scaled for _ in range(2)]
        ds.seed(9)
        ld = ds.AsyncLoader(12)
        for e in range(2):
            np.testing.assert_array_equal(cg.nn.as_nhwc(ld.next()).numpy(), mixed_ref[e])
        ld.close()
        if cs == "hsl":      # the pool really is in the new space: converted back on the device it is the rgb the blocking loader reads,
            ds.colorSpace = "rgb"      # to the bound of the hsl round trip (tests/test_colorspace_host.py; yuv's matrices are no exact inverses)
            ds.seed(9)
            rgb = ds.loadRandomImages(12).scaled
            assert np.abs(cg.nn_utils.toRgb(cg.Tensor.from_numpy(mixed_ref[0]), cs) - rgb).max() <= 2.5e-5
    finally:
        ds.colorSpace = "rgb"
        ds.seed(1)


# ---------------------------------------------------------------- 9. the CLIs
@pytest.mark.parametrize("cs", ["hsl", "yuv"])
def test_train_and_sample_clis_run_in_the_colour_space(tmp_path, cs):
    from PIL import Image
    logs = tmp_path / "logs"
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--synthetic", "--colorSpace", cs, "--epochs", "1", "--N_epoch", "64",
           "--batchSize", "16", "--saveFreq", "1", "--save", str(logs)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Number of free parameters in D: 6664777" in out.stdout          # three planes
    for sub, side in (("images", 10), ("images_good", 7), ("images_bad", 7)):
        files = sorted(os.listdir(str(logs / sub)))
        assert len(files) == 1 and files[0].endswith(".png"), (sub, files)
        im = np.asarray(Image.open(str(logs / sub / files[0])))
        assert im.shape == (side * 32 + 7, side * 32, 3), (sub, im.shape)
    assert (logs / "adversarial.net").exists()
    data = tmp_path / "data"
    os.makedirs(str(data))
    make_jpgs(str(data), n=12)
    dst = tmp_path / "samples"
    cmd = [sys.executable, os.path.join(ROOT, "sample.py"), "--save", str(logs), "--colorSpace", cs, "--nSamples", "64",
           "--dataDir", str(data), "--writeto", str(dst)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    for name in ("trainset_s1_0001_base.jpg", "random256_0001_base.jpg", "random1024_0001_base.jpg", "best_0001_base.jpg",
                 "worst_0001_base.jpg", "random_0001_base.jpg"):
        im = np.asarray(Image.open(str(dst / name)))
        assert im.ndim == 3 and im.shape[2] == 3, (name, im.shape)
