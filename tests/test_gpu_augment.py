"""On-the-fly augmentation on the MI355X: cg_images_u8_augment_to_f32 bit-equal to dataset.augment_images -> image_scale ->
rgbToColorSpace (whose own yardsticks are in tests/test_augment_host.py) and, with the identity descriptor, to
cg_images_u8_scale_to_f32; its argument checks; AsyncLoader's augmented pools against the blocking loader's; train.py --augment end to
end, twice, to the same checkpoint."""
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
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 1, 0], np.float32)
# Hs, Ws, h, w.  The last three: image.scale's two axes in different branches of its footprint rule (down / up, equal / down, up / equal)
GEOMETRIES = [(64, 64, 32, 32), (64, 64, 64, 64), (32, 32, 64, 64), (96, 60, 32, 24), (13, 4, 5, 9), (7, 11, 7, 4), (5, 11, 13, 11)]


@pytest.fixture(scope="module")
def cg():
    assert torch.cuda.is_available()
    return importlib.import_module("cat-generator_amd")


@pytest.fixture()
def ds():
    d = importlib.import_module("cat-generator_amd.dataset")
    yield d
    d.setAugmentation(False)
    d.colorSpace = "rgb"
    d.setHeight(32); d.setWidth(32)
    d.seed(1)


def _device(cg, u8, desc, h, w, cs, sigma, seed, offset):
    N, Hs, Ws, _ = u8.shape
    src, dsc = torch.from_numpy(u8).cuda(), torch.from_numpy(np.ascontiguousarray(desc, dtype=np.float32)).cuda()
    dst = cg.Tensor.empty((N, 1 if cs == "y" else 3, h, w), "nhwc")
    cg.lib().images_u8_augment_to_f32(cg.tensor.stream(), src.data_ptr(), dst.ptr, N, Hs, Ws, h, w, CODE[cs], dsc.data_ptr(), sigma, seed, offset)
    return dst.numpy()


def _host(ds, u8, desc, h, w, cs, sigma, seed, offset):
    warped = ds.augment_images(u8, desc, sigma, seed, offset)
    return ds.rgbToColorSpace(np.stack([ds.image_scale(im, w, h) for im in warped]), cs)


# ---------------------------------------------------------------- 7. kernel against the host restatement
@pytest.mark.parametrize("cs", ["rgb", "y", "yuv", "hsl"])
@pytest.mark.parametrize("Hs,Ws,h,w", GEOMETRIES)
def test_kernel_equals_the_host_restatement_bit_for_bit(cg, ds, cs, Hs, Ws, h, w):
    seed, offset = 0x5DEECE66D1234567, 987654321
    for N in (1, 5, 257):
        rs = np.random.RandomState(N + Hs + h)
        u8 = rs.randint(0, 256, size=(N, Hs, Ws, 3)).astype(np.uint8)
        if cs == "hsl":      # grey pixels and ties between channels
            u8[0, : Hs // 4] = u8[0, : Hs // 4, :, :1]
        ds.seed(N)
        ds.setAugmentation(True)
        desc = ds.augment_descriptors(N, Hs, Ws)
        assert desc[:, 7].any() or N == 1
        got = _device(cg, u8, desc, h, w, cs, 0.02, seed, offset)
        np.testing.assert_array_equal(got, _host(ds, u8, desc, h, w, cs, 0.02, seed, offset), err_msg=f"N={N}")
    # extreme descriptors: every clamp branch of both axes, positions far outside the image, a flip among them
    draws = [(0.5, 0, 0, 0), (2.0, 0, 0, 0), (1.0, 45, 0, 0), (1.0, -45, 0, 0), (1.0, 0, Ws, 0), (1.0, 0, -Ws, 0), (1.0, 0, 0, Hs),
             (1.0, 0, 0, -Hs), (0.5, 45, Ws, -Hs), (2.0, -45, -Ws, Hs)]
    n = len(draws)
    draw = dict(scale=[d[0] for d in draws], rotation=[d[1] for d in draws], tx=[d[2] for d in draws], ty=[d[3] for d in draws],
                brightness=[0.85 + 0.03 * i for i in range(n)], flip=[i % 2 for i in range(n)])
    desc = ds.augment_descriptors(n, Hs, Ws, draw)
    u8 = np.random.RandomState(77).randint(0, 256, size=(n, Hs, Ws, 3)).astype(np.uint8)
    got = _device(cg, u8, desc, h, w, cs, 0.02, seed, offset)
    np.testing.assert_array_equal(got, _host(ds, u8, desc, h, w, cs, 0.02, seed, offset), err_msg="extremes")


# ---------------------------------------------------------------- 8. identity = the scaling kernel
@pytest.mark.parametrize("cs", ["rgb", "y", "yuv", "hsl"])
def test_identity_descriptor_equals_the_scaling_kernel(cg, cs):
    for (Hs, Ws, h, w) in GEOMETRIES:
        u8 = np.random.RandomState(Hs + w).randint(0, 256, size=(5, Hs, Ws, 3)).astype(np.uint8)
        src = torch.from_numpy(u8).cuda()
        want = cg.Tensor.empty((5, 1 if cs == "y" else 3, h, w), "nhwc")
        cg.lib().images_u8_scale_to_f32(cg.tensor.stream(), src.data_ptr(), want.ptr, 5, Hs, Ws, h, w, CODE[cs])
        got = _device(cg, u8, np.tile(IDENTITY, (5, 1)), h, w, cs, 0.0, 3, 4)
        np.testing.assert_array_equal(got, want.numpy(), err_msg=f"{Hs}x{Ws} -> {h}x{w}")


# ---------------------------------------------------------------- 9. argument checks
def test_bad_arguments_are_refused_before_any_launch(cg):
    u8 = torch.zeros((2, 64, 64, 3), dtype=torch.uint8).cuda()
    big = torch.zeros((1, 256, 256, 3), dtype=torch.uint8).cuda()
    desc = torch.from_numpy(np.tile(IDENTITY, (2, 1))).cuda()
    dst = cg.Tensor.from_numpy(np.full((2, 3, 64, 64), -1.0, np.float32))
    s, f = cg.tensor.stream(), cg.lib().images_u8_augment_to_f32
    for args in ((None, dst.ptr, 2, 64, 64, 32, 32, 0, desc.data_ptr(), 0.02, 1, 0),
                 (u8.data_ptr(), None, 2, 64, 64, 32, 32, 0, desc.data_ptr(), 0.02, 1, 0),
                 (u8.data_ptr(), dst.ptr, 2, 64, 64, 32, 32, 0, None, 0.02, 1, 0),
                 (u8.data_ptr(), dst.ptr, 2, 64, 64, 32, 32, -1, desc.data_ptr(), 0.02, 1, 0),
                 (u8.data_ptr(), dst.ptr, 2, 64, 64, 32, 32, 4, desc.data_ptr(), 0.02, 1, 0),
                 (u8.data_ptr(), dst.ptr, 0, 64, 64, 32, 32, 0, desc.data_ptr(), 0.02, 1, 0),
                 (u8.data_ptr(), dst.ptr, 2, 64, 64, 32, 32, 0, desc.data_ptr(), -0.5, 1, 0)):
        with pytest.raises(cg.CatganError, match="bad arguments"):
            f(s, *args)
    with pytest.raises(cg.CatganError, match="more than 6"):
        f(s, u8.data_ptr(), dst.ptr, 2, 64, 64, 8, 8, 0, desc.data_ptr(), 0.02, 1, 0)
    with pytest.raises(cg.CatganError, match="LDS"):      # 256 x 256 x 12 bytes = 768 KB: no workgroup has that
        f(s, big.data_ptr(), dst.ptr, 1, 256, 256, 64, 64, 0, desc.data_ptr(), 0.02, 1, 0)
    torch.cuda.synchronize()
    assert np.all(dst.numpy() == -1.0)


# ---------------------------------------------------------------- 10. the two loaders
@pytest.mark.parametrize("cs", ["rgb", "hsl"])
def test_async_loader_augmented_pools_equal_the_blocking_loader(cg, ds, tmp_path, cs):
    from PIL import Image
    make_jpgs(str(tmp_path), n=9)
    Image.fromarray(np.random.RandomState(11).randint(0, 256, size=(48, 80, 3)).astype(np.uint8)).save(str(tmp_path / "odd.jpg"), quality=95)
    ds.setDirs([str(tmp_path)]); ds.setFileExtension("jpg"); ds.setHeight(32); ds.setWidth(32)
    ds.colorSpace = cs
    ds.setAugmentation(True)
    ds.seed(5)
    plain_first = None
    for count in (7, 20):      # 20: more than the directory holds - partial pools of all 10 files, the odd one always among them
        ds.seed(5)
        ref = [ds.loadRandomImages(count).scaled for _ in range(3)]
        ds.seed(5)
        ld = ds.AsyncLoader(count)
        assert ld.aug and not ld.host_all
        keep = []
        for e in range(3):
            pool = ld.next()
            assert pool.shape == (min(count, 10), 3, 32, 32)
            np.testing.assert_array_equal(cg.nn.as_nhwc(pool).numpy(), ref[e], err_msg=f"count {count} pool {e}")
            keep.append(pool.t.sum())
        torch.cuda.synchronize()
        ld.close()
        assert not np.array_equal(ref[0], ref[1])
    ds.setAugmentation(False)      # and the pools really are augmented: the same files without it differ
    ds.seed(5)
    plain_first = ds.loadRandomImages(20).scaled
    assert not np.array_equal(plain_first, ref[0])


# ---------------------------------------------------------------- 11. train.py --augment
def test_train_cli_with_augment_is_reproducible(tmp_path):
    from PIL import Image
    data = tmp_path / "data"
    os.makedirs(str(data))
    make_jpgs(str(data), n=40)
    Image.fromarray(np.random.RandomState(12).randint(0, 256, size=(64, 40, 3)).astype(np.uint8)).save(str(data / "odd.jpg"), quality=95)
    saved = []
    for run in ("a", "b"):
        os.makedirs(str(tmp_path / run))
        logs = tmp_path / run / "logs"      # the checkpoint stores the options: the same relative --save from two directories
        cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "train.py"), "--augment", "--batchSize", "16", "--N_epoch", "32",
               "--epochs", "2", "--dataDir", str(data), "--save", "logs", "--saveFreq", "1"]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=700, cwd=str(tmp_path / run))
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.count("<trainer> Epoch #") == 2
        for sub in ("images", "images_good", "images_bad"):
            files = sorted(os.listdir(str(logs / sub)))
            assert len(files) == 2 and all(f.endswith(".png") for f in files), (sub, files)
        assert (logs / "adversarial.npz").exists() and (logs / "adversarial.net").exists()
        saved.append(np.load(str(logs / "adversarial.npz"), allow_pickle=False))
    a, b = saved
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
