"""On-the-fly augmentation on the host (dataset.setAugmentation / augment_draw / augment_descriptors / augment_noise / augment_images:
the restatement of dataset/dataset.py:284-306 and dataset/ImageAugmenter.py:160-190 that cg_images_u8_augment_to_f32 repeats on the
device, tests/test_gpu_augment.py).  The warp's independent yardstick is scipy.ndimage.map_coordinates in fp64; the noise is checked
against Python-integer splitmix64 and by its moments; the descriptors by their ranges and by what they consume of the loader's
generator."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import make_jpgs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 1, 0], np.float32)
GEOMETRIES = [(64, 64, 32, 32), (64, 64, 64, 64), (32, 32, 64, 64), (96, 60, 32, 24)]      # Hs, Ws, h, w


@pytest.fixture()
def ds():
    d = importlib.import_module("cat-generator_amd.dataset")
    yield d
    d.setAugmentation(False)
    d.colorSpace = "rgb"
    d.setHeight(32); d.setWidth(32)
    d.seed(1)


# ---------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("cs", ["rgb", "y", "yuv", "hsl"])
@pytest.mark.parametrize("Hs,Ws,h,w", GEOMETRIES)
def test_identity_descriptor_is_the_plain_loader(ds, cs, Hs, Ws, h, w):
    u8 = np.random.RandomState(Hs + w).randint(0, 256, size=(3, Hs, Ws, 3)).astype(np.uint8)
    desc = np.tile(IDENTITY, (3, 1))
    warped = ds.augment_images(u8, desc, 0.0, seed=5, offset=7)
    got = ds.rgbToColorSpace(np.stack([ds.image_scale(im, w, h) for im in warped]), cs)
    plain = u8.astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255.0)
    want = ds.rgbToColorSpace(np.stack([ds.image_scale(im, w, h) for im in plain]), cs)
    np.testing.assert_array_equal(warped, plain)
    np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------- 2. the warp against scipy in fp64
def test_warp_against_map_coordinates_in_fp64(ds):
    """300 descriptors from the default ranges on a uniform-random 64 x 64 x 3 image (the steepest gradients there are).  Bound 1e-4
    absolute, derived, not measured: a source coordinate <= 64 carries <= 3 fp32 roundings (<= 2.3e-5 px), neighbouring values differ
    by <= 1, two axes, plus the roundings of the three lerps (a few 6e-8).  A wrong tap or a transposed matrix is O(0.1)."""
    from scipy.ndimage import map_coordinates
    ds.seed(11)
    ds.setAugmentation(True)
    draw = ds.augment_draw(300)
    desc = ds.augment_descriptors(300, 64, 64, draw)
    desc[:, 6], desc[:, 7] = 1, 0                                     # the warp alone: brightness 1, no flip
    u8 = np.random.RandomState(2).randint(0, 256, size=(1, 64, 64, 3)).astype(np.uint8)
    src = u8[0].astype(np.float64) / 255.0
    ys, xs = np.mgrid[0:64, 0:64].astype(np.float64)
    worst = 0.0
    for i in range(300):
        got = ds.augment_images(u8, desc[i:i + 1], 0.0, 0, 0)[0]
        inv = np.linalg.inv(ds.augment_matrix(draw["scale"][i], draw["rotation"][i], draw["tx"][i], draw["ty"][i], 64, 64))
        sx = inv[0, 0] * xs + inv[0, 1] * ys + inv[0, 2]
        sy = inv[1, 0] * xs + inv[1, 1] * ys + inv[1, 2]
        for c in range(3):
            want = map_coordinates(src[:, :, c], [sy, sx], order=1, mode="nearest")
            worst = max(worst, float(np.abs(got[c] - want).max()))
    print(f"max |augment_images - map_coordinates(fp64)| over 300 descriptors: {worst:.3e}")
    assert worst <= 1e-4


def test_forward_matrix_is_skimage_s_composition(ds):
    """to_center . A . to_topleft: the image centre (int(W/2), int(H/2)) maps to itself plus the translation, a point one pixel to
    its right to the centre + s (cos r, sin r) + t (AffineTransform's rotation convention), and the descriptor is the inverse."""
    M = ds.augment_matrix(1.25, 30, 3, -2, 60, 96)
    c = np.array([48, 30, 1.0])
    np.testing.assert_allclose(M @ c, [48 + 3, 30 - 2, 1], atol=1e-12)
    r = np.deg2rad(30)
    np.testing.assert_allclose(M @ (c + [1, 0, 0]), [51 + 1.25 * np.cos(r), 28 + 1.25 * np.sin(r), 1], atol=1e-12)
    draw = dict(scale=[1.25], rotation=[30], tx=[3], ty=[-2], brightness=[1.1], flip=[1])
    d = ds.augment_descriptor(draw, 0, 60, 96)
    assert d.dtype == np.float32 and d.shape == (8,)
    np.testing.assert_array_equal(d[:6], np.linalg.inv(M)[:2].reshape(6).astype(np.float32))
    assert d[6] == np.float32(1.1) and d[7] == 1


# ---------------------------------------------------------------- 3. exact cases
def test_flip_translation_and_brightness_exactly(ds):
    u8 = np.random.RandomState(4).randint(0, 256, size=(1, 64, 64, 3)).astype(np.uint8)
    p = u8[0].astype(np.float32).transpose(2, 0, 1) / np.float32(255.0)
    flip = IDENTITY.copy(); flip[7] = 1
    np.testing.assert_array_equal(ds.augment_images(u8, flip[None], 0.0, 0, 0)[0], p[:, :, ::-1])
    # tx = 3 through the real path: forward matrix -> inverse -> descriptor; the output shows p[y][x - 3], the edge column left of it
    draw = dict(scale=[1.0], rotation=[0], tx=[3], ty=[0], brightness=[1.0], flip=[0])
    d = ds.augment_descriptor(draw, 0, 64, 64)
    np.testing.assert_array_equal(d, np.array([1, 0, -3, 0, 1, 0, 1, 0], np.float32))
    out = ds.augment_images(u8, d[None], 0.0, 0, 0)[0]
    np.testing.assert_array_equal(out[:, :, 3:], p[:, :, :-3])
    np.testing.assert_array_equal(out[:, :, :3], np.repeat(p[:, :, :1], 3, axis=2))
    # brightness: 255 * 1.15 clips to exactly 1, a darker byte is one fp32 product
    u8[0, 0, 0] = (255, 255, 100)
    b = IDENTITY.copy(); b[6] = 1.15
    out = ds.augment_images(u8, b[None], 0.0, 0, 0)[0]
    assert out[0, 0, 0] == 1.0 and out[1, 0, 0] == 1.0
    assert out[2, 0, 0] == (np.float32(100) / np.float32(255)) * np.float32(1.15)
    assert out.max() <= 1.0 and out.min() >= 0.0


# ---------------------------------------------------------------- 4. the noise
def _splitmix_py(seed, ctr):
    M = (1 << 64) - 1
    z = (seed + (ctr + 1) * 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def test_noise_known_answers_and_moments(ds):
    seed, offset = 0x1234567890ABCDEF, 1000003
    js = [0, 1, 2, 12287, 12288, 10000 * 12288 + 5, (1 << 40) + 17]
    want = []
    for j in js:
        S = 0
        for k in range(3):
            z = _splitmix_py(seed, offset + 3 * j + k)
            S += sum((z >> sh) & 0xFFFF for sh in (0, 16, 32, 48))
        want.append(np.float32(S - 393210) / np.float32(65536.0))
    got = ds.augment_noise(seed, offset, np.array(js, np.uint64))
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, np.array(want, np.float32))
    # the generator is the engine's own: SplitMix.u01 is the top 24 bits of the same outputs
    T = importlib.import_module("cat-generator_amd.tensor")
    sm = T.SplitMix(7); sm.offset = 30
    assert sm.u01(1)[0] == np.float32(_splitmix_py(7, 30) >> 40) / np.float32(16777216.0)
    n = 200000
    z = ds.augment_noise(99, 5, np.arange(n)).astype(np.float64)
    print(f"noise over {n} samples: mean {z.mean():+.3e} std {z.std():.6f} min {z.min():.3f} max {z.max():.3f}")
    assert abs(z.mean()) <= 4 / np.sqrt(n)
    assert abs(z.std() - 1) <= 4 / np.sqrt(2 * n)
    assert z.min() >= -6 and z.max() <= 6
    # in the images: sigma scales it, index0 places an image in its pool, and the counters follow j = ((n Hs + y) Ws + x) 3 + c
    u8 = np.full((2, 8, 6, 3), 128, np.uint8)
    out = ds.augment_images(u8, np.tile(IDENTITY, (2, 1)), 0.02, seed, offset, index0=3)
    j = np.arange(2 * 8 * 6 * 3).reshape(2, 8, 6, 3) + 3 * 8 * 6 * 3
    want = (np.float32(128) / np.float32(255)) * np.float32(1) + np.float32(0.02) * ds.augment_noise(seed, offset, j)
    np.testing.assert_array_equal(out, want.transpose(0, 3, 1, 2))


# ---------------------------------------------------------------- 5. descriptors and the generator
def test_descriptor_draws(ds, tmp_path):
    n = 10000
    ds.seed(21)
    ds.setAugmentation(True)
    d = ds.augment_draw(n)
    assert set(np.unique(d["flip"])) == {0, 1}
    assert abs(d["flip"].mean() - 0.5) <= 4 * 0.5 / np.sqrt(n)
    assert d["scale"].min() >= 0.93 and d["scale"].max() <= 1.08 and d["scale"].max() - d["scale"].min() > 0.14
    for k, lim in (("rotation", 8), ("tx", 4), ("ty", 4)):
        assert d[k].dtype.kind == "i" and set(np.unique(d[k])) == set(range(-lim, lim + 1)), k
    assert d["brightness"].min() >= 0.85 and d["brightness"].max() <= 1.15 and d["brightness"].max() - d["brightness"].min() > 0.29
    assert 0 <= d["seed"] < 2 ** 63 and d["noise_std"] == 0.02
    ds.seed(21)
    d2 = ds.augment_draw(n)
    assert all(np.array_equal(d[k], d2[k]) for k in d)
    ds.seed(21)
    a = ds.augment_descriptors(50, 64, 64)                      # draws for itself
    ds.seed(21)
    np.testing.assert_array_equal(a, ds.augment_descriptors(50, 64, 64, ds.augment_draw(50)))
    assert not np.array_equal(a, ds.augment_descriptors(50, 64, 64))
    # overrides reach the draws
    ds.setAugmentation(True, hflip=False, scale=(1.0, 1.0), rotation=0, translation=0, brightness=0.0, noise_std=0.0)
    np.testing.assert_array_equal(ds.augment_descriptors(5, 64, 64), np.tile(IDENTITY, (5, 1)))
    with pytest.raises(TypeError):
        ds.setAugmentation(True, shear=3)
    with pytest.raises(ValueError):
        ds.setAugmentation(True, scale=(0.0, 1.0))


def test_generator_consumption_and_checkpoint(ds, tmp_path):
    make_jpgs(str(tmp_path), n=9)
    ds.setDirs([str(tmp_path)]); ds.setFileExtension("jpg")
    # off: nothing beyond the permutations is consumed
    assert ds.augmentation is None
    ds.seed(3)
    picks = [ds._pick(5) for _ in range(3)]
    ds.loadRandomImages(5)
    fresh = np.random.RandomState(3)
    for p in picks:
        perm = fresh.permutation(9)
        assert p == [ds.paths[perm[i]] for i in range(5)]
    ds.seed(3)
    ds.loadRandomImages(5); ds.loadRandomImages(5)
    fresh = np.random.RandomState(3)
    fresh.permutation(9); fresh.permutation(9)
    assert ds._rs.randint(0, 1 << 30) == fresh.randint(0, 1 << 30)
    # on: the draws follow each pick, and a checkpoint taken between two pools (blocking: the current state; asynchronous: the state
    # from before the pending pick) brings back the same files AND the same descriptors
    ds.setAugmentation(True)
    ds.seed(3)
    run = []
    for _ in range(4):
        files = ds._pick(5)
        run.append((files, ds.augment_draw(5)))
    assert run[0][0] == picks[0] and run[1][0] != picks[1]      # the draws moved the generator
    ds.seed(3)
    ds._pick(5); ds.augment_draw(5)
    st = ds.checkpoint_state()
    ds.seed(99); ds.restore_state(st)
    files, d = ds._pick(5), ds.augment_draw(5)
    assert files == run[1][0] and all(np.array_equal(d[k], run[1][1][k]) for k in d)
    ds.seed(3)
    ds._prefetch_pick(5); ds.augment_draw(5)                     # AsyncLoader: pool 1 consumed ...
    ds._prefetch_pick(5); ds.augment_draw(5)                     # ... pool 2 pending when the checkpoint is written
    st = ds.checkpoint_state()
    ds.seed(98); ds.restore_state(st)
    files, d = ds._prefetch_pick(5), ds.augment_draw(5)
    assert files == run[1][0] and all(np.array_equal(d[k], run[1][1][k]) for k in d)
    # the blocking loader end to end: same seed -> same pool, augmented pools differ from the plain ones and from each other
    ds.seed(5)
    a = ds.loadRandomImages(4).scaled
    b = ds.loadRandomImages(4).scaled
    ds.seed(5)
    np.testing.assert_array_equal(ds.loadRandomImages(4).scaled, a)
    assert a.shape == (4, 3, 32, 32) and a.dtype == np.float32 and not np.array_equal(a, b)
    assert a.min() >= 0 and a.max() <= 1
    ds.setAugmentation(False)
    ds.seed(5)
    plain = ds.loadRandomImages(4).scaled
    assert 0.005 < np.abs(a - plain).mean() < 0.2               # the same faces, moved a little


# ---------------------------------------------------------------- 6. the CLIs
@pytest.mark.parametrize("script", ["train.py", "train_v.py"])
def test_cli_lists_the_switches_and_defaults_to_off(script):
    out = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    for flag in ("--augment", "--augNoFlip", "--augScale", "--augRotation", "--augTranslation", "--augBrightness", "--augNoise"):
        assert flag in out.stdout, flag
    assert "UN-augmented" in out.stdout
    sys.path.insert(0, ROOT)
    try:
        mod = importlib.import_module(script[:-3])
    finally:
        sys.path.remove(ROOT)
    argv, sys.argv = sys.argv, [script]
    try:
        o = mod.parse()
    finally:
        sys.argv = argv
    assert o.augment is False and o.augNoFlip is False
    ds = importlib.import_module("cat-generator_amd.dataset")
    assert (tuple(o.augScale), o.augRotation, o.augTranslation, o.augBrightness, o.augNoise) == \
        (ds.AUG_DEFAULTS["scale"], ds.AUG_DEFAULTS["rotation"], ds.AUG_DEFAULTS["translation"], ds.AUG_DEFAULTS["brightness"],
         ds.AUG_DEFAULTS["noise_std"])
    assert ds.augmentation is None
