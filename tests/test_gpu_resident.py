"""The training set resident on the MI355X: cg_images_u8_gather_scale_to_f32 / cg_images_u8_gather_augment_to_f32 bit-equal to the
non-gather entry points on set[idx] (and to the host restatement), their out-of-range rule, a set beyond 2^31 bytes, their argument
checks; dataset.ResidentLoader's pools against loadRandomImages', across a checkpoint; ResidentSet.chunks against the file order; and
train.py / sample.py --neighbours picking a pack up by themselves, to the same results as without one."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import make_jpgs
from test_gpu_augment import CODE, GEOMETRIES, IDENTITY

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M_SET = 37
SEED, OFFSET, SIGMA = 0x5DEECE66D1234567, 987654321, 0.02


@pytest.fixture(scope="module")
def cg():
    assert torch.cuda.is_available()
    return importlib.import_module("cat-generator_amd")


@pytest.fixture()
def ds():
    d = importlib.import_module("cat-generator_amd.dataset")
    d.setFileExtension("jpg")
    yield d
    d.setAugmentation(False)
    d.colorSpace = "rgb"
    d.setHeight(32); d.setWidth(32)
    d.setDirs([])
    d.seed(1)


def _out(cg, N, cs, h, w, fill=-1.0):
    return cg.Tensor.from_numpy(np.full((N, 1 if cs == "y" else 3, h, w), fill, np.float32))


def _plain(cg, src, N, Hs, Ws, h, w, cs, desc=None):
    """the existing entry points on N materialised images (src: a device uint8 tensor)"""
    dst = _out(cg, N, cs, h, w)
    if desc is None:
        cg.lib().images_u8_scale_to_f32(cg.tensor.stream(), src.data_ptr(), dst.ptr, N, Hs, Ws, h, w, CODE[cs])
    else:
        cg.lib().images_u8_augment_to_f32(cg.tensor.stream(), src.data_ptr(), dst.ptr, N, Hs, Ws, h, w, CODE[cs], desc.data_ptr(), SIGMA, SEED, OFFSET)
    return dst.numpy()


def _gather(cg, dev_set, M, idx, N, Hs, Ws, h, w, cs, desc=None):
    """the gather entry points on the set in place (idx: a device int32 tensor)"""
    dst = _out(cg, N, cs, h, w)
    if desc is None:
        cg.lib().images_u8_gather_scale_to_f32(cg.tensor.stream(), dev_set.data_ptr(), M, idx.data_ptr(), dst.ptr, N, Hs, Ws, h, w, CODE[cs])
    else:
        cg.lib().images_u8_gather_augment_to_f32(cg.tensor.stream(), dev_set.data_ptr(), M, idx.data_ptr(), dst.ptr, N, Hs, Ws, h, w, CODE[cs],
                                                 desc.data_ptr(), SIGMA, SEED, OFFSET)
    return dst.numpy()


def _descriptors(ds, N, Hs, Ws):
    ds.seed(N)
    ds.setAugmentation(True)
    return ds.augment_descriptors(N, Hs, Ws)


# ---------------------------------------------------------------- 1. the kernels against the non-gather ones on set[idx]
@pytest.mark.parametrize("cs", ["rgb", "y", "yuv", "hsl"])
@pytest.mark.parametrize("Hs,Ws,h,w", GEOMETRIES)
def test_gather_equals_the_plain_kernels_on_the_materialised_images(cg, ds, cs, Hs, Ws, h, w):
    u8 = np.random.RandomState(Hs + h).randint(0, 256, size=(M_SET, Hs, Ws, 3)).astype(np.uint8)
    if cs == "hsl":      # grey pixels and ties between channels
        u8[0, : Hs // 4] = u8[0, : Hs // 4, :, :1]
    dev_set = torch.from_numpy(u8).cuda()
    for N in (1, 5, 257):
        idx = np.random.RandomState(N).randint(0, M_SET, size=N).astype(np.int32)
        if N == 5:
            idx[:] = [36, 0, 36, 3, 0]      # repeats, out of order, both ends of the set
        assert N == 1 or (len(set(idx.tolist())) < N and (np.diff(idx) < 0).any())
        dev_idx = torch.from_numpy(idx).cuda()
        picked = dev_set[dev_idx.long()].contiguous()      # set[idx] materialised by torch
        desc = _descriptors(ds, N, Hs, Ws)
        dev_desc = torch.from_numpy(desc).cuda()
        got_s = _gather(cg, dev_set, M_SET, dev_idx, N, Hs, Ws, h, w, cs)
        got_a = _gather(cg, dev_set, M_SET, dev_idx, N, Hs, Ws, h, w, cs, dev_desc)
        np.testing.assert_array_equal(got_s, _plain(cg, picked, N, Hs, Ws, h, w, cs), err_msg=f"scale N={N}")
        np.testing.assert_array_equal(got_a, _plain(cg, picked, N, Hs, Ws, h, w, cs, dev_desc), err_msg=f"augment N={N}")
        if (Hs, Ws, h, w) == GEOMETRIES[0] and N <= 5:      # and against the host restatement
            flt = u8[idx].astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255.0)
            np.testing.assert_array_equal(got_s, ds.rgbToColorSpace(np.stack([ds.image_scale(im, w, h) for im in flt]), cs), err_msg=f"host scale N={N}")
            warped = ds.augment_images(u8[idx], desc, SIGMA, SEED, OFFSET)
            np.testing.assert_array_equal(got_a, ds.rgbToColorSpace(np.stack([ds.image_scale(im, w, h) for im in warped]), cs), err_msg=f"host augment N={N}")


# ---------------------------------------------------------------- 2. an index outside the set
@pytest.mark.parametrize("cs", ["rgb", "y"])
def test_out_of_range_indices_give_zero_images(cg, ds, cs):
    Hs, Ws, h, w = GEOMETRIES[0]
    u8 = np.random.RandomState(9).randint(1, 256, size=(M_SET, Hs, Ws, 3)).astype(np.uint8)
    dev_set = torch.from_numpy(u8).cuda()
    idx = np.array([3, -1, 0, M_SET, 36], np.int32)
    good = np.array([0, 2, 4])
    dev_idx = torch.from_numpy(idx).cuda()
    desc = _descriptors(ds, 5, Hs, Ws)
    dev_desc = torch.from_numpy(desc).cuda()
    safe = torch.from_numpy(np.where((idx >= 0) & (idx < M_SET), idx, 0)).cuda()
    picked = dev_set[safe.long()].contiguous()
    for d in (None, dev_desc):
        got = _gather(cg, dev_set, M_SET, dev_idx, 5, Hs, Ws, h, w, cs, d)
        want = _plain(cg, picked, 5, Hs, Ws, h, w, cs, d)
        assert np.all(got[[1, 3]] == 0.0) and not np.signbit(got[[1, 3]]).any()
        np.testing.assert_array_equal(got[good], want[good])
        assert (want[good] != 0).any()


# ---------------------------------------------------------------- 3. a set beyond 2^31 bytes
def test_a_set_beyond_two_gib_is_addressed_with_64_bits(cg, ds):
    Hs, Ws, h, w = GEOMETRIES[0]
    M, per = 180_000, Hs * Ws * 3
    rows = [0, 174_762, 174_763, 179_999]
    assert rows[1] * per < 2 ** 31 < (rows[1] + 1) * per      # that image straddles the 2^31st byte
    big = torch.empty(M * per, dtype=torch.uint8, device="cuda").view(M, Hs, Ws, 3)      # 2.2 GB; only the four rows are written
    u8 = np.random.RandomState(4).randint(0, 256, size=(4, Hs, Ws, 3)).astype(np.uint8)
    four = torch.from_numpy(u8).cuda()
    for k, r in enumerate(rows):
        big[r] = four[k]
    dev_idx = torch.tensor(rows, dtype=torch.int32).cuda()
    dev_desc = torch.from_numpy(_descriptors(ds, 4, Hs, Ws)).cuda()
    for d in (None, dev_desc):
        got = _gather(cg, big, M, dev_idx, 4, Hs, Ws, h, w, "rgb", d)
        np.testing.assert_array_equal(got, _plain(cg, four, 4, Hs, Ws, h, w, "rgb", d))
    del big


# ---------------------------------------------------------------- 4. argument checks
def test_bad_arguments_are_refused_before_any_launch(cg):
    u8 = torch.zeros((2, 64, 64, 3), dtype=torch.uint8).cuda()
    big = torch.zeros((1, 256, 256, 3), dtype=torch.uint8).cuda()
    idx = torch.zeros(2, dtype=torch.int32).cuda()
    desc = torch.from_numpy(np.tile(IDENTITY, (2, 1))).cuda()
    dst = cg.Tensor.from_numpy(np.full((2, 3, 64, 64), -1.0, np.float32))
    s, fs, fa = cg.tensor.stream(), cg.lib().images_u8_gather_scale_to_f32, cg.lib().images_u8_gather_augment_to_f32
    S, I, D, E = u8.data_ptr(), idx.data_ptr(), dst.ptr, desc.data_ptr()
    geo = (64, 64, 32, 32)
    for head in ((None, 2, I, D, 2), (S, 2, None, D, 2), (S, 2, I, None, 2), (S, 0, I, D, 2), (S, -3, I, D, 2), (S, 2, I, D, 0), (S, 2, I, D, -1)):
        with pytest.raises(cg.CatganError, match="bad arguments"):
            fs(s, *head, *geo, 0)
        with pytest.raises(cg.CatganError, match="bad arguments"):
            fa(s, *head, *geo, 0, E, 0.02, 1, 0)
    for code in (-1, 4):
        with pytest.raises(cg.CatganError, match="bad arguments"):
            fs(s, S, 2, I, D, 2, *geo, code)
        with pytest.raises(cg.CatganError, match="bad arguments"):
            fa(s, S, 2, I, D, 2, *geo, code, E, 0.02, 1, 0)
    with pytest.raises(cg.CatganError, match="bad arguments"):
        fa(s, S, 2, I, D, 2, *geo, 0, None, 0.02, 1, 0)
    with pytest.raises(cg.CatganError, match="bad arguments"):
        fa(s, S, 2, I, D, 2, *geo, 0, E, -0.5, 1, 0)
    with pytest.raises(cg.CatganError, match="more than 6"):
        fs(s, S, 2, I, D, 2, 64, 64, 8, 8, 0)
    with pytest.raises(cg.CatganError, match="more than 6"):
        fa(s, S, 2, I, D, 2, 64, 64, 8, 8, 0, E, 0.02, 1, 0)
    with pytest.raises(cg.CatganError, match="LDS"):      # 256 x 256 x 12 bytes = 768 KB: no workgroup has that
        fa(s, big.data_ptr(), 1, I, D, 1, 256, 256, 64, 64, 0, E, 0.02, 1, 0)
    torch.cuda.synchronize()
    assert np.all(dst.numpy() == -1.0)


# ---------------------------------------------------------------- 5. the loader
def _resident(ds, d):
    ds.buildPack(d, threads=2)
    pack = ds.openPack(d)
    assert pack is not None
    return ds.ResidentSet(pack)


def _configure(ds, d, cs, aug):
    ds.setDirs([d]); ds.setHeight(32); ds.setWidth(32)
    ds.colorSpace = cs
    ds.setAugmentation(aug)


@pytest.mark.parametrize("aug", [False, True], ids=["plain", "augmented"])
@pytest.mark.parametrize("cs", ["rgb", "hsl"])
def test_resident_loader_pools_equal_the_blocking_loader(cg, ds, tmp_path, cs, aug):
    make_jpgs(str(tmp_path), n=10)
    _configure(ds, str(tmp_path), cs, aug)
    rset = _resident(ds, str(tmp_path))
    assert (rset.M, rset.Hs, rset.Ws) == (10, 64, 64)
    for count in (7, 20):      # 20: more than the directory holds - pools of all 10 files
        ds.seed(5)
        ref = [ds.loadRandomImages(count).scaled for _ in range(3)]
        end = ds._rs.get_state()[1].copy()
        ds.seed(5)
        ld = ds.ResidentLoader(count, rset)
        assert ld.aug == aug
        for e in range(3):
            pool = ld.next()
            assert pool.shape == (min(count, 10), 3, 32, 32) and pool.fmt == "nhwc"
            np.testing.assert_array_equal(cg.nn.as_nhwc(pool).numpy(), ref[e], err_msg=f"count {count} pool {e}")
        np.testing.assert_array_equal(ds._rs.get_state()[1], end)      # the generator is where three blocking loads leave it
        ld.close()
        assert not np.array_equal(ref[0], ref[1])
    rset.close()


def test_resident_loader_refuses_what_the_kernels_cannot_serve(cg, ds, tmp_path):
    make_jpgs(str(tmp_path), n=3)
    _configure(ds, str(tmp_path), "rgb", False)
    rset = _resident(ds, str(tmp_path))
    ds.setHeight(8); ds.setWidth(8)
    with pytest.raises(ValueError, match="more than 6x"):
        ds.ResidentLoader(3, rset)
    with pytest.raises(ValueError, match="more than 6x"):
        rset.chunks(2)
    rset.close()


def test_checkpoint_state_resumes_the_resident_pools(cg, ds, tmp_path):
    make_jpgs(str(tmp_path), n=10)
    _configure(ds, str(tmp_path), "rgb", True)
    rset = _resident(ds, str(tmp_path))
    ds.seed(7)
    ld = ds.ResidentLoader(7, rset)
    first = cg.nn.as_nhwc(ld.next()).numpy()
    state = ds.checkpoint_state()
    rest = [cg.nn.as_nhwc(ld.next()).numpy() for _ in range(2)]
    ld.close()
    ds.seed(99)                      # a fresh process: another generator until the checkpoint is restored
    ld = ds.ResidentLoader(7, rset)
    ds.restore_state(state)
    for e in range(2):
        np.testing.assert_array_equal(cg.nn.as_nhwc(ld.next()).numpy(), rest[e], err_msg=f"pool {e + 2}")
    ld.close()
    rset.close()
    assert not np.array_equal(first, rest[0])


# ---------------------------------------------------------------- 6. one pass over the set
@pytest.mark.parametrize("cs", ["rgb", "y"])
def test_chunks_walk_the_set_in_file_order(cg, ds, tmp_path, cs):
    make_jpgs(str(tmp_path), 20)
    _configure(ds, str(tmp_path), cs, False)
    files = ds.loadPaths()
    ds.seed(5)
    order = [files.index(f) for f in ds.pickFiles(10 ** 9)]
    ds.seed(5)
    shuffled = ds.loadRandomImages(10 ** 9).scaled
    ref = np.empty_like(shuffled)
    ref[order] = shuffled                                      # re-ordered to file order
    rset = _resident(ds, str(tmp_path))
    state = ds._rs.get_state()[1].copy()
    it = rset.chunks(8)
    assert it.files == files
    got, where = [], []
    for pool, index0, n in it:
        got.append(cg.nn.as_nhwc(pool).numpy())
        where.append((index0, n))
    assert where == [(0, 8), (8, 8), (16, 4)] and it.next() is None
    np.testing.assert_array_equal(np.concatenate(got), ref)
    np.testing.assert_array_equal(ds._rs.get_state()[1], state)      # the generator is not touched
    it.close()
    rset.close()


# ---------------------------------------------------------------- 7. the front-ends pick a pack up by themselves
def _run(cmd, cwd, limit=600):
    out = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, timeout=limit + 60, cwd=cwd)
    assert out.returncode == 0, out.stderr[-2000:]
    return out


def test_train_cli_with_a_pack_trains_to_the_same_checkpoint(ds, tmp_path):
    data = tmp_path / "data"
    os.makedirs(str(data))
    make_jpgs(str(data), n=40)
    saved, lines = [], []
    for run in ("files", "pack"):
        os.makedirs(str(tmp_path / run))
        if run == "pack":
            ds.buildPack(str(data), threads=2)
        out = _run([sys.executable, os.path.join(ROOT, "train.py"), "--batchSize", "16", "--N_epoch", "32", "--epochs", "2", "--saveFreq", "1",
                    "--dataDir", str(data), "--save", "logs"], str(tmp_path / run))
        assert out.stdout.count("<trainer> Epoch #") == 2
        lines.append([l for l in out.stdout.splitlines() if l.startswith("<dataset>")])
        saved.append(np.load(str(tmp_path / run / "logs" / "adversarial.npz"), allow_pickle=False))
    assert lines == [[], ["<dataset> 40 images resident on the device (images_u8.cgpack)"]]
    a, b = saved
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_sample_cli_neighbours_with_a_pack_finds_the_same_files(ds, tmp_path):
    data = tmp_path / "data"
    os.makedirs(str(data))
    make_jpgs(str(data), n=40)
    logs = tmp_path / "logs"
    _run([sys.executable, os.path.join(ROOT, "train.py"), "--batchSize", "16", "--N_epoch", "32", "--epochs", "1", "--noplot", "--dataDir", str(data),
          "--save", str(logs), "--saveFreq", "1"], str(tmp_path))
    outs = []
    for run in ("files", "pack"):
        if run == "pack":
            ds.buildPack(str(data), threads=2)
        outs.append(_run([sys.executable, os.path.join(ROOT, "sample.py"), "--save", str(logs), "--dataDir", str(data), "--batchSize", "64",
                          "--neighbours", "--neighbourChunk", "16", "--writeto", str(tmp_path / run)], str(tmp_path)))
    assert "<dataset>" not in outs[0].stdout and "<dataset> 40 images resident on the device (images_u8.cgpack)" in outs[1].stdout
    names = sorted(os.listdir(str(tmp_path / "files")))
    assert "best_0001_neighbours_base.jpg" in names and sorted(os.listdir(str(tmp_path / "pack"))) == names
    for name in names:      # the neighbours' grid holds the files found: byte for byte the same, like every other grid of the run
        assert (tmp_path / "pack" / name).read_bytes() == (tmp_path / "files" / name).read_bytes(), name
