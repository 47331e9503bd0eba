"""The nearest-neighbour search on the MI355X: cg_nearest_update bit-equal to nn_utils.nearest_d2_np + nearest_merge_np (whose own
yardstick is in tests/test_nearest_host.py) over the listed shapes, independent of the chunking, with the tie and zero rules; against the
reference's rule in fp64; the NCHW -> NHWC permutation of NearestSearch; dataset.SequentialLoader against the blocking loader;
sample.py --neighbours against --neighboursHost."""
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
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def cg():
    assert torch.cuda.is_available()
    return importlib.import_module("cat-generator_amd")


@pytest.fixture(scope="module")
def U(cg):
    return cg.nn_utils


@pytest.fixture()
def ds():
    d = importlib.import_module("cat-generator_amd.dataset")
    yield d
    d.colorSpace = "rgb"
    d.setHeight(32); d.setWidth(32)
    d.seed(1)


def _search(cg, U, pool, queries, chunks=None):
    """The device result (best_d2, best_idx) for pool [N, D] and queries [Q, D]; chunks = [(first row, rows)] in the order they are fed."""
    N = pool.shape[0]
    dev = cg.Tensor.from_numpy(pool) if N else None
    s = U.NearestSearch(queries)
    for a, n in ([(0, N)] if chunks is None else chunks):
        if n:
            s.update(dev.rows(a + 1, a + n), a)
    s.result()
    return s.best_d2.cpu().numpy(), s.best_idx.cpu().numpy(), s


def _restated(U, pool, queries):
    return U.nearest_merge_np(*U.nearest_reset_np(queries.shape[0]), U.nearest_d2_np(pool, queries), 0)


def _same_bits(got_d, got_i, want_d, want_i, msg=""):
    np.testing.assert_array_equal(got_i, want_i, err_msg=msg)
    np.testing.assert_array_equal(got_d.view(np.uint32), want_d.view(np.uint32), err_msg=msg)


# every listed D, N and Q appears; N = 4099 takes more than one workgroup's rows, 257 and 63 leave workgroups and waves half empty
SHAPES = [(1, 1, 1), (1, 4099, 64), (105, 63, 3), (105, 257, 16), (105, 4099, 64), (1024, 1, 3), (1024, 63, 64), (1024, 257, 16),
          (3072, 1, 1), (3072, 63, 16), (3072, 257, 64), (3072, 4099, 1)]


@pytest.mark.parametrize("D,N,Q", SHAPES)
def test_kernel_equals_the_restatement_bit_for_bit(cg, U, D, N, Q):
    rs = np.random.RandomState(D + 7 * N + 31 * Q)
    pool, queries = rs.rand(N, D).astype(np.float32), rs.rand(Q, D).astype(np.float32)
    got_d, got_i, _ = _search(cg, U, pool, queries)
    _same_bits(got_d, got_i, *_restated(U, pool, queries), msg=f"D={D} N={N} Q={Q}")


# The launch geometry (speed only): 16 rows per workgroup below 16 384 rows, 32 below 32 768, 64 from there on - two, four passes of a
# wave over its row pairs - and from 1025 row blocks on (N > 65 536) the workgroups walk several row blocks and carry their best along.
# Each case plants one row at several indices: in different row blocks, in the first and the last pass of a wave inside one block, and
# (last case) in two row blocks of the SAME workgroup (blocks 0 and 1024, 1 and 1025), so the lowest index has to win at every level.
GEOMETRIES = [(16384 + 37, 105, 3, [(0, (16000, 41, 9000)), (1, (16420, 16389))]),                      # 32 rows per workgroup
              (32768 + 70, 105, 4, [(0, (32800, 63, 20001)), (1, (32837, 32770)), (3, (127, 64))]),     # 64 rows per workgroup
              (65536 + 200, 1, 2, [(0, (65540, 9)), (1, (65735, 65600, 70))]),                          # ... walked grid-stride
              (65536 + 200, 105, 5, [(0, (65540, 9)), (1, (65700, 65601)), (4, (65735,))])]


@pytest.mark.parametrize("N,D,Q,plant", GEOMETRIES)
def test_every_launch_geometry_equals_the_restatement(cg, U, N, D, Q, plant):
    rs = np.random.RandomState(N + D)
    pool, queries = rs.rand(N, D).astype(np.float32), rs.rand(Q, D).astype(np.float32)
    for q, rows in plant:
        pool[list(rows)] = queries[q]
    got_d, got_i, _ = _search(cg, U, pool, queries)
    want_d, want_i = _restated(U, pool, queries)
    for q, rows in plant:
        assert want_i[q] == min(rows) and want_d[q] == 0.0      # the restatement's own tie rule, before the device is held to it
    _same_bits(got_d, got_i, want_d, want_i, msg=f"N={N} D={D} Q={Q}")
    # the same pool in two chunks that cut a row block, at an index0 of their own, fed last chunk first
    cut = N // 2 + 5
    d, i, _ = _search(cg, U, pool, queries, [(cut, N - cut), (0, cut)])
    _same_bits(d, i, want_d, want_i, msg=f"N={N} D={D} Q={Q}, two chunks")


@pytest.fixture(scope="module")
def planted():
    """N = 1000, D = 105, Q = 16: one training row at 5, 300 and 999 (three workgroup tiles, three chunks of 256); query 0 is that row,
    query 1 is at distance 0 from nothing."""
    rs = np.random.RandomState(11)
    pool, queries = rs.rand(1000, 105).astype(np.float32), rs.rand(16, 105).astype(np.float32)
    pool[300] = pool[999] = pool[5]
    queries[0] = pool[5]
    return pool, queries


def _chunks(N, size):
    return [(a, min(size, N - a)) for a in range(0, N, size)]


def test_chunking_and_chunk_order_do_not_show(cg, U, planted):
    pool, queries = planted
    one_d, one_i, _ = _search(cg, U, pool, queries)
    _same_bits(one_d, one_i, *_restated(U, pool, queries))
    for size in (1, 7, 256):
        for chunks in (_chunks(1000, size), _chunks(1000, size)[::-1]):
            d, i, _ = _search(cg, U, pool, queries, chunks)
            _same_bits(d, i, one_d, one_i, msg=f"chunks of {size}, first chunk {chunks[0]}")
    # reset = 1 forgets an earlier sequence: first a pool that holds every query itself (d2 = 0 everywhere), then the real one
    s = U.NearestSearch(queries)
    s.update(cg.Tensor.from_numpy(queries), 0)
    idx, dist = s.result()
    assert (idx == np.arange(16)).all() and (dist == 0).all()
    s.reset()
    dev = cg.Tensor.from_numpy(pool)
    for a, n in _chunks(1000, 256):
        s.update(dev.rows(a + 1, a + n), a)
    s.result()
    _same_bits(s.best_d2.cpu().numpy(), s.best_idx.cpu().numpy(), one_d, one_i)


def test_ties_and_zeros(cg, U, planted):
    pool, queries = planted
    want_d, want_i = _restated(U, pool, queries)
    for chunks in (None, _chunks(1000, 256), _chunks(1000, 256)[::-1]):
        d, i, _ = _search(cg, U, pool, queries, chunks)
        assert i[0] == 5 and d[0] == 0.0 and not np.signbit(d[0])
        assert i[1] == want_i[1] and d[1] == want_d[1] and d[1] > 0
    s = U.NearestSearch(queries)      # N = 0 with reset leaves (+inf, -1)
    idx, dist = s.result()
    assert (idx == -1).all() and np.isposinf(dist).all() and np.isposinf(s.best_d2.cpu().numpy()).all()


def test_device_index_is_the_fp64_argmin(cg, U):
    rs = np.random.RandomState(5)
    N, D, Q = 1000, 3072, 16
    pool, queries = rs.rand(N, D).astype(np.float32), rs.rand(Q, D).astype(np.float32)
    p64 = pool.astype(np.float64)
    d64 = np.stack([((p64 - q.astype(np.float64)) ** 2).sum(axis=1) for q in queries])
    order = np.argsort(d64, axis=1)
    best, second = d64[np.arange(Q), order[:, 0]], d64[np.arange(Q), order[:, 1]]
    k = U.NEAREST_PER_LANE + U.NEAREST_TREE + -(-D // U.NEAREST_TILE)
    gap = (second - best) / best
    print(f"fp64 gaps {gap.min():.3e} .. {gap.max():.3e}, needed {2 * (k + 3) * U24:.3e}")
    assert (gap > 2 * (k + 3) * U24).all()      # a condition on the inputs: no query is excused
    s = U.NearestSearch(queries).update(cg.Tensor.from_numpy(pool), 0)
    idx, dist = s.result()
    np.testing.assert_array_equal(idx, order[:, 0].astype(np.int32))
    want = np.sqrt(best).astype(np.float32)
    ulp = np.abs(dist.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    print(f"distance against float32(sqrt(fp64 d2)): {ulp.max()} ulp")
    assert ulp.max() <= 2


def test_queries_are_permuted_to_the_pool_layout(cg, U):
    rs = np.random.RandomState(2)
    train = rs.rand(40, 3, 5, 7).astype(np.float32)        # NCHW on the host, NHWC in the engine
    picks = [33, 0, 17, 39]
    s = U.NearestSearch(train[picks]).update(cg.Tensor.from_numpy(train), 0)
    idx, dist = s.result()
    np.testing.assert_array_equal(idx, picks)
    assert (dist == 0).all()


@pytest.mark.parametrize("cs", ["rgb", "y"])
def test_sequential_loader_and_the_device_search_over_it(cg, U, ds, tmp_path, cs):
    make_jpgs(str(tmp_path), 23, odd=13)
    ds.setDirs([str(tmp_path)]); ds.setFileExtension("jpg"); ds.setHeight(32); ds.setWidth(32)
    ds.colorSpace = cs
    ds.seed(5)
    files = ds.pickFiles(10 ** 9)
    ds.seed(5)
    ref = ds.loadRandomImages(10 ** 9).scaled
    state = ds._rs.get_state()[1].copy()
    ld = ds.SequentialLoader(files, 8)
    try:
        got, where = [], []
        for pool, index0, n in ld:
            got.append(cg.nn.as_nhwc(pool).numpy())
            where.append((index0, n))
        assert where == [(0, 8), (8, 8), (16, 7)] and ld.next() is None
        np.testing.assert_array_equal(np.concatenate(got), ref)
    finally:
        ld.close()
    np.testing.assert_array_equal(ds._rs.get_state()[1], state)      # the generator is not touched
    queries = ref[[3, 13, 22]] + np.float32(1e-3)
    host = U.findClosestNeighboursOf(queries, ref)
    ld = ds.SequentialLoader(files, 8)
    try:
        pairs, idx = U.findClosestNeighboursOnDevice(queries, ld)
    finally:
        ld.close()
    np.testing.assert_array_equal(idx, [3, 13, 22])
    for (img, nb, dist), (himg, hnb, hdist) in zip(pairs, host):
        np.testing.assert_array_equal(img, himg)
        np.testing.assert_array_equal(nb, hnb)
        assert abs(dist - hdist) <= 1e-6 * hdist


def test_sample_cli_neighbours_on_the_device_write_the_host_path_files(tmp_path):
    """train.py for one epoch, then sample.py --neighbours --runs 2 on the device and on the host: every file of both runs byte for byte
    the same (the generator draws of later runs are preserved), and --neighboursOf 64 writes 64 pairs."""
    from PIL import Image
    make_jpgs(str(tmp_path), 40)
    logs = tmp_path / "logs"
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--batchSize", "16", "--N_epoch", "32", "--epochs", "1", "--noplot",
           "--dataDir", str(tmp_path), "--save", str(logs), "--saveFreq", "1"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    base = [sys.executable, os.path.join(ROOT, "sample.py"), "--save", str(logs), "--dataDir", str(tmp_path), "--batchSize", "64"]
    for dst, extra in (("dev", ["--neighbours", "--runs", "2", "--neighbourChunk", "16"]), ("host", ["--neighboursHost", "--neighbours", "--runs", "2"]),
                       ("k64", ["--neighbours", "--neighboursOf", "64", "--nSamples", "128"])):
        out = subprocess.run(base + ["--writeto", str(tmp_path / dst)] + extra, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
    names = sorted(os.listdir(str(tmp_path / "host")))
    assert len(names) == 14 and "best_0002_neighbours_base.jpg" in names and "trainset_s1_0002_base.jpg" in names
    assert sorted(os.listdir(str(tmp_path / "dev"))) == names
    for name in names:
        assert (tmp_path / "dev" / name).read_bytes() == (tmp_path / "host" / name).read_bytes(), name
    assert np.asarray(Image.open(str(tmp_path / "host" / "best_0001_neighbours_base.jpg"))).shape == (2 * 32, 16 * 32, 3)
    assert np.asarray(Image.open(str(tmp_path / "k64" / "best_0001_neighbours_base.jpg"))).shape == (2 * 32, 64 * 32, 3)
