"""CPU checks of the device nearest-neighbour search (sample.lua:131-151, cg_nearest_update): the two C entry points and their
argument checks, nn_utils.nearest_d2_np - the numpy restatement of the kernel's fp32 summation order - against the fp64 sum of squares,
and the merge rule's independence of the chunk order."""
import ctypes
import importlib

import numpy as np
import pytest


@pytest.fixture(scope="module")
def cg():
    return importlib.import_module("cat-generator_amd")


@pytest.fixture(scope="module")
def U():
    return importlib.import_module("cat-generator_amd.nn_utils")


def test_exports_and_argument_checks(cg):
    abi = importlib.import_module("cat-generator_amd._abi")
    protos = abi.parse_header()
    dll = ctypes.CDLL(abi.LIB_PATH)
    for name in ("cg_nearest_workspace_bytes", "cg_nearest_update"):
        assert name in protos and hasattr(dll, name)
    L = cg.lib()
    assert L.nearest_workspace_bytes(4096, 64, 3072) > 0
    p = 4096      # a non-null address that is never touched: every case below fails its check before anything is launched
    cases = [("outside 1..64", (None, p, 8, 16, p, 0, 0, 1, p, p, p)), ("outside 1..64", (None, p, 8, 16, p, 65, 0, 1, p, p, p)),
             ("bad geometry", (None, p, 8, 0, p, 4, 0, 1, p, p, p)), ("null pointer", (None, p, 8, 16, p, 4, 0, 1, None, p, p)),
             ("does not fit int32", (None, p, 8, 16, p, 4, -1, 1, p, p, p)), ("bad geometry", (None, p, -1, 16, p, 4, 0, 1, p, p, p)),
             ("does not fit int32", (None, p, 8, 16, p, 4, 2 ** 31 - 4, 1, p, p, p)), ("null pointer", (None, None, 8, 16, p, 4, 0, 1, p, p, p))]
    for message, args in cases:      # (stream, pool, N, D, queries, Q, index0, reset, best_d2, best_idx, workspace)
        with pytest.raises(cg.CatganError, match="cg_nearest_update: .*" + message):
            L.nearest_update(*args)


@pytest.mark.parametrize("D", [1, 105, 1024, 3072])
def test_restatement_stays_within_the_bound_of_its_summation_order(U, D):
    """The order is documented in include/catgan.h: partials of NEAREST_PER_LANE sequential additions, a tree of NEAREST_TREE levels, one
    addition per tile.  Every term is a non-negative square (one rounding), so the relative error of the sum against the exact sum of the
    same fp32 differences is at most (1 + u)^(k + 1) - 1 <= (k + 3) u with u = 2^-24 and k the longest chain - a bound, no measurement."""
    k = U.NEAREST_PER_LANE + U.NEAREST_TREE + -(-D // U.NEAREST_TILE)
    assert k == U.nearest_chain_length(D) and U.NEAREST_TILE == U.NEAREST_LANES * U.NEAREST_PER_LANE == 512
    rs = np.random.RandomState(D)
    pool, queries = rs.rand(200, D).astype(np.float32), rs.rand(5, D).astype(np.float32)
    pool[17] = queries[2]
    pool[44] = queries[0]
    got = U.nearest_d2_np(pool, queries)
    assert got.shape == (5, 200) and got.dtype == np.float32
    diff = (pool[None, :, :] - queries[:, None, :]).astype(np.float64)      # the fp32 differences, exactly
    want = (diff * diff).sum(axis=2)
    assert got[2, 17] == 0.0 and got[0, 44] == 0.0                          # exactly 0 for identical rows
    nz = want > 0
    rel = np.abs(got.astype(np.float64)[nz] - want[nz]) / want[nz]
    print(f"D={D} k={k} max relative error {rel.max():.3e} bound {(k + 3) * 2.0 ** -24:.3e}")
    assert rel.max() <= (k + 3) * 2.0 ** -24
    assert np.array_equal(got[~nz], np.zeros((~nz).sum(), np.float32))


def test_merge_rule_keeps_the_lower_index_in_any_chunk_order(U):
    rs = np.random.RandomState(3)
    d2 = rs.rand(4, 90).astype(np.float32) + np.float32(1)
    d2[0, [11, 40, 77]] = 0.25          # three equal minima in three chunks
    d2[1, [85, 2]] = 0.0
    d2[2, 89] = 0.5
    bounds = [(0, 30), (30, 60), (60, 90)]
    want_idx = np.array([11, 2, 89, int(np.argmin(d2[3]))], np.int32)
    import itertools
    for order in itertools.permutations(bounds):
        bd, bi = U.nearest_reset_np(4)
        assert np.isinf(bd).all() and (bi == -1).all()
        for a, b in order:
            bd, bi = U.nearest_merge_np(bd, bi, d2[:, a:b], a)
        np.testing.assert_array_equal(bi, want_idx)
        np.testing.assert_array_equal(bd, d2[np.arange(4), want_idx])
        bd2, bi2 = U.nearest_merge_np(bd, bi, d2[:, 0:0], 0)               # an empty chunk changes nothing
        assert np.array_equal(bd2, bd) and np.array_equal(bi2, bi)
    bd, bi = U.nearest_merge_np(*U.nearest_reset_np(4), d2, 1000)          # index0 is added
    np.testing.assert_array_equal(bi, want_idx + 1000)
