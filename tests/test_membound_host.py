"""Without a GPU: what test_gpu_membound_edges.py rests on.  Every case's regime holds for the caps this library was built with (read
through the ABI; the column reductions' out of common.h), the three restated launch calculations have the properties the kernels
need, and with the chosen seeds the elements whose side of batch-norm + PReLU's kink is the last bit's stay below 0.1 % of a tensor."""
import importlib
import os
import re

import numpy as np
import pytest

import test_gpu_membound_edges as E
from helpers import col_launch, col_tree, ew_grid, fixed_channel_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("cat-generator_amd").lib()


def test_caps_read_through_the_abi_and_the_header(L):
    src = open(os.path.join(ROOT, "cat-generator_amd", "csrc", "common.h")).read()
    k = {n: int(re.search(rf"\b{n} = (\d+)", src).group(1)) for n in ("kNumCU", "kEwWgsPerCU", "kColReduceWgsPerCU")}
    assert E.ew_cap(L) == k["kNumCU"] * k["kEwWgsPerCU"]
    assert E.COL_WGS == k["kNumCU"] * k["kColReduceWgsPerCU"]
    assert E.group_cap(L) >= 1
    cap = E.ew_cap(L)
    for n in (1, 256, 257, cap * 256, cap * 256 + 1, 10 ** 9):
        assert int(L.prelu_backward_workspace_bytes(n)) // 8 == ew_grid(n, cap)


def test_every_case_is_in_the_regime_it_names(L):
    for n, mis, regime in E.ACT_CASES:
        assert E.act_regime(L, n, mis) == regime, (n, mis)
    for G, n, regime in E.GROUPED_PRELU_CASES:
        assert E.grouped_regime(L, n // 4) == regime, (G, n)
    for C, M, run, regime in E.BN_CASES:
        assert E.bn_regime(L, C, M, regime.get("misaligned", False)) == regime, (C, M, E.bn_regime(L, C, M))
    for G, NG, H, W, C, masked, acts, slopes, regime in E.POOL_CASES:
        assert len(slopes) == G and E.pool_regime(L, G, NG, H, W, C) == regime, (G, NG, H, W, C, E.pool_regime(L, G, NG, H, W, C))
    cap = E.ew_cap(L)
    for N, H, W, C, regime in E.PLAIN_POOL_CASES:
        assert (E.ew_regime(N * (H // 2) * (W // 2) * C, cap), E.ew_regime(N * 4 * H * W * C, cap)) == regime, (N, H, W, C)
    for Cs, N, HW, regime in E.CONCAT_CASES:
        assert E.ew_regime(N * HW * sum(Cs) // 4, cap) == regime, (Cs, N, HW)
    for N, HW, C, regime, paths in E.MASK_CASES:
        assert E.ew_regime(N * HW * C // 4, cap) == regime
        assert tuple(E.mask_path(N * HW * C, C, sp, not xa, not ma) for xa, ma, sp in E.MASK_RUNS) == paths
    assert E.ew_regime(E.OPT_N, cap) == "wrap"


def test_the_cases_cover_the_regimes_the_kernels_have():
    R = [(C, M, r) for C, M, _, r in E.BN_CASES]
    for v4 in (False, True):     # every row regime meets a scalar and a vector channel count
        mine = [r for _, _, r in R if r["v4"] == v4]
        assert any(r["chunks"] == 1 for r in mine) and any(1 < r["chunks"] <= 16 for r in mine)
        assert any(r["ngroups"] == 2 and r["last"] == 1 for r in mine), "two ColTree groups, the last of size 1"
        assert any(r["ngroups"] == 16 for r in mine)
    assert any(r["chunks"] == 256 and r["ngroups"] == 16 and r["last"] == 16 for _, _, r in R)
    for C in sorted({C for C, _, _ in R}):     # every channel count meets a sum over more than one group
        assert any(r["ngroups"] > 1 for c, _, r in R if c == C), C
    assert {C for C, _, r in R if "second_block" in r} == {70, 72, 136}
    assert any(r.get("below_row_lanes") for _, _, r in R) and any(M % 4 for _, M, _ in R) and any(r.get("trips") == 2 for _, _, r in R)
    applies = {r.get("apply") for _, _, r in R}
    assert {"wrap, C4 = 3 does not divide 256", "wrap, C4 = 18 does not divide 256", "wrap"} <= applies
    assert {G for G, *_ in E.POOL_CASES} == {1, 2, 4} and {G for G, _, _ in E.GROUPED_PRELU_CASES} == {1, 2, 4}


def test_restated_launch_arithmetic_keeps_what_the_kernels_need():
    for C4 in (1, 3, 18, 32, 34, 100):
        for n4 in (1, 255, 257, 5000, 262144, 262145, 10 ** 7):
            g = fixed_channel_grid(n4, C4, 1024)
            assert 1 <= g <= max(1024, C4) and (g * 256) % C4 == 0
    for C, v4 in ((3, False), (70, False), (4, True), (72, True), (128, True), (136, True)):
        for M in (1, 5, 64, 65, 1027, 16384, 16400, 131592):
            cl = col_launch(M, C, v4, 256)
            assert cl["rows"] % 4 == 0 and (cl["chunks"] - 1) * cl["rows"] < M <= cl["chunks"] * cl["rows"]
            assert cl["chunks"] * cl["cblocks"] <= 256
            t = col_tree(cl["chunks"])
            assert t["ngroups"] <= 32 and (t["ngroups"] - 1) * t["G"] + t["last"] == cl["chunks"] and 1 <= t["last"] <= t["G"]


def test_kink_band_stays_below_a_thousandth_with_the_chosen_seeds():
    """The elements of u = xhat gamma + beta within 4 roundings of zero (where the device's side of PReLU's kink may differ from fp64's and
    is taken over): with these seeds none in the small cases, a handful per million in the large ones."""
    for C, M, run, _ in E.BN_CASES:
        _, x, _, gamma, beta = E.bn_inputs(C, M)
        x64 = x.astype(np.float64)
        S = E.stat_bounds(x64, M, float(np.float32(1e-5)))
        _, u, near = E.bn_near_kink(x, S["mean"].astype(np.float32), S["inv"].astype(np.float32), gamma, beta)
        assert near.sum() <= 1e-3 * u.size, (C, M, int(near.sum()), u.size)
        assert near.sum() <= max(0, 20e-6 * u.size)
