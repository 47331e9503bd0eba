"""The memory-bound kernels of csrc/ops.hip (with csrc/optim.hip's Adam) and csrc/fused.hip over their dispatch edges, through the C ABI, against fp64 numpy on the
same fp32 inputs: scalar twins (n % 4, C % 4, a pointer off its 16-byte boundary), the grid-stride wrap behind cg::ew_grid's cap with
channel counts that do not divide 256, every regime of the column reductions' chunk / ColTree arithmetic, stacked groups, and the value
edges the oracle defines (+-0.0 at the kink, ties in the max pool).

Every case states the regime it is meant to hit and asserts it from the caps read through the ABI and three launch calculations
restated in helpers.py (test_membound_host.py runs the same assertions without a GPU).  Two measures only, both per element (per column
for a reduction), none scaled by a tensor's maximum:
  bits_equal      where the kernel's expression has no multiply feeding an add (nothing for the compiler to contract)
  rounding_close  |d| <= r 2^-24 sum|terms|, r = the fp32 roundings on the longest chain of the kernel's expression + 2, written next
                  to each use with the line of the kernel it was counted from
Batch norm is checked in two steps: the statistics against fp64 statistics (bound propagated through var = E[x^2] - mean^2), then y
and dx against fp64 evaluated WITH the device's save_mean / save_invstd.  Inputs are well conditioned (|mean| <= std per channel)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from helpers import (U24, bits_equal, col_launch, col_tree, dev, duplicate_in_windows, edge_normal, fixed_channel_grid, host, out_like,
                     rounding_close)
from oracle import oracle as O

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
COL_WGS = 256             # common.h kNumCU * kColReduceWgsPerCU (test_membound_host.py reads both constants out of the header)


@pytest.fixture(scope="module")
def cg():
    mod = importlib.import_module("cat-generator_amd")
    assert torch.cuda.is_available(), "these tests need the MI355X"
    mod.lib()  # fails loudly if the HIP extension is missing
    return mod


# ------------------------------------------------------------------------------ caps and regimes
def ew_cap(L):
    """cg::ew_grid's cap: cg_prelu_backward_workspace_bytes(n) / 8 is ew_grid(n), which a huge n drives into the cap."""
    return int(L.prelu_backward_workspace_bytes(1 << 40)) // 8


def group_cap(L):
    """act_pool_bwd_blocks' cap (fused.hip): workgroups per group of the stacked-group backward kernels."""
    return int(L.act_pool2_mask_backward_workspace_bytes(1, 1 << 20, 64, 64, 64)) // 8


def ew_regime(n, cap):
    """'one' workgroup, 'many' without a wrap, or 'wrap': lanes past cap * 256 make a thread take a second element."""
    return "wrap" if n > cap * 256 else ("many" if n > 256 else "one")


# n, misaligned, the regime: (vector?, ew_regime of the launched lanes)
ACT_CASES = [
    (1, False, (False, "one")), (3, False, (False, "one")), (255, False, (False, "one")), (257, False, (False, "many")),
    (256, False, (True, "one")), (256, True, (False, "one")),                    # the same multiple of 4 through a pointer 4 bytes off
    (262144 + 5, False, (False, "wrap")),                                        # the scalar kernel wraps
    (4 * 262144 + 4, False, (True, "wrap")),                                     # the vector kernel wraps, one float4 in the last pass
    (4 * 262144 + 4, True, (False, "wrap")),
]


def act_regime(L, n, misaligned):
    v4 = n % 4 == 0 and not misaligned                                           # cg::vec_ok in cg_prelu_* / cg_leakyrelu_*
    return v4, ew_regime(n // 4 if v4 else n, ew_cap(L))


# G, n per group, regime: workgroups per group (None = the cap) and whether a group wraps
GROUPED_PRELU_CASES = [(1, 4, (1, False)), (2, 1028, (2, False)), (4, 2052, (3, False)), (2, 4 * 262144 + 8, (None, True))]


def grouped_regime(L, n_per_group4):
    cap = group_cap(L)
    blocks = max(1, min((n_per_group4 + 255) // 256, cap))                       # act_pool_bwd_blocks
    return (None if blocks == cap else blocks), n_per_group4 > blocks * 256


# C, M, what is run, the regime.  v4: the float4 kernels; chunks / ngroups / last: the ColTree; second_block: live channels of the last
# channel block where there are two; trips: of the rb loop (colreduce4_k, bn_act_bwd_stats_k); apply: the bn_act apply kernels' regime.
BN_CASES = [
    (3, 1, "all", dict(v4=False, chunks=1, ngroups=1, last=1)),
    (3, 5, "all", dict(v4=False, chunks=1, ngroups=1, last=1)),
    (3, 64, "all", dict(v4=False, chunks=1, ngroups=1, last=1)),
    (3, 65, "all", dict(v4=False, chunks=2, ngroups=1, last=2)),
    (3, 1027, "all", dict(v4=False, chunks=17, ngroups=2, last=1)),
    (3, 16384, "all", dict(v4=False, chunks=256, ngroups=16, last=16)),
    (3, 16400, "all", dict(v4=False, chunks=242, ngroups=16, last=2)),           # 257 chunks wanted; the cap, then rows % 4 == 0, leave 242
    (70, 5, "all", dict(v4=False, chunks=1, ngroups=1, last=1, second_block=6)),
    (70, 1027, "all", dict(v4=False, chunks=17, ngroups=2, last=1, second_block=6)),
    (4, 1, "all", dict(v4=True, chunks=1, ngroups=1, last=1, below_row_lanes=True)),
    (4, 5, "all", dict(v4=True, chunks=1, ngroups=1, last=1, below_row_lanes=True)),
    (4, 64, "all", dict(v4=True, chunks=1, ngroups=1, last=1)),
    (4, 65, "all", dict(v4=True, chunks=2, ngroups=1, last=2)),
    (4, 1027, "all", dict(v4=True, chunks=17, ngroups=2, last=1)),
    (4, 16384, "all", dict(v4=True, chunks=256, ngroups=16, last=16)),           # exactly 256 chunks: 16 full groups
    (4, 16400, "all", dict(v4=True, chunks=242, ngroups=16, last=2)),
    (12, 1027, "all", dict(v4=True, chunks=17, ngroups=2, last=1, apply="wrap, C4 = 3 does not divide 256")),   # 12 workgroups for 13
    # C % 4 == 0 through tensors 4 bytes off their boundary: the scalar kernels and the separate passes inside cg_bn_act_forward
    (12, 1027, "all", dict(v4=False, misaligned=True, chunks=17, ngroups=2, last=1)),
    (12, 87400, "all", dict(v4=True, chunks=255, ngroups=16, last=15, apply="wrap, C4 = 3 does not divide 256")),   # past the cap
    (72, 5, "all", dict(v4=True, chunks=1, ngroups=1, last=1, second_block=8, below_row_lanes=True, apply="many, C4 = 18 does not divide 256")),
    (72, 1027, "all", dict(v4=True, chunks=17, ngroups=2, last=1, second_block=8, apply="wrap, C4 = 18 does not divide 256")),
    (72, 16400, "all", dict(v4=True, chunks=125, ngroups=8, last=13, second_block=8, apply="wrap, C4 = 18 does not divide 256")),
    (136, 5, "all", dict(v4=True, chunks=1, ngroups=1, last=1, second_block=8, below_row_lanes=True, apply="many, C4 = 34 does not divide 256")),
    (136, 1027, "all", dict(v4=True, chunks=17, ngroups=2, last=1, second_block=8, apply="wrap, C4 = 34 does not divide 256")),
    # two trips of the rb loop (516 rows per chunk > 64 * RL = 512), UB batches and a ragged tail; 16.8 M elements: the column sums of
    # cg_bn_stats and of cg_bn_act_backward_stats (with the slope) only
    (128, 131072 + 520, "sums", dict(v4=True, chunks=256, ngroups=16, last=16, trips=2, apply="wrap")),
]


def bn_regime(L, C, M, misaligned=False):
    v4 = C % 4 == 0 and not misaligned                                           # cg::vec_ok in colreduce_launch, cg_bn_*
    cl = col_launch(M, C, v4, COL_WGS)
    tr = col_tree(cl["chunks"])
    got = dict(v4=v4, chunks=cl["chunks"], ngroups=tr["ngroups"], last=tr["last"])
    if misaligned:
        got["misaligned"] = True
    if cl["cblocks"] > 1:
        assert cl["cblocks"] == 2
        got["second_block"] = C - (cl["qb"] * 4 if v4 else 64)
    if v4 and M < cl["RL"]:
        got["below_row_lanes"] = True
    trips = -(-cl["rows"] // (64 * cl["RL"]))
    if trips > 1:
        got["trips"] = trips
    if v4 and C > 8:                                                             # the apply kernels of bn_act (cg_bn_act_forward / _backward)
        cap, n4, C4 = ew_cap(L), M * (C // 4), C // 4
        grid = fixed_channel_grid(n4, C4, cap)
        assert (grid * 256) % C4 == 0, "the stride must keep a thread on one channel quad"
        got["apply"] = ("wrap" if n4 > grid * 256 else "many") + (f", C4 = {C4} does not divide 256" if 256 % C4 else "")
    return got


# G, NG, H, W, C, mask ("none" / "zero rows"), the acts to run, slopes, regime: (forward, backward) wrap
POOL_CASES = [
    (1, 2, 6, 10, 4, "none", (0, 1, 2), (0.25,), ("one", "one")),
    (2, 2, 6, 10, 120, "zero rows", (0, 1, 2), (0.25, -0.1), ("many", "many")),
    (4, 1, 6, 10, 4, "zero rows", (0, 1, 2), (0.25, -0.1, 0.6, 1.5), ("one", "one")),
    (2, 2, 6, 10, 120, "none", (1,), (0.0, -0.5), ("many", "many")),              # ties: slope 0 makes every all-negative window tie
    (2, 10, 60, 60, 120, "zero rows", (1,), (0.25, -0.1), ("wrap", "wrap")),      # a wrap inside a group
]


def pool_regime(L, G, NG, H, W, C):
    per_group4 = NG * (H // 2) * (W // 2) * (C // 4)
    blocks = int(L.act_pool2_mask_backward_workspace_bytes(G, NG, H, W, C)) // 8 // G
    bwd = "wrap" if per_group4 > blocks * 256 else ("many" if blocks > 1 else "one")
    return ew_regime(G * per_group4, ew_cap(L)), bwd


# N, H, W, C and the regime of the pooled / the upsampled launch
PLAIN_POOL_CASES = [(2, 6, 10, 1, ("one", "many")), (3, 4, 6, 3, ("one", "many")), (2, 6, 10, 10, ("many", "many")),
                    (16, 64, 112, 10, ("wrap", "wrap"))]
# widths of the branches, N, HW, regime
CONCAT_CASES = [((4,), 3, 5, "one"), ((4, 12), 3, 5, "one"), ((4, 12, 8), 3, 5, "one"), ((4, 12, 8, 40), 3, 50, "many"),
                ((4, 12, 8, 40), 3, 5500, "wrap")]
HEAD_O, HEAD_N, HEAD_F = (1, 2, 3, 4), (1, 3, 4, 5), (1, 63, 64, 65, 256)
OPT_N = 262144 + 3


def bn_inputs(C, M):
    rng = np.random.default_rng(1000 * C + M % 997)
    x = edge_normal(rng, (M, C))
    dy = edge_normal(rng, (M, C))
    gamma = rng.uniform(0.2, 1.0, C).astype(f32) * np.where(rng.random(C) < 0.25, -1, 1).astype(f32)
    beta = (rng.standard_normal(C) * 0.3).astype(f32)
    return rng, x, dy, gamma, beta


def bn_near_kink(x, mean, invstd, gamma, beta):
    """fp64 u = xhat gamma + beta from fp32 statistics, and where it lies within 4 roundings of zero (the side of the kink is then the
    device's last bit's, not the operation's: bn_act_fwd_v4k / bn_act_bwd_*_k recompute u in fp32 and branch on u > 0)."""
    xh = (x.astype(f64) - mean.astype(f64)) * invstd.astype(f64)
    t = xh * gamma.astype(f64)
    u = t + beta.astype(f64)
    return xh, u, np.abs(u) <= 4 * U24 * (np.abs(t) + np.abs(beta.astype(f64)))


# ------------------------------------------------------------------------------ device plumbing
def ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def scalar(v):
    return dev(np.array([v], f32))


def nchw(a):
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2))


def nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


# ------------------------------------------------------------------------------ activations
@pytest.mark.parametrize("n,misaligned,regime", ACT_CASES)
def test_activation_twins_and_wraps(cg, n, misaligned, regime):
    L, st = cg.lib(), cg.tensor.stream()
    assert act_regime(L, n, misaligned) == regime
    rng = np.random.default_rng(n + misaligned)
    x, dy = edge_normal(rng, (n, 1)).ravel(), edge_normal(rng, (n, 1)).ravel()
    a, s = f32(0.25), f32(0.333)
    xt, dyt, al = dev(x, misaligned), dev(dy, misaligned), scalar(a)
    pos, nonneg = x > 0, x >= 0                                                   # -0.0, +0.0: PReLU's negative side, LeakyReLU's positive
    y = out_like(n, misaligned)
    L.prelu_forward(st, xt.data_ptr(), al.data_ptr(), y.data_ptr(), n)
    bits_equal(host(y), np.where(pos, x, a * x), "prelu forward")
    assert np.array_equal(host(y), O.PReLU().forward(x))
    dx, ga = out_like(n, misaligned), scalar(1.0)                                 # accumulate semantics: galpha starts at 1
    wsb = int(L.prelu_backward_workspace_bytes(n))
    ws = torch.zeros(wsb // 8, dtype=torch.float64, device="cuda")
    L.prelu_backward(st, xt.data_ptr(), dyt.data_ptr(), al.data_ptr(), dx.data_ptr(), ga.data_ptr(), 0.5, n, ws.data_ptr(), wsb)
    dx_ref = np.where(pos, dy, a * dy)
    bits_equal(host(dx), dx_ref, "prelu dx")
    prod = (x.astype(f64) * dy.astype(f64))[~pos]
    # prelu_bwd_k<4> (cg::slope_acc): a product, the 3 sums beside it, one sum into s per pass and two passes at most; the cast and the +=
    # of prelu_galpha_reduce_k: 1 + 3 + 2 + 2, + 2
    assert n <= 2 * 4 * ew_cap(L) * 256
    rounding_close(host(ga), [1.0 + 0.5 * prod.sum()], [1.0 + 0.5 * np.abs(prod).sum()], 10, "prelu galpha")
    dx2 = out_like(n, misaligned)
    L.prelu_backward(st, xt.data_ptr(), dyt.data_ptr(), al.data_ptr(), dx2.data_ptr(), None, 0.0, n, None, 0)   # updateGradInput only
    bits_equal(host(dx2), dx_ref, "prelu dx without galpha")
    y2, dx3 = out_like(n, misaligned), out_like(n, misaligned)
    L.leakyrelu_forward(st, xt.data_ptr(), y2.data_ptr(), float(s), n)
    L.leakyrelu_backward(st, xt.data_ptr(), dyt.data_ptr(), dx3.data_ptr(), float(s), n)
    bits_equal(host(y2), np.where(nonneg, x, s * x), "leakyrelu forward")
    bits_equal(host(dx3), np.where(nonneg, dy, s * dy), "leakyrelu dx")
    Ol = O.LeakyReLU(0.333)
    assert np.array_equal(host(y2), Ol.forward(x)) and np.array_equal(host(dx3), Ol.backward(dy))
    if misaligned:                                                                # the scalar twin against the vector kernel, same data
        assert act_regime(L, n, False)[0], "the aligned run of this length takes the vector kernels"
        xa, dya, ya, dxa, ya2, dxa2 = dev(x), dev(dy), out_like(n), out_like(n), out_like(n), out_like(n)
        L.prelu_forward(st, xa.data_ptr(), al.data_ptr(), ya.data_ptr(), n)
        L.prelu_backward(st, xa.data_ptr(), dya.data_ptr(), al.data_ptr(), dxa.data_ptr(), None, 0.0, n, None, 0)
        L.leakyrelu_forward(st, xa.data_ptr(), ya2.data_ptr(), float(s), n)
        L.leakyrelu_backward(st, xa.data_ptr(), dya.data_ptr(), dxa2.data_ptr(), float(s), n)
        for got, twin, what in ((y, ya, "prelu"), (dx2, dxa, "prelu dx"), (y2, ya2, "leakyrelu"), (dx3, dxa2, "leakyrelu dx")):
            bits_equal(host(got), host(twin), what + ": scalar twin against the vector kernel")


@pytest.mark.parametrize("G,n,regime", GROUPED_PRELU_CASES)
def test_prelu_backward_over_stacked_groups(cg, G, n, regime):
    L, st = cg.lib(), cg.tensor.stream()
    assert grouped_regime(L, n // 4) == regime
    assert int(L.prelu_backward_grouped_workspace_bytes(G, n)) // 8 // G == (regime[0] or group_cap(L))
    rng = np.random.default_rng(G * 7 + n)
    x, dy = edge_normal(rng, (G * n, 1)).reshape(G, n), edge_normal(rng, (G * n, 1)).reshape(G, n)
    slopes = [f32(v) for v in (0.25, -0.1, 0.0, 1.5)[:G]]
    xt, dyt, dx = dev(x), dev(dy), out_like(G * n)
    al, ga = [scalar(v) for v in slopes], [scalar(1.0) for _ in slopes]
    wsb = int(L.prelu_backward_grouped_workspace_bytes(G, n))
    ws = torch.zeros(wsb // 8, dtype=torch.float64, device="cuda")
    L.prelu_backward_grouped(st, xt.data_ptr(), dyt.data_ptr(), ptrs(al), dx.data_ptr(), ptrs(ga), 0.5, G, n, ws.data_ptr(), wsb)
    got = host(dx, (G, n))
    for g in range(G):
        pos = x[g] > 0
        bits_equal(got[g], np.where(pos, dy[g], slopes[g] * dy[g]), f"group {g} dx")
        prod = (x[g].astype(f64) * dy[g].astype(f64))[~pos]
        # prelu_bwd_groups_v4k adds as prelu_bwd_k<4> does (both are cg::prelu_bwd_walk<4>): 6; galpha_groups_reduce_k: cast, product, sum
        rounding_close(host(ga[g]), [1.0 + 0.5 * prod.sum()], [1.0 + 0.5 * np.abs(prod).sum()], 11, f"group {g} galpha")


# ------------------------------------------------------------------------------ column reductions and the batch-norm family
def stat_bounds(x64, M, eps):
    """fp64 statistics of the columns of x and how far the device's may lie from them: its sums are 66-rounding sums (fp32 partials of at
    most 64 rows - `cnt == 64` in colreduce_k, `64L * RL` in colreduce4_k - then fp64), var = E[x^2] - mean^2 in fp64 from those sums
    (bn_prepare_k), the results cast to fp32."""
    s1, s2, a1 = x64.sum(0), (x64 * x64).sum(0), np.abs(x64).sum(0)
    a2 = s2
    mean = s1 / M
    var = np.maximum(s2 / M - mean * mean, 0.0)
    dmean = 66 * U24 * a1 / M
    dvar = 66 * U24 * a2 / M + 2 * np.abs(mean) * dmean + dmean * dmean
    inv = 1.0 / np.sqrt(var + eps)
    inv_lo, inv_hi = 1.0 / np.sqrt(var + dvar + eps), 1.0 / np.sqrt(np.maximum(var - dvar, 0.0) + eps)
    return dict(s1=s1, s2=s2, a1=a1, a2=a2, mean=mean, var=var, dmean=dmean, dvar=dvar, inv=inv, dinv=np.maximum(inv_hi - inv, inv - inv_lo))


@pytest.mark.parametrize("C,M,run,regime", BN_CASES)
def test_column_reductions_and_batchnorm(cg, C, M, run, regime):
    L, st = cg.lib(), cg.tensor.stream()
    mis = regime.get("misaligned", False)
    assert bn_regime(L, C, M, mis) == regime
    rng, x, dy, gamma, beta = bn_inputs(C, M)
    eps, mom, cnt = float(f32(1e-5)), 0.1, float(M)
    x64, dy64, g64, b64 = x.astype(f64), dy.astype(f64), gamma.astype(f64), beta.astype(f64)
    xt, dyt, gt, bt = dev(x, mis), dev(dy, mis), dev(gamma), dev(beta)
    p = lambda t: t.data_ptr()
    dsums = lambda k: torch.full((k,), 3.0, dtype=torch.float64, device="cuda")

    # ---- statistics
    sums = dsums(2 * C)
    L.bn_stats(st, p(xt), M, C, p(sums))
    S = stat_bounds(x64, M, eps)
    hs = sums.cpu().numpy()
    rounding_close(hs[:C], S["s1"], S["a1"], 66, "bn_stats sum x")
    rounding_close(hs[C:], S["s2"], S["a2"], 66, "bn_stats sum x^2")
    full = run == "all"
    alpha = f32(0.25)
    if full:
        rm0, rv0 = (rng.standard_normal(C) * 0.5).astype(f32), rng.uniform(0.5, 2.0, C).astype(f32)
        rm, rv, sm, si, y = dev(rm0), dev(rv0), out_like(C), out_like(C), out_like(M * C, mis)
        L.bn_forward(st, p(xt), p(y), p(gt), p(bt), p(sums), cnt, M, C, eps, mom, p(rm), p(rv), p(sm), p(si))
        mean, inv = host(sm), host(si)
        rounding_close(mean, S["mean"], np.abs(S["mean"]), 1, "save_mean", slack=S["dmean"])
        rounding_close(inv, S["inv"], S["inv"], 1, "save_invstd", slack=S["dinv"])
        # bn_prepare_k's running statistics: 1 - momentum, two products, one sum: 4, + 2
        rounding_close(host(rm), 0.9 * rm0.astype(f64) + 0.1 * S["mean"], 0.9 * np.abs(rm0) + 0.1 * np.abs(S["mean"]), 6, "running_mean",
                       slack=0.1 * (S["dmean"] + U24 * np.abs(S["mean"])))
        unb, dunb = (S["var"] * M / (M - 1.0), S["dvar"] * M / (M - 1.0)) if M > 1 else (S["var"], S["dvar"])
        rounding_close(host(rv), 0.9 * rv0.astype(f64) + 0.1 * unb, 0.9 * np.abs(rv0) + 0.1 * unb, 6, "running_var",
                       slack=0.1 * (dunb + U24 * unb))
        # ---- apply, against fp64 WITH the device's statistics.  bn_apply_k (cg::bn_norm): difference, two products, sum: 4, + 2
        xh = (x64 - mean) * inv.astype(f64)
        rounding_close(host(y, (M, C)), xh * g64 + b64, np.abs(xh * g64) + np.abs(b64), 6, "bn_forward y")
        # ---- backward sums (mode 1).  The term dy * xhat is built from two more roundings: 68
        bs = dsums(2 * C)
        L.bn_backward_stats(st, p(xt), p(dyt), p(sm), p(si), M, C, p(bs))
        hb = bs.cpu().numpy()
        rounding_close(hb[:C], dy64.sum(0), np.abs(dy64).sum(0), 66, "bn_backward_stats sum dy")
        rounding_close(hb[C:], (dy64 * xh).sum(0), np.abs(dy64 * xh).sum(0), 68, "bn_backward_stats sum dy xhat")
        # ---- backward apply with the device's sums.  bn_bwd_k (cg::bn_dx): xhat 2, the cast of m2 1, xhat m2 1, two differences 1
        # (the other one is off the chain), gamma invstd beside it, the last product 1: 7, + 2
        dx, gg, gb = out_like(M * C, mis), dev(np.ones(C, f32)), dev(np.ones(C, f32))
        L.bn_backward(st, p(xt), p(dyt), p(gt), p(sm), p(si), p(bs), cnt, p(bs), M, C, p(dx), p(gg), p(gb), 0.5)
        m1, m2 = (hb[:C] / cnt).astype(f32).astype(f64), (hb[C:] / cnt).astype(f32).astype(f64)
        gi = g64 * inv.astype(f64)
        rounding_close(host(dx, (M, C)), gi * (dy64 - m1 - xh * m2), np.abs(gi) * (np.abs(dy64) + np.abs(m1) + np.abs(xh * m2)), 9,
                       "bn_backward dx")
        # bn_bwd_param_k: cast, product, sum: 3, + 2; accumulates onto 1 with scale 0.5
        rounding_close(host(gb), 1.0 + 0.5 * hb[:C], 1.0 + 0.5 * np.abs(hb[:C]), 5, "gbeta")
        rounding_close(host(gg), 1.0 + 0.5 * hb[C:], 1.0 + 0.5 * np.abs(hb[C:]), 5, "ggamma")
        # ---- bias gradient (mode 2): the 66-rounding sum, cast, product, sum
        gbias, ws = dev(np.ones(C, f32)), dsums(C)
        L.bias_grad(st, p(dyt), p(gbias), M, C, 0.5, p(ws), 8 * C)
        rounding_close(host(gbias), 1.0 + 0.5 * dy64.sum(0), 1.0 + 0.5 * np.abs(dy64).sum(0), 69, "bias_grad")
        # ---- evaluation mode.  bn_eval_k: difference, rv + eps, square root, quotient, product, sum: 6, + 2
        ye = out_like(M * C, mis)
        rme, rve = dev(rm0), dev(rv0)
        L.bn_forward_eval(st, p(xt), p(ye), p(gt), p(bt), p(rme), p(rve), M, C, eps)
        t = (x64 - rm0) / np.sqrt(rv0.astype(f64) + eps) * g64
        rounding_close(host(ye, (M, C)), t + b64, np.abs(t) + np.abs(b64), 8, "bn_forward_eval")

    # ---- batch norm + PReLU in one pass, with a slope and with alpha = NULL
    for with_alpha in ((True, False) if full else (True,)):
        rm2, rv2 = (dev(rm0), dev(rv0)) if full else (dev(np.zeros(C, f32)), dev(np.ones(C, f32)))
        sm2, si2, y2 = out_like(C), out_like(C), out_like(M * C, mis)
        al = scalar(alpha) if with_alpha else None
        L.bn_act_forward(st, p(xt), p(y2), p(gt), p(bt), p(sums), cnt, M, C, eps, mom, p(rm2), p(rv2), p(sm2), p(si2), p(al) if al is not None else None)
        mean, inv = host(sm2), host(si2)
        if full:   # bn_act_fwd_v4k derives them "exactly as bn_prepare_k does": the bits of cg_bn_forward's
            bits_equal(mean, host(sm), "bn_act save_mean"); bits_equal(inv, host(si), "bn_act save_invstd")
            bits_equal(host(rm2), host(rm), "bn_act running_mean"); bits_equal(host(rv2), host(rv), "bn_act running_var")
        else:
            rounding_close(mean, S["mean"], np.abs(S["mean"]), 1, "save_mean", slack=S["dmean"])
            rounding_close(inv, S["inv"], S["inv"], 1, "save_invstd", slack=S["dinv"])
        xh, u, near = bn_near_kink(x, mean, inv, gamma, beta)
        yd = host(y2, (M, C))
        tu = np.abs(xh * g64) + np.abs(b64)
        if not with_alpha:
            rounding_close(yd, u, tu, 6, "bn_act_forward y, no slope")
            pos = np.ones(u.shape, bool)
        else:
            # within 4 roundings of zero the device's side of the kink holds (teacher-forced, as helpers.torch_twin does with KINK);
            # the slope is positive, so the sign of y tells the side the device took
            pos = np.where(near, yd > 0, u > 0)
            flips = int((pos != (u > 0)).sum())
            print(f"kink: {int(near.sum())} of {u.size} elements within 4 roundings of zero, {flips} on the other side")
            assert near.sum() <= 1e-3 * u.size
            # bn_act_fwd_v4k (cg::bn_norm, cg::act): the 4 of the apply and the slope's product: 5, + 2
            rounding_close(yd, np.where(pos, u, f64(alpha) * u), tu, 7, "bn_act_forward y")
        if not regime["v4"]:
            continue                                                             # cg_bn_act_backward* take C % 4 == 0 only (their CG_REQUIRE)
        bs = dsums(2 * C + 1)
        L.bn_act_backward_stats(st, p(xt), p(dyt), p(sm2), p(si2), p(gt), p(bt), p(al) if al is not None else None, M, C, p(bs))
        hb = bs.cpu().numpy()
        dd = np.where(pos, dy64, f64(alpha) * dy64)
        rounding_close(hb[:C], dd.sum(0), np.abs(dd).sum(0), 66, "bn_act_backward_stats sum d")
        rounding_close(hb[C:2 * C], (dd * xh).sum(0), np.abs(dd * xh).sum(0), 68, "bn_act_backward_stats sum d xhat")
        if with_alpha:
            # sg of bn_act_bwd_stats_k: 4 channels x 64 rows added in fp32 per lane, u 4 and its product 1: 261, + 2
            ud = (u * dy64)[~pos]
            rounding_close(hb[2 * C:], [ud.sum()], [np.abs(ud).sum()], 263, "bn_act_backward_stats sum u dy")
        else:
            assert hb[2 * C] == 0.0
        if not full:
            continue
        dx, gg, gb, ga = out_like(M * C), dev(np.ones(C, f32)), dev(np.ones(C, f32)), scalar(1.0)
        L.bn_act_backward(st, p(xt), p(dyt), p(gt), p(bt), p(sm2), p(si2), p(al) if al is not None else None, p(bs), cnt, p(bs), M, C,
                          p(dx), p(gg), p(gb), p(ga), 0.5)
        m1, m2 = (hb[:C] / cnt).astype(f32).astype(f64), (hb[C:2 * C] / cnt).astype(f32).astype(f64)
        gi = g64 * inv.astype(f64)
        # bn_act_bwd_v4k (cg::bn_dx of cg::dact): bn_bwd_k's 7 and the slope's product on dd: 8, + 2
        rounding_close(host(dx, (M, C)), gi * (dd - m1 - xh * m2), np.abs(gi) * (np.abs(dd) + np.abs(m1) + np.abs(xh * m2)), 10,
                       "bn_act_backward dx")
        rounding_close(host(gb), 1.0 + 0.5 * hb[:C], 1.0 + 0.5 * np.abs(hb[:C]), 5, "bn_act gbeta")
        rounding_close(host(gg), 1.0 + 0.5 * hb[C:2 * C], 1.0 + 0.5 * np.abs(hb[C:2 * C]), 5, "bn_act ggamma")
        if with_alpha:
            rounding_close(host(ga), [1.0 + 0.5 * hb[2 * C]], [1.0 + 0.5 * abs(hb[2 * C])], 5, "bn_act galpha")
        else:
            bits_equal(host(ga), np.ones(1, f32), "galpha without a slope stays")


# ------------------------------------------------------------------------------ activation -> pooling -> spatial dropout
@pytest.mark.parametrize("G,NG,H,W,C,masked,acts,slopes,regime", POOL_CASES)
def test_act_pool_mask_over_groups(cg, G, NG, H, W, C, masked, acts, slopes, regime):
    L, st = cg.lib(), cg.tensor.stream()
    assert pool_regime(L, G, NG, H, W, C) == regime
    rng = np.random.default_rng(G * 1000 + NG * 100 + C + len(acts))
    N, Ho, Wo = G * NG, H // 2, W // 2
    x = duplicate_in_windows(rng, edge_normal(rng, (N, H, W, C)))
    gy = edge_normal(rng, (N, Ho, Wo, C))
    mask = None
    if masked == "zero rows":
        mask = (rng.random((N, C)) < 0.8).astype(f32)
        mask[N // 2] = 0.0                                                        # whole samples dropped
        mask[N - 1] = 0.0
    xt, gt = dev(x), dev(gy)
    mt = dev(mask) if mask is not None else None
    mp = mt.data_ptr() if mt is not None else None
    mb = mask[:, None, None, :] if mask is not None else f32(1.0)
    al = [scalar(v) for v in slopes]
    xn = nchw(x)
    for pool_max in (1, 0):
        for act in acts:
            y, dx = out_like(N * Ho * Wo * C), out_like(x.size)
            ga = [scalar(1.0) for _ in slopes]
            L.act_pool2_mask_forward(st, xt.data_ptr(), y.data_ptr(), mp, G, NG, H, W, C, act, 0.333, ptrs(al) if act == 1 else None, pool_max)
            wsb = int(L.act_pool2_mask_backward_workspace_bytes(G, NG, H, W, C))
            ws = torch.zeros(wsb // 8, dtype=torch.float64, device="cuda")
            L.act_pool2_mask_backward(st, xt.data_ptr(), gt.data_ptr(), mp, dx.data_ptr(), G, NG, H, W, C, act, 0.333,
                                      ptrs(al) if act == 1 else None, ptrs(ga) if act == 1 else None, 0.5, pool_max, ws.data_ptr(), wsb)
            yd, dxd = host(y, (N, Ho, Wo, C)), host(dx, x.shape)
            for g in range(G):
                sl = slice(g * NG, (g + 1) * NG)
                what = f"act {act} pool {'max' if pool_max else 'avg'} group {g}"
                A = O.PReLU() if act == 1 else (O.LeakyReLU(0.333) if act == 2 else None)
                if act == 1:
                    A.weight[...] = slopes[g]
                P = O.MaxPool2() if pool_max else O.AvgPool2()
                h = A.forward(xn[sl]) if A else xn[sl]
                pooled = P.forward(h)
                gm = (gy[sl] * mb[sl]) if mask is not None else gy[sl]
                e = P.backward(nchw(gm))                                          # the gradient w.r.t. act(x); max: O.MaxPool2's first argmax
                dref = nhwc(A.backward(e)) if A else nhwc(e)
                bits_equal(dxd[sl], dref, what + " dx")
                if pool_max:
                    # the FIRST maximum's own bits (np.max may return either zero of a -0.0 / +0.0 tie)
                    d = h.reshape(NG, C, Ho, 2, Wo, 2)
                    cand = np.stack([d[:, :, :, 0, :, 0], d[:, :, :, 0, :, 1], d[:, :, :, 1, :, 0], d[:, :, :, 1, :, 1]], axis=-1)
                    pooled = np.take_along_axis(cand, P.arg[..., None], axis=-1)[..., 0]
                if pool_max or act == 0:
                    bits_equal(yd[sl], nhwc(pooled) * mb[sl] if mask is not None else nhwc(pooled), what + " y")
                else:
                    # act_pool2_fwd_k's average: the slope's product feeds the sum: 1 + 3 sums + the (exact) quarter and mask: 4, + 2
                    h64 = nhwc(h).astype(f64).reshape(NG, Ho, 2, Wo, 2, C)
                    mbs = mb[sl] if mask is not None else 1.0
                    rounding_close(yd[sl], h64.sum((2, 4)) * 0.25 * mbs, np.abs(h64).sum((2, 4)) * 0.25 * mbs, 6, what + " y")
                if act == 1:
                    neg = xn[sl] <= 0
                    prod = (xn[sl].astype(f64) * e.astype(f64))[neg]
                    # act_pool2_bwd_k (cg::slope_term): a product, the 3 sums beside it, 4 sums into s per float4 and two passes at most,
                    # then galpha_groups_reduce_k's cast, product and sum: 1 + 3 + 8 + 3, + 2
                    rounding_close(host(ga[g]), [1.0 + 0.5 * prod.sum()], [1.0 + 0.5 * np.abs(prod).sum()], 17, what + " galpha")
                    if slopes[g] == 0.0 and pool_max:
                        ties = int(((cand == cand.max(-1, keepdims=True)).sum(-1) > 1).sum())
                        assert ties > 0.02 * cand[..., 0].size, "slope 0 must make whole windows tie"


@pytest.mark.parametrize("N,H,W,C,regime", PLAIN_POOL_CASES)
def test_plain_pools_and_upsampling(cg, N, H, W, C, regime):
    L, st = cg.lib(), cg.tensor.stream()
    cap = ew_cap(L)
    assert (ew_regime(N * (H // 2) * (W // 2) * C, cap), ew_regime(N * 4 * H * W * C, cap)) == regime
    rng = np.random.default_rng(N * H + C)
    x = duplicate_in_windows(rng, edge_normal(rng, (N, H, W, C)))
    g = edge_normal(rng, (N, H // 2, W // 2, C))
    xt, gt = dev(x, misaligned=True), dev(g, misaligned=True)                     # these kernels are scalar: any alignment
    for name, P in (("maxpool2", O.MaxPool2()), ("avgpool2", O.AvgPool2())):
        y, dx = out_like(g.size), out_like(x.size)
        getattr(L, name + "_forward")(st, xt.data_ptr(), y.data_ptr(), N, H, W, C)
        if name == "maxpool2":
            L.maxpool2_backward(st, xt.data_ptr(), gt.data_ptr(), dx.data_ptr(), N, H, W, C)
        else:
            L.avgpool2_backward(st, gt.data_ptr(), dx.data_ptr(), N, H, W, C)
        ref = P.forward(nchw(x))
        if name == "maxpool2":
            d = nchw(x).reshape(N, C, H // 2, 2, W // 2, 2)
            cand = np.stack([d[:, :, :, 0, :, 0], d[:, :, :, 0, :, 1], d[:, :, :, 1, :, 0], d[:, :, :, 1, :, 1]], axis=-1)
            ref = np.take_along_axis(cand, P.arg[..., None], axis=-1)[..., 0]
        bits_equal(host(y, g.shape), nhwc(ref), name + " forward")
        bits_equal(host(dx, x.shape), nhwc(P.backward(nchw(g))), name + " backward")
    U = O.UpSample2()
    up, gu = out_like(4 * x.size), edge_normal(rng, (N, 2 * H, 2 * W, C))
    L.upsample2x_forward(st, xt.data_ptr(), up.data_ptr(), N, H, W, C)
    bits_equal(host(up, gu.shape), nhwc(U.forward(nchw(x))), "upsample forward")
    dxu = out_like(x.size)
    L.upsample2x_backward(st, dev(gu).data_ptr(), dxu.data_ptr(), N, H, W, C)
    bits_equal(host(dxu, x.shape), nhwc(U.backward(nchw(gu))), "upsample backward")
    # layout changes and copies of the same tensor
    a, b = out_like(x.size), out_like(x.size)
    L.nhwc_to_nchw(st, xt.data_ptr(), a.data_ptr(), N, C, H, W)
    bits_equal(host(a, (N, C, H, W)), nchw(x), "nhwc_to_nchw")
    L.nchw_to_nhwc(st, a.data_ptr(), b.data_ptr(), N, C, H, W)
    bits_equal(host(b, x.shape), x, "nchw_to_nhwc")
    M, Cd = N * H * W, C + 5
    dst = dev(np.full((M, Cd), 9.0, f32))
    co = max(1, C - 1)
    L.copy_channels(st, xt.data_ptr(), dst.data_ptr(), M, C, C - co, Cd, 3, co)
    ref = np.full((M, Cd), 9.0, f32); ref[:, 3:3 + co] = x.reshape(M, C)[:, C - co:]
    bits_equal(host(dst, (M, Cd)), ref, "copy_channels")
    rows = N * H
    idx = rng.integers(0, rows, rows + 3).astype(np.int32)
    gd = out_like(idx.size * W * C)
    L.gather_rows(st, xt.data_ptr(), dev(idx).data_ptr(), gd.data_ptr(), idx.size, W * C)
    bits_equal(host(gd, (idx.size, W * C)), x.reshape(rows, W * C)[idx], "gather_rows")


# ------------------------------------------------------------------------------ concat / split / sum / concat-dropout, mask_mul
@pytest.mark.parametrize("Cs,N,HW,regime", CONCAT_CASES)
def test_concat_split_sum_and_dropout(cg, Cs, N, HW, regime):
    L, st = cg.lib(), cg.tensor.stream()
    n, Ct, M = len(Cs), sum(Cs), N * HW
    assert ew_regime(M * Ct // 4, ew_cap(L)) == regime
    rng = np.random.default_rng(Ct + HW)
    parts = [edge_normal(rng, (M, c)) for c in Cs]
    pt = [dev(a) for a in parts]
    cc = (ctypes.c_int * 4)(*(list(Cs) + [0] * (4 - n)))
    cat_ref = np.concatenate(parts, axis=1)
    cat = out_like(M * Ct)
    L.concat_channels(st, n, ptrs(pt), cc, cat.data_ptr(), M)
    bits_equal(host(cat, (M, Ct)), cat_ref, "concat")
    whole = edge_normal(rng, (M, Ct))
    wt = dev(whole)
    outs = [out_like(M * c) for c in Cs]
    L.split_channels(st, n, wt.data_ptr(), ptrs(outs), cc, M)
    for o, c, ref in zip(outs, Cs, np.split(whole, np.cumsum(Cs)[:-1], axis=1)):
        bits_equal(host(o, (M, c)), ref, "split")
    if n >= 2:     # sum4_v4k: ((a + b) + c) + d
        same = [edge_normal(rng, (M, 4)) for _ in range(n)]
        s = out_like(M * 4)
        L.sum_n(st, n, ptrs([dev(a) for a in same]), s.data_ptr(), M * 4)
        ref = same[0] + same[1]
        for a in same[2:]:
            ref = ref + a
        bits_equal(host(s, (M, 4)), ref, f"sum_n of {n}")
    # nn.Concat -> nn.SpatialDropout in one launch: the noise is cg_rng_bernoulli_dev's at the same offsets, no rescale (value 1)
    seed, off = 20240607, 4099
    out, noise, rn = out_like(M * Ct), out_like(N * Ct), out_like(N * Ct)
    L.concat_channels_dropout(st, n, ptrs(pt), cc, out.data_ptr(), noise.data_ptr(), N, HW, 0.8, 1.0, seed, off, None)
    L.rng_bernoulli_dev(st, rn.data_ptr(), N * Ct, 0.8, 1.0, seed, off, None)
    nz = host(noise, (N, Ct))
    bits_equal(nz, host(rn, (N, Ct)), "noise drawn in the launch")
    assert set(np.unique(nz)) <= {0.0, 1.0} and 0.6 < nz.mean() < 0.95
    D = O.SpatialDropout(0.2, None); D.fixed = nz
    ref = nhwc(D.forward(nchw(cat_ref.reshape(N, HW, 1, Ct))))
    bits_equal(host(out, (N, HW, 1, Ct)), ref, "concat -> dropout against the oracle's module")
    sep = out_like(M * Ct)                                                        # ... and against the launches it replaces
    L.mask_mul(st, cat.data_ptr(), rn.data_ptr(), sep.data_ptr(), N, HW, Ct, 1)
    bits_equal(host(out), host(sep), "concat -> dropout against concat, mask_mul")
    d1, d0, gm = [out_like(M * c) for c in Cs], [out_like(M * c) for c in Cs], out_like(M * Ct)
    L.split_channels_masked(st, n, wt.data_ptr(), noise.data_ptr(), ptrs(d1), cc, N, HW)
    L.mask_mul(st, wt.data_ptr(), noise.data_ptr(), gm.data_ptr(), N, HW, Ct, 1)
    L.split_channels(st, n, gm.data_ptr(), ptrs(d0), cc, M)
    for a, b, c, ref in zip(d1, d0, Cs, np.split(whole.reshape(N, HW, Ct) * nz[:, None, :], np.cumsum(Cs)[:-1], axis=2)):
        bits_equal(host(a), host(b), "masked split against mask_mul, split")
        bits_equal(host(a, (N, HW, c)), ref, "masked split")


# N, HW, C, regime of the vector launch, and the kernel each of the four runs below takes
MASK_CASES = [(3, 5, 12, "one", ("spatial v4", "scalar", "flat v4", "scalar")),
              (2, 7, 10, "one", ("scalar", "scalar", "flat v4", "scalar")),      # C % 4 != 0: the spatial form is scalar
              (5, 17500, 12, "wrap", ("spatial v4", "scalar", "flat v4", "scalar"))]
# (x misaligned, mask misaligned, spatial) of the four runs
MASK_RUNS = ((False, False, 1), (True, False, 1), (False, False, 0), (False, True, 0))


def mask_path(total, C, spatial, x_aligned, mask_aligned):
    """cg_mask_mul's dispatch."""
    if x_aligned and spatial and C % 4 == 0:
        return "spatial v4"
    if x_aligned and not spatial and total % 4 == 0 and mask_aligned:
        return "flat v4"
    return "scalar"


@pytest.mark.parametrize("N,HW,C,regime,paths", MASK_CASES)
def test_mask_mul_paths_agree(cg, N, HW, C, regime, paths):
    """Spatial vector (C % 4 == 0), flat vector (a full-size aligned mask) and the scalar kernel through C % 4 != 0, a misaligned tensor
    or a misaligned mask: the same products on every path."""
    L, st = cg.lib(), cg.tensor.stream()
    total = N * HW * C
    assert ew_regime(total // 4, ew_cap(L)) == regime
    assert tuple(mask_path(total, C, sp, not xa, not ma) for xa, ma, sp in MASK_RUNS) == paths
    rng = np.random.default_rng(C + HW)
    x = edge_normal(rng, (N, HW, C))
    m = (rng.random((N, C)) < 0.7).astype(f32) * f32(1.25)
    full = np.ascontiguousarray(np.broadcast_to(m[:, None, :], x.shape))
    for (xa, ma, sp), path in zip(MASK_RUNS, paths):
        xt, mt, y = dev(x, xa), dev(m if sp else full, ma), out_like(total, xa)
        L.mask_mul(st, xt.data_ptr(), mt.data_ptr(), y.data_ptr(), N, HW, C, sp)
        bits_equal(host(y, x.shape), x * full, f"mask_mul {path}, spatial = {sp}")


# ------------------------------------------------------------------------------ D's head
def head_check(cg, N, F, Oo, rng):
    L, st = cg.lib(), cg.tensor.stream()
    assert L.drop_linear_sigmoid_supported(N, F, Oo) == 1
    seed, off = 99, 3 * N + F
    x = edge_normal(rng, (N, F))
    w = (rng.standard_normal((Oo, F)) * 0.1).astype(f32)
    b, dp = rng.standard_normal(Oo).astype(f32), rng.standard_normal((N, Oo)).astype(f32)
    xt, wt, bt, dpt = dev(x), dev(w), dev(b), dev(dp)
    nz, xd, z, p, rn = out_like(N * F), out_like(N * F), out_like(N * Oo), out_like(N * Oo), out_like(N * F)
    L.drop_linear_sigmoid_forward(st, xt.data_ptr(), wt.data_ptr(), bt.data_ptr(), nz.data_ptr(), xd.data_ptr(), z.data_ptr(), p.data_ptr(),
                                  N, F, Oo, 0.5, 2.0, seed, off, None)
    L.rng_bernoulli_dev(st, rn.data_ptr(), N * F, 0.5, 2.0, seed, off, None)
    mk = host(rn, (N, F))
    bits_equal(host(nz, (N, F)), mk, "head noise")
    D = O.Dropout(0.5, None); D.fixed = mk                                        # Dropout v2: the mask carries 1 / (1 - p)
    xdr = D.forward(x)
    bits_equal(host(xd, (N, F)), xdr, "head xd")
    what = f"head N={N} F={F} O={Oo}"
    w64, xd64 = w.astype(f64), xdr.astype(f64)
    # head_fwd_k: a product, ceil(F / 64) sums per lane, 6 levels of wave_sum, the bias
    per = -(-F // 64)
    zd = host(z, (N, Oo))
    rounding_close(zd, xd64 @ w64.T + b, np.abs(xd64) @ np.abs(w64).T + np.abs(b), per + 8 + 2, what + " z")
    # p = 1 / (1 + expf(-z)) from the device's z (head_fwd_k): expf within 1 ulp (2 roundings' worth), sum, quotient: 4, + 2
    pd = host(p, (N, Oo))
    pr = 1.0 / (1.0 + np.exp(-zd.astype(f64)))
    rounding_close(pd, pr, pr, 6, what + " p")
    gx, gw, gb = out_like(N * F), dev(np.ones((Oo, F), f32)), dev(np.ones(Oo, f32))   # accumulate semantics: start at 1, scale 0.5
    L.drop_linear_sigmoid_backward(st, dpt.data_ptr(), p.data_ptr(), xd.data_ptr(), nz.data_ptr(), wt.data_ptr(), gx.data_ptr(), gw.data_ptr(),
                                   gb.data_ptr(), N, F, Oo, 0.5)
    gz = dp.astype(f64) * (1.0 - pd) * pd                                         # head_bwd_k: 3 roundings
    # gx (head_bwd_k's sample loop): gz 3, a product, O sums, the mask: O + 5, + 2
    rounding_close(host(gx, (N, F)), (gz @ w64) * mk, (np.abs(gz) @ np.abs(w64)) * mk, Oo + 7, what + " gx")
    # gw (the sample loop, then the four lanes' partials): gz 3, a product, ceil(N / 4) sums per lane, 3 sums over the lanes, scale, +=: ceil(N / 4) + 9, + 2
    rounding_close(host(gw, (Oo, F)), 1.0 + 0.5 * gz.T @ xd64, 1.0 + 0.5 * np.abs(gz).T @ np.abs(xd64), -(-N // 4) + 9 + 2, what + " gw")
    # gb (head_bwd_k's last block): gz 3, N sums, scale, +=
    rounding_close(host(gb), 1.0 + 0.5 * gz.sum(0), 1.0 + 0.5 * np.abs(gz).sum(0), N + 5 + 2, what + " gb")
    gx2 = out_like(N * F)
    L.drop_linear_sigmoid_backward(st, dpt.data_ptr(), p.data_ptr(), None, nz.data_ptr(), wt.data_ptr(), gx2.data_ptr(), None, None, N, F, Oo, 0.0)
    bits_equal(host(gx2), host(gx), what + " gx alone")


@pytest.mark.parametrize("Oo", HEAD_O)
def test_head_over_its_lane_edges(cg, Oo):
    rng = np.random.default_rng(Oo)
    for N in HEAD_N:
        for F in HEAD_F:
            head_check(cg, N, F, Oo, rng)


def head_max_n(L, F=65, Oo=1):
    lo, hi = 1, 1 << 20
    assert L.drop_linear_sigmoid_supported(lo, F, Oo) == 1 and L.drop_linear_sigmoid_supported(hi, F, Oo) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if L.drop_linear_sigmoid_supported(mid, F, Oo) else (lo, mid)
    return lo


def test_head_at_the_largest_batch_it_accepts(cg):
    L, st = cg.lib(), cg.tensor.stream()
    N, F = head_max_n(L), 65
    assert N >= 4096, "the backward keeps gz[N][O] in the LDS: the benchmarked batches must fit"
    head_check(cg, N, F, 1, np.random.default_rng(5))
    t = out_like((N + 1) * F)
    for call in (lambda: L.drop_linear_sigmoid_forward(st, t.data_ptr(), t.data_ptr(), None, t.data_ptr(), t.data_ptr(), t.data_ptr(),
                                                       t.data_ptr(), N + 1, F, 1, 0.5, 2.0, 1, 0, None),
                 lambda: L.drop_linear_sigmoid_backward(st, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(),
                                                        None, None, N + 1, F, 1, 0.5)):
        with pytest.raises(cg.CatganError, match="unsupported shape"):
            call()
    bits_equal(host(t), np.full((N + 1) * F, 555.0, f32), "a refused call launches nothing")


# ------------------------------------------------------------------------------ optimiser kernels
def test_optimiser_kernels_past_the_wrap(cg):
    L, st = cg.lib(), cg.tensor.stream()
    n = OPT_N
    assert ew_regime(n, ew_cap(L)) == "wrap"
    rng = np.random.default_rng(8)
    p0, g = edge_normal(rng, (n, 1)).ravel(), edge_normal(rng, (n, 1)).ravel()
    m0, v0 = (rng.standard_normal(n) * 0.1).astype(f32), (rng.random(n) * 0.1).astype(f32)
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    # adam_k and O.adam's fp32 restatement each stay within r roundings of the exact update, so of one another
    # within 2 r.  m: 1 - b1, two products, sum: 4.  v: 1 - b2, three products, sum: 5, halved by the root.  p: m 4, v 3, root, + eps,
    # step product, quotient, difference: 12, + 2.  One difference between the two is no rounding of an operation: the kernel forms 1 - b
    # in fp32 from the fp32 b (exactly), optim.adam and the oracle round the double 1 - b.  The two weights differ by the rounding of
    # b itself, at most 2^-24 absolutely (1.3e-5 of 1 - b2): a slack of 2^-24 |g| on m and 2^-24 g^2 on v, carried into p.  Likewise the
    # ABI takes lr and the betas as floats, so cg_adam_step's bias corrections 1 - b^t are those of the rounded betas (d(b^t) = t b^t
    # 2^-24): the step differs from optim.adam's by up to 2^-24 (1 + t b1^t / (1 - b1^t) + t b2^t / 2 (1 - b2^t)), 6.7e-6 of it at t = 1.
    for t in (1, 2, 3):
        po, st_o = p0.copy(), {"t": t - 1, "m": m0.copy(), "v": v0.copy()}
        O.adam(po, g, st_o, lr=lr, b1=b1, b2=b2, eps=eps)
        pt, gt, mt, vt = dev(p0), dev(g), dev(m0), dev(v0)
        L.adam_step(st, pt.data_ptr(), gt.data_ptr(), mt.data_ptr(), vt.data_ptr(), n, lr, b1, b2, eps, t, 0.0, 0.0, 0.0, 0)
        tm = b1 * np.abs(m0.astype(f64)) + (1 - b1) * np.abs(g.astype(f64))
        tv = b2 * v0.astype(f64) + (1 - b2) * g.astype(f64) ** 2
        dm, dv = U24 * np.abs(g.astype(f64)), U24 * g.astype(f64) ** 2
        rounding_close(host(mt), st_o["m"], tm, 2 * 6, f"adam m, t = {t}", slack=dm)
        rounding_close(host(vt), st_o["v"], tv, 2 * 7, f"adam v, t = {t}", slack=dv)
        step, den = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t), np.sqrt(tv) + eps
        dstep = U24 * (1 + t * b1 ** t / (1 - b1 ** t) + 0.5 * t * b2 ** t / (1 - b2 ** t))
        rounding_close(host(pt), po, np.abs(p0.astype(f64)) + step * tm / den, 2 * 14, f"adam p, t = {t}",
                       slack=step * (dm + tm * 0.5 * dv / np.maximum(tv, 1e-300) + tm * dstep) / den)
        # the replay-safe form reads t from device memory and derives the same step (adam_k's `t_dev` branch): the same bits
        p2, g2, m2, v2 = dev(p0), dev(g), dev(m0), dev(v0)
        td = torch.tensor([t], dtype=torch.int64, device="cuda")
        L.adam_step_dev(st, p2.data_ptr(), g2.data_ptr(), m2.data_ptr(), v2.data_ptr(), n, lr, b1, b2, eps, td.data_ptr(), 0.0, 0.0, 0.0, 0)
        for a, b, what in ((p2, pt, "p"), (m2, mt, "m"), (v2, vt, "v")):
            bits_equal(host(a), host(b), f"adam_step_dev {what}, t = {t}")
    # sgd_k: 1 - dampening, two products, sum, lr product, difference: 6, + 2; without momentum 2, + 2; the same
    # slack for 1 - dampening
    for mom in (0.0, 0.9):
        po, st_o = p0.copy(), ({"v": m0.copy()} if mom else {})
        O.sgd(po, g, st_o, lr=0.02, momentum=mom)
        pt, gt, vt = dev(p0), dev(g), dev(m0)
        L.sgd_step(st, pt.data_ptr(), gt.data_ptr(), vt.data_ptr(), n, 0.02, mom, mom, 0.0, 0.0, 0.0, 0)
        d = mom * np.abs(m0.astype(f64)) + (1 - mom) * np.abs(g.astype(f64))
        dd = U24 * np.abs(g.astype(f64)) if mom else 0.0
        rounding_close(host(pt), po, np.abs(p0.astype(f64)) + 0.02 * d, 2 * (8 if mom else 4), f"sgd p, momentum {mom}", slack=0.02 * dd)
        if mom:
            rounding_close(host(vt), st_o["v"], d, 2 * 6, "sgd v", slack=dd)
    # adagrad_k: var 2, halved by the root 1, root, + 1e-10, lr product, quotient, difference: 6, + 2
    po, st_o = p0.copy(), {"var": v0.copy()}
    O.adagrad(po, g, st_o, lr=1e-3)
    pt, gt, vt = dev(p0), dev(g), dev(v0)
    L.adagrad_step(st, pt.data_ptr(), gt.data_ptr(), vt.data_ptr(), n, 1e-3, 0.0, 0.0, 0.0, 0)
    var = v0.astype(f64) + g.astype(f64) ** 2
    rounding_close(host(vt), st_o["var"], var, 2 * 4, "adagrad var")
    rounding_close(host(pt), po, np.abs(p0.astype(f64)) + 1e-3 * np.abs(g.astype(f64)) / (np.sqrt(var) + 1e-10), 2 * 8, "adagrad p")
