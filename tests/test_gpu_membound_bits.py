"""Bit-for-bit pins of the memory-bound kernels of csrc/ops.hip (with csrc/optim.hip's Adam) and csrc/fused.hip, and of the two other users of the shared activation
(the GEMM epilogue of csrc/gemm.hip, the localisation launch of csrc/locnet.hip).

The element arithmetic of these kernels is written once, in csrc/common.h, and every scalar / float4 twin is one template: a restructuring
of that must not move a single bit, neither between a fused kernel and the kernels it replaces nor between a vector kernel and its scalar
twin.  Every case below calls the C ABI directly on fixed-seed inputs - the cases, seeds and inputs of tests/test_gpu_membound_edges.py, which
proved that they reach each dispatch regime - and takes one sha256 over the raw bytes of the results.  tests/golden/membound_bits.json holds
the digests, RECORDED ON A BUILD OF THE COMMIT BEFORE THE RESTRUCTURING by this same file, before a kernel was touched:

    CG_MEMBOUND_BITS_RECORD=<file.json> pytest tests/test_gpu_membound_bits.py      # writes the digests instead of comparing them

Nothing here compares with a reference implementation - that is tests/test_gpu_membound_edges.py and tests/test_gpu_parity.py.  The
LeakyReLU slopes of the epilogue and localisation cases are negative and their inputs hold whole zero samples behind zero biases: the
pre-activation is then exactly +0.0, and only there do `>=` and `>` part (+0.0 against slope * +0.0 = -0.0)."""
import ctypes
import hashlib
import importlib
import json
import os

import numpy as np
import pytest
import torch

import test_gpu_membound_edges as E
from helpers import dev, duplicate_in_windows, edge_normal, host, options, out_like
from test_gpu_locnet_stages import mfma_shape
from test_gpu_membound_edges import ptrs, scalar

pytestmark = pytest.mark.gpu
f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "membound_bits.json")
RECORD = os.environ.get("CG_MEMBOUND_BITS_RECORD")
_recorded = {}


@pytest.fixture(scope="module")
def cg():
    mod = importlib.import_module("cat-generator_amd")
    assert torch.cuda.is_available(), "these tests need the MI355X"
    mod.lib()
    yield mod
    if RECORD:
        with open(RECORD, "w") as f:
            json.dump(_recorded, f, indent=1, sort_keys=True)
            f.write("\n")


@pytest.fixture(scope="module")
def golden():
    if RECORD:
        return {}
    with open(GOLDEN) as f:
        return json.load(f)


def arr(t):
    """Host bytes of a result: a guarded tensor of the edge sweep (its guards are checked), a plain device tensor, or an array."""
    if isinstance(t, np.ndarray):
        return t
    return host(t) if hasattr(t, "guard") else t.cpu().numpy()


def check(golden, case, *tensors, vanishes=()):
    """One digest over the raw bytes of `tensors`.  vanishes: positions of results that are zero by construction (stated at the call)."""
    h = hashlib.sha256()
    for k, t in enumerate(tensors):
        a = np.ascontiguousarray(arr(t))
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f"{case}: result {k} is not finite"
        assert k in vanishes or np.abs(a).max() > 0, f"{case}: result {k} is all zero and pins nothing"
        h.update(a.tobytes())
    digest = h.hexdigest()
    print(f"{case}: sha256 {digest}")
    if RECORD:
        assert case not in _recorded, f"{case}: two results under one name"
        _recorded[case] = digest
        return
    assert case in golden, f"{case}: no digest in {GOLDEN}"
    assert digest == golden[case], f"{case}: the results differ from the recorded bits"


def p(t):
    return t.data_ptr() if t is not None else None


def dsums(k):
    return torch.full((k,), 3.0, dtype=torch.float64, device="cuda")


# ------------------------------------------------------------------------------ activations, add, axpy
@pytest.mark.parametrize("n,misaligned,regime", E.ACT_CASES)
def test_activations_add_axpy(cg, golden, n, misaligned, regime):
    """The inputs are the edge sweep's: +0.0, -0.0 and +-1e-30 planted, where PReLU (x > 0) and LeakyReLU (x >= 0) part."""
    L, st = cg.lib(), cg.tensor.stream()
    assert E.act_regime(L, n, misaligned) == regime
    rng = np.random.default_rng(n + misaligned)
    x, dy = edge_normal(rng, (n, 1)).ravel(), edge_normal(rng, (n, 1)).ravel()
    assert (x == 0).any() or n == 1
    case = f"n {n}{' misaligned' if misaligned else ''}"
    xt, dyt, al = dev(x, misaligned), dev(dy, misaligned), scalar(f32(0.25))
    y, dx, ga = out_like(n, misaligned), out_like(n, misaligned), scalar(1.0)
    L.prelu_forward(st, p(xt), p(al), p(y), n)
    wsb = int(L.prelu_backward_workspace_bytes(n))
    ws = torch.zeros(wsb // 8, dtype=torch.float64, device="cuda")
    L.prelu_backward(st, p(xt), p(dyt), p(al), p(dx), p(ga), 0.5, n, p(ws), wsb)
    check(golden, f"prelu / {case}", y, dx, ga)
    y2, dx2 = out_like(n, misaligned), out_like(n, misaligned)
    L.leakyrelu_forward(st, p(xt), p(y2), 0.333, n)
    L.leakyrelu_backward(st, p(xt), p(dyt), p(dx2), 0.333, n)
    check(golden, f"leakyrelu / {case}", y2, dx2)
    s, acc = out_like(n, misaligned), dev(dy, misaligned)
    L.add(st, p(xt), p(dyt), p(s), n)
    L.axpy(st, 0.333, p(xt), p(acc), n)
    check(golden, f"add, axpy / {case}", s, acc)


@pytest.mark.parametrize("G,n,regime", E.GROUPED_PRELU_CASES)
def test_prelu_backward_grouped(cg, golden, G, n, regime):
    L, st = cg.lib(), cg.tensor.stream()
    assert E.grouped_regime(L, n // 4) == regime
    rng = np.random.default_rng(G * 7 + n)
    x, dy = edge_normal(rng, (G * n, 1)), edge_normal(rng, (G * n, 1))
    slopes = [f32(v) for v in (0.25, -0.1, 0.0, 1.5)[:G]]
    xt, dyt, dx = dev(x), dev(dy), out_like(G * n)
    al, ga = [scalar(v) for v in slopes], [scalar(1.0) for _ in slopes]
    wsb = int(L.prelu_backward_grouped_workspace_bytes(G, n))
    ws = torch.zeros(wsb // 8, dtype=torch.float64, device="cuda")
    L.prelu_backward_grouped(st, p(xt), p(dyt), ptrs(al), p(dx), ptrs(ga), 0.5, G, n, p(ws), wsb)
    check(golden, f"prelu grouped / G {G} n {n}", dx, *ga)


# ------------------------------------------------------------------------------ the batch-norm family
@pytest.mark.parametrize("C,M,run,regime", [c for c in E.BN_CASES if c[2] == "all"])     # the 16.8 M-row case stays in the edge sweep
def test_batchnorm(cg, golden, C, M, run, regime):
    L, st = cg.lib(), cg.tensor.stream()
    mis = regime.get("misaligned", False)
    assert E.bn_regime(L, C, M, mis) == regime
    rng, x, dy, gamma, beta = E.bn_inputs(C, M)
    eps, mom, cnt = float(f32(1e-5)), 0.1, float(M)
    rm0, rv0 = (rng.standard_normal(C) * 0.5).astype(f32), rng.uniform(0.5, 2.0, C).astype(f32)
    xt, dyt, gt, bt = dev(x, mis), dev(dy, mis), dev(gamma), dev(beta)
    case = f"bn C {C} M {M}{' misaligned' if mis else ''}"
    one_row = (0,) if M == 1 else ()            # a batch of one row: xhat = 0 and dy - mean(dy) = 0, so dx vanishes
    sums = dsums(2 * C)
    L.bn_stats(st, p(xt), M, C, p(sums))
    rm, rv, sm, si, y = dev(rm0), dev(rv0), out_like(C), out_like(C), out_like(M * C, mis)
    L.bn_forward(st, p(xt), p(y), p(gt), p(bt), p(sums), cnt, M, C, eps, mom, p(rm), p(rv), p(sm), p(si))
    check(golden, f"{case} / statistics, forward", sums, sm, si, rm, rv, y)
    bs = dsums(2 * C)
    L.bn_backward_stats(st, p(xt), p(dyt), p(sm), p(si), M, C, p(bs))
    dx, gg, gb = out_like(M * C, mis), dev(np.ones(C, f32)), dev(np.ones(C, f32))
    L.bn_backward(st, p(xt), p(dyt), p(gt), p(sm), p(si), p(bs), cnt, p(bs), M, C, p(dx), p(gg), p(gb), 0.5)
    check(golden, f"{case} / backward", dx, bs, gg, gb, vanishes=one_row)
    for with_alpha in (True, False):
        rm2, rv2, sm2, si2, y2 = dev(rm0), dev(rv0), out_like(C), out_like(C), out_like(M * C, mis)
        al = scalar(f32(0.25)) if with_alpha else None
        L.bn_act_forward(st, p(xt), p(y2), p(gt), p(bt), p(sums), cnt, M, C, eps, mom, p(rm2), p(rv2), p(sm2), p(si2), p(al))
        check(golden, f"{case} / bn_act forward, slope {int(with_alpha)}", y2, sm2, si2, rm2, rv2)
        if not regime["v4"]:
            continue                            # cg_bn_act_backward* take C % 4 == 0 and aligned tensors only
        bs2 = dsums(2 * C + 1)
        L.bn_act_backward_stats(st, p(xt), p(dyt), p(sm2), p(si2), p(gt), p(bt), p(al), M, C, p(bs2))
        dx2, gg2, gb2, ga2 = out_like(M * C), dev(np.ones(C, f32)), dev(np.ones(C, f32)), scalar(1.0)
        L.bn_act_backward(st, p(xt), p(dyt), p(gt), p(bt), p(sm2), p(si2), p(al), p(bs2), cnt, p(bs2), M, C, p(dx2), p(gg2), p(gb2), p(ga2), 0.5)
        check(golden, f"{case} / bn_act backward, slope {int(with_alpha)}", dx2, bs2, gg2, gb2, ga2, vanishes=one_row)


# ------------------------------------------------------------------------------ activation -> pooling -> spatial dropout, plain pools
@pytest.mark.parametrize("G,NG,H,W,C,masked,acts,slopes,regime", E.POOL_CASES)
def test_act_pool_mask(cg, golden, G, NG, H, W, C, masked, acts, slopes, regime):
    L, st = cg.lib(), cg.tensor.stream()
    assert E.pool_regime(L, G, NG, H, W, C) == regime
    rng = np.random.default_rng(G * 1000 + NG * 100 + C + len(acts))
    N, Ho, Wo = G * NG, H // 2, W // 2
    x = duplicate_in_windows(rng, edge_normal(rng, (N, H, W, C)))
    gy = edge_normal(rng, (N, Ho, Wo, C))
    mt = None
    if masked == "zero rows":
        mask = (rng.random((N, C)) < 0.8).astype(f32)
        mask[N // 2] = 0.0
        mask[N - 1] = 0.0
        mt = dev(mask)
    xt, gt, al = dev(x), dev(gy), [scalar(v) for v in slopes]
    for pool_max in (1, 0):
        for act in acts:
            y, dx, ga = out_like(N * Ho * Wo * C), out_like(x.size), [scalar(1.0) for _ in slopes]
            L.act_pool2_mask_forward(st, p(xt), p(y), p(mt), G, NG, H, W, C, act, 0.333, ptrs(al) if act == 1 else None, pool_max)
            wsb = int(L.act_pool2_mask_backward_workspace_bytes(G, NG, H, W, C))
            ws = torch.zeros(wsb // 8, dtype=torch.float64, device="cuda")
            L.act_pool2_mask_backward(st, p(xt), p(gt), p(mt), p(dx), G, NG, H, W, C, act, 0.333, ptrs(al) if act == 1 else None,
                                      ptrs(ga) if act == 1 else None, 0.5, pool_max, p(ws), wsb)
            check(golden, f"act_pool G {G} NG {NG} {H}x{W}x{C} {masked} {slopes} / act {act} / {'max' if pool_max else 'avg'}", y, dx, *ga)


@pytest.mark.parametrize("N,H,W,C,regime", E.PLAIN_POOL_CASES)
def test_plain_pools_upsampling_layout(cg, golden, N, H, W, C, regime):
    L, st = cg.lib(), cg.tensor.stream()
    rng = np.random.default_rng(N * H + C)
    x = duplicate_in_windows(rng, edge_normal(rng, (N, H, W, C)))
    g = edge_normal(rng, (N, H // 2, W // 2, C))
    xt, gt = dev(x, misaligned=True), dev(g, misaligned=True)
    ym, dxm, ya, dxa = out_like(g.size), out_like(x.size), out_like(g.size), out_like(x.size)
    L.maxpool2_forward(st, p(xt), p(ym), N, H, W, C)
    L.maxpool2_backward(st, p(xt), p(gt), p(dxm), N, H, W, C)
    L.avgpool2_forward(st, p(xt), p(ya), N, H, W, C)
    L.avgpool2_backward(st, p(gt), p(dxa), N, H, W, C)
    up, gu, dxu = out_like(4 * x.size), edge_normal(rng, (N, 2 * H, 2 * W, C)), out_like(x.size)
    L.upsample2x_forward(st, p(xt), p(up), N, H, W, C)
    L.upsample2x_backward(st, p(dev(gu)), p(dxu), N, H, W, C)
    a, b = out_like(x.size), out_like(x.size)
    L.nhwc_to_nchw(st, p(xt), p(a), N, C, H, W)
    L.nchw_to_nhwc(st, p(a), p(b), N, C, H, W)
    check(golden, f"pools, upsampling, layout {N}x{H}x{W}x{C}", ym, dxm, ya, dxa, up, dxu, a, b)


# ------------------------------------------------------------------------------ concat / split / sum / concat-dropout, mask_mul
@pytest.mark.parametrize("Cs,N,HW,regime", E.CONCAT_CASES)
def test_concat_split_sum_dropout(cg, golden, Cs, N, HW, regime):
    L, st = cg.lib(), cg.tensor.stream()
    n, Ct, M = len(Cs), sum(Cs), N * HW
    rng = np.random.default_rng(Ct + HW)
    pt = [dev(edge_normal(rng, (M, c))) for c in Cs]
    cc = (ctypes.c_int * 4)(*(list(Cs) + [0] * (4 - n)))
    cat, wt, outs = out_like(M * Ct), dev(edge_normal(rng, (M, Ct))), [out_like(M * c) for c in Cs]
    L.concat_channels(st, n, ptrs(pt), cc, p(cat), M)
    L.split_channels(st, n, p(wt), ptrs(outs), cc, M)
    res = [cat, *outs]
    if n >= 2:
        s = out_like(M * 4)
        L.sum_n(st, n, ptrs([dev(edge_normal(rng, (M, 4))) for _ in range(n)]), p(s), M * 4)
        res.append(s)
    out, noise, gm, d1 = out_like(M * Ct), out_like(N * Ct), out_like(M * Ct), [out_like(M * c) for c in Cs]
    L.concat_channels_dropout(st, n, ptrs(pt), cc, p(out), p(noise), N, HW, 0.8, 1.0, 20240607, 4099, None)
    L.mask_mul(st, p(wt), p(noise), p(gm), N, HW, Ct, 1)
    L.split_channels_masked(st, n, p(wt), p(noise), ptrs(d1), cc, N, HW)
    check(golden, f"concat {Cs} N {N} HW {HW}", *res, out, noise, gm, *d1)


@pytest.mark.parametrize("N,HW,C,regime,paths", E.MASK_CASES)
def test_mask_mul(cg, golden, N, HW, C, regime, paths):
    L, st = cg.lib(), cg.tensor.stream()
    total = N * HW * C
    assert tuple(E.mask_path(total, C, sp, not xa, not ma) for xa, ma, sp in E.MASK_RUNS) == paths
    rng = np.random.default_rng(C + HW)
    x = edge_normal(rng, (N, HW, C))
    m = (rng.random((N, C)) < 0.7).astype(f32) * f32(1.25)
    full = np.ascontiguousarray(np.broadcast_to(m[:, None, :], x.shape))
    for (xa, ma, sp), path in zip(E.MASK_RUNS, paths):
        xt, mt, y = dev(x, xa), dev(m if sp else full, ma), out_like(total, xa)
        L.mask_mul(st, p(xt), p(mt), p(y), N, HW, C, sp)
        check(golden, f"mask_mul {N}x{HW}x{C} / x off {int(xa)} mask off {int(ma)} spatial {sp} ({path})", y)


# ------------------------------------------------------------------------------ the bilinear sampler
@pytest.mark.parametrize("C,misaligned", [(4, False), (3, False), (4, True)], ids=["float4", "scalar", "float4 shape, 4 bytes off"])
def test_bilinear_sampler(cg, golden, C, misaligned):
    """Grids from -1.3 to 1.3: each of the four taps lies outside the image for some pixel.  The plain and the shared forward (two
    sibling grids on the same images), and one backward (the deterministic gather form, whose per-lane vector moved to common.h)."""
    L, st = cg.lib(), cg.tensor.stream()
    N, G, Hi, Ho = 2, 2, 5, 4
    rs = np.random.RandomState(10 * C + misaligned)
    img = rs.randn(N, Hi, Hi, C).astype(f32)
    grid = (rs.rand(G * N, Ho, Ho, 2) * 2.6 - 1.3).astype(f32)
    gout = rs.randn(G * N, Ho, Ho, C).astype(f32)
    for yx in (0, 1):       # every tap really is outside for some pixel: the top-left cell index reaches -1 and the last row / column
        c = (grid[..., yx].astype(np.float64) + 1) * (Hi - 1) * 0.5
        assert np.floor(c).min() == -1 and np.floor(c).max() >= Hi - 1
    ti, tg, to = dev(img, misaligned), dev(grid), dev(gout, misaligned)
    out, outs = out_like(N * Ho * Ho * C, misaligned), out_like(G * N * Ho * Ho * C, misaligned)
    L.bilinear_sampler_forward(st, p(ti), p(tg), p(out), N, Hi, Hi, C, Ho, Ho)
    L.bilinear_sampler_forward_shared(st, G, p(ti), p(tg), p(outs), N, Hi, Hi, C, Ho, Ho)
    gimg, ggrid = out_like(N * Hi * Hi * C, misaligned), out_like(N * Ho * Ho * 2)
    L.bilinear_sampler_backward(st, p(ti), p(tg), p(to), p(gimg), p(ggrid), N, Hi, Hi, C, Ho, Ho)
    check(golden, f"sampler C {C}{' misaligned' if misaligned else ''}", out, outs, gimg, ggrid)


# ------------------------------------------------------------------------------ the other users of the shared activation
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("act", [1, 2])
def test_gemm_activation_epilogue(cg, golden, act, splits):
    """cg_conv2d_forward_ex with act = 1 (PReLU) and 2 (LeakyReLU): y and y_act, unsplit (the activation in the GEMM's epilogue) and with
    three forced splits (in the reduce kernel).  Sample 1 is all zero and the first eight biases are zero: exact +0.0 pre-activations."""
    L, st = cg.lib(), cg.tensor.stream()
    N, H, Cin, Cout = 2, 8, 32, 64
    rs = np.random.RandomState(act)
    x = rs.randn(N, H, H, Cin).astype(f32)
    x[1] = 0.0
    w, b = (rs.randn(Cout, Cin, 3, 3) / np.sqrt(9 * Cin)).astype(f32), rs.randn(Cout).astype(f32)
    b[:8] = 0.0
    xt, wt, bt, al = dev(x), dev(w), dev(b), scalar(f32(-0.25))
    wf = out_like(int(L.pack_conv_weight_floats(Cout, Cin, 3, 3)))
    L.pack_conv_weight(st, p(wt), p(wf), None, Cout, Cin, 3, 3)
    with options(cg, CG_NN_SPLITS=splits):
        wsb = int(L.conv2d_workspace_bytes(N, H, H, Cin, Cout, 3, 3, 1, 1, 0))
        ws = torch.zeros(max(wsb, 16), dtype=torch.uint8, device="cuda")
        y, ya = out_like(N * H * H * Cout), out_like(N * H * H * Cout)
        L.conv2d_forward_ex(st, 1, ptrs([xt]), ptrs([wf]), ptrs([bt]), ptrs([y]), N, H, H, Cin, Cout, 3, 3, 1, 1, 0, act, -0.2,
                            ptrs([al]) if act == 1 else None, ptrs([ya]), None, p(ws), wsb)
    yh = host(y).reshape(N, H, H, Cout)
    assert (yh[1, :, :, :8] == 0).all() and not np.signbit(yh[1, :, :, :8]).any(), "the planted pre-activations must be +0.0"
    check(golden, f"conv epilogue act {act} / splits {splits}", y, ya)


def locnet_weights(cg, rs, S, Cin, P, zero_b3):
    """The 12 device tensors of one localisation net (the canonical eight, then cg_pack_conv_weight's copies of both convolutions);
    every second bias of the first convolution (zero_b3: and of the first linear layer) is zero."""
    L, st = cg.lib(), cg.tensor.stream()
    K3 = 16 * (S // 2) ** 2
    T = lambda *shape, sc=1.0: (rs.randn(*shape) * sc).astype(f32)
    w1, b1, w2, b2 = T(16, Cin, 3, 3, sc=0.1), T(16, sc=0.1), T(16, 16, 3, 3, sc=0.1), T(16, sc=0.1)
    w3, b3, w4, b4 = T(64, K3, sc=0.05), T(64, sc=0.1), T(P, 64, sc=0.05), T(P, sc=0.1)
    b1[::2] = 0.0
    if zero_b3:
        b3[::2] = 0.0
    ts = [dev(a) for a in (w1, b1, w2, b2, w3, b3, w4, b4)]
    ts += [out_like(9 * Cin * 16), out_like(9 * 16 * Cin), out_like(9 * 256), out_like(9 * 256)]
    L.pack_conv_weight(st, p(ts[0]), p(ts[8]), p(ts[9]), 16, Cin, 3, 3)
    L.pack_conv_weight(st, p(ts[2]), p(ts[10]), p(ts[11]), 16, 16, 3, 3)
    return ts


def locnet_forward_outs(cg, G, N, S, Cin, flags, hw, ts, x, x_shared):
    L, st = cg.lib(), cg.tensor.stream()
    P, GN, K3 = flags[0] + flags[1] + 2 * flags[2], G * N, 16 * (S // 2) ** 2
    xt = dev(x)
    sizes = (GN * S * S * Cin, GN * S * S * 16, GN * S * S * 16, GN * K3, GN * 64, GN * P, GN * hw[0] * hw[1] * 2)
    outs = [out_like(k) for k in sizes]
    L.locnet_forward(st, G, N, p(xt), x_shared, ptrs(ts), S, Cin, P, *flags, -0.333, *hw, *[p(o) for o in outs])
    return outs


def locnet_backward_outs(cg, G, N, S, Cin, flags, hw, ts, seed):
    """cg_locnet_backward at slope 0.25 on independent arrays with zeros planted (the backward is a pure function of its arrays, as the
    `indep` cases of tests/test_gpu_locnet_stages.py use it): ga1, ga2, g3, g4, gx."""
    L, st = cg.lib(), cg.tensor.stream()
    P, GN = flags[0] + flags[1] + 2 * flags[2], G * N
    rng = np.random.default_rng(seed)
    h1, m2, h3 = edge_normal(rng, (GN, S, S, 16)), edge_normal(rng, (GN, S, S, 16)), edge_normal(rng, (GN, 64))
    prm = np.concatenate(([rng.uniform(-3.0, 3.0, (GN, 1))] if flags[0] else []) + ([rng.uniform(0.5, 1.5, (GN, 1))] if flags[1] else [])
                         + ([rng.uniform(-0.5, 0.5, (GN, 2))] if flags[2] else []), 1).astype(f32)
    ggrid = edge_normal(rng, (GN, *hw, 2))
    assert all((a == 0).any() for a in (h1, m2, h3, ggrid))
    ins = [dev(a) for a in (h1, m2, h3, prm, ggrid)]
    outs = [out_like(k) for k in (GN * S * S * 16, GN * S * S * 16, GN * 64, GN * P, GN * 4 * S * S * Cin)]
    L.locnet_backward(st, G, N, ptrs(ts), S, Cin, P, *flags, 0.25, *hw, *[p(t) for t in ins], *[p(o) for o in outs])
    return outs


def test_locnet_forward(cg, golden):
    """cg_locnet_forward at the smallest localisation shape of tests/test_gpu_parity.py (16 x 16 input of 8 planes: S = 8, all four
    transform parameters), one group of two samples; sample 1 is all zero and every second bias of the first convolution is zero."""
    G, N, S, Cin, P = 1, 2, 8, 8, 4
    assert cg.lib().locnet_supported(S, Cin, P) == 1 and not mfma_shape(S, Cin)
    rs = np.random.RandomState(S)
    ts = locnet_weights(cg, rs, S, Cin, P, zero_b3=False)
    x = (rs.randn(N, 2 * S, 2 * S, Cin) * 1.0).astype(f32)
    x[1] = 0.0
    check(golden, "locnet forward S 8 Cin 8 P 4", *locnet_forward_outs(cg, G, N, S, Cin, (1, 1, 1), (2 * S, 2 * S), ts, x, 0))


def test_locnet_backward_valu(cg, golden):
    """cg_locnet_backward of the VALU kernels at the forward case's shape (S 8, Cin 8, P 4, one group of two samples), slope 0.25."""
    G, N, S, Cin, P = 1, 2, 8, 8, 4
    assert cg.lib().locnet_supported(S, Cin, P) == 1 and not mfma_shape(S, Cin)
    ts = locnet_weights(cg, np.random.RandomState(S + 100), S, Cin, P, zero_b3=True)
    check(golden, "locnet backward S 8 Cin 8 P 4", *locnet_backward_outs(cg, G, N, S, Cin, (1, 1, 1), (2 * S, 2 * S), ts, seed=S))


@pytest.mark.parametrize("S,Cin,G,shared,hw", [
    (4, 64, 1, 0, (8, 8)),         # one M tile, the K3 = 64 paths, conv 2 on wave 0
    (8, 64, 1, 0, (16, 16)),       # KSPLIT partials over the pooled image, NSPLIT data gradient
    (16, 3, 2, 1, (32, 32)),       # zero-padded K step and N tile, the scalar pooling branch; two groups on one input
    (4, 64, 1, 0, (1, 7)),         # Hg == 1: the n == 1 side of the grid coordinate
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_locnet_mfma(cg, golden, S, Cin, G, shared, hw):
    """cg_locnet_forward (slope -0.333) and cg_locnet_backward (slope 0.25) of the MFMA kernels, one case per instantiated shape: two
    samples per group, sample 1 all zero, every second bias of conv 1 and of linear 1 zero."""
    N, P = 2, 4
    assert cg.lib().locnet_supported(S, Cin, P) == 1 and mfma_shape(S, Cin)
    rs = np.random.RandomState(1000 * S + Cin + hw[0])
    ts = [t for _ in range(G) for t in locnet_weights(cg, rs, S, Cin, P, zero_b3=True)]
    x = rs.randn(N if shared else G * N, 2 * S, 2 * S, Cin).astype(f32)
    x[1::2] = 0.0
    case = f"locnet MFMA S {S} Cin {Cin} G {G} shared {shared} grid {hw[0]}x{hw[1]}"
    check(golden, f"{case} / forward", *locnet_forward_outs(cg, G, N, S, Cin, (1, 1, 1), hw, ts, x, shared))
    check(golden, f"{case} / backward", *locnet_backward_outs(cg, G, N, S, Cin, (1, 1, 1), hw, ts, seed=S + Cin + hw[1]))


@pytest.mark.parametrize("flags", [(1, 1, 1), (1, 0, 0)], ids=["TTT", "TFF"])
def test_affine_entry_points(cg, golden, flags):
    """The four cg_affine_* entry points called directly: five samples, row 1 of the parameters all zero, on grids (5, 12) and (1, 7)
    (H == 1: the n == 1 side of the grid coordinate)."""
    L, st = cg.lib(), cg.tensor.stream()
    N, P = 5, flags[0] + flags[1] + 2 * flags[2]
    rng = np.random.default_rng(70 + P)
    prm = np.concatenate(([rng.uniform(-3.1, 3.1, (N, 1))] if flags[0] else []) + ([rng.uniform(0.3, 2.0, (N, 1))] if flags[1] else [])
                         + ([rng.uniform(-1.0, 1.0, (N, 2))] if flags[2] else []), 1).astype(f32)
    prm[1] = 0.0
    pt, T = dev(prm), out_like(N * 6)
    L.affine_matrix_forward(st, p(pt), p(T), N, *flags)
    res = [T]
    for hw in ((5, 12), (1, 7)):
        grid, gT, gp = out_like(N * hw[0] * hw[1] * 2), out_like(N * 6), out_like(N * P)
        gg = dev(edge_normal(rng, (N, *hw, 2)))
        L.affine_grid_forward(st, p(T), p(grid), N, *hw)
        L.affine_grid_backward(st, p(gg), p(gT), N, *hw)
        L.affine_matrix_backward(st, p(pt), p(gT), p(gp), N, *flags)
        res += [grid, gT, gp]
    check(golden, f"affine entry points flags {flags}", *res)
