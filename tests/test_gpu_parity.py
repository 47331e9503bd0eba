"""GPU parity tests: the HIP path (through the C ABI / the nn module layer) against the CPU oracle on the same
seeded inputs, plus size-independent properties at BASELINE.json's full sizes.

Tolerance (fp32, stated per north_star): both sides are fp32 with different summation orders, so
|d| <= tol * sqrt(K/1024) * max(1, max|ref|) with tol = 2e-5 for single operators (K = reduction length);
whole-network gradients additionally see PReLU-kink sign flips of |x| < 1e-5 activations (see
tests/test_oracle_vs_torch.py) and are checked tight-on-the-bulk / loose-on-the-max.
"""
import importlib

import os

import numpy as np
import pytest
import torch

from helpers import bulk_close, close
from oracle import oracle as O

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def cg():
    mod = importlib.import_module("cat-generator_amd")
    assert torch.cuda.is_available(), "these tests need the MI355X"
    mod.lib()  # fails loudly if the HIP extension is missing
    mod.nn.SpatialConvolution.winograd_min_tiles = 0  # small test shapes must exercise the Winograd kernels too
    return mod


# ------------------------------------------------------------------------------ convolution
CONV_CASES = [
    # N, Cin, H, W, Cout, k, ups
    (2, 3, 8, 8, 5, 3, 0),       # scalar A and B paths, ragged tiles
    (3, 8, 5, 7, 12, 3, 0),      # M = 105: ragged M, non-square
    (4, 16, 16, 16, 16, 3, 0),   # localisation-net conv: K tile straddles taps, (128,32) tile
    (4, 3, 32, 32, 64, 3, 0),    # D conv1 (models.lua:646)
    (2, 64, 16, 16, 64, 3, 0),   # D branch conv
    (2, 64, 16, 16, 128, 5, 0),  # D branch-4 5x5 (models.lua:681)
    (2, 128, 8, 8, 128, 7, 0),   # D branch-4 7x7 (models.lua:685)
    (2, 512, 4, 4, 512, 3, 1),   # G conv1 with folded upsampling (models.lua:205-206), split-K
    (1, 256, 16, 16, 128, 5, 1), # G conv3 (models.lua:217-218)
    (3, 16, 3, 5, 8, 3, 1),      # folded upsampling on a ragged, non-power-of-two grid
    (3, 128, 6, 4, 128, 5, 1),   # Winograd F(2x2,3x3) path (planes % 128, even grid), ragged tile count, borders
    (2, 8, 4, 4, 4, 5, 1),       # 5x5 phases through the generic (Cin % 16 != 0) gather
    (2, 32, 4, 4, 32, 7, 1),     # 7x7 -> 4x4 phase kernels
    (2, 128, 32, 32, 3, 3, 0),   # G conv4, Cout = 3 (models.lua:222)
    (2, 64, 8, 8, 1, 3, 0),      # Cout = 1
]


@pytest.mark.parametrize("N,Cin,H,W,Cout,k,ups", CONV_CASES)
def test_spatial_convolution_fwd_bwd(cg, N, Cin, H, W, Cout, k, ups):
    rs = np.random.RandomState(hash((N, Cin, H, Cout, k)) % 2**31)
    pad = (k - 1) // 2
    m = cg.nn.SpatialConvolution(Cin, Cout, k, k, 1, 1, pad)
    w = (rs.randn(Cout, Cin, k, k) / np.sqrt(Cin * k * k)).astype(f32)
    b = rs.randn(Cout).astype(f32)
    m.weight.copy(w); m.bias.copy(b)
    x = rs.randn(N, Cin, H, W).astype(f32)
    xin = cg.Tensor.from_numpy(x)
    xl = x
    if ups:
        up = cg.nn.SpatialUpSamplingNearest(2)
        xin = up.forward(xin)
        xl = np.repeat(np.repeat(x, 2, axis=2), 2, axis=3)
    Kf = Cin * k * k
    y = m.forward(xin).numpy()
    close(y, O.conv2d_forward(xl, w, b, pad), K=Kf, what="updateOutput")
    dy = rs.randn(*y.shape).astype(f32)
    m.gradWeight.fill(1.0); m.gradBias.fill(1.0)  # accGradParameters must ACCUMULATE
    gi_t = m.backward(xin, cg.Tensor.from_numpy(dy))
    if not ups:
        close(gi_t.numpy(), O.conv2d_backward_data(dy, w, xl.shape, pad), K=Cout * k * k, what="updateGradInput")
    gw, gb = np.ones_like(w), np.ones_like(b)
    O.conv2d_backward_weight(xl, dy, gw, gb, pad)
    P = y.shape[0] * y.shape[2] * y.shape[3]
    close(m.gradWeight.numpy(), gw, K=P, tol=4e-5, what="gradWeight")
    close(m.gradBias.numpy(), gb, K=P, tol=4e-5, what="gradBias")
    if ups:  # the upsampling module's own backward: 2x2 block sum
        g_lo = up.updateGradInput(None, m.gradInput).numpy()
        ref = O.UpSample2().backward(O.conv2d_backward_data(dy, w, xl.shape, pad))
        close(g_lo, ref, K=4 * Cout * k * k, what="upsample backward")


def test_winograd_path_matches_direct_phase_path(cg):
    """csrc/winograd.hip vs the direct phase-folded kernels on G's 5x5 layer shape (models.lua:217-218)."""
    rs = np.random.RandomState(5)
    N, Cin, H, Cout = 4, 256, 16, 128
    x = cg.Tensor.from_numpy(rs.randn(N, Cin, H, H).astype(f32))
    dy = cg.Tensor.from_numpy(rs.randn(N, Cout, 2 * H, 2 * H).astype(f32))
    res = {}
    for wino in (True, False):
        cg.nn.SpatialConvolution.winograd = wino
        try:
            m = cg.nn.SpatialConvolution(Cin, Cout, 5, 5, 1, 1, 2)
            m.weight.copy((np.random.RandomState(6).randn(Cout, Cin, 5, 5) / 80).astype(f32))
            m.bias.copy(np.random.RandomState(7).randn(Cout).astype(f32))
            up = cg.nn.SpatialUpSamplingNearest(2)
            y = m.forward(up.forward(x)).numpy()
            m.gradWeight.zero(); m.gradBias.zero()
            gi = up.updateGradInput(None, m.backward(up.output, dy)).numpy()
            assert bool(getattr(m, "_wino", False)) == wino
            res[wino] = (y, gi, m.gradWeight.numpy(), m.gradBias.numpy())
            if wino:   # the planner's form of the data gradient: K rows in slices over blockIdx.z + fixed-order sum (cg_conv2d_ups2_wino_dgrad_split)
                L, st = cg.lib(), importlib.import_module("cat-generator_amd.tensor").stream()
                npart = L.conv2d_ups2_wino_dgrad_part_floats(N, H, H, Cin, Cout)
                assert npart == 4 * N * H * H * Cin                      # 8 workgroups unsplit: four slices
                dev = m._u_bwd.device
                part = torch.empty(npart, dtype=torch.float32, device=dev)
                vdy = torch.empty(L.conv2d_ups2_wino_v_floats(N, H, H, 4 * Cout), dtype=torch.float32, device=dev)
                dxs = torch.full((N, H, H, Cin), float("nan"), dtype=torch.float32, device=dev)
                dyn = cg.nn.as_nhwc(dy)
                torch.cuda.synchronize()
                assert L.conv2d_ups2_wino_dgrad_split(st, dyn.ptr, m._u_bwd.data_ptr(), dxs.data_ptr(), vdy.data_ptr(), part.data_ptr(), N, H, H, Cin, Cout) == 0
                torch.cuda.synchronize()
                close(dxs.cpu().numpy().transpose(0, 3, 1, 2), gi, K=4 * Cout * 9, what="winograd data gradient in K slices vs unsplit")
        finally:
            cg.nn.SpatialConvolution.winograd = True
    for a, b, K, what in zip(res[True], res[False], (Cin * 9, 4 * Cout * 9, N * 4 * H * H, N * 4 * H * H),
                             ("output", "gradInput", "gradWeight", "gradBias")):
        close(a, b, K=K, what=f"winograd vs direct: {what}")


@pytest.mark.parametrize("N,Cin,H,Cout", [(2, 128, 8, 128), (3, 256, 6, 128), (32, 512, 8, 256), (64, 512, 16, 128)])
def test_winograd22_of_the_3x3_layers_behind_an_upsampling(cg, N, Cin, H, Cout):
    """F(2x2,2x2) forward and data gradient (cg_conv2d_ups2_wino22_*, csrc/winograd.hip; models.lua:211-212) through the C ABI against the ORACLE's
    upsample -> conv3x3 and against the phase-folded direct kernel, incl. the batch-norm statistics partials of the epilogue and the
    borders (zero padding on the low-res grid) - the third case is G's 512 -> 256 layer at a quarter of the benchmarked batch.  The
    planned pass takes this path at >= 2048 tiles (whole-generator tests at batch 128 run it inside G).  The data gradient splits its
    K slices over blockIdx.z below one workgroup per CU (the first three cases) and runs unsplit above (the last one, checked against
    the phase-folded kernel only: its own parity with the oracle is test_conv_fwd_bwd's)."""
    big = N * H * H * Cin * Cout >= 1 << 30
    tensor_mod = importlib.import_module("cat-generator_amd.tensor")
    rs = np.random.RandomState(N + Cin)
    L, st = cg.lib(), tensor_mod.stream()
    xl = rs.randn(N, Cin, H, H).astype(f32)
    w = (rs.randn(Cout, Cin, 3, 3) / np.sqrt(Cin * 9)).astype(f32); bias = rs.randn(Cout).astype(f32)
    m = cg.nn.SpatialConvolution(Cin, Cout, 3, 3, 1, 1, 1)
    m.weight.copy(w); m.bias.copy(bias)
    up = cg.nn.SpatialUpSamplingNearest(2)
    y_direct = m.forward(up.forward(cg.Tensor.from_numpy(xl))).numpy()       # packs m._wf_ph (the phase-summed kernels)
    assert L.conv2d_ups2_wino22_supported(N, H, H, Cin, Cout) == 1
    dev = m._wf_ph.device
    u22 = torch.empty(L.conv2d_ups2_wino22_u_floats(Cin, Cout), dtype=torch.float32, device=dev)
    u22b = torch.empty_like(u22)
    assert L.conv2d_ups2_wino22_pack(st, m._wf_ph.data_ptr(), m._wb_ph.data_ptr(), u22.data_ptr(), u22b.data_ptr(), Cout, Cin) == 0
    v = torch.empty(L.conv2d_ups2_wino22_v_floats(N, H, H, Cin), dtype=torch.float32, device=dev)
    x_lo = torch.from_numpy(np.ascontiguousarray(xl.transpose(0, 2, 3, 1))).to(dev)        # NHWC low-res map
    y = torch.full((N, 2 * H, 2 * H, Cout), float("nan"), dtype=torch.float32, device=dev)
    rows = L.conv2d_ups2_wino_stats_rows(N, H, H, Cin, Cout)
    part = torch.zeros((max(rows, 1), 2, Cout), dtype=torch.float32, device=dev)
    b_dev = torch.from_numpy(bias).to(dev)
    torch.cuda.synchronize()           # the torch-side fills above ran on torch's stream, the launch below on the library's
    assert L.conv2d_ups2_wino22_forward_stats(st, x_lo.data_ptr(), u22.data_ptr(), b_dev.data_ptr(), y.data_ptr(), v.data_ptr(),
                                              N, H, H, Cin, Cout, part.data_ptr() if rows else None) == 0
    torch.cuda.synchronize()
    got = y.cpu().numpy().transpose(0, 3, 1, 2)
    ref = y_direct if big else O.conv2d_forward(O.UpSample2().forward(xl), w, bias, 1)
    close(got, ref, K=Cin * 9, what="F(2x2,2x2) forward vs oracle")
    close(got, y_direct, K=Cin * 9, what="F(2x2,2x2) forward vs the phase-folded kernel")
    if rows:
        p_ = part.cpu().numpy().astype(np.float64)
        close(p_[:, 0].sum(0), ref.astype(np.float64).sum((0, 2, 3)), K=N * 4 * H * H, tol=5e-5, what="epilogue sum")
        close(p_[:, 1].sum(0), (ref.astype(np.float64) ** 2).sum((0, 2, 3)), K=N * 4 * H * H, tol=5e-5, what="epilogue sum of squares")
    # updateGradInput in the same form: the four phase sub-lattices of dy side by side along K, flipped kernels (cg_conv2d_ups2_wino22_dgrad)
    dy = rs.randn(N, Cout, 2 * H, 2 * H).astype(f32)
    gi_direct = up.updateGradInput(None, m.updateGradInput(up.output, cg.Tensor.from_numpy(dy))).numpy()
    dy_dev = torch.from_numpy(np.ascontiguousarray(dy.transpose(0, 2, 3, 1))).to(dev)
    vdy = torch.empty(L.conv2d_ups2_wino22_dgrad_v_floats(N, H, H, Cin, Cout), dtype=torch.float32, device=dev)
    dx = torch.full((N, H, H, Cin), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    assert L.conv2d_ups2_wino22_dgrad(st, dy_dev.data_ptr(), u22b.data_ptr(), dx.data_ptr(), vdy.data_ptr(), N, H, H, Cin, Cout) == 0
    torch.cuda.synchronize()
    assert (L.conv2d_ups2_wino22_dgrad_v_floats(N, H, H, Cin, Cout) > 36 * N * (H // 2) ** 2 * Cout) == (not big)    # split / unsplit
    gref = gi_direct if big else O.UpSample2().backward(O.conv2d_backward_data(dy, w, (N, Cin, 2 * H, 2 * H), 1))
    close(dx.cpu().numpy().transpose(0, 3, 1, 2), gref, K=4 * Cout * 9, what="F(2x2,2x2) data gradient vs oracle")
    close(dx.cpu().numpy().transpose(0, 3, 1, 2), gi_direct, K=4 * Cout * 9, what="F(2x2,2x2) data gradient vs the phase-folded kernel")


@pytest.mark.parametrize("N,i,o", [(128, 100, 8192), (6, 20480, 256), (5, 64, 4), (3, 256, 1), (64, 1024, 64)])
def test_linear_fwd_bwd(cg, N, i, o):
    rs = np.random.RandomState(N + i + o)
    m = cg.nn.Linear(i, o)
    w = (rs.randn(o, i) / np.sqrt(i)).astype(f32); b = rs.randn(o).astype(f32)
    m.weight.copy(w); m.bias.copy(b)
    x = rs.randn(N, i).astype(f32); dy = rs.randn(N, o).astype(f32)
    close(m.forward(cg.Tensor.from_numpy(x)).numpy(), O.linear_forward(x, w, b), K=i, what="forward")
    m.gradWeight.zero(); m.gradBias.zero()
    gi = m.backward(cg.Tensor.from_numpy(x), cg.Tensor.from_numpy(dy)).numpy()
    close(gi, O.linear_backward_data(dy, w), K=o, what="gradInput")
    gw, gb = np.zeros_like(w), np.zeros_like(b)
    O.linear_backward_weight(x, dy, gw, gb)
    close(m.gradWeight.numpy(), gw, K=N, what="gradWeight"); close(m.gradBias.numpy(), gb, K=N, what="gradBias")


def test_conv_upsample_layer_is_a_view(cg):
    """layers/SpatialConvolutionUpsample.lua:16-24: NCHW buffer [N,nOut*f^2,h,w] reinterpreted, not pixel-shuffled."""
    rs = np.random.RandomState(0)
    m = cg.nn.SpatialConvolutionUpsample(4, 3, 3, 3, 2)
    w, b = m.weight.numpy(), m.bias.numpy()
    x = rs.randn(2, 4, 5, 5).astype(f32)
    y = m.forward(cg.Tensor.from_numpy(x)).numpy()
    ref = O.conv2d_forward(x, w, b, 1).reshape(2, 3, 10, 10)
    close(y, ref, K=36)
    dy = rs.randn(2, 3, 10, 10).astype(f32)
    gi = m.backward(cg.Tensor.from_numpy(x), cg.Tensor.from_numpy(dy, fmt="plain")).numpy()
    close(gi, O.conv2d_backward_data(dy.reshape(2, 12, 5, 5), w, x.shape, 1), K=108)


# ------------------------------------------------------------------------ memory-bound operators
def test_activations_and_bce(cg):
    rs = np.random.RandomState(1)
    x = rs.randn(3, 8, 6, 6).astype(f32); dy = rs.randn(3, 8, 6, 6).astype(f32)
    x[0, 0, 0, 0] = 0.0
    for P, Oc in ((cg.nn.PReLU(), O.PReLU()), (cg.nn.LeakyReLU(), O.LeakyReLU()), (cg.nn.Sigmoid(), O.Sigmoid())):
        yo = Oc.forward(x); go = Oc.backward(dy)
        xin = cg.Tensor.from_numpy(x)
        close(P.forward(xin).numpy(), yo, tol=1e-6, what=type(Oc).__name__)
        close(P.backward(xin, cg.Tensor.from_numpy(dy)).numpy(), go, tol=1e-6, what=type(Oc).__name__ + " bwd")
        if isinstance(Oc, O.PReLU):
            close(P.gradWeight.numpy(), Oc.grad_weight, K=x.size, what="dalpha")
    p = rs.rand(16, 1).astype(f32) * 0.98 + 0.01; t = (rs.rand(16) > 0.5).astype(f32)
    crit = cg.nn.BCECriterion()
    f = float(crit.forward(cg.Tensor.from_numpy(p), cg.Tensor.from_numpy(t)))
    assert abs(f - O.bce_forward(p, t)) < 1e-6
    close(crit.backward(cg.Tensor.from_numpy(p), cg.Tensor.from_numpy(t)).numpy(), O.bce_backward(p, t.reshape(16, 1)), tol=1e-6)


@pytest.mark.parametrize("N,C,H", [(4, 16, 8), (8, 128, 16), (3, 70, 5)])
def test_batchnorm_train(cg, N, C, H):
    rs = np.random.RandomState(C)
    x = (rs.randn(N, C, H, H) * 1.5 + 0.7).astype(f32); dy = rs.randn(N, C, H, H).astype(f32)
    P, Oc = cg.nn.SpatialBatchNormalization(C), O.SBN(C, O.RNG(3))
    Oc.weight[...] = P.weight.numpy(); Oc.bias[...] = rs.randn(C).astype(f32); P.bias.copy(Oc.bias)
    xin = cg.Tensor.from_numpy(x)
    close(P.forward(xin).numpy(), Oc.forward(x), tol=2e-5, what="bn fwd")
    close(P.running_mean.numpy(), Oc.running_mean, tol=1e-6); close(P.running_var.numpy(), Oc.running_var, tol=1e-5)
    gi = P.backward(xin, cg.Tensor.from_numpy(dy)).numpy()
    close(gi, Oc.backward(dy), tol=5e-5, what="bn bwd")
    close(P.gradWeight.numpy(), Oc.grad_weight, K=N * H * H, what="dgamma")
    close(P.gradBias.numpy(), Oc.grad_bias, K=N * H * H, what="dbeta")
    P.evaluate(); Oc.train = False
    close(P.forward(xin).numpy(), Oc.forward(x), tol=2e-5, what="bn eval")


def test_pooling_upsample_layout(cg):
    rs = np.random.RandomState(2)
    x = rs.randn(3, 10, 8, 12).astype(f32)
    for P, Oc in ((cg.nn.SpatialAveragePooling(2, 2, 2, 2), O.AvgPool2()), (cg.nn.SpatialMaxPooling(2, 2), O.MaxPool2())):
        xin = cg.Tensor.from_numpy(x)
        yo = Oc.forward(x); g = rs.randn(*yo.shape).astype(f32)
        close(P.forward(xin).numpy(), yo, tol=1e-6)
        close(P.backward(xin, cg.Tensor.from_numpy(g)).numpy(), Oc.backward(g), tol=1e-6)
    up = cg.nn.SpatialUpSamplingNearest(2)
    close(cg.nn.materialise(up.forward(cg.Tensor.from_numpy(x))).numpy(), O.UpSample2().forward(x), tol=0)
    # View: the NCHW reinterpretation must survive NHWC storage (models.lua:202, :696)
    v = cg.nn.View(10, 8, 12); flat = x.reshape(3, -1)
    t = v.forward(cg.Tensor.from_numpy(flat))
    assert t.fmt == "nhwc"; close(t.numpy(), x, tol=0)
    close(v.backward(None, t).numpy(), flat, tol=0)
    v2 = cg.nn.View(10 * 8 * 12)
    close(v2.forward(cg.Tensor.from_numpy(x)).numpy(), flat, tol=0)


def test_dropout_masks_share_the_counter_stream(cg):
    cg.manual_seed(11); rng = O.RNG(11)
    x4 = np.random.RandomState(3).randn(6, 20, 4, 4).astype(f32)
    x2 = np.random.RandomState(4).randn(6, 256).astype(f32)  # nn.Dropout sits on the [N,256] head (models.lua:699)
    for P, Oc in ((cg.nn.SpatialDropout(0.2), O.SpatialDropout(0.2, rng)), (cg.nn.Dropout(), O.Dropout(0.5, rng)),
                  (cg.nn.SpatialDropout(), O.SpatialDropout(0.5, rng))):
        x = x2 if isinstance(Oc, O.Dropout) else x4
        xin = cg.Tensor.from_numpy(x)
        close(P.forward(xin).numpy(), Oc.forward(x), tol=0, what="mask")
        close(P.backward(xin, xin).numpy(), Oc.backward(x), tol=0)
    P.evaluate(); Oc.train = False
    close(P.forward(cg.Tensor.from_numpy(x)).numpy(), Oc.forward(x), tol=1e-7)


@pytest.mark.parametrize("size,ch,rot,scale,trans", [(16, 8, True, True, True), (32, 3, True, False, False), (16, 64, True, True, True),
                                                      (64, 3, True, False, False), (32, 64, True, True, True)])
def test_spatial_transformer_module(cg, size, ch, rot, scale, trans):
    """createSpatialTransformer (models.lua:814-906) end to end, with a non-identity classifier, at the shapes D32_st3 uses at
    32x32 and 64x64 (first transformer: C planes at full size, rotation only; branch transformers: 64 planes at half size).  The
    planned pass runs the localisation branch as cg_locnet_forward / _backward (csrc/locnet.hip) and its weight gradients on the
    GEMM path; CG_FUSE_LOCNET=0 / the per-module walk run the ten modules."""
    cg.manual_seed(5); rng = O.RNG(5)
    P = cg.models.createSpatialTransformer(rot, scale, trans, size, ch, False)
    Oc = O.SpatialTransformer(rot, scale, trans, size, ch, rng)
    rs = np.random.RandomState(4)
    nP = int(rot) + int(scale) + 2 * int(trans)
    wcls = (rs.randn(nP, 64) * 0.05).astype(f32)
    P.modules[0].modules[1].modules[0].modules[-1].weight.copy(wcls)
    Oc.loc.mods[-1].weight[...] = wcls
    for (pp, _), po in zip(Oc.parameters(), P.parameters()[0]):
        np.testing.assert_array_equal(pp, po.numpy())
    x = rs.rand(5, ch, size, size).astype(f32); dy = rs.randn(5, ch, size, size).astype(f32)
    xin = cg.Tensor.from_numpy(x)
    close(P.forward(xin).numpy(), Oc.forward(x), tol=3e-5, what="st fwd")
    assert P._planned_last
    names = {type(m).__name__ for m in P.listModules()}
    assert "AffineGridGeneratorBHWD" in names
    P.zeroGradParameters()
    gi = P.backward(xin, cg.Tensor.from_numpy(dy)).numpy()
    go = Oc.backward(dy)
    close(gi, go, K=4096, tol=5e-5, what="st gradInput")
    for (_, go_), gp in zip(Oc.parameters(), P.parameters()[1]):
        bulk_close(gp.numpy(), go_, max_rel=2e-3, mean_rel=2e-4, what="st param grad")
    if (size, ch) != (16, 8):
        return
    # identity initialisation reproduces the input exactly (models.lua:859-860)
    P2 = cg.models.createSpatialTransformer(True, False, False, 32, 3, False)
    x2 = rs.rand(2, 3, 32, 32).astype(f32)
    close(P2.forward(cg.Tensor.from_numpy(x2)).numpy(), x2, tol=1e-6)


@pytest.mark.parametrize("C,H", [(64, 16), (3, 32), (6, 8)])
def test_shared_image_sampler_equals_one_launch_per_branch(cg, C, H):
    """cg_bilinear_sampler_{forward,backward}_shared (G sibling transformers on the same images, one launch) against G plain
    calls - bit for bit (the backward is the deterministic gather form) - and the plain forward against the oracle, for
    the float4 (C % 4 == 0) and the scalar kernels; grids reach outside [-1, 1]."""
    rs = np.random.RandomState(C)
    N, G = 5, 3
    img = rs.randn(N, H, H, C).astype(f32)
    grid = (rs.rand(G * N, H, H, 2) * 2.6 - 1.3).astype(f32)
    gout = rs.randn(G * N, H, H, C).astype(f32)
    L, st = cg.lib(), cg.tensor.stream()
    T = lambda a: cg.Tensor.from_numpy(a, "plain")
    ti, tg, to = T(img), T(grid), T(gout)
    out = cg.Tensor.empty((G * N, H, H, C)); gimg = cg.Tensor.empty((G * N, H, H, C)); ggrid = cg.Tensor.empty((G * N, H, H, 2))
    L.bilinear_sampler_forward_shared(st, G, ti.ptr, tg.ptr, out.ptr, N, H, H, C, H, H)
    L.bilinear_sampler_backward_shared(st, G, ti.ptr, tg.ptr, to.ptr, gimg.ptr, ggrid.ptr, N, H, H, C, H, H)
    o_s, gi_s, gg_s = out.numpy(), gimg.numpy(), ggrid.numpy()
    for b in range(G):
        sl = slice(b * N, (b + 1) * N)
        tgb, tob = T(grid[sl]), T(gout[sl])
        o1 = cg.Tensor.empty((N, H, H, C)); gi1 = cg.Tensor.empty((N, H, H, C)); gg1 = cg.Tensor.empty((N, H, H, 2))
        L.bilinear_sampler_forward(st, ti.ptr, tgb.ptr, o1.ptr, N, H, H, C, H, H)
        L.bilinear_sampler_backward(st, ti.ptr, tgb.ptr, tob.ptr, gi1.ptr, gg1.ptr, N, H, H, C, H, H)
        np.testing.assert_array_equal(o_s[sl], o1.numpy())
        np.testing.assert_array_equal(gi_s[sl], gi1.numpy())
        np.testing.assert_array_equal(gg_s[sl], gg1.numpy())
        close(o1.numpy(), O.bilinear_forward(img, grid[sl]), tol=2e-6, what="sampler forward")
        gi_o, gg_o = O.bilinear_backward(img, grid[sl], gout[sl])
        close(gi1.numpy(), gi_o, K=16, tol=1e-5, what="sampler gradInput")
        close(gg1.numpy(), gg_o, K=C, tol=2e-5, what="sampler gradGrid")


@pytest.mark.parametrize("C,H", [(64, 16), (3, 32)])
@pytest.mark.parametrize("scale", [0.0, 0.01, 0.1])
def test_sampler_backward_under_a_collapsed_transformer(cg, C, H, scale):
    """A localisation net that collapses (scale -> 0) maps every output pixel into ONE source cell: up to H*W taps in one bucket of the
    deterministic gather backward (csrc/sampler.hip, bilinear_bwd_det_k).  Round 6 found the step 40 % slower for 25 iterations of a long run
    because of it (a single thread insertion-sorted the bucket, one lane group summed it: 2-8 ms instead of 11-28 us): buckets are now
    ordered by rank in parallel and pixels with more than 64 taps are summed by the whole workgroup in a fixed order.  Against the oracle's
    scatter, twice (bit-equal: the order is fixed), and bounded in time."""
    import time
    rs = np.random.RandomState(7)
    N = 16
    img = rs.randn(N, H, H, C).astype(f32)
    ys, xs = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, H), indexing="ij")
    grid = (np.stack([ys, xs], -1)[None].repeat(N, 0) * scale + rs.uniform(-0.3, 0.3, (N, 1, 1, 2))).astype(f32)
    gout = rs.randn(N, H, H, C).astype(f32)
    L, st = cg.lib(), cg.tensor.stream()
    T = lambda a: cg.Tensor.from_numpy(a, "plain")
    ti, tg, to = T(img), T(grid), T(gout)
    runs = []
    for _ in range(2):
        gi, gg = cg.Tensor.empty((N, H, H, C)), cg.Tensor.empty((N, H, H, 2))
        L.bilinear_sampler_backward(st, ti.ptr, tg.ptr, to.ptr, gi.ptr, gg.ptr, N, H, H, C, H, H)
        runs.append((gi.numpy().copy(), gg.numpy().copy()))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    gi_o, gg_o = O.bilinear_backward(img, grid, gout)
    close(runs[0][0], gi_o, K=H * H, tol=1e-5, what="sampler gradInput, collapsed grid")       # up to H*W taps meet in one pixel
    close(runs[0][1], gg_o, K=C, tol=2e-5, what="sampler gradGrid, collapsed grid")
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        L.bilinear_sampler_backward(st, ti.ptr, tg.ptr, to.ptr, gi.ptr, gg.ptr, N, H, H, C, H, H)
    torch.cuda.synchronize()
    assert (time.perf_counter() - t0) / 5 < 1.5e-3, "the collapsed-grid backward is slow again"


def test_adam_and_fused_penalty_clamp(cg):
    rs = np.random.RandomState(6)
    n = 100003
    p0 = rs.randn(n).astype(f32); st_o = {}
    x = cg.Tensor.from_numpy(p0.copy()); st_p = {}
    po = p0.copy()
    for it in range(3):
        g = (rs.randn(n) * 3).astype(f32)
        go = g + f32(1e-4) * po
        np.clip(go, -1, 1, out=go)
        O.adam(po, go.astype(f32), st_o)
        gt = cg.Tensor.from_numpy(g)
        cg.optim.adam(lambda _: (0.0, gt), x, st_p, fused=dict(l1=0.0, l2=1e-4, clamp=1.0))
        close(gt.numpy(), go, tol=1e-6, what="clamped grad written back")
    close(x.numpy(), po, tol=2e-6, what="adam params")
    close(st_p["m"].numpy(), st_o["m"], tol=1e-6); close(st_p["v"].numpy(), st_o["v"], tol=1e-6)


def test_sgd_and_adagrad(cg):
    rs = np.random.RandomState(8)
    n = 50001
    for name in ("sgd", "sgd_mom", "adagrad"):
        p0 = rs.randn(n).astype(f32); po = p0.copy(); st_o, st_p = {}, {}
        x = cg.Tensor.from_numpy(p0.copy())
        for it in range(3):
            g = rs.randn(n).astype(f32)
            gt = cg.Tensor.from_numpy(g)
            if name == "adagrad":
                O.adagrad(po, g, st_o, lr=1e-3); cg.optim.adagrad(lambda _: (0.0, gt), x, {"learningRate": 1e-3}, st_p)
            else:
                mom = 0.9 if name == "sgd_mom" else 0.0
                O.sgd(po, g, st_o, lr=0.02, momentum=mom)
                cg.optim.sgd(lambda _: (0.0, gt), x, {"learningRate": 0.02, "momentum": mom}, st_p)
        close(x.numpy(), po, tol=2e-6, what=name)


# ------------------------------------------------------------------------------ whole networks
def _pair(cg, seed, which, size=32, ch=3):
    cg.manual_seed(seed); rng = O.RNG(seed)
    if which == "G":
        return cg.models.create_G((ch, size, size), 100), O.create_G32up_c(ch, 100, rng), rng
    if which == "G32up":
        return cg.models.create_G_decoder_upsampling32((ch, size, size), 100), O.create_G32up(ch, 100, rng), rng
    return cg.models.create_D((ch, size, size)), O.create_D32_st3(ch, size, rng), rng


@pytest.mark.parametrize("which,ch", [("G", 3), ("G32up", 1)])
def test_generator_forward_backward(cg, which, ch):
    P, Oc, _ = _pair(cg, 21, which, ch=ch)
    pP, gP = P.getParameters(); pO, gO = O.get_parameters(Oc)
    np.testing.assert_array_equal(pP.numpy(), pO)
    rs = np.random.RandomState(7)
    z = (rs.rand(6, 100) * 2 - 1).astype(f32); dy = (rs.randn(6, ch, 32, 32) * 0.1).astype(f32)
    zin = cg.Tensor.from_numpy(z)
    close(P.forward(zin).numpy(), Oc.forward(z), tol=5e-5, what="G forward")
    P.backward(zin, cg.Tensor.from_numpy(dy)); Oc.backward(dy)
    off = 0
    for p_, _ in Oc.parameters():
        a, b = gP.numpy()[off:off + p_.size], gO[off:off + p_.size]
        off += p_.size
        scale = max(np.abs(b).max(), 1e-4 * np.abs(gO).max())
        d = np.abs(a - b)
        assert d.max() <= 3e-2 * scale and (a.size == 1 or d.mean() <= 2e-3 * scale), (p_.shape, d.max(), scale)


def test_discriminator_forward_backward(cg):
    P, Oc, rng = _pair(cg, 22, "D")
    pP, gP = P.getParameters(); pO, gO = O.get_parameters(Oc)
    np.testing.assert_array_equal(pP.numpy(), pO)
    # make the spatial transformers do something: perturb their (zero-initialised) classifiers identically
    rs = np.random.RandomState(8)
    bump = (rs.randn(pO.size) * 0.01).astype(f32)
    pO += bump; pP.copy(pO)
    x = rs.rand(6, 3, 32, 32).astype(f32); t = np.array([1, 1, 1, 0, 0, 0], f32)
    xin = cg.Tensor.from_numpy(x)
    out_p = P.forward(xin).numpy(); out_o = Oc.forward(x)
    close(out_p, out_o, tol=5e-5, what="D forward")
    g = O.bce_backward(out_o, t.reshape(out_o.shape))
    gi_p = P.backward(xin, cg.Tensor.from_numpy(g)).numpy(); gi_o = Oc.backward(g)
    bulk_close(gi_p, gi_o, what="D gradInput")
    bulk_close(gP.numpy(), gO, what="D flat gradient")


@pytest.mark.parametrize("fused", [True, False])
def test_three_training_steps(cg, fused):
    """adversarial.lua:51-275 x3 against the oracle Trainer on identical real batches / noise / masks."""
    seed, N = 31, 8
    cg.manual_seed(seed); rng = O.RNG(seed)
    G, D = cg.models.create_G((3, 32, 32), 100), cg.models.create_D((3, 32, 32))
    Go, Do = O.create_G32up_c(3, 100, rng), O.create_D32_st3(3, 32, rng)
    S = cg.adversarial.State(dict(batchSize=N, fused_update=fused), G, D)
    S.keep_outputs = True
    T = O.Trainer(Go, Do)
    np.testing.assert_array_equal(S.PARAMETERS_D.numpy(), T.pD)
    rs = np.random.RandomState(9)
    pool = rs.rand(32, 3, 32, 32).astype(f32)
    data = cg.adversarial.TrainData(pool)
    for step in range(3):
        idx = rs.randint(0, 32, size=N // 2)
        nd = (rs.rand(N // 2, 100) * 2 - 1).astype(f32); ng = (rs.rand(N, 100) * 2 - 1).astype(f32)
        cg.adversarial.iteration(S, data, N, real_idx=idx, noise_D=nd, noise_G=ng)
        r = T.step(pool[idx], nd, ng)
        # step 0 sees identical parameters; later steps inherit Adam's +-lr sign flips on ~0 gradients
        # (a handful of weights differ by 2e-3), which shows up at the 1e-3 level in images / D outputs
        close(S._last_fake.numpy(), r["fake"], tol=2e-4 if step == 0 else 4e-2, what=f"step {step} fake images")
        close(cg.nn.as_plain(S._last["outputs_D"]).numpy(), r["outD"], tol=5e-4 if step == 0 else 5e-2,
              what=f"step {step} D outputs")
        assert abs(float(S._last["f_G"]) - r["fG"]) < 5e-3
        lr = 1e-3
        for name, a, b in (("pD", S.PARAMETERS_D.numpy(), T.pD), ("pG", S.PARAMETERS_G.numpy(), T.pG)):
            d = np.abs(a - b)
            print(f"[drift] fused={fused} {name} step {step}: max {d.max():.2e} mean {d.mean():.2e} frac>1e-4 {np.mean(d > 1e-4):.2e}")
            assert d.max() <= 2.5 * lr * (step + 1), f"{name} step {step}: max drift {d.max():.2e}"
            assert d.mean() <= 4e-5 * (step + 1), f"{name} step {step}: mean drift {d.mean():.2e}"
            # Adam's first update is lr*sign(g): the outlier count measures sign flips of near-zero gradients and is
            # chaotic in the rounding order (measured: changing only the split-K partition, per-layer results equal to
            # the last ulp, moves pG step 0 between 1e-5 and 1.4e-2), so it is a loose bound; max and mean are the checks
            assert np.mean(d > 1e-4) < 5e-2 * (step + 1), f"{name} step {step}: {np.mean(d > 1e-4):.2e} outliers"


@pytest.mark.parametrize("cfg", ["G32up-y-32", "G32up-c-64"])
def test_other_baseline_configs_one_step(cg, cfg):
    """BASELINE.json configs[2] (G32up, grayscale) and configs[4] (G32up-c scaled to 64x64, D32_st3 at 64x64):
    one full D+G update against the oracle at a small batch."""
    seed, N = 51, 4
    cg.manual_seed(seed); rng = O.RNG(seed)
    if cfg == "G32up-y-32":
        ch, size = 1, 32
        G = cg.models.create_G_decoder_upsampling32((ch, size, size), 100); Go = O.create_G32up(ch, 100, rng)
    else:
        ch, size = 3, 64
        G = cg.models.create_G((ch, size, size), 100); Go = O.create_G32up_c(ch, 100, rng, base=8)
    D = cg.models.create_D((ch, size, size)); Do = O.create_D32_st3(ch, size, rng)
    S = cg.adversarial.State(dict(batchSize=N), G, D); S.keep_outputs = True
    T = O.Trainer(Go, Do)
    np.testing.assert_array_equal(S.PARAMETERS_G.numpy(), T.pG)
    np.testing.assert_array_equal(S.PARAMETERS_D.numpy(), T.pD)
    rs = np.random.RandomState(3)
    pool = rs.rand(8, ch, size, size).astype(f32)
    idx = rs.randint(0, 8, size=N // 2)
    nd = (rs.rand(N // 2, 100) * 2 - 1).astype(f32); ng = (rs.rand(N, 100) * 2 - 1).astype(f32)
    cg.adversarial.iteration(S, cg.adversarial.TrainData(pool), N, real_idx=idx, noise_D=nd, noise_G=ng)
    r = T.step(pool[idx], nd, ng)
    close(S._last_fake.numpy(), r["fake"], tol=2e-4, what="fake images")
    close(cg.nn.as_plain(S._last["outputs_D"]).numpy(), r["outD"], tol=5e-4, what="D outputs")
    for name, a, b in (("pD", S.PARAMETERS_D.numpy(), T.pD), ("pG", S.PARAMETERS_G.numpy(), T.pG)):
        d = np.abs(a - b)
        assert d.max() <= 2.5e-3 and d.mean() <= 2e-5, (name, d.max(), d.mean())


# ------------------------------------------------- size-independent properties at BASELINE sizes
def test_conv_adjoint_identity_at_full_size(cg):
    """<conv(x;w), dy> = <x_up, dgrad(dy;w)> = <w, wgrad(x,dy)> for the dominant layer at config #2's size
    (conv 5x5 256->128 on 128 x 16x16 upsampled to 32x32; models.lua:217-218)."""
    N = 128
    m = cg.nn.SpatialConvolution(256, 128, 5, 5, 1, 1, 2)
    m.bias.zero()
    g = torch.Generator(device="cuda").manual_seed(0)
    x = cg.Tensor(torch.randn(N * 16 * 16 * 256, device="cuda", generator=g), (N, 256, 16, 16), "nhwc")
    dy = cg.Tensor(torch.randn(N * 32 * 32 * 128, device="cuda", generator=g), (N, 128, 32, 32), "nhwc")
    up = cg.nn.SpatialUpSamplingNearest(2)
    xin = up.forward(x)
    y = m.forward(xin)
    m.gradWeight.zero(); m.gradBias.zero()
    gi_hi = m.backward(xin, dy)
    gi_lo = up.updateGradInput(x, gi_hi)
    a = torch.dot(y.t.double(), dy.t.double()).item()
    b = torch.dot(x.t.double(), gi_lo.t.double()).item()
    c = torch.dot(m.weight.t.reshape(-1).double(), m.gradWeight.t.reshape(-1).double()).item()
    assert abs(a - b) <= 1e-5 * abs(a) + 1e-2, (a, b)
    assert abs(a - c) <= 1e-5 * abs(a) + 1e-2, (a, c)
    # linearity: conv(2x) = 2 conv(x) exactly (power-of-two scaling commutes with fp32 rounding)
    y1 = y.t.clone()
    x.t.mul_(2.0)
    y2 = m.forward(up.forward(x))
    assert torch.equal(y2.t, 2 * y1)


def test_full_batch_step_runs_and_stays_finite(cg):
    """Config #2 (batch 128) for two iterations: finite parameters, D output in (0,1), Adam state advanced."""
    cg.manual_seed(1)
    G, D = cg.models.create_G((3, 32, 32), 100), cg.models.create_D((3, 32, 32))
    S = cg.adversarial.State(dict(batchSize=128), G, D)
    pool = np.random.RandomState(0).rand(256, 3, 32, 32).astype(f32)
    data = cg.adversarial.TrainData(pool)
    p0 = S.PARAMETERS_G.numpy().copy()
    for _ in range(2):
        cg.adversarial.iteration(S, data)
    torch.cuda.synchronize()
    pg, pd = S.PARAMETERS_G.numpy(), S.PARAMETERS_D.numpy()
    assert np.isfinite(pg).all() and np.isfinite(pd).all()
    assert S.OPTSTATE["adam"]["G"]["t"] == 2 and S.OPTSTATE["adam"]["D"]["t"] == 2
    d = np.abs(pg - p0)
    assert 0 < d.max() <= 2.1e-3  # |step| <= lr per Adam update at t<=2 (bias-corrected), two updates
    out = cg.nn.as_plain(S._last["outputs_D"]).numpy()
    assert out.shape == (128, 1) and (out > 0).all() and (out < 1).all()
    S.CONFUSION.updateValids()
    assert S.CONFUSION.counts.sum().item() == 256


def test_both_generator_forwards_side_by_side_are_result_neutral(cg):
    """OPT.concurrent_g_both (both generator forwards of an iteration side by side from its head - adversarial.lua:232-233 and :185 read the
    same G parameters; since round 6 ONE call below the ABI, cg_net_forward_pair / cg_net_pair_join) is a schedule, not arithmetic - WITHOUT
    injecting anything: the G-step's noise is drawn ahead of time at the position it has in the reference's order (behind the D-step's
    dropout masks), the second pass defers its batch-norm running statistics and the library moves them behind the fake-image pass's.  Four iterations (the first one
    runs one after the other either way: D's draw count is learned there) give the same bits in the parameters of G and D, in the
    running statistics and in the position of the counter stream."""
    N = 16

    def run(both):
        cg.manual_seed(47)
        G, D = cg.models.create_G((3, 32, 32), 100), cg.models.create_D((3, 32, 32))
        S = cg.adversarial.State(dict(batchSize=N, concurrent_g_both=both, seed=3), G, D)
        data = cg.adversarial.TrainData(np.random.RandomState(6).rand(64, 3, 32, 32).astype(f32))
        for _ in range(4):
            cg.adversarial.iteration(S, data, N)
        torch.cuda.synchronize()
        bns = [m for m in G.listModules() if type(m).__name__ == "SpatialBatchNormalization"]
        assert len(bns) == 3
        used = bool(getattr(S, "_d_draws", None)) and both
        return (S.PARAMETERS_G.numpy(), S.PARAMETERS_D.numpy(), [b.running_mean.numpy() for b in bns], [b.running_var.numpy() for b in bns],
                cg.tensor.rng().offset, used)
    g0, d0, rm0, rv0, o0, _ = run(False)
    g1, d1, rm1, rv1, o1, used = run(True)
    assert used and o0 == o1
    np.testing.assert_array_equal(g0, g1)
    np.testing.assert_array_equal(d0, d1)
    for a, b in zip(rm0 + rv0, rm1 + rv1):
        np.testing.assert_array_equal(a, b)


def test_graph_replay_matches_eager(cg):
    """hipGraph replay of the iteration vs eager launches: same parameters (to drift tolerance) after 3 steps (device-side RNG/Adam
    counters make the replay advance its mask / noise / index streams and step counts exactly like eager mode)."""
    def run(graph):
        cg.manual_seed(41)
        G, D = cg.models.create_G((3, 32, 32), 100), cg.models.create_D((3, 32, 32))
        S = cg.adversarial.State(dict(batchSize=16), G, D)
        pool = np.random.RandomState(5).rand(64, 3, 32, 32).astype(f32)
        data = cg.adversarial.TrainData(pool)
        if graph:
            it = cg.adversarial.GraphedIteration(S, data, 16, warmup=2)   # 2 eager steps
            it()                                                          # + 1 replayed
        else:
            S.device_rng = True
            for k in ("D", "G"):
                S.OPTSTATE["adam"][k]["device_step"] = True
            r = cg.tensor.rng(); r.enable_device_base()
            for _ in range(3):
                off0 = r.offset
                cg.adversarial.iteration(S, data, 16)
                cg.lib().counter_add(cg.tensor.stream(), r.dev_base.data_ptr(), r.offset - off0)
                r.offset = off0
        torch.cuda.synchronize()
        assert S.OPTSTATE["adam"]["G"]["t"] == int(S.OPTSTATE["adam"]["G"]["t_dev"].item()), "host step count drifted"
        return S.PARAMETERS_G.numpy(), S.PARAMETERS_D.numpy(), int(S.OPTSTATE["adam"]["G"]["t_dev"].item())
    gG, gD, tg = run(True)
    eG, eD, te = run(False)
    assert tg == te == 3
    # same kernels, same streams, same step counts, and no float atomics anywhere on the path (the sampler's image gradient
    # is a gather, csrc/sampler.hip bilinear_bwd_det_k): replay and eager launches give the same bits
    np.testing.assert_array_equal(gG, eG)
    np.testing.assert_array_equal(gD, eD)


def test_copy_wrapped_nets_take_and_return_host_tensors(cg):
    """GPU-mode construction of the reference: D built with nn.Copy layers at head and tail (models.lua:642-644,
    703-706) and G wrapped by NN_UTILS.activateCuda (nn_utils.lua:620-680) consume / produce host FloatTensors."""
    cg.manual_seed(61)
    D_plain = cg.models.create_D((3, 32, 32), False)
    cg.manual_seed(61)
    D_copy = cg.models.create_D((3, 32, 32), True)
    assert D_copy.modules[0].typename == "nn.Copy" and D_copy.modules[-1].typename == "nn.Copy"
    for m in D_plain.listModules() + D_copy.listModules():
        if isinstance(m, (cg.nn.SpatialDropout, cg.nn.Dropout)):
            m.train = False  # deterministic comparison
    x = np.random.RandomState(1).rand(4, 3, 32, 32).astype(f32)
    out_h = D_copy.forward(x)
    assert isinstance(out_h, np.ndarray) and out_h.shape == (4, 1)
    close(out_h, D_plain.forward(cg.Tensor.from_numpy(x)).numpy(), tol=1e-6)
    g = np.ones((4, 1), f32)
    gi_h = D_copy.backward(x, g)
    assert isinstance(gi_h, np.ndarray) and gi_h.shape == x.shape
    close(gi_h, D_plain.backward(cg.Tensor.from_numpy(x), cg.Tensor.from_numpy(g)).numpy(), tol=1e-5)
    G = cg.nn_utils.activateCuda(cg.models.create_G((3, 32, 32), 100))
    img = G.forward((np.random.RandomState(2).rand(4, 100) * 2 - 1).astype(f32))
    assert isinstance(img, np.ndarray) and img.shape == (4, 3, 32, 32) and (img > 0).all() and (img < 1).all()
    assert cg.nn_utils.activateCuda(G) is G  # already contains Copy layers


def test_adversarial_train_epoch_loop(cg, capsys):
    """adversarial.train (adversarial.lua:27-292): one epoch = ceil(N_epoch / (batchSize/2)) iterations, confusion
    matrix over every D batch, accuracy gate inert at the default D_maxAcc."""
    cg.manual_seed(62)
    G, D = cg.models.create_G((3, 32, 32), 100), cg.models.create_D((3, 32, 32))
    S = cg.adversarial.State(dict(batchSize=16, N_epoch=40), G, D)
    data = cg.adversarial.TrainData(np.random.RandomState(3).rand(64, 3, 32, 32).astype(f32))
    tV = cg.adversarial.train(S, data, maxAccuracyD=1.01, accsInterval=20)
    out = capsys.readouterr().out
    assert "<trainer> Epoch #1 [batchSize = 16]" in out and "time to learn 1 sample" in out and "trained D 5 of 5" in out
    assert 0.0 <= tV <= 1.0 and S.EPOCH == 2
    assert S.OPTSTATE["adam"]["D"]["t"] == 5 and S.OPTSTATE["adam"]["G"]["t"] == 5
    # the gate (adversarial.lua:144-166): with maxAccuracyD = 0 D is never trained, G still is
    pD = S.PARAMETERS_D.numpy().copy()
    cg.adversarial.train(S, data, maxAccuracyD=0.0, accsInterval=20, verbose=False)
    np.testing.assert_array_equal(S.PARAMETERS_D.numpy(), pD)
    assert S.OPTSTATE["adam"]["G"]["t"] == 10 and S.OPTSTATE["adam"]["D"]["t"] == 5


def test_checkpoint_resume_continues_the_run(cg, tmp_path):
    """save after 2 iterations, resume in a fresh State, and the 3rd iteration equals the uninterrupted run
    bit for bit: parameters, Adam moments, step counts, BN running statistics, the counter-stream position, AND the host
    generator that draws the real-batch indices (nothing is injected here)."""
    def fresh():
        cg.manual_seed(71)
        G, D = cg.models.create_G((3, 32, 32), 100), cg.models.create_D((3, 32, 32))
        return cg.adversarial.State(dict(batchSize=8, seed=5), G, D)
    pool = np.random.RandomState(9).rand(32, 3, 32, 32).astype(f32)
    data = cg.adversarial.TrainData(pool)
    A = fresh()
    for k in range(2):
        cg.adversarial.iteration(A, data, 8)
    ck = cg.checkpoint.save(str(tmp_path / "adversarial.npz"), A)
    cg.adversarial.iteration(A, data, 8)
    pG_ref, pD_ref = A.PARAMETERS_G.numpy(), A.PARAMETERS_D.numpy()
    B = fresh()   # reseeds every generator, as a fresh `train.py --network ...` process does
    cg.checkpoint.load(ck, B)
    assert B.OPTSTATE["adam"]["G"]["t"] == 2 and B.OPTSTATE["adam"]["D"]["t"] == 2
    cg.adversarial.iteration(B, data, 8)
    np.testing.assert_array_equal(B.PARAMETERS_G.numpy(), pG_ref)
    np.testing.assert_array_equal(B.PARAMETERS_D.numpy(), pD_ref)


def test_checkpoint_resume_through_graph_replay(cg, tmp_path):
    """The same through GraphedIteration: the stream position lives in the device-side base and Adam's step count in a device
    counter; both must be in the checkpoint, and the host step count must equal the device one."""
    def fresh():
        cg.manual_seed(72)
        G, D = cg.models.create_G((3, 32, 32), 100), cg.models.create_D((3, 32, 32))
        return cg.adversarial.State(dict(batchSize=8, seed=6), G, D)
    data = cg.adversarial.TrainData(np.random.RandomState(10).rand(32, 3, 32, 32).astype(f32))
    A = fresh()
    itA = cg.adversarial.GraphedIteration(A, data, 8, warmup=1)   # 1 eager step
    itA()                                                           # + 1 replay
    torch.cuda.synchronize()
    assert A.OPTSTATE["adam"]["D"]["t"] == int(A.OPTSTATE["adam"]["D"]["t_dev"].item()) == 2
    ck = cg.checkpoint.save(str(tmp_path / "graph.npz"), A)
    itA()
    torch.cuda.synchronize()
    ref = (A.PARAMETERS_G.numpy(), A.PARAMETERS_D.numpy())
    B = fresh()
    cg.checkpoint.load(ck, B)
    assert B.OPTSTATE["adam"]["D"]["t"] == 2
    # continue eagerly from the restored position (device-side base included), with the device step counters
    B.device_rng = True
    for k in ("D", "G"):
        B.OPTSTATE["adam"][k]["device_step"] = True
    cg.adversarial.iteration(B, data, 8)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(B.PARAMETERS_G.numpy(), ref[0])
    np.testing.assert_array_equal(B.PARAMETERS_D.numpy(), ref[1])


def test_sampling_in_evaluate_mode_and_ranking(cg):
    """SURVEY.md §8 f4 (sample.lua:89-105, nn_utils.lua:89-117,334-349): G in evaluate() mode normalises with the
    BN running statistics, D ranks the images; against the oracle in the same mode."""
    seed = 81
    cg.manual_seed(seed); rng = O.RNG(seed)
    G, D = cg.models.create_G((3, 32, 32), 100), cg.models.create_D((3, 32, 32))
    Go, Do = O.create_G32up_c(3, 100, rng), O.create_D32_st3(3, 32, rng)
    S = cg.adversarial.State(dict(batchSize=8), G, D)
    rs = np.random.RandomState(2)
    z0 = (rs.rand(8, 100) * 2 - 1).astype(f32)
    G.forward(cg.Tensor.from_numpy(z0)); Go.forward(z0)       # one training-mode pass moves the running stats
    cg.nn_utils.switchToEvaluationMode(S); Go.training(False); Do.training(False)
    z = (rs.rand(20, 100) * 2 - 1).astype(f32)
    imgs = cg.nn_utils.createImagesFromNoise(S, z)
    ref = np.concatenate([Go.forward(z[i:i + 8]) for i in range(0, 20, 8)])
    close(imgs.numpy(), ref, tol=1e-4, what="evaluate-mode images")
    sorted_imgs, preds = cg.nn_utils.sortImagesByPrediction(S, imgs)
    ref_preds = np.concatenate([Do.forward(ref[i:i + 8]) for i in range(0, 20, 8)]).reshape(-1)
    close(np.sort(preds)[::-1], np.sort(ref_preds)[::-1], tol=2e-4, what="D ratings")
    assert np.all(np.diff(preds) <= 0) and sorted_imgs.shape == (20, 3, 32, 32)
    cg.nn_utils.switchToTrainingMode(S)
    assert all(m.train for m in G.listModules())


def test_visualize_progress_writes_the_three_grids_and_rates_with_v(cg, tmp_path):
    """nn_utils.lua:130-186: fixed-noise images, D's best / worst 50 with the two planted sanity images,
    the PNG grids with the epoch digits, V's ratings; the nets come back in training mode."""
    from PIL import Image
    cg.manual_seed(3)
    G, D = cg.models.create_G((3, 32, 32), 100), cg.models.create_D((3, 32, 32))
    S = cg.adversarial.State(dict(batchSize=32), G, D)
    S.EPOCH = 12
    S.MODEL_V = cg.nn.Sequential().add(cg.nn.View(3 * 32 * 32)).add(cg.nn.Linear(3 * 32 * 32, 2)).add(cg.nn.Sigmoid())
    rs = np.random.RandomState(1)
    z = (rs.rand(100, 100) * 2 - 1).astype(f32)
    train = rs.rand(60, 3, 32, 32).astype(f32)
    plot = []
    out = cg.nn_utils.visualizeProgress(S, z, train, str(tmp_path), start_time=7, plot_data=plot)
    for sub, side in (("images", 10), ("images_good", 7), ("images_bad", 7)):
        im = np.asarray(Image.open(out[sub]))
        assert out[sub].endswith(os.path.join(sub, "7_00012.png")) and im.shape == (side * 32 + 7, side * 32, 3)
        assert im[-7:-2, -8:-5].max() == 255            # the last digit ('2') is drawn
    assert len(plot) == 1 and plot[0][0] == 12 and all(0.0 <= r <= 1.0 for r in plot[0][1:])
    imgs = cg.nn_utils.createImagesFromNoise(S, z)       # V's rating of the fixed-noise images, recomputed by hand
    cg.nn_utils.switchToEvaluationMode(S)
    ev = cg.nn.as_nhwc(cg.nn_utils.createImagesFromNoise(S, z)).numpy()
    cg.nn_utils.switchToTrainingMode(S)
    w, b = S.MODEL_V.modules[1].weight.numpy(), S.MODEL_V.modules[1].bias.numpy()
    p0 = 1.0 / (1.0 + np.exp(-(ev.reshape(100, -1) @ w[0] + b[0])))
    assert abs((1.0 - p0.mean()) - out["ratings"][0]) < 1e-4
    assert all(m.train for m in G.listModules()) and all(m.train for m in D.listModules())
    del imgs


# ------------------------------------------------------------------------------ fused chains / planned passes
def test_fused_chain_entry_points_against_oracle_modules(cg):
    """csrc/fused.hip through the C ABI, against the oracle's separate modules: activation -> 2x2 pooling -> spatial dropout
    (models.lua:649-651, 656-658) for three stacked groups with their own PReLU slopes, and batch-norm -> PReLU
    (models.lua:207-208) forward + two-pass backward."""
    import ctypes
    L, st = cg.lib(), cg.tensor.stream()
    rs = np.random.RandomState(3)
    G, N, C, H = 3, 4, 8, 6
    x = rs.randn(G * N, C, H, H).astype(f32); x[0, 0, 0, 0] = 0.0
    gy = rs.randn(G * N, C, H // 2, H // 2).astype(f32)
    mask = (rs.rand(G * N, C) < 0.8).astype(f32)
    alphas = [0.25, -0.1, 0.6]
    al_t = [cg.Tensor.from_numpy(np.array([a], f32)) for a in alphas]
    ga_t = [cg.Tensor.from_numpy(np.array([1.0], f32)) for _ in alphas]   # accumulate semantics: starts at 1
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.ptr for t in ts])
    xt, gt, mt = cg.nn.as_nhwc(cg.Tensor.from_numpy(x)), cg.nn.as_nhwc(cg.Tensor.from_numpy(gy)), cg.Tensor.from_numpy(mask)
    for pool_max in (0, 1):
        for act in (1, 2, 0):
            y = cg.Tensor.empty((G * N, C, H // 2, H // 2), "nhwc"); dx = cg.Tensor.empty(x.shape, "nhwc")
            L.act_pool2_mask_forward(st, xt.ptr, y.ptr, mt.ptr, G, N, H, H, C, act, 0.333, arr(al_t) if act == 1 else None, pool_max)
            ws, wsb = cg.tensor.WS.get(L.act_pool2_mask_backward_workspace_bytes(G, N, H, H, C))
            L.act_pool2_mask_backward(st, xt.ptr, gt.ptr, mt.ptr, dx.ptr, G, N, H, H, C, act, 0.333,
                                      arr(al_t) if act == 1 else None, arr(ga_t) if act == 1 else None, 0.5, pool_max, ws, wsb)
            for g in range(G):
                sl = slice(g * N, (g + 1) * N)
                A = O.PReLU() if act == 1 else (O.LeakyReLU(0.333) if act == 2 else None)
                if act == 1:
                    A.weight[...] = alphas[g]
                P = O.MaxPool2() if pool_max else O.AvgPool2()
                h = A.forward(x[sl]) if A else x[sl]
                ref = P.forward(h) * mask[sl][:, :, None, None]
                close(y.numpy()[sl], ref, tol=1e-6, what=f"act {act} pool {pool_max} group {g} forward")
                gref = P.backward(gy[sl] * mask[sl][:, :, None, None])
                if A:
                    gref = A.backward(gref)
                close(dx.numpy()[sl], gref, tol=1e-6, what=f"act {act} pool {pool_max} group {g} backward")
    # galpha accumulation: fresh accumulators, one call, against the oracle's PReLU
    ga_t = [cg.Tensor.from_numpy(np.array([1.0], f32)) for _ in alphas]
    dx = cg.Tensor.empty(x.shape, "nhwc")
    ws, wsb = cg.tensor.WS.get(L.act_pool2_mask_backward_workspace_bytes(G, N, H, H, C))
    L.act_pool2_mask_backward(st, xt.ptr, gt.ptr, mt.ptr, dx.ptr, G, N, H, H, C, 1, 0.0, arr(al_t), arr(ga_t), 0.5, 1, ws, wsb)
    for g in range(G):
        sl = slice(g * N, (g + 1) * N)
        A = O.PReLU(); A.weight[...] = alphas[g]; P = O.MaxPool2()
        P.forward(A.forward(x[sl])); A.backward(P.backward(gy[sl] * mask[sl][:, :, None, None]))
        close(ga_t[g].numpy(), 1.0 + 0.5 * np.asarray(A.grad_weight, f32).reshape(1), tol=1e-5, what=f"galpha group {g}")
    # batch-norm + PReLU
    N, C, H = 6, 16, 8
    x = (rs.randn(N, C, H, H) * 1.5 + 0.3).astype(f32); dy = rs.randn(N, C, H, H).astype(f32)
    Bo, Ao = O.SBN(C, O.RNG(4)), O.PReLU()
    Bo.bias[...] = rs.randn(C).astype(f32) * 0.3
    gam, bet = cg.Tensor.from_numpy(Bo.weight.copy()), cg.Tensor.from_numpy(Bo.bias.copy())
    alpha, galpha = cg.Tensor.from_numpy(np.array([0.25], f32)), cg.Tensor.zeros((1,))
    ggam, gbet = cg.Tensor.zeros((C,)), cg.Tensor.zeros((C,))
    rm, rv = cg.Tensor.zeros((C,)), cg.Tensor.from_numpy(np.ones(C, f32))
    sm, si = cg.Tensor.zeros((C,)), cg.Tensor.zeros((C,))
    xt, dyt = cg.nn.as_nhwc(cg.Tensor.from_numpy(x)), cg.nn.as_nhwc(cg.Tensor.from_numpy(dy))
    y, dxt = cg.Tensor.empty(x.shape, "nhwc"), cg.Tensor.empty(x.shape, "nhwc")
    M = N * H * H
    sums = torch.zeros(2 * C, dtype=torch.float64, device="cuda")
    L.bn_stats(st, xt.ptr, M, C, sums.data_ptr())
    L.bn_act_forward(st, xt.ptr, y.ptr, gam.ptr, bet.ptr, sums.data_ptr(), float(M), M, C, 1e-5, 0.1, rm.ptr, rv.ptr, sm.ptr, si.ptr,
                     alpha.ptr)
    yo = Ao.forward(Bo.forward(x))
    close(y.numpy(), yo, tol=2e-5, what="bn+prelu forward")
    close(rm.numpy(), Bo.running_mean, tol=1e-6); close(rv.numpy(), Bo.running_var, tol=1e-5)
    bs = torch.zeros(2 * C + 1, dtype=torch.float64, device="cuda")
    L.bn_act_backward_stats(st, xt.ptr, dyt.ptr, sm.ptr, si.ptr, gam.ptr, bet.ptr, alpha.ptr, M, C, bs.data_ptr())
    L.bn_act_backward(st, xt.ptr, dyt.ptr, gam.ptr, bet.ptr, sm.ptr, si.ptr, alpha.ptr, bs.data_ptr(), float(M), bs.data_ptr(), M, C,
                      dxt.ptr, ggam.ptr, gbet.ptr, galpha.ptr, 1.0)
    go = Bo.backward(Ao.backward(dy))
    close(dxt.numpy(), go, tol=5e-5, what="bn+prelu backward")
    close(ggam.numpy(), Bo.grad_weight, K=M, what="dgamma"); close(gbet.numpy(), Bo.grad_bias, K=M, what="dbeta")
    close(galpha.numpy(), np.asarray(Ao.grad_weight, f32).reshape(1), K=M * C, what="dalpha")


def test_column_reduction_captured_on_a_stream_of_its_own(cg):
    """The deterministic column reductions keep their partials in a per-stream scratch.  torch.cuda.graph captures on a stream the
    library has never seen: it must get a block without allocating (bench.py times its roofline kernels this way), and the replayed
    sums must equal the eager ones bit for bit."""
    L = cg.lib()
    rs = np.random.RandomState(4)
    M, C = 4096, 128
    x = cg.Tensor.from_numpy(rs.randn(M, C).astype(f32))
    eager = torch.zeros(2 * C, dtype=torch.float64, device="cuda")
    L.bn_stats(cg.tensor.stream(), x.ptr, M, C, eager.data_ptr())         # first use of the scratch pool: outside any capture
    torch.cuda.synchronize()
    sums = torch.zeros(2 * C, dtype=torch.float64, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        L.bn_stats(cg.tensor.stream(), x.ptr, M, C, sums.data_ptr())
    g.replay(); g.replay()
    torch.cuda.synchronize()
    assert torch.equal(sums, eager)
    ref = np.concatenate([x.numpy().astype(np.float64).sum(0), (x.numpy().astype(np.float64) ** 2).sum(0)])
    close(sums.cpu().numpy(), ref, K=M, what="captured bn_stats")


def test_concat_dropout_and_head_launches(cg):
    """csrc/fused.hip: nn.Concat -> nn.SpatialDropout and nn.Dropout -> nn.Linear(F, 1) -> nn.Sigmoid as single launches.  The masks
    drawn inside the launches are bit-equal to cg_rng_bernoulli_dev at the same offsets; the concat / split results are bit-equal to
    the separate kernels; the head against float64 numpy."""
    import ctypes
    L, st = cg.lib(), cg.tensor.stream()
    rs = np.random.RandomState(12)
    N, H, Cs = 6, 4, (8, 8, 8, 16)
    Ct = sum(Cs)
    seed, off = 1234567, 777
    srcs = [cg.nn.as_nhwc(cg.Tensor.from_numpy(rs.randn(N, c, H, H).astype(f32))) for c in Cs]
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.ptr for t in ts])
    cc = (ctypes.c_int * 4)(*Cs)
    out, noise = cg.Tensor.empty((N, Ct, H, H), "nhwc"), cg.Tensor.zeros((N, Ct))
    L.concat_channels_dropout(st, 4, arr(srcs), cc, out.ptr, noise.ptr, N, H * H, 0.5, 1.0, seed, off, None)
    ref_noise, cat, ref = cg.Tensor.zeros((N, Ct)), cg.Tensor.empty((N, Ct, H, H), "nhwc"), cg.Tensor.empty((N, Ct, H, H), "nhwc")
    L.rng_bernoulli_dev(st, ref_noise.ptr, N * Ct, 0.5, 1.0, seed, off, None)
    L.concat_channels(st, 4, arr(srcs), cc, cat.ptr, N * H * H)
    L.mask_mul(st, cat.ptr, ref_noise.ptr, ref.ptr, N, H * H, Ct, 1)
    np.testing.assert_array_equal(noise.numpy(), ref_noise.numpy())
    assert 0.3 < noise.numpy().mean() < 0.7
    np.testing.assert_array_equal(out.numpy(), ref.numpy())
    g = cg.nn.as_nhwc(cg.Tensor.from_numpy(rs.randn(N, Ct, H, H).astype(f32)))
    d1 = [cg.Tensor.empty((N, c, H, H), "nhwc") for c in Cs]; d0 = [cg.Tensor.empty((N, c, H, H), "nhwc") for c in Cs]
    L.split_channels_masked(st, 4, g.ptr, noise.ptr, arr(d1), cc, N, H * H)
    gm = cg.Tensor.empty((N, Ct, H, H), "nhwc")
    L.mask_mul(st, g.ptr, noise.ptr, gm.ptr, N, H * H, Ct, 1)
    L.split_channels(st, 4, gm.ptr, arr(d0), cc, N * H * H)
    for a, b in zip(d1, d0):
        np.testing.assert_array_equal(a.numpy(), b.numpy())
    # the head, O = 1 (models.lua:700) and O = 3
    for Nn, F, Oo in ((128, 256, 1), (10, 100, 3)):
        assert L.drop_linear_sigmoid_supported(Nn, F, Oo) == 1
        x = rs.randn(Nn, F).astype(f32); w = (rs.randn(Oo, F) * 0.1).astype(f32); b = rs.randn(Oo).astype(f32)
        dp = rs.randn(Nn, Oo).astype(f32)
        xt, wt, bt = cg.Tensor.from_numpy(x), cg.Tensor.from_numpy(w), cg.Tensor.from_numpy(b)
        nz, xd, z, p = cg.Tensor.zeros((Nn, F)), cg.Tensor.zeros((Nn, F)), cg.Tensor.zeros((Nn, Oo)), cg.Tensor.zeros((Nn, Oo))
        L.drop_linear_sigmoid_forward(st, xt.ptr, wt.ptr, bt.ptr, nz.ptr, xd.ptr, z.ptr, p.ptr, Nn, F, Oo, 0.5, 2.0, seed, off + 5, None)
        rn = cg.Tensor.zeros((Nn, F))
        L.rng_bernoulli_dev(st, rn.ptr, Nn * F, 0.5, 2.0, seed, off + 5, None)
        np.testing.assert_array_equal(nz.numpy(), rn.numpy())
        m = rn.numpy().astype(np.float64)
        xd_ref = x * rn.numpy()
        np.testing.assert_array_equal(xd.numpy(), xd_ref)
        z_ref = xd_ref.astype(np.float64) @ w.astype(np.float64).T + b
        close(z.numpy(), z_ref, K=F, what=f"head z O={Oo}")
        p_ref = 1.0 / (1.0 + np.exp(-z_ref))
        close(p.numpy(), p_ref, tol=2e-6, what=f"head p O={Oo}")
        gx, gw, gb = cg.Tensor.zeros((Nn, F)), cg.Tensor.from_numpy(np.ones((Oo, F), f32)), cg.Tensor.from_numpy(np.ones(Oo, f32))
        dpt = cg.Tensor.from_numpy(dp)
        L.drop_linear_sigmoid_backward(st, dpt.ptr, p.ptr, xd.ptr, nz.ptr, wt.ptr, gx.ptr, gw.ptr, gb.ptr, Nn, F, Oo, 0.5)
        pn = p.numpy().astype(np.float64)
        gz = dp * pn * (1 - pn)
        close(gx.numpy(), (gz @ w.astype(np.float64)) * m, K=Oo, what=f"head gx O={Oo}")
        close(gw.numpy(), 1.0 + 0.5 * gz.T @ xd_ref.astype(np.float64), K=Nn, what=f"head gw O={Oo}")     # accumulate semantics
        close(gb.numpy(), 1.0 + 0.5 * gz.sum(0), K=Nn, what=f"head gb O={Oo}")
        gx2 = cg.Tensor.zeros((Nn, F))
        L.drop_linear_sigmoid_backward(st, dpt.ptr, p.ptr, None, nz.ptr, wt.ptr, gx2.ptr, None, None, Nn, F, Oo, 0.0)   # updateGradInput only
        np.testing.assert_array_equal(gx2.numpy(), gx.numpy())


@pytest.mark.parametrize("which", ["G", "D"])
def test_planned_pass_matches_the_per_module_walk(cg, which):
    """The planned executor (cg_net_*: fused segments, lockstep branches, side stream, deferred reductions) against the plain
    nn.Module walk - one C call per module method - on the real networks (training mode, batch 6): same outputs and gradients
    up to the summation order of the slope / statistics reductions and of the fused head's dot product."""
    res = {}
    for planned in (True, False):
        cg.nn.planned = planned
        try:
            P, _, _ = _pair(cg, 77, which)
            pP, gP = P.getParameters()
            rs = np.random.RandomState(5)
            if which == "D":
                pP.copy(pP.numpy() + (rs.randn(pP.nElement()) * 0.01).astype(f32))   # move the transformers off the identity
                x = rs.rand(6, 3, 32, 32).astype(f32); dy = rs.randn(6, 1).astype(f32)
            else:
                x = (rs.rand(6, 100) * 2 - 1).astype(f32); dy = (rs.randn(6, 3, 32, 32) * 0.1).astype(f32)
            xin = cg.Tensor.from_numpy(x)
            out = P.forward(xin).numpy()
            assert P._planned_last == planned
            gi = cg.nn.as_plain(P.backward(xin, cg.Tensor.from_numpy(dy))).numpy()
            if planned:
                st = P._pnet[1].stats()
                assert st["programs"] == 1 and 0 < st["launches_forward"] < (20 if which == "G" else 50), st
                # module state is served by the plan: the first module's gradInput (adversarial.lua:193), fused-away outputs are None
                assert P.modules[0].gradInput is not None
                fused_away = [m for m in P.listModules() if isinstance(m, cg.nn.SpatialBatchNormalization)]
                assert all(P.module_state(m, "output") is None for m in fused_away)
            res[planned] = (out, gi, gP.numpy().copy())
        finally:
            cg.nn.planned = True
    (o1, g1, p1), (o0, g0, p0) = res[True], res[False]
    if which == "D":
        close(o1, o0, tol=1e-6, what="D output planned vs per-module")     # the head's 256-term dot product runs in another order
        close(g1, g0, tol=1e-6, what="D gradInput planned vs per-module")
    else:
        close(o1, o0, tol=2e-6, what="G output planned vs per-module")
        close(g1, g0, tol=1e-5, what="G gradInput (w.r.t. the noise) planned vs per-module")
    bulk_close(p1, p0, max_rel=1e-4, mean_rel=1e-6, what=f"{which} flat gradient planned vs per-module")


def test_generator_and_discriminator_passes_are_bit_reproducible(cg):
    """No floating-point atomics anywhere on the path: batch-norm statistics, their backward sums, bias / slope gradients and the
    sampler's image gradient are all summed in a fixed order (two-stage sums whose last workgroup adds the partials in order), so
    running the same forward + backward twice gives the same bits - for G (three batch-norm layers) as for D.  The reference buys
    this property for its sampler by pinning it to the CPU (models.lua:889-899)."""
    for which, N in (("G", 64), ("D", 32)):
        P, _, _ = _pair(cg, 13, which)
        pP, gP = P.getParameters()
        rs = np.random.RandomState(2)
        if which == "D":
            pP.copy(pP.numpy() + (rs.randn(pP.nElement()) * 0.01).astype(f32))
            x = rs.rand(N, 3, 32, 32).astype(f32); dy = rs.randn(N, 1).astype(f32)
        else:
            x = (rs.rand(N, 100) * 2 - 1).astype(f32); dy = (rs.randn(N, 3, 32, 32) * 0.1).astype(f32)
        xin, dyt = cg.Tensor.from_numpy(x), cg.Tensor.from_numpy(dy)
        runs = []
        for _ in range(3):
            cg.manual_seed(7)
            out = P.forward(xin).numpy()
            gP.zero()
            gi = cg.nn.as_plain(P.backward(xin, dyt)).numpy()
            runs.append((out, gi, gP.numpy().copy()))
        for r in runs[1:]:
            for a, b, what in zip(r, runs[0], ("output", "gradInput", "flat gradient")):
                np.testing.assert_array_equal(a, b, err_msg=f"{which}: {what} differs between two identical passes")


@pytest.mark.parametrize("which", ["G", "D"])
def test_plan_options_are_result_neutral(cg, which):
    """cg_net_set_option's ablation switches on the real networks at batch 16: deferred + batched weight-gradient reductions
    (cg_conv2d_wgrad_grouped_deferred + one cg_conv2d_wgrad_flush) against the immediate form, the side stream for the second
    branch group against one stream, shared pooling / shared-image sampling against one launch per branch: the flat gradient
    vectors must be equal bit for bit, and nothing may stay queued."""
    import ctypes
    res = {}
    for name, opts in (("default", {}), ("immediate", {"defer_wgrad": 0}), ("one stream", {"overlap_groups": 0}),
                       ("unshared", {"share_pool": 0, "sampler_shared": 0}), ("separate localisation modules", {"fuse_locnet": 0}),
                       ("packing on the pass's stream", {"pack_overlap": 0}), ("head modules one by one", {"head_fuse": 0})):
        P, _, _ = _pair(cg, 31, which)
        pP, gP = P.getParameters()
        rs = np.random.RandomState(9)
        if which == "D":
            pP.copy(pP.numpy() + (rs.randn(pP.nElement()) * 0.01).astype(f32))
            x = rs.rand(16, 3, 32, 32).astype(f32); dy = rs.randn(16, 1).astype(f32)
        else:
            x = (rs.rand(16, 100) * 2 - 1).astype(f32); dy = (rs.randn(16, 3, 32, 32) * 0.1).astype(f32)
        xin, dyt = cg.Tensor.from_numpy(x), cg.Tensor.from_numpy(dy)
        net = P._planned_net()
        for k, v in opts.items():
            cg.lib().net_set_option(net.h, k.encode(), v)
        cg.manual_seed(5)                     # same dropout masks in every variant
        P.forward(xin)
        gP.zero()
        P.backward(xin, dyt)
        P.backward(xin, dyt)                  # accumulate semantics: every layer a second time
        n = ctypes.c_int(-1)
        cg.lib().conv2d_wgrad_pending(cg.tensor.stream(), ctypes.byref(n))
        assert n.value == 0, f"{name}: weight-gradient reductions still queued after cg_net_backward"
        res[name] = gP.numpy().copy()
        assert np.abs(res[name]).max() > 0
    for name in ("immediate", "one stream", "unshared", "packing on the pass's stream"):
        np.testing.assert_array_equal(res[name], res["default"], err_msg=name)
    # the fused localisation launches (csrc/locnet.hip) sum their convolutions in another order than the GEMM kernels: fp32 re-association
    bulk_close(res["separate localisation modules"], res["default"], max_rel=2e-4, mean_rel=2e-6, what=f"{which} fused vs separate localisation nets")
    # the fused head (csrc/fused.hip head_fwd_k) adds its 256 products in another order than the GEMM
    bulk_close(res["head modules one by one"], res["default"], max_rel=2e-4, mean_rel=2e-6, what=f"{which} fused vs separate head")


def test_collectives_through_the_c_abi_single_rank(cg):
    """csrc/comm.hip on the one GPU gpurun provides: RCCL bound at run time, a 1-rank communicator, all-reduce (sum, average,
    fp32 and fp64) and broadcast on the side stream with event fork/join against the compute stream.  With one rank every
    collective is the identity, so this pins the plumbing (dlopen, ncclCommInitRank, stream ordering), not the maths; the
    sharded == full-batch identity is pinned with two ranks in tests/test_dp_gloo.py."""
    import ctypes
    L, st = cg.lib(), cg.tensor.stream()
    ok = ctypes.c_int(0)
    L.comm_available(ctypes.byref(ok))
    assert ok.value == 1, "librccl.so.1 must be loadable on the GPU box"
    uid = ctypes.create_string_buffer(128)
    L.comm_unique_id(uid, 128)
    h = ctypes.c_void_p()
    L.comm_init(ctypes.byref(h), 1, 0, uid.raw, 128)
    try:
        n, r = ctypes.c_int(-1), ctypes.c_int(-1)
        L.comm_size(h, ctypes.byref(n), ctypes.byref(r))
        assert (n.value, r.value) == (1, 0)
        g = torch.Generator(device="cuda").manual_seed(3)
        a = torch.randn(1 << 20, device="cuda", generator=g)
        ref = (a * 2).cpu()
        a.mul_(2.0)                                           # producer kernel on the compute stream ...
        L.comm_allreduce(h, st, a.data_ptr(), a.numel(), 0, 1)    # ... must be visible to the collective (fork)
        L.comm_wait(h, st)                                    # ... and the consumer must see the collective's result (join)
        b = a + 0.0
        torch.cuda.synchronize()
        assert torch.equal(b.cpu(), ref)
        d = torch.arange(257, dtype=torch.float64, device="cuda")
        L.comm_allreduce(h, st, d.data_ptr(), d.numel(), 1, 0)
        L.comm_broadcast(h, st, d.data_ptr(), d.numel(), 1, 0)
        L.comm_wait(h, st)
        L.comm_sync(h)
        assert torch.equal(d.cpu(), torch.arange(257, dtype=torch.float64))
    finally:
        L.comm_destroy(h)
