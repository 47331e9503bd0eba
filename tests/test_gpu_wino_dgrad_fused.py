"""The fused-transform data gradient of upsample2 -> conv5x5 (wino_dgrad_fused_kernel, csrc/winograd.hip; option CG_WINO_DGRAD_FUSE)
through cg_conv2d_ups2_wino_dgrad: against the oracle's conv2d_backward_data + UpSample2().backward and against the transform +
wino_gemm_g_kernel pair it replaces (CG_WINO_DGRAD_FUSE = 0), both under helpers.close with the K of the existing tests of this gradient,
K = 4 * Cout * 9.  Every case also shows that the fused kernel was the one launched (the CG_WINO_DGRAD_FUSE_LAUNCHES counter), that two
calls give equal bytes, that every element of dx_lo is written (NaN pre-fill) and that the v_dy workspace is left untouched.  The fused
kernel adds every product in the pair's order, so beyond the tolerance its dx_lo is also held to the pair's bytes."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from helpers import close, options
from oracle import oracle as O

pytestmark = pytest.mark.gpu
f32 = np.float32

CASES = [
    # N, Cin, Hp, Wp, Cout
    (1, 128, 2, 2, 128),      # one tile: every patch pixel outside the image on two sides
    (3, 128, 6, 4, 128),      # ragged tile count, a non-square grid, a partly filled tile block
    (2, 256, 16, 16, 128),    # the benchmarked layer's geometry: full 8 x 8 tile blocks, Cin = 256 = four 64-column blocks
    (5, 128, 8, 8, 256),      # 4 * Cout = 1024 planes of K, a batch that is no power of two, 4 x 4 tiles per image
]
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def cg():
    mod = importlib.import_module("cat-generator_amd")
    assert torch.cuda.is_available(), "these tests need the MI355X"
    mod.lib()
    mod.nn.SpatialConvolution.winograd_min_tiles = 0
    return mod


def launches(L):
    v = ctypes.c_long(-1)
    assert L.get_option(b"CG_WINO_DGRAD_FUSE_LAUNCHES", ctypes.byref(v)) == 0
    return v.value


@pytest.mark.parametrize("N,Cin,Hp,Wp,Cout", CASES)
def test_fused_dgrad_against_oracle_and_unfused(cg, N, Cin, Hp, Wp, Cout):
    rs = np.random.RandomState(1000 * N + Hp + Cout)
    w = (rs.randn(Cout, Cin, 5, 5) / np.sqrt(Cin * 25)).astype(f32)
    x = rs.randn(N, Cin, Hp, Wp).astype(f32)
    dy = rs.randn(N, Cout, 2 * Hp, 2 * Wp).astype(f32)
    ref = O.UpSample2().backward(O.conv2d_backward_data(dy, w, (N, Cin, 2 * Hp, 2 * Wp), 2))      # [N][Cin][Hp][Wp]

    m = cg.nn.SpatialConvolution(Cin, Cout, 5, 5, 1, 1, 2)
    m.weight.copy(w); m.bias.zero()
    m.forward(cg.nn.SpatialUpSamplingNearest(2).forward(cg.Tensor.from_numpy(x)))      # packs the Winograd-domain filters
    assert getattr(m, "_wino", False)
    L, st = cg.lib(), importlib.import_module("cat-generator_amd.tensor").stream()
    dev = m._u_bwd.device
    dyn = cg.nn.as_nhwc(cg.Tensor.from_numpy(dy))
    nv = L.conv2d_ups2_wino_v_floats(N, Hp, Wp, 4 * Cout)

    def run(mode):
        vdy = torch.full((nv,), SENTINEL, dtype=torch.float32, device=dev)
        dx = torch.full((N, Hp, Wp, Cin), float("nan"), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with options(cg, CG_WINO_DGRAD_FUSE=mode):
            before = launches(L)
            assert L.conv2d_ups2_wino_dgrad(st, dyn.ptr, m._u_bwd.data_ptr(), dx.data_ptr(), vdy.data_ptr(), N, Hp, Wp, Cin, Cout) == 0
            torch.cuda.synchronize()
            count = launches(L) - before
        return dx.cpu().numpy(), vdy, count

    fused, vdy, count = run(2)
    assert count == 1, "the fused path was requested and supports the shape, but the fallback ran"
    assert bool((vdy == SENTINEL).all()), "the fused path wrote to the v_dy workspace"
    assert np.isfinite(fused).all(), "dx_lo not fully written"
    again, _, count = run(2)
    assert count == 1 and fused.tobytes() == again.tobytes(), "two calls on the same inputs differ"
    old, vdy0, count = run(0)
    assert count == 0 and not bool((vdy0 == SENTINEL).all())      # the transform + GEMM pair ran and filled V
    K = 4 * Cout * 9
    e1 = close(fused.transpose(0, 3, 1, 2), ref, K=K, what="fused data gradient vs oracle")
    e2 = close(fused, old, K=K, what="fused vs transform + GEMM pair")
    e3 = close(old.transpose(0, 3, 1, 2), ref, K=K, what="transform + GEMM pair vs oracle")
    print(f"max|d|: fused-oracle {e1:.3e}, fused-unfused {e2:.3e}, unfused-oracle {e3:.3e}")
    assert fused.tobytes() == old.tobytes(), f"fused and unfused differ in bits (max|d| {e2:.3e})"
