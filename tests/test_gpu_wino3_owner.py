"""Who owns the transformed filters of the fused Winograd 3x3 kernel (wino3_fused_k, csrc/wino3.hip; option CG_WINO3).

They ride behind the packed operand: cg_pack_conv_weight(_batch) writes them at offset 9*64*64 of wf / wb of a 64 -> 64 plane 3x3 layer,
whatever CG_WINO3 says, and cg_pack_conv_weight_floats sizes those buffers.  Before, the library kept them in a process-wide table keyed by
the operand's address, which a pack under CG_WINO3 = 0 neither refreshed nor dropped and which a copied operand missed.  The cases:

* the bits of output and gradInput under CG_WINO3 = 2 are those of tests/golden/wino3_bits.json, RECORDED ON A BUILD OF THE COMMIT BEFORE
  THE CHANGE OF OWNERSHIP by this same file (the kernels did not change):

      CG_WINO3_BITS_RECORD=<file.json> pytest tests/test_gpu_wino3_owner.py -k same_bits

* filters packed while the option was off are the ones the fused kernel uses once it is on again (this sequence gave the OLD weights'
  output on the commit before);
* a device-to-device copy of a packed operand is as good as the original;
* CG_WINO3_LAUNCHES says which kernel ran: one launch per fused forward and per fused data gradient, none with the option off, none for
  a width that is no multiple of 16.
"""
import hashlib
import importlib
import json
import os

import numpy as np
import pytest
import torch

from helpers import close, counter, options
from oracle import oracle as O
from test_gpu_parity_full import WINO3_CASES

pytestmark = pytest.mark.gpu
f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino3_bits.json")
RECORD = os.environ.get("CG_WINO3_BITS_RECORD")
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


def launches(cg):
    return counter(cg, "CG_WINO3_LAUNCHES")


def weights(rs):
    return (rs.randn(64, 64, 3, 3) / np.sqrt(64 * 9)).astype(f32), rs.randn(64).astype(f32)


def layer(cg, w, b):
    m = cg.nn.SpatialConvolution(64, 64, 3, 3, 1, 1, 1)
    m.weight.copy(w); m.bias.copy(b)
    return m


@pytest.mark.parametrize("N,H,W", WINO3_CASES)
def test_same_bits_as_before_the_change_of_ownership(cg, N, H, W):
    rs = np.random.RandomState(N + H + W)
    m = layer(cg, *weights(rs))
    x = cg.Tensor.from_numpy(rs.randn(N, 64, H, W).astype(f32))
    with options(cg, CG_WINO3=2):
        y = m.forward(x).numpy().copy()
        gi = m.updateGradInput(x, cg.Tensor.from_numpy(rs.randn(*y.shape).astype(f32))).numpy().copy()
    h = hashlib.sha256()
    for a in (y, gi):
        assert np.isfinite(a).all() and np.abs(a).max() > 0, "an all-zero or non-finite tensor pins nothing"
        h.update(np.ascontiguousarray(a, dtype=f32).tobytes())
    case, digest = f"{N} x 64 x {H} x {W}", h.hexdigest()
    print(f"{case}: sha256 {digest}")
    if RECORD:
        _recorded[case] = digest
        return
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert case in golden, f"{case}: no digest in {GOLDEN}"
    assert digest == golden[case], f"{case}: output / gradInput differ from the bits recorded before the change"


def test_filters_packed_with_the_option_off_are_used_when_it_is_on_again(cg):
    N, H, W = 2, 8, 16
    rs = np.random.RandomState(11)
    w_old, b = weights(rs)
    w_new, _ = weights(rs)
    x = rs.randn(N, 64, H, W).astype(f32)
    xin = cg.Tensor.from_numpy(x)
    m = layer(cg, w_old, b)
    with options(cg, CG_WINO3=2):
        m.forward(xin)
    with options(cg, CG_WINO3=0):
        m.weight.copy(w_new)
        m.forward(xin)                              # re-packs, on the direct kernel
    with options(cg, CG_WINO3=2):
        before = launches(cg)
        y = m.forward(xin).numpy().copy()
        assert launches(cg) - before == 1, "the fused kernel was requested and the geometry fits, but another kernel ran"
        fresh = layer(cg, w_new, b).forward(xin).numpy().copy()
    close(y, O.conv2d_forward(x, w_new, b, 1), K=64 * 9, what="updateOutput after a re-pack under CG_WINO3 = 0")
    assert y.tobytes() == fresh.tobytes(), "a fresh module with the same weights gives other bits"


def test_a_copied_operand_is_as_good_as_the_original(cg):
    N, H, W = 3, 16, 16
    rs = np.random.RandomState(12)
    w, b = weights(rs)
    L, st = cg.lib(), importlib.import_module("cat-generator_amd.tensor").stream()
    n = L.pack_conv_weight_floats(64, 64, 3, 3)
    assert n == 9 * 4096 + 16 * 4096
    wc, bias = cg.Tensor.from_numpy(w), cg.Tensor.from_numpy(b)
    x = cg.nn.as_nhwc(cg.Tensor.from_numpy(rs.randn(N, 64, H, W).astype(f32)))
    wf = torch.empty(n, dtype=torch.float32, device="cuda")
    L.pack_conv_weight(st, wc.ptr, wf.data_ptr(), None, 64, 64, 3, 3)
    copy = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    L.memcpy_d2d(st, copy.data_ptr(), wf.data_ptr(), 4 * n)
    geom = (N, H, W, 64, 64, 3, 3, 1, 1, 0)
    nws = L.conv2d_workspace_bytes(*geom)
    ws = torch.empty(max(nws, 4) // 4, dtype=torch.float32, device="cuda")

    def run(operand):
        y = torch.full((N, H, W, 64), float("nan"), dtype=torch.float32, device="cuda")
        before = launches(cg)
        L.conv2d_forward(st, x.ptr, operand.data_ptr(), bias.ptr, y.data_ptr(), *geom, ws.data_ptr(), nws)
        torch.cuda.synchronize()
        return y.cpu().numpy(), launches(cg) - before

    with options(cg, CG_WINO3=2):
        y0, c0 = run(wf)
        wf.fill_(float("nan"))                      # the copy stands alone
        y1, c1 = run(copy)
    assert c0 == 1 and c1 == 1, "the fused kernel did not run on the packed operand / on its copy"
    assert np.isfinite(y0).all() and y0.tobytes() == y1.tobytes()


def test_the_counter_says_which_kernel_ran(cg):
    rs = np.random.RandomState(13)
    m = layer(cg, *weights(rs))

    def count(N, H, W):
        x = cg.Tensor.from_numpy(rs.randn(N, 64, H, W).astype(f32))
        dy = cg.Tensor.from_numpy(rs.randn(N, 64, H, W).astype(f32))
        c0 = launches(cg)
        m.forward(x)
        c1 = launches(cg)
        m.updateGradInput(x, dy)
        return c1 - c0, launches(cg) - c1

    with options(cg, CG_WINO3=2):
        for N, H, W in WINO3_CASES[:2]:
            assert count(N, H, W) == (1, 1), "one launch per fused forward and per fused data gradient"
        assert count(2, 8, 8) == (0, 0), "a width that is no multiple of 16 is not the fused kernel's"
    with options(cg, CG_WINO3=0):
        assert count(2, 8, 16) == (0, 0), "CG_WINO3 = 0 keeps every launch on the direct kernel"
