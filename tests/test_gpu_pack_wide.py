"""The wide launches of the weight re-packing (option CG_PACK_WIDE, default 1) against the kernels they replace (CG_PACK_WIDE = 0).

A re-pack is a permutation of the canonical weights plus, behind a folded upsampling, a few tap sums added in a fixed order, so the wide
kernels are held to the BYTES of the old ones, not to a tolerance:

* cg_pack_conv_weight_ups2 (pack_weight_ups2_wide_kernel, csrc/pack.hip): full 32 x 16 blocks, ragged blocks in both dimensions and fewer
  than 32 channels, both operands and each one alone.  The phase sums are also restated in numpy float32 in the kernels' (dy, dx) order,
  which is exact, so both settings are held to that as well; every output is pre-filled with a sentinel no sum can produce and is followed
  by a guard that must stay untouched.
* cg_conv2d_ups2_wino_pack / cg_conv2d_ups2_wino22_pack (both operands in one launch, csrc/winograd.hip) on the benchmarked layers.
* cg_pack_conv_weight_batch (pack_weight_batch_wide_kernel, csrc/pack.hip): tap chunks of 9 (3x3), 7 (7x7), 4 (the View -> Linear map
  layout) and 1 taps, a short last chunk (5x5), ragged blocks, a missing wb; the tap permutation is also held to numpy's, and the
  fused-Winograd filters behind the 64 -> 64 layer's operands, which the wide launch computes in workgroups of its own, to those of
  wino3_pack_k through the single-layer entry point.
* two batch-8 training iterations on injected indices and noise (the second one runs on re-packed weights) end on the same parameter bytes
  under both settings."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from helpers import options

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = -12345.5
GUARD = 64


@pytest.fixture(scope="module")
def cg():
    mod = importlib.import_module("cat-generator_amd")
    assert torch.cuda.is_available(), "these tests need the MI355X"
    mod.lib()
    return mod


def _stream():
    return importlib.import_module("cat-generator_amd.tensor").stream()


def _out(n):
    return torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")


def _host(t, n, what):
    a = t.cpu().numpy()
    assert (a[n:] == SENTINEL).all(), f"{what}: written past its {n} floats"
    assert not (a[:n] == SENTINEL).any(), f"{what}: not every element written"
    return a[:n]


def _phase_map(a, d, pad):
    return ((a + d - pad) >> 1) - ((a - pad) >> 1)


def _ups2_reference(w):
    """wf_ph [p][t'][ci][co] and wb_ph [p][t'][co][ci]: every phase tap summed from 0.f in (dy, dx) order, in float32 like the kernels."""
    Cout, Cin, k, _ = w.shape
    pad = (k - 1) // 2
    kp = _phase_map(0, k - 1, pad) + 1
    wb = np.zeros((4, kp * kp, Cout, Cin), f32)
    for p in range(4):
        for dy in range(k):
            for dx in range(k):
                t = _phase_map(p >> 1, dy, pad) * kp + _phase_map(p & 1, dx, pad)
                wb[p, t] = wb[p, t] + w[:, :, dy, dx]
    return np.ascontiguousarray(wb.transpose(0, 1, 3, 2)).ravel(), wb.ravel()


def _pack_ups2(L, w_dev, Cout, Cin, k, want_wf=True, want_wb=True):
    n = L.pack_conv_weight_ups2_floats(Cout, Cin, k, (k - 1) // 2)
    wf, wb = _out(n), _out(n)
    torch.cuda.synchronize()
    L.pack_conv_weight_ups2(_stream(), w_dev.data_ptr(), wf.data_ptr() if want_wf else None, wb.data_ptr() if want_wb else None,
                            Cout, Cin, k, (k - 1) // 2)
    torch.cuda.synchronize()
    return wf, wb, n


UPS2_CASES = [(128, 256, 5), (256, 512, 3), (72, 40, 5), (8, 16, 3), (33, 31, 5)]


@pytest.mark.parametrize("Cout,Cin,k", UPS2_CASES)
def test_upsampled_pack_same_bytes(cg, Cout, Cin, k):
    L = cg.lib()
    w = np.random.RandomState(Cout + Cin + k).randn(Cout, Cin, k, k).astype(f32)
    w_dev = torch.from_numpy(w).cuda()
    ref_f, ref_b = _ups2_reference(w)
    got = {}
    for mode in (0, 1):
        with options(cg, CG_PACK_WIDE=mode):
            wf, wb, n = _pack_ups2(L, w_dev, Cout, Cin, k)
        got[mode] = (_host(wf, n, f"wf_ph, CG_PACK_WIDE={mode}"), _host(wb, n, f"wb_ph, CG_PACK_WIDE={mode}"))
        assert got[mode][0].tobytes() == ref_f.tobytes(), f"wf_ph, CG_PACK_WIDE={mode}: not the sums in (dy, dx) order"
        assert got[mode][1].tobytes() == ref_b.tobytes(), f"wb_ph, CG_PACK_WIDE={mode}: not the sums in (dy, dx) order"
    assert got[1][0].tobytes() == got[0][0].tobytes(), "wf_ph differs between CG_PACK_WIDE = 1 and 0"
    assert got[1][1].tobytes() == got[0][1].tobytes(), "wb_ph differs between CG_PACK_WIDE = 1 and 0"
    with options(cg, CG_PACK_WIDE=1):       # one operand alone: the other stays untouched
        wf, wb, n = _pack_ups2(L, w_dev, Cout, Cin, k, want_wb=False)
        assert _host(wf, n, "wf_ph alone").tobytes() == got[0][0].tobytes()
        assert bool((wb == SENTINEL).all()), "wb_ph written though null was passed"
        wf, wb, n = _pack_ups2(L, w_dev, Cout, Cin, k, want_wf=False)
        assert _host(wb, n, "wb_ph alone").tobytes() == got[0][1].tobytes()
        assert bool((wf == SENTINEL).all()), "wf_ph written though null was passed"


@pytest.mark.parametrize("Cout,Cin,k", [(128, 256, 5), (256, 512, 3)])
def test_winograd_filter_forms_same_bytes(cg, Cout, Cin, k):
    """F(2x2,3x3) of the 256 -> 128 5x5 layer (u_fwd / u_bwd) and F(2x2,2x2) of the 512 -> 256 3x3 layer (u22 / u22b)."""
    L = cg.lib()
    w = np.random.RandomState(7 * k + Cout).randn(Cout, Cin, k, k).astype(f32)
    w_dev = torch.from_numpy(w).cuda()
    nu = L.conv2d_ups2_wino_u_floats(Cin, Cout) if k == 5 else L.conv2d_ups2_wino22_u_floats(Cin, Cout)
    pack = L.conv2d_ups2_wino_pack if k == 5 else L.conv2d_ups2_wino22_pack
    got = {}
    for mode in (0, 1):
        with options(cg, CG_PACK_WIDE=mode):
            wf, wb, _ = _pack_ups2(L, w_dev, Cout, Cin, k)
            uf, ub = _out(nu), _out(nu)
            torch.cuda.synchronize()
            pack(_stream(), wf.data_ptr(), wb.data_ptr(), uf.data_ptr(), ub.data_ptr(), Cout, Cin)
            torch.cuda.synchronize()
        got[mode] = (_host(uf, nu, f"u_fwd, CG_PACK_WIDE={mode}"), _host(ub, nu, f"u_bwd, CG_PACK_WIDE={mode}"))
    assert got[1][0].tobytes() == got[0][0].tobytes(), "the forward operand's filters differ between CG_PACK_WIDE = 1 and 0"
    assert got[1][1].tobytes() == got[0][1].tobytes(), "the data gradient's filters differ between CG_PACK_WIDE = 1 and 0"


# Cout, Cin, kH, kW, View -> Linear map layout, wb given
BATCH_LAYERS = [(64, 64, 3, 3, 0, True), (128, 128, 7, 7, 0, True), (256, 320, 2, 2, 1, True), (72, 40, 1, 1, 0, False),
                (24, 40, 5, 5, 0, True)]      # the last one: chunks of 7, 7, 7 and 4 taps, ragged in both dimensions


def _pack_batch(L, ws):
    n = len(BATCH_LAYERS)
    sizes = [L.pack_conv_weight_floats(co, ci, kh, kw) for co, ci, kh, kw, _, _ in BATCH_LAYERS]
    wf = [_out(s) for s in sizes]
    wb = [_out(s) if lay[5] else None for s, lay in zip(sizes, BATCH_LAYERS)]
    ptrs = lambda ts: ctypes.cast((ctypes.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in ts]), ctypes.c_void_p)
    ints = lambda col: (ctypes.c_int * n)(*[int(lay[col]) for lay in BATCH_LAYERS])
    torch.cuda.synchronize()
    L.pack_conv_weight_batch(_stream(), n, ptrs(ws), ptrs(wf), ptrs(wb), ints(0), ints(1), ints(2), ints(3), ints(4))
    torch.cuda.synchronize()
    return wf, wb, sizes


def test_plain_batch_pack_same_bytes(cg):
    L = cg.lib()
    rs = np.random.RandomState(5)
    w_host = [rs.randn(co, ci, kh, kw).astype(f32) for co, ci, kh, kw, _, _ in BATCH_LAYERS]
    ws = [torch.from_numpy(w).cuda() for w in w_host]
    got = {}
    for mode in (0, 1):
        with options(cg, CG_PACK_WIDE=mode):
            wf, wb, sizes = _pack_batch(L, ws)
        got[mode] = []
        for i, (co, ci, kh, kw, as_map, has_wb) in enumerate(BATCH_LAYERS):
            used = co * ci * kh * kw if as_map else sizes[i]       # the map layout writes no transformed filters
            f = wf[i].cpu().numpy()
            assert (f[used:] == SENTINEL).all() and not (f[:used] == SENTINEL).any(), f"layer {i}: wf"
            b = wb[i].cpu().numpy() if has_wb else None
            if has_wb:
                assert (b[used:] == SENTINEL).all() and not (b[:used] == SENTINEL).any(), f"layer {i}: wb"
            taps = co * ci * kh * kw
            w = w_host[i].reshape(co, ci, kh * kw)
            assert f[:taps].tobytes() == np.ascontiguousarray(w.transpose(2, 1, 0)).tobytes(), f"layer {i}: wf [tap][ci][co]"
            if has_wb:
                want = w.transpose(0, 2, 1) if as_map else w[:, :, ::-1].transpose(2, 0, 1)      # wbT [co][tap][ci] / [KK-1-tap][co][ci]
                assert b[:taps].tobytes() == np.ascontiguousarray(want).tobytes(), f"layer {i}: wb"
            got[mode].append((f[:used].copy(), b[:used].copy() if has_wb else None))
    for i, ((f0, b0), (f1, b1)) in enumerate(zip(got[0], got[1])):
        assert f1.tobytes() == f0.tobytes(), f"layer {i}: wf differs between CG_PACK_WIDE = 1 and 0"
        assert (b1 is None) == (b0 is None) and (b1 is None or b1.tobytes() == b0.tobytes()), f"layer {i}: wb differs"
    # the 64 -> 64 layer's transformed filters behind the taps: those of the single-layer entry point
    n0 = L.pack_conv_weight_floats(64, 64, 3, 3)
    assert n0 > 64 * 64 * 9
    sf, sb = _out(n0), _out(n0)
    torch.cuda.synchronize()
    L.pack_conv_weight(_stream(), ws[0].data_ptr(), sf.data_ptr(), sb.data_ptr(), 64, 64, 3, 3)
    torch.cuda.synchronize()
    assert _host(sf, n0, "single wf").tobytes() == got[1][0][0].tobytes(), "fused-Winograd filters behind wf"
    assert _host(sb, n0, "single wb").tobytes() == got[1][0][1].tobytes(), "fused-Winograd filters behind wb"


def _two_iterations(cg, mode):
    N = 8
    with options(cg, CG_PACK_WIDE=mode):
        cg.manual_seed(11)
        G, D = cg.models.create_G((3, 32, 32), 100), cg.models.create_D((3, 32, 32))
        S = cg.adversarial.State(dict(batchSize=N), G, D)
        rs = np.random.RandomState(2)
        data = cg.adversarial.TrainData(rs.rand(16, 3, 32, 32).astype(f32))
        for _ in range(2):       # the second iteration reads operands re-packed from the first one's update
            idx = rs.randint(0, 16, size=N // 2)
            nd = (rs.rand(N // 2, 100) * 2 - 1).astype(f32); ng = (rs.rand(N, 100) * 2 - 1).astype(f32)
            cg.adversarial.iteration(S, data, N, real_idx=idx, noise_D=nd, noise_G=ng)
        torch.cuda.synchronize()
        return S.PARAMETERS_G.numpy().copy(), S.PARAMETERS_D.numpy().copy()


def test_training_step_same_parameter_bytes(cg):
    g0, d0 = _two_iterations(cg, 0)
    g1, d1 = _two_iterations(cg, 1)
    assert np.isfinite(g1).all() and np.isfinite(d1).all()
    assert g1.tobytes() == g0.tobytes(), f"G's parameters differ in {int((g1 != g0).sum())} of {g1.size} entries"
    assert d1.tobytes() == d0.tobytes(), f"D's parameters differ in {int((d1 != d0).sum())} of {d1.size} entries"
