"""Bit-for-bit pins of csrc/winograd.hip: F(2x2,3x3) behind upsample2 -> conv5x5 and F(2x2,2x2) behind upsample2 -> conv3x3.

The transform kernels of the two families share their tile walk and their patch loaders, the filter transforms one walker, the two GEMM
kernels their workgroup placement, their output-transform coefficients and their store-and-statistics tail, and the host one predicate and
one sliced-data-gradient helper; a restructuring of those must not move a single bit.  Every case below calls the C ABI directly (no planner
threshold decides what runs), forces ONE branch through `helpers.options`, runs on fixed-seed inputs and takes one sha256 over the raw bytes
of the results.  tests/golden/wino_bits.json holds the digests, RECORDED ON A BUILD OF THE COMMIT BEFORE THE RESTRUCTURING by this same file,
before winograd.hip was touched:

    CG_WINO_BITS_RECORD=<file.json> pytest tests/test_gpu_wino_bits.py      # writes the digests instead of comparing them

Nothing here compares with a reference implementation - that is tests/test_gpu_parity.py, test_gpu_wino_dgrad_fused.py and
test_forced_winograd_variants.
"""
import hashlib
import importlib
import json
import os

import numpy as np
import pytest
import torch

from helpers import options

pytestmark = pytest.mark.gpu
f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino_bits.json")
RECORD = os.environ.get("CG_WINO_BITS_RECORD")
_recorded = {}

# (N, Cin, Hp, Wp, Cout), the smallest that reach each branch:
SHAPES = [
    (3, 128, 6, 4, 128),       # T = 18: one partly filled tile block, a 3 x 2 tile grid - the generic epilogue with its divisions, no XCD placement
    (2, 256, 8, 8, 128),       # T = 32, a power-of-two grid: the lean epilogue; two column blocks in the data gradient
    (8, 128, 16, 16, 256),     # T = 512: eight tile blocks, so the XCD placement is live; two column blocks forward, K = 1024 in the data gradient
]
# 5x5 -> F(2x2,3x3): 9 phase taps, 16 positions; 3x3 -> F(2x2,2x2): 4 phase taps, 9 positions
FAMILIES = {"f23": dict(taps=9, pack="conv2d_ups2_wino_pack", u="conv2d_ups2_wino_u_floats", fwd="conv2d_ups2_wino_forward_stats"),
            "f22": dict(taps=4, pack="conv2d_ups2_wino22_pack", u="conv2d_ups2_wino22_u_floats", fwd="conv2d_ups2_wino22_forward_stats")}


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


def check(golden, case, *tensors):
    h = hashlib.sha256()
    for t in tensors:
        a = np.ascontiguousarray(t.cpu().numpy(), dtype=f32)
        assert np.isfinite(a).all() and np.abs(a).max() > 0, f"{case}: an all-zero or non-finite tensor pins nothing"
        h.update(a.tobytes())
    digest = h.hexdigest()
    print(f"{case}: sha256 {digest}")
    if RECORD:
        _recorded[case] = digest
        return
    assert case in golden, f"{case}: no digest in {GOLDEN}"
    assert digest == golden[case], f"{case}: the results differ from the recorded bits"


def _stream():
    return importlib.import_module("cat-generator_amd.tensor").stream()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).cuda()


def _nan(n):
    """An output buffer: an element the kernels leave unwritten fails check()'s finiteness test."""
    return torch.full((int(n),), float("nan"), dtype=torch.float32, device="cuda")


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _phase_filters(rs, fam, Cin, Cout):
    """wf_ph [p][tap][ci][co], wb_ph [p][tap][co][ci]: what cg_pack_conv_weight_ups2 would hand on, here plain fixed-seed values."""
    n = 4 * FAMILIES[fam]["taps"] * Cin * Cout
    s = 1.0 / np.sqrt(Cin * FAMILIES[fam]["taps"])
    return _dev(rs.randn(n) * s), _dev(rs.randn(n) * s)


def _pack(cg, fam, wf, wb, Cin, Cout, want_f=True, want_b=True):
    L = cg.lib()
    nu = getattr(L, FAMILIES[fam]["u"])(Cin, Cout)
    uf, ub = (_nan(nu) if want_f else None), (_nan(nu) if want_b else None)
    torch.cuda.synchronize()
    getattr(L, FAMILIES[fam]["pack"])(_stream(), _ptr(wf) if want_f else None, _ptr(wb) if want_b else None, _ptr(uf), _ptr(ub), Cout, Cin)
    torch.cuda.synchronize()
    return uf, ub


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_pack(cg, golden, fam, shape):
    """u_fwd and u_bwd from one launch (CG_PACK_WIDE = 1) and from two (0), and each operand alone with a null pair."""
    _, Cin, _, _, Cout = shape
    wf, wb = _phase_filters(np.random.RandomState(Cin + 2 * Cout), fam, Cin, Cout)
    for wide in (0, 1):
        with options(cg, CG_PACK_WIDE=wide):
            check(golden, f"pack {fam} {shape} / wide {wide}", *_pack(cg, fam, wf, wb, Cin, Cout))
            check(golden, f"pack {fam} {shape} / wide {wide} / forward operand alone", _pack(cg, fam, wf, wb, Cin, Cout, want_b=False)[0])
            check(golden, f"pack {fam} {shape} / wide {wide} / data-gradient operand alone", _pack(cg, fam, wf, wb, Cin, Cout, want_f=False)[1])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_forward_stats(cg, golden, fam, shape):
    """y, V and the statistics rows with a bias: both staging families (F(2x2,2x2) has the LDS-direct one only) x both K steps, on the
    third shape with and without the XCD placement, and one call without statistics."""
    N, Cin, Hp, Wp, Cout = shape
    L = cg.lib()
    rs = np.random.RandomState(N + Cin + Hp + Wp + Cout)
    wf, wb = _phase_filters(rs, fam, Cin, Cout)
    uf, _ = _pack(cg, fam, wf, wb, Cin, Cout, want_b=False)
    x = _dev(rs.randn(N, Hp, Wp, Cin))
    bias = _dev(rs.randn(Cout))
    nv = L.conv2d_ups2_wino_v_floats(N, Hp, Wp, Cin) if fam == "f23" else L.conv2d_ups2_wino22_v_floats(N, Hp, Wp, Cin)
    rows = L.conv2d_ups2_wino_stats_rows(N, Hp, Wp, Cin, Cout)
    assert rows > 0

    def run(with_stats=True):
        y, v, stats = _nan(N * 4 * Hp * Wp * Cout), _nan(nv), _nan(rows * 2 * Cout)
        torch.cuda.synchronize()
        getattr(L, FAMILIES[fam]["fwd"])(_stream(), _ptr(x), _ptr(uf), _ptr(bias), _ptr(y), _ptr(v), N, Hp, Wp, Cin, Cout,
                                         _ptr(stats) if with_stats else None)
        torch.cuda.synchronize()
        return (y, v, stats) if with_stats else (y, v)

    for glds in ((0, 1) if fam == "f23" else (1,)):
        for bk in (16, 32):
            for xcd in ((0, 7) if shape == SHAPES[2] else (None,)):
                kv = dict(CG_WINO_GLDS=glds, CG_WINO_BK=bk)
                if xcd is not None:
                    kv["CG_XCD_SWIZZLE"] = xcd
                with options(cg, **kv):
                    check(golden, f"forward {fam} {shape} / glds {glds} / bk {bk}" + (f" / xcd {xcd}" if xcd is not None else ""), *run())
    check(golden, f"forward {fam} {shape} / no statistics", *run(with_stats=False))


def _dgrad_inputs(cg, fam, shape):
    N, Cin, Hp, Wp, Cout = shape
    rs = np.random.RandomState(7 * N + Cin + Hp + 3 * Wp + Cout)
    wf, wb = _phase_filters(rs, fam, Cin, Cout)
    _, ub = _pack(cg, fam, wf, wb, Cin, Cout, want_f=False)
    return ub, _dev(rs.randn(N, 2 * Hp, 2 * Wp, Cout))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_dgrad_f23(cg, golden, shape):
    """cg_conv2d_ups2_wino_dgrad: the transform + GEMM pair (CG_WINO_DGRAD_FUSE = 0) in both staging families and K steps, dx_lo and V;
    and the fused kernel (2), which writes no V."""
    N, Cin, Hp, Wp, Cout = shape
    L = cg.lib()
    ub, dy = _dgrad_inputs(cg, "f23", shape)
    nv = L.conv2d_ups2_wino_v_floats(N, Hp, Wp, 4 * Cout)

    def run():
        dx, v = _nan(N * Hp * Wp * Cin), _nan(nv)
        torch.cuda.synchronize()
        L.conv2d_ups2_wino_dgrad(_stream(), _ptr(dy), _ptr(ub), _ptr(dx), _ptr(v), N, Hp, Wp, Cin, Cout)
        torch.cuda.synchronize()
        return dx, v

    for glds in (0, 1):
        for bk in (16, 32):
            with options(cg, CG_WINO_DGRAD_FUSE=0, CG_WINO_GLDS=glds, CG_WINO_BK=bk):
                check(golden, f"dgrad f23 {shape} / pair / glds {glds} / bk {bk}", *run())
    with options(cg, CG_WINO_DGRAD_FUSE=2):
        dx, v = run()
        assert bool(torch.isnan(v).all()), "the fused data gradient wrote to the v_dy workspace"
        check(golden, f"dgrad f23 {shape} / fused", dx)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_dgrad_f23_split(cg, golden, shape):
    """cg_conv2d_ups2_wino_dgrad_split with a part buffer: these shapes give 4 K slices and the fixed-order sum."""
    N, Cin, Hp, Wp, Cout = shape
    L = cg.lib()
    ub, dy = _dgrad_inputs(cg, "f23", shape)
    nv = L.conv2d_ups2_wino_v_floats(N, Hp, Wp, 4 * Cout)
    npart = L.conv2d_ups2_wino_dgrad_part_floats(N, Hp, Wp, Cin, Cout)
    assert npart == 4 * N * Hp * Wp * Cin > 0, "the shape no longer takes the 4-slice form"
    for bk in (16, 32):
        with options(cg, CG_WINO_BK=bk):
            dx, v, part = _nan(N * Hp * Wp * Cin), _nan(nv), _nan(npart)
            torch.cuda.synchronize()
            L.conv2d_ups2_wino_dgrad_split(_stream(), _ptr(dy), _ptr(ub), _ptr(dx), _ptr(v), _ptr(part), N, Hp, Wp, Cin, Cout)
            torch.cuda.synchronize()
            check(golden, f"dgrad f23 {shape} / 4 slices / bk {bk}", dx, v)


def _dgrad_f22(cg, golden, shape, ub, dy, sliced, case):
    N, Cin, Hp, Wp, Cout = shape
    L = cg.lib()
    assert L.conv2d_ups2_wino22_dgrad_supported(N, Hp, Wp, Cin, Cout) == 1
    T = N * (Hp // 2) * (Wp // 2)
    nv = L.conv2d_ups2_wino22_dgrad_v_floats(N, Hp, Wp, Cin, Cout)
    assert nv == 36 * T * Cout + (4 * 4 * T * Cin if sliced else 0), "the shape does not take the expected form (4 slices / unsliced)"
    dx, v = _nan(N * Hp * Wp * Cin), _nan(nv)
    torch.cuda.synchronize()
    L.conv2d_ups2_wino22_dgrad(_stream(), _ptr(dy), _ptr(ub), _ptr(dx), _ptr(v), N, Hp, Wp, Cin, Cout)
    torch.cuda.synchronize()
    check(golden, case, dx, v[:36 * T * Cout])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_dgrad_f22(cg, golden, shape):
    """cg_conv2d_ups2_wino22_dgrad in its 4-slice form (fewer workgroups than CUs), both K steps: dx_lo and V."""
    ub, dy = _dgrad_inputs(cg, "f22", shape)
    for bk in (16, 32):
        with options(cg, CG_WINO_BK=bk):
            _dgrad_f22(cg, golden, shape, ub, dy, True, f"dgrad f22 {shape} / 4 slices / bk {bk}")


def test_dgrad_f22_unsliced(cg, golden):
    """The unsliced form needs ceil(T/64) * Cin/128 >= 256 workgroups; this is the smallest such shape.  dy is one fixed-seed image
    tiled over the batch with per-image scales (formed on the device: an elementwise fp32 product, one rounding)."""
    shape = (64, 128, 32, 32, 128)
    N, Cin, Hp, Wp, Cout = shape
    rs = np.random.RandomState(64)
    wf, wb = _phase_filters(rs, "f22", Cin, Cout)
    _, ub = _pack(cg, "f22", wf, wb, Cin, Cout, want_f=False)
    block = _dev(rs.randn(1, 2 * Hp, 2 * Wp, Cout))
    scales = _dev(0.5 + np.arange(N) / 61.0).reshape(N, 1, 1, 1)
    dy = (block * scales).contiguous()
    _dgrad_f22(cg, golden, shape, ub, dy, False, f"dgrad f22 {shape} / unsliced")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_wgrad_f23(cg, golden, shape):
    """cg_conv2d_ups2_wino_wgrad onto a non-zero gw and gb with scale 0.5, with gb and without, both TN staging families."""
    N, Cin, Hp, Wp, Cout = shape
    L = cg.lib()
    rs = np.random.RandomState(N + 2 * Cin + Hp + Wp + 3 * Cout)
    v = _dev(rs.randn(L.conv2d_ups2_wino_v_floats(N, Hp, Wp, Cin)))
    dy = _dev(rs.randn(N, 2 * Hp, 2 * Wp, Cout))
    gw0, gb0 = _dev(rs.randn(Cout * Cin * 25)), _dev(rs.randn(Cout))
    nws = L.conv2d_ups2_wino_wgrad_workspace_bytes(N, Hp, Wp, Cin, Cout)
    assert nws > 0
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda")
    for tn in (0, 1):
        for with_gb in (True, False):
            gw, gb = gw0.clone(), gb0.clone()
            torch.cuda.synchronize()
            with options(cg, CG_TN_GLDS=tn):
                L.conv2d_ups2_wino_wgrad(_stream(), _ptr(v), _ptr(dy), _ptr(gw), _ptr(gb) if with_gb else None, N, Hp, Wp, Cin, Cout, 0.5,
                                         ws.data_ptr(), nws)
                torch.cuda.synchronize()
            assert not torch.equal(gw, gw0) and (torch.equal(gb, gb0) != with_gb), "gw must move; gb exactly when it is passed"
            check(golden, f"wgrad f23 {shape} / tn glds {tn} / gb {int(with_gb)}", gw, gb)
