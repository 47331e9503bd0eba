"""Bit-for-bit pins of the implicit-GEMM kernels of csrc/gemm.hip, of the weight-gradient finishes of csrc/wgrad_finish.hip and of the VALU
skinny kernels of csrc/skinny.hip.

The four GEMM kernels (igemm_nn / igemm_nng / igemm_tn / igemm_tng) share their epilogues, their tile decode and their host-side
argument packing; a restructuring of those must not move a single bit.  Every case below forces ONE branch of the shared code through
`cg_set_option` (reset afterwards), runs a small layer forward and backward on fixed inputs and takes one sha256 over the raw bytes of
output, gradInput, gradWeight and gradBias.  tests/golden/gemm_bits.json holds the digests, RECORDED ON A BUILD OF THE COMMIT BEFORE THE
RESTRUCTURING by this same file (the finish cases at the end: before the finishes moved out of gemm.hip):

    CG_GEMM_BITS_RECORD=<file.json> pytest tests/test_gpu_gemm_bits.py      # writes the digests instead of comparing them

Nothing here compares with a reference implementation - the oracle-compared parity of the same shapes is tests/test_gpu_parity_full.py.
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
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_bits.json")
RECORD = os.environ.get("CG_GEMM_BITS_RECORD")
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


def check(golden, case, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a, dtype=f32)
        assert np.isfinite(a).all() and np.abs(a).max() > 0, f"{case}: an all-zero or non-finite tensor pins nothing"
        h.update(a.tobytes())
    digest = h.hexdigest()
    print(f"{case}: sha256 {digest}")
    if RECORD:
        _recorded[case] = digest
        return digest
    assert case in golden, f"{case}: no digest in {GOLDEN}"
    assert digest == golden[case], f"{case}: output / gradInput / gradWeight / gradBias differ from the recorded bits"
    return digest


# the two staging families (register staging / LDS-direct loads) of the NN and TN kernels
FAMILIES = {"regs": dict(CG_NN_GLDS=0, CG_TN_GLDS=0), "glds": dict(CG_NN_GLDS=3, CG_TN_GLDS=1)}
NO_OTHER = dict(CG_SKINNY=0, CG_WINO3=0)      # keep the skinny and the fused-Winograd kernels out of the way


def conv_bits(cg, N, Cin, H, W, Cout, k, ups, seed):
    """One SpatialConvolution (optionally behind the lazy 2x upsampling), forward and backward on fixed inputs."""
    rs = np.random.RandomState(seed)
    pad = (k - 1) // 2
    cg.nn.SpatialConvolution.winograd = False
    try:
        m = cg.nn.SpatialConvolution(Cin, Cout, k, k, 1, 1, pad)
        m.weight.copy((rs.randn(Cout, Cin, k, k) / np.sqrt(Cin * k * k)).astype(f32))
        m.bias.copy(rs.randn(Cout).astype(f32))
        xin = cg.Tensor.from_numpy(rs.randn(N, Cin, H, W).astype(f32))
        if ups:
            up = cg.nn.SpatialUpSamplingNearest(2)
            xin = up.forward(xin)
        y = m.forward(xin).numpy().copy()
        dy = rs.randn(*y.shape).astype(f32)
        m.gradWeight.zero(); m.gradBias.zero()
        gi = m.backward(xin, cg.Tensor.from_numpy(dy))
        if ups:
            gi = up.updateGradInput(None, gi)
        return y, gi.numpy().copy(), m.gradWeight.numpy().copy(), m.gradBias.numpy().copy()
    finally:
        cg.nn.SpatialConvolution.winograd = True


# (N, Cin, H, W, Cout, k, ups): H, W are the convolution's input dims before the folded upsampling
TAILS = {
    "ragged generic tail": (3, 64, 10, 6, 72, 3, 0),            # M = 180, Cout = 72: no full tile anywhere
    "lean consecutive tail": (4, 64, 16, 16, 128, 3, 0),        # M = 1024, Cout = 128: full tiles, consecutive rows
    "strided tail, four phases": (2, 32, 8, 8, 128, 3, 1),      # lean strided stores in the LDS-direct family, generic in the other
    "strided tail, 3x5 grid": (3, 16, 3, 5, 8, 3, 1),           # no power-of-two grid: the pixel decode by division
}


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("tail", list(TAILS))
def test_store_tails(cg, golden, tail, family, splits):
    """Unsplit (one forced split: the value 0 would leave the count to the plan, which splits the first two shapes four ways) the NN
    epilogue adds the bias and stores the output itself; with three forced splits it stores partials and the reduce kernels finish."""
    with options(cg, CG_NN_SPLITS=splits, CG_TN_SPLITS=splits, **FAMILIES[family], **NO_OTHER):
        check(golden, f"{tail} / {family} / splits {splits}", *conv_bits(cg, *TAILS[tail], seed=len(tail)))


# The branches of the kernels' SET-UP (tile order, row / column decode, tap masks and walk, lean addressing, K step, rows per pass): what
# the two staging families share in front of and inside the K loop (csrc/gemm_tile.h).
LEAN = TAILS["lean consecutive tail"]


def test_no_vector_path(cg, golden):
    """(2, 5, 6, 5, 7, 3, 0): M = 2 * 6 * 5 = 60 rows of a 6 x 5 grid (no power of two: lgW = -1, the pixel decode divides), Cin = 5 and
    Cout = 7, so Cin % 16 != 0 (FAST off: igemm_nn_kernel's per-element gather), Cout % 4 != 0 forward and Cin % 4 != 0 in the data
    gradient (VECB off: scalar weight loads) -> igemm_nn_kernel<128, 32, 4, 1, false, false, 16> both ways; the weight gradient has
    Cin % 4 != 0 and Cout % 4 != 0 -> igemm_tn_kernel<..., false, false> (four columns decoded per thread, scalar dy loads, never lean)."""
    with options(cg, **NO_OTHER):
        check(golden, "no vector path", *conv_bits(cg, 2, 5, 6, 5, 7, 3, 0, seed=19))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_k_step_16(cg, golden, family):
    """CG_GEMM_BK32 = 0 on (4, 64, 16, 16, 128, 3, 0): the plan picks 64-row tiles (M = 1024: 8 x 1 tiles of 128 rows < 2 x 256 CUs), which
    run K step 32 by default; with the option off igemm_nn_kernel<64, 128, 2, 2, true, true, 16> (regs) and igemm_nng_kernel<64, 128, 2, 2, 16>
    (glds: CG_NN_GLDS = 3 allows its K step 16) - KV = 4 quads per row, the two-bit swizzles, ARPP = 64 rows per pass."""
    with options(cg, CG_GEMM_BK32=0, **FAMILIES[family], **NO_OTHER):
        check(golden, f"k step 16 / {family}", *conv_bits(cg, *LEAN, seed=23))


@pytest.mark.parametrize("bk32", [1, 0])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_128_row_tiles(cg, golden, family, bk32):
    """CG_NN_TILE = CG_TN_TILE = 128128 on the same shape.  NN: MI = 2 accumulator rows per wave; K step 32 only in the LDS-direct family
    (igemm_nng_kernel<128, 128, 2, 2, 32>: ARPP = 32, AROWS = 4), the register kernel keeps K step 16 for 128-row tiles (ARPP = 64,
    AROWS = 2) and so does LDS-direct with CG_GEMM_BK32 = 0.  TN: AVEC = 32 quads per row, ARPP = 8, APASS = 2 passes per K tile for both
    operands (the 64-row tiles: one A pass of 16 rows); Ktot = 576 = 4.5 row tiles, so the last tile is half empty (c_ok, generic store)."""
    with options(cg, CG_NN_TILE=128128, CG_TN_TILE=128128, CG_GEMM_BK32=bk32, **FAMILIES[family], **NO_OTHER):
        check(golden, f"128-row tiles / {family} / bk32 {bk32}", *conv_bits(cg, *LEAN, seed=29))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_tile_orders(cg, golden, family):
    """(8, 256, 8, 8, 256, 3, 0), CG_NN_SPLITS = 1, CG_TN_SPLITS = 8, at CG_XCD_SWIZZLE 0 (natural order), 1 and 7.
    NN (forward and data gradient alike, Cin = Cout): M = 8 * 64 = 512, Cout = 256 -> BN = 128, and 4 x 2 tiles of 128 rows < 2 x 256 CUs
    -> BM = 64: gridDim.x = 8 row tiles x 2 column tiles = 16, a multiple of 8, so bit 1 hands every XCD a row range; ntn = 2, xg = 4 XCDs
    per column tile, 8 row tiles % 4 == 0 and ntn * xb + (8 / ntn) * wb < xb + 8 * wb (xb = 8 * 64 * 256 * 4 = 0.5 MB < 4 wb,
    wb = 2304 * 256 * 4 = 2.4 MB), so bit 4 makes the LDS-direct kernel weights-stationary (the register kernel has bit 1 only).
    TN: Ktot = 2304 -> 18 x 2 tiles of 128 x 128, 512 / 16 = 32 K tiles in 8 splits of 64 pixels: gridDim.y & 7 == 0, so bit 2 gives every
    XCD its pixel chunks (gridDim.x = 36 is no multiple of 8: bit 1 alone leaves the natural order).
    The order decides only which workgroup computes which tile: the three digests are equal, and pinned."""
    digests = []
    for swz in (0, 1, 7):
        with options(cg, CG_XCD_SWIZZLE=swz, CG_NN_SPLITS=1, CG_TN_SPLITS=8, **FAMILIES[family], **NO_OTHER):
            digests.append(check(golden, f"tile order / {family} / swizzle {swz}", *conv_bits(cg, 8, 256, 8, 8, 256, 3, 0, seed=31)))
    assert digests[0] == digests[1] == digests[2], f"the tile order changed the bits: {digests}"


def planned_bits(cg, build, x, fusion, seed):
    """A small nn.Sequential through the planned executor: output, gradInput and the flat gradient (weights and biases)."""
    cg.manual_seed(seed)
    net = build()
    p, g = net.getParameters()
    rs = np.random.RandomState(seed)
    p.copy(p.numpy() + (rs.randn(p.nElement()) * 0.01).astype(f32))
    xin = cg.Tensor.from_numpy(x)
    if x.ndim == 4:
        xin = cg.nn.as_nhwc(xin)
    pn = net._planned_net()
    assert pn is not None
    cg.lib().net_set_option(pn.h, b"fusion", int(fusion))
    y = cg.nn.as_plain(net.forward(xin)).numpy().copy()
    assert net._planned_last
    dy = cg.Tensor.from_numpy(rs.randn(*y.shape).astype(f32))
    g.zero()
    gi = cg.nn.as_plain(net.backward(xin, dy)).numpy().copy()
    return (y, gi, g.numpy().copy()), pn.stats()["launches_forward"]


def _act_net(cg):
    net = cg.nn.Sequential()
    net.add(cg.nn.SpatialConvolution(64, 64, 3, 3, 1, 1, 1)); net.add(cg.nn.PReLU(None, None, True))
    net.add(cg.nn.SpatialConvolution(64, 128, 3, 3, 1, 1, 1)); net.add(cg.nn.LeakyReLU(0.2))
    return net


def _stats_net(cg, planes=128):
    net = cg.nn.Sequential()
    net.add(cg.nn.SpatialUpSamplingNearest(2)); net.add(cg.nn.SpatialConvolution(64, planes, 3, 3, 1, 1, 1))
    net.add(cg.nn.SpatialBatchNormalization(planes)); net.add(cg.nn.PReLU(None, None, True))
    return net


EPILOGUE_NETS = {"activation": (_act_net, 16), "statistics": (_stats_net, 8), "statistics, 64 planes": (lambda cg: _stats_net(cg, 64), 8)}


@pytest.mark.parametrize("fusion", [1, 0], ids=["fused", "unfused"])
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("which", list(EPILOGUE_NETS))
def test_epilogue_with_activation_and_with_statistics(cg, golden, which, family, fusion):
    """conv -> PReLU, conv -> LeakyReLU (the activation in the GEMM's epilogue, two outputs) and upsample -> conv -> batch norm -> PReLU (the
    batch-norm column sums in the epilogue of the four phase GEMMs; 128 planes = 64-column wave tiles, 64 planes = 32-column ones, whose
    sums of squares are formed differently) at N = 4, unsplit: a split launch leaves both to its reduce kernel.  The fused leg must really
    have folded the modules into the GEMM launches: its forward plan is shorter than the unfused one, whose bits it shares."""
    build, hw = EPILOGUE_NETS[which]
    x = np.random.RandomState(5).randn(4, 64, hw, hw).astype(f32)
    with options(cg, CG_NN_SPLITS=1, **FAMILIES[family], **NO_OTHER):
        bits, launches = planned_bits(cg, lambda: build(cg), x, fusion, seed=3)
        if fusion:
            _, unfused = planned_bits(cg, lambda: build(cg), x, 0, seed=3)
            print(f"epilogue {which} / {family}: {launches} forward launches fused, {unfused} unfused")
            assert launches < unfused, f"{which}: nothing was folded into the GEMM's epilogue ({launches} launches against {unfused})"
        check(golden, f"epilogue {which} / {family} / fusion {fusion}", *bits)


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("shape", [(64, 128, 8, 128, 7), (64, 32, 4, 64, 5)])
def test_position_major_rows_and_k_tiles(cg, golden, shape, splits):
    """igemm_nng_kernel<..., PM> (forward, data gradient) and igemm_tng_kernel mode 2 (weight gradient): unsplit the NN kernel stores
    through its position-major lean path, split its partials take the consecutive one."""
    N, Cin, H, Cout, k = shape
    with options(cg, CG_PAD_SKIP=1, CG_NN_TILE=64000 + (128 if Cout >= 128 else 64), CG_NN_SPLITS=splits, CG_TN_SPLITS=splits, **NO_OTHER):
        check(golden, f"position-major {shape} / splits {splits}", *conv_bits(cg, N, Cin, H, H, Cout, k, 0, seed=5 + k))


@pytest.mark.parametrize("N,i,o", [(64, 1024, 64), (5, 64, 4)])
def test_flat_tn_mode(cg, golden, N, i, o):
    """nn.Linear: the weight gradient is igemm_tng_kernel's flat mode at N = 64 and the register-staged kernel on the ragged N = 5."""
    rs = np.random.RandomState(N + i + o)
    m = cg.nn.Linear(i, o)
    m.weight.copy((rs.randn(o, i) / np.sqrt(i)).astype(f32)); m.bias.copy(rs.randn(o).astype(f32))
    x = cg.Tensor.from_numpy(rs.randn(N, i).astype(f32))
    y = m.forward(x).numpy().copy()
    m.gradWeight.zero(); m.gradBias.zero()
    gi = m.backward(x, cg.Tensor.from_numpy(rs.randn(N, o).astype(f32))).numpy().copy()
    check(golden, f"linear {N} x {i} -> {o}", y, gi, m.gradWeight.numpy(), m.gradBias.numpy())


@pytest.mark.parametrize("splits", [0, 1])
def test_grouped_launch(cg, golden, splits):
    """Three structurally identical conv 64 -> 64 -> PReLU branches under nn.Concat run as ONE grouped launch (blockIdx.z = branch):
    the four-pointer fields of the kernel arguments, with the plan's own split and unsplit (activation in the epilogue)."""
    def build():
        net = cg.nn.Sequential()
        cat = cg.nn.Concat(2)
        for _ in range(3):
            cat.add(cg.nn.Sequential().add(cg.nn.SpatialConvolution(64, 64, 3, 3, 1, 1, 1)).add(cg.nn.PReLU()))
        return net.add(cat)
    x = np.random.RandomState(12).randn(2, 64, 16, 16).astype(f32)
    with options(cg, CG_NN_SPLITS=splits, **NO_OTHER):
        check(golden, f"grouped branches / splits {splits}", *planned_bits(cg, build, x, 1, seed=12)[0])


@pytest.mark.parametrize("shape", [(2, 128, 32, 32, 3), (2, 64, 8, 8, 1)])
def test_valu_skinny_kernels(cg, golden, shape):
    """skinny_conv3x3_kernel / skinny_wgrad3x3_kernel (CG_SKINNY = 2: the VALU family wherever a skinny layer runs)."""
    N, Cin, H, W, Cout = shape
    with options(cg, CG_SKINNY=2):
        check(golden, f"skinny valu {shape}", *conv_bits(cg, N, Cin, H, W, Cout, 3, 0, seed=N + Cin + H + W + Cout))


# The finishes of the weight gradient (csrc/wgrad_finish.hip).  The cases above all land in the small forms with 1 or 3 splits; these reach
# the tiled kernels (Cin / 8 x Cout / 32 blocks, not fewer than the chip has CUs) and the long small forms, where a lane group adds more
# than one split.  (N, Cin, H, W, Cout, k, ups) and the forced TN split count; which kernels each launches: profiles/finish_cases_kernels.txt
FINISHES = {
    "tiled plain": ((2, 256, 8, 8, 256, 3, 0), 3),              # wgrad_reduce_kernel<false> + bias_part_reduce_kernel, 32 x 8 full blocks
    "tiled plain, ragged": ((2, 260, 8, 8, 250, 3, 0), 3),      # 33 x 8 blocks, guards in both dimensions
    "tiled ups": ((2, 256, 4, 4, 256, 3, 1), 3),                # wgrad_reduce_kernel<true> (M = 32 pixels per phase: the plan makes 2 splits of 3)
    "small v4, long": ((11, 64, 8, 8, 64, 3, 0), 44),           # M = 704 = 44 K tiles: lane group 0 adds 0, 8, 16, 24 in one round, then 32, 40
    "small scalar, long": ((11, 64, 8, 8, 6, 3, 0), 44),        # Cout % 4 != 0: the 32-element form and its bias blocks
    "small ups, long": ((11, 32, 8, 8, 8, 3, 1), 44),           # the phase fold with the eight-lane interleave
}


@pytest.mark.parametrize("finish", list(FINISHES))
def test_wgrad_finishes(cg, golden, finish):
    """Split-K partials -> canonical gradWeight / gradBias through each finish: tiled (splits in order, phases inside a split) and small
    (lane group ln adds splits ln, ln + 8, ..., then the groups in order)."""
    shape, splits = FINISHES[finish]
    with options(cg, CG_TN_SPLITS=splits, **NO_OTHER):
        check(golden, f"finish {finish} / splits {splits}", *conv_bits(cg, *shape, seed=len(finish)))


def test_deferred_transpose_and_v4_jobs(cg, golden):
    """Two linear layers through the planned executor queue their finishes and flush them in ONE wgrad_reduce_batch_kernel launch: the first
    (64 -> 32, both multiples of 32) as transpose tiles, the second (32 -> 4) as a 16-byte job.  CG_PAD_SKIP = 0 keeps headwg.hip out."""
    def build():
        return cg.nn.Sequential().add(cg.nn.Linear(64, 32)).add(cg.nn.LeakyReLU(0.2)).add(cg.nn.Linear(32, 4))
    x = np.random.RandomState(21).randn(64, 64).astype(f32)
    with options(cg, CG_PAD_SKIP=0, **NO_OTHER):
        check(golden, "deferred linear 64 -> 32 -> 4", *planned_bits(cg, build, x, 1, seed=21)[0])


def test_mfma_skinny_finish(cg, golden):
    """skinny.hip's MFMA weight gradient (CG_SKINNY = 1) leaves 256 partial planes and their bias partials to the small finish."""
    shape = (2, 128, 32, 32, 3)
    with options(cg, CG_SKINNY=1):
        check(golden, f"skinny mfma {shape}", *conv_bits(cg, *shape, 3, 0, seed=sum(shape)))
