"""The bilinear sampler of csrc/sampler.hip - bilinear_fwd_k<1|4>, the deterministic gather backward bilinear_bwd_det_k<G, CACC, VW> with its
whole-workgroup path for source pixels that collect more than kHeavy = 64 taps, the float-atomic fallback bilinear_bwd_k<G> and the
host dispatch behind cg_bilinear_sampler_{forward,backward}[_shared] - over its dispatch and value edges, through the C ABI, against
the fp64 restatement of tests/sampler_ref.py on the same fp32 inputs.

Every case states its regime in its table row (sampler_ref.describe of sampler_ref.sampler_plan: path, lane plan, chunk plan, LDS bytes,
forward kernel and grid regime); tests/test_sampler_ref_host.py asserts the same rows and the plan's constants without a GPU.  The
CG_SAMPLER_ATOMIC_LAUNCHES counter shows which backward ran: its delta is 0 for `det`, 1 for `atomic`.

Inputs live in guarded buffers (helpers.dev), outputs are prefilled with NaN - the gather backward has no memset, so a gimg element it
leaves unwritten fails - and the guards are checked after every call (helpers.host).  Grids are uniform in [-1.3, 1.3] with planted
values (make_grid): exactly -1 and +1 and the corners, nextafter of +-1 both ways, -0.0, +-3, +-1e6, +-1e30, pixel centres where
size - 1 is a power of two (there the fp32 taps return the cell exactly with weight exactly 1, asserted), and the last sample of every
case with two or more samples has every coordinate outside the image: its output, gimg slice and ggrid must be exact zeros.

Two measures, per element, none scaled by a maximum: equality where the result is exact (numeric: a -0.0 product may meet a +0.0
accumulator), and helpers.rounding_close with r = the fp32 roundings on the longest chain of the kernel's expression + 2:
  out    bilinear_fwd_k's four tap() calls: tap 00 - its weight's product 1, the product with img 1, four sums 4 - or tap 01 -
         1 - wx0 and the weight's product 2, the product with img 1, three sums 3: 6, + 2 = 8
  ggrid  the channel dot of a lane (`d00 += ...` in part (A) of bilinear_bwd_det_k / the channel loop of bilinear_bwd_k): 4 for a
         float4 lane (V::dot: a product and three sums, added to an exact zero), 2 CACC for a scalar lane of the gather form,
         2 ceil(C / G) for the atomic form; log2 G shuffle sums; then `gy = -wx0 * d00 + ...`: 1 - wx0 off the longest chain, a product
         and three sums 4; `* (float)(Hi - 1)` 1, `* 0.5f` exact: lane + log2 G + 5, + 2
  gimg   T = the taps that meet at the source pixel (sampler_ref.backward's count, equal to heavy_pixels).  The weight `wx * wy` with
         both factors formed as 1 - w: 3, the product with gout 1, then the sums: T on the light path (one chain, `V::fma(acc[k], w[u],
         g[u][k])`; the padding adds exact zeros), ceil(T / ngrp) + ngrp on the heavy path (a lane group's share, then the group sum
         `V::fma(tot[k], 1.f, ...)` over ngrp partials): sums + 4, + 2.  The atomic path gets the order-free T + 4, + 2.
Only the gather path is additionally asserted bit-equal over two runs.

Worst |d| / bound measured on the MI355X, per buffer and path (every case of this file; 1.0 is the bound):
  path     out     ggrid   gimg    gimg where a pixel is heavy
  det      0.463   0.323   0.349   0.185        (59 cases; 6 of them with source pixels of more than 64 taps)
  atomic   0.434   0.279   0.358   -            (8 cases)"""
import importlib

import numpy as np
import pytest
import torch

import sampler_ref as R
from helpers import counter, dev, edge_normal, host, out_like, rounding_close

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
COUNTER = "CG_SAMPLER_ATOMIC_LAUNCHES"

# id, N (samples), Nimg (images: N > Nimg runs the shared forms with N / Nimg groups), (Hi, Wi, Ho, Wo), C, every tensor 4 bytes off
# its 16-byte boundary, the grid alone off (None: as the tensors), the grid builder of the heavy cases, and the regime
CASES = [
    ("channels-1", 2, 2, (5, 9, 7, 4), 1, False, None, None,
     "det scalar G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=3220 | bilinear_fwd_k<1> one"),
    ("channels-2", 2, 2, (5, 9, 7, 4), 2, False, None, None,
     "det scalar G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=3220 | bilinear_fwd_k<1> one"),
    ("channels-3", 2, 2, (5, 9, 7, 4), 3, False, None, None,
     "det scalar G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=3220 | bilinear_fwd_k<1> one"),
    ("channels-4", 2, 2, (5, 9, 7, 4), 4, False, None, None,
     "det v4 G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=6292 | bilinear_fwd_k<4> one"),
    ("channels-5", 2, 2, (5, 9, 7, 4), 5, False, None, None,
     "det scalar G=8 CACC=1 idle-lanes want=16 S=32 chunks=2 ragged ngrp=32 lds=3220 | bilinear_fwd_k<1> many"),
    ("channels-8", 2, 2, (5, 9, 7, 4), 8, False, None, None,
     "det v4 G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=6292 | bilinear_fwd_k<4> one"),
    ("channels-17", 2, 2, (5, 9, 7, 4), 17, False, None, None,
     "det scalar G=32 CACC=1 idle-lanes want=16 S=32 chunks=2 ragged ngrp=8 lds=3220 | bilinear_fwd_k<1> many"),
    ("channels-20", 2, 2, (5, 9, 7, 4), 20, False, None, None,
     "det v4 G=8 CACC=1 idle-lanes want=16 S=32 chunks=2 ragged ngrp=32 lds=6292 | bilinear_fwd_k<4> many"),
    ("channels-63", 2, 2, (5, 9, 7, 4), 63, False, None, None,
     "det scalar G=64 CACC=1 idle-lanes want=16 S=32 chunks=2 ragged ngrp=4 lds=3220 | bilinear_fwd_k<1> many"),
    ("channels-64", 2, 2, (5, 9, 7, 4), 64, False, None, None,
     "det v4 G=16 CACC=1 want=16 S=32 chunks=2 ragged ngrp=16 lds=6292 | bilinear_fwd_k<4> many"),
    ("channels-65", 2, 2, (5, 9, 7, 4), 65, False, None, None,
     "det scalar G=64 CACC=2 idle-lanes want=16 S=32 chunks=2 ragged ngrp=4 lds=4244 | bilinear_fwd_k<1> many"),
    ("channels-68", 2, 2, (5, 9, 7, 4), 68, False, None, None,
     "det v4 G=32 CACC=1 idle-lanes want=16 S=32 chunks=2 ragged ngrp=8 lds=6292 | bilinear_fwd_k<4> many"),
    ("channels-128", 2, 2, (5, 9, 7, 4), 128, False, None, None,
     "det v4 G=32 CACC=1 want=16 S=32 chunks=2 ragged ngrp=8 lds=6292 | bilinear_fwd_k<4> many"),
    ("channels-129", 2, 2, (5, 9, 7, 4), 129, False, None, None,
     "det scalar G=64 CACC=4 idle-lanes want=16 S=32 chunks=2 ragged ngrp=4 lds=6292 | bilinear_fwd_k<1> many"),
    ("channels-252", 2, 2, (5, 9, 7, 4), 252, False, None, None,
     "det v4 G=64 CACC=1 idle-lanes want=16 S=32 chunks=2 ragged ngrp=4 lds=6292 | bilinear_fwd_k<4> many"),
    ("channels-256", 2, 2, (5, 9, 7, 4), 256, False, None, None,
     "det v4 G=64 CACC=1 want=16 S=32 chunks=2 ragged ngrp=4 lds=6292 | bilinear_fwd_k<4> many"),
    ("channels-4-off", 2, 2, (5, 9, 7, 4), 4, True, None, None,
     "det scalar G=4 CACC=1 want=16 S=64 chunks=1 ragged ngrp=64 lds=3220 | bilinear_fwd_k<1> one"),
    ("channels-64-off", 2, 2, (5, 9, 7, 4), 64, True, None, None,
     "det scalar G=64 CACC=1 want=16 S=32 chunks=2 ragged ngrp=4 lds=3220 | bilinear_fwd_k<1> many"),
    ("channels-256-off", 2, 2, (5, 9, 7, 4), 256, True, None, None,
     "det scalar G=64 CACC=4 want=16 S=32 chunks=2 ragged ngrp=4 lds=6292 | bilinear_fwd_k<1> many"),
    ("channels-257-atomic", 2, 2, (5, 9, 7, 4), 257, False, None, None,
     "atomic(C) G=64 blocks=14 | bilinear_fwd_k<1> many"),
    ("channels-260-atomic", 2, 2, (5, 9, 7, 4), 260, False, None, None,
     "atomic(C) G=64 blocks=14 | bilinear_fwd_k<4> many"),
    ("shared-3", 6, 2, (5, 9, 7, 4), 3, False, None, None,
     "det scalar G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=3220 | bilinear_fwd_k<1> many"),
    ("shared-4", 6, 2, (5, 9, 7, 4), 4, False, None, None,
     "det v4 G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=6292 | bilinear_fwd_k<4> one"),
    ("shared-64-off", 6, 2, (5, 9, 7, 4), 64, True, None, None,
     "det scalar G=64 CACC=1 want=16 S=32 chunks=2 ragged ngrp=4 lds=3220 | bilinear_fwd_k<1> many"),
    ("shared-65", 6, 2, (5, 9, 7, 4), 65, False, None, None,
     "det scalar G=64 CACC=2 idle-lanes want=16 S=32 chunks=2 ragged ngrp=4 lds=4244 | bilinear_fwd_k<1> many"),
    ("shared-257", 6, 2, (5, 9, 7, 4), 257, False, None, None,
     "atomic(C) G=64 blocks=42 | bilinear_fwd_k<1> many"),
    ("geom-1x1x3x3-N2-C3", 2, 2, (1, 1, 3, 3), 3, False, None, None,
     "det scalar G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=2316 | bilinear_fwd_k<1> one"),
    ("geom-1x1x3x3-N2-C4", 2, 2, (1, 1, 3, 3), 4, False, None, None,
     "det v4 G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=5388 | bilinear_fwd_k<4> one"),
    ("geom-1x6x4x4-N2-C3", 2, 2, (1, 6, 4, 4), 3, False, None, None,
     "det scalar G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=2564 | bilinear_fwd_k<1> one"),
    ("geom-1x6x4x4-N2-C4", 2, 2, (1, 6, 4, 4), 4, False, None, None,
     "det v4 G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=5636 | bilinear_fwd_k<4> one"),
    ("geom-6x1x4x4-N2-C3", 2, 2, (6, 1, 4, 4), 3, False, None, None,
     "det scalar G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=2564 | bilinear_fwd_k<1> one"),
    ("geom-6x1x4x4-N2-C4", 2, 2, (6, 1, 4, 4), 4, False, None, None,
     "det v4 G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=5636 | bilinear_fwd_k<4> one"),
    ("geom-5x9x1x1-N2-C3", 2, 2, (5, 9, 1, 1), 3, False, None, None,
     "det scalar G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=2572 | bilinear_fwd_k<1> one"),
    ("geom-5x9x1x1-N2-C4", 2, 2, (5, 9, 1, 1), 4, False, None, None,
     "det v4 G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=5644 | bilinear_fwd_k<4> one"),
    ("geom-9x5x4x7-N2-C3", 2, 2, (9, 5, 4, 7), 3, False, None, None,
     "det scalar G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=3220 | bilinear_fwd_k<1> one"),
    ("geom-9x5x4x7-N2-C4", 2, 2, (9, 5, 4, 7), 4, False, None, None,
     "det v4 G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=6292 | bilinear_fwd_k<4> one"),
    ("geom-4x7x9x5-N2-C3", 2, 2, (4, 7, 9, 5), 3, False, None, None,
     "det scalar G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=3468 | bilinear_fwd_k<1> many"),
    ("geom-4x7x9x5-N2-C4", 2, 2, (4, 7, 9, 5), 4, False, None, None,
     "det v4 G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ragged ngrp=64 lds=6540 | bilinear_fwd_k<4> one"),
    ("geom-16x16x16x16-N2-C3", 2, 2, (16, 16, 16, 16), 3, False, None, None,
     "det scalar G=4 CACC=1 idle-lanes want=16 S=64 chunks=4 ngrp=64 lds=10524 | bilinear_fwd_k<1> many"),
    ("geom-16x16x16x16-N2-C4", 2, 2, (16, 16, 16, 16), 4, False, None, None,
     "det v4 G=4 CACC=1 idle-lanes want=16 S=64 chunks=4 ngrp=64 lds=13596 | bilinear_fwd_k<4> many"),
    ("geom-33x33x33x33-N1-C3", 1, 1, (33, 33, 33, 33), 3, False, None, None,
     "det scalar G=4 CACC=1 idle-lanes want=16 S=69 chunks=16 ragged ngrp=64 lds=37452 | bilinear_fwd_k<1> many"),
    ("geom-33x33x33x33-N1-C4", 1, 1, (33, 33, 33, 33), 4, False, None, None,
     "det v4 G=4 CACC=1 idle-lanes want=16 S=69 chunks=16 ragged ngrp=64 lds=40524 | bilinear_fwd_k<4> many"),
    ("geom-33x33x33x33-N1-C64-off", 1, 1, (33, 33, 33, 33), 64, True, None, None,
     "det scalar G=64 CACC=1 want=16 S=69 chunks=16 ragged ngrp=4 lds=37452 | bilinear_fwd_k<1> many"),
    ("geom-33x33x33x33-N2-C3", 2, 2, (33, 33, 33, 33), 3, False, None, None,
     "det scalar G=4 CACC=1 idle-lanes want=16 S=69 chunks=16 ragged ngrp=64 lds=37452 | bilinear_fwd_k<1> many"),
    ("geom-33x33x33x33-N2-C4", 2, 2, (33, 33, 33, 33), 4, False, None, None,
     "det v4 G=4 CACC=1 idle-lanes want=16 S=69 chunks=16 ragged ngrp=64 lds=40524 | bilinear_fwd_k<4> many"),
    ("geom-33x33x33x33-N2-C64-off", 2, 2, (33, 33, 33, 33), 64, True, None, None,
     "det scalar G=64 CACC=1 want=16 S=69 chunks=16 ragged ngrp=4 lds=37452 | bilinear_fwd_k<1> many"),
    ("geom-66x66x66x66-N2-C3", 2, 2, (66, 66, 66, 66), 3, False, None, None,
     "det scalar G=4 CACC=1 idle-lanes want=16 S=273 chunks=16 ragged ngrp=64 lds=142524 | bilinear_fwd_k<1> many"),
    ("geom-66x66x66x66-N2-C4", 2, 2, (66, 66, 66, 66), 4, False, None, None,
     "det v4 G=4 CACC=1 idle-lanes want=16 S=273 chunks=16 ragged ngrp=64 lds=145596 | bilinear_fwd_k<4> many"),
    ("geom-67x67x67x67-N2-C3", 2, 2, (67, 67, 67, 67), 3, False, None, None,
     "atomic(lds) G=4 blocks=141 | bilinear_fwd_k<1> many"),
    ("geom-67x67x67x67-N2-C4", 2, 2, (67, 67, 67, 67), 4, False, None, None,
     "atomic(lds) G=4 blocks=141 | bilinear_fwd_k<4> many"),
    ("geom-66x66x70x64-N2-C3", 2, 2, (66, 66, 70, 64), 3, False, None, None,
     "atomic(lds) G=4 blocks=140 | bilinear_fwd_k<1> many"),
    ("geom-66x66x70x64-N2-C4", 2, 2, (66, 66, 70, 64), 4, False, None, None,
     "atomic(lds) G=4 blocks=140 | bilinear_fwd_k<4> many"),
    ("chunks-N1", 1, 1, (8, 8, 8, 8), 4, False, None, None,
     "det v4 G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ngrp=64 lds=7324 | bilinear_fwd_k<4> one"),
    ("chunks-N70", 70, 70, (8, 8, 8, 8), 4, False, None, None,
     "det v4 G=4 CACC=1 idle-lanes want=14 S=64 chunks=1 ngrp=64 lds=7324 | bilinear_fwd_k<4> many"),
    ("chunks-N300", 300, 300, (8, 8, 8, 8), 4, False, None, None,
     "det v4 G=4 CACC=1 idle-lanes want=3 S=64 chunks=1 ngrp=64 lds=7324 | bilinear_fwd_k<4> many"),
    ("chunks-N1100", 1100, 1100, (8, 8, 8, 8), 4, False, None, None,
     "det v4 G=4 CACC=1 idle-lanes want=1 S=64 chunks=1 ngrp=64 lds=7324 | bilinear_fwd_k<4> many"),
    ("heavy-64-light", 3, 3, (5, 5, 8, 8), 3, False, None, 'cell64',
     "det scalar G=4 CACC=1 idle-lanes want=16 S=64 chunks=1 ngrp=64 lds=3892 | bilinear_fwd_k<1> many"),
    ("heavy-65", 3, 3, (5, 5, 5, 13), 3, False, None, 'cell65',
     "det scalar G=4 CACC=1 idle-lanes want=16 S=64 chunks=2 ragged ngrp=64 lds=3916 | bilinear_fwd_k<1> many"),
    ("heavy-four-buckets-C3", 3, 3, (5, 5, 5, 13), 3, False, None, 'four',
     "det scalar G=4 CACC=1 idle-lanes want=16 S=64 chunks=2 ragged ngrp=64 lds=3916 | bilinear_fwd_k<1> many"),
    ("heavy-four-buckets-C8", 3, 3, (5, 5, 5, 13), 8, False, None, 'four',
     "det v4 G=4 CACC=1 idle-lanes want=16 S=64 chunks=2 ragged ngrp=64 lds=6988 | bilinear_fwd_k<4> many"),
    ("heavy-1024-C3", 3, 3, (5, 5, 32, 32), 3, False, None, 'cell1024',
     "det scalar G=4 CACC=1 idle-lanes want=16 S=64 chunks=16 ngrp=64 lds=26932 | bilinear_fwd_k<1> many"),
    ("heavy-1024-C64-off", 3, 3, (5, 5, 32, 32), 64, True, None, 'cell1024',
     "det scalar G=64 CACC=1 want=16 S=64 chunks=16 ngrp=4 lds=26932 | bilinear_fwd_k<1> many"),
    ("heavy-two-in-a-row", 3, 3, (5, 5, 10, 13), 3, False, None, 'pair',
     "det scalar G=4 CACC=1 idle-lanes want=16 S=64 chunks=3 ragged ngrp=64 lds=5476 | bilinear_fwd_k<1> many"),
    ("wrap-forward-scalar", 22, 22, (64, 64, 64, 64), 3, False, None, None,
     "det scalar G=4 CACC=1 idle-lanes want=16 S=256 chunks=16 ngrp=64 lds=134172 | bilinear_fwd_k<1> wrap"),
    ("wrap-forward-float4", 5, 5, (64, 64, 64, 64), 64, False, None, None,
     "det v4 G=16 CACC=1 want=16 S=256 chunks=16 ngrp=16 lds=137244 | bilinear_fwd_k<4> wrap"),
    ("wrap-forward-grid-off", 5, 5, (64, 64, 64, 64), 64, False, True, None,
     "det v4 G=16 CACC=1 want=16 S=256 chunks=16 ngrp=16 lds=137244 | bilinear_fwd_k<1> wrap"),
    ("wrap-atomic", 3, 3, (64, 64, 64, 64), 257, False, None, None,
     "atomic(C) G=64 blocks=2048 wraps | bilinear_fwd_k<1> wrap"),
]
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def cg():
    mod = importlib.import_module("cat-generator_amd")
    assert torch.cuda.is_available(), "these tests need the MI355X"
    mod.lib()  # fails loudly if the HIP extension is missing
    return mod


# ------------------------------------------------------------------------------ grids
def pow2(k):
    return k >= 1 and k & (k - 1) == 0


def centre(k, size):
    """The coordinate of pixel k's centre, exact in fp32 where size - 1 is a power of two."""
    return f32(2.0 * k / (size - 1) - 1.0)


def outside_values(rng, size, n):
    """n coordinates with no tap on an axis of `size` > 1 pixels: below -1 - 2 / (size - 1) the right tap is outside too, from
    1 + 2 / (size - 1) up the left one is."""
    hi = 1.0 + 2.0 / (size - 1)
    vals = np.array([hi * 1.01, -hi * 1.01, hi * 1.25 + 0.5, -hi * 1.25 - 0.5, 3.0 * hi, -3.0 * hi, 1e6, -1e6, 1e30, -1e30], f32)
    return vals[rng.integers(0, vals.size, n)]


def make_grid(rng, N, Hi, Wi, Ho, Wo):
    """-> grid [N][Ho][Wo][2] (y, x), and the planted pixels whose two coordinates are pixel centres: (n, flat pixel, ky, kx).
    The plants go to the first, the last and random pixels of the samples before the all-outside one; a case with fewer pixels than
    three times the plants takes a random subset of them (the seeds differ per case, the larger cases take all)."""
    g = rng.uniform(-1.3, 1.3, (N, Ho, Wo, 2)).astype(f32)
    P = Ho * Wo
    live = N - 1 if N >= 2 and max(Hi, Wi) > 1 else N
    if live < N:
        for axis, size in ((0, Hi), (1, Wi)):
            if size > 1:
                g[live:, :, :, axis] = outside_values(rng, size, (N - live) * P).reshape(N - live, Ho, Wo)
    one = f32(1)
    near = [np.nextafter(one, f32(2)), np.nextafter(one, f32(0)), np.nextafter(-one, f32(-2)), np.nextafter(-one, f32(0))]
    plants = [(v, None) for v in (-one, one)] + [(None, v) for v in (-one, one)] + [(-one, one), (one, -one)]
    for v in near + [f32(-0.0), f32(3), f32(-3), f32(1e6), f32(-1e6), f32(1e30), f32(-1e30)]:
        plants += [(v, None), (None, v)]
    py, px = pow2(Hi - 1), pow2(Wi - 1)
    for ky, kx in ((0, Wi - 1), (Hi - 1, 0), (int(rng.integers(0, Hi)), int(rng.integers(0, Wi)))):
        if py or px:
            plants.append((centre(ky, Hi) if py else None, centre(kx, Wi) if px else None, ky, kx))
    flat = g[:live].reshape(live * P, 2)
    npx = flat.shape[0]
    k = min(len(plants), max(1, npx // 3))
    pick = [plants[i] for i in rng.permutation(len(plants))[:k]]
    pos = [int(p) for p in rng.permutation(npx)[:k] if p not in (0, npx - 1)]
    fixed = [(0, (-one, -one)), (npx - 1, (one, one))]           # two of the corners at the first and the last pixel
    centres = []
    for p, pl in fixed + list(zip(pos, pick)):
        if pl[0] is not None:
            flat[p, 0] = pl[0]
        if pl[1] is not None:
            flat[p, 1] = pl[1]
        if len(pl) == 4:
            y0, x0, wy0, wx0, _ = R.bilin_taps(flat[p:p + 1], Hi, Wi)
            if py:
                assert y0[0] == pl[2] and wy0[0] == 1.0, "the fp32 taps of a pixel centre: the cell itself, weight 1"
            if px:
                assert x0[0] == pl[3] and wx0[0] == 1.0, "the fp32 taps of a pixel centre: the cell itself, weight 1"
            if py and px:
                centres.append((p // P, p % P, pl[2], pl[3]))
    g[:live] = flat.reshape(live, Ho, Wo, 2)
    return g, centres


def in_cell(rng, cy, cx, n, Hi, Wi):
    """n (y, x) coordinates strictly inside the cell whose top-left pixel is (cy, cx) (cy = -1: the half cell above row 0)."""
    yc, xc = rng.uniform(cy + 0.05, cy + 0.95, n), rng.uniform(cx + 0.05, cx + 0.95, n)
    return np.stack([2.0 * yc / (Hi - 1) - 1.0, 2.0 * xc / (Wi - 1) - 1.0], -1).astype(f32)


def heavy_grid(kind, rng, g, Hi, Wi):
    """Sample 0 of g rebuilt on the host for a 5 x 5 image; asserts the tap totals it is meant to produce with heavy_pixels."""
    P = g.shape[1] * g.shape[2]
    if kind in ("cell64", "cell65", "cell1024"):
        s0 = in_cell(rng, 1, 1, P, Hi, Wi)
        want = {(1, 1): P, (1, 2): P, (2, 1): P, (2, 2): P}
        assert P == int(kind[4:])
    elif kind == "four":                                          # source pixel (2, 2) collects 20 + 20 + 20 + 5 from its four buckets
        s0 = np.concatenate([in_cell(rng, 1, 1, 20, Hi, Wi), in_cell(rng, 1, 2, 20, Hi, Wi), in_cell(rng, 2, 1, 20, Hi, Wi),
                             in_cell(rng, 2, 2, 5, Hi, Wi)])
        s0 = s0[rng.permutation(65)]
        want = {(2, 2): 65, (1, 1): 20, (1, 2): 40, (2, 1): 40, (2, 3): 25, (3, 2): 25, (3, 3): 5, (1, 3): 20, (3, 1): 20}
    else:                                                         # "pair": 70 taps from the half cell above pixels (0, 1) and (0, 2)
        assert kind == "pair"
        s0 = g[0].reshape(P, 2).copy()
        s0[:70] = in_cell(rng, -1, 1, 70, Hi, Wi)
        s0 = s0[rng.permutation(P)]
        want = None
    g[0] = s0.reshape(g.shape[1:])
    hp = R.heavy_pixels(g, Hi, Wi)
    if want is not None:
        assert {(y, x): int(hp[0, y, x]) for y in range(Hi) for x in range(Wi) if hp[0, y, x]} == want
    else:
        heavy = [int(q) for q in np.flatnonzero(hp[0].ravel() > R.HEAVY)]
        assert heavy == [1, 2], "two heavy source pixels in a row, the rest light"
        assert ((hp[0].ravel() > 0) & (hp[0].ravel() <= R.HEAVY)).sum() >= 10
    return g


def case_inputs(id_, N, Nimg, geom, C, special):
    Hi, Wi, Ho, Wo = geom
    rng = np.random.default_rng(1000 * IDS.index(id_) + C)
    img = edge_normal(rng, (Nimg, Hi, Wi, C))
    gout = edge_normal(rng, (N, Ho, Wo, C))
    grid, centres = make_grid(rng, N, Hi, Wi, Ho, Wo)
    if special:
        grid, centres = heavy_grid(special, rng, grid, Hi, Wi), [c for c in centres if c[0] != 0]
    return img, gout, grid, centres


def log2(G):
    return G.bit_length() - 1


# ------------------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("id_,N,Nimg,geom,C,mis,grid_mis,special,regime", CASES, ids=IDS)
def test_sampler_over_dispatch_and_value_edges(cg, id_, N, Nimg, geom, C, mis, grid_mis, special, regime):
    L, st = cg.lib(), cg.tensor.stream()
    Hi, Wi, Ho, Wo = geom
    plan = R.sampler_plan(N, Nimg, Hi, Wi, C, Ho, Wo, not mis, None if grid_mis is None else not grid_mis)
    assert R.describe(plan) == regime
    B = plan["backward"]
    det = B["path"] == "det"
    img, gout, grid, centres = case_inputs(id_, N, Nimg, geom, C, special)
    ref_out, out_terms = R.forward(img, grid)
    ref = R.backward(img, grid, gout)
    T = ref["taps"]
    assert np.array_equal(T, R.heavy_pixels(grid, Hi, Wi))
    zero = N - 1 if N >= 2 and max(Hi, Wi) > 1 else None        # the all-outside sample
    if zero is not None:
        assert T[zero].sum() == 0 and T[:zero].sum() > 0
    if special and special != "cell64":
        assert (T > R.HEAVY).any() and det
    nan = float("nan")
    ti, tg, to = dev(img, mis), dev(grid, mis if grid_mis is None else grid_mis), dev(gout, mis)
    p = lambda t: t.data_ptr()
    groups = N // Nimg
    assert groups * Nimg == N

    def forward():
        out = out_like(N * Ho * Wo * C, mis, nan)
        if groups == 1:
            L.bilinear_sampler_forward(st, p(ti), p(tg), p(out), N, Hi, Wi, C, Ho, Wo)
        else:
            L.bilinear_sampler_forward_shared(st, groups, p(ti), p(tg), p(out), Nimg, Hi, Wi, C, Ho, Wo)
        return host(out, (N, Ho, Wo, C))

    def backward():
        gimg, ggrid = out_like(N * Hi * Wi * C, mis, nan), out_like(N * Ho * Wo * 2, mis, nan)
        before = counter(cg, COUNTER)
        if groups == 1:
            L.bilinear_sampler_backward(st, p(ti), p(tg), p(to), p(gimg), p(ggrid), N, Hi, Wi, C, Ho, Wo)
        else:
            L.bilinear_sampler_backward_shared(st, groups, p(ti), p(tg), p(to), p(gimg), p(ggrid), Nimg, Hi, Wi, C, Ho, Wo)
        assert counter(cg, COUNTER) - before == (0 if det else 1), f"{id_}: the case names the {B['path']} path"
        return host(gimg, (N, Hi, Wi, C)), host(ggrid, (N, Ho, Wo, 2))

    out = forward()
    gimg, ggrid = backward()
    for t in (ti, tg, to):
        host(t)                                                  # the guards around the inputs
    path = B["path"]
    rounding_close(out, ref_out, out_terms, 8, f"{path} out")
    G = B["G"]
    lane = (4 if B["v4"] else 2 * B["CACC"]) if det else 2 * -(-C // G)
    rounding_close(ggrid, ref["ggrid"], ref["ggrid_terms"], lane + log2(G) + 5 + 2, f"{path} ggrid")
    if det:
        ngrp = B["ngrp"]
        sums = np.where(T > R.HEAVY, -(-T // ngrp) + ngrp, T)
        heavy = bool((T > R.HEAVY).any())
    else:
        sums, heavy = T, False
    rounding_close(gimg, ref["gimg"], ref["gimg_terms"], (sums + 4 + 2)[..., None], f"{path}{' heavy' if heavy else ''} gimg")
    # ---- exact results
    if zero is not None:
        assert (out[zero] == 0).all() and (gimg[zero] == 0).all() and (ggrid[zero] == 0).all(), "a sample without a tap: exact zeros"
    assert (gimg[T == 0] == 0).all(), "a source pixel no tap reaches is written as zeros"
    if Hi == 1:
        assert (ggrid[..., 0] == 0).all(), "Hi - 1 = 0: no gradient along y"
    if Wi == 1:
        assert (ggrid[..., 1] == 0).all(), "Wi - 1 = 0: no gradient along x"
    for n, pix, ky, kx in centres:                               # weight exactly 1 on one pixel, exactly 0 on its neighbours
        assert np.array_equal(out[n].reshape(Ho * Wo, C)[pix], img[n % Nimg, ky, kx]), "a sample on a pixel centre returns the pixel"
    if det:                                                      # the gather form is reproducible
        gimg2, ggrid2 = backward()
        assert np.array_equal(gimg.view(np.uint32), gimg2.view(np.uint32)) and np.array_equal(ggrid.view(np.uint32), ggrid2.view(np.uint32))
