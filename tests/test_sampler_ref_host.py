"""tests/sampler_ref.py checked on its own, without a GPU: the fp64 restatement (taps="f64") against torch's fp64 grid_sample and its
autograd, the fp32 taps the GPU sweep compares with against the fp64 taps, the plan's constants against the source, and every case of
tests/test_gpu_sampler_edges.py against the regime its table row states."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sampler_ref as R
import test_gpu_sampler_edges as E

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U24 = 2.0 ** -24


def torch_sampler(img, grid, gout):
    """F.grid_sample works on NCHW images and (x, y) grids; ours are NHWC and (y, x).  Sample n reads image n % Nimg."""
    N, Nimg = grid.shape[0], img.shape[0]
    ti = torch.tensor(np.asarray(img, f64), requires_grad=True)
    tg = torch.tensor(np.asarray(grid, f64), requires_grad=True)
    x = ti[torch.arange(N) % Nimg].permute(0, 3, 1, 2)
    out = F.grid_sample(x, tg.flip(-1), mode="bilinear", padding_mode="zeros", align_corners=True).permute(0, 2, 3, 1)
    out.backward(torch.tensor(np.asarray(gout, f64)))
    return out.detach().numpy(), ti.grad.numpy(), tg.grad.numpy()


def planted_grid(rs, N, Ho, Wo):
    g = rs.uniform(-1.3, 1.3, (N, Ho, Wo, 2)).astype(f32)
    flat = g.reshape(-1)
    vals = np.array([1, -1, 3, -3, 1e30, -1e30], f32)
    flat[rs.permutation(flat.size)[:2 * vals.size]] = np.tile(vals, 2)
    flat[:2] = -1
    flat[-2:] = 1
    return g


# N, Nimg, Hi, Wi, C, Ho, Wo: non-square, P != Q both ways, one-pixel axes, shared images
TORCH_CASES = [(2, 2, 5, 9, 3, 7, 4), (3, 3, 9, 5, 4, 4, 7), (2, 2, 4, 7, 5, 9, 5), (6, 2, 5, 9, 3, 7, 4), (4, 2, 6, 6, 2, 3, 8),
               (2, 2, 1, 6, 3, 4, 4), (2, 2, 6, 1, 3, 4, 4), (2, 1, 16, 16, 8, 16, 16)]


@pytest.mark.parametrize("N,Nimg,Hi,Wi,C,Ho,Wo", TORCH_CASES)
def test_fp64_taps_equal_torch_grid_sample_and_its_autograd(N, Nimg, Hi, Wi, C, Ho, Wo):
    rs = np.random.RandomState(N * 100 + Hi * 10 + Wo)
    img = rs.randn(Nimg, Hi, Wi, C).astype(f32)
    gout = rs.randn(N, Ho, Wo, C).astype(f32)
    grid = planted_grid(rs, N, Ho, Wo)
    out, terms = R.forward(img, grid, taps="f64")
    B = R.backward(img, grid, gout, taps="f64")
    t_out, t_gimg, t_ggrid = torch_sampler(img, grid, gout)
    # the shared form keeps gimg per sample; torch's autograd sums the samples that read one image
    gimg = B["gimg"].reshape(N // Nimg, Nimg, Hi, Wi, C).sum(0)
    gterms = B["gimg_terms"].reshape(N // Nimg, Nimg, Hi, Wi, C).sum(0)
    for a, b, t, what in ((out, t_out, terms, "out"), (gimg, t_gimg, gterms, "gimg"), (B["ggrid"], t_ggrid, B["ggrid_terms"], "ggrid")):
        d = np.abs(a - b)
        assert a.shape == b.shape and (d <= 1e-12 * t + 1e-300).all(), f"{what}: max |d| / terms = {(d / (t + 1e-300)).max():.3e}"
    assert (terms >= np.abs(out) * (1 - 1e-12)).all() and (gterms >= np.abs(gimg) * (1 - 1e-12)).all()
    assert (B["ggrid_terms"] >= np.abs(B["ggrid"]) * (1 - 1e-12)).all()
    assert np.array_equal(R.backward(img, grid, gout)["taps"], R.heavy_pixels(grid, Hi, Wi))


def test_fp32_taps_against_fp64_taps():
    """Where the two agree on the cell the weights differ by four fp32 roundings: x + 1 and its product with W - 1 (each at most
    2^-24 of |xc|; the half is exact), xc - floor(xc) (exact for xc >= 0, where the fraction is a multiple of xc's ulp below 1; for xc in
    (-1, 0) the floor is -1 and xc + 1 rounds: at most 2^-24) and 1 - fraction (at most 2^-24, the result is at most 1):
    |w32 - w64| <= (2 |xc| + 2) 2^-24.  The cells disagree only where xc lies within the first two roundings of an integer.  The share of
    such points among 200 000 uniform ones in [-1.3, 1.3] per width is printed (with this seed 0 for the widths 5, 16, 33, 64 and 67; a
    few per million were seen for 67 with other seeds); above 1e-4 this fails.  It is a statement about the reference: the GPU sweep
    excludes nothing, it compares with the fp32 cells."""
    rs = np.random.RandomState(11)
    for W in (5, 16, 33, 64, 67):
        g = rs.uniform(-1.3, 1.3, (1, 1, 200000, 2)).astype(f32)
        y32, x32, wy32, wx32, _ = R.bilin_taps(g, W, W)
        y64, x64, wy64, wx64, _ = R.bilin_taps(g, W, W, taps="f64")
        differ = (x32 != x64) | (y32 != y64)
        share = differ.mean()
        print(f"width {W}: the fp32 and fp64 cells differ at {share:.2e} of the points")
        assert share <= 1e-4
        # bilin_taps clips the cell to [-2, size]: at the clip two different outside cells look alike, and no tap is taken from either
        for w32, w64, c, same in ((wx32, wx64, g[..., 1], (x32 == x64) & (x32 > -2) & (x32 < W)), (wy32, wy64, g[..., 0], (y32 == y64) & (y32 > -2) & (y32 < W))):
            xc = np.abs((c.astype(f64) + 1) * (W - 1) * 0.5)
            assert (np.abs(w32 - w64)[same] <= ((2 * xc + 2) * U24 * (1 + 1e-6))[same]).all()
        # where they differ, xc sits on the boundary: one of them has weight ~1 on the cell the other gives weight ~0 on
        assert (np.minimum(wx32, 1 - wx32)[x32 != x64] <= 4 * W * U24).all()


def test_the_plan_uses_the_constants_of_the_source():
    common = open(os.path.join(ROOT, "cat-generator_amd", "csrc", "common.h")).read()
    ops = open(os.path.join(ROOT, "cat-generator_amd", "csrc", "sampler.hip")).read()
    k = {n: int(re.search(rf"\b{n} = (\d+)", common).group(1)) for n in ("kNumCU", "kEwWgsPerCU")}
    assert (R.NUM_CU, R.EW_WGS_PER_CU) == (k["kNumCU"], k["kEwWgsPerCU"])
    body = ops[ops.index("int sampler_backward("):ops.index("int cg_bilinear_sampler_forward(")]
    m = re.search(r"shb <= (\d+) \* (\d+) && C <= (\d+)", body)
    assert int(m.group(1)) * int(m.group(2)) == R.DET_LDS_LIMIT and int(m.group(3)) == R.DET_MAX_C
    assert int(re.search(r"blocks > cg::kNumCU \* (\d+)\) blocks = cg::kNumCU \* (\d+)", body).group(1)) == R.ATOMIC_BLOCKS_PER_CU
    assert int(re.search(r"constexpr int kHeavy = (\d+)", ops).group(1)) == R.HEAVY
    assert re.search(r"shb = \(\(size_t\)6 \* P \+ 2 \* \(\(size_t\)\(Hi \+ 1\) \* \(Wi \+ 1\)\) \+ 1\) \* 4", body), "the LDS need sampler_plan restates"
    assert "std::min(16, (int)(cg::kNumCU * 4 / std::max(1, N)))" in body and "std::max(std::max(32, 256 / G), cg::cdiv(std::max(P, Q), want))" in body
    assert "cg::opt_count(cg::OPT_SAMPLER_ATOMIC_LAUNCHES)" in body
    assert body.index("opt_count") > body.index("return 0;"), "the counter sits in the fallback branch"


def test_every_case_is_in_the_regime_it_names():
    for id_, N, Nimg, (Hi, Wi, Ho, Wo), C, mis, grid_mis, special, regime in E.CASES:
        plan = R.sampler_plan(N, Nimg, Hi, Wi, C, Ho, Wo, not mis, None if grid_mis is None else not grid_mis)
        assert R.describe(plan) == regime, (id_, R.describe(plan))
        b = plan["backward"]
        if b["path"] == "det":
            assert b["lds"] <= 160 * 1024 and b["S"] * b["nchunks"] >= max(Hi * Wi, Ho * Wo) > b["S"] * (b["nchunks"] - 1)


def test_the_cases_cover_the_regimes_the_kernels_have():
    P = [(c, R.sampler_plan(c[1], c[2], *c[3][:2], c[4], *c[3][2:], not c[5], None if c[6] is None else not c[6])) for c in E.CASES]
    det = [p["backward"] for _, p in P if p["backward"]["path"] == "det"]
    atomic = [p["backward"] for _, p in P if p["backward"]["path"] == "atomic"]
    assert {(b["G"], b["CACC"]) for b in det if not b["v4"]} >= {(4, 1), (8, 1), (32, 1), (64, 1), (64, 2), (64, 4)}
    assert {b["G"] for b in det if b["v4"]} == {4, 8, 16, 32, 64}
    assert any(b["v4"] and b["idle_lanes"] and b["G"] == g for b in det for g in (8, 32, 64))
    assert {b["want"] for b in det} >= {16, 14, 3, 1}
    assert any(b["S"] % b["ngrp"] and b["ragged"] and b["nchunks"] > 1 for b in det)
    assert max(b["lds"] for b in det) == 145596 and any(b["lds"] == 142524 for b in det)     # 66 x 66 onto 66 x 66: 140 460 B dynamic
    assert {b["why"] for b in atomic} == {"C", "lds"} and any(b["wraps"] for b in atomic) and any(not b["wraps"] for b in atomic)
    fw = {(p["forward"]["kernel"], p["forward"]["ew"]) for _, p in P}
    assert fw == {(k, e) for k in ("bilinear_fwd_k<1>", "bilinear_fwd_k<4>") for e in ("one", "many", "wrap")}
    grid_off = [p for c, p in P if c[6]]
    assert grid_off and all(p["forward"]["kernel"] == "bilinear_fwd_k<1>" and p["backward"].get("v4") for p in grid_off)
    assert any(c[1] > c[2] for c, p in P if p["backward"]["path"] == "det") and any(c[1] > c[2] for c, p in P if p["backward"]["path"] == "atomic")


def test_the_heavy_grids_hold_the_tap_totals_they_name():
    """heavy_grid asserts its totals itself; here: which cases cross kHeavy, and that 64 taps stay on the light path."""
    for c in E.CASES:
        id_, N, Nimg, geom, C, mis, grid_mis, special, regime = c
        if not special:
            continue
        _, _, grid, _ = E.case_inputs(id_, N, Nimg, geom, C, special)
        hp = R.heavy_pixels(grid, geom[0], geom[1])
        assert (hp[N - 1] == 0).all()
        if special == "cell64":
            assert hp.max() == 64 == R.HEAVY
        else:
            assert hp[0].max() > R.HEAVY and ((hp[0] > 0) & (hp[0] <= R.HEAVY)).any() == (special in ("four", "pair"))
