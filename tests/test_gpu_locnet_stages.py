"""cg_locnet_forward / cg_locnet_backward (csrc/locnet.hip) buffer by buffer against the fp64 stages of tests/locnet_ref.py.

The comparison is teacher-forced: each of the twelve buffers a call writes - pooled, h1, m2, h2, h3, params, grid; g4, g3, ga2, ga1,
gx - is compared with the fp64 stage applied to the DEVICE's own previous buffer, so errors do not compound, LeakyReLU's side is
never in doubt in the backward (it is the sign of the array the call was given) and a failure names the stage.  A case collects all
twelve verdicts before it fails.

Measure: helpers.rounding_close, per element, |d| <= r (U24 terms + TINY); nothing is scaled by a tensor's maximum, no element is
left out and there is no outlier allowance.  r is counted from the stage's expression (locnet_ref.r_sum: a sum of K addends in any
association has at most K roundings on an addend's way, r = K + 2):

    pooled, h2   K = 5                      h1   K = 9 Cin + 1, + 1 for the slope product     m2, ga1, gx   K = 145
    h3           K = K3 + 1                 params   K = 65            g3   K = P             ga2           K = 64

The affine stages (grid from params, g4 from ggrid and params; T, grid, gT, gparams of the four cg_affine_* entry points) count the
roundings of the expression the same way (locnet_ref.R_T .. R_G4) plus the error of sinf / cosf.  The ROCm installation ships no
accuracy table for them, so the figure is the reference side's: numpy's fp32 sin / cos against fp64 over |theta| < pi measure
1.42 ulp (locnet_ref.trig_ulp_measured), times 4 for a different libm = 5.68 ulp, counted as 12 roundings.  Nothing here was
calibrated on the device's output.  The inputs keep |theta| < pi.

Every output buffer lies inside a larger allocation with 64 sentinel floats on either side, which must be bit-unchanged after the
call, and is pre-filled with NaN, none of which may be left.

One case per family runs in exact arithmetic: scale-only transform on a 3x3 grid, slope 0.25, inputs and weights in {-1, 0, 1}.
There every addend of pooled .. h3 and of g4 .. gx is a multiple of 2^-12 and an element's addends sum to less than 2^12 in
magnitude (the case asserts both), so every partial sum in any order is an fp32 number and the ten buffers must EQUAL the fp64
values.  This is what sees an error of a few ulp in a factor - 0.2500001 for 0.25 in a pooling, say - which the K + 2 bound of a
145-term stage lets through.

Each case first asserts its premises: cg_locnet_supported() == 1, the kernel family (locnet.hip's v2::has restated) and, for the
VALU kernels, the tap split conv3x3_lds takes in the forward convolutions and in conv 1's data gradient (conv_split restated below,
as helpers.col_launch restates the column reduction's) - a retuned threshold fails the premise, not the case silently.

Measured on the MI355X when the file was written, worst |d| / bound per buffer over a shape's cases (every case prints its own line;
split = the tap splits of the forward convolutions, conv 2's and conv 1's data gradient):

    family S  Cin split    cases pooled h1    m2    h2    h3    params grid  g4    g3    ga2   ga1   gx
    MFMA   4  64  -        12    0.353  0.003 0.035 0.350 0.020 0.012  0.103 0.076 0.587 0.025 0.030 0.040
    MFMA   8  64  -        2     0.352  0.003 0.022 0.265 0.002 0.013  0.053 0.024 0.571 0.053 0.025 0.033
    MFMA   16 3   -        2     0.302  0.103 0.024 0.286 0.000 0.009  0.060 0.031 0.534 0.051 0.035 0.026
    VALU   8  3   9, 9, 9  11    0.329  0.091 0.012 0.370 0.003 0.027  0.118 0.048 0.586 0.066 0.012 0.014
    VALU   8  1   9, 9, 9  1     0.237  0.198 0.007 0.379 0.002 0.010  0.058 0.002 0.546 0.044 0.013 0.007
    VALU   8  6   9, 9, 9  1     0.265  0.021 0.008 0.242 0.002 0.011  0.043 0.064 0.289 0.047 0.010 0.009
    VALU   16 1   3, 3, 9  1     0.271  0.140 0.010 0.351 0.000 0.006  0.054 0.002 0.556 0.045 0.015 0.006
    VALU   16 8   3, 3, 3  1     0.262  0.019 0.011 0.265 0.000 0.012  0.095 0.030 0.208 0.064 0.017 0.012
    VALU   16 24  3, 3, 1  1     0.318  0.006 0.011 0.285 0.000 0.013  0.106 0.061 0.283 0.058 0.015 0.032

The direct cg_affine_* calls: T 0.141, grid 0.236, gT 0.163, gparams 0.119; the two exact cases: every buffer equal.  h3 at S >= 8 and
h1 at Cin 64 stay below 0.01 of their bound everywhere (long sums whose roundings cancel): those two could be tightened later."""
import collections
import ctypes
import importlib

import numpy as np
import pytest
import torch

import locnet_ref as R
from helpers import bulk_close, close, edge_normal, rounding_close

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD, SENTINEL = 64, 777.0
NT = 768                  # locnet.hip: threads of a VALU workgroup


@pytest.fixture(scope="module")
def cg():
    mod = importlib.import_module("cat-generator_amd")
    assert torch.cuda.is_available(), "these tests need the MI355X"
    mod.lib()
    return mod


def conv_split(S, OUT):
    """locnet.hip conv_split(): tap groups of conv3x3_lds - 1 (all nine taps per item), 3 (one kernel row) or 9 (one tap)."""
    items = ((S * S) >> 2) * (OUT >> 2)
    return 1 if 2 * items >= NT else (3 if 6 * items >= NT else 9)


def mfma_shape(S, Cin):
    """locnet.hip v2::has(): the geometries of the MFMA kernels."""
    return (S, Cin) in ((16, 3), (8, 64), (4, 64))


class Guarded:
    """n floats of NaN on the device between two runs of GUARD sentinel floats."""

    def __init__(self, n):
        self.n = int(n)
        self.big = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.big[GUARD:GUARD + self.n] = float("nan")
        self.ptr = self.big.data_ptr() + 4 * GUARD
        assert self.ptr % 16 == 0

    def raw(self, what):
        g = self.big.cpu().numpy()
        want = np.full(GUARD, SENTINEL, f32).view(np.uint32)
        assert (g[:GUARD].view(np.uint32) == want).all() and (g[GUARD + self.n:].view(np.uint32) == want).all(), f"{what}: a write outside the buffer"
        return g[GUARD:GUARD + self.n]

    def host(self, shape, what):
        a = self.raw(what)
        assert not np.isnan(a).any(), f"{what}: {int(np.isnan(a).sum())} of {a.size} elements never written"
        return a.reshape(shape).copy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32).reshape(-1)).cuda()


def ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


Case = collections.namedtuple("Case", "S Cin flags G N shared hw slope indep exact", defaults=(0.333, False, False))
FWD = ("pooled", "h1", "m2", "h2", "h3", "params", "grid")
BWD = ("ga1", "ga2", "g3", "g4", "gx")
TTT, TFF = (1, 1, 1), (1, 0, 0)


def case_id(c):
    return f"S{c.S}-Cin{c.Cin if c.Cin > 0 else 'r1'}-G{c.G}-N{c.N}-sh{int(c.shared)}-{c.hw[0]}x{c.hw[1]}-{'exact' if c.exact else 'indep' if c.indep else 'fwd'}"


def make_weights(rng, S, Cin, P):
    """The eight canonical tensors of one localisation net; every second bias of conv 1 and of linear 1 is zero (with the all-zero
    sample their pre-activations are exactly +0.0, which takes the x >= 0 side)."""
    K3 = 16 * (S // 2) ** 2
    T = lambda *shape, sc: (rng.standard_normal(shape) * sc).astype(f32)
    W = [T(16, Cin, 3, 3, sc=1.0 / np.sqrt(9 * Cin)), T(16, sc=0.1), T(16, 16, 3, 3, sc=1.0 / 12), T(16, sc=0.1),
         T(64, K3, sc=1.0 / np.sqrt(K3)), T(64, sc=0.1), T(P, 64, sc=0.02), T(P, sc=0.3)]
    W[1][::2] = 0.0
    W[5][::2] = 0.0
    return W


def exact_weights(rng, S, Cin, P):
    """Weights of the exact-arithmetic cases: entries in {-1, 0, 1}.  conv 1 and linear 2 are dense (genuine sums of 9 Cin, 144 and 64
    terms); conv 2 has one tap of one input plane per output plane and linear 1 one input per K3 / 64 outputs, so that the values keep
    few enough bits on their way through the chain."""
    K3 = 16 * (S // 2) ** 2
    ints = lambda *shape: rng.integers(-1, 2, shape).astype(f32)
    w2, w3 = np.zeros((16, 16, 3, 3), f32), np.zeros((64, K3), f32)
    for co in range(16):
        w2[co, rng.integers(16), rng.integers(3), rng.integers(3)] = rng.choice([-1.0, 1.0])
    w3[np.arange(K3) % 64, np.arange(K3)] = rng.choice([-1.0, 1.0], K3)
    W = [ints(16, Cin, 3, 3), ints(16), w2, ints(16), w3, ints(64), ints(P, 64), np.ones(P, f32)]
    W[1][::2] = 0.0
    W[5][::2] = 0.0
    return W


def device_weights(cg, W, Cin):
    """The 12 device tensors cg_locnet_* take per group: the canonical eight, then cg_pack_conv_weight's copies of both convolutions."""
    L, st = cg.lib(), cg.tensor.stream()
    ts = [dev(w) for w in W]
    ts += [torch.zeros(n, dtype=torch.float32, device="cuda") for n in (9 * Cin * 16, 9 * 16 * Cin, 9 * 256, 9 * 256)]
    L.pack_conv_weight(st, ts[0].data_ptr(), ts[8].data_ptr(), ts[9].data_ptr(), 16, Cin, 3, 3)
    L.pack_conv_weight(st, ts[2].data_ptr(), ts[10].data_ptr(), ts[11].data_ptr(), 16, 16, 3, 3)
    return ts


def shapes(c):
    S, Cin, P, GN, K3 = c.S, c.Cin, R.nparams(c.flags), c.G * c.N, 16 * (c.S // 2) ** 2
    fwd = dict(pooled=(GN, S, S, Cin), h1=(GN, S, S, 16), m2=(GN, S, S, 16), h2=(GN, K3), h3=(GN, 64), params=(GN, P), grid=(GN, *c.hw, 2))
    bwd = dict(ga1=(GN, S, S, 16), ga2=(GN, S, S, 16), g3=(GN, 64), g4=(GN, P), gx=(GN, 2 * S, 2 * S, Cin))
    return fwd, bwd


def device_forward(cg, c, x, wts):
    L, st = cg.lib(), cg.tensor.stream()
    fwd, _ = shapes(c)
    outs = {k: Guarded(np.prod(fwd[k])) for k in FWD}
    xt = dev(x)
    L.locnet_forward(st, c.G, c.N, xt.data_ptr(), int(c.shared), ptrs([t for ts in wts for t in ts]), c.S, c.Cin, R.nparams(c.flags), *c.flags,
                     c.slope, *c.hw, *[outs[k].ptr for k in FWD])
    return {k: outs[k].host(fwd[k], k) for k in FWD}


def backward_call(cg, c, acts, ggrid, wts, outs, slope=None, flags=None):
    L, st = cg.lib(), cg.tensor.stream()
    ins = [dev(acts[k]) for k in ("h1", "m2", "h3", "params")] + [dev(ggrid)]
    L.locnet_backward(st, c.G, c.N, ptrs([t for ts in wts for t in ts]), c.S, c.Cin, R.nparams(c.flags), *(flags or c.flags),
                      c.slope if slope is None else slope, *c.hw, *[t.data_ptr() for t in ins], *[outs[k].ptr for k in BWD])


def device_backward(cg, c, acts, ggrid, wts, slope=None):
    _, bwd = shapes(c)
    outs = {k: Guarded(np.prod(bwd[k])) for k in BWD}
    backward_call(cg, c, acts, ggrid, wts, outs, slope)
    return {k: outs[k].host(bwd[k], k) for k in BWD}


def refused(cg, c, acts, ggrid, wts, match, **kw):
    """The call raises, and no output buffer (NaN between its sentinels) has been touched."""
    outs = {k: Guarded(np.prod(shapes(c)[1][k])) for k in BWD}
    with pytest.raises(cg.CatganError, match=match):
        backward_call(cg, c, acts, ggrid, wts, outs, **kw)
    torch.cuda.synchronize()
    for k in BWD:
        assert np.isnan(outs[k].raw(k)).all(), f"{kw}: refused, but {k} was written"


def premises(cg, c):
    """-> (family, tap splits of (the forward convolutions, conv 2's data gradient, conv 1's data gradient)); None for the MFMA kernels."""
    assert cg.lib().locnet_supported(c.S, c.Cin, R.nparams(c.flags)) == 1, c
    if mfma_shape(c.S, c.Cin):
        return "MFMA", None
    return "VALU", (conv_split(c.S, 16), conv_split(c.S, 16), conv_split(c.S, (c.Cin + 3) & ~3))


def run_case(cg, c, seed, want_family, want_split=None):
    family, split = premises(cg, c)
    assert family == want_family and split == want_split, (c, family, split)
    S, Cin, P, GN = c.S, c.Cin, R.nparams(c.flags), c.G * c.N
    K3 = 16 * (S // 2) ** 2
    rng = np.random.default_rng(seed)
    Ws = [(exact_weights if c.exact else make_weights)(rng, S, Cin, P) for _ in range(c.G)]
    wts = [device_weights(cg, W, Cin) for W in Ws]
    Nx = c.N if c.shared else GN
    x = edge_normal(rng, (Nx, 2 * S, 2 * S, Cin))
    ggrid = edge_normal(rng, (GN, *c.hw, 2))
    if c.exact:
        x, ggrid = rng.integers(-1, 2, x.shape).astype(f32), rng.integers(-1, 2, ggrid.shape).astype(f32)
    if Nx > 1:
        x[Nx - 1] = 0.0                                  # one sample is all zero
    d = device_forward(cg, c, x, wts)
    if P > 0 and c.flags[0]:
        assert np.abs(d["params"][:, 0]).max() < np.pi, "premise: |theta| < pi"
    if c.indep:                                          # the backward is a pure function of its arrays: independent ones, zeros planted
        acts = dict(h1=edge_normal(rng, (GN, S, S, 16)), m2=edge_normal(rng, (GN, S, S, 16)), h3=edge_normal(rng, (GN, 64)))
        prm = np.concatenate(([rng.uniform(-3.0, 3.0, (GN, 1))] if c.flags[0] else []) + ([rng.uniform(0.5, 1.5, (GN, 1))] if c.flags[1] else [])
                             + ([rng.uniform(-0.5, 0.5, (GN, 2))] if c.flags[2] else []), 1).astype(f32)
        acts["params"] = prm
    else:
        acts = {k: d[k] for k in ("h1", "m2", "h3", "params")}
    b = device_backward(cg, c, acts, ggrid, wts)

    verdict = {}

    def check(name, got, stage, r):
        try:
            verdict[name] = rounding_close(got, stage[0], stage[1], r, what=f"{name} ({family} S {S} Cin {Cin})")
        except AssertionError as e:
            verdict[name] = str(e)
            return
        if c.exact and name not in ("params", "grid"):
            # every addend is a multiple of 2^-12 and the magnitudes of an element's addends sum to less than 2^12: all partial sums,
            # in any order and fused or not, are fp32 numbers, so the device's value is THE value - bound 0
            ref, terms = stage
            assert (ref * 4096 == np.round(ref * 4096)).all() and terms.max() < 4096 and np.abs(ref).max() > 0, f"premise of the exact case: {name}"
            bad = got.astype(np.float64) != ref
            if bad.any():
                verdict[name] = (f"{name} ({family} S {S} Cin {Cin}): exact arithmetic, yet {int(bad.sum())} of {bad.size} elements differ, "
                                 f"max |d| / |ref| = {float((np.abs(got - ref)[bad] / np.abs(ref)[bad]).max()):.3e}")

    sl, cat = c.slope, lambda parts: tuple(np.concatenate([p[k] for p in parts]) for k in (0, 1))
    per_group = lambda fn: cat([fn(g, slice(g * c.N, (g + 1) * c.N), Ws[g]) for g in range(c.G)])
    check("pooled", d["pooled"], per_group(lambda g, s, W: R.avgpool2(x[slice(0, c.N) if c.shared else s])), R.r_sum(5))
    check("h1", d["h1"], per_group(lambda g, s, W: R.conv_lrelu(d["pooled"][s], W[0], W[1], sl)), R.r_sum(9 * Cin + 1 + 1))
    check("m2", d["m2"], per_group(lambda g, s, W: R.conv_lrelu(d["h1"][s], W[2], W[3], sl)), R.r_sum(145))
    check("h2", d["h2"], R.pool_flatten(d["m2"]), R.r_sum(5))
    check("h3", d["h3"], per_group(lambda g, s, W: R.linear_lrelu(d["h2"][s], W[4], W[5], sl)), R.r_sum(K3 + 1))
    check("params", d["params"], per_group(lambda g, s, W: R.linear(d["h3"][s], W[6], W[7])), R.r_sum(65))
    check("grid", d["grid"], R.grid_from_params(d["params"], c.flags, *c.hw), R.R_GRID)
    check("g4", b["g4"], R.g4_from_ggrid(ggrid, acts["params"], c.flags), R.R_G4)
    check("g3", b["g3"], per_group(lambda g, s, W: R.g3_from_g4(b["g4"][s], acts["h3"][s], W[6], sl)), R.r_sum(P))
    check("ga2", b["ga2"], per_group(lambda g, s, W: R.ga2_from_g3(b["g3"][s], acts["m2"][s], W[4], sl)), R.r_sum(64))
    check("ga1", b["ga1"], per_group(lambda g, s, W: R.ga1_from_ga2(b["ga2"][s], acts["h1"][s], W[2], sl)), R.r_sum(145))
    check("gx", b["gx"], per_group(lambda g, s, W: R.gx_from_ga1(b["ga1"][s], W[0])), R.r_sum(145))
    print(f"LOCNET-STAGES {family} S {S} Cin {Cin} flags {''.join('FT'[f] for f in c.flags)} G {c.G} N {c.N} shared {int(c.shared)} grid {c.hw} "
          f"slope {c.slope} indep {int(c.indep)} exact {int(c.exact)} split {split}: " + " ".join(f"{k} {v:.3f}" if isinstance(v, float) else f"{k} FAILED" for k, v in verdict.items()))
    failed = {k: v for k, v in verdict.items() if not isinstance(v, float)}
    assert not failed, "stages outside their bound: " + "; ".join(failed.values())
    return d, b, Ws, x


# ------------------------------------------------------------------------------ the MFMA kernels
@pytest.mark.parametrize("flags", R.FLAGS, ids=lambda f: "".join("FT"[v] for v in f))
def test_mfma_4x4x64_every_transform(cg, flags):
    """S 4, Cin 64: one M tile, the K3 = 64 paths, conv 2 on wave 0 alone; all seven (rot, scale, trans)."""
    run_case(cg, Case(4, 64, flags, 1, 5, False, (8, 8)), 40 + R.nparams(flags), "MFMA")


@pytest.mark.parametrize("c", [
    Case(4, 64, TTT, 4, 70, True, (8, 8)),                 # 280 workgroups: more than the 256 CUs
    Case(4, 64, TTT, 2, 5, False, (24, 24)),               # 576 grid points for 256 threads; every group its own input
    Case(4, 64, TTT, 2, 5, False, (5, 12)),
    Case(4, 64, TFF, 1, 5, False, (1, 7)),                 # Hg == 1: y = -1
    Case(4, 64, TTT, 1, 5, False, (8, 8), 0.05, True),     # independent backward arrays, another slope
    Case(4, 64, (0, 1, 0), 2, 5, False, (3, 3), 0.25, False, True),   # exact arithmetic: ten buffers must be THE value
    Case(8, 64, TTT, 1, 5, False, (16, 16)),               # KSPLIT partials over the pooled image, NSPLIT data gradient
    Case(8, 64, TFF, 4, 1, False, (16, 16)),
    Case(16, 3, TFF, 1, 5, False, (32, 32)),               # zero-padded K-step and N tile, scalar pooling path
    Case(16, 3, TTT, 2, 1, True, (32, 32)),
], ids=case_id)
def test_mfma_shapes_groups_grids(cg, c):
    run_case(cg, c, 100 + c.S + c.G + c.N + c.hw[1], "MFMA")


# ------------------------------------------------------------------------------ the VALU kernels
@pytest.mark.parametrize("flags", R.FLAGS, ids=lambda f: "".join("FT"[v] for v in f))
def test_valu_8x8x3_every_transform(cg, flags):
    """S 8, Cin 3 (the first transformer at 16 px): one tap per thread (R = 9) both ways; all seven (rot, scale, trans)."""
    run_case(cg, Case(8, 3, flags, 1, 5, False, (16, 16)), 60 + R.nparams(flags), "VALU", (9, 9, 9))


def r1_cin(cg):
    """The Cin of the R = 1 case: 24, or the smallest Cin divisible by 4 whose data gradient takes all nine taps per item and which the
    launches cover."""
    for Cin in [24] + list(range(4, 129, 4)):
        if conv_split(16, Cin) == 1 and cg.lib().locnet_supported(16, Cin, 4) == 1:
            return Cin
    raise AssertionError("no supported Cin at S 16 reaches conv_split == 1")


@pytest.mark.parametrize("c,split", [
    (Case(8, 3, TTT, 4, 70, False, (16, 16)), (9, 9, 9)),              # 280 workgroups, every group and sample its own input
    (Case(8, 3, TTT, 2, 5, True, (5, 12)), (9, 9, 9)),
    (Case(8, 3, TFF, 1, 5, False, (1, 7)), (9, 9, 9)),
    (Case(8, 3, TTT, 1, 5, False, (16, 16), 0.05, True), (9, 9, 9)),   # independent backward arrays, another slope
    (Case(8, 3, (0, 1, 0), 2, 5, True, (3, 3), 0.25, False, True), (9, 9, 9)),   # exact arithmetic: ten buffers must be THE value
    (Case(8, 1, TFF, 2, 5, True, (16, 16)), (9, 9, 9)),                # the first transformer at 16 px grayscale
    (Case(8, 6, TTT, 1, 5, False, (16, 16)), (9, 9, 9)),               # CinQ = 8: two padded planes
    (Case(16, 1, TFF, 1, 5, False, (32, 32)), (3, 3, 9)),              # bench config 3: R = 3 forward, R = 9 in conv 1's data gradient
    (Case(16, 8, TTT, 2, 1, False, (32, 32)), (3, 3, 3)),              # R = 3 in conv 1's data gradient
    (Case(16, -1, TTT, 1, 5, False, (32, 32)), (3, 3, 1)),             # R = 1 in conv 1's data gradient (Cin: r1_cin)
], ids=lambda v: case_id(v) if isinstance(v, Case) else "R" + "".join(map(str, v)))
def test_valu_shapes_groups_grids(cg, c, split):
    if c.Cin < 0:
        c = c._replace(Cin=r1_cin(cg))
    run_case(cg, c, 200 + c.S + c.Cin + c.G + c.N + c.hw[1], "VALU", split)


# ------------------------------------------------------------------------------ the four cg_affine_* entry points
@pytest.mark.parametrize("flags", R.FLAGS, ids=lambda f: "".join("FT"[v] for v in f))
def test_affine_entry_points_direct(cg, flags):
    """cg_affine_matrix_forward / _backward and cg_affine_grid_forward / _backward called directly, N = 1, 5 and 300 (more workgroups than
    CUs in the grid's backward) on grids (8, 8), (5, 12) and (1, 7), against the same fp64 stages; each on the device's previous result."""
    L, st = cg.lib(), cg.tensor.stream()
    P = R.nparams(flags)
    rng = np.random.default_rng(7 + P)
    worst = collections.defaultdict(float)
    for N in (1, 5, 300):
        prm = np.concatenate(([rng.uniform(-3.1, 3.1, (N, 1))] if flags[0] else []) + ([rng.uniform(0.3, 2.0, (N, 1))] if flags[1] else [])
                             + ([rng.uniform(-1.0, 1.0, (N, 2))] if flags[2] else []), 1).astype(f32)
        if N > 1:
            prm[1] = 0.0                       # theta = 0, scale = 0, no translation
        pt, T = dev(prm), Guarded(N * 6)
        L.affine_matrix_forward(st, pt.data_ptr(), T.ptr, N, *flags)
        Td = T.host((N, 2, 3), "T")
        worst["T"] = max(worst["T"], rounding_close(Td, *R.affine_T(prm, flags), R.R_T, what=f"T N {N}"))
        for hw in ((8, 8), (5, 12), (1, 7)):
            grid = Guarded(N * hw[0] * hw[1] * 2)
            L.affine_grid_forward(st, dev(Td).data_ptr(), grid.ptr, N, *hw)
            worst["grid"] = max(worst["grid"], rounding_close(grid.host((N, *hw, 2), "grid"), *R.grid_from_T(Td, np.abs(Td), *hw), R.R_GRID_T,
                                                              what=f"grid N {N} {hw}"))
            gg = edge_normal(rng, (N, *hw, 2))
            gT = Guarded(N * 6)
            L.affine_grid_backward(st, dev(gg).data_ptr(), gT.ptr, N, *hw)
            gTd = gT.host((N, 2, 3), "gT")
            worst["gT"] = max(worst["gT"], rounding_close(gTd, *R.gT_from_ggrid(gg), R.R_GT, what=f"gT N {N} {hw}"))
            gp = Guarded(N * P)
            L.affine_matrix_backward(st, pt.data_ptr(), dev(gTd).data_ptr(), gp.ptr, N, *flags)
            worst["gparams"] = max(worst["gparams"], rounding_close(gp.host((N, P), "gparams"), *R.g4_from_gT(gTd, np.abs(gTd), prm, flags), R.R_G4_T,
                                                                    what=f"gparams N {N} {hw}"))
    print(f"LOCNET-STAGES affine direct flags {''.join('FT'[f] for f in flags)}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------ refusals and the negative slope
def _small(cg):
    c = Case(8, 3, TTT, 1, 2, False, (16, 16))
    rng = np.random.default_rng(1)
    Ws = [make_weights(rng, c.S, c.Cin, 4)]
    wts = [device_weights(cg, W, c.Cin) for W in Ws]
    d = device_forward(cg, c, edge_normal(rng, (2, 16, 16, 3)), wts)
    return c, wts, d, edge_normal(rng, (2, 16, 16, 2))


def test_backward_refuses_a_slope_that_is_not_positive_before_any_launch(cg):
    """LeakyReLU's side in the backward is read off the stored activations, which have the sign of the layers' inputs only for
    slope > 0.  The forward takes any slope (tests/test_gpu_membound_bits.py pins it at -0.333)."""
    c, wts, d, gg = _small(cg)
    for slope in (0.0, -0.0, -0.333, float("nan")):
        refused(cg, c, d, gg, wts, "slope", slope=slope)
    device_forward(cg, c._replace(slope=-0.333), edge_normal(np.random.default_rng(2), (2, 16, 16, 3)), wts)
    device_backward(cg, c, d, gg, wts, slope=1e-3)


def test_backward_refuses_P_that_does_not_match_the_transform_before_any_launch(cg):
    c, wts, d, gg = _small(cg)
    for flags in ((1, 0, 0), (1, 1, 0), (0, 0, 1), (0, 0, 0)):
        refused(cg, c, d, gg, wts, "P does not match", flags=flags)


@pytest.mark.parametrize("size,ch", [(16, 3), (8, 64)])
def test_transformer_with_a_negative_slope_takes_the_modules(cg, size, ch):
    """createSpatialTransformer with nn.LeakyReLU(-0.2) in the localisation net, at a shape the fused launches cover (VALU: S 8, Cin 3;
    MFMA: S 4, Cin 64): the planner walks the ten modules (match_loc refuses the slope), and the planned pass agrees with the
    per-module walk under tests/test_gpu_scale16.py's _check_transformer bounds."""
    assert cg.lib().locnet_supported(size // 2, ch, 4) == 1
    cg.manual_seed(5)
    P = cg.models.createSpatialTransformer(True, True, True, size, ch, False)
    acts = [m for m in P.listModules() if m.typename == "nn.LeakyReLU"]
    assert len(acts) == 3
    for m in acts:
        m.negative_scale = -0.2
    rs = np.random.RandomState(4)
    P.modules[0].modules[1].modules[0].modules[-1].weight.copy((rs.randn(4, 64) * 0.05).astype(f32))
    x = rs.rand(5, ch, size, size).astype(f32); dy = rs.randn(5, ch, size, size).astype(f32)
    xin, dyt = cg.Tensor.from_numpy(x), cg.Tensor.from_numpy(dy)

    out = P.forward(xin).numpy().copy()
    assert P._planned_last
    st = P._pnet[1].stats()
    assert st["launches_forward"] >= 9, st                  # the module launch count, not the fused launch's 2
    P.zeroGradParameters()
    gi = P.backward(xin, dyt).numpy().copy()
    grads = [g.numpy().copy() for g in P.parameters()[1]]

    out_w = P.updateOutput(xin).numpy().copy()
    assert not P._planned_last
    P.zeroGradParameters()
    gi_w = P.backward(xin, dyt).numpy().copy()
    grads_w = [g.numpy().copy() for g in P.parameters()[1]]

    close(out, out_w, tol=3e-5, what="negative slope fwd")
    close(gi, gi_w, K=4096, tol=5e-5, what="negative slope gradInput")
    assert len(grads) == len(grads_w) == 8
    for a, b in zip(grads, grads_w):
        assert np.abs(b).max() > 0
        bulk_close(a, b, max_rel=2e-3, mean_rel=2e-4, what="negative slope param grad")


# ------------------------------------------------------------------------------ context: how small gx is beside the sampler's gradient
def test_context_gx_against_the_sampler_image_gradient(cg):
    """Information, not an assertion: at the branch transformers' 32 px shape (16x16 input of 64 planes: S 8, Cin 64) with the sampler
    behind the localisation launch, max|gx| / max|sampler gimg|.  In the module's gradInput gx is ADDED to gimg, so this ratio is the
    share of gx that a bound scaled by the sum's maximum leaves unexamined.  Classifier weights as test_spatial_transformer_module."""
    L, st = cg.lib(), cg.tensor.stream()
    cg.manual_seed(5)
    P = cg.models.createSpatialTransformer(True, True, True, 16, 64, False)
    rs = np.random.RandomState(4)
    W = [p.numpy().copy() for p in P.parameters()[0]]
    W[6] = (rs.randn(4, 64) * 0.05).astype(f32)
    assert [w.shape for w in W] == [(16, 64, 3, 3), (16,), (16, 16, 3, 3), (16,), (64, 256), (64,), (4, 64), (4,)]
    c = Case(8, 64, TTT, 1, 5, False, (16, 16))
    wts = [device_weights(cg, W, 64)]
    x = np.ascontiguousarray(rs.rand(5, 64, 16, 16).astype(f32).transpose(0, 2, 3, 1))
    gout = np.ascontiguousarray(rs.randn(5, 64, 16, 16).astype(f32).transpose(0, 2, 3, 1))
    d = device_forward(cg, c, x, wts)
    gimg, ggrid = Guarded(x.size), Guarded(5 * 16 * 16 * 2)
    L.bilinear_sampler_backward(st, dev(x).data_ptr(), dev(d["grid"]).data_ptr(), dev(gout).data_ptr(), gimg.ptr, ggrid.ptr, 5, 16, 16, 64, 16, 16)
    b = device_backward(cg, c, d, ggrid.host((5, 16, 16, 2), "ggrid"), wts)
    gi = gimg.host(x.shape, "gimg")
    ratio = float(np.abs(b["gx"]).max() / np.abs(gi).max())
    print(f"LOCNET-STAGES context S 8 Cin 64: max|gx| {np.abs(b['gx']).max():.3e} / max|sampler gimg| {np.abs(gi).max():.3e} = {ratio:.3e}")
    assert np.isfinite(ratio)
