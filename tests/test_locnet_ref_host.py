"""tests/locnet_ref.py checked on its own, without a GPU: the fp64 stages composed into the whole localisation chain against torch
fp64 autograd of avg_pool2d -> conv2d -> ... -> linear -> T -> affine_grid (T's entries typed in as the closed form of
include/catgan.h, the grid through F.affine_grid with the (y, x) <-> (x, y) swap: neither is how locnet_ref gets them), and against
the localisation half of oracle.SpatialTransformer at the fp32 tolerances of tests/test_oracle_vs_torch.py.  The twin applies
LeakyReLU to the layers' INPUTS, the stages' backward decides on the activations: for slope > 0 the two must agree."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import locnet_ref as R
from oracle import oracle as O

f32 = np.float32
t64 = lambda a: torch.tensor(np.asarray(a, np.float64))


def make_weights(rs, S, Cin, P):
    K3 = 16 * (S // 2) ** 2
    T = lambda *shape, sc: (rs.randn(*shape) * sc).astype(f32)
    return [T(16, Cin, 3, 3, sc=1.0 / np.sqrt(9 * Cin)), T(16, sc=0.1), T(16, 16, 3, 3, sc=1.0 / 12), T(16, sc=0.1),
            T(64, K3, sc=1.0 / np.sqrt(K3)), T(64, sc=0.1), T(P, 64, sc=0.1), T(P, sc=0.3)]


def _torch_T(p, flags):
    """include/catgan.h: rows [c s, -sn s, c s tx - sn s ty], [sn s, c s, sn s tx + c s ty]."""
    N = p.shape[0]
    k = 0
    th, sc, tx, ty = torch.zeros(N, dtype=p.dtype), torch.ones(N, dtype=p.dtype), torch.zeros(N, dtype=p.dtype), torch.zeros(N, dtype=p.dtype)
    if flags[0]:
        th = p[:, k]; k += 1
    if flags[1]:
        sc = p[:, k]; k += 1
    if flags[2]:
        tx, ty = p[:, k], p[:, k + 1]
    c, s = torch.cos(th), torch.sin(th)
    return torch.stack([torch.stack([c * sc, -s * sc, c * sc * tx - s * sc * ty], 1),
                        torch.stack([s * sc, c * sc, s * sc * tx + c * sc * ty], 1)], 1)


def _torch_grid(T, H, W):
    """F.affine_grid works in (x, y); T acts on (y, x, 1) and emits (y, x).  -> [N][H][W][2] in (y, x)."""
    Tx = torch.stack([torch.stack([T[:, 1, 1], T[:, 1, 0], T[:, 1, 2]], 1), torch.stack([T[:, 0, 1], T[:, 0, 0], T[:, 0, 2]], 1)], 1)
    if H > 1 and W > 1:
        return F.affine_grid(Tx, (T.shape[0], 1, H, W), align_corners=True).flip(-1)
    # a unit-size axis sits at -1 (the kernels' `H > 1 ? ... : -1`; F.affine_grid puts it at 0): the base grid written out
    ax = lambda n: torch.linspace(-1, 1, n, dtype=T.dtype) if n > 1 else -torch.ones(1, dtype=T.dtype)
    y, x = torch.meshgrid(ax(H), ax(W), indexing="ij")
    return torch.einsum("ijk,nrk->nijr", torch.stack([y, x, torch.ones_like(y)], -1), T)


def torch_chain(x, W, flags, slope, Hg, Wg, ggrid):
    """-> grid, gx (NHWC), the eight parameter gradients."""
    xt = t64(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ws = [t64(w).requires_grad_(True) for w in W]
    lr = lambda h: torch.where(h >= 0, h, h * slope)
    h = F.avg_pool2d(xt, 2)
    h = lr(F.conv2d(h, ws[0], ws[1], padding=1))
    h = lr(F.conv2d(h, ws[2], ws[3], padding=1))
    h = F.avg_pool2d(h, 2).reshape(x.shape[0], -1)
    h = lr(F.linear(h, ws[4], ws[5]))
    grid = _torch_grid(_torch_T(F.linear(h, ws[6], ws[7]), flags), Hg, Wg)
    grid.backward(t64(ggrid))
    return grid.detach().numpy(), xt.grad.permute(0, 2, 3, 1).numpy(), [w.grad.numpy() for w in ws]


def stage_grads(x, W, flags, slope, Hg, Wg, ggrid):
    acts = R.forward(x, W, flags, slope, Hg, Wg)
    g = R.backward(acts, ggrid, W, flags, slope)
    gw = [*R.conv_wgrad(acts["pooled"], g["ga1"]), *R.conv_wgrad(acts["h1"], g["ga2"]),
          *R.linear_wgrad(acts["h2"], g["g3"]), *R.linear_wgrad(acts["h3"], g["g4"])]
    return acts, g, gw


def tight(a, b, what):
    scale = max(float(np.abs(b).max()), 1e-300)
    d = float(np.abs(np.asarray(a) - b).max())
    assert np.asarray(a).shape == b.shape and d <= 1e-12 * scale, f"{what}: max|d| {d:.3e} against scale {scale:.3e}"


CASES = [(S, Cin, fl, (2 * S, 2 * S)) for (S, Cin) in ((4, 64), (8, 3), (16, 1)) for fl in R.FLAGS] + [(8, 3, (1, 1, 1), (5, 12)), (4, 64, (0, 1, 1), (1, 7))]


@pytest.mark.parametrize("S,Cin,flags,hw", CASES)
def test_stages_composed_equal_torch_fp64_autograd(S, Cin, flags, hw):
    rs = np.random.RandomState(S * 100 + Cin + 7 * R.nparams(flags))
    P, N, slope = R.nparams(flags), 3, 0.333
    W = make_weights(rs, S, Cin, P)
    x = rs.randn(N, 2 * S, 2 * S, Cin).astype(f32)
    ggrid = rs.randn(N, *hw, 2).astype(f32)
    acts, g, gw = stage_grads(x, W, flags, slope, *hw, ggrid)
    grid_t, gx_t, gw_t = torch_chain(x, W, flags, slope, *hw, ggrid)
    assert np.abs(acts["params"][:, 0]).max() < np.pi
    tight(acts["grid"], grid_t, "grid")
    tight(g["gx"], gx_t, "gx")      # the twin's LeakyReLU looks at the layers' inputs, the stages at the activations: slope > 0
    for a, b, nme in zip(gw, gw_t, ("w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4")):
        tight(a, b, "grad " + nme)


def oclose(a, b, rtol=1e-5, atol=1e-5, K=1024):
    """tests/test_oracle_vs_torch.py's close()."""
    s = max(1.0, np.sqrt(K / 1024.0))
    np.testing.assert_allclose(a, b, rtol=rtol * s, atol=atol * s)


@pytest.mark.parametrize("S,Cin,flags,hw", [(4, 64, (1, 1, 1), (8, 8)), (8, 3, (1, 0, 0), (5, 12)), (16, 1, (0, 1, 1), (32, 32)), (8, 3, (1, 1, 0), (16, 16))])
def test_stages_against_the_oracle_localisation_half(S, Cin, flags, hw):
    """Every stage on the ORACLE's previous buffer (so that its fp32 errors do not compound), at the tolerances test_oracle_vs_torch.py
    has for the same pieces: 1e-5 sqrt(K / 1024) for the convolutions, linear layers and pools, 1e-5 for the grid, rtol 1e-4 /
    atol 2e-4 for the parameters' gradient."""
    rs = np.random.RandomState(S + Cin)
    P, N, slope = R.nparams(flags), 3, 0.333
    W = make_weights(rs, S, Cin, P)
    x = rs.randn(N, 2 * S, 2 * S, Cin).astype(f32)
    ggrid = rs.randn(N, *hw, 2).astype(f32)
    st = O.SpatialTransformer(bool(flags[0]), bool(flags[1]), bool(flags[2]), 2 * S, Cin, O.RNG(1))
    mods = st.loc.mods
    for m, (w, b) in zip((mods[1], mods[3], mods[7], mods[9]), zip(W[0::2], W[1::2])):
        m.weight[...] = w; m.bias[...] = b
        m.grad_weight[...] = 0; m.grad_bias[...] = 0
    nhwc = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1))
    outs, h = [], np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    for m in mods:
        h = m.forward(h)
        outs.append(h)
    pooled, h1, m2, h2, h3, prm = nhwc(outs[0]), nhwc(outs[2]), nhwc(outs[4]), outs[6], outs[8], outs[9]
    agg = O.AffineGrid(*hw)
    grid = agg.forward(st.atm.forward(prm))
    oclose(pooled, R.avgpool2(x)[0])
    oclose(h1, R.conv_lrelu(pooled, W[0], W[1], slope)[0], K=9 * Cin)
    oclose(m2, R.conv_lrelu(h1, W[2], W[3], slope)[0], K=144)
    oclose(h2, R.pool_flatten(m2)[0])
    oclose(h3, R.linear_lrelu(h2, W[4], W[5], slope)[0], K=h2.shape[1])
    oclose(prm, R.linear(h3, W[6], W[7])[0])
    oclose(grid, R.grid_from_params(prm, flags, *hw)[0])
    # backward: the oracle's modules keep their inputs; each stage takes the oracle's incoming gradient
    g4 = st.atm.backward(agg.backward(ggrid))
    oclose(g4, R.g4_from_ggrid(ggrid, prm, flags)[0], rtol=1e-4, atol=2e-4)
    gs, gcur = {}, g4
    for i in range(9, -1, -1):
        gs[i] = gcur                     # the gradient w.r.t. module i's output
        gcur = mods[i].backward(gcur)
    g3, ga2, ga1, gx = gs[7], nhwc(gs[3]), nhwc(gs[1]), nhwc(gcur)
    oclose(g3, R.g3_from_g4(g4, h3, W[6], slope)[0])
    oclose(ga2, R.ga2_from_g3(g3, m2, W[4], slope)[0])
    oclose(ga1, R.ga1_from_ga2(ga2, h1, W[2], slope)[0], K=144)
    oclose(gx, R.gx_from_ga1(ga1, W[0])[0], K=144)
    K = N * S * S
    for m, (gw, gb) in zip((mods[1], mods[3], mods[7], mods[9]),
                           (R.conv_wgrad(pooled, ga1), R.conv_wgrad(h1, ga2), R.linear_wgrad(h2, g3), R.linear_wgrad(h3, g4))):
        oclose(m.grad_weight, gw, K=K, atol=1e-4)
        oclose(m.grad_bias, gb, K=K, atol=1e-4)


def test_trig_error_of_the_reference_side_is_within_the_recorded_figure():
    """locnet_ref.TRIG_ULP is four times the error measured for numpy's fp32 sin / cos (TRIG_ULP_MEASURED); another numpy build may
    measure another figure, which has to stay inside that factor for the GPU test's bound to mean what it says."""
    got = R.trig_ulp_measured()
    print(f"numpy fp32 sin / cos against fp64 over |theta| < pi: {got:.3f} ulp (recorded {R.TRIG_ULP_MEASURED}, allowed {R.TRIG_ULP})")
    assert 0.4 <= got <= R.TRIG_ULP


def test_terms_bound_the_values_and_count_every_addend():
    """terms >= |value| everywhere, with equality where all addends have one sign (all-positive inputs)."""
    rs = np.random.RandomState(3)
    S, Cin, flags = 8, 6, (1, 1, 1)
    W = [np.abs(w) for w in make_weights(rs, S, Cin, 4)]
    x = np.abs(rs.randn(2, 2 * S, 2 * S, Cin)).astype(f32)
    v, t = R.avgpool2(x)
    np.testing.assert_allclose(t, v, rtol=1e-15)
    v1, t1 = R.conv_lrelu(v.astype(f32), W[0], W[1], 0.333)
    np.testing.assert_allclose(t1, v1, rtol=1e-14)
    g = rs.randn(2, S, S, 16).astype(f32)
    for v2, t2 in (R.gx_from_ga1(g, W[0]), R.ga1_from_ga2(g, v1.astype(f32), W[2], 0.333), R.gT_from_ggrid(rs.randn(2, 5, 12, 2)),
                   R.affine_T(rs.randn(4, 4), flags), R.g4_from_ggrid(rs.randn(4, 5, 12, 2), rs.randn(4, 4), flags)):
        assert (t2 >= np.abs(v2) * (1 - 1e-12)).all()
