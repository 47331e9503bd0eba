"""The localisation chain of a spatial transformer (csrc/locnet.hip; models.lua:842-860, :877-878) restated in fp64, stage by stage
(a plain module, imported as tests/plan_trace.py is).  Every stage takes fp32 arrays in the layouts of include/catgan.h's locnet
section - images NHWC, canonical Torch7 weights - and returns (value, terms): the fp64 value and, per element, the sum of the
magnitudes of its addends, which is what helpers.rounding_close scales its bound by.  The backward stages are pure functions of the
arrays cg_locnet_backward takes: LeakyReLU's side there is the test `>= 0` on the GIVEN activation array.

The affine stages multiply R(theta) S(s) Tr(tx, ty) out as 3x3 matrices and let torch autograd differentiate the product: no closed
form of T's entries or of their derivatives is typed in here.  `terms` of those stages come from the same product of the matrices'
magnitudes."""
import numpy as np
import torch

f64 = np.float64
LC, LH = 16, 64           # planes of both convolutions, hidden units of the first linear layer

FLAGS = [(r, s, t) for r in (1, 0) for s in (1, 0) for t in (1, 0) if r or s or t]      # the seven non-empty (rot, scale, trans)


def nparams(flags):
    return int(flags[0]) + int(flags[1]) + 2 * int(flags[2])


def a64(a):
    return np.asarray(a, dtype=f64)


# ------------------------------------------------------------------------------ forward stages
def avgpool2(x):
    """[N][H][W][C] -> [N][H/2][W/2][C]: the mean of each 2x2 window."""
    x = a64(x)
    N, H, W, C = x.shape
    q = x.reshape(N, H // 2, 2, W // 2, 2, C)
    return 0.25 * q.sum((2, 4)), 0.25 * np.abs(q).sum((2, 4))


def _corr3(x, w):
    """3x3 / pad 1 cross-correlation, x [N][S][S][Ci] NHWC, w [Co][Ci][3][3] -> [N][S][S][Co]."""
    N, H, W, _ = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((N, H, W, w.shape[0]), f64)
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("nyxc,oc->nyxo", xp[:, ky:ky + H, kx:kx + W, :], w[:, :, ky, kx])
    return out


def lrelu(pre, terms, slope):
    """LeakyReLU.lua: x >= 0 passes.  terms stay those of the pre-activation on either side (|slope| <= 1): where fp32 lands on the other
    side of the kink than fp64 both values lie within the pre-activation's own bound of zero, and LeakyReLU is 1-Lipschitz."""
    assert abs(slope) <= 1.0
    return np.where(pre >= 0, pre, slope * pre), terms


def conv_lrelu(x, w, b, slope):
    """lrelu(conv3x3(x, w) + b): x [N][S][S][Ci], w [16][Ci][3][3], b [16]."""
    x, w, b = a64(x), a64(w), a64(b)
    return lrelu(_corr3(x, w) + b, _corr3(np.abs(x), np.abs(w)) + np.abs(b), slope)


def pool_flatten(m2):
    """h2: the 2x2 mean of m2 [N][S][S][16], flattened per sample in (c, y, x) order as nn.View leaves the NCHW map."""
    v, t = avgpool2(m2)
    fl = lambda a: np.ascontiguousarray(a.transpose(0, 3, 1, 2)).reshape(a.shape[0], -1)
    return fl(v), fl(t)


def linear(x, w, b):
    x, w, b = a64(x), a64(w), a64(b)
    return x @ w.T + b, np.abs(x) @ np.abs(w).T + np.abs(b)


def linear_lrelu(x, w, b, slope):
    return lrelu(*linear(x, w, b), slope)


# ------------------------------------------------------------------------------ the affine stages
def _matrices(p, flags, magnitudes=False):
    """R, S, Tr [N][3][3] (torch fp64) of params p [N][P], consumed in the order [theta][s][tx, ty]; acting on (y, x, 1).
    magnitudes: every entry replaced by its magnitude (the factors of `terms`)."""
    N = p.shape[0]
    one, zero = torch.ones(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    k = 0
    th, sc, tx, ty = zero, one, zero, zero
    if flags[0]:
        th = p[:, k]; k += 1
    if flags[1]:
        sc = p[:, k]; k += 1
    if flags[2]:
        tx, ty = p[:, k], p[:, k + 1]; k += 2
    assert k == p.shape[1], "P does not match the flags"
    c, s = torch.cos(th), torch.sin(th)
    m = (lambda v: v.abs()) if magnitudes else (lambda v: v)
    rows = lambda *r: torch.stack([torch.stack(list(x), 1) for x in r], 1)
    R = rows((m(c), m(-s), zero), (m(s), m(c), zero), (zero, zero, one))
    S = rows((m(sc), zero, zero), (zero, m(sc), zero), (zero, zero, one))
    Tr = rows((one, zero, m(tx)), (zero, one, m(ty)), (zero, zero, one))
    return R, S, Tr


def affine_T(params, flags):
    """T [N][2][3]: the top two rows of R S Tr."""
    p = torch.tensor(a64(params))
    R, S, Tr = _matrices(p, flags)
    Ra, Sa, Ta = _matrices(p, flags, True)
    return (R @ S @ Tr)[:, :2].numpy(), (Ra @ Sa @ Ta)[:, :2].numpy()


def _coords(Hg, Wg):
    """(y_i, x_j, 1) per grid point [Hg][Wg][3] and the magnitudes of the addends of each: y_i = -1 + 2 i / (Hg - 1), -1 for Hg == 1."""
    ax = lambda n: (-1.0 + 2.0 * np.arange(n, dtype=f64) / (n - 1)) if n > 1 else np.full(1, -1.0)
    axt = lambda n: (1.0 + 2.0 * np.arange(n, dtype=f64) / (n - 1)) if n > 1 else np.full(1, 1.0)
    y, x = np.meshgrid(ax(Hg), ax(Wg), indexing="ij")
    yt, xt = np.meshgrid(axt(Hg), axt(Wg), indexing="ij")
    one = np.ones_like(y)
    return np.stack([y, x, one], -1), np.stack([yt, xt, one], -1)


def grid_from_T(T, T_terms, Hg, Wg):
    """AffineGridGeneratorBHWD: grid[n, i, j, :] = T_n (y_i, x_j, 1) -> [N][Hg][Wg][2].  T_terms: |T| for a T given as data."""
    c, ct = _coords(Hg, Wg)
    return np.einsum("nrk,ijk->nijr", a64(T), c), np.einsum("nrk,ijk->nijr", a64(T_terms), ct)


def grid_from_params(params, flags, Hg, Wg):
    return grid_from_T(*affine_T(params, flags), Hg, Wg)


def gT_from_ggrid(ggrid):
    """AffineGridGeneratorBHWD backward: gT[n][r][:] = sum_ij ggrid[n, i, j, r] (y_i, x_j, 1) -> [N][2][3]."""
    g = a64(ggrid)
    c, ct = _coords(g.shape[1], g.shape[2])
    return np.einsum("nijr,ijk->nrk", g, c), np.einsum("nijr,ijk->nrk", np.abs(g), ct)


def g4_from_gT(gT, gT_terms, params, flags):
    """AffineTransformMatrixGenerator backward by autograd of sum(gT * T(params)) -> [N][P].  gT_terms: |gT| for a gT given as data."""
    p = torch.tensor(a64(params), requires_grad=True)
    R, S, Tr = _matrices(p, flags)
    ((R @ S @ Tr)[:, :2] * torch.tensor(a64(gT))).sum().backward()
    # terms: sum_k gT_terms[k] * (the magnitudes' product with the differentiated factor's magnitudes in place)
    Ra, Sa, Ta = (m.detach() for m in _matrices(p.detach(), flags, True))
    N = p.shape[0]
    E = lambda pairs: torch.tensor([[1.0 if (i, j) in pairs else 0.0 for j in range(3)] for i in range(3)], dtype=torch.float64).expand(N, 3, 3)
    dRa = Ra[:, [1, 0, 2]] * E({(0, 0), (0, 1), (1, 0), (1, 1)})       # |dR/dtheta|: |cos| and |sin| change places, the constant row goes
    cols = []
    if flags[0]:
        cols.append(dRa @ Sa @ Ta)
    if flags[1]:
        cols.append(Ra @ E({(0, 0), (1, 1)}) @ Ta)
    if flags[2]:
        cols += [Ra @ Sa @ E({(0, 2)}), Ra @ Sa @ E({(1, 2)})]
    gt = torch.tensor(a64(gT_terms))
    terms = torch.stack([(d[:, :2] * gt).sum((1, 2)) for d in cols], 1)
    return p.grad.numpy(), terms.numpy()


def g4_from_ggrid(ggrid, params, flags):
    return g4_from_gT(*gT_from_ggrid(ggrid), params, flags)


# ------------------------------------------------------------------------------ backward stages
def _dact(h, g, terms, slope):
    side = np.asarray(h) >= 0            # the sign test on the given activation array (-0.0 passes)
    return np.where(side, g, slope * g), np.where(side, terms, abs(slope) * terms)


def g3_from_g4(g4, h3, w4, slope):
    """g3[k] = lrelu'(h3[k]) sum_p w4[p][k] g4[p] -> [N][64]."""
    g4, w4 = a64(g4), a64(w4)
    return _dact(h3, g4 @ w4, np.abs(g4) @ np.abs(w4), slope)


def ga2_from_g3(g3, m2, w3, slope):
    """Linear 1's data gradient [N][K3] in (c, y, x) order, the pooling's backward (x 0.25 to each pixel of the window), LeakyReLU's
    backward at conv 2's output -> [N][S][S][16]."""
    g3, w3 = a64(g3), a64(w3)
    N, S = m2.shape[0], m2.shape[1]
    up = lambda a: 0.25 * a.reshape(N, LC, S // 2, S // 2).repeat(2, 2).repeat(2, 3).transpose(0, 2, 3, 1)
    return _dact(m2, up(g3 @ w3), up(np.abs(g3) @ np.abs(w3)), slope)


def _dgrad3(dy, w):
    """Data gradient of the 3x3 / pad 1 convolution with w [Co][Ci][3][3]: dx[ci] at q = sum_{tap, co} dy[q - off(tap)][co] w[co][ci][tap]."""
    return _corr3(dy, np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3)))


def ga1_from_ga2(ga2, h1, w2, slope):
    ga2, w2 = a64(ga2), a64(w2)
    return _dact(h1, _dgrad3(ga2, w2), _dgrad3(np.abs(ga2), np.abs(w2)), slope)


def gx_from_ga1(ga1, w1):
    """conv 1's data gradient, then the first pooling's backward -> [N][2S][2S][Cin]."""
    ga1, w1 = a64(ga1), a64(w1)
    up = lambda a: 0.25 * a.repeat(2, 1).repeat(2, 2)
    return up(_dgrad3(ga1, w1)), up(_dgrad3(np.abs(ga1), np.abs(w1)))


# ------------------------------------------------------------------------------ the composed chain (tests/test_locnet_ref_host.py)
def forward(x, W, flags, slope, Hg, Wg):
    """All seven forward buffers in fp64, each stage on the previous one's fp64 value.  W: the eight canonical tensors."""
    w1, b1, w2, b2, w3, b3, w4, b4 = W
    pooled = avgpool2(x)[0]
    h1 = conv_lrelu(pooled, w1, b1, slope)[0]
    m2 = conv_lrelu(h1, w2, b2, slope)[0]
    h2 = pool_flatten(m2)[0]
    h3 = linear_lrelu(h2, w3, b3, slope)[0]
    params = linear(h3, w4, b4)[0]
    grid = grid_from_params(params, flags, Hg, Wg)[0]
    return dict(pooled=pooled, h1=h1, m2=m2, h2=h2, h3=h3, params=params, grid=grid)


def backward(acts, ggrid, W, flags, slope):
    w1, b1, w2, b2, w3, b3, w4, b4 = W
    g4 = g4_from_ggrid(ggrid, acts["params"], flags)[0]
    g3 = g3_from_g4(g4, acts["h3"], w4, slope)[0]
    ga2 = ga2_from_g3(g3, acts["m2"], w3, slope)[0]
    ga1 = ga1_from_ga2(ga2, acts["h1"], w2, slope)[0]
    gx = gx_from_ga1(ga1, w1)[0]
    return dict(g4=g4, g3=g3, ga2=ga2, ga1=ga1, gx=gx)


def conv_wgrad(x, dy):
    """Weight and bias gradient of a 3x3 / pad 1 convolution from its input x [N][S][S][Ci] and dy [N][S][S][Co] -> [Co][Ci][3][3], [Co]."""
    x, dy = a64(x), a64(dy)
    N, H, W, _ = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    gw = np.stack([np.stack([np.einsum("nyxc,nyxo->oc", xp[:, ky:ky + H, kx:kx + W, :], dy) for kx in range(3)], -1) for ky in range(3)], -2)
    return gw, dy.sum((0, 1, 2))


def linear_wgrad(x, dy):
    x, dy = a64(x), a64(dy)
    return dy.T @ x, dy.sum(0)


# ------------------------------------------------------------------------------ rounding counts (r of helpers.rounding_close)
# A sum of K addends, in any association and with or without fused multiply-adds, puts at most K roundings on an addend's way to the
# result (its product, then at most K - 1 additions); r = K + 2.  Multiplications by 0.25 are exact.
def r_sum(K):
    return K + 2


# sinf / cosf: no accuracy table ships with the ROCm installation, so the figure is the reference side's own - the worst error of
# numpy's fp32 sin / cos against fp64 over |theta| < pi, trig_ulp_measured(): 1.42 ulp (numpy's vectorised float32 loops) - times 4
# for a different libm.  One ulp is at most 2 U24 of the value, so the error counts as 2 * TRIG_ULP roundings, rounded up.
TRIG_ULP_MEASURED = 1.42
TRIG_ULP = 4 * TRIG_ULP_MEASURED
R_TRIG = int(np.ceil(2 * TRIG_ULP))
R_T = R_TRIG + 3 + 2                  # cos -> * sc -> * tx -> the difference of the two products
R_GRID_T = 2 + 1 + 2 + 2              # T given: y_i (a quotient, a sum), its product with T, two additions
R_GRID = R_TRIG + 1 + 2 + 1 + 2 + 2   # from params: (cos * sc) * y_i, two additions (the T[2] path is shorter)
R_GT = 2 + 1 + 1 + 2                  # y_i, the fp32 product, (fp64 sum), the cast to fp32
R_G4_T = R_TRIG + 3 + 1 + 5 + 2       # gT given: a derivative entry as T[2], its product with gT, the six-term sum
R_G4 = R_GT - 2 + R_G4_T              # from ggrid


def trig_ulp_measured(theta=None):
    """Worst error, in ulps of the fp32 result, of numpy's fp32 sin and cos against fp64 over fp32 angles in (-pi, pi)."""
    if theta is None:
        rs = np.random.RandomState(0)
        theta = np.concatenate([np.linspace(-3.1415, 3.1415, 1 << 20), rs.uniform(-1e-3, 1e-3, 1 << 14),
                                np.pi / 2 + rs.uniform(-1e-3, 1e-3, 1 << 14), -np.pi / 2 + rs.uniform(-1e-3, 1e-3, 1 << 14)])
    t = np.asarray(theta, np.float32)
    worst = 0.0
    for fn in (np.sin, np.cos):
        got, ref = fn(t).astype(f64), fn(t.astype(f64))
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(f64)
        worst = max(worst, float((np.abs(got - ref) / ulp).max()))
    return worst
