"""tests/update_ref.py checked on its own, without a GPU: the fp64 twin against the in-tree fp32 oracle (O.adam, O.sgd, O.adagrad and the
penalty and clamp lines of Trainer.feval_D / feval_G) on seeded data, in the measure the GPU sweep uses, fused_args against the option
table it restates, and every case of tests/test_gpu_update_kernels.py against the regime its row states."""
import importlib

import numpy as np
import pytest

import test_gpu_update_kernels as E
import update_ref as R
from helpers import U24, bits_equal, edge_normal, ew_grid, rounding_close
from oracle import oracle as O

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("cat-generator_amd").lib()


def data(n=4099, seed=3):
    rng = np.random.default_rng(seed)
    p, g = edge_normal(rng, (n, 1)).ravel(), edge_normal(rng, (n, 1)).ravel()
    return p, g, (rng.standard_normal(n) * 0.1).astype(f32), (rng.random(n) * 0.1).astype(f32)


# ------------------------------------------------------------------------------ the twin against the fp32 oracle
def test_adam_twin_against_the_oracle():
    """O.adam rounds the double 1 - b where the twin (as the kernel) forms 1 - b from the fp32 b, and takes its bias corrections from the
    double betas: the slacks test_optimiser_kernels_past_the_wrap derives for the same two differences, with r roundings (one fp32
    implementation against fp64) where that test has 2 r (two fp32 implementations)."""
    p0, g, m0, v0 = data()
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    for t in (1, 2, 7):
        po, st = p0.copy(), {"t": t - 1, "m": m0.copy(), "v": v0.copy()}
        O.adam(po, g, st, lr=lr, b1=b1, b2=b2, eps=eps)
        (p1, m1, v1), (tp, tm, tv) = R.adam(p0, g, m0, v0, lr, b1, b2, eps, t)
        dm, dv = U24 * np.abs(g.astype(f64)), U24 * g.astype(f64) ** 2
        rounding_close(st["m"], m1, tm, R.R_ADAM_M, f"adam m, t = {t}", slack=dm)
        rounding_close(st["v"], v1, tv, R.R_ADAM_V, f"adam v, t = {t}", slack=dv)
        step, den = R.adam_step_size(lr, b1, b2, t), np.sqrt(tv) + eps
        dstep = U24 * (1 + t * b1 ** t / (1 - b1 ** t) + 0.5 * t * b2 ** t / (1 - b2 ** t))
        rounding_close(po, p1, tp, R.R_ADAM_P, f"adam p, t = {t}", slack=step * (dm + tm * 0.5 * dv / np.maximum(tv, 1e-300) + tm * dstep) / den)


def test_sgd_twin_against_the_oracle():
    p0, g, v0, _ = data()
    for mom in (0.0, 0.9):
        po, st = p0.copy(), ({"v": v0.copy()} if mom else {})
        O.sgd(po, g, st, lr=0.02, momentum=mom)
        (p1, d1), (tp, td) = R.sgd(p0, g, v0, 0.02, mom, mom)
        dd = U24 * np.abs(g.astype(f64)) if mom else 0.0          # f32(1 - momentum) against 1 - f32(momentum)
        rounding_close(po, p1, tp, R.R_SGD_P if mom else R.R_SGD_P0, f"sgd p, momentum {mom}", slack=0.02 * dd)
        if mom:
            rounding_close(st["v"], d1, td, R.R_SGD_V, "sgd v", slack=dd)
    # the first step with momentum: the oracle copies g, the twin reaches the same through zero velocity and dampening 0
    po, st = p0.copy(), {}
    O.sgd(po, g, st, lr=0.02, momentum=0.9)
    (p1, d1), (tp, _) = R.sgd(p0, g, np.zeros_like(g), 0.02, 0.9, 0.0)
    np.testing.assert_array_equal(d1, g.astype(f64))
    np.testing.assert_array_equal(st["v"], g)
    rounding_close(po, p1, tp, R.R_SGD_P0, "sgd first step p")


def test_adagrad_twin_against_the_oracle():
    p0, g, _, v0 = data()
    po, st = p0.copy(), {"var": v0.copy()}
    O.adagrad(po, g, st, lr=3e-3)
    (p1, var1), (tp, tvar) = R.adagrad(p0, g, v0, 3e-3)
    rounding_close(st["var"], var1, tvar, R.R_ADAGRAD_VAR, "adagrad var")
    rounding_close(po, p1, tp, R.R_ADAGRAD_P, "adagrad p")


def test_ema_twin_is_optims_restatement():
    optim = importlib.import_module("cat-generator_amd.optim")
    p0, g, _, _ = data()
    for n in (1, 2, 9, 8990, 8991):
        d = R.ema_decay(0.999, n)
        assert d == optim.ema_decay(0.999, n)
        np.testing.assert_array_equal(R.ema(g, p0, d)[0], optim.ema_np(g, p0, d))


def tiny_trainer(**opt):
    rng = O.RNG(5)
    G = O.Sequential(O.Linear(6, 40, rng), O.Sigmoid())
    D = O.Sequential(O.Linear(40, 1, rng), O.Sigmoid())
    T = O.Trainer(G, D, **opt)
    for q in (T.pD, T.pG):                      # +-0.0 and a denormal-range value among the parameters: sign(0) = 0
        q[:4] = [0.0, -0.0, 1e-30, -1e-30]
    return T


PENALTIES = [dict(D_L1=0.0, D_L2=0.0, G_L1=0.0, G_L2=0.0), dict(D_L1=0.03, D_L2=0.0, G_L1=0.03, G_L2=0.0),
             dict(D_L1=0.0, D_L2=0.25, G_L1=0.0, G_L2=0.25), dict(D_L1=0.03, D_L2=0.25, G_L1=0.03, G_L2=0.25)]


@pytest.mark.parametrize("pen", PENALTIES)
@pytest.mark.parametrize("clamped", [False, True])
def test_penalise_and_fused_args_against_the_trainers_own_lines(pen, clamped):
    """Trainer.feval_D / feval_G with every option zero give the raw gradient; with the options set, the same pass gives what the
    oracle hands to its optimiser and reports as the loss.  penalise(raw, *fused_args(...)[:3]) and penalty_loss must say the same - for
    G that includes the sign term scaled by G_L2."""
    rs = np.random.RandomState(1)
    x, z = rs.rand(8, 40).astype(f32), (rs.rand(8, 6) * 2 - 1).astype(f32)
    tD, tG = np.array([1, 1, 1, 1, 0, 0, 0, 0], f32), np.ones(8, f32)
    raw = tiny_trainer(D_L1=0.0, D_L2=0.0, G_L1=0.0, G_L2=0.0, D_clamp=0.0, G_clamp=0.0)
    fD0, _ = raw.feval_D(x, tD)
    gD0 = raw.gD.copy()                         # feval_G's pass through D adds to gD
    fG0 = raw.feval_G(z, tG)[0]
    # a clamp at the median magnitude of the raw gradient cuts half of the elements and spares the other half
    opt = dict(pen, D_clamp=float(np.median(np.abs(gD0))) if clamped else 0.0, G_clamp=float(np.median(np.abs(raw.gG))) if clamped else 0.0)
    T = tiny_trainer(**opt)
    fD, _ = T.feval_D(x, tD)
    gD1 = T.gD.copy()
    fG = T.feval_G(z, tG)[0]
    for which, p, g0, g1, f0, f1 in (("D", T.pD, gD0, gD1, fD0, fD), ("G", T.pG, raw.gG, T.gG, fG0, fG)):
        l1, l2, clamp = R.fused_args(opt, which, "adam")[:3]
        gref, terms = R.penalise(p, g0, l1, l2, clamp)
        if clamp:
            assert (np.abs(g0) > clamp).any() and (np.abs(g0) < clamp).any(), "the clamp must cut some elements and spare others"
        rounding_close(g1, gref, terms, R.R_PEN, f"{which}: the oracle's penalised and clamped gradient, {opt}")
        add = R.penalty_loss(opt, which, p)
        assert abs((f1 - f0) - add) <= 1e-12 * max(1.0, abs(add)) + 4 * np.spacing(abs(f1)), (which, f1 - f0, add)


def test_fused_args_table():
    """adversarial.lua:92-112, 201-212 and train.lua:191-207, case by case."""
    fa = R.fused_args
    assert fa({}, "D", "adam") == (0.0, 1e-4, 1.0, 1e-3, 0.0, 0.0)
    assert fa({}, "G", "adam") == (0.0, 0.0, 5.0, 1e-3, 0.0, 0.0)
    assert fa(dict(D_L1=3e-5), "D", "adam")[:3] == (3e-5, 1e-4, 1.0)
    assert fa(dict(G_L1=1e-3, G_L2=0.0), "G", "adam")[:3] == (0.0, 0.0, 5.0)          # line 206: G_L1 never reaches the gradient
    assert fa(dict(G_L1=0.0, G_L2=2e-4), "G", "adam")[:3] == (2e-4, 2e-4, 5.0)        # ... and the sign term carries G_L2
    assert fa(dict(D_clamp=0, G_clamp=0), "D", "sgd")[2] == 0 and fa(dict(D_clamp=0, G_clamp=0), "G", "sgd")[2] == 0
    assert fa({}, "D", "adagrad")[3:] == (1e-3, 0.0, 0.0) and fa({}, "G", "adagrad")[3:] == (3e-3, 0.0, 0.0)
    assert fa({}, "D", "sgd")[3:] == (0.02, 0.0, 0.0)
    assert fa(dict(D_sgd_momentum=0.9, G_sgd_lr=0.05), "D", "sgd")[3:] == (0.02, 0.9, 0.9)
    assert fa(dict(D_sgd_momentum=0.9, G_sgd_lr=0.05), "G", "sgd")[3:] == (0.05, 0.0, 0.0)


def test_fp32_restatements_of_the_separate_passes():
    p = np.array([0.0, -0.0, 1e-30, -1e-30, 2.0, -3.0, np.nan], f32)
    y = np.array([1.0, 1.0, 1.0, 1.0, -0.0, 0.25, 1.0], f32)
    bits_equal(R.axpy_sign32(0.25, p, y), np.array([1.0, 1.0, 1.25, 0.75, 0.25, 0.0, 1.0], f32), "axpy_sign32")
    bits_equal(R.clamp32(np.array([-2.0, -0.0, 0.5, 2.0], f32), -1.0, 1.0), np.array([-1.0, -0.0, 0.5, 1.0], f32), "clamp32")


# ------------------------------------------------------------------------------ the regimes of the GPU sweep
def test_every_case_is_in_the_regime_it_names(L):
    cap = E.ew_cap(L)
    for n, mis, want in E.CASES:
        assert E.regime(n, mis, cap) == want, (n, mis)
        blocks = ew_grid(n, cap)                                  # the launch itself: one workgroup, several, or fewer lanes than elements
        assert {"one": blocks == 1, "many": 1 < blocks and n <= blocks * 256, "wrap": n > blocks * 256}[want[0]], (n, blocks)
        v4, tail = want[1]
        if v4:                                                    # adam_ema_k<4> / ema_k<4>: n / 4 lanes, never a wrap at these lengths
            assert n // 4 <= ew_grid(n // 4, cap) * 256 and tail == n - n // 4 * 4
    assert E.ew_regime(E.OPT_N, cap) == "wrap"


def test_the_cases_cover_what_the_kernels_branch_on():
    regs = [w for _, _, w in E.CASES]
    assert {r[0] for r in regs} == {"one", "many", "wrap"}
    assert any(r[1] == (True, 3) for r in regs) and any(r[1] == (True, 0) for r in regs) and any(r[1] == (False, 0) for r in regs)
    assert any(r[2] for r in regs) and any(not r[2] and n % 4 == 0 for n, _, r in E.CASES)
    assert {256 - 1, 256, 256 + 1} <= {n for n, _, _ in E.CASES}
    assert (0.0, 0.0, 0.0) in E.PEN and len({(bool(a), bool(b), bool(c)) for a, b, c in E.PEN}) == 6


def test_planted_values_are_where_the_docstring_says():
    """+-0.0 and +-1e-30 in p; g at +-C, one ulp either side; elements only the penalty carries across the clamp; cancelling sums."""
    a = E.inputs(1027)
    p, g = a["p"], a["g"]
    c = f32(E.C)
    assert (p == 0).sum() >= 2 and np.signbit(p[p == 0]).any() and not np.signbit(p[p == 0]).all() and (np.abs(p) == f32(1e-30)).any()
    for v in (c, -c, np.nextafter(c, f32(9)), np.nextafter(-c, f32(-9)), np.nextafter(c, f32(0)), np.nextafter(-c, f32(0))):
        assert (g == v).any(), v
    pen = R.sign(p) * R.c32(E.A) + p.astype(f64) * R.c32(E.B)
    both, _ = R.penalise(p, g, E.A, E.B, E.C)
    clamp_first = np.clip(g.astype(f64), -E.C, E.C) + pen
    carried = (np.abs(g) < c) & (np.abs(both) == c) & (np.abs(clamp_first - both) > 1e-3)
    assert carried.sum() >= 4, "elements whose clamped value depends on the order of penalty and clamp"
    assert (np.abs(g.astype(f64) + R.c32(E.B) * p.astype(f64)) <= U24 * np.abs(g)).sum() >= 4, "g = -l2 p"
    assert (a["v"] == 0).any() and (a["v"] >= 0).all()
