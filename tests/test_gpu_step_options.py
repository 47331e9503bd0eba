"""The host plumbing that turns OPT into kernel arguments (adversarial.iteration, optim.py), step by step, at the options no other test
sets: D_L1, G's sign term scaled by G_L2 (adversarial.lua:206, kept), clamp = 0, sgd with momentum and adagrad for either net with
their own learning rates, several D and G iterations, the running average behind an sgd step, and the accuracy gate.  G16up / D32_st3
at 16 px, batch 8, injected rows and noise.

A recorder wraps optim.adam / sgd / adagrad and snapshots, around the real call, the parameters, the optimiser state, the gradient
as the closure returned it and as the kernel wrote it back, and the average.  Every recorded call is then checked on its own against
tests/update_ref.py with the measures and counts of tests/test_gpu_update_kernels.py - stage one: the written-back gradient against
penalise(x_before, g_from_opfunc, fused_args(OPT, ...)); stage two: x, state and average against the twin evaluated FROM the
written-back gradient - so nothing is compared across a forward pass and no bound has to allow for chaos.

Then one iteration against the CPU oracle for three of the configurations."""
import importlib

import numpy as np
import pytest
import torch

import scale16 as S16
import update_ref as R
from helpers import bits_equal, close, rounding_close
from oracle import oracle as O

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
N, SEED = 8, 31
U53 = 2.0 ** -53

CONFIGS = {
    "defaults": {},
    "D_L1": dict(D_L1=3e-5, D_L2=1e-4),
    "G_L1": dict(G_L1=1e-3, G_L2=0.0),
    "G_L2": dict(G_L1=0.0, G_L2=2e-4),                       # the sign term must carry 2e-4
    "no_clamp": dict(D_clamp=0, G_clamp=0),
    "sgd_adagrad": dict(D_optmethod="sgd", D_sgd_momentum=0.9, G_optmethod="adagrad"),
    "adagrad_sgd": dict(D_optmethod="adagrad", G_optmethod="sgd", G_sgd_momentum=0.9),
    "iterations": dict(D_iterations=2, G_iterations=3),
    "ema_sgd": dict(G_ema=0.999, G_optmethod="sgd"),         # the average runs behind the step
}


@pytest.fixture(scope="module")
def cg():
    mod = importlib.import_module("cat-generator_amd")
    assert torch.cuda.is_available(), "these tests need the MI355X"
    mod.lib()
    return mod


def opt_of(cfg):
    o = dict(R.DEFAULTS)
    o.update(cfg)
    return o


def make_state(cg, cfg, fused):
    cg.manual_seed(SEED)
    G, D = cg.models.create_G((3, 16, 16), 100), cg.models.create_D((3, 16, 16))
    S = cg.adversarial.State(dict(batchSize=N, fused_update=fused, **cfg), G, D)
    S.keep_outputs = True
    return S


def draws():
    """The pool and, per iteration, the injected real rows and the two noise batches: the same for every run."""
    rs = np.random.RandomState(9)
    pool = rs.rand(32, 3, 16, 16).astype(f32)
    its = [(rs.randint(0, 32, size=N // 2), (rs.rand(N // 2, 100) * 2 - 1).astype(f32), (rs.rand(N, 100) * 2 - 1).astype(f32)) for _ in range(3)]
    return pool, its


def snap(d):
    """Host copy of an optimiser state: vectors as arrays, counts and rates as they are (device counters left out)."""
    return {k: (v.numpy().copy() if hasattr(v, "numpy") and not isinstance(v, torch.Tensor) else v) for k, v in d.items()
            if not isinstance(v, torch.Tensor)}


class Recorder:
    """optim.adam / sgd / adagrad wrapped for one State: log[i] holds what went into and came out of the i-th call."""

    def __init__(self, cg, S, monkeypatch):
        self.log, self.S = [], S
        for name in ("adam", "sgd", "adagrad"):
            fn = getattr(cg.optim, name)
            monkeypatch.setattr(cg.optim, name, self.wrap(name, getattr(fn, "real", fn)))      # never a recorder around a recorder

    def wrap(self, name, real):
        S, log = self.S, self.log

        def wrapped(opfunc, x, config=None, state=None, fused=None, ema=None):
            assert x is S.PARAMETERS_D or x is S.PARAMETERS_G
            which = "D" if x is S.PARAMETERS_D else "G"
            st = state if state is not None else config
            rec = dict(method=name, which=which, x_before=x.numpy().copy(), state_before=snap(st), fused=fused, f=None, g_raw=None, g_after=None)
            if ema is not None:
                rec.update(e_before=ema["e"].numpy().copy(), n_before=ema["n"])
            held = {}

            def op(xx):
                f, g = opfunc(xx)
                rec["f"] = f if f is False else float(f)       # a lazily read device scalar: read it before the next criterion call reuses it
                rec["outputs"] = S._last["outputs_" + which].numpy().copy()
                if f is not False:
                    rec["g_raw"] = g.numpy().copy()
                    held["g"] = g
                return f, g

            out = real(op, x, config, state, fused=fused, ema=ema)
            rec.update(x_after=x.numpy().copy(), state_after=snap(st))
            if "g" in held:
                rec["g_after"] = held["g"].numpy().copy()
            if ema is not None:
                rec.update(e_after=ema["e"].numpy().copy(), n_after=ema["n"], decay=ema["decay"])
            log.append(rec)
            return out

        wrapped.real = real
        return wrapped


def run(cg, monkeypatch, cfg, fused, gates):
    """A fresh State, one iteration per entry of `gates` (maxAccuracyD: 1.01 = the gate cannot trigger, 0.0 = D is never updated) -> the
    records per iteration, the axpy_sign calls per iteration, the State."""
    S = make_state(cg, cfg, fused)
    rec = Recorder(cg, S, monkeypatch)
    pool, its = draws()
    data = cg.adversarial.TrainData(pool)
    L = cg.lib()
    per_it, signs = [], []
    for (idx, nd, ng), gate in zip(its, gates):
        k0 = len(rec.log)
        L.trace = []
        try:
            trained = cg.adversarial.iteration(S, data, N, maxAccuracyD=gate, real_idx=idx, noise_D=nd, noise_G=ng)
        finally:
            calls, L.trace = L.trace, None
        assert trained == (gate > 1.0)
        per_it.append(rec.log[k0:])
        signs.append([a for name, a in calls if name == "cg_axpy_sign"])
    return per_it, signs, S


def zeros_like(a):
    return np.zeros_like(a)


def check_record(rec, OPT, fused, what):
    """Stage one (fused runs) and stage two of one recorded call."""
    l1, l2, clamp, lr, mom, damp = R.fused_args(OPT, rec["which"], rec["method"])
    x0, x1, s0, s1, g1 = rec["x_before"], rec["x_after"], rec["state_before"], rec["state_after"], rec["g_after"]
    if fused:
        gref, terms = R.penalise(x0, rec["g_raw"], l1, l2, clamp)
        rounding_close(g1, gref, terms, R.R_PEN, what + ": g written back")
    else:       # the penalty was applied inside the closure; the kernel gets no penalty, no clamp and does not write g back
        assert rec["fused"] is None
        bits_equal(g1, rec["g_raw"], what + ": the separate-pass update leaves g as the closure made it")
    m = rec["method"]
    if m == "adam":
        t = s1["t"]
        assert t == s0.get("t", 0) + 1
        (p1, m1, v1), (tp, tm, tv) = R.adam(x0, g1, s0.get("m", zeros_like(x0)), s0.get("v", zeros_like(x0)), lr, R.ADAM["b1"], R.ADAM["b2"], R.ADAM["eps"], t)
        rounding_close(s1["m"], m1, tm, R.R_ADAM_M, what + ": adam m")
        rounding_close(s1["v"], v1, tv, R.R_ADAM_V, what + ": adam v")
        rounding_close(x1, p1, tp, R.R_ADAM_P, what + f": adam p, t = {t}")
    elif m == "sgd":
        first = "dfdx" not in s0
        assert s1["evalCounter"] == s0.get("evalCounter", 0) + 1 and s0.get("momentum", 0) == mom and R.c32(s0["learningRate"]) == R.c32(lr)
        if mom != 0:       # optim.sgd's first step with momentum copies the gradient: zero velocity, dampening 0
            (p1, d1), (tp, td) = R.sgd(x0, g1, zeros_like(x0) if first else s0["dfdx"], lr, mom, 0.0 if first else damp)
            rounding_close(s1["dfdx"], d1, td, R.R_SGD_V, what + ": sgd velocity")
            rounding_close(x1, p1, tp, R.R_SGD_P, what + ": sgd p")
            if first:
                assert np.array_equal(s1["dfdx"], g1), what + ": the first momentum step's velocity is g"       # 0.9 (+0) + 1 (-0) is +0: values, not signs of zero
        else:
            assert "dfdx" not in s1
            (p1, _), (tp, _) = R.sgd(x0, g1, None, lr, 0.0, 0.0)
            rounding_close(x1, p1, tp, R.R_SGD_P0, what + ": sgd p")
    else:
        assert s1["evalCounter"] == s0.get("evalCounter", 0) + 1 and R.c32(s0["learningRate"]) == R.c32(lr)
        (p1, var1), (tp, tvar) = R.adagrad(x0, g1, s0.get("paramVariance", zeros_like(x0)), lr)
        rounding_close(s1["paramVariance"], var1, tvar, R.R_ADAGRAD_VAR, what + ": adagrad var")
        rounding_close(x1, p1, tp, R.R_ADAGRAD_P, what + ": adagrad p")
    if "e_after" in rec:
        assert rec["which"] == "G" and rec["n_after"] == rec["n_before"] + 1
        e1, te = R.ema(rec["e_before"], x1, R.ema_decay(rec["decay"], rec["n_after"]))
        rounding_close(rec["e_after"], e1, te, R.R_EMA, what + f": the average, update {rec['n_after']}")
    assert (x1 != x0).any(), what + ": the update moved nothing"


def check_order(recs, OPT, what):
    want = [("D", OPT["D_optmethod"])] * OPT["D_iterations"] + [("G", OPT["G_optmethod"])] * OPT["G_iterations"]
    assert [(r["which"], r["method"]) for r in recs] == want, what


def check_unchanged(rec, what):
    """The gate's `return false, false`: parameters, every entry of the optimiser state and the step count stay as they were."""
    assert rec["f"] is False and rec["g_after"] is None
    bits_equal(rec["x_after"], rec["x_before"], what + ": parameters")
    assert rec["state_after"].keys() == rec["state_before"].keys(), what
    for k, v in rec["state_before"].items():
        if isinstance(v, np.ndarray):
            bits_equal(rec["state_after"][k], v, what + f": state[{k}]")
        else:
            assert rec["state_after"][k] == v, what + f": state[{k}]"


def check_loss(f_sep, f_fused, add, n, what):
    """The separate pass reports f + X_L1 |p|_1 + X_L2 |p|_2^2 / 2 with the norms summed in doubles (sumred_k): n 2^-53 of the sums, and
    the few double operations that combine them."""
    tol = (n + 8) * U53 * (abs(float(f_sep)) + add)
    print(f"{what}: f {float(f_sep)!r} = {float(f_fused)!r} + {add!r}, |d| = {abs(float(f_sep) - float(f_fused) - add):.3e} against {tol:.3e}")
    assert abs(float(f_sep) - float(f_fused) - add) <= tol, what


@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_update_of_two_iterations_against_the_twin(cg, monkeypatch, name):
    cfg, OPT = CONFIGS[name], opt_of(CONFIGS[name])
    # ---- fused: two open iterations, then one with the gate closed on a state that exists
    F, _, S = run(cg, monkeypatch, cfg, True, (1.01, 1.01, 0.0))
    for it in (0, 1):
        check_order(F[it], OPT, f"{name}, fused, iteration {it}")
        for k, rec in enumerate(F[it]):
            check_record(rec, OPT, True, f"{name}, fused, iteration {it}, call {k} ({rec['which']} {rec['method']})")
    check_order(F[2], OPT, f"{name}, fused, gated iteration")
    for k, rec in enumerate(F[2]):
        what = f"{name}, fused, gate closed, call {k} ({rec['which']} {rec['method']})"
        if rec["which"] == "D":
            check_unchanged(rec, what)
        else:
            check_record(rec, OPT, True, what)
    # ---- the separate passes: the same three iterations
    P, signs, S2 = run(cg, monkeypatch, cfg, False, (1.01, 1.01, 0.0))
    d_pen, g_pen = OPT["D_L1"] != 0 or OPT["D_L2"] != 0, OPT["G_L1"] != 0 or OPT["G_L2"] != 0
    for it in (0, 1, 2):
        check_order(P[it], OPT, f"{name}, separate, iteration {it}")
        for k, rec in enumerate(P[it]):
            what = f"{name}, separate, iteration {it}, call {k} ({rec['which']} {rec['method']})"
            if it == 2 and rec["which"] == "D":
                check_unchanged(rec, what)
            else:
                check_record(rec, OPT, False, what)
        # cg_axpy_sign runs for D only where D_L1 is set, with D_L1; for G wherever a G penalty is set, with G_L2 (adversarial.lua:206)
        want = [("D", OPT["D_L1"])] * (OPT["D_iterations"] if d_pen and OPT["D_L1"] != 0 else 0) + [("G", OPT["G_L2"])] * (OPT["G_iterations"] if g_pen else 0)
        got = [("D" if a[2] == S2.PARAMETERS_D.ptr else "G" if a[2] == S2.PARAMETERS_G.ptr else "?", a[1]) for a in signs[it]]
        assert got == want, f"{name}, separate, iteration {it}: cg_axpy_sign calls {got}"
    # D's first update of the first iteration: the raw gradient is the fused run's bit for bit (same parameters, same draws, same
    # launches up to here - asserted on D's outputs), so its penalised gradient is checked against the fused run's stage-one reference
    a, b = F[0][0], P[0][0]
    assert a["which"] == b["which"] == "D"
    bits_equal(b["outputs"], a["outputs"], f"{name}: D's outputs in front of its first update, separate against fused")
    bits_equal(b["x_before"], a["x_before"], f"{name}: D's parameters in front of its first update")
    l1, l2, clamp = R.fused_args(OPT, "D", OPT["D_optmethod"])[:3]
    gref, terms = R.penalise(a["x_before"], a["g_raw"], l1, l2, clamp)
    rounding_close(b["g_raw"], gref, terms, R.R_SEP, f"{name}: D's gradient behind the separate passes")
    check_loss(b["f"], a["f"], R.penalty_loss(OPT, "D", a["x_before"]), a["x_before"].size, f"{name}: f_D of the separate pass")


@pytest.mark.parametrize("name", list(CONFIGS))
def test_closed_gate_leaves_d_alone_and_shows_gs_raw_gradient(cg, monkeypatch, name):
    """With maxAccuracyD = 0.0 from the first iteration D is never updated, so G's raw gradient in the separate-pass run is the fused
    run's bit for bit (asserted on D's outputs in the G-step) and its penalised gradient meets the fused run's stage-one reference."""
    cfg, OPT = CONFIGS[name], opt_of(CONFIGS[name])
    F, _, S = run(cg, monkeypatch, cfg, True, (0.0,))
    P, _, S2 = run(cg, monkeypatch, cfg, False, (0.0,))
    for recs, fused, St in ((F[0], True, S), (P[0], False, S2)):
        check_order(recs, OPT, f"{name}, gate closed from the start")
        for k, rec in enumerate(recs):
            what = f"{name}, {'fused' if fused else 'separate'}, gate closed from the start, call {k} ({rec['which']} {rec['method']})"
            if rec["which"] == "D":
                check_unchanged(rec, what)
                assert "t" not in rec["state_after"] and "evalCounter" not in rec["state_after"], what + ": a count moved"
            else:
                check_record(rec, OPT, fused, what)
    a, b = F[0][OPT["D_iterations"]], P[0][OPT["D_iterations"]]
    assert a["which"] == b["which"] == "G"
    bits_equal(b["outputs"], a["outputs"], f"{name}: D's outputs in G's first step, separate against fused")
    l1, l2, clamp = R.fused_args(OPT, "G", OPT["G_optmethod"])[:3]
    gref, terms = R.penalise(a["x_before"], a["g_raw"], l1, l2, clamp)
    rounding_close(b["g_raw"], gref, terms, R.R_SEP, f"{name}: G's gradient behind the separate passes")
    check_loss(b["f"], a["f"], R.penalty_loss(OPT, "G", a["x_before"]), a["x_before"].size, f"{name}: f_G of the separate pass")


# ------------------------------------------------------------------------------ one iteration against the oracle
ORACLE_CONFIGS = {
    "sgd_adagrad": (CONFIGS["sgd_adagrad"], dict(D_optmethod="sgd", D_sgd_momentum=0.9, G_optmethod="adagrad")),
    "D_L1_G_L2": (dict(D_L1=3e-5, D_L2=1e-4, G_L1=0.0, G_L2=2e-4), dict(D_L1=3e-5, D_L2=1e-4, G_L1=0.0, G_L2=2e-4)),
    "iterations": (CONFIGS["iterations"], dict(D_iterations=2, G_iterations=3)),
}


@pytest.mark.parametrize("name", list(ORACLE_CONFIGS))
def test_one_training_step_against_the_oracle(cg, name):
    """test_three_training_steps_at_16px's step-0 procedure and bounds, with lr the method's own learning rate.  The fused update (the
    path every front end runs) reports the criterion alone as f - the norms behind the penalty's share would synchronise - where the
    oracle, as adversarial.lua:203-204, adds G_L1 |p|_1 + G_L2 |p|_2^2 / 2: that share is added here in fp64 from G's parameters in front
    of its update (0.095 of 0.79 at G_L2 = 2e-4) before the two are compared within the same 5e-3."""
    cfg, ocfg = ORACLE_CONFIGS[name]
    OPT = opt_of(cfg)
    cg.manual_seed(SEED); rng = O.RNG(SEED)
    G, D = cg.models.create_G((3, 16, 16), 100), cg.models.create_D((3, 16, 16))
    Go, Do = S16.oracle_G16up(3, 100, rng), O.create_D32_st3(3, 16, rng)
    S = cg.adversarial.State(dict(batchSize=N, fused_update=True, **cfg), G, D)
    S.keep_outputs = True
    T = O.Trainer(Go, Do, **ocfg)
    np.testing.assert_array_equal(S.PARAMETERS_D.numpy(), T.pD)
    np.testing.assert_array_equal(S.PARAMETERS_G.numpy(), T.pG)
    pool, its = draws()
    data = cg.adversarial.TrainData(pool)
    idx, nd, ng = its[0]
    assert OPT["G_iterations"] == 1 or (OPT["G_L1"] == 0 and OPT["G_L2"] == 0)       # else the last G iteration's parameters were needed
    f_pen = R.penalty_loss(OPT, "G", S.PARAMETERS_G.numpy())
    cg.adversarial.iteration(S, data, N, real_idx=idx, noise_D=nd, noise_G=ng)
    r = T.step(pool[idx], nd, ng)
    step = 0
    close(S._last_fake.numpy(), r["fake"], tol=2e-4, what=f"{name}: fake images")
    close(cg.nn.as_plain(S._last["outputs_D"]).numpy(), r["outD"], tol=5e-4, what=f"{name}: D outputs (of the last D iteration)")
    print(f"{name}: f_G {float(S._last['f_G'])!r} + the penalty's {f_pen!r} against the oracle's {r['fG']!r}")
    assert abs(float(S._last["f_G"]) + f_pen - r["fG"]) < 5e-3
    for which, a, b in (("D", S.PARAMETERS_D.numpy(), T.pD), ("G", S.PARAMETERS_G.numpy(), T.pG)):
        lr = R.fused_args(OPT, which, OPT[which + "_optmethod"])[3]
        d = np.abs(a - b)
        print(f"[drift] {name} p{which}: lr {lr:g} max {d.max():.2e} mean {d.mean():.2e} frac>1e-4 {np.mean(d > 1e-4):.2e}")
        assert d.max() <= 2.5 * lr * (step + 1), f"p{which}: max drift {d.max():.2e}"
        assert d.mean() <= 4e-5 * (step + 1), f"p{which}: mean drift {d.mean():.2e}"
        assert np.mean(d > 1e-4) < 5e-2 * (step + 1), f"p{which}: {np.mean(d > 1e-4):.2e} outliers"
