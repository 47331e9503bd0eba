"""The update path's kernels through the C ABI at their non-default arguments, against the fp64 twin tests/update_ref.py: the penalty and
clamp prologue of the six optimiser entry points (csrc/optim.hip adam_elem, pen_clamp), write_back_grad = 0, clamp = 0, sgd away from
dampening == momentum, the separate passes the unfused update is made of (csrc/ops.hip axpy_sign_k, axpy_k, clamp_k, scale_k), the
norms behind the reported loss (sumred_k) and non-finite gradients.

Two measures only (helpers.py): bits_equal, and rounding_close with r counted in update_ref.py beside the kernel line it comes from.
The fused steps are checked in two stages, as batch norm is from the device's statistics: the written-back gradient against
penalise(), then parameters and state against the twin evaluated FROM that written-back gradient, so that an ulp in g next to
sqrt(v) ~ 0 needs no bound.  Nothing is excluded: the clamp is continuous and the sign an exact comparison on the input.

Every length states the regime it is meant to hit; test_update_ref_host.py asserts the table without a GPU."""
import importlib

import numpy as np
import pytest
import torch

import update_ref as R
from helpers import bits_equal, dev, edge_normal, host, rounding_close

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
OPT_N = 262144 + 3                            # past cg::ew_grid's cap of 262 144 lanes: the scalar kernels' stride wraps
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
A, B, C = 0.03, 0.25, 0.5                     # l1, l2, clamp: large enough to move every element of N(., 1) data by many ulps
PEN = [(0.0, 0.0, 0.0), (A, 0.0, 0.0), (0.0, B, 0.0), (0.0, 0.0, C), (A, B, C), (A, B, 0.0)]
EMA_D, EMA_COUNT = 0.999, 3                   # d_3 = 4 / 13: 1 - d rounds
ENTRIES = ("adam", "adam_dev", "adam_ema", "adam_ema_dev", "sgd", "adagrad")

# n, misaligned, (the scalar kernels' regime, adam_ema_k / ema_k: (float4 body?, live tail), axpy_k: float4?)
CASES = [
    (1, False, ("one", (True, 1), False)), (3, False, ("one", (True, 3), False)), (255, False, ("one", (True, 3), False)),
    (256, False, ("one", (True, 0), True)), (257, False, ("many", (True, 1), False)), (1027, False, ("many", (True, 3), False)),
    (1028, False, ("many", (True, 0), True)), (1028, True, ("many", (False, 0), False)),      # the same multiple of 4 through a pointer 4 bytes off
    (OPT_N, False, ("wrap", (True, 3), False)),
]


def ew_regime(n, cap):
    return "wrap" if n > cap * 256 else ("many" if n > 256 else "one")


def regime(n, misaligned, cap):
    """cg_*_step (CG_EW_LAUNCH over n), cg_adam_step_ema / cg_ema_update (vec_ok(0, ...): alignment alone, the n % 4 floats behind the
    float4 body one per thread), cg_axpy (vec_ok(n, ...))."""
    return ew_regime(n, cap), ((True, n % 4) if not misaligned else (False, 0)), (n % 4 == 0 and not misaligned)


@pytest.fixture(scope="module")
def cg():
    mod = importlib.import_module("cat-generator_amd")
    assert torch.cuda.is_available(), "these tests need the MI355X"
    mod.lib()
    return mod


def ew_cap(L):
    return int(L.prelu_backward_workspace_bytes(1 << 40)) // 8


def ptr(t):
    return t.data_ptr()


_INPUTS = {}


def inputs(n):
    """p, g, m, v, e for a length, made once and never changed.  p: edge_normal with +-0.0 and +-1e-30 planted.  g: normal data with,
    at random places, +-C exactly, one ulp beyond and one inside, elements that only the penalty carries across the clamp
    (g = s C - pen / 2 with pen = sign(p) A + p B and s its sign: penalty-then-clamp gives s C, clamp-then-penalty s C + pen / 2) and
    elements where g = -B p, so that the l2 sum cancels.  A few v are zero (a state that has seen no gradient)."""
    if n in _INPUTS:
        return _INPUTS[n]
    rng = np.random.default_rng(1000 + n)
    p, e = edge_normal(rng, (n, 1)).ravel(), edge_normal(rng, (n, 1)).ravel()
    g = edge_normal(rng, (n, 1), plant=False).ravel()
    m, v = (rng.standard_normal(n) * 0.1).astype(f32), (rng.random(n) * 0.1).astype(f32)
    c = f32(C)
    pos = rng.permutation(n)
    pen = (R.sign(p) * R.c32(A) + p.astype(f64) * R.c32(B))
    s = np.where(pen >= 0, 1.0, -1.0)
    reps = max(1, min(16, n // 16))
    plants = [lambda i: c, lambda i: -c, lambda i: np.nextafter(c, f32(np.inf)), lambda i: np.nextafter(-c, f32(-np.inf)),
              lambda i: np.nextafter(c, f32(0)), lambda i: np.nextafter(-c, f32(0)),
              lambda i: f32(s[i] * C - 0.5 * pen[i]), lambda i: f32(-R.c32(B) * p[i]), lambda i: f32(-pen[i])]
    for k, i in enumerate(pos[:reps * len(plants)]):
        g[i] = plants[k % len(plants)](i)
    v[pos[::7][:reps]] = 0.0
    _INPUTS[n] = dict(p=p, g=g, m=m, v=v, e=e)
    return _INPUTS[n]


def run(L, st, entry, a, n, pen, wb, t=2, mis=False, sgd=(0.02, 0.9, 0.9), null_v=False, g=None):
    """One launch of an optimiser entry point on guarded copies of the inputs -> {name: host array} of everything it may write."""
    l1, l2, clamp = pen
    names = {"adam": "pgmv", "adam_dev": "pgmv", "adam_ema": "pgmve", "adam_ema_dev": "pgmve", "sgd": "pgm", "adagrad": "pgv"}[entry]
    bufs = {k: dev(a[k] if k != "g" or g is None else g, mis) for k in names}
    P = {k: ptr(b) for k, b in bufs.items()}
    td = torch.tensor([t], dtype=torch.int64, device="cuda")
    nd = torch.tensor([EMA_COUNT], dtype=torch.int64, device="cuda")
    if entry == "adam":
        L.adam_step(st, P["p"], P["g"], P["m"], P["v"], n, LR, B1, B2, EPS, t, l1, l2, clamp, wb)
    elif entry == "adam_dev":
        L.adam_step_dev(st, P["p"], P["g"], P["m"], P["v"], n, LR, B1, B2, EPS, ptr(td), l1, l2, clamp, wb)
    elif entry == "adam_ema":
        L.adam_step_ema(st, P["p"], P["g"], P["m"], P["v"], P["e"], n, LR, B1, B2, EPS, t, l1, l2, clamp, wb, R.ema_decay(EMA_D, EMA_COUNT))
    elif entry == "adam_ema_dev":
        L.adam_step_ema_dev(st, P["p"], P["g"], P["m"], P["v"], P["e"], n, LR, B1, B2, EPS, ptr(td), l1, l2, clamp, wb, R.c32(EMA_D), ptr(nd))
    elif entry == "sgd":
        L.sgd_step(st, P["p"], P["g"], None if null_v else P["m"], n, sgd[0], sgd[1], sgd[2], l1, l2, clamp, wb)
    else:
        L.adagrad_step(st, P["p"], P["g"], P["v"], n, LR, l1, l2, clamp, wb)
    assert int(td.item()) == t and int(nd.item()) == EMA_COUNT, "the kernels read the counters, the host advances them"
    return {k: host(b) for k, b in bufs.items()}


def check_stage_two(entry, a, out, what, t=2, sgd=(0.02, 0.9, 0.9), vel=None):
    """p and the state against the twin evaluated from the device's written-back g (out["g"]): R_* as counted in update_ref.py."""
    gd = out["g"]
    if entry.startswith("adam"):
        (p1, m1, v1), (tp, tm, tv) = R.adam(a["p"], gd, a["m"], a["v"], LR, B1, B2, EPS, t)
        rounding_close(out["m"], m1, tm, R.R_ADAM_M, what + " m")
        rounding_close(out["v"], v1, tv, R.R_ADAM_V, what + " v")
        rounding_close(out["p"], p1, tp, R.R_ADAM_P, what + " p")
        if "e" in out:       # from the device's own p', as test_gpu_ema.py checks it
            e1, te = R.ema(a["e"], out["p"], R.ema_decay(EMA_D, EMA_COUNT))
            rounding_close(out["e"], e1, te, R.R_EMA, what + " e")
    elif entry == "sgd":
        v0 = a["m"] if vel is None else vel
        (p1, d1), (tp, td) = R.sgd(a["p"], gd, v0, *sgd)
        if sgd[1] != 0:
            rounding_close(out["m"], d1, td, R.R_SGD_V, what + " velocity")
            rounding_close(out["p"], p1, tp, R.R_SGD_P, what + " p")
        else:
            rounding_close(out["p"], p1, tp, R.R_SGD_P0, what + " p")
    else:
        (p1, var1), (tp, tvar) = R.adagrad(a["p"], gd, a["v"], LR)
        rounding_close(out["v"], var1, tvar, R.R_ADAGRAD_VAR, what + " var")
        rounding_close(out["p"], p1, tp, R.R_ADAGRAD_P, what + " p")


# ------------------------------------------------------------------------------ 1. the penalty / clamp matrix
@pytest.mark.parametrize("n,mis,want", CASES)
def test_penalty_clamp_matrix_of_every_optimiser_entry(cg, n, mis, want):
    L, st = cg.lib(), cg.tensor.stream()
    assert regime(n, mis, ew_cap(L)) == want
    a = inputs(n)
    for entry in ENTRIES:
        for pen in PEN:
            what = f"{entry}, n = {n}{' off alignment' if mis else ''}, (l1, l2, clamp) = {pen}"
            out = run(L, st, entry, a, n, pen, 1, mis=mis)
            gref, terms = R.penalise(a["p"], a["g"], *pen)
            rounding_close(out["g"], gref, terms, R.R_PEN, what + ": g written back")     # stage one
            if pen[2] > 0:
                assert np.abs(out["g"]).max() <= f32(pen[2]), what + ": the written-back g lies outside the clamp"
            if pen == (0.0, 0.0, 0.0):
                bits_equal(out["g"], a["g"], what + ": nothing to add, nothing to clamp")
            check_stage_two(entry, a, out, what)                                           # stage two
            out0 = run(L, st, entry, a, n, pen, 0, mis=mis)
            bits_equal(out0["g"], a["g"], what + ": write_back_grad = 0 leaves g alone")
            for k in out:
                if k != "g":
                    bits_equal(out0[k], out[k], what + f": {k} with write_back_grad = 0 against 1")


# ------------------------------------------------------------------------------ 2. adam_elem is written once
@pytest.mark.parametrize("n,mis", [(1027, False), (1028, False), (1028, True), (OPT_N, False)])
def test_the_four_adam_entry_points_agree_bit_for_bit_with_the_penalty_live(cg, n, mis):
    L, st = cg.lib(), cg.tensor.stream()
    a = inputs(n)
    for t in (1, 3):
        for pen in PEN[1:]:
            outs = [run(L, st, entry, a, n, pen, 1, t=t, mis=mis) for entry in ENTRIES[:4]]
            for entry, o in zip(ENTRIES[1:4], outs[1:]):
                for k in "pgmv":
                    bits_equal(o[k], outs[0][k], f"{entry} {k} against cg_adam_step, n = {n}, t = {t}, (l1, l2, clamp) = {pen}")
            bits_equal(outs[3]["e"], outs[2]["e"], f"cg_adam_step_ema_dev e against cg_adam_step_ema, n = {n}, t = {t}")


# ------------------------------------------------------------------------------ 3. sgd away from dampening == momentum
@pytest.mark.parametrize("n,mis,want", CASES)
def test_sgd_momentum_and_dampening(cg, n, mis, want):
    L, st = cg.lib(), cg.tensor.stream()
    a = inputs(n)
    pen = (A, B, C)
    # momentum 0: sgd_k never touches v, and the entry point takes a null pointer for it
    out = run(L, st, "sgd", a, n, pen, 1, mis=mis, sgd=(0.02, 0.0, 0.0), null_v=True)
    check_stage_two("sgd", a, out, f"sgd, momentum 0, null velocity, n = {n}", sgd=(0.02, 0.0, 0.0))
    bits_equal(out["m"], a["m"], "the velocity buffer that was not handed over")
    for damp in (0.9, 0.0, 0.3):
        out = run(L, st, "sgd", a, n, pen, 1, mis=mis, sgd=(0.02, 0.9, damp))
        check_stage_two("sgd", a, out, f"sgd, momentum 0.9, dampening {damp}, n = {n}", sgd=(0.02, 0.9, damp))
    # the first step as optim.sgd builds it: zero velocity, dampening 0 -> v = 0.9 * 0 + 1 * g = g exactly, p - lr g in two roundings
    zero = dict(a, m=np.zeros(n, f32))
    out = run(L, st, "sgd", zero, n, pen, 1, mis=mis, sgd=(0.02, 0.9, 0.0))
    bits_equal(out["m"], out["g"], f"first momentum step: v = g, n = {n}")
    (p1, _), (tp, _) = R.sgd(a["p"], out["g"], None, 0.02, 0.0, 0.0)
    rounding_close(out["p"], p1, tp, R.R_SGD_P0, f"first momentum step: p - lr g, n = {n}")


def test_rejected_arguments_launch_nothing(cg):
    L, st = cg.lib(), cg.tensor.stream()
    n = 1027
    a = inputs(n)
    b = {k: dev(a[k]) for k in "pgmve"}
    P = {k: ptr(x) for k, x in b.items()}
    td, nd = (torch.tensor([2], dtype=torch.int64, device="cuda") for _ in range(2))
    calls = [lambda: L.sgd_step(st, P["p"], P["g"], None, n, 0.02, 0.9, 0.9, A, B, C, 1),                       # momentum without a velocity
             lambda: L.adam_step(st, P["p"], P["g"], P["m"], P["v"], n, LR, B1, B2, EPS, 0, A, B, C, 1),           # t < 1
             lambda: L.adam_step_ema(st, P["p"], P["g"], P["m"], P["v"], P["e"], n, LR, B1, B2, EPS, 0, A, B, C, 1, 0.5)]
    for d in (0.0, 1.0, 1.5, -0.1, float("nan")):                                                                  # a decay outside (0, 1)
        calls += [lambda d=d: L.ema_update(st, P["e"], P["p"], n, d),
                  lambda d=d: L.ema_update_dev(st, P["e"], P["p"], n, d, ptr(nd)),
                  lambda d=d: L.adam_step_ema(st, P["p"], P["g"], P["m"], P["v"], P["e"], n, LR, B1, B2, EPS, 2, A, B, C, 1, d),
                  lambda d=d: L.adam_step_ema_dev(st, P["p"], P["g"], P["m"], P["v"], P["e"], n, LR, B1, B2, EPS, ptr(td), A, B, C, 1, d, ptr(nd))]
    for call in calls:
        with pytest.raises(cg.CatganError):
            call()
    for k in "pgmve":
        bits_equal(host(b[k]), a[k], f"a refused call launches nothing: {k}")


# ------------------------------------------------------------------------------ 4. the separate passes
@pytest.mark.parametrize("n,mis,want", CASES)
def test_separate_passes_against_the_twin_and_the_fused_prologue(cg, n, mis, want):
    L, st = cg.lib(), cg.tensor.stream()
    assert regime(n, mis, ew_cap(L)) == want
    a = inputs(n)
    p, g = a["p"], a["g"]
    pt, y = dev(p, mis), dev(g, mis)
    # axpy_sign_k `y[i] += al * (v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f))`: a product with +-1 or 0 and one sum - the bits of fp32 numpy
    L.axpy_sign(st, A, ptr(pt), ptr(y), n)
    y1 = host(y)
    bits_equal(y1, R.axpy_sign32(A, p, g), f"cg_axpy_sign, n = {n}")
    assert (y1[p == 0] == g[p == 0]).all(), "sign(+-0.0) is 0"
    # axpy_k `acc += w * g`: a product and a sum, or one fma: 2, + 2
    L.axpy(st, B, ptr(pt), ptr(y), n)
    y2 = host(y)
    bq = R.c32(B)
    rounding_close(y2, y1.astype(f64) + bq * p.astype(f64), np.abs(y1.astype(f64)) + bq * np.abs(p.astype(f64)), 2 + 2, f"cg_axpy, n = {n}")
    # clamp_k `fminf(fmaxf(x[i], lo), hi)`: no arithmetic
    L.clamp(st, ptr(y), -C, C, n)
    y3 = host(y)
    bits_equal(y3, R.clamp32(y2, -C, C), f"cg_clamp, n = {n}")
    bits_equal(host(pt), p, "the separate passes read p")
    # the three in sequence are penalise(): R_SEP
    gref, terms = R.penalise(p, g, A, B, C)
    rounding_close(y3, gref, terms, R.R_SEP, f"axpy_sign, axpy, clamp in sequence, n = {n}")
    # ... and the fused prologues' g lies within the sum of the two bounds of it
    for entry in ("adam", "sgd", "adagrad", "adam_ema"):
        out = run(L, st, entry, a, n, (A, B, C), 1, mis=mis)
        rounding_close(out["g"], y3.astype(f64), terms, R.R_PEN + R.R_SEP, f"{entry}'s fused g against the separate passes', n = {n}")
    # scale_k `x[i] *= al`: one product
    x = dev(g, mis)
    L.scale(st, ptr(x), 0.3, n)
    bits_equal(host(x), g * f32(0.3), f"cg_scale, n = {n}")


# ------------------------------------------------------------------------------ 5. the norms
def norm_inputs(n):
    """edge_normal data (+-0.0 and +-1e-30 planted) with, from n = 255 on, three elements each of 1e19 and -3e19: 9e38 is past fp32's
    largest value and 1e38 within 2^-24 of it is not what fp64 holds, so a square formed in fp32 fails either way."""
    rng = np.random.default_rng(2000 + n)
    x = edge_normal(rng, (n, 1)).ravel()
    if n >= 255:
        pos = rng.permutation(n)[:6]
        x[pos[:3]] = 1e19
        x[pos[3:]] = -3e19
    return x


@pytest.mark.parametrize("n,mis,want", CASES)
def test_norms_against_fp64_sums(cg, n, mis, want):
    """sumred_k adds doubles: each element enters exactly (|v|, or the double product v v of two fp32 values, which is exact), so the
    only error is that of at most n - 1 double additions in an order the atomics do not fix: n 2^-53 sum|terms|."""
    L, st = cg.lib(), cg.tensor.stream()
    assert regime(n, mis, ew_cap(L))[0] == want[0]
    x = norm_inputs(n)
    x64 = x.astype(f64)
    xt = dev(x, mis)
    s1, s2 = float(np.abs(x64).sum()), float((x64 * x64).sum())
    u53 = 2.0 ** -53
    acc = torch.full((1,), 123.0, dtype=torch.float64, device="cuda")      # the memset inside the call is part of the contract
    for call, ref, what in ((L.sumabs, s1, "cg_sumabs"), (L.sumsq, s2, "cg_sumsq")):
        for again in (False, True):                                        # the second result replaces the first
            call(st, ptr(xt), n, ptr(acc))
            got = float(acc.item())
            print(f"{what}, n = {n}: |d| / bound = {abs(got - ref) / max(n * u53 * ref, 1e-300):.3f}")
            assert np.isfinite(got) and abs(got - ref) <= n * u53 * ref, f"{what}, n = {n}{', called again' if again else ''}: {got!r} vs {ref!r}"
    bits_equal(host(xt), x, "the norms read x")
    if not mis:
        T = cg.Tensor.from_numpy(x)
        n1, n2 = T.norm(1), T.norm(2)
        assert abs(n1 - s1) <= n * u53 * s1, f"Tensor.norm(1), n = {n}"
        # sqrt halves the sum's relative error; its own rounding adds 2^-53
        assert np.isfinite(n2) and abs(n2 - np.sqrt(s2)) <= (0.5 * n + 1) * u53 * np.sqrt(s2), f"Tensor.norm(2), n = {n}: {n2!r} vs {np.sqrt(s2)!r}"


# ------------------------------------------------------------------------------ 6. non-finite gradients
@pytest.mark.parametrize("n", [3, 1027, 1028])
def test_nonfinite_gradients_meet_the_clamp(cg, n):
    """+-inf in g comes out as +-clamp on every path, whatever the penalty adds.  A NaN in g comes out as -clamp, from the fused
    prologues and from cg_clamp alike: fmaxf(NaN, -clamp) is -clamp (C's fmax returns the operand that is a number), and fminf(-clamp,
    clamp) keeps it.  So a NaN gradient element is not propagated into the parameters; it pushes them as a gradient of -clamp does."""
    L, st = cg.lib(), cg.tensor.stream()
    a = inputs(n)
    g = a["g"].copy()
    g[0], g[1], g[2] = np.inf, -np.inf, np.nan
    c = f32(C)
    want = np.array([c, -c, -c], f32)
    for pen in ((0.0, 0.0, C), (A, B, C)):
        y, pt = dev(g), dev(a["p"])
        if pen[0]:
            L.axpy_sign(st, A, ptr(pt), ptr(y), n)
            L.axpy(st, B, ptr(pt), ptr(y), n)
        L.clamp(st, ptr(y), -C, C, n)
        sep = host(y)
        bits_equal(sep[:3], want, f"cg_clamp on +inf, -inf, NaN, (l1, l2, clamp) = {pen}")
        for entry in ENTRIES:
            out = run(L, st, entry, a, n, pen, 1, g=g)
            bits_equal(out["g"][:3], want, f"{entry} on +inf, -inf, NaN, (l1, l2, clamp) = {pen}")
            for k in out:
                assert np.isfinite(out[k]).all(), f"{entry}: {k} is not finite behind the clamp"
            check_stage_two(entry, a, out, f"{entry} behind a non-finite g, n = {n}")
