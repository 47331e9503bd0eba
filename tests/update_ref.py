"""What happens to a gradient between backward and the next forward, restated in fp64 numpy from the kernels' text (csrc/optim.hip
pen_clamp / adam_elem / sgd_k / adagrad_k / ema_elem, csrc/ops.hip axpy_sign_k / axpy_k / clamp_k) and from optim.py, with the
magnitude sums the per-element bounds of helpers.rounding_close need.  A plain module, imported as tests/sampler_ref.py is.

Every scalar the C ABI takes as a float (l1, l2, clamp, lr, the betas, eps, momentum, dampening, the decay) enters here as the fp32
value the kernel receives, held in a double; every vector is the fp32 input held in doubles.  1 - b and 1 - dampening are formed
from those fp32 values, as the kernels form them.  Nothing below is rounded to fp32 except Adam's step size, which the host entry
points hand to the kernel as a float.

fused_args() restates, from adversarial.lua:92-112, 201-212, 240-265 and train.lua:191-207 and not from adversarial.py, which scalars
the update of net D or G receives for an OPT table."""
import numpy as np

f32, f64 = np.float32, np.float64

# roundings on the longest chain of each kernel expression, + 2 (helpers.rounding_close's r), with the line they are counted from
R_PEN = 3 + 2       # pen_clamp / adam_elem `gi += sg * l1 + pi * l2`: the product pi * l2, the inner sum, the sum into gi (sg * l1 is exact)
R_ADAM_M = 4 + 2    # adam_elem `mi = b1 * mi + (1.f - b1) * gi`: 1 - b1, two products, the sum
R_ADAM_V = 5 + 2    # adam_elem `vi = b2 * vi + (1.f - b2) * gi * gi`: 1 - b2, three products, the sum
R_ADAM_P = 12 + 2   # adam_elem `pi = pi - step * mi / (sqrtf(vi) + eps)`: m 4, v 5 halved by the root 3, root, + eps, product, quotient, difference
R_SGD_V = 4 + 2     # sgd_k `d = mom * v[i] + (1.f - damp) * gi`: 1 - damp, two products, the sum
R_SGD_P = 6 + 2     # sgd_k `p[i] = pi - lr * d` behind d
R_SGD_P0 = 2 + 2    # the same line with d = gi (momentum 0)
R_ADAGRAD_VAR = 2 + 2   # adagrad_k `vi = var[i] + gi * gi`
R_ADAGRAD_P = 6 + 2     # adagrad_k `p[i] = pi - lr * gi / (sqrtf(vi) + 1e-10f)`: var 2 halved by the root 1, root, + 1e-10, product, quotient, difference
R_EMA = 3 + 2       # ema_elem `fmaf(d, e, __fmul_rn(omd, p))`: 1 - d, the product, the fma
R_SEP = 3 + 2       # cg_axpy_sign, cg_axpy, cg_clamp in sequence: the sum of axpy_sign_k, the fma of axpy_k, + 1 where it is not contracted


def c32(x):
    """The double that holds the float the C ABI receives for x."""
    return float(f32(x))


def d64(a):
    return np.asarray(a, f32).astype(f64)


def sign(p):
    """`pi > 0.f ? 1.f : (pi < 0.f ? -1.f : 0.f)`: an exact comparison on the input, 0 for +-0.0 (and for a NaN)."""
    p = np.asarray(p)
    return np.where(p > 0, 1.0, np.where(p < 0, -1.0, 0.0))


def penalise(p, g, l1, l2, clamp):
    """pen_clamp / adam_elem's prologue: g + sign(p) l1 + p l2 where either weight is set, THEN the clamp where clamp > 0.
    -> the fp64 gradient, terms = |g| + l1 [p != 0] + l2 |p| (the clamp is 1-Lipschitz: it adds no term)."""
    p, g = d64(p), d64(g)
    l1, l2, clamp = c32(l1), c32(l2), c32(clamp)
    terms = np.abs(g)
    if l1 != 0 or l2 != 0:
        g = g + (sign(p) * l1 + p * l2)
        terms = terms + np.abs(l1) * (p != 0) + np.abs(l2) * np.abs(p)
    if clamp > 0:
        g = np.clip(g, -clamp, clamp)
    return g, terms


def adam_step_size(lr, b1, b2, t):
    """adam_step_host / adam_step_dev: (float)(lr sqrt(1 - b2^t) / (1 - b1^t)) in doubles from the fp32 lr and betas."""
    lr, b1, b2 = c32(lr), c32(b1), c32(b2)
    return c32(lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))


def adam(p, g, m, v, lr, b1, b2, eps, t):
    """adam_elem behind its prologue -> (p', m', v'), terms (p, m, v) as test_optimiser_kernels_past_the_wrap forms them."""
    p, g, m, v = d64(p), d64(g), d64(m), d64(v)
    b1, b2, eps = c32(b1), c32(b2), c32(eps)
    step = adam_step_size(lr, b1, b2, t)
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    p1 = p - step * m1 / (np.sqrt(v1) + eps)
    tm = b1 * np.abs(m) + (1.0 - b1) * np.abs(g)
    tv = b2 * np.abs(v) + (1.0 - b2) * g * g
    tp = np.abs(p) + step * tm / (np.sqrt(tv) + eps)
    return (p1, m1, v1), (tp, tm, tv)


def sgd(p, g, v, lr, mom, damp):
    """sgd_k behind pen_clamp -> (p', v' or None), terms (p, v or None).  v is ignored (may be None) where mom == 0."""
    p, g = d64(p), d64(g)
    lr, mom, damp = c32(lr), c32(mom), c32(damp)
    if mom != 0:
        v = d64(v)
        d = mom * v + (1.0 - damp) * g
        td = np.abs(mom) * np.abs(v) + np.abs(1.0 - damp) * np.abs(g)
        return (p - lr * d, d), (np.abs(p) + lr * td, td)
    return (p - lr * g, None), (np.abs(p) + lr * np.abs(g), None)


def adagrad(p, g, var, lr):
    """adagrad_k behind pen_clamp -> (p', var'), terms (p, var)."""
    p, g, var = d64(p), d64(g), d64(var)
    lr = c32(lr)
    var1 = var + g * g
    tvar = np.abs(var) + g * g
    den = np.sqrt(var1) + c32(1e-10)
    return (p - lr * g / den, var1), (np.abs(p) + lr * np.abs(g) / (np.sqrt(tvar) + c32(1e-10)), tvar)


def ema(e, p, d):
    """ema_elem: d e + (1 - d) p for the fp32 decay d -> e', terms."""
    e, p, d = d64(e), d64(p), c32(d)
    return d * e + (1.0 - d) * p, d * np.abs(e) + (1.0 - d) * np.abs(p)


def ema_decay(D, n):
    """optim.ema_decay / ema_decay_dev: the decay of the n-th applied update (n from 1)."""
    return c32(min(c32(D), (1.0 + n) / (10.0 + n)))


# ------------------------------------------------------------------------------ the separate passes, in fp32
def axpy_sign32(al, x, y):
    """axpy_sign_k `y[i] += al * sign`: a product with +-1 or 0 (exact) and one fp32 sum - contracted or not, the same bits."""
    return (np.asarray(y, f32) + f32(al) * sign(x).astype(f32)).astype(f32)


def clamp32(x, lo, hi):
    """clamp_k `fminf(fmaxf(x, lo), hi)`."""
    return np.minimum(np.maximum(np.asarray(x, f32), f32(lo)), f32(hi))


# ------------------------------------------------------------------------------ OPT -> kernel arguments
ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)           # optim.adam's defaults: train.lua:197-200 leaves OPTSTATE.adam.{D,G} empty
DEFAULTS = dict(G_L1=0.0, G_L2=0.0, D_L1=0.0, D_L2=1e-4, D_clamp=1.0, G_clamp=5.0, D_optmethod="adam", G_optmethod="adam",
                D_iterations=1, G_iterations=1, D_sgd_lr=0.02, G_sgd_lr=0.02, D_sgd_momentum=0.0, G_sgd_momentum=0.0)   # train.lua:26-45


def fused_args(OPT, which, method):
    """(l1, l2, clamp, lr, momentum, dampening) of net `which`'s update under `method`.
    D (adversarial.lua:92-98, 110-112): sign(p) D_L1 + p D_L2, clamp D_clamp (0 = none).
    G (:201-212): where G_L1 or G_L2 is set, sign(p) G_L2 + p G_L2 - the sign term carries G_L2, line 206 - clamp G_clamp.
    Learning rates (train.lua:191-207): adagrad 1e-3 for D and 3e-3 for G, adam optim's default 1e-3, sgd X_sgd_lr with X_sgd_momentum;
    optim.sgd's dampening defaults to the momentum (its first step with momentum copies the gradient: a state, not an argument)."""
    o = dict(DEFAULTS)
    o.update(OPT)
    if which == "D":
        l1, l2, clamp = o["D_L1"], o["D_L2"], o["D_clamp"]
    else:
        l1 = l2 = o["G_L2"] if (o["G_L1"] != 0 or o["G_L2"] != 0) else 0.0
        clamp = o["G_clamp"]
    if method == "adam":
        lr, mom = ADAM["lr"], 0.0
    elif method == "adagrad":
        lr, mom = (1e-3 if which == "D" else 3e-3), 0.0
    else:
        assert method == "sgd", method
        lr, mom = o[which + "_sgd_lr"], o[which + "_sgd_momentum"]
    return l1, l2, clamp, lr, mom, mom


def penalty_loss(OPT, which, p):
    """What feval adds to the reported loss (adversarial.lua:94-95, 203-204): X_L1 |p|_1 + X_L2 |p|_2^2 / 2 where either is set."""
    o = dict(DEFAULTS)
    o.update(OPT)
    a, b = o[which + "_L1"], o[which + "_L2"]
    if a == 0 and b == 0:
        return 0.0
    p = d64(p)
    return a * float(np.abs(p).sum()) + b * float((p * p).sum()) / 2
