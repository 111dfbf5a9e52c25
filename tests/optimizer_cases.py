"""Cases shared by tests/test_optimizers_cpu.py and tests/test_optimizers_gpu.py: sizes, scalar sets, inputs and
special-value rows for the SGD, Adam and Adadelta updates, the Adam and Adadelta rules written once more in float64, and the error bound of
the float32 statement (keras/optimizers.py) against that float64 evaluation.  No GPU is imported here.

The float64 evaluations below do not call the statement: they are the Keras 2.2.4 rules typed again, on the scalars the
statement uses (the float32 values of beta_1, beta_2, rho, epsilon, lr; 1 - beta subtracted in float32, 1 - rho in float64).

Error bound (`*_f64` return it next to every value).  u = 2^-24 is the unit round-off of one float32 operation.  Every value
is followed by a first-order bound of its float32 evaluation's error, propagated operation by operation; where signed terms
are added the rounding is charged on the sum of the ABSOLUTE terms (gabs, mabs below), where all terms are non-negative on
the value itself:

    g'   two products and a sum, plus the error p brings:        dg = 2u*gabs + 2*l2*dp,   gabs = |g*gs| + |2*l2*p|
    m    carried error, g', two products and a sum:              dm = b1*dm + omb1*dg + 3u*mabs,   mabs = b1*mabs + omb1*gabs
    v    square (2|g'|dg + u g'^2), two products and a sum:      dv = b2*dv + omb2*(2|g'|dg + u*g'^2) + 3u*v
    D = sqrt(d) + eps:  dD = dd/(2 sqrt(d)) + u*sqrt(d) + u*D     (d = v, or vhat with dvhat = max of the two bounds)
    q = lr_t*m/D:       dq = lr_t*dm/D + |q|*dD/D + 2u*|q|
    p = p - q:          dp = dp + dq + u*(|p| + |q|)

and likewise for Adadelta (a like v; u_ = g' sqrt(d+eps) / sqrt(a+eps) with five roundings and the three operand errors;
d like v from u_).  The asserted bound is SAFETY = 2 times the first-order bound, for the second-order terms it drops; it is
not fitted to what the code gives."""
import math

import numpy as np

U = 2.0 ** -24
SAFETY = 2.0
SIZES = [1, 3, 4, 5, 63, 257, 1021]
STEPS = 3


def several_passes(groups_per_pass):
    """Smallest interesting n for which threads of the capped grid take a second group: the cap is the launcher's."""
    return 4 * int(groups_per_pass) + 4 * 1000 + 3


# lr per step: Adam takes lr_t (Adam.step_size()), Adadelta and SGD the decayed lr.  "dyadic": every scalar exact in float32.
SCALAR_SETS = {
    "dyadic": dict(adam=dict(lr_t=[2.0 ** -6] * STEPS, beta_1=0.5, beta_2=0.5, epsilon=2.0 ** -8),
                   adadelta=dict(lr=[0.5] * STEPS, rho=0.5, epsilon=2.0 ** -10),
                   sgd=dict(lr_t=[0.25] * STEPS, momentum=(0.0, 0.5)),
                   l2=(0.0, 2.0 ** -4), grad_scale=(1.0, 0.125)),
    "normal": dict(adam=dict(lr_t=[0.001 / (1 + 1e-4 * i) * math.sqrt(1 - 0.999 ** (i + 1)) / (1 - 0.9 ** (i + 1))
                                   for i in range(STEPS)], beta_1=0.9, beta_2=0.999, epsilon=1e-7),
                   adadelta=dict(lr=[1.0 / (1 + 1e-4 * i) for i in range(STEPS)], rho=0.95, epsilon=1e-7),
                   sgd=dict(lr_t=[0.1 / (1 + 1e-4 * i) for i in range(STEPS)], momentum=(0.0, 0.9)),
                   l2=(0.0, 5e-4), grad_scale=(1.0, 0.125)),
}

# SGD beyond the small sizes: (nesterov, index of momentum, of l2, of grad_scale); every value of every parameter occurs with
# both values of nesterov
SGD_FEW = [(0, 1, 1, 1), (0, 0, 0, 0), (0, 0, 1, 0), (1, 1, 0, 1), (1, 0, 1, 0), (1, 0, 0, 1)]


def inputs(n, kind, seed=5):
    """-> p (n,), g (STEPS, n), float32.  dyadic: multiples of 1/8 in [-4, 4]; normal: p ~ N(0, 1), g ~ N(0, 0.1)."""
    rng = np.random.default_rng(seed + 1000003 * (kind == "normal"))
    if kind == "dyadic":
        return (rng.integers(-32, 33, n) / 8.0).astype(np.float32), (rng.integers(-32, 33, (STEPS, n)) / 8.0).astype(np.float32)
    return rng.standard_normal(n).astype(np.float32), (0.1 * rng.standard_normal((STEPS, n))).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------
# one step in which EVERY operation is exact in float32 (so float32 and float64 evaluations must agree element for element)
# ----------------------------------------------------------------------------------------------------------------------
def exact_adam_case(n=257, seed=9):
    """g' = g/8 + p/8 is a multiple of 1/8 with |g'| <= 1.5; b1 = b2 = 1/2; v0 = 2 s^2 - g'^2 with s = 4 - eps, so that the new
    v is s^2, sqrt(v) + eps = 4 and the quotient divides by a power of two; m0 a multiple of 1/8."""
    rng = np.random.default_rng(seed)
    eps = 2.0 ** -8
    p = rng.integers(-4, 5, n).astype(np.float64)
    g = rng.integers(-8, 9, n).astype(np.float64)
    ge = g * 0.125 + 0.125 * p
    s = 4.0 - eps
    v0 = 2.0 * s * s - ge * ge
    m0 = rng.integers(-16, 17, n) / 8.0
    arrays = dict(p=p, g=g, m=m0, v=v0, vhat=np.full(n, s * s - 1.0))     # vhat below the new v: amsgrad takes v
    assert all(np.array_equal(a.astype(np.float32).astype(np.float64), a) for a in arrays.values())
    return ({k: a.astype(np.float32) for k, a in arrays.items()},
            dict(lr_t=2.0 ** -6, beta_1=0.5, beta_2=0.5, epsilon=eps, l2=2.0 ** -4, grad_scale=0.125))


def exact_adadelta_case(n=257, seed=10):
    """rho = 1/2; d0 + eps = 2^-4 (square root 1/4); a0 = 2 (16 - eps) - g'^2 so that the new a + eps is 16 (square root 4)."""
    rng = np.random.default_rng(seed)
    eps = 2.0 ** -10
    p = rng.integers(-4, 5, n).astype(np.float64)
    g = rng.integers(-8, 9, n).astype(np.float64)
    ge = g * 0.125 + 0.125 * p
    a0 = 2.0 * (16.0 - eps) - ge * ge
    d0 = np.full(n, 2.0 ** -4 - eps)
    arrays = dict(p=p, g=g, a=a0, d=d0)
    assert all(np.array_equal(x.astype(np.float32).astype(np.float64), x) for x in arrays.values())
    return ({k: x.astype(np.float32) for k, x in arrays.items()},
            dict(lr=0.5, rho=0.5, epsilon=eps, l2=2.0 ** -4, grad_scale=0.125))


# ----------------------------------------------------------------------------------------------------------------------
# special values: one row per element, l2 = 0, grad_scale = 1, the default scalars
# ----------------------------------------------------------------------------------------------------------------------
_INF, _NAN = np.inf, np.nan
#                  p     g        second-moment state (Adam v and vhat; Adadelta accumulator)
SPECIAL_ROWS = [(1.5, 0.0, 0.0),          # g = 0 on zero state: p unchanged
                (1.5, _INF, 0.0), (1.5, -_INF, 0.0), (1.5, _NAN, 0.0),
                (_INF, 0.25, 0.0),        # p = Inf with l2 = 0: 0 * Inf in the effective gradient
                (0.5, 1e-20, 0.0), (0.5, -1e-20, 0.0),      # g^2 is a float32 denormal
                (0.5, 0.25, 2.0 ** 60), (0.5, -0.25, 1e30),  # a large second moment: sqrt swallows epsilon
                (-0.0, 0.0, 0.0), (0.0, -0.0, 0.0)]


def special_inputs():
    rows = np.array(SPECIAL_ROWS, dtype=np.float64)
    return tuple(rows[:, i].astype(np.float32) for i in range(3))


# ----------------------------------------------------------------------------------------------------------------------
# the rules in float64, with the first-order error bound of their float32 evaluation (module docstring)
# ----------------------------------------------------------------------------------------------------------------------
def _head(p, dp, g, l2, gs):
    two_l2 = float(np.float32(2.0) * np.float32(l2))
    gs = float(np.float32(gs))
    ge = g * gs + two_l2 * p
    gabs = np.abs(g * gs) + np.abs(two_l2 * p)
    return ge, gabs, 2 * U * gabs + two_l2 * dp


def adam_f64(state, g, lr_t, beta_1, beta_2, epsilon, l2, grad_scale, amsgrad):
    """state: dict p, m, v, vhat (float64) and their bounds dp, dm, dv, dvhat and mabs; updated in place, one step."""
    b1, b2 = float(np.float32(beta_1)), float(np.float32(beta_2))
    omb1, omb2 = float(np.float32(1) - np.float32(beta_1)), float(np.float32(1) - np.float32(beta_2))
    eps, lr_t = float(np.float32(epsilon)), float(np.float32(lr_t))
    s = state
    ge, gabs, dg = _head(s["p"], s["dp"], np.asarray(g, np.float64), l2, grad_scale)
    s["mabs"] = b1 * s["mabs"] + omb1 * gabs
    s["dm"] = b1 * s["dm"] + omb1 * dg + 3 * U * s["mabs"]
    s["m"] = b1 * s["m"] + omb1 * ge
    s["v"] = b2 * s["v"] + omb2 * (ge * ge)
    s["dv"] = b2 * s["dv"] + omb2 * (2 * np.abs(ge) * dg + U * ge * ge) + 3 * U * s["v"]
    d, dd = s["v"], s["dv"]
    if amsgrad:
        s["vhat"] = np.maximum(s["vhat"], s["v"])
        s["dvhat"] = np.maximum(s["dvhat"], s["dv"])
        d, dd = s["vhat"], s["dvhat"]
    root = np.sqrt(d)
    D = root + eps
    dD = dd / (2 * np.where(root > 0, root, 1.0)) + U * root + U * D      # d = 0 only from zero gradients: dd is 0 there
    assert not np.any((root == 0) & (dd > 0))
    q = lr_t * s["m"] / D
    dq = lr_t * s["dm"] / D + np.abs(q) * dD / D + 2 * U * np.abs(q)
    s["dp"] = s["dp"] + dq + U * (np.abs(s["p"]) + np.abs(q))
    s["p"] = s["p"] - q
    return s


def adam_state(p):
    z = lambda: np.zeros(len(p), np.float64)
    return dict(p=np.asarray(p, np.float64), m=z(), v=z(), vhat=z(), dp=z(), dm=z(), dv=z(), dvhat=z(), mabs=z())


def adadelta_f64(state, g, lr, rho, epsilon, l2, grad_scale):
    """state: dict p, a, d (float64) and their bounds dp, da, dd; updated in place, one step."""
    omr, rho = float(np.float32(1.0 - float(rho))), float(np.float32(rho))
    eps, lr = float(np.float32(epsilon)), float(np.float32(lr))
    s = state
    ge, gabs, dg = _head(s["p"], s["dp"], np.asarray(g, np.float64), l2, grad_scale)
    s["a"] = rho * s["a"] + omr * (ge * ge)
    s["da"] = rho * s["da"] + omr * (2 * np.abs(ge) * dg + U * ge * ge) + 3 * U * s["a"]
    num, den = np.sqrt(s["d"] + eps), np.sqrt(s["a"] + eps)
    u = ge * num / den
    du = dg * num / den + np.abs(u) * (s["dd"] / (2 * (s["d"] + eps)) + s["da"] / (2 * (s["a"] + eps)) + 5 * U)
    s["dp"] = s["dp"] + lr * du + U * (np.abs(s["p"]) + 2 * np.abs(lr * u))
    s["p"] = s["p"] - lr * u
    s["d"] = rho * s["d"] + omr * (u * u)
    s["dd"] = rho * s["dd"] + omr * (2 * np.abs(u) * du + U * u * u) + 3 * U * s["d"]
    return s


def adadelta_state(p):
    z = lambda: np.zeros(len(p), np.float64)
    return dict(p=np.asarray(p, np.float64), a=z(), d=z(), dp=z(), da=z(), dd=z())


# ----------------------------------------------------------------------------------------------------------------------
# launch geometry of csrc/dj_optim.hip, for the bound of the sum of squares
# ----------------------------------------------------------------------------------------------------------------------
THREADS = 256


def terms_per_thread(n, groups_per_pass):
    """Most float32 terms one thread adds to its partial sum: four per group, one group per pass of the capped grid."""
    groups = (n + 3) // 4
    blocks = min(max(-(-groups // THREADS), 1), groups_per_pass // THREADS)
    return 4 * -(-groups // (blocks * THREADS))


def sumsq_bound(n, groups_per_pass):
    """Relative bound of start + sum(p^2) as the kernel adds it: the products' rounding, k - 1 float32 additions per thread,
    6 shuffle levels, the rounding of the float64 total and the final float32 addition; all terms non-negative."""
    return (terms_per_thread(n, groups_per_pass) + 8) * U
