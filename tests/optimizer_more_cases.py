"""Cases shared by tests/test_optimizers_more_cpu.py and tests/test_optimizers_more_gpu.py: the RMSprop, Adagrad, Adamax and
Nadam updates.  Sizes, scalar sets, inputs and special-value rows, the four rules written once more in float64, and the
error bound of the float32 statement (keras/optimizers.py) against that float64 evaluation.  No GPU is imported here.

Every rule is described by one entry of RULES: the C entry point, the statement's name, and the state buffers in the order
both take them.  Both are called as (p, g, *state, [n,] *scalars, l2, grad_scale[, sumsq]), with the same scalars in the
same order, so one driver serves the four.

The float64 evaluations do not call the statement: they are the Keras 2.2.4 rules typed again, on the scalars the statement
uses (the float32 values of lr, rho, the betas, epsilon and the Nadam schedule scalars; 1 - rho and 1 - beta subtracted in
float32).  The Nadam schedule (`nadam_schedule`) is typed again too, as a plain loop over the steps.

Error bound (`*_f64` keep it next to every value).  u = 2^-24 is the unit round-off of one float32 operation.  Every value is
followed by a first-order bound of its float32 evaluation's error, propagated operation by operation; where signed terms are
added the rounding is charged on the sum of the ABSOLUTE terms, where all terms are non-negative on the value itself:

    g'   two products and a sum, plus the error p brings:        dg = 2u*gabs + 2*l2*dp,   gabs = |g*gs| + |2*l2*p|
    m    carried error, g', two products and a sum:              dm = b1*dm + omb1*dg + 3u*mabs,   mabs = b1*mabs + omb1*gabs
    a, v square (2|g'|dg + u g'^2), two products and a sum:      da = rho*da + omr*(2|g'|dg + u*g'^2) + 3u*a      (RMSprop, Nadam)
    a    square and a sum (Adagrad):                             da = da + 2|g'|dg + u*g'^2 + u*a
    u    a product and a maximum, which rounds nothing and moves by no more than its operands do (Adamax):
                                                                 du = max(b2*du + u*b2*u_, dg)
    D = sqrt(d) + eps:  dD = dd/(2 sqrt(d)) + u*sqrt(d) + u*D     (Adamax: D = u_ + eps, dD = du + u*D)
    q = lr*x/D:         dq = lr*dx/D + |q|*dD/D + 2u*|q|          (x = g', m or mbar)
    p = p - q:          dp = dp + dq + u*(|p| + |q|)
    Nadam:  g'c_g and m c_m are one product each (c*dx + u|.|), v c_v likewise; mbar is two products and a sum of signed
            terms:  dmbar = omc*d(g'c_g) + mc1*d(m c_m) + 3u*(omc*|g'c_g| + mc1*|m c_m|)

The asserted bound is SAFETY = 2 times the first-order bound, for the second-order terms it drops; it is not fitted to what
the code gives."""
import numpy as np

U = 2.0 ** -24
SAFETY = 2.0
SIZES = [1, 3, 4, 5, 7, 1021]
STEPS = 3
THREADS = 256

RULES = {
    "rmsprop": dict(entry="dj_rmsprop_update", host="rmsprop_host", state=("a",)),
    "adagrad": dict(entry="dj_adagrad_update", host="adagrad_host", state=("a",)),
    "adamax": dict(entry="dj_adamax_update", host="adamax_host", state=("m", "u")),
    "nadam": dict(entry="dj_nadam_update", host="nadam_host", state=("m", "v")),
}


def several_passes(groups_per_pass):
    """Smallest interesting n for which threads of the capped grid take a second group: the cap is the launcher's."""
    return 4 * int(groups_per_pass) + 4 * 1000 + 3


def nadam_schedule(step, beta_1=0.9, beta_2=0.999, schedule_decay=0.004):
    """(c_g, c_m, c_v, 1 - mc(t), mc(t+1)) of the step that starts at iterations = `step`, float64: Keras' get_updates with
    its m_schedule variable carried through the steps before."""
    mc = lambda i: beta_1 * (1.0 - 0.5 * (0.96 ** (i * schedule_decay)))
    m_schedule = 1.0
    for done in range(step):
        m_schedule = m_schedule * mc(done + 1)
    t = step + 1
    new = m_schedule * mc(t)
    nxt = new * mc(t + 1)
    return (1.0 / (1.0 - new), 1.0 / (1.0 - nxt), 1.0 / (1.0 - beta_2 ** t), 1.0 - mc(t), mc(t + 1))


# the scalars of each step, in the order the statement and the entry point take them.  "dyadic": every scalar exact in float32
SCALAR_SETS = {
    "dyadic": dict(rmsprop=[(2.0 ** -6, 0.5, 2.0 ** -8)] * STEPS,
                   adagrad=[(2.0 ** -6, 2.0 ** -8)] * STEPS,
                   adamax=[(2.0 ** -6, 0.5, 0.5, 2.0 ** -8)] * STEPS,
                   nadam=[(2.0 ** -6, 0.5, 0.5, 2.0 ** -8, 2.0, 4.0, 2.0, 0.5, 0.25)] * STEPS,
                   l2=(0.0, 2.0 ** -4), grad_scale=(1.0, 0.5)),
    "normal": dict(rmsprop=[(0.001 / (1 + 1e-4 * i), 0.9, 1e-7) for i in range(STEPS)],
                   adagrad=[(0.01 / (1 + 1e-4 * i), 1e-7) for i in range(STEPS)],
                   adamax=[(0.002 / (1 + 1e-4 * i) / (1 - 0.9 ** (i + 1)), 0.9, 0.999, 1e-7) for i in range(STEPS)],
                   nadam=[(0.002, 0.9, 0.999, 1e-7) + nadam_schedule(i) for i in range(STEPS)],
                   l2=(0.0, 5e-4), grad_scale=(1.0, 0.5)),
}


def inputs(n, kind, seed=15):
    """-> p (n,), g (STEPS, n), float32.  dyadic: multiples of 1/8 in [-4, 4]; normal: p ~ N(0, 1), g ~ N(0, 0.1)."""
    rng = np.random.default_rng(seed + 1000003 * (kind == "normal"))
    if kind == "dyadic":
        return (rng.integers(-32, 33, n) / 8.0).astype(np.float32), (rng.integers(-32, 33, (STEPS, n)) / 8.0).astype(np.float32)
    return rng.standard_normal(n).astype(np.float32), (0.1 * rng.standard_normal((STEPS, n))).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------
# one step in which EVERY operation is exact in float32 (so float32 and float64 evaluations must agree element for element)
# ----------------------------------------------------------------------------------------------------------------------
def exact_case(rule, n=257, seed=19):
    """-> (arrays p, g and the rule's state, scalars, l2, grad_scale).  g' = g/8 + p/8 is a multiple of 1/8 with |g'| <= 1.5;
    eps = 2^-8, S = 4 - eps, lr = 2^-6, and every rho / beta is 1/2.
    rmsprop: a0 = 2 S^2 - g'^2, so that the new a is S^2, sqrt(a) + eps = 4 and the quotient divides by a power of two.
    adagrad: a0 = S^2 - g'^2, likewise.
    adamax:  m0 a multiple of 1/8; even elements u0 = 2 S (the decayed norm S wins the maximum, u + eps = 4); odd elements
             u0 = 0 and m0 = -g' (|g'| wins; the new m is 0, so the quotient 0 / (|g'| + eps) is exact too).
    nadam:   c_g = 2, c_m = 4, c_v = 4, 1 - mc_t = 1/2, mc_t1 = 1/4; v0 = S^2 / 2 - g'^2, so that v c_v = S^2."""
    rng = np.random.default_rng(seed)
    eps, lr = 2.0 ** -8, 2.0 ** -6
    p = rng.integers(-4, 5, n).astype(np.float64)
    g = rng.integers(-8, 9, n).astype(np.float64)
    ge = g * 0.125 + 0.125 * p
    S = 4.0 - eps
    m0 = rng.integers(-16, 17, n) / 8.0
    if rule == "rmsprop":
        arrays, scalars = dict(p=p, g=g, a=2.0 * S * S - ge * ge), (lr, 0.5, eps)
    elif rule == "adagrad":
        arrays, scalars = dict(p=p, g=g, a=S * S - ge * ge), (lr, eps)
    elif rule == "adamax":
        odd = np.arange(n) % 2 == 1
        arrays = dict(p=p, g=g, m=np.where(odd, -ge, m0), u=np.where(odd, 0.0, 2.0 * S))
        scalars = (lr, 0.5, 0.5, eps)
    else:
        arrays, scalars = dict(p=p, g=g, m=m0, v=S * S / 2.0 - ge * ge), (lr, 0.5, 0.5, eps, 2.0, 4.0, 4.0, 0.5, 0.25)
    assert all(np.array_equal(a.astype(np.float32).astype(np.float64), a) for a in arrays.values())
    return {k: a.astype(np.float32) for k, a in arrays.items()}, scalars, 2.0 ** -4, 0.125


# ----------------------------------------------------------------------------------------------------------------------
# special values: one row per element, l2 = 0, grad_scale = 1, the default scalars
# ----------------------------------------------------------------------------------------------------------------------
_INF, _NAN = np.inf, np.nan
#                  p     g        second state (the accumulator, Adamax' u, Nadam's v); the first-moment state starts at 0
SPECIAL_ROWS = [(1.5, 0.0, 0.0),          # g = 0 on zero state: 0 / (0 + eps), p unchanged; Adamax: u stays 0
                (1.5, _INF, 0.0), (1.5, -_INF, 0.0),
                (1.5, _NAN, 0.0),         # NaN enters Adamax' maximum from the gradient's side
                (0.5, 0.25, _NAN),        # ... and from the state's side
                (_INF, 0.25, 0.0),        # p = Inf with l2 = 0: 0 * Inf in the effective gradient
                (0.5, 1e-20, 0.0), (0.5, -1e-20, 0.0),      # g^2 is a float32 denormal
                (0.5, 0.0, 1e-40), (0.5, 1e-30, 1e-40),     # a denormal state
                (0.5, 0.25, 2.0 ** 60), (0.5, -0.25, 1e30),  # a large second state: it swallows epsilon
                (-0.0, 0.0, 0.0), (0.0, -0.0, 0.0)]
UNCHANGED, NAN_ROWS, FINITE_FROM = 0, slice(1, 6), 6


def special_inputs():
    rows = np.array(SPECIAL_ROWS, dtype=np.float64)
    return tuple(rows[:, i].astype(np.float32) for i in range(3))


# ----------------------------------------------------------------------------------------------------------------------
# the rules in float64, with the first-order error bound of their float32 evaluation (module docstring)
# ----------------------------------------------------------------------------------------------------------------------
def _f(x):
    return float(np.float32(x))


def _head(s, g, l2, gs):
    two_l2 = float(np.float32(2.0) * np.float32(l2))
    gs = _f(gs)
    g = np.asarray(g, np.float64)
    ge = g * gs + two_l2 * s["p"]
    gabs = np.abs(g * gs) + np.abs(two_l2 * s["p"])
    return ge, gabs, 2 * U * gabs + two_l2 * s["dp"]


def _move(s, lr, x, dx, D, dD):
    """p = p - lr*x/D with the bound of the module docstring."""
    q = lr * x / D
    dq = lr * dx / D + np.abs(q) * dD / D + 2 * U * np.abs(q)
    s["dp"] = s["dp"] + dq + U * (np.abs(s["p"]) + np.abs(q))
    s["p"] = s["p"] - q


def _root_plus_eps(d, dd, eps):
    root = np.sqrt(d)
    D = root + eps
    assert not np.any((root == 0) & (dd > 0))        # d = 0 only from zero gradients: dd is 0 there
    return D, dd / (2 * np.where(root > 0, root, 1.0)) + U * root + U * D


def _first_moment(s, ge, gabs, dg, beta_1):
    b1, omb1 = _f(beta_1), float(np.float32(1) - np.float32(beta_1))
    s["mabs"] = b1 * s["mabs"] + omb1 * gabs
    s["dm"] = b1 * s["dm"] + omb1 * dg + 3 * U * s["mabs"]
    s["m"] = b1 * s["m"] + omb1 * ge


def _second_moment(s, name, ge, dg, beta):
    b, omb = _f(beta), float(np.float32(1) - np.float32(beta))
    s[name] = b * s[name] + omb * (ge * ge)
    s["d" + name] = b * s["d" + name] + omb * (2 * np.abs(ge) * dg + U * ge * ge) + 3 * U * s[name]


def rmsprop_f64(s, g, lr, rho, epsilon, l2, grad_scale):
    ge, _, dg = _head(s, g, l2, grad_scale)
    _second_moment(s, "a", ge, dg, rho)
    D, dD = _root_plus_eps(s["a"], s["da"], _f(epsilon))
    _move(s, _f(lr), ge, dg, D, dD)
    return s


def adagrad_f64(s, g, lr, epsilon, l2, grad_scale):
    ge, _, dg = _head(s, g, l2, grad_scale)
    s["a"] = s["a"] + ge * ge
    s["da"] = s["da"] + 2 * np.abs(ge) * dg + U * ge * ge + U * s["a"]
    D, dD = _root_plus_eps(s["a"], s["da"], _f(epsilon))
    _move(s, _f(lr), ge, dg, D, dD)
    return s


def adamax_f64(s, g, lr_t, beta_1, beta_2, epsilon, l2, grad_scale):
    ge, gabs, dg = _head(s, g, l2, grad_scale)
    _first_moment(s, ge, gabs, dg, beta_1)
    b2 = _f(beta_2)
    s["du"] = np.maximum(b2 * s["du"] + U * b2 * s["u"], dg)
    s["u"] = np.maximum(b2 * s["u"], np.abs(ge))
    D = s["u"] + _f(epsilon)
    _move(s, _f(lr_t), s["m"], s["dm"], D, s["du"] + U * D)
    return s


def nadam_f64(s, g, lr, beta_1, beta_2, epsilon, c_g, c_m, c_v, omc_t, mc_t1, l2, grad_scale):
    c_g, c_m, c_v, omc_t, mc_t1 = (_f(x) for x in (c_g, c_m, c_v, omc_t, mc_t1))
    ge, gabs, dg = _head(s, g, l2, grad_scale)
    _first_moment(s, ge, gabs, dg, beta_1)
    _second_moment(s, "v", ge, dg, beta_2)
    gp, mp, vp = ge * c_g, s["m"] * c_m, s["v"] * c_v
    dgp, dmp, dvp = c_g * dg + U * np.abs(gp), c_m * s["dm"] + U * np.abs(mp), c_v * s["dv"] + U * vp
    mbar = omc_t * gp + mc_t1 * mp
    dmbar = omc_t * dgp + mc_t1 * dmp + 3 * U * (omc_t * np.abs(gp) + mc_t1 * np.abs(mp))
    D, dD = _root_plus_eps(vp, dvp, _f(epsilon))
    _move(s, _f(lr), mbar, dmbar, D, dD)
    return s


F64 = {"rmsprop": rmsprop_f64, "adagrad": adagrad_f64, "adamax": adamax_f64, "nadam": nadam_f64}


def f64_state(rule, p, **given):
    """The float64 state of a rule: p, its state buffers (zero unless given), and a zero bound for each (and mabs)."""
    z = lambda: np.zeros(len(p), np.float64)
    s = dict(p=np.asarray(p, np.float64), dp=z(), mabs=z())
    for name in RULES[rule]["state"]:
        s[name] = np.asarray(given[name], np.float64) if name in given else z()
        s["d" + name] = z()
    return s


# ----------------------------------------------------------------------------------------------------------------------
# launch geometry of csrc/dj_optim.hip, for the bound of the sum of squares
# ----------------------------------------------------------------------------------------------------------------------
def terms_per_thread(n, groups_per_pass):
    """Most float32 terms one thread adds to its partial sum: four per group, one group per pass of the capped grid."""
    groups = (n + 3) // 4
    blocks = min(max(-(-groups // THREADS), 1), groups_per_pass // THREADS)
    return 4 * -(-groups // (blocks * THREADS))


def sumsq_bound(n, groups_per_pass):
    """The project's bound of start + sum(p^2) as the kernel adds it, relative: (k + 8) 2^-24, k the terms per thread."""
    return (terms_per_thread(n, groups_per_pass) + 8) * U
