"""keras.optimizers.Adam / Adadelta without a GPU: compile() accepts them, the classes' surface, and the float32 statement
(adam_host, adadelta_host) pinned independently of itself -- against the rules typed again in float64
(tests/optimizer_cases.py), exactly where every operation is exact and within the derived bound elsewhere, and against
known answers worked out by hand.  SGD's statement (sgd_host): its fma against an evaluation in integers, the step against
the oracle's (tests/loss_head_cases.py), exactly on dyadic data and within that file's bound elsewhere."""
import math
import os

import numpy as np
import pytest

import loss_head_cases as lc
import optimizer_cases as oc


def _graph_only_model():
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras import layers as L
    from jpeg_detection_resnet_ssd_amd.keras.models import Model
    K.clear_session()
    x = L.Input(shape=(4, 4, 3))
    y = L.Dense(6, activation="softmax")(L.GlobalAveragePooling2D()(L.Conv2D(8, (3, 3), padding="same")(x)))
    return Model(x, y)


@pytest.mark.parametrize("spec", ["Adam()", "Adam(amsgrad=True)", "Adadelta()", "'sgd'", "'SGD'", "SGD()"])
def test_compile_accepts_instances_of_the_three_optimizers(spec):
    from jpeg_detection_resnet_ssd_amd.keras import optimizers as O
    opt = eval(spec, {"Adam": O.Adam, "Adadelta": O.Adadelta, "SGD": O.SGD})
    model = _graph_only_model()
    model.compile(optimizer=opt, loss="categorical_crossentropy")
    want = {"adam": O.Adam, "adadelta": O.Adadelta, "sgd": O.SGD}[spec.strip("'").split("(")[0].lower()]
    assert type(model.optimizer) is want
    if not isinstance(opt, str):
        assert model.optimizer is opt


@pytest.mark.parametrize("bad", ["rmsprop", "nadam", "adam", "Adadelta", object(), None, 3])
def test_unknown_optimizers_still_raise_and_name_what_exists(bad):
    """'adam' and 'adadelta' among them: compile(optimizer="adam") raised before the two classes existed, an existing test
    (tests/test_callbacks_cpu.py) asserts that it does, and nothing that existed changes behaviour -- instances only."""
    with pytest.raises(NotImplementedError) as e:
        _graph_only_model().compile(optimizer=bad, loss="categorical_crossentropy")
    assert all(name in str(e.value) for name in ("SGD", "Adam", "Adadelta"))


def test_defaults_config_and_keyword_arguments():
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import SGD, Adadelta, Adam
    a = Adam()
    assert a.get_config() == {"lr": 0.001, "beta_1": 0.9, "beta_2": 0.999, "decay": 0.0, "epsilon": 1e-7, "amsgrad": False}
    assert a.iterations == 0
    ref = Adam(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-08, decay=0.0)          # the reference's own call
    assert ref.epsilon == 1e-8 and ref.get_config()["epsilon"] == 1e-8
    assert Adam(amsgrad=True).get_config()["amsgrad"] is True
    d = Adadelta()
    assert d.get_config() == {"lr": 1.0, "rho": 0.95, "decay": 0.0, "epsilon": 1e-7}
    assert d.iterations == 0
    for cls in (Adam, Adadelta, SGD):
        for clip in ("clipnorm", "clipvalue"):
            with pytest.raises(NotImplementedError, match=clip):
                cls(**{clip: 1.0})
    for cls in (Adam, Adadelta):
        with pytest.raises(TypeError):
            cls(momentum=0.9)


def test_current_lr_and_step_size():
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import Adadelta, Adam
    for opt, lr in ((Adam(lr=0.002), 0.002), (Adadelta(lr=0.5), 0.5)):
        opt.iterations = 999
        assert opt.current_lr() == lr
    for opt, lr in ((Adam(lr=0.002, decay=1e-3), 0.002), (Adadelta(lr=0.5, decay=1e-3), 0.5)):
        assert opt.current_lr() == lr
        opt.iterations = 999
        assert opt.current_lr() == lr / (1.0 + 1e-3 * 999)
    for decay in (0.0, 1e-4):
        opt = Adam(lr=0.001, beta_1=0.9, beta_2=0.999, decay=decay)
        for it in (0, 1, 999):
            opt.iterations = it
            lr_dec = 0.001 / (1.0 + decay * it) if decay else 0.001
            want = lr_dec * math.sqrt(1.0 - 0.999 ** (it + 1)) / (1.0 - 0.9 ** (it + 1))
            assert opt.step_size() == pytest.approx(want, rel=1e-15)
            assert opt.current_lr() == lr_dec
    opt = Adam()
    assert opt.step_size() == pytest.approx(0.001 * math.sqrt(0.001) / 0.1, rel=1e-12)     # t = 1 by hand


@pytest.mark.parametrize("amsgrad", [False, True])
def test_adam_statement_is_exact_where_every_operation_is(amsgrad):
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import adam_host
    arr, sc = oc.exact_adam_case()
    got = adam_host(arr["p"], arr["g"], arr["m"], arr["v"], arr["vhat"] if amsgrad else None, **sc)
    s = oc.adam_state(arr["p"])
    s.update(m=arr["m"].astype(np.float64), v=arr["v"].astype(np.float64), vhat=arr["vhat"].astype(np.float64))
    oc.adam_f64(s, arr["g"], amsgrad=amsgrad, **sc)
    for name, g in zip(("p", "m", "v"), got):
        assert g.dtype == np.float32 and np.array_equal(g.astype(np.float64), s[name]), name
    if amsgrad:
        assert np.array_equal(got[3].astype(np.float64), s["vhat"]) and np.array_equal(got[3], got[2])
    else:
        assert got[3] is None
    assert not np.array_equal(got[0], arr["p"])


def test_adadelta_statement_is_exact_where_every_operation_is():
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import adadelta_host
    arr, sc = oc.exact_adadelta_case()
    got = adadelta_host(arr["p"], arr["g"], arr["a"], arr["d"], sc["lr"], sc["rho"], sc["epsilon"], sc["l2"], sc["grad_scale"])
    s = oc.adadelta_state(arr["p"])
    s.update(a=arr["a"].astype(np.float64), d=arr["d"].astype(np.float64))
    oc.adadelta_f64(s, arr["g"], **sc)
    for name, g in zip(("p", "a", "d"), got):
        assert g.dtype == np.float32 and np.array_equal(g.astype(np.float64), s[name]), name
    assert not np.array_equal(got[0], arr["p"])


def _within(got, want, bound, name):
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= oc.SAFETY * bound), "%s: worst error / bound = %.3g" % (name, float(np.max(err / (oc.SAFETY * bound))))


@pytest.mark.parametrize("kind", ["dyadic", "normal"])
@pytest.mark.parametrize("amsgrad", [False, True])
def test_adam_statement_stays_within_the_derived_bound_over_three_steps(kind, amsgrad):
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import adam_host
    sc = oc.SCALAR_SETS[kind]
    k = sc["adam"]
    p0, gs = oc.inputs(1021, kind)
    for l2 in sc["l2"]:
        for scale in sc["grad_scale"]:
            p, m, v = p0, np.zeros_like(p0), np.zeros_like(p0)
            vhat = np.zeros_like(p0) if amsgrad else None
            s = oc.adam_state(p0)
            for t in range(oc.STEPS):
                p, m, v, vhat = adam_host(p, gs[t], m, v, vhat, k["lr_t"][t], k["beta_1"], k["beta_2"], k["epsilon"], l2, scale)
                oc.adam_f64(s, gs[t], k["lr_t"][t], k["beta_1"], k["beta_2"], k["epsilon"], l2, scale, amsgrad)
                _within(p, s["p"], s["dp"], "p")
                _within(m, s["m"], s["dm"], "m")
                _within(v, s["v"], s["dv"], "v")
                if amsgrad:
                    _within(vhat, s["vhat"], s["dvhat"], "vhat")
            assert float(np.max(s["dp"] / (np.abs(s["p"]) + 1e-3))) < 1e-4        # the bound itself is tight enough to mean something


@pytest.mark.parametrize("kind", ["dyadic", "normal"])
def test_adadelta_statement_stays_within_the_derived_bound_over_three_steps(kind):
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import adadelta_host
    sc = oc.SCALAR_SETS[kind]
    k = sc["adadelta"]
    p0, gs = oc.inputs(1021, kind)
    for l2 in sc["l2"]:
        for scale in sc["grad_scale"]:
            p, a, d = p0, np.zeros_like(p0), np.zeros_like(p0)
            s = oc.adadelta_state(p0)
            for t in range(oc.STEPS):
                p, a, d = adadelta_host(p, gs[t], a, d, k["lr"][t], k["rho"], k["epsilon"], l2, scale)
                oc.adadelta_f64(s, gs[t], k["lr"][t], k["rho"], k["epsilon"], l2, scale)
                _within(p, s["p"], s["dp"], "p")
                _within(a, s["a"], s["da"], "a")
                _within(d, s["d"], s["dd"], "d")
            assert float(np.max(s["dp"] / (np.abs(s["p"]) + 1e-3))) < 1e-4


def test_adam_known_answers_from_zero_state():
    """m = (1-b1) g, v = (1-b2) g^2, lr_t = lr sqrt(1-b2)/(1-b1): p moves by lr_t m / (sqrt(v) + eps) = lr g / (|g| + eps')
    with eps' = eps / sqrt(1-b2) -- the sign of g times lr, to a relative 3e-6 for |g| >= 1 and the default eps."""
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import Adam, adam_host
    opt = Adam()
    g = np.array([1.0, -2.0, 1000.0, -1e4], np.float32)
    p0 = np.array([0.5, -0.5, 2.0, 0.0], np.float32)
    z = np.zeros(4, np.float32)
    p, m, v, vhat = adam_host(p0, g, z, z, None, opt.step_size(), opt.beta_1, opt.beta_2, opt.epsilon, 0.0, 1.0)
    assert vhat is None
    np.testing.assert_allclose(m, 0.1 * g.astype(np.float64), rtol=1e-6)
    omb2 = float(np.float32(1) - np.float32(0.999))          # 0.00100005: Keras holds beta_2 as a float32 variable
    np.testing.assert_allclose(v, omb2 * g.astype(np.float64) ** 2, rtol=1e-6)
    np.testing.assert_allclose(v, 0.001 * g.astype(np.float64) ** 2, rtol=1e-4)
    eps1 = 1e-7 / math.sqrt(0.001)
    np.testing.assert_allclose(p.astype(np.float64) - p0, -0.001 * g / (np.abs(g) + eps1), rtol=1e-4, atol=0)
    np.testing.assert_allclose(p.astype(np.float64) - p0, -0.001 * np.sign(g), rtol=1e-4)
    # a power-of-two example where nothing rounds: b1 = b2 = 1/2, lr_t = 1/4, eps = 0, g = 2 -> m = 1; with v0 = 28 the new v is
    # 14 + 2 = 16, sqrt 4, step (1/4) / 4 = 1/16
    p, m, v, _ = adam_host([1.0], [2.0], [0.0], [28.0], None, 0.25, 0.5, 0.5, 0.0, 0.0, 1.0)
    assert (float(p[0]), float(m[0]), float(v[0])) == (1.0 - 0.0625, 1.0, 16.0)
    # l2 and grad_scale enter the gradient: g' = 8 * 0.25 + 2 * 0.5 * 2 = 4
    p, m, v, _ = adam_host([2.0], [8.0], [0.0], [0.0], None, 0.25, 0.5, 0.5, 0.0, 0.5, 0.25)
    assert (float(m[0]), float(v[0])) == (2.0, 8.0)


def test_adadelta_known_answers_from_zero_state():
    """a = (1-rho) g^2; u = g sqrt(eps) / sqrt(a + eps); p -= lr u; d = (1-rho) u^2."""
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import adadelta_host
    # rho = 3/4, eps = 1/4, g = 3: a = 9/4, u = 3 * (1/2) / sqrt(10/4)
    p, a, d = adadelta_host([1.0], [3.0], [0.0], [0.0], 1.0, 0.75, 0.25, 0.0, 1.0)
    u = 1.5 / math.sqrt(2.5)
    assert float(a[0]) == 2.25
    assert float(p[0]) == pytest.approx(1.0 - u, abs=2.0 ** -23)         # the subtraction rounds at the size of p = 1
    assert float(d[0]) == pytest.approx(0.25 * u * u, rel=3e-7)
    # every operation exact: rho = 1/2, eps = 1/4, g = 4, a0 = 15.5 -> a = 15.75, sqrt(16) = 4, u = 4 * (1/2) / 4 = 1/2
    p, a, d = adadelta_host([1.0], [4.0], [15.5], [0.0], 0.5, 0.5, 0.25, 0.0, 1.0)
    assert (float(p[0]), float(a[0]), float(d[0])) == (0.75, 15.75, 0.125)
    # the defaults on a large gradient: u -> sqrt(eps) / sqrt(1 - rho) * sign(g)
    p, a, d = adadelta_host([0.0, 0.0], [100.0, -100.0], [0.0, 0.0], [0.0, 0.0], 1.0, 0.95, 1e-7, 0.0, 1.0)
    np.testing.assert_allclose(p, [-math.sqrt(1e-7 / 0.05), math.sqrt(1e-7 / 0.05)], rtol=1e-5)


def test_amsgrad_keeps_vhat_when_v_decreases():
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import adam_host
    z = np.zeros(3, np.float32)
    g1, g2 = np.array([4.0, -4.0, 0.5], np.float32), np.array([0.25, 0.25, 2.0], np.float32)
    p, m, v1, h1 = adam_host(z, g1, z, z, z, 0.25, 0.5, 0.5, 0.0, 0.0, 1.0)
    assert np.array_equal(h1, v1) and np.array_equal(v1, [8.0, 8.0, 0.125])
    p2, m2, v2, h2 = adam_host(p, g2, m, v1, h1, 0.25, 0.5, 0.5, 0.0, 0.0, 1.0)
    assert np.all(v2[:2] < v1[:2]) and np.array_equal(h2[:2], v1[:2]) and v2[2] > v1[2] and h2[2] == v2[2]
    want = p.astype(np.float64) - 0.25 * m2.astype(np.float64) / np.sqrt(h2.astype(np.float64))
    np.testing.assert_allclose(p2, want, rtol=1e-6)
    plain = adam_host(p, g2, m, v1, None, 0.25, 0.5, 0.5, 0.0, 0.0, 1.0)[0]
    assert np.all(np.abs(p2[:2] - p[:2]) < np.abs(plain[:2] - p[:2]))       # the kept maximum shortens the step


def test_nan_and_inf_propagate():
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import adadelta_host, adam_host
    z = np.zeros(3, np.float32)
    g = np.array([np.nan, 1.0, np.inf], np.float32)
    p, m, v, h = adam_host(z + 1, g, z, z, z, 0.001, 0.9, 0.999, 1e-7, 0.0, 1.0)
    assert all(np.isnan(t[0]) for t in (p, m, v, h)) and all(np.isfinite(t[1]) for t in (p, m, v, h))
    assert np.isinf(m[2]) and np.isinf(v[2]) and np.isnan(p[2])             # Inf / Inf
    h = adam_host(z + 1, z, z, z, np.array([np.nan, 0, 0], np.float32), 0.001, 0.9, 0.999, 1e-7, 0.0, 1.0)[3]
    assert np.isnan(h[0]) and h[1] == 0                                      # NaN in vhat stays (np.maximum)
    p, a, d = adadelta_host(z + 1, g, z, z, 1.0, 0.95, 1e-7, 0.0, 1.0)
    assert all(np.isnan(t[0]) for t in (p, a, d)) and all(np.isfinite(t[1]) for t in (p, a, d))
    # p = Inf with l2 = 0: the penalty is a product all the same
    assert np.isnan(adam_host([np.inf], [0.25], [0.0], [0.0], None, 0.001, 0.9, 0.999, 1e-7, 0.0, 1.0)[0][0])
    # g = 0 on zero state leaves p alone
    assert adam_host([1.5], [0.0], [0.0], [0.0], None, 0.001, 0.9, 0.999, 1e-7, 0.0, 1.0)[0][0] == np.float32(1.5)
    assert adadelta_host([1.5], [0.0], [0.0], [0.0], 1.0, 0.95, 1e-7, 0.0, 1.0)[0][0] == np.float32(1.5)


# ----------------------------------------------------------------------------------------------------------------------
# SGD
# ----------------------------------------------------------------------------------------------------------------------
def _int_parts(x):
    """A finite float32 as m * 2^e with m an integer."""
    m, e = math.frexp(float(x))
    return int(m * 2 ** 24), e - 24


def _round_to_f32(n, e):
    """n * 2^e (n any Python integer) rounded to the nearest float32, ties to even, with denormals and overflow."""
    if n == 0:
        return np.float32(0.0)
    sign, n = (-1.0 if n < 0 else 1.0), abs(n)
    q = max(n.bit_length() - 1 + e - 23, -149)          # exponent of the last place kept
    shift = q - e
    if shift <= 0:
        r, q = n, e
    else:
        r, rem, half = n >> shift, n & ((1 << shift) - 1), 1 << (shift - 1)
        if rem > half or (rem == half and r & 1):
            r += 1
    if r.bit_length() + q > 128:
        return np.float32(sign * np.inf)
    return np.float32(sign * math.ldexp(r, q))


def _exact_fma(a, b, c):
    (ma, ea), (mb, eb), (mc, ec) = _int_parts(a), _int_parts(b), _int_parts(c)
    e = min(ea + eb, ec)
    return _round_to_f32((ma * mb << (ea + eb - e)) + (mc << (ec - e)), e)


def _fma_traps():
    """a*b + c whose exact value lies within 2^-60 (relative) of the midpoint of two float32 values, on either side of it:
    a*b = 2^16 (1 - k^2 2^-46) and c = +-C 2^17, C an integer of 24 bits.  The float64 sum of the exact product and c is the
    midpoint itself, so rounding it to float32 goes to the even neighbour whatever the side."""
    out = []
    for k in (1, 2, 3, 7, 32):
        a, b = np.float32(256 * (1 + k * 2.0 ** -23)), np.float32(256 * (1 - k * 2.0 ** -23))
        for C in (2 ** 23 + 1, 2 ** 23 + 2, 2 ** 23 + 5, 2 ** 24 - 1, 2 ** 24 - 2, 12345678, 12345679):
            for sa in (1, -1):
                for sc in (1, -1):
                    out.append((np.float32(sa) * a, b, np.float32(sc * C * 2.0 ** 17)))
    return out


def test_fma32_equals_the_evaluation_in_integers_on_random_triples():
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import fma32
    rng = np.random.default_rng(11)
    n = 4000
    mant = lambda: (rng.integers(2 ** 23, 2 ** 24, n) * rng.choice([-1.0, 1.0], n))
    a = (mant() * 2.0 ** rng.integers(-40, 10, n)).astype(np.float32)
    b = (mant() * 2.0 ** rng.integers(-40, 10, n)).astype(np.float32)
    c = (mant() * 2.0 ** rng.integers(-60, 10, n)).astype(np.float32)
    near = rng.random(n) < 0.5          # half of them cancel: c within a few float32 ulp of -a*b
    c[near] = (-(a[near].astype(np.float64) * b[near]) * (1 + rng.integers(-4, 5, near.sum()) * 2.0 ** -23)).astype(np.float32)
    tiny = rng.random(n) < 0.1          # results among the float32 denormals
    a[tiny] = (a[tiny].astype(np.float64) * 2.0 ** -100).astype(np.float32)
    c[tiny] = (c[tiny].astype(np.float64) * 2.0 ** -100).astype(np.float32)
    huge = np.arange(n) % 97 == 0       # overflow
    a[huge], b[huge] = np.float32(2.0 ** 100), np.float32(3.0 * 2.0 ** 27)
    got = fma32(a, b, c)
    want = np.array([_exact_fma(*t) for t in zip(a, b, c)], np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.isinf(want).any() and ((want != 0) & (np.abs(want) < np.finfo(np.float32).tiny)).any()
    assert ((want != 0) & (np.abs(want) < 2.0 ** -20 * np.abs(c))).any()             # cancellation did happen
    # by hand: 1 + 2^-24 is a tie (to even: 1), anything above it is not
    one, h = np.float32(1), np.float32(2.0 ** -12)
    assert fma32(h, h, one) == one and fma32(h, np.float32(2.0 ** -12 + 2.0 ** -35), one) == np.float32(1 + 2.0 ** -23)
    assert np.isnan(fma32(np.float32(np.inf), np.float32(0), one)) and fma32(np.float32(np.inf), one, one) == np.inf


def test_fma32_at_double_rounding_traps():
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import fma32
    traps = _fma_traps()
    wrong = 0
    for a, b, c in traps:
        (ma, ea), (mb, eb), (mc, ec) = _int_parts(a), _int_parts(b), _int_parts(c)
        e = min(ea + eb, ec)
        exact = (ma * mb << (ea + eb - e)) + (mc << (ec - e))           # the value is exact * 2^e
        want = _exact_fma(a, b, c)
        mw, ew = _int_parts(want)
        near = mw << (ew - e)                                           # the float32 it rounds to, and the one on the other side
        other = np.nextafter(want, np.float32(np.inf if exact > near else -np.inf))
        mo, eo = _int_parts(other)
        twice_mid = near + (mo << (eo - e))
        dist = abs(2 * exact - twice_mid)                               # twice the distance to the midpoint
        assert 0 < dist and dist << 60 <= 2 * abs(exact), (a, b, c)
        assert fma32(a, b, c) == want and fma32(b, a, c) == want, (a, b, c)
        wrong += int(np.float32(np.float64(a) * np.float64(b) + np.float64(c)) != want)
    assert len(traps) >= 100 and wrong >= len(traps) // 4        # the float64 expression rounded to float32 falls into them


def test_sgd_statement_equals_the_oracle_on_dyadic_data():
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import sgd_host
    for n in (63, 257):
        p, g, v = lc.sgd_input(n, "dyadic")
        for cfg in lc.sgd_configs(n, "dyadic"):
            p64, v64 = lc.ref_sgd(p, g, v, cfg)
            pn, vn = sgd_host(p, g, v, cfg.lr_t, cfg.momentum, cfg.nesterov, cfg.l2, cfg.grad_scale)
            assert pn.dtype == vn.dtype == np.float32
            assert np.array_equal(pn.astype(np.float64), p64) and np.array_equal(vn.astype(np.float64), v64), cfg
    assert not np.array_equal(pn, p)


def test_sgd_statement_stays_within_the_bound_of_the_loss_head_cases():
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import sgd_host
    import torch
    for n in (63, 257):
        p, g, v = lc.sgd_input(n, "normal")
        for cfg in lc.sgd_configs(n, "normal"):
            p64, v64 = lc.ref_sgd(p, g, v, cfg)
            p32, v32 = lc.ref_sgd(p, g, v, cfg, torch.float32)
            sp, sv = lc.sgd_scales(p, g, v, cfg)
            pn, vn = sgd_host(p, g, v, cfg.lr_t, cfg.momentum, cfg.nesterov, cfg.l2, cfg.grad_scale)
            assert lc.rel_err(pn, p64, sp) <= lc.bound(p32, p64, sp), cfg
            assert lc.rel_err(vn, v64, sv) <= lc.bound(v32, v64, sv), cfg


def test_sgd_known_answers():
    """Nothing rounds: g' = 8 * 0.25 + 2 * 0.5 * 2 = 4; v = 0.5 * 2 - 0.25 * 4 = 0; with v0 = 6: v = 2, p = 2 + 2, and with
    nesterov p = 2 + 0.5 * 2 - 1 = 2."""
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import sgd_host
    assert [float(t[0]) for t in sgd_host([2.0], [8.0], [2.0], 0.25, 0.5, False, 0.5, 0.25)] == [2.0, 0.0]
    assert [float(t[0]) for t in sgd_host([2.0], [8.0], [6.0], 0.25, 0.5, False, 0.5, 0.25)] == [4.0, 2.0]
    assert [float(t[0]) for t in sgd_host([2.0], [8.0], [6.0], 0.25, 0.5, True, 0.5, 0.25)] == [2.0, 2.0]
    assert np.isnan(sgd_host([np.inf], [0.25], [0.0], 0.1, 0.9, False, 0.0, 1.0)[0][0])       # 0 * Inf in the penalty


def test_get_weights_needs_a_compiled_model():
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import Adam
    with pytest.raises(RuntimeError, match="compile"):
        Adam().get_weights()
    with pytest.raises(RuntimeError, match="compile"):
        Adam().set_weights([])


def _built_lib():
    from jpeg_detection_resnet_ssd_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("the HIP library has not been built")
    return _lib.load()


def test_library_exports_the_entry_points_and_keeps_its_abi_version():
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _built_lib()
    for name in ("dj_sgd_momentum_update", "dj_adam_update", "dj_adadelta_update", "dj_optim_groups_per_pass"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.dj_abi_version() == 5 and _lib.ABI_VERSION == 5
    assert lib.dj_optim_groups_per_pass() > 0 and lib.dj_optim_groups_per_pass() % 256 == 0


def test_argument_checks_refuse_before_any_launch():
    """Device pointers are made up and never dereferenced: every call here must fail in the host checks."""
    lib = _built_lib()
    P, G, M, V, H, S = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
    sc = (0.001, 0.9, 0.999, 1e-7, 0.0, 1.0)
    bad_adam = [(None, G, M, V, H, 64), (P, None, M, V, H, 64), (P, G, None, V, H, 64), (P, G, M, None, None, 64),
                (P, G, M, V, H, 0), (P, G, M, V, None, -4), (P, G, P, V, H, 64), (P, G, M, P, None, 64), (P, G, M, V, P, 64),
                (P, G, P + 4 * 63, V, None, 64), (P, G, M, M, None, 64)]
    for (p, g, m, v, h, n) in bad_adam:
        assert lib.dj_adam_update(p, g, m, v, h, n, *sc, S, None) == -1, (p, g, m, v, h, n)
        assert b"dj_adam_update" in lib.dj_last_error()
    sd = (1.0, 0.95, 0.05, 1e-7, 0.0, 1.0)
    bad_adadelta = [(None, G, M, V, 64), (P, None, M, V, 64), (P, G, None, V, 64), (P, G, M, None, 64), (P, G, M, V, 0),
                    (P, G, P, V, 64), (P, G, M, P, 64), (P, G, M, P + 4 * 63, 64), (P, G, M, M, 64)]
    for (p, g, a, d, n) in bad_adadelta:
        assert lib.dj_adadelta_update(p, g, a, d, n, *sd, None, None) == -1, (p, g, a, d, n)
        assert b"dj_adadelta_update" in lib.dj_last_error()
    ss = (0.1, 0.9, 1, 5e-4, 1.0)
    bad_sgd = [(None, G, V, 64), (P, None, V, 64), (P, G, None, 64), (P, G, V, 0), (P, G, V, -4), (P, G, P, 64), (P, P, V, 64),
               (P, G, P + 4 * 63, 64), (P, G, G, 64)]
    for (p, g, v, n) in bad_sgd:
        assert lib.dj_sgd_momentum_update(p, g, v, n, *ss, S, None) == -1, (p, g, v, n)
        assert b"dj_sgd_momentum_update" in lib.dj_last_error()
