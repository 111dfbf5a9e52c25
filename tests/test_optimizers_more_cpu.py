"""keras.optimizers.RMSprop / Adagrad / Adamax / Nadam without a GPU: compile() accepts them, the classes' surface, and
the float32 statements (rmsprop_host, adagrad_host, adamax_host, nadam_host) pinned independently of themselves -- against
the rules typed again in float64 (tests/optimizer_more_cases.py), exactly where every operation is exact and within the
derived bound elsewhere, and against known answers worked out by hand."""
import math

import numpy as np
import pytest

import optimizer_more_cases as mc

RULE_NAMES = sorted(mc.RULES)


def _O():
    from jpeg_detection_resnet_ssd_amd.keras import optimizers
    return optimizers


def _host(rule):
    return getattr(_O(), mc.RULES[rule]["host"])


def _classes():
    O = _O()
    return {"rmsprop": O.RMSprop, "adagrad": O.Adagrad, "adamax": O.Adamax, "nadam": O.Nadam}


def _graph_only_model():
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras import layers as L
    from jpeg_detection_resnet_ssd_amd.keras.models import Model
    K.clear_session()
    x = L.Input(shape=(4, 4, 3))
    y = L.Dense(6, activation="softmax")(L.GlobalAveragePooling2D()(L.Conv2D(8, (3, 3), padding="same")(x)))
    return Model(x, y)


# ----------------------------------------------------------------------------------------------------------------------
# the statements
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULE_NAMES)
def test_statement_is_exact_where_every_operation_is(rule):
    arr, scalars, l2, scale = mc.exact_case(rule)
    names = mc.RULES[rule]["state"]
    got = _host(rule)(arr["p"], arr["g"], *[arr[k] for k in names], *scalars, l2, scale)
    s = mc.f64_state(rule, arr["p"], **{k: arr[k] for k in names})
    mc.F64[rule](s, arr["g"], *scalars, l2, scale)
    assert len(got) == 1 + len(names)
    for name, t in zip(("p",) + names, got):
        assert t.dtype == np.float32 and np.array_equal(t.astype(np.float64), s[name]), name
    moved = got[0] != arr["p"]
    assert np.any(moved)
    if rule == "adamax":        # both sides of the maximum: the decayed norm on even elements, |g'| on odd ones (m is 0 there)
        ge = arr["g"].astype(np.float64) / 8 + arr["p"].astype(np.float64) / 8
        assert np.array_equal(got[2][1::2], np.abs(ge[1::2]).astype(np.float32)) and np.all(got[2][0::2] == np.float32(4 - 2.0 ** -8))
        assert not np.any(moved[1::2]) and np.any(ge[1::2] != 0)


def _within(got, want, bound, name):
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= mc.SAFETY * bound), "%s: worst error / bound = %.3g" % (name, float(np.max(err / (mc.SAFETY * bound))))


@pytest.mark.parametrize("kind", ["dyadic", "normal"])
@pytest.mark.parametrize("rule", RULE_NAMES)
def test_statement_stays_within_the_derived_bound_over_three_steps(rule, kind):
    sc = mc.SCALAR_SETS[kind]
    names = mc.RULES[rule]["state"]
    p0, gs = mc.inputs(1021, kind)
    for l2 in sc["l2"]:
        for scale in sc["grad_scale"]:
            cur = (p0,) + tuple(np.zeros_like(p0) for _ in names)
            s = mc.f64_state(rule, p0)
            for t in range(mc.STEPS):
                cur = _host(rule)(cur[0], gs[t], *cur[1:], *sc[rule][t], l2, scale)
                mc.F64[rule](s, gs[t], *sc[rule][t], l2, scale)
                for name, got in zip(("p",) + names, cur):
                    _within(got, s[name], s["d" + name], "%s step %d" % (name, t))
            assert not np.array_equal(cur[0], p0)
            assert float(np.max(s["dp"] / (np.abs(s["p"]) + 1e-3))) < 1e-4        # the bound itself is tight enough to mean something


def test_rmsprop_known_answers():
    """a = rho a + (1 - rho) g'^2; p -= lr g' / (sqrt(a) + eps)."""
    rmsprop_host = _O().rmsprop_host
    # nothing rounds: rho = 1/2, g = 4, a0 = 16 -> a = 8 + 8 = 16, sqrt 4, step (1/4 * 4) / 4 = 1/4
    p, a = rmsprop_host([1.0], [4.0], [16.0], 0.25, 0.5, 0.0, 0.0, 1.0)
    assert (float(p[0]), float(a[0])) == (0.75, 16.0)
    # l2 and grad_scale enter the gradient: g' = 8 * 0.25 + 2 * 0.5 * 2 = 4, the same step from p = 2
    p, a = rmsprop_host([2.0], [8.0], [16.0], 0.25, 0.5, 0.0, 0.5, 0.25)
    assert (float(p[0]), float(a[0])) == (1.75, 16.0)
    # the defaults from zero state: a = (1 - rho) g^2, the step lr sign(g) / sqrt(1 - rho) for |g| >> eps
    g = np.array([1.0, -2.0, 1000.0, -1e4], np.float32)
    p0 = np.array([0.5, -0.5, 2.0, 0.0], np.float32)
    p, a = rmsprop_host(p0, g, np.zeros(4, np.float32), 0.001, 0.9, 1e-7, 0.0, 1.0)
    omr = float(np.float32(1) - np.float32(0.9))            # 0.100000024: Keras holds rho as a float32 variable
    np.testing.assert_allclose(a, omr * g.astype(np.float64) ** 2, rtol=1e-6)
    np.testing.assert_allclose(p.astype(np.float64) - p0, -0.001 * np.sign(g) / math.sqrt(0.1), rtol=1e-4)


def test_adagrad_known_answers():
    """a += g'^2; p -= lr g' / (sqrt(a) + eps)."""
    adagrad_host = _O().adagrad_host
    # nothing rounds: g = 4, a0 = 48 -> a = 64, sqrt 8, step (1/2 * 4) / 8 = 1/4
    p, a = adagrad_host([1.0], [4.0], [48.0], 0.5, 0.0, 0.0, 1.0)
    assert (float(p[0]), float(a[0])) == (0.75, 64.0)
    p, a = adagrad_host([2.0], [8.0], [48.0], 0.5, 0.0, 0.5, 0.25)      # g' = 8 * 0.25 + 2 * 0.5 * 2 = 4
    assert (float(p[0]), float(a[0])) == (1.75, 64.0)
    # from zero state: a = g^2, the step lr g / (|g| + eps) = lr sign(g)
    g = np.array([1.0, -2.0, 1000.0, -1e4], np.float32)
    p0 = np.array([0.5, -0.5, 2.0, 0.0], np.float32)
    p, a = adagrad_host(p0, g, np.zeros(4, np.float32), 0.01, 1e-7, 0.0, 1.0)
    assert np.array_equal(a, g * g)
    np.testing.assert_allclose(p.astype(np.float64) - p0, -0.01 * np.sign(g), rtol=1e-5)
    # the accumulator only grows: a second equal gradient moves p by 1/sqrt(2) of the first step
    p2, a2 = adagrad_host(p, g, a, 0.01, 1e-7, 0.0, 1.0)
    assert np.array_equal(a2, 2 * g * g)
    np.testing.assert_allclose(p2.astype(np.float64) - p, -0.01 * np.sign(g) / math.sqrt(2), rtol=1e-4)


def test_adamax_known_answers():
    """m = b1 m + (1 - b1) g'; u = max(b2 u, |g'|); p -= lr_t m / (u + eps)."""
    adamax_host = _O().adamax_host
    # nothing rounds: b1 = b2 = 1/2, m0 = 2, g = 4 -> m = 3.  u0 = 4: max(2, 4) = 4 (the gradient wins), step (1/2 * 3) / 4
    p, m, u = adamax_host([1.0], [4.0], [2.0], [4.0], 0.5, 0.5, 0.5, 0.0, 0.0, 1.0)
    assert (float(p[0]), float(m[0]), float(u[0])) == (1.0 - 0.375, 3.0, 4.0)
    # u0 = 16: max(8, 4) = 8 (the decayed norm wins), step 1.5 / 8; a negative gradient enters by its absolute value
    p, m, u = adamax_host([1.0, 1.0], [4.0, -4.0], [2.0, -2.0], [16.0, 2.0], 0.5, 0.5, 0.5, 0.0, 0.0, 1.0)
    assert [float(x) for x in p] == [1.0 - 0.1875, 1.0 + 0.375] and [float(x) for x in u] == [8.0, 4.0]
    p, m, u = adamax_host([2.0], [8.0], [2.0], [4.0], 0.5, 0.5, 0.5, 0.0, 0.5, 0.25)     # g' = 8 * 0.25 + 2 * 0.5 * 2 = 4
    assert (float(p[0]), float(m[0]), float(u[0])) == (2.0 - 0.375, 3.0, 4.0)
    # the defaults from zero state: m = 0.1 g, u = |g|, lr_t = lr / 0.1: the step is lr sign(g)
    g = np.array([1.0, -2.0, 1000.0, -1e4], np.float32)
    p0 = np.array([0.5, -0.5, 2.0, 0.0], np.float32)
    z = np.zeros(4, np.float32)
    p, m, u = adamax_host(p0, g, z, z, _O().Adamax().step_size(), 0.9, 0.999, 1e-7, 0.0, 1.0)
    assert np.array_equal(u, np.abs(g))
    np.testing.assert_allclose(p.astype(np.float64) - p0, -0.002 * np.sign(g), rtol=1e-4)      # the subtraction rounds at the size of p


def _mc_by_exp(i, beta_1=0.9, schedule_decay=0.004):
    """The momentum cache by another route than the power: 0.96^x = exp(x ln 0.96)."""
    return beta_1 * (1.0 - 0.5 * math.exp(i * schedule_decay * math.log(0.96)))


def test_nadam_known_answers_and_schedule_scalars():
    O = _O()
    # nothing rounds: b1 = b2 = 1/2, g = 4 from zero state -> m = 2, v = 8; c_g = 2, c_m = 4, c_v = 2: v c_v = 16, sqrt 4;
    # mbar = 1/2 (4 * 2) + 1/4 (2 * 4) = 6; step (1/4 * 6) / 4 = 3/8
    p, m, v = O.nadam_host([1.0], [4.0], [0.0], [0.0], 0.25, 0.5, 0.5, 0.0, 2.0, 4.0, 2.0, 0.5, 0.25, 0.0, 1.0)
    assert (float(p[0]), float(m[0]), float(v[0])) == (0.625, 2.0, 8.0)
    p, m, v = O.nadam_host([2.0], [8.0], [0.0], [0.0], 0.25, 0.5, 0.5, 0.0, 2.0, 4.0, 2.0, 0.5, 0.25, 0.5, 0.25)   # g' = 4
    assert (float(p[0]), float(m[0]), float(v[0])) == (1.625, 2.0, 8.0)
    # the schedule of the defaults, by hand: 0.96^0.004 = exp(0.004 ln 0.96) = exp(-0.000163288) = 0.99983673, so
    # mc(1) = 0.9 (1 - 0.499918364) = 0.45007347
    assert _mc_by_exp(1) == pytest.approx(0.45007347, rel=2e-8)
    opt = O.Nadam()
    assert opt.m_schedule == 1.0
    c_g, c_m, c_v, omc, mc1 = opt.step_scalars()
    m1, m2, m3 = _mc_by_exp(1), _mc_by_exp(2), _mc_by_exp(3)
    assert c_g == pytest.approx(1.0 / (1.0 - m1), rel=1e-12) and c_g == pytest.approx(1.0 / 0.54992653, rel=1e-7)
    assert c_m == pytest.approx(1.0 / (1.0 - m1 * m2), rel=1e-12)
    assert c_v == pytest.approx(1000.0, rel=1e-9)                # 1 / (1 - 0.999)
    assert omc == pytest.approx(1.0 - m1, rel=1e-12) and mc1 == pytest.approx(m2, rel=1e-12)
    opt.iterations = 1
    assert opt.m_schedule == pytest.approx(m1, rel=1e-12)
    c_g, c_m, c_v, omc, mc1 = opt.step_scalars()
    assert c_g == pytest.approx(1.0 / (1.0 - m1 * m2), rel=1e-12)
    assert c_m == pytest.approx(1.0 / (1.0 - m1 * m2 * m3), rel=1e-12)
    assert c_v == pytest.approx(1.0 / (1.0 - 0.999 * 0.999), rel=1e-12)
    assert omc == pytest.approx(1.0 - m2, rel=1e-12) and mc1 == pytest.approx(m3, rel=1e-12)
    for it in (0, 1, 2):        # the cases module carries Keras' variable through the steps instead
        opt.iterations = it
        assert opt.step_scalars() == pytest.approx(mc.nadam_schedule(it), rel=1e-14)
    # the defaults from zero state on one large gradient: m = 0.1 g, v = 0.001 g^2, v c_v = g^2; mbar = (1 - mc_1) g c_g +
    # mc_2 0.1 g c_m, and the step lr mbar / |g|
    opt.iterations = 0
    c_g, c_m, c_v, omc, mc1 = opt.step_scalars()
    p, m, v = O.nadam_host([0.5, -0.5], [100.0, -100.0], [0.0, 0.0], [0.0, 0.0], 0.002, 0.9, 0.999, 1e-7, c_g, c_m, c_v, omc, mc1,
                           0.0, 1.0)
    want = 0.002 * (omc * c_g + mc1 * 0.1 * c_m)
    np.testing.assert_allclose(p.astype(np.float64) - [0.5, -0.5], [-want, want], rtol=1e-4)
    assert 0.002 < want < 0.0025               # (1 - mc_1) c_g = 1 exactly in real numbers; the momentum term adds 0.1 mc_2 c_m


def test_nan_inf_and_zero_gradients():
    p0, g, second = mc.special_inputs()
    z = np.zeros(len(p0), np.float32)
    sc = mc.SCALAR_SETS["normal"]
    for rule in RULE_NAMES:
        first = (z,) if len(mc.RULES[rule]["state"]) == 2 else ()
        out = _host(rule)(p0, g, *first, second, *sc[rule][0], 0.0, 1.0)
        p = out[0]
        assert p[mc.UNCHANGED] == p0[mc.UNCHANGED], rule                # 0 / (0 + eps)
        assert out[-1][mc.UNCHANGED] == 0, rule
        assert np.isnan(p[mc.NAN_ROWS]).all() and np.isfinite(p[mc.FINITE_FROM:]).all(), rule
    O = _O()
    # NaN passes through Adamax' maximum from either side
    u = O.adamax_host([1.0, 1.0], [np.nan, 0.5], [0.0, 0.0], [1.0, np.nan], 0.002, 0.9, 0.999, 1e-7, 0.0, 1.0)[2]
    assert np.isnan(u).all()
    # denormals are kept: RMSprop's accumulator of a gradient whose square is one, Adamax' decayed norm of a denormal state
    a = O.rmsprop_host([0.5], [1e-20], [0.0], 0.001, 0.9, 1e-7, 0.0, 1.0)[1]
    assert 0 < a[0] < np.finfo(np.float32).tiny
    u = O.adamax_host([0.5], [0.0], [0.0], [1e-40], 0.002, 0.9, 0.999, 1e-7, 0.0, 1.0)[2]
    assert 0 < u[0] < np.float32(1e-40)


# ----------------------------------------------------------------------------------------------------------------------
# the classes
# ----------------------------------------------------------------------------------------------------------------------
def test_defaults_and_config():
    O = _O()
    assert O.RMSprop().get_config() == {"lr": 0.001, "rho": 0.9, "decay": 0.0, "epsilon": 1e-7}
    assert O.Adagrad().get_config() == {"lr": 0.01, "decay": 0.0, "epsilon": 1e-7}
    assert O.Adamax().get_config() == {"lr": 0.002, "beta_1": 0.9, "beta_2": 0.999, "decay": 0.0, "epsilon": 1e-7}
    assert O.Nadam().get_config() == {"lr": 0.002, "beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7, "schedule_decay": 0.004}
    for cls in _classes().values():
        opt = cls()
        assert opt.iterations == 0 and isinstance(opt, O.Optimizer)
        assert cls(epsilon=None).epsilon == 1e-7 and cls(epsilon=1e-8).get_config()["epsilon"] == 1e-8
        twin = cls(**cls(lr=0.5, epsilon=1e-3).get_config())
        assert twin.get_config() == cls(lr=0.5, epsilon=1e-3).get_config()
    assert O.RMSprop.state_names == O.Adagrad.state_names == ("accumulators",)
    assert O.Adamax.state_names == ("ms", "us") and O.Nadam.state_names == ("ms", "vs")


def test_stray_keywords_and_clipping_raise():
    for cls in _classes().values():
        for clip in ("clipnorm", "clipvalue"):
            with pytest.raises(NotImplementedError, match=clip):
                cls(**{clip: 1.0})
        with pytest.raises(TypeError, match="momentum"):
            cls(momentum=0.9)
    with pytest.raises(TypeError):
        _O().Nadam(decay=1e-4)             # Keras' Nadam has no decay argument


def test_current_lr_and_adamax_step_size():
    O = _O()
    for cls in (O.RMSprop, O.Adagrad, O.Adamax):
        opt = cls(lr=0.5)
        opt.iterations = 999
        assert opt.current_lr() == 0.5
        opt = cls(lr=0.5, decay=1e-3)
        assert opt.current_lr() == 0.5
        opt.iterations = 999
        assert opt.current_lr() == 0.5 / (1.0 + 1e-3 * 999)
    opt = O.Nadam(lr=0.5)
    opt.iterations = 999
    assert opt.current_lr() == 0.5
    for decay in (0.0, 1e-4):
        opt = O.Adamax(lr=0.002, beta_1=0.9, decay=decay)
        for it in (0, 1, 999):
            opt.iterations = it
            lr_dec = 0.002 / (1.0 + decay * it) if decay else 0.002
            assert opt.step_size() == pytest.approx(lr_dec / (1.0 - 0.9 ** (it + 1)), rel=1e-15)
    assert O.Adamax().step_size() == pytest.approx(0.02, rel=1e-12)          # t = 1 by hand: 0.002 / 0.1


def test_update_calls_name_the_entry_points_and_carry_the_step_scalars():
    O = _O()
    asked = []
    buffer = lambda name: asked.append(name) or name
    opt = O.RMSprop(lr=0.5, decay=1e-3)
    opt.iterations = 4
    assert opt.update_call(buffer) == ("dj_rmsprop_update", ["accumulators"], (0.5 / (1.0 + 1e-3 * 4), 0.9, 1e-7))
    opt = O.Adagrad(lr=0.5, decay=1e-3)
    opt.iterations = 4
    assert opt.update_call(buffer) == ("dj_adagrad_update", ["accumulators"], (0.5 / (1.0 + 1e-3 * 4), 1e-7))
    opt = O.Adamax()
    opt.iterations = 4
    assert opt.update_call(buffer) == ("dj_adamax_update", ["ms", "us"], (opt.step_size(), 0.9, 0.999, 1e-7))
    opt = O.Nadam()
    opt.iterations = 4
    assert opt.update_call(buffer) == ("dj_nadam_update", ["ms", "vs"], (0.002, 0.9, 0.999, 1e-7) + mc.nadam_schedule(4))
    assert asked == ["accumulators", "accumulators", "ms", "us", "ms", "vs"]
    from jpeg_detection_resnet_ssd_amd import _lib
    for rule, d in mc.RULES.items():           # (param, grad, *state, n, *scalars, l2, grad_scale, sumsq, stream)
        res, args = _lib.SIGNATURES[d["entry"]]
        assert len(args) == 2 + len(d["state"]) + 1 + len(mc.SCALAR_SETS["normal"][rule][0]) + 4, rule


def test_nadam_m_schedule_is_a_function_of_iterations_alone():
    O = _O()
    product = lambda k, b1=0.9, sd=0.004: math.prod(b1 * (1.0 - 0.5 * 0.96 ** (i * sd)) for i in range(1, k + 1))
    opt = O.Nadam()
    for it in (0, 1, 2, 7, 500):
        opt.iterations = it                      # set directly, as set_weights and a restart do
        assert opt.m_schedule == pytest.approx(product(it), rel=1e-13)
    walked = O.Nadam()
    for it in range(501):                        # ... and bit for bit what a run that took every step holds
        walked.iterations = it
        walked.m_schedule
    assert walked.m_schedule == opt.m_schedule
    opt.iterations = 3                           # going back
    assert opt.m_schedule == pytest.approx(product(3), rel=1e-13)
    other = O.Nadam(beta_1=0.8, schedule_decay=0.01)
    other.iterations = 5
    assert other.m_schedule == pytest.approx(product(5, 0.8, 0.01), rel=1e-13)
    assert "m_schedule" not in other.get_config() and O.Nadam.state_names == ("ms", "vs")


@pytest.mark.parametrize("rule", RULE_NAMES)
def test_compile_accepts_an_instance(rule):
    opt = _classes()[rule]()
    model = _graph_only_model()
    model.compile(optimizer=opt, loss="categorical_crossentropy")
    assert model.optimizer is opt


@pytest.mark.parametrize("bad", ["rmsprop", "RMSprop", "adagrad", "adamax", "nadam", "adam"])
def test_names_are_still_not_resolved(bad):
    with pytest.raises(NotImplementedError) as e:
        _graph_only_model().compile(optimizer=bad, loss="categorical_crossentropy")
    import re
    assert all(re.search(r"\b%s\b" % name, str(e.value)) for name in ("SGD", "Adam", "Adadelta", "RMSprop", "Adagrad", "Adamax", "Nadam"))


@pytest.mark.parametrize("rule", RULE_NAMES)
def test_get_weights_and_set_weights_errors_without_a_gpu(rule):
    cls = _classes()[rule]
    with pytest.raises(RuntimeError, match="compile"):
        cls().get_weights()
    with pytest.raises(RuntimeError, match="compile"):
        cls().set_weights([])
    model = _graph_only_model()
    opt = cls()
    model.compile(optimizer=opt, loss="categorical_crossentropy")
    shapes = [tuple(w.shape) for w in model.weight_specs if w.trainable]
    assert len(shapes) == 4
    good = [np.asarray(7, np.int64)] + [np.zeros(s, np.float32) for _ in cls.state_names for s in shapes]
    with pytest.raises(ValueError, match=r"Length of the specified weight list \(%d\) does not match the number of weights of "
                                         r"the optimizer \(%d\)" % (len(good) - 1, len(good))):
        opt.set_weights(good[:-1])
    wrong = list(good)
    wrong[2] = np.zeros(shapes[1] + (2,), np.float32)
    with pytest.raises(ValueError, match="Optimizer weight shape .* not compatible with provided weight shape"):
        opt.set_weights(wrong)
    assert opt.iterations == 0                   # refused before any write
    stale = cls()
    model.compile(optimizer=stale, loss="categorical_crossentropy")
    with pytest.raises(RuntimeError, match="compile"):
        opt.get_weights()                        # no longer the model's optimizer


def test_header_declares_the_entry_points_the_binding_lists():
    import os
    import re
    from jpeg_detection_resnet_ssd_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "dj_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for d in mc.RULES.values():
        assert re.search(r"\bint %s\s*\(" % d["entry"], header) and d["entry"] in _lib.SIGNATURES and hasattr(lib, d["entry"])
    assert "#define DJ_ABI_VERSION 5" in header and lib.dj_abi_version() == _lib.ABI_VERSION == 5


def test_argument_checks_refuse_before_any_launch():
    """Device pointers are made up and never dereferenced: every call here must fail in the host checks, naming the rule."""
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    P, G, A, B, S = 0x100000, 0x200000, 0x300000, 0x400000, 0x600000
    for rule, d in mc.RULES.items():
        scalars = mc.SCALAR_SETS["normal"][rule][0] + (0.0, 1.0)
        fn = getattr(lib, d["entry"])
        if len(d["state"]) == 1:
            bad = [(None, G, A, 64), (P, None, A, 64), (P, G, None, 64), (P, G, A, 0), (P, G, A, -4), (P, G, P, 64), (P, P, A, 64),
                   (P, G, G, 64), (P, G, P + 4 * 63, 64), (P, P - 4 * 63, A, 64)]
        else:
            bad = [(None, G, A, B, 64), (P, None, A, B, 64), (P, G, None, B, 64), (P, G, A, None, 64), (P, G, A, B, 0),
                   (P, G, A, B, -4), (P, G, P, B, 64), (P, G, A, P, 64), (P, G, A, A, 64), (P, G, A, A + 4 * 63, 64), (P, P, A, B, 64)]
        for args in bad:
            assert fn(*args, *scalars, S, None) == -1, (rule, args)
            assert d["entry"].encode() in lib.dj_last_error(), (rule, args)
