"""dj_rmsprop_update / dj_adagrad_update / dj_adamax_update / dj_nadam_update against the host statement
(keras/optimizers.py), bit for bit, and the four optimizers behind Model.compile: sizes around the group of four and the
tail, a size that takes the grid-stride loop round more than once, a base pointer that is not 16-byte aligned, both scalar
sets, l2 with a sum of squares and without either, grad_scale, three chained steps, special values, the argument checks,
teacher-forced training steps of a small model (the statement applied to the engine's own gradients), float16 mode, the
get_weights / set_weights round trip into a fresh model, and the state dropped on a change of optimizer.

No test compares two training runs with each other: the weight-gradient GEMMs may accumulate with atomics.  The round trip
applies the statement to each model's own gradients instead."""
import numpy as np
import pytest
import torch

import optimizer_more_cases as mc

pytestmark = pytest.mark.gpu

GUARD = 7.0
RULE_NAMES = sorted(mc.RULES)
START = 3.25            # what a sum-of-squares slot holds before the launch adds to it


def _lib():
    from jpeg_detection_resnet_ssd_amd import _lib
    return _lib.load()


def _gpp():
    return int(_lib().dj_optim_groups_per_pass())


def _host(rule):
    from jpeg_detection_resnet_ssd_amd.keras import optimizers
    return getattr(optimizers, mc.RULES[rule]["host"])


def _same_bits(got, want, what=""):
    """Equal bit for bit, NaNs at the same positions (their payloads are not compared)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), what


class Buffers(object):
    """Device copies of host arrays of n elements at element offset `off` of an aligned allocation, each followed by a
    guard element."""

    def __init__(self, cuda, off, **arrays):
        self.t = {}
        for name, a in arrays.items():
            host = np.full(len(a) + off + 1, GUARD, np.float32)
            host[off:off + len(a)] = a
            view = torch.from_numpy(host).to(cuda)[off:]
            assert (view.data_ptr() % 16 == 0) == (off == 0)
            self.t[name] = view

    def __getitem__(self, name):
        return self.t[name]

    def host(self, name, n):
        h = self.t[name].cpu().numpy()
        assert h[n] == GUARD, name + ": the element after the last was written"
        return h[:n]


def _launch(rule, b, n, scalars, l2, scale, sumsq=None):
    from jpeg_detection_resnet_ssd_amd.engine import call
    d = mc.RULES[rule]
    call(d["entry"], b["p"], b["g"], *[b[k] for k in d["state"]], n, *scalars, l2, scale, sumsq)


def _chain(cuda, rule, n, kind, off, l2, scale, p0, gs):
    """Three steps with the state carried, each compared with the statement; with l2 the launch also adds sum(p^2) of the
    parameters it started from to a slot, without l2 it is given none."""
    names = mc.RULES[rule]["state"]
    sc = mc.SCALAR_SETS[kind][rule]
    cur = (p0,) + tuple(np.zeros(n, np.float32) for _ in names)
    b = Buffers(cuda, off, p=p0, g=gs[0], **dict(zip(names, cur[1:])))
    bound = mc.sumsq_bound(n, _gpp())
    for t in range(mc.STEPS):
        if t:
            b["g"][:n].copy_(torch.from_numpy(gs[t]))
        ss = torch.full((3,), START, device=cuda) if l2 else None
        exact = START + float(np.sum(cur[0].astype(np.float64) ** 2))
        _launch(rule, b, n, sc[t], l2, scale, ss[1:2] if l2 else None)
        cur = _host(rule)(cur[0], gs[t], *cur[1:], *sc[t], l2, scale)
        what = "%s n=%d %s off=%d l2=%g scale=%g step %d: " % (rule, n, kind, off, l2, scale, t)
        for name, want in zip(("p",) + names, cur):
            _same_bits(b.host(name, n), want, what + name)
        _same_bits(b.host("g", n), gs[t], what + "g")                   # the gradient is left alone
        if l2:
            ssh = ss.cpu().numpy()
            assert ssh[0] == START and ssh[2] == START, what
            print(what + "sumsq relative error %.3g, bound %.3g" % (abs(float(ssh[1]) - exact) / exact, bound))
            assert abs(float(ssh[1]) - exact) <= bound * exact, what
    return cur


@pytest.mark.parametrize("n", mc.SIZES)
@pytest.mark.parametrize("rule", RULE_NAMES)
def test_kernels_equal_the_host_statement(cuda, rule, n):
    for kind, sc in mc.SCALAR_SETS.items():
        p0, gs = mc.inputs(n, kind)
        for off in (0, 1):                  # off 1: no pointer is 16-byte aligned, so the 16-byte path must fall back
            for l2 in sc["l2"]:
                for scale in sc["grad_scale"]:
                    _chain(cuda, rule, n, kind, off, l2, scale, p0, gs)


@pytest.mark.parametrize("rule", RULE_NAMES)
def test_several_passes_of_the_capped_grid(cuda, rule):
    n = mc.several_passes(_gpp())
    assert mc.terms_per_thread(n, _gpp()) > 4
    p0, gs = mc.inputs(n, "normal")
    _chain(cuda, rule, n, "normal", 0, 5e-4, 0.5, p0, gs)


@pytest.mark.parametrize("rule", RULE_NAMES)
def test_a_single_misaligned_pointer_takes_the_fallback(cuda, rule):
    """Only one buffer is offset: the launcher must look at every pointer."""
    n = 1021
    names = mc.RULES[rule]["state"]
    p0, gs = mc.inputs(n, "normal")
    sc = mc.SCALAR_SETS["normal"][rule][0]
    start = dict(p=p0, g=gs[0], **{k: np.abs(gs[1 + i]) for i, k in enumerate(names)})
    want = _host(rule)(p0, gs[0], *[start[k] for k in names], *sc, 5e-4, 1.0)
    for odd in ("p", "g") + names:
        b = Buffers(cuda, 0, **start)
        b.t[odd] = Buffers(cuda, 1, x=start[odd])["x"]
        _launch(rule, b, n, sc, 5e-4, 1.0)
        for name, w in zip(("p",) + names, want):
            _same_bits(b.host(name, n), w, "%s, %s offset: %s" % (rule, odd, name))


@pytest.mark.parametrize("rule", RULE_NAMES)
def test_special_values(cuda, rule):
    """g = 0 on zero state (0 / (0 + eps); Adamax: u = 0), +-Inf, NaN in the gradient and in the state (either side of
    Adamax' maximum), p = Inf with l2 = 0, gradients whose square is a float32 denormal, a denormal state, signed zeros and a
    large second state: whatever the statement gives (checked by hand in tests/test_optimizers_more_cpu.py), bit for bit."""
    p0, g, second = mc.special_inputs()
    n = len(p0)
    names = mc.RULES[rule]["state"]
    sc = mc.SCALAR_SETS["normal"][rule][0]
    start = dict(zip(names, ((np.zeros(n, np.float32),) if len(names) == 2 else ()) + (second,)))
    want = _host(rule)(p0, g, *[start[k] for k in names], *sc, 0.0, 1.0)
    assert want[0][mc.UNCHANGED] == p0[mc.UNCHANGED] and want[-1][mc.UNCHANGED] == 0
    assert np.isnan(want[0][mc.NAN_ROWS]).all() and np.isfinite(want[0][mc.FINITE_FROM:]).all()
    if rule == "adamax":
        assert np.isnan(want[2][3]) and np.isnan(want[2][4])            # NaN from the gradient's side and from the state's
    tiny = np.finfo(np.float32).tiny
    assert any(np.any((w > 0) & (w < tiny)) for w in want[1:])          # a denormal state survives
    for off in (0, 1):
        b = Buffers(cuda, off, p=p0, g=g, **start)
        _launch(rule, b, n, sc, 0.0, 1.0)
        for name, w in zip(("p",) + names, want):
            _same_bits(b.host(name, n), w, "%s special values off=%d: %s" % (rule, off, name))


@pytest.mark.parametrize("rule", RULE_NAMES)
def test_updates_do_not_depend_on_the_sum_of_squares(cuda, rule):
    n = 1021
    names = mc.RULES[rule]["state"]
    p0, gs = mc.inputs(n, "normal", seed=18)
    sc = mc.SCALAR_SETS["normal"][rule][0]
    z = np.zeros(n, np.float32)
    got = []
    for with_sum in (True, False):
        b = Buffers(cuda, 0, p=p0, g=gs[0], **{k: z for k in names})
        ss = torch.full((3,), START, device=cuda)
        _launch(rule, b, n, sc, 5e-4, 1.0, ss[1:2] if with_sum else None)
        assert (float(ss[1]) != START) == with_sum and float(ss[0]) == float(ss[2]) == START
        got.append([b.host(name, n) for name in ("p",) + names])
    for x, y in zip(*got):
        _same_bits(x, y, "with and without sumsq")


@pytest.mark.parametrize("rule", RULE_NAMES)
def test_argument_checks_launch_nothing(cuda, rule):
    lib = _lib()
    n = 64
    d = mc.RULES[rule]
    p0, gs = mc.inputs(n, "normal")
    z = np.zeros(n, np.float32)
    scalars = mc.SCALAR_SETS["normal"][rule][0] + (0.0, 1.0)
    stream = torch.cuda.current_stream().cuda_stream
    b = Buffers(cuda, 0, p=p0, g=gs[0], a=z, b=z, ss=np.zeros(1, np.float32))
    P, G, A, B, S = (b[k].data_ptr() for k in ("p", "g", "a", "b", "ss"))
    if len(d["state"]) == 1:
        bad = [(None, G, A, n), (P, None, A, n), (P, G, None, n), (P, G, A, 0), (P, G, A, -4), (P, G, P, n), (P, P, A, n),
               (P, G, G, n), (P, G, P + 4 * (n - 1), n), (P, P - 4 * (n - 1), A, n)]
    else:
        bad = [(None, G, A, B, n), (P, None, A, B, n), (P, G, None, B, n), (P, G, A, None, n), (P, G, A, B, 0), (P, G, A, B, -4),
               (P, G, P, B, n), (P, G, A, P, n), (P, G, A, A, n), (P, G, A, A + 4 * (n - 1), n), (P, P, A, B, n)]
    fn = getattr(lib, d["entry"])
    for args in bad:
        assert fn(*args, *scalars, S, stream) == -1, args
        assert d["entry"].encode() in lib.dj_last_error(), args
    torch.cuda.synchronize()
    for name, want in (("p", p0), ("g", gs[0]), ("a", z), ("b", z), ("ss", np.zeros(1, np.float32))):
        _same_bits(b.host(name, len(want)), want, name + " after refused calls")


# ----------------------------------------------------------------------------------------------------------------------
# model level
# ----------------------------------------------------------------------------------------------------------------------
N_CLASSES, BATCH = 6, 8


def _optimizers():
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import Adagrad, Adamax, Nadam, RMSprop
    return {"rmsprop": lambda: RMSprop(lr=1e-3, decay=1e-4), "adagrad": lambda: Adagrad(decay=1e-4),
            "adamax": lambda: Adamax(decay=1e-4), "nadam": lambda: Nadam()}


def _model(optimizer, seed=5):
    """Conv2D (l2 5e-4, no bias) - BatchNormalization - ReLU - Conv2D (un-regularised) - GlobalAveragePooling2D - Dense
    (l2 1e-3): two l2 segments, an un-regularised segment (biases, gamma, beta, the second kernel) and moving statistics."""
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras import layers as L
    from jpeg_detection_resnet_ssd_amd.keras.models import Model
    from jpeg_detection_resnet_ssd_amd.keras.regularizers import l2
    K.clear_session()
    K.set_random_seed(seed)
    x = L.Input(shape=(8, 8, 32))
    h = L.Conv2D(32, (3, 3), padding="same", use_bias=False, kernel_regularizer=l2(5e-4), name="conv1")(x)
    h = L.Activation("relu", name="relu1")(L.BatchNormalization(name="bn1")(h))
    h = L.Conv2D(32, (1, 1), padding="same", activation="relu", name="conv2")(h)
    y = L.Dense(N_CLASSES, activation="softmax", kernel_regularizer=l2(1e-3), name="probs")(L.GlobalAveragePooling2D(name="pool")(h))
    model = Model(x, y)
    model.compile(optimizer=optimizer, loss="categorical_crossentropy")
    return model


def _batch(seed=3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((BATCH, 8, 8, 32)).astype(np.float32)
    y = np.eye(N_CLASSES, dtype=np.float32)[rng.integers(0, N_CLASSES, BATCH)]
    return x, y


def _snapshot(model):
    st = model._store
    torch.cuda.synchronize()
    snap = dict(p=st["flat"][:st["n_train"]].cpu().numpy().copy(), rest=st["flat"][st["n_train"]:].cpu().numpy().copy())
    for name in model.optimizer.state_names:
        snap[name] = model._optimizer_buffer(name).cpu().numpy().copy()
    return snap


def _statement_step(model, before, iterations):
    """The host statement applied per segment to the engine's own gradients and the state captured before the step, with
    the scalars of a fresh optimizer object at `iterations` (for Nadam: the schedule rebuilt from `iterations` alone)."""
    from jpeg_detection_resnet_ssd_amd.keras import optimizers as O
    opt, st = model.optimizer, model._store
    grads = st["grads"].cpu().numpy()
    want = {k: v.copy() for k, v in before.items()}
    twin = type(opt)(**opt.get_config())
    twin.iterations = iterations
    if isinstance(opt, O.RMSprop):
        host, scalars = O.rmsprop_host, (twin.current_lr(), twin.rho, twin.epsilon)
    elif isinstance(opt, O.Adagrad):
        host, scalars = O.adagrad_host, (twin.current_lr(), twin.epsilon)
    elif isinstance(opt, O.Adamax):
        host, scalars = O.adamax_host, (twin.step_size(), twin.beta_1, twin.beta_2, twin.epsilon)
    else:
        host, scalars = O.nadam_host, (twin.lr, twin.beta_1, twin.beta_2, twin.epsilon) + twin.step_scalars()
    names = ("p",) + opt.state_names
    for (a, b, l2) in st["segments"]:
        out = host(before["p"][a:b], grads[a:b], *[before[k][a:b] for k in opt.state_names], *scalars, l2, 1.0)
        for name, o in zip(names, out):
            want[name][a:b] = o
    return want


def _check_step(model, before, iterations, what):
    want = _statement_step(model, before, iterations)
    after = _snapshot(model)
    for name in ("p",) + model.optimizer.state_names:
        _same_bits(after[name], want[name], "%s: %s" % (what, name))
    assert not np.array_equal(after["p"], before["p"])
    return after


@pytest.mark.parametrize("which", RULE_NAMES)
def test_training_steps_apply_the_statement_to_the_engines_gradients(cuda, which):
    model = _model(_optimizers()[which]())
    x, y = _batch()
    model._ensure_params()
    st = model._store
    assert sorted(l2 for (_, _, l2) in st["segments"]) == [0.0, 5e-4, 1e-3] and st["flat"].numel() > st["n_train"]
    for step in range(2):
        before = _snapshot(model)
        if step == 0:
            assert all(not np.any(before[name]) for name in model.optimizer.state_names)     # allocated zeroed
        loss = model.train_on_batch(x, y)
        assert np.isfinite(loss) and model.optimizer.iterations == step + 1
        _check_step(model, before, step, "%s step %d" % (which, step))
        reg = sum(l2 * float(np.sum(before["p"][a:b].astype(np.float64) ** 2)) for (a, b, l2) in st["segments"])
        info = model.last_step_info
        assert info["reg_loss"] == pytest.approx(reg, rel=mc.sumsq_bound(st["n_train"], _gpp()) + 1e-12) and reg > 0
    # third step in pieces: the optimizer alone leaves the non-trainable state (the moving statistics) as it is
    plan = model._plan(BATCH, True, True)
    model._upload(plan, x, y)
    plan.run_forward()
    plan.run_backward()
    before = _snapshot(model)
    model._apply_optimizer(plan)
    after = _check_step(model, before, 2, which + " step 2")
    assert model.optimizer.iterations == 3
    _same_bits(after["rest"], before["rest"], "non-trainable state")


def test_float16_mode_moves_the_fp32_masters(cuda):
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    x, y = _batch()
    try:
        K.set_floatx("float16")
        model = _model(_optimizers()["nadam"]())
        model._ensure_params()
        before = _snapshot(model)
        loss = model.train_on_batch(x, y)
        assert np.isfinite(loss) and model._plan(BATCH, True, True).compute_mode == 1
        _check_step(model, before, 0, "nadam float16")
        st = model._store
        model._plan(BATCH, True, True).run_forward()    # the next forward pass refreshes the 16-bit shadows from the masters
        torch.cuda.synchronize()
        nt = st["n_train"]
        assert torch.equal(st["flat16"][:nt], st["flat"][:nt].to(torch.float16))
    finally:
        K.set_floatx("float32")


@pytest.mark.parametrize("which", RULE_NAMES)
def test_get_weights_into_a_fresh_model_goes_on_exactly(cuda, which):
    """Two steps, get_weights, a freshly built and compiled model, set_weights, two more steps there: each equals the
    statement applied, at the iteration count of the uninterrupted run, to the state the uninterrupted run had.  For Nadam
    nothing but `iterations` carries the momentum schedule across."""
    make = _optimizers()[which]
    model = _model(make())
    x, y = _batch()
    for _ in range(2):
        model.train_on_batch(x, y)
    opt, st = model.optimizer, model._store
    train = [w for w in model.weight_specs if w.trainable]
    weights = opt.get_weights()
    assert len(weights) == 1 + len(opt.state_names) * len(train)
    assert weights[0].dtype == np.int64 and weights[0].shape == () and int(weights[0]) == 2
    for i, name in enumerate(opt.state_names):
        buf = model._optimizer_buffer(name).cpu().numpy()
        assert np.any(buf != 0)
        for w, c in zip(train, weights[1 + i * len(train):1 + (i + 1) * len(train)]):
            a = st["offsets"][id(w)]
            assert c.shape == tuple(w.shape) and c.dtype == np.float32
            _same_bits(c.reshape(-1), buf[a:a + w.size], "%s of %s" % (name, w.key))
    twin = _model(make(), seed=6)
    twin.set_weights(model.get_weights())
    twin.optimizer.set_weights(weights)
    assert twin.optimizer.iterations == 2 and twin.optimizer is not opt
    for name in opt.state_names:
        _same_bits(twin._optimizer_buffer(name).cpu().numpy(), model._optimizer_buffer(name).cpu().numpy(), name)
    _same_bits(twin._store["flat"].cpu().numpy(), st["flat"].cpu().numpy())
    # the uninterrupted run's own third step would start from the same bits with the same entry point and scalars
    assert twin.optimizer.update_call(lambda name: name) == opt.update_call(lambda name: name)
    if which == "nadam":
        assert twin.optimizer.m_schedule == opt.m_schedule != 1.0
    for step in (2, 3):
        before = _snapshot(twin)
        twin.train_on_batch(x, y)
        _check_step(twin, before, step, "%s twin step %d" % (which, step))
    with pytest.raises(ValueError, match="Length of the specified weight list"):
        twin.optimizer.set_weights(weights[:-1])
    assert twin.optimizer.iterations == 4


def test_switching_optimizers_drops_the_old_state(cuda):
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import Adagrad, Adamax, Nadam, RMSprop
    model = _model(Adamax())
    x, y = _batch()
    model.train_on_batch(x, y)
    assert sorted(model._store["opt_state"]) == ["ms", "us"]
    assert all(float(model._optimizer_buffer(n).abs().sum()) > 0 for n in ("ms", "us"))
    model.compile(optimizer=Nadam(), loss="categorical_crossentropy")
    assert "opt_state" not in model._store
    before = _snapshot(model)
    assert not np.any(before["ms"]) and not np.any(before["vs"])        # Adamax' ms did not become Nadam's
    model.train_on_batch(x, y)
    _check_step(model, before, 0, "nadam after adamax")
    assert sorted(model._store["opt_state"]) == ["ms", "vs"]
    model.compile(optimizer=RMSprop(), loss="categorical_crossentropy")
    assert "opt_state" not in model._store
    model.train_on_batch(x, y)
    assert sorted(model._store["opt_state"]) == ["accumulators"]
    model.compile(optimizer=Adagrad(), loss="categorical_crossentropy")        # the same list name, another kind: zeroed too
    assert "opt_state" not in model._store
    before = _snapshot(model)
    assert not np.any(before["accumulators"])
    model.train_on_batch(x, y)
    _check_step(model, before, 0, "adagrad after rmsprop")
