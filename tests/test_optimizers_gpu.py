"""dj_sgd_momentum_update / dj_adam_update / dj_adadelta_update against the host statement (keras/optimizers.py), bit for bit, and the optimizers
behind Model.compile: sizes around the group of four and the tail, a size that takes the grid-stride loop round more than
once, a base pointer that is not 16-byte aligned, both scalar sets with and without l2 and grad_scale, amsgrad, three
chained steps, special values, the sum of squares, the argument checks, teacher-forced training steps of a small model
(the statement applied to the engine's own gradients), float16 mode, and get_weights / set_weights.

No test compares two training runs with each other: the weight-gradient GEMMs may accumulate with atomics."""
import numpy as np
import pytest
import torch

import optimizer_cases as oc

pytestmark = pytest.mark.gpu

GUARD = 7.0


def _lib():
    from jpeg_detection_resnet_ssd_amd import _lib
    return _lib.load()


def _gpp():
    return int(_lib().dj_optim_groups_per_pass())


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
        self.off, self.t = off, {}
        for name, a in arrays.items():
            if a is None:
                self.t[name] = None
                continue
            host = np.full(len(a) + off + 1, GUARD, np.float32)
            host[off:off + len(a)] = a
            full = torch.from_numpy(host).to(cuda)
            view = full[off:]
            assert (view.data_ptr() % 16 == 0) == (off == 0)
            self.t[name] = view

    def __getitem__(self, name):
        return self.t[name]

    def host(self, name, n):
        h = self.t[name].cpu().numpy()
        assert h[n] == GUARD, name + ": the element after the last was written"
        return h[:n]


def _adam_launch(b, n, lr_t, k, l2, scale, sumsq=None):
    from jpeg_detection_resnet_ssd_amd.engine import call
    call("dj_adam_update", b["p"], b["g"], b["m"], b["v"], b["vhat"], n, lr_t, k["beta_1"], k["beta_2"], k["epsilon"], l2, scale,
         sumsq)


def _adadelta_launch(b, n, lr, k, l2, scale, sumsq=None):
    from jpeg_detection_resnet_ssd_amd.engine import call
    call("dj_adadelta_update", b["p"], b["g"], b["a"], b["d"], n, lr, k["rho"], 1.0 - k["rho"], k["epsilon"], l2, scale, sumsq)


def _sgd_launch(b, n, lr_t, momentum, nesterov, l2, scale, sumsq=None):
    from jpeg_detection_resnet_ssd_amd.engine import call
    call("dj_sgd_momentum_update", b["p"], b["g"], b["v"], n, lr_t, momentum, int(nesterov), l2, scale, sumsq)


def _sgd_chain(cuda, n, kind, off, l2, scale, momentum, nesterov, p0, gs, steps=oc.STEPS):
    """The velocity starts from the last gradient, so that the first step already multiplies something."""
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import sgd_host
    lr = oc.SCALAR_SETS[kind]["sgd"]["lr_t"]
    b = Buffers(cuda, off, p=p0, g=gs[0], v=gs[-1])
    p, v = p0, gs[-1]
    for t in range(steps):
        if t:
            b["g"][:n].copy_(torch.from_numpy(gs[t]))
        _sgd_launch(b, n, lr[t], momentum, nesterov, l2, scale)
        p, v = sgd_host(p, gs[t], v, lr[t], momentum, nesterov, l2, scale)
        what = "sgd n=%d %s off=%d l2=%g scale=%g momentum=%g nesterov=%d step %d: " % (n, kind, off, l2, scale, momentum,
                                                                                      nesterov, t)
        _same_bits(b.host("p", n), p, what + "p")
        _same_bits(b.host("v", n), v, what + "v")
        _same_bits(b.host("g", n), gs[t], what + "g")


def _adam_chain(cuda, n, kind, off, l2, scale, amsgrad, p0, gs):
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import adam_host
    k = oc.SCALAR_SETS[kind]["adam"]
    z = np.zeros(n, np.float32)
    b = Buffers(cuda, off, p=p0, g=gs[0], m=z, v=z, vhat=z if amsgrad else None)
    p, m, v, vhat = p0, z, z, (z if amsgrad else None)
    for t in range(oc.STEPS):
        if t:
            b["g"][:n].copy_(torch.from_numpy(gs[t]))
        _adam_launch(b, n, k["lr_t"][t], k, l2, scale)
        p, m, v, vhat = adam_host(p, gs[t], m, v, vhat, k["lr_t"][t], k["beta_1"], k["beta_2"], k["epsilon"], l2, scale)
        what = "adam n=%d %s off=%d l2=%g scale=%g amsgrad=%d step %d: " % (n, kind, off, l2, scale, amsgrad, t)
        _same_bits(b.host("p", n), p, what + "p")
        _same_bits(b.host("m", n), m, what + "m")
        _same_bits(b.host("v", n), v, what + "v")
        if amsgrad:
            _same_bits(b.host("vhat", n), vhat, what + "vhat")
        _same_bits(b.host("g", n), gs[t], what + "g")                   # the gradient is left alone


def _adadelta_chain(cuda, n, kind, off, l2, scale, p0, gs):
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import adadelta_host
    k = oc.SCALAR_SETS[kind]["adadelta"]
    z = np.zeros(n, np.float32)
    b = Buffers(cuda, off, p=p0, g=gs[0], a=z, d=z)
    p, a, d = p0, z, z
    for t in range(oc.STEPS):
        if t:
            b["g"][:n].copy_(torch.from_numpy(gs[t]))
        _adadelta_launch(b, n, k["lr"][t], k, l2, scale)
        p, a, d = adadelta_host(p, gs[t], a, d, k["lr"][t], k["rho"], k["epsilon"], l2, scale)
        what = "adadelta n=%d %s off=%d l2=%g scale=%g step %d: " % (n, kind, off, l2, scale, t)
        _same_bits(b.host("p", n), p, what + "p")
        _same_bits(b.host("a", n), a, what + "a")
        _same_bits(b.host("d", n), d, what + "d")
        _same_bits(b.host("g", n), gs[t], what + "g")


@pytest.mark.parametrize("n", oc.SIZES)
def test_kernels_equal_the_host_statement(cuda, n):
    for kind, sc in oc.SCALAR_SETS.items():
        p0, gs = oc.inputs(n, kind)
        for off in (0, 1):                  # off 1: no pointer is 16-byte aligned, so the 16-byte path must fall back
            for l2 in sc["l2"]:
                for scale in sc["grad_scale"]:
                    for amsgrad in (False, True):
                        _adam_chain(cuda, n, kind, off, l2, scale, amsgrad, p0, gs)
                    _adadelta_chain(cuda, n, kind, off, l2, scale, p0, gs)
                    for momentum in sc["sgd"]["momentum"]:
                        for nesterov in (False, True):
                            _sgd_chain(cuda, n, kind, off, l2, scale, momentum, nesterov, p0, gs)


def test_several_passes_of_the_capped_grid(cuda):
    n = oc.several_passes(_gpp())
    assert oc.terms_per_thread(n, _gpp()) > 4
    p0, gs = oc.inputs(n, "normal")
    _adam_chain(cuda, n, "normal", 0, 5e-4, 0.125, True, p0, gs)
    _adadelta_chain(cuda, n, "normal", 0, 5e-4, 0.125, p0, gs)


def test_several_passes_of_the_capped_grid_sgd(cuda):
    """One step of each of the six configurations of optimizer_cases.SGD_FEW, on the 16-byte path."""
    n = oc.several_passes(_gpp())
    sc = oc.SCALAR_SETS["normal"]
    p0, gs = oc.inputs(n, "normal")
    for nesterov, a, b, c in oc.SGD_FEW:
        _sgd_chain(cuda, n, "normal", 0, sc["l2"][b], sc["grad_scale"][c], sc["sgd"]["momentum"][a], nesterov, p0, gs, steps=1)


def test_a_single_misaligned_pointer_takes_the_fallback(cuda):
    """Only the state buffers are offset: the launcher must look at every pointer."""
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import adadelta_host, adam_host, sgd_host
    n = 1021
    p0, gs = oc.inputs(n, "normal")
    for odd in ("v", "p", "g"):
        for nesterov in (False, True):
            b = Buffers(cuda, 0, p=p0, g=gs[0], v=gs[1])
            b.t[odd] = Buffers(cuda, 1, x=dict(p=p0, g=gs[0], v=gs[1])[odd])["x"]
            _sgd_launch(b, n, 0.1, 0.9, nesterov, 5e-4, 1.0)
            for name, w in zip(("p", "v"), sgd_host(p0, gs[0], gs[1], 0.1, 0.9, nesterov, 5e-4, 1.0)):
                _same_bits(b.host(name, n), w, "sgd, %s offset: %s" % (odd, name))
    k = oc.SCALAR_SETS["normal"]["adam"]
    z = np.zeros(n, np.float32)
    for odd in ("p", "g", "m", "v", "vhat"):
        b = Buffers(cuda, 0, p=p0, g=gs[0], m=z, v=z, vhat=z)
        b.t[odd] = Buffers(cuda, 1, x=dict(p=p0, g=gs[0]).get(odd, z))["x"]
        _adam_launch(b, n, k["lr_t"][0], k, 5e-4, 1.0)
        want = adam_host(p0, gs[0], z, z, z, k["lr_t"][0], k["beta_1"], k["beta_2"], k["epsilon"], 5e-4, 1.0)
        for name, w in zip(("p", "m", "v", "vhat"), want):
            _same_bits(b.host(name, n), w, odd + " offset: " + name)
    k = oc.SCALAR_SETS["normal"]["adadelta"]
    for odd in ("p", "g", "a", "d"):
        b = Buffers(cuda, 0, p=p0, g=gs[0], a=z, d=z)
        b.t[odd] = Buffers(cuda, 1, x=dict(p=p0, g=gs[0]).get(odd, z))["x"]
        _adadelta_launch(b, n, k["lr"][0], k, 5e-4, 1.0)
        want = adadelta_host(p0, gs[0], z, z, k["lr"][0], k["rho"], k["epsilon"], 5e-4, 1.0)
        for name, w in zip(("p", "a", "d"), want):
            _same_bits(b.host(name, n), w, odd + " offset: " + name)


def test_special_values(cuda):
    """g = 0 on zero state, +-Inf, NaN, p = Inf with l2 = 0, gradients whose square is a float32 denormal, signed zeros and
    a large second moment: whatever the statement gives (checked by hand in tests/test_optimizers_cpu.py), bit for bit."""
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import adadelta_host, adam_host, sgd_host
    p0, g, second = oc.special_inputs()
    n = len(p0)
    z = np.zeros(n, np.float32)
    for off in (0, 1):
        for nesterov in (False, True):
            b = Buffers(cuda, off, p=p0, g=g, v=second)
            _sgd_launch(b, n, 0.1, 0.9, nesterov, 0.0, 1.0)
            want = sgd_host(p0, g, second, 0.1, 0.9, nesterov, 0.0, 1.0)
            assert want[0][0] == p0[0] and np.isinf(want[0][1:3]).all() and np.isnan(want[0][3:5]).all()
            for name, w in zip(("p", "v"), want):
                _same_bits(b.host(name, n), w, "sgd special values off=%d nesterov=%d: %s" % (off, nesterov, name))
    k = oc.SCALAR_SETS["normal"]["adam"]
    assert 0 < np.float32(1e-20) * np.float32(1e-20) < np.finfo(np.float32).tiny
    for off in (0, 1):
        for amsgrad in (False, True):
            b = Buffers(cuda, off, p=p0, g=g, m=z, v=second, vhat=second if amsgrad else None)
            _adam_launch(b, n, k["lr_t"][0], k, 0.0, 1.0)
            want = adam_host(p0, g, z, second, second if amsgrad else None, k["lr_t"][0], k["beta_1"], k["beta_2"], k["epsilon"],
                             0.0, 1.0)
            assert want[0][0] == p0[0] and np.isnan(want[0][1:5]).all() and np.isfinite(want[0][5:]).all()
            assert want[2][5] > 0 and want[2][5] < np.finfo(np.float32).tiny         # a denormal second moment survives
            for name, w in zip(("p", "m", "v", "vhat"), want):
                if w is not None:
                    _same_bits(b.host(name, n), w, "adam special values off=%d amsgrad=%d: %s" % (off, amsgrad, name))
        kd = oc.SCALAR_SETS["normal"]["adadelta"]
        b = Buffers(cuda, off, p=p0, g=g, a=second, d=z)
        _adadelta_launch(b, n, 1.0, kd, 0.0, 1.0)
        want = adadelta_host(p0, g, second, z, 1.0, kd["rho"], kd["epsilon"], 0.0, 1.0)
        assert want[0][0] == p0[0] and np.isnan(want[0][1:5]).all() and np.isfinite(want[0][5:]).all()
        for name, w in zip(("p", "a", "d"), want):
            _same_bits(b.host(name, n), w, "adadelta special values off=%d: %s" % (off, name))


@pytest.mark.parametrize("n", [5, 1021, "several passes"])
def test_sum_of_squares(cuda, n):
    """sumsq[0] += sum(p^2) of the parameters BEFORE the update, within the bound of the kernel's own summation tree
    (optimizer_cases.sumsq_bound); the updates do not depend on whether it is asked for."""
    n = oc.several_passes(_gpp()) if n == "several passes" else n
    p0, gs = oc.inputs(n, "normal", seed=8)
    z = np.zeros(n, np.float32)
    start = 3.25
    exact = start + float(np.sum(p0.astype(np.float64) ** 2))
    bound = oc.sumsq_bound(n, _gpp())
    ka, kd = oc.SCALAR_SETS["normal"]["adam"], oc.SCALAR_SETS["normal"]["adadelta"]
    for off in (0, 1):
        for amsgrad in (False, True):
            got = []
            for with_sum in (True, False):
                b = Buffers(cuda, off, p=p0, g=gs[0], m=z, v=z, vhat=z if amsgrad else None)
                ss = torch.full((3,), start, device=cuda)
                _adam_launch(b, n, ka["lr_t"][0], ka, 5e-4, 1.0, ss[1:2] if with_sum else None)
                ssh = ss.cpu().numpy()
                assert ssh[0] == start and ssh[2] == start
                if with_sum:
                    print("adam n=%d off=%d: sumsq relative error %.3g, bound %.3g" % (n, off, abs(float(ssh[1]) - exact) / exact, bound))
                    assert abs(float(ssh[1]) - exact) <= bound * exact
                else:
                    assert ssh[1] == start
                got.append([b.host(name, n) for name in ("p", "m", "v") + (("vhat",) if amsgrad else ())])
            for x, y in zip(*got):
                _same_bits(x, y, "with and without sumsq")
        for which in ("sgd", "sgd nesterov"):
            got = []
            for with_sum in (True, False):
                b = Buffers(cuda, off, p=p0, g=gs[0], v=gs[1])
                ss = torch.full((3,), start, device=cuda)
                _sgd_launch(b, n, 0.1, 0.9, which != "sgd", 5e-4, 1.0, ss[1:2] if with_sum else None)
                ssh = ss.cpu().numpy()
                assert ssh[0] == start and ssh[2] == start
                if with_sum:
                    print("%s n=%d off=%d: sumsq relative error %.3g, bound %.3g" % (which, n, off, abs(float(ssh[1]) - exact) / exact, bound))
                    assert abs(float(ssh[1]) - exact) <= bound * exact
                else:
                    assert ssh[1] == start
                got.append([b.host(name, n) for name in ("p", "v")])
            for x, y in zip(*got):
                _same_bits(x, y, "with and without sumsq")
        got = []
        for with_sum in (True, False):
            b = Buffers(cuda, off, p=p0, g=gs[0], a=z, d=z)
            ss = torch.full((3,), start, device=cuda)
            _adadelta_launch(b, n, 1.0, kd, 5e-4, 1.0, ss[1:2] if with_sum else None)
            ssh = ss.cpu().numpy()
            assert ssh[0] == start and ssh[2] == start
            if with_sum:
                print("adadelta n=%d off=%d: sumsq relative error %.3g, bound %.3g" % (n, off, abs(float(ssh[1]) - exact) / exact, bound))
                assert abs(float(ssh[1]) - exact) <= bound * exact
            got.append([b.host(name, n) for name in ("p", "a", "d")])
        for x, y in zip(*got):
            _same_bits(x, y, "with and without sumsq")


def test_sum_of_squares_slots_are_clean_after_many_launches(cuda):
    """More launches than the library has accumulator slots, SGD's among Adam's (the slots are shared): each leaves its
    slot cleared for the next user."""
    n = 1021
    p0, gs = oc.inputs(n, "normal", seed=8)
    z = np.zeros(n, np.float32)
    ka = oc.SCALAR_SETS["normal"]["adam"]
    b = Buffers(cuda, 0, p=p0, g=gs[0], m=z, v=z, vhat=None)
    ss = torch.zeros(80, device=cuda)
    for i in range(80):
        if i % 3 == 1:
            _sgd_launch(b, n, 0.0, 0.9, False, 0.0, 0.0, ss[i:i + 1])    # on v = 0: the velocity stays 0 and p what it is
        else:
            _adam_launch(b, n, 0.0, ka, 0.0, 0.0, ss[i:i + 1])          # lr_t = 0, grad_scale = 0: p stays what it is
    ssh = ss.cpu().numpy()
    _same_bits(b.host("p", n), p0)
    assert np.all(ssh == ssh[0])
    exact = float(np.sum(p0.astype(np.float64) ** 2))
    assert abs(float(ssh[0]) - exact) <= oc.sumsq_bound(n, _gpp()) * exact


def test_argument_checks_launch_nothing(cuda):
    lib = _lib()
    n = 64
    p0, gs = oc.inputs(n, "normal")
    z = np.zeros(n, np.float32)
    sa, sd = (0.001, 0.9, 0.999, 1e-7, 0.0, 1.0), (1.0, 0.95, 0.05, 1e-7, 0.0, 1.0)
    stream = torch.cuda.current_stream().cuda_stream
    b = Buffers(cuda, 0, p=p0, g=gs[0], m=z, v=z, vhat=z, ss=np.zeros(1, np.float32))
    P, G, M, V, H, S = (b[k].data_ptr() for k in ("p", "g", "m", "v", "vhat", "ss"))
    bad_adam = [(None, G, M, V, H, n), (P, None, M, V, H, n), (P, G, None, V, H, n), (P, G, M, None, H, n), (P, G, M, V, H, 0),
                (P, G, P, V, H, n), (P, G, M, P, H, n), (P, G, M, V, P, n), (P, G, M, M + 4 * (n - 1), None, n)]
    for args in bad_adam:
        assert lib.dj_adam_update(*args, *sa, S, stream) == -1, args
        assert len(lib.dj_last_error()) > 10
    bad_adadelta = [(None, G, M, V, n), (P, None, M, V, n), (P, G, None, V, n), (P, G, M, None, n), (P, G, M, V, 0),
                    (P, G, P, V, n), (P, G, M, P, n), (P, G, M, M, n)]
    for args in bad_adadelta:
        assert lib.dj_adadelta_update(*args, *sd, S, stream) == -1, args
        assert len(lib.dj_last_error()) > 10
    ssgd = (0.1, 0.9, 1, 5e-4, 1.0)
    bad_sgd = [(None, G, V, n), (P, None, V, n), (P, G, None, n), (P, G, V, 0),
               (P, G, P, n), (P, P, V, n), (P, G, P + 4 * (n - 1), n), (P, P - 4 * (n - 1), V, n), (P, G, G, n)]
    for args in bad_sgd:
        assert lib.dj_sgd_momentum_update(*args, *ssgd, S, stream) == -1, args
        assert b"dj_sgd_momentum_update" in lib.dj_last_error()
    torch.cuda.synchronize()
    for name, want in (("p", p0), ("g", gs[0]), ("m", z), ("v", z), ("vhat", z), ("ss", np.zeros(1, np.float32))):
        _same_bits(b.host(name, len(want)), want, name + " after refused calls")


# ----------------------------------------------------------------------------------------------------------------------
# model level
# ----------------------------------------------------------------------------------------------------------------------
N_CLASSES, BATCH = 6, 8


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


def _state_names(opt):
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import Adam
    if isinstance(opt, Adam):
        return ("ms", "vs") + (("vhats",) if opt.amsgrad else ())
    return ("accumulators", "delta_accumulators")


def _snapshot(model):
    st = model._store
    torch.cuda.synchronize()
    snap = dict(p=st["flat"][:st["n_train"]].cpu().numpy().copy(), rest=st["flat"][st["n_train"]:].cpu().numpy().copy())
    for name in _state_names(model.optimizer):
        snap[name] = model._optimizer_buffer(name).cpu().numpy().copy()
    return snap


def _statement_step(model, before, iterations):
    """The host statement applied per segment to the engine's own gradients and the state captured before the step, with
    the scalars of a fresh optimizer object at `iterations`."""
    from jpeg_detection_resnet_ssd_amd.keras import optimizers as O
    opt, st = model.optimizer, model._store
    grads = st["grads"].cpu().numpy()
    want = {k: v.copy() for k, v in before.items()}
    twin = type(opt)(**opt.get_config())
    twin.iterations = iterations
    for (a, b, l2) in st["segments"]:
        if isinstance(opt, O.Adam):
            vhat = before["vhats"][a:b] if opt.amsgrad else None
            out = O.adam_host(before["p"][a:b], grads[a:b], before["ms"][a:b], before["vs"][a:b], vhat, twin.step_size(),
                              twin.beta_1, twin.beta_2, twin.epsilon, l2, 1.0)
            names = ("p", "ms", "vs", "vhats")
        else:
            out = O.adadelta_host(before["p"][a:b], grads[a:b], before["accumulators"][a:b], before["delta_accumulators"][a:b],
                                  twin.current_lr(), twin.rho, twin.epsilon, l2, 1.0)
            names = ("p", "accumulators", "delta_accumulators")
        for name, o in zip(names, out):
            if o is not None:
                want[name][a:b] = o
    return want


def _check_step(model, before, iterations, what):
    want = _statement_step(model, before, iterations)
    after = _snapshot(model)
    for name in ("p",) + _state_names(model.optimizer):
        _same_bits(after[name], want[name], "%s: %s" % (what, name))
    assert not np.array_equal(after["p"], before["p"])
    return after


def _optimizers():
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import Adadelta, Adam
    return {"adam": lambda: Adam(lr=1e-3, decay=1e-4, amsgrad=True), "adadelta": lambda: Adadelta(decay=1e-4)}


@pytest.mark.parametrize("which", ["adam", "adadelta"])
def test_training_steps_apply_the_statement_to_the_engines_gradients(cuda, which):
    model = _model(_optimizers()[which]())
    x, y = _batch()
    model._ensure_params()
    st = model._store
    l2s = sorted(l2 for (_, _, l2) in st["segments"])
    assert l2s == [0.0, 5e-4, 1e-3] and st["flat"].numel() > st["n_train"]
    for step in range(2):
        before = _snapshot(model)
        loss = model.train_on_batch(x, y)
        assert model.optimizer.iterations == step + 1
        _check_step(model, before, step, "%s step %d" % (which, step))
        # the reported loss: data loss + sum over the segments of l2 * sum(p^2) of the parameters the step started from
        reg = sum(l2 * float(np.sum(before["p"][a:b].astype(np.float64) ** 2)) for (a, b, l2) in st["segments"])
        info = model.last_step_info
        assert info["reg_loss"] == pytest.approx(reg, rel=oc.sumsq_bound(st["n_train"], _gpp()) + 1e-12) and reg > 0
        assert loss == pytest.approx(info["data_loss"] + info["reg_loss"], rel=1e-12)
        assert loss == pytest.approx(float(model._plan(BATCH, True, True).loss_out[0]) + reg, rel=1e-6)
    # third step in pieces: the optimizer alone leaves the non-trainable state (the moving statistics) as it is
    plan = model._plan(BATCH, True, True)
    model._upload(plan, x, y)
    plan.run_forward()
    plan.run_backward()
    before = _snapshot(model)
    assert not np.array_equal(before["rest"], np.zeros_like(before["rest"]))
    model._apply_optimizer(plan)
    after = _check_step(model, before, 2, which + " step 2")
    assert model.optimizer.iterations == 3
    _same_bits(after["rest"], before["rest"], "non-trainable state")


def test_float16_mode_moves_the_fp32_masters_and_refreshes_the_shadows(cuda):
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    x, y = _batch()
    try:
        K.set_floatx("float16")
        for which, make in _optimizers().items():
            model = _model(make())
            model._ensure_params()
            before = _snapshot(model)
            loss = model.train_on_batch(x, y)
            assert np.isfinite(loss) and model._plan(BATCH, True, True).compute_mode == 1
            _check_step(model, before, 0, which + " float16")
            st = model._store
            assert "flat16" in st
            stale = st["flat16"][:st["n_train"]].float().cpu().numpy()
            assert not np.array_equal(stale, st["flat"][:st["n_train"]].half().float().cpu().numpy())   # refreshed per pass
            model._plan(BATCH, True, True).run_forward()    # the next forward pass
            torch.cuda.synchronize()
            nt = st["n_train"]          # past it lie the moving statistics, which that forward pass itself went on to update
            assert torch.equal(st["flat16"][:nt], st["flat"][:nt].to(torch.float16))
            assert torch.equal(st["flatbf"][:nt], st["flat"][:nt].to(torch.bfloat16))
    finally:
        K.set_floatx("float32")


@pytest.mark.parametrize("which", ["adam", "adam without amsgrad", "adadelta", "sgd"])
def test_get_weights_and_set_weights(cuda, which):
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import SGD, Adam
    make = dict(_optimizers(), **{"adam without amsgrad": lambda: Adam(lr=1e-3), "sgd": lambda: SGD(lr=0.01, momentum=0.9)})[which]
    model = _model(make())
    x, y = _batch()
    for _ in range(2):
        model.train_on_batch(x, y)
    opt, st = model.optimizer, model._store
    train = [w for w in model.weight_specs if w.trainable]
    weights = opt.get_weights()
    lists = {"adam": ("ms", "vs", "vhats"), "adam without amsgrad": ("ms", "vs", "vhats"),
             "adadelta": ("accumulators", "delta_accumulators"), "sgd": ("moments",)}[which]
    assert len(weights) == 1 + len(lists) * len(train)
    assert weights[0].dtype == np.int64 and weights[0].shape == () and int(weights[0]) == 2
    for i, name in enumerate(lists):
        chunk = weights[1 + i * len(train):1 + (i + 1) * len(train)]
        if which == "adam without amsgrad" and name == "vhats":
            assert all(c.shape == (1,) and c[0] == 0 for c in chunk)          # Keras 2.2.4's placeholders
            continue
        buf = model._optimizer_buffer(name).cpu().numpy()
        assert np.any(buf != 0)
        for w, c in zip(train, chunk):
            a = st["offsets"][id(w)]
            assert c.shape == tuple(w.shape) and c.dtype == np.float32
            _same_bits(c.reshape(-1), buf[a:a + w.size], "%s of %s" % (name, w.key))
    # a freshly built and compiled twin takes the weights and the optimizer state, and goes on exactly
    twin = _model(make(), seed=6)
    twin.set_weights(model.get_weights())
    twin.optimizer.set_weights(weights)
    assert twin.optimizer.iterations == 2
    for name in lists:
        if not (which == "adam without amsgrad" and name == "vhats"):
            _same_bits(twin._optimizer_buffer(name).cpu().numpy(), model._optimizer_buffer(name).cpu().numpy(), name)
    _same_bits(twin._store["flat"].cpu().numpy(), st["flat"].cpu().numpy())
    if which != "sgd":
        before = _snapshot(twin)
        twin.train_on_batch(x, y)
        _check_step(twin, before, 2, which + " twin")
    # Keras' errors
    with pytest.raises(ValueError, match=r"Length of the specified weight list \(%d\) does not match the number of weights of "
                                         r"the optimizer \(%d\)" % (len(weights) - 1, len(weights))):
        twin.optimizer.set_weights(weights[:-1])
    wrong = list(weights)
    wrong[1] = np.zeros(wrong[1].shape + (2,), np.float32)
    with pytest.raises(ValueError, match="Optimizer weight shape .* not compatible with provided weight shape"):
        twin.optimizer.set_weights(wrong)
    assert twin.optimizer.iterations == 3 if which != "sgd" else twin.optimizer.iterations == 2      # refused before any write


def test_switching_optimizers_starts_from_zeroed_state(cuda):
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import SGD, Adam
    model = _model(Adam(amsgrad=True))
    x, y = _batch()
    model.train_on_batch(x, y)
    assert all(float(model._optimizer_buffer(n).abs().sum()) > 0 for n in ("ms", "vs", "vhats"))
    model.compile(optimizer=SGD(lr=0.01, momentum=0.9), loss="categorical_crossentropy")
    assert "opt_state" not in model._store and float(model._store["vel"].abs().sum()) == 0
    model.train_on_batch(x, y)
    assert float(model._store["vel"].abs().sum()) > 0
    model.compile(optimizer=Adam(amsgrad=True), loss="categorical_crossentropy")
    assert float(model._store["vel"].abs().sum()) == 0
    assert all(float(model._optimizer_buffer(n).abs().sum()) == 0 for n in ("ms", "vs", "vhats"))
    before = _snapshot(model)
    model.train_on_batch(x, y)
    _check_step(model, before, 0, "adam after sgd")
