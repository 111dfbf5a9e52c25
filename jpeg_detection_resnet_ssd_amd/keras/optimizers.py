"""keras.optimizers.SGD, Adam (with amsgrad), Adadelta, RMSprop, Adagrad, Adamax and Nadam with the Keras 2.2.4 update rules.

SGD (differs from torch.optim.SGD whenever the learning rate changes): lr_t = lr / (1 + decay * iterations);
v = momentum*v - lr_t*g; p += v  (or p += momentum*v - lr_t*g with nesterov=True).
Call sites: localisation_part/training_dct_pascal_j2d_resnet.py:152,
classification_part/config/resnet/config_file.py:58-63.
Adam and Adadelta.  Call sites: localisation_part/evaluation.py:102 and inference.py:104 (Adam(lr=0.001, beta_1=0.9,
beta_2=0.999, epsilon=1e-08, decay=0.0)); classification_part/template_keras/config/template_config.py (Adadelta).

Keras is not a dependency: `sgd_host`, `adam_host`, `adadelta_host` and the four `*_host` after them below are the statement
of the rules, in numpy, and csrc/dj_optim.hip equals them bit for bit.  All tensor arithmetic is float32; every product, sum, quotient and square
root is rounded once, in the order written (fl); nothing is fused but the two fma of SGD, which round a*b + c once.
grad_scale is the data-parallel 1/world and l2 the segment's kernel_regularizer (in Keras the penalty is part of the loss,
so it enters the moments; 0 for un-regularised segments -- a product all the same, so p = Inf gives NaN).

SGD (the roundings are those of the kernel SGD had before it was stated here, which its compiler chose; l2 + l2 is exact):

    t   = fl( fl32(l2 + l2) * p )
    g'  = fma(g, grad_scale, t)
    v   = fl( fl(momentum * v) - fl(lr_t * g') )
    p   = fl( fma(momentum, v, p) - fl(lr_t * g') )  with nesterov,  else  fl(p + v)

with lr_t = lr / (1 + decay * iterations) in Python float64 (SGD.current_lr()), rounded once to float32 by the caller.

Adam and Adadelta share an effective gradient that, unlike SGD's g', rounds both products:

    g' = fl( fl(g * grad_scale) + fl( fl32(2*l2) * p ) )

Adam (Keras holds the betas as float32 variables, so 1 - beta is a float32 subtraction):

    omb1 = fl32(1) - fl32(beta_1);  omb2 = fl32(1) - fl32(beta_2)
    m  = fl(fl(b1 * m) + fl(omb1 * g'))
    v  = fl(fl(b2 * v) + fl(omb2 * fl(g' * g')))
    amsgrad:  vhat = max(vhat, v)  (np.maximum: NaN in either gives NaN);  d = vhat     else  d = v
    p  = fl(p - fl( fl(lr_t * m) / fl(sqrt(d) + eps) ))

with, in Python float64 and rounded once to float32 by the caller,

    lr_dec = lr / (1 + decay * iterations) if decay > 0 else lr          (Adam.current_lr())
    t = iterations + 1
    lr_t = lr_dec * sqrt(1 - beta_2**t) / (1 - beta_1**t)                (Adam.step_size())

Adadelta (rho is a Python float in Keras: 1 - rho is subtracted in float64 and rounded once):

    omr = fl32(1.0 - rho)
    a   = fl(fl(rho * a) + fl(omr * fl(g' * g')))
    u   = fl( fl(g' * fl(sqrt(fl(d + eps)))) / fl(sqrt(fl(a + eps))) )
    p   = fl(p - fl(lr_dec * u))
    d   = fl(fl(rho * d) + fl(omr * fl(u * u)))

RMSprop, Adagrad, Adamax and Nadam (Keras 2.2.4's get_updates; rmsprop_host, adagrad_host, adamax_host, nadam_host; no call
site in the reference, they complete keras.optimizers) take the same g'.  Their scalars are computed in Python float64 and
rounded once to float32 at the call, as lr_t above; Keras computes some of them (lr_dec, lr_t, the Nadam schedule and bias
corrections) in float32 tensor arithmetic, so its last bits may differ.  Keras is not installed here: this module, not
Keras, is the contract.

RMSprop (rho is a float32 variable in Keras, so 1 - rho is a float32 subtraction):

    omr = fl32(1) - fl32(rho)
    a   = fl(fl(rho * a) + fl(omr * fl(g' * g')))
    p   = fl(p - fl( fl(lr_dec * g') / fl(sqrt(a) + eps) ))

Adagrad:

    a   = fl(a + fl(g' * g'))
    p   = fl(p - fl( fl(lr_dec * g') / fl(sqrt(a) + eps) ))

Adamax (omb1 as Adam's; no square root: u is the exponentially weighted infinity norm):

    m   = fl(fl(b1 * m) + fl(omb1 * g'))
    u   = max(fl(b2 * u), |g'|)          (np.maximum: NaN in either gives NaN)
    p   = fl(p - fl( fl(lr_t * m) / fl(u + eps) ))        lr_t = lr_dec / (1 - beta_1**t)        (Adamax.step_size())

Nadam (no decay argument).  The momentum schedule, in float64 (Nadam.step_scalars()):

    mc(i)   = beta_1 * (1 - 0.5 * 0.96**(i * schedule_decay))
    ms_new  = m_schedule * mc(t);   ms_next = ms_new * mc(t + 1);   m_schedule = mc(1) * ... * mc(iterations)
    c_g = 1 / (1 - ms_new);   c_m = 1 / (1 - ms_next);   c_v = 1 / (1 - beta_2**t);   omc_t = 1 - mc(t);   mc_t1 = mc(t + 1)

each rounded once to float32, then

    m    = fl(fl(b1 * m) + fl(omb1 * g'))
    v    = fl(fl(b2 * v) + fl(omb2 * fl(g' * g')))
    mbar = fl( fl(omc_t * fl(g' * c_g)) + fl(mc_t1 * fl(m * c_m)) )
    p    = fl(p - fl( fl(lr * mbar) / fl(sqrt(fl(v * c_v)) + eps) ))

A departure from Keras: where Keras divides g', m and v by (1 - ms_new), (1 - ms_next) and (1 - beta_2**t), the statement
and the kernel multiply by the reciprocals c_g, c_m and c_v.  Keras keeps m_schedule as a variable; here it is a function
of `iterations` alone (Nadam.m_schedule, cached per step), so restoring `iterations` restores it and get_weights() has
no entry for it.

epsilon=None means K.epsilon() = 1e-7.  clipnorm / clipvalue are not implemented and raise.  Model.compile takes the
seven classes as instances; by name only 'sgd', as before (see `get`).

Optimizer state.  `get_weights()` / `set_weights()` work once the optimizer is compiled into a model, and return / accept
numpy arrays in Keras' order, the per-weight arrays in the order of the model's trainable weights and shaped like them:
SGD [iterations] + moments;  Adam [iterations] + ms + vs + vhats;  Adadelta [iterations] + accumulators + delta_accumulators;
RMSprop and Adagrad [iterations] + accumulators;  Adamax [iterations] + ms + us;  Nadam [iterations] + ms + vs.
`iterations` is an int64 scalar.  Without amsgrad Keras 2.2.4 keeps every vhat as one zeros(1): so does this list, so that
its length is what a Keras user expects; set_weights checks those entries' shape and otherwise ignores them."""
import math
import weakref

import numpy as np

EPSILON = 1e-7      # K.epsilon()


def _f32(x):
    return np.float32(x)


def effective_gradient_host(p, g, l2, grad_scale):
    """g' of the module docstring, float32."""
    p, g = np.asarray(p, np.float32), np.asarray(g, np.float32)
    with np.errstate(all="ignore"):
        return g * _f32(grad_scale) + (_f32(2.0) * _f32(l2)) * p


def fma32(a, b, c):
    """fl32(a*b + c) of float32 operands, rounded once.  The float64 product of two float32 is exact; TwoSum gives the
    float64 sum s and its exact error; where the sum is inexact s is moved to its odd neighbour on the side of the error
    (round to odd), after which the rounding to float32 cannot go wrong.  (fl32 of the float64 a*b + c rounds twice.)"""
    a, b, c = (np.asarray(t, np.float32).astype(np.float64) for t in (a, b, c))
    with np.errstate(all="ignore"):
        x = a * b
        s = np.asarray(x + c)
        t = s - x
        err = (x - (s - t)) + (c - t)
        even = (s.view(np.int64) & 1) == 0
        odd_neighbour = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        return np.where(np.isfinite(s) & (err != 0) & even, odd_neighbour, s).astype(np.float32)


def sgd_host(p, g, v, lr_t, momentum, nesterov, l2, grad_scale):
    """One SGD step as the module docstring states it -> (p, v)."""
    p, g, v = (np.asarray(t, np.float32) for t in (p, g, v))
    lr_t, momentum = _f32(lr_t), _f32(momentum)
    with np.errstate(all="ignore"):
        ge = fma32(g, _f32(grad_scale), (_f32(l2) + _f32(l2)) * p)
        step = lr_t * ge
        v = momentum * v - step
        p = fma32(momentum, v, p) - step if nesterov else p + v
    assert p.dtype == v.dtype == np.float32
    return p, v


def adam_host(p, g, m, v, vhat, lr_t, beta_1, beta_2, epsilon, l2, grad_scale):
    """One Adam step as the module docstring states it -> (p, m, v, vhat); vhat None = no amsgrad (None is returned)."""
    p, m, v = (np.asarray(t, np.float32) for t in (p, m, v))
    b1, b2, one = _f32(beta_1), _f32(beta_2), _f32(1.0)
    omb1, omb2 = one - b1, one - b2
    with np.errstate(all="ignore"):
        ge = effective_gradient_host(p, g, l2, grad_scale)
        m = b1 * m + omb1 * ge
        v = b2 * v + omb2 * (ge * ge)
        if vhat is not None:
            vhat = np.maximum(np.asarray(vhat, np.float32), v)
            d = vhat
        else:
            d = v
        p = p - (_f32(lr_t) * m) / (np.sqrt(d) + _f32(epsilon))
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v, vhat


def adadelta_host(p, g, a, d, lr_dec, rho, epsilon, l2, grad_scale):
    """One Adadelta step as the module docstring states it -> (p, accumulator, delta_accumulator)."""
    p, a, d = (np.asarray(t, np.float32) for t in (p, a, d))
    omr, rho, eps = _f32(1.0 - float(rho)), _f32(rho), _f32(epsilon)
    with np.errstate(all="ignore"):
        ge = effective_gradient_host(p, g, l2, grad_scale)
        a = rho * a + omr * (ge * ge)
        u = (ge * np.sqrt(d + eps)) / np.sqrt(a + eps)
        p = p - _f32(lr_dec) * u
        d = rho * d + omr * (u * u)
    assert p.dtype == a.dtype == d.dtype == np.float32
    return p, a, d


def rmsprop_host(p, g, a, lr_dec, rho, epsilon, l2, grad_scale):
    """One RMSprop step as the module docstring states it -> (p, accumulator)."""
    p, a = (np.asarray(t, np.float32) for t in (p, a))
    rho = _f32(rho)
    omr = _f32(1.0) - rho
    with np.errstate(all="ignore"):
        ge = effective_gradient_host(p, g, l2, grad_scale)
        a = rho * a + omr * (ge * ge)
        p = p - (_f32(lr_dec) * ge) / (np.sqrt(a) + _f32(epsilon))
    assert p.dtype == a.dtype == np.float32
    return p, a


def adagrad_host(p, g, a, lr_dec, epsilon, l2, grad_scale):
    """One Adagrad step as the module docstring states it -> (p, accumulator)."""
    p, a = (np.asarray(t, np.float32) for t in (p, a))
    with np.errstate(all="ignore"):
        ge = effective_gradient_host(p, g, l2, grad_scale)
        a = a + ge * ge
        p = p - (_f32(lr_dec) * ge) / (np.sqrt(a) + _f32(epsilon))
    assert p.dtype == a.dtype == np.float32
    return p, a


def adamax_host(p, g, m, u, lr_t, beta_1, beta_2, epsilon, l2, grad_scale):
    """One Adamax step as the module docstring states it -> (p, m, u)."""
    p, m, u = (np.asarray(t, np.float32) for t in (p, m, u))
    b1, b2 = _f32(beta_1), _f32(beta_2)
    omb1 = _f32(1.0) - b1
    with np.errstate(all="ignore"):
        ge = effective_gradient_host(p, g, l2, grad_scale)
        m = b1 * m + omb1 * ge
        u = np.maximum(b2 * u, np.abs(ge))
        p = p - (_f32(lr_t) * m) / (u + _f32(epsilon))
    assert p.dtype == m.dtype == u.dtype == np.float32
    return p, m, u


def nadam_host(p, g, m, v, lr, beta_1, beta_2, epsilon, c_g, c_m, c_v, omc_t, mc_t1, l2, grad_scale):
    """One Nadam step as the module docstring states it -> (p, m, v); the five schedule scalars are Nadam.step_scalars()."""
    p, m, v = (np.asarray(t, np.float32) for t in (p, m, v))
    b1, b2, one = _f32(beta_1), _f32(beta_2), _f32(1.0)
    omb1, omb2 = one - b1, one - b2
    with np.errstate(all="ignore"):
        ge = effective_gradient_host(p, g, l2, grad_scale)
        m = b1 * m + omb1 * ge
        v = b2 * v + omb2 * (ge * ge)
        mbar = _f32(omc_t) * (ge * _f32(c_g)) + _f32(mc_t1) * (m * _f32(c_m))
        p = p - (_f32(lr) * mbar) / (np.sqrt(v * _f32(c_v)) + _f32(epsilon))
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def _check_kwargs(kwargs, strict):
    for k in kwargs:
        if k in ("clipnorm", "clipvalue"):
            raise NotImplementedError("%s is not implemented: no gradient clipping runs on the update kernels" % k)
        if strict:
            raise TypeError("Unexpected keyword argument passed to optimizer: " + str(k))


class Optimizer(object):
    state_names = ()        # the per-weight state lists of get_weights(), in Keras' order

    def update_call(self, buffer):
        """The update kernel's entry point, its state buffers (`buffer(name)` gives the flat buffer of a state list; None
        for one the entry point takes as NULL) and the scalars of the coming step.  Every entry point is called as
        (param, grad, *state, n, *scalars, l2, grad_scale, sumsq)."""
        raise NotImplementedError

    def _bind(self, model):
        self._model = weakref.ref(model)

    def _bound_model(self):
        model = getattr(self, "_model", lambda: None)()
        if model is None or model.optimizer is not self:
            raise RuntimeError("the optimizer's weights exist once it is compiled into a model: model.compile(optimizer, ...)")
        return model

    def get_weights(self):
        """[iterations] + the state lists (see the module docstring), as numpy arrays."""
        model = self._bound_model()
        out = [np.asarray(self.iterations, dtype=np.int64)]
        for name in self.state_names:
            out.extend(model._optimizer_state_arrays(name))
        return out

    def set_weights(self, weights):
        model = self._bound_model()
        want = [()] + [s for name in self.state_names for s in model._optimizer_state_shapes(name)]
        if len(want) != len(weights):
            raise ValueError("Length of the specified weight list (" + str(len(weights)) + ") does not match the number of "
                             "weights of the optimizer (" + str(len(want)) + ")")
        weights = [np.asarray(w) for w in weights]
        for pv, w in zip(want, weights):
            if tuple(pv) != tuple(w.shape):
                raise ValueError("Optimizer weight shape " + str(tuple(pv)) + " not compatible with provided weight shape "
                                 + str(tuple(w.shape)))
        self.iterations = int(weights[0])
        i = 1
        for name in self.state_names:
            k = len(model._optimizer_state_shapes(name))
            model._set_optimizer_state_arrays(name, weights[i:i + k])
            i += k


class SGD(Optimizer):
    state_names = ("moments",)

    def __init__(self, lr=0.01, momentum=0.0, decay=0.0, nesterov=False, **kwargs):
        _check_kwargs(kwargs, strict=False)
        self.lr = float(lr)
        self.momentum = float(momentum)
        self.decay = float(decay)
        self.initial_decay = float(decay)
        self.nesterov = bool(nesterov)
        self.iterations = 0

    def current_lr(self):
        lr = self.lr
        if self.initial_decay > 0:
            lr = lr * (1.0 / (1.0 + self.decay * self.iterations))
        return lr

    def update_call(self, buffer):
        return "dj_sgd_momentum_update", [buffer("moments")], (self.current_lr(), self.momentum, int(self.nesterov))

    def get_config(self):
        return {"lr": self.lr, "momentum": self.momentum, "decay": self.decay, "nesterov": self.nesterov}


class Adam(Optimizer):
    state_names = ("ms", "vs", "vhats")

    def __init__(self, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0., amsgrad=False, **kwargs):
        _check_kwargs(kwargs, strict=True)
        self.lr = float(lr)
        self.beta_1 = float(beta_1)
        self.beta_2 = float(beta_2)
        self.epsilon = EPSILON if epsilon is None else float(epsilon)
        self.decay = float(decay)
        self.initial_decay = float(decay)
        self.amsgrad = bool(amsgrad)
        self.iterations = 0

    def current_lr(self):
        lr = self.lr
        if self.initial_decay > 0:
            lr = lr / (1.0 + self.decay * self.iterations)
        return lr

    def step_size(self):
        """lr_t of the next step, in float64; the kernel takes it rounded once to float32."""
        t = self.iterations + 1
        return self.current_lr() * math.sqrt(1.0 - self.beta_2 ** t) / (1.0 - self.beta_1 ** t)

    def update_call(self, buffer):
        return ("dj_adam_update", [buffer("ms"), buffer("vs"), buffer("vhats") if self.amsgrad else None],
                (self.step_size(), self.beta_1, self.beta_2, self.epsilon))

    def get_config(self):
        return {"lr": self.lr, "beta_1": self.beta_1, "beta_2": self.beta_2, "decay": self.decay, "epsilon": self.epsilon,
                "amsgrad": self.amsgrad}


class Adadelta(Optimizer):
    state_names = ("accumulators", "delta_accumulators")

    def __init__(self, lr=1.0, rho=0.95, epsilon=None, decay=0., **kwargs):
        _check_kwargs(kwargs, strict=True)
        self.lr = float(lr)
        self.rho = float(rho)
        self.epsilon = EPSILON if epsilon is None else float(epsilon)
        self.decay = float(decay)
        self.initial_decay = float(decay)
        self.iterations = 0

    def current_lr(self):
        lr = self.lr
        if self.initial_decay > 0:
            lr = lr / (1.0 + self.decay * self.iterations)
        return lr

    def update_call(self, buffer):
        return ("dj_adadelta_update", [buffer("accumulators"), buffer("delta_accumulators")],
                (self.current_lr(), self.rho, 1.0 - self.rho, self.epsilon))

    def get_config(self):
        return {"lr": self.lr, "rho": self.rho, "decay": self.decay, "epsilon": self.epsilon}


class RMSprop(Optimizer):
    state_names = ("accumulators",)

    def __init__(self, lr=0.001, rho=0.9, epsilon=None, decay=0., **kwargs):
        _check_kwargs(kwargs, strict=True)
        self.lr = float(lr)
        self.rho = float(rho)
        self.epsilon = EPSILON if epsilon is None else float(epsilon)
        self.decay = float(decay)
        self.initial_decay = float(decay)
        self.iterations = 0

    def current_lr(self):
        lr = self.lr
        if self.initial_decay > 0:
            lr = lr / (1.0 + self.decay * self.iterations)
        return lr

    def update_call(self, buffer):
        return "dj_rmsprop_update", [buffer("accumulators")], (self.current_lr(), self.rho, self.epsilon)

    def get_config(self):
        return {"lr": self.lr, "rho": self.rho, "decay": self.decay, "epsilon": self.epsilon}


class Adagrad(Optimizer):
    state_names = ("accumulators",)

    def __init__(self, lr=0.01, epsilon=None, decay=0., **kwargs):
        _check_kwargs(kwargs, strict=True)
        self.lr = float(lr)
        self.epsilon = EPSILON if epsilon is None else float(epsilon)
        self.decay = float(decay)
        self.initial_decay = float(decay)
        self.iterations = 0

    def current_lr(self):
        lr = self.lr
        if self.initial_decay > 0:
            lr = lr / (1.0 + self.decay * self.iterations)
        return lr

    def update_call(self, buffer):
        return "dj_adagrad_update", [buffer("accumulators")], (self.current_lr(), self.epsilon)

    def get_config(self):
        return {"lr": self.lr, "decay": self.decay, "epsilon": self.epsilon}


class Adamax(Optimizer):
    state_names = ("ms", "us")

    def __init__(self, lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0., **kwargs):
        _check_kwargs(kwargs, strict=True)
        self.lr = float(lr)
        self.beta_1 = float(beta_1)
        self.beta_2 = float(beta_2)
        self.epsilon = EPSILON if epsilon is None else float(epsilon)
        self.decay = float(decay)
        self.initial_decay = float(decay)
        self.iterations = 0

    def current_lr(self):
        lr = self.lr
        if self.initial_decay > 0:
            lr = lr / (1.0 + self.decay * self.iterations)
        return lr

    def step_size(self):
        """lr_t of the next step, in float64; the kernel takes it rounded once to float32."""
        return self.current_lr() / (1.0 - self.beta_1 ** (self.iterations + 1))

    def update_call(self, buffer):
        return ("dj_adamax_update", [buffer("ms"), buffer("us")],
                (self.step_size(), self.beta_1, self.beta_2, self.epsilon))

    def get_config(self):
        return {"lr": self.lr, "beta_1": self.beta_1, "beta_2": self.beta_2, "decay": self.decay, "epsilon": self.epsilon}


class Nadam(Optimizer):
    state_names = ("ms", "vs")

    def __init__(self, lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=None, schedule_decay=0.004, **kwargs):
        _check_kwargs(kwargs, strict=True)
        self.lr = float(lr)
        self.beta_1 = float(beta_1)
        self.beta_2 = float(beta_2)
        self.epsilon = EPSILON if epsilon is None else float(epsilon)
        self.schedule_decay = float(schedule_decay)
        self.iterations = 0
        self._schedule = (0, 1.0, None)     # (iterations, m_schedule there, the (beta_1, schedule_decay) it was made for)

    def current_lr(self):
        return self.lr

    def momentum_cache(self, i):
        """mc(i) of the module docstring, float64."""
        return self.beta_1 * (1.0 - 0.5 * 0.96 ** (i * self.schedule_decay))

    @property
    def m_schedule(self):
        """mc(1) * ... * mc(iterations), multiplied from the left in float64 (Keras' variable of that name).  A function of
        `iterations` alone: the value of the last call is kept, so a training step costs one product and a restored or
        rewound `iterations` the whole chain, which gives the same bits."""
        key = (self.beta_1, self.schedule_decay)
        at, value, made_for = self._schedule
        if at > self.iterations or made_for != key:
            at, value = 0, 1.0
        for i in range(at + 1, self.iterations + 1):
            value = value * self.momentum_cache(i)
        self._schedule = (self.iterations, value, key)
        return value

    def step_scalars(self):
        """(c_g, c_m, c_v, 1 - mc(t), mc(t + 1)) of the next step, in float64; the kernel takes each rounded once to float32."""
        t = self.iterations + 1
        mc_t, mc_t1 = self.momentum_cache(t), self.momentum_cache(t + 1)
        ms_new = self.m_schedule * mc_t
        ms_next = ms_new * mc_t1
        return (1.0 / (1.0 - ms_new), 1.0 / (1.0 - ms_next), 1.0 / (1.0 - self.beta_2 ** t), 1.0 - mc_t, mc_t1)

    def update_call(self, buffer):
        return ("dj_nadam_update", [buffer("ms"), buffer("vs")],
                (self.lr, self.beta_1, self.beta_2, self.epsilon) + self.step_scalars())

    def get_config(self):
        return {"lr": self.lr, "beta_1": self.beta_1, "beta_2": self.beta_2, "epsilon": self.epsilon,
                "schedule_decay": self.schedule_decay}


def get(identifier):
    """What Model.compile takes: an instance of SGD, Adam, Adadelta, RMSprop, Adagrad, Adamax or Nadam, or the name 'sgd'
    (case-insensitive).  No other is resolved by name: compile(optimizer="adam") has always raised NotImplementedError
    here and code may rely on it (tests/test_callbacks_cpu.py does), so all but SGD are passed as instances."""
    if isinstance(identifier, str) and identifier.lower() == "sgd":
        return SGD()
    if isinstance(identifier, (SGD, Adam, Adadelta, RMSprop, Adagrad, Adamax, Nadam)):
        return identifier
    raise NotImplementedError("optimizer %r: pass an instance of keras.optimizers.SGD, Adam, Adadelta, RMSprop, Adagrad, "
                              "Adamax or Nadam (the seven with an update kernel), or the name 'sgd'" % (identifier,))
