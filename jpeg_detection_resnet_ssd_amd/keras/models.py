"""keras.models.Model facade over engine.Plan: the methods the reference's entry points call --
compile / fit_generator / predict / train_on_batch / load_weights(by_name) / save_weights /
get_layer(name).output_shape / layers / summary / count_params
(localisation_part/training_dct_pascal_j2d_resnet.py:134-156,244-249,330-336;
classification_part/training.py:159-198; localisation_part/eval_utils/average_precision_evaluator.py:381)."""
import math
import os
import time

import numpy as np
import torch

from .. import engine
from ..engine import GradRef, Plan, Value, call, query
from . import callbacks as cbks
from . import layers as L
from . import optimizers


def _align4(n):
    return (n + 3) // 4 * 4


class Model(object):
    def __init__(self, inputs, outputs, name=None):
        self.inputs = list(inputs) if isinstance(inputs, (list, tuple)) else [inputs]
        self.outputs = list(outputs) if isinstance(outputs, (list, tuple)) else [outputs]
        self.name = name or "model_1"
        # collect the layers reachable from the outputs; creation order is a topological order
        seen, stack = {}, [t.layer for t in self.outputs]
        while stack:
            lyr = stack.pop()
            if id(lyr) in seen:
                continue
            seen[id(lyr)] = lyr
            for t in lyr.inbound:
                stack.append(t.layer)
        for t in self.inputs:
            if id(t.layer) not in seen:
                raise ValueError("Graph disconnected: input %r does not reach the outputs" % (t,))
        self.layers = sorted(seen.values(), key=lambda l: l.serial)
        names = {}
        for lyr in self.layers:
            if lyr.name in names:
                raise ValueError('The name "%s" is used %d times in the model. All layer names should be unique.'
                                 % (lyr.name, 2))
            names[lyr.name] = lyr
        self._by_name = names
        self._consumers = {}
        for lyr in self.layers:
            for t in lyr.inbound:
                self._consumers.setdefault(id(t), []).append(lyr)
        self.optimizer = None
        self.loss = None
        self.metrics = []
        self.stop_training = False
        self._plans = {}
        self._store = None
        self._device = None
        self.dist = None          # set by dist.DataParallel
        self._last_train_plan = None
        self.last_step_info = {}

    # ---- graph queries ------------------------------------------------------------
    def consumers_of(self, ktensor):
        return self._consumers.get(id(ktensor), [])

    def get_layer(self, name=None, index=None):
        if index is not None:
            return self.layers[index]
        if name not in self._by_name:
            raise ValueError("No such layer: " + str(name))
        return self._by_name[name]

    @property
    def weight_specs(self):
        out = []
        for lyr in self.layers:
            out.extend(lyr.weight_specs)
        return out

    def count_params(self):
        return sum(w.size for w in self.weight_specs)

    def summary(self, print_fn=print):
        print_fn("_" * 98)
        print_fn("%-45s %-28s %12s" % ("Layer (type)", "Output Shape", "Param #"))
        print_fn("=" * 98)
        for lyr in self.layers:
            print_fn("%-45s %-28s %12d" % ("%s (%s)" % (lyr.name, lyr.__class__.__name__), str(lyr.output_shape),
                                            lyr.count_params()))
        tr = sum(w.size for w in self.weight_specs if w.trainable)
        tot = self.count_params()
        print_fn("=" * 98)
        print_fn("Total params: {:,}".format(tot))
        print_fn("Trainable params: {:,}".format(tr))
        print_fn("Non-trainable params: {:,}".format(tot - tr))

    # ---- parameters -----------------------------------------------------------------
    def _ensure_params(self, device=None):
        """Allocate every weight in ONE flat HBM buffer (plus one for gradients and one for the SGD
        velocity): [un-regularised trainables | l2-regularised trainables (grouped by l2) | state]."""
        if self._store is not None:
            return
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("no MI355X visible: the compute path has no CPU fallback")
            device = torch.device("cuda", torch.cuda.current_device())
        self._device = device
        specs = self.weight_specs
        plain = [w for w in specs if w.trainable and not w.l2]
        reg = sorted([w for w in specs if w.trainable and w.l2], key=lambda w: w.l2)
        state = [w for w in specs if not w.trainable]
        order = plain + reg + state
        offs, o = {}, 0
        for w in order:
            offs[id(w)] = o
            o += _align4(w.size)
        total = o
        n_train = offs[id(state[0])] if state else total
        flat = torch.zeros(total, dtype=torch.float32, device=device)
        grads = torch.zeros(n_train, dtype=torch.float32, device=device)
        vel = torch.zeros(n_train, dtype=torch.float32, device=device)
        host = torch.zeros(total, dtype=torch.float32)
        for w in order:
            a = offs[id(w)]
            val = w.init_value if w.init_value is not None else w.initializer(w.shape)
            host[a:a + w.size] = torch.as_tensor(val, dtype=torch.float32).reshape(-1)
            w.init_value = None
            w.param = flat[a:a + w.size].view(*w.shape)
            if w.trainable:
                w.grad = grads[a:a + w.size].view(*w.shape)
        flat.copy_(host)
        # SGD segments: (begin, end, l2)
        segs = []
        if plain:
            segs.append((0, offs[id(reg[0])] if reg else n_train, 0.0))
        i = 0
        while i < len(reg):
            j = i
            while j < len(reg) and reg[j].l2 == reg[i].l2:
                j += 1
            end = offs[id(reg[j])] if j < len(reg) else n_train
            segs.append((offs[id(reg[i])], end, reg[i].l2))
            i = j
        self._store = dict(flat=flat, grads=grads, vel=vel, n_train=n_train, segments=segs, offsets=offs,
                           sumsq=torch.zeros(len(segs), dtype=torch.float32, device=device))

    def weight_shadows(self, plan):
        """fp16 and bf16 copies of the flat weight buffer (K.set_floatx('float16')): what the reduced-precision GEMMs read as
        their B operand -- fp16 in the forward pass, bf16 in the input gradient -- instead of converting the fp32 master
        weights again in every tile.  `spec.param16` / `spec.parambf` are views like `spec.param`; one dj_shadow_weights
        launch at the head of `plan`'s forward list refreshes them every step, whoever changed the master copy."""
        self._ensure_params()
        st = self._store
        if "flat16" not in st:
            n = st["flat"].numel()
            st["flat16"] = torch.empty(n, dtype=torch.float16, device=self._device)
            st["flatbf"] = torch.empty(n, dtype=torch.bfloat16, device=self._device)
            for w in self.weight_specs:
                a = st["offsets"][id(w)]
                w.param16 = st["flat16"][a:a + w.size].view(*w.shape)
                w.parambf = st["flatbf"][a:a + w.size].view(*w.shape)
            if self._device.type == "cuda":
                call("dj_shadow_weights", st["flat"], st["flat16"], st["flatbf"], n)
        if not getattr(plan, "_shadows_refreshed", False):
            flat, f16, fbf, n = st["flat"], st["flat16"], st["flatbf"], st["flat"].numel()
            plan.fwd.insert(0, lambda: call("dj_shadow_weights", flat, f16, fbf, n))
            plan._shadows_refreshed = True

    @property
    def flat_gradients(self):
        self._ensure_params()
        return self._store["grads"]

    @property
    def flat_trainable(self):
        self._ensure_params()
        return self._store["flat"][: self._store["n_train"]]

    @property
    def flat_all(self):
        self._ensure_params()
        return self._store["flat"]

    def get_weights_dict(self):
        """{'<layer>/<weight>': numpy array} -- Keras-named, as `load_weights(by_name=True)` matches them."""
        self._ensure_params()
        torch.cuda.synchronize()
        return {w.key: w.param.detach().cpu().numpy().copy() for w in self.weight_specs}

    def set_weights_dict(self, d, strict=False):
        self._ensure_params()
        n = 0
        for w in self.weight_specs:
            if w.key in d:
                v = np.asarray(d[w.key], dtype=np.float32)
                if tuple(v.shape) != w.shape:
                    raise ValueError("Layer weight shape %s not compatible with provided weight shape %s (%s)"
                                     % (w.shape, v.shape, w.key))
                w.param.copy_(torch.from_numpy(v).to(w.param.device))
                n += 1
            elif strict:
                raise ValueError("missing weight " + w.key)
        return n

    def get_weights(self):
        d = self.get_weights_dict()
        return [d[w.key] for w in self.weight_specs]

    def set_weights(self, weights):
        specs = self.weight_specs
        if len(weights) != len(specs):
            raise ValueError("You called `set_weights(weights)` with a weight list of length %d, but the model was "
                             "expecting %d weights." % (len(weights), len(specs)))
        self.set_weights_dict({w.key: v for w, v in zip(specs, weights)})

    def save_weights(self, filepath, overwrite=True):
        """Keras writes HDF5; h5py is not available here, so the same name->array mapping is stored as
        an .npz archive under the given path (the path is used verbatim, suffix included)."""
        d = self.get_weights_dict()
        with open(filepath, "wb") as f:
            np.savez(f, **d)

    save = save_weights

    def load_weights(self, filepath, by_name=False):
        with np.load(filepath, allow_pickle=False) as z:
            d = {k: z[k] for k in z.files}
        if by_name:
            return self.set_weights_dict(d)
        return self.set_weights_dict(d, strict=True)

    # ---- compile ----------------------------------------------------------------------
    def compile(self, optimizer, loss=None, metrics=None, **kwargs):
        optimizer = optimizers.get(optimizer)
        if self.optimizer is not None and type(optimizer) is not type(self.optimizer) and self._store is not None:
            # an optimizer of another kind starts from zeroed state, as a fresh Keras optimizer does
            self._store.pop("opt_state", None)
            self._store["vel"].zero_()
        self.optimizer = optimizer
        optimizer._bind(self)
        self.metrics = list(metrics or [])
        owner = getattr(loss, "__self__", None)
        if owner is not None and hasattr(owner, "_dj_loss"):
            self.loss = ("ssd", owner)
        elif loss == "categorical_crossentropy" or getattr(loss, "_dj_loss", None) == "categorical_crossentropy":
            self.loss = ("cce", None)
        elif loss is None:
            self.loss = None
        elif callable(loss):
            # Keras loss protocol (localisation_part/training_dct_pascal_j2d_resnet.py:154-156): any
            # loss(y_true, y_pred) -> (batch,) written in torch ops.  It is evaluated on the device-resident tensors and
            # differentiated by torch autograd with respect to y_pred only; the model's own backward pass (the HIP
            # launch list) starts from that gradient.  Checked here, at compile time, on a tiny probe so that a callable
            # that cannot take device tensors fails now and not in the middle of fit_generator.
            self._probe_loss(loss)
            self.loss = ("callable", loss)
        else:
            raise NotImplementedError("loss %r has no MI355X lowering: pass SSDLoss(...).compute_loss, "
                                      "'categorical_crossentropy', or a callable loss(y_true, y_pred) written in torch "
                                      "ops on CUDA tensors" % (loss,))
        self._plans = {}

    def _probe_loss(self, loss):
        if not torch.cuda.is_available():
            return      # graph building without a GPU (structure tests): the probe runs on the first GPU compile
        shape = (2,) + tuple(int(d) for d in self.outputs[0].shape[1:])
        dev = torch.device("cuda", torch.cuda.current_device())
        yp = torch.rand(shape, device=dev).requires_grad_(True)
        yt = torch.rand(shape, device=dev)
        try:
            val = loss(yt, yp)
            if not (isinstance(val, torch.Tensor) and val.requires_grad):
                raise TypeError("it returned %r, not a torch tensor that depends on y_pred" % (type(val).__name__,))
            val.mean().backward()
        except Exception as e:
            raise TypeError("loss %r cannot be compiled: a custom loss must be loss(y_true, y_pred) -> (batch,) in "
                            "differentiable torch ops on CUDA tensors (probe on shape %s failed: %s: %s)"
                            % (loss, shape, type(e).__name__, e))

    # ---- plans ------------------------------------------------------------------------
    def _plan(self, batch_size, training, with_loss, external_grad=False):
        """`external_grad`: training plan without a loss whose backward starts from a caller-filled
        gradient of the first output (`plan.external_grad`) -- used for layer-level parity tests."""
        key = (batch_size, training, with_loss, external_grad)
        if key in self._plans:
            return self._plans[key]
        self._ensure_params()
        plan = Plan(self._device, batch_size, training)
        if training:
            plan.clear_gradients_first(self._store["grads"])
        for lyr in self.layers:
            lyr_ins = [plan.values[id(t)] for t in lyr.inbound]
            if isinstance(lyr, L.InputLayer):
                if not any(lyr is t.layer for t in self.inputs):
                    raise ValueError("Input layer %s is not a model input" % lyr.name)
            if not (hasattr(lyr, "runs_beside") and lyr.runs_beside(plan, self, lyr_ins)):
                plan.wait_side_inputs(lyr_ins)
            out = lyr.lower(plan, self, lyr_ins)
            plan.values[id(lyr.outbound[0])] = out
            # a tensor with several readers may have some that only feed the end of the forward pass (SSD predictor
            # heads): note the point where it is final, so that they can run beside the main chain (Plan.emit_side)
            if (training and isinstance(out, Value) and len(self.consumers_of(lyr.outbound[0])) > 1
                    and out.pending_add is None and out.side_done is None):
                plan.mark_ready(out)
        # model inputs in the order given to Model(...)
        order = []
        for t in self.inputs:
            order.append(plan.values[id(t)].buf)
        plan.inputs = order
        plan.outputs = [plan.values[id(t)] for t in self.outputs]
        if with_loss:
            self._lower_loss(plan)
        if external_grad:
            def seed_gradient():
                plan.external_grad, _ = plan.grad_of(plan.outputs[0])
            plan.on_backward(seed_gradient)
        if training:
            plan.build_backward()
        if os.environ.get("DJ_AUTOTUNE", "1") != "0":
            plan.autotune(reps=int(os.environ.get("DJ_AUTOTUNE_REPS", "2")),
                          verbose=os.environ.get("DJ_AUTOTUNE_VERBOSE", "0") == "1",
                          measure=os.environ.get("DJ_AUTOTUNE", "1") != "table")
            plan.finalize_workspaces()
            if os.environ.get("DJ_TUNE_SAVE"):
                from ..engine import save_tune_db
                save_tune_db(os.environ["DJ_TUNE_SAVE"])
        if training:
            if self.dist is not None and with_loss:
                self.dist.attach(plan)
        self._plans[key] = plan
        return plan

    def _lower_loss(self, plan):
        if self.loss is None:
            raise RuntimeError("You must compile a model before training/testing. Use `model.compile(optimizer, loss)`.")
        kind, obj = self.loss
        pred = plan.outputs[0]
        yp = pred.buf
        assert not pred.is_affine and yp.is_contiguous()
        plan.y_true = plan.empty(*yp.shape)
        plan.loss_out = plan.zeros(8)
        yt = plan.y_true
        if kind == "ssd":
            n_cls = yp.shape[-1] - 12
            nbox = yp.numel() // yp.shape[-1]
            ws = plan.empty(query("dj_ssd_loss_workspace_floats", nbox))
            out5 = plan.loss_out
            ratio, nmin, alpha = int(obj.neg_pos_ratio), int(obj.n_neg_min), float(obj.alpha)

            def loss_fwd():
                if plan.targets_event is not None:   # y_true is being encoded on the side stream (see _upload)
                    torch.cuda.current_stream().wait_event(plan.targets_event)
                    plan.targets_event = None
                call("dj_ssd_loss_fwd", yt, yp, nbox, n_cls, ratio, nmin, alpha, ws, out5)
            plan.emit(loss_fwd)

            def build_backward():
                d, beta = plan.grad_of(pred)
                assert beta == 0
                plan.emit_bwd(lambda: call("dj_ssd_loss_bwd", yt, yp, nbox, n_cls, alpha, 1.0, ws, out5, d))

            plan.on_backward(build_backward)
        elif kind == "callable":
            out = plan.loss_out
            dpred = plan.empty(*yp.shape) if plan.training else None

            def loss_fwd():
                if plan.targets_event is not None:   # y_true is being encoded on the side stream (see _upload)
                    torch.cuda.current_stream().wait_event(plan.targets_event)
                    plan.targets_event = None
                # Keras: total loss = mean over the batch of loss(y_true, y_pred); torch autograd supplies d/d y_pred
                leaf = yp.detach().requires_grad_(plan.training)
                with torch.enable_grad():
                    val = obj(yt, leaf).mean()
                    if plan.training:
                        dpred.copy_(torch.autograd.grad(val, leaf)[0])
                out[0:1].copy_(val.detach().reshape(1))
            plan.emit(loss_fwd)

            def build_backward():
                plan.set_grad_ref(pred, GradRef(dpred))

            plan.on_backward(build_backward)
        else:
            rows, c = yp.shape[0], yp.shape[1]
            loss_rows = plan.empty(rows)
            dprobs = plan.empty(rows, c) if plan.training else None
            out = plan.loss_out
            plan.emit(lambda: call("dj_categorical_crossentropy", yt, yp, rows, c, 1.0, loss_rows, dprobs, out))

            def build_backward():
                plan.set_grad_ref(pred, GradRef(dprobs))

            plan.on_backward(build_backward)

    # ---- steps ----------------------------------------------------------------------
    @staticmethod
    def _as_list(x):
        return list(x) if isinstance(x, (list, tuple)) else [x]

    def _upload(self, plan, x, y):
        if isinstance(x, (list, tuple)) and len(x) == 1 and hasattr(x[0], "emit_into"):
            x = x[0]                     # (`predict` slices its inputs into a list)
        if hasattr(x, "emit_into"):      # PendingDCTInputs: the pixels go up, the JPEG transform runs on the device
            shapes = [tuple(s) for s in x.shapes]
            if len(shapes) != len(plan.inputs):
                raise ValueError("Error when checking model input: expected %d arrays but got %d"
                                 % (len(plan.inputs), len(shapes)))
            for buf, shp in zip(plan.inputs, shapes):
                if shp != tuple(buf.shape):
                    raise ValueError("Error when checking input: expected shape %s but got array with shape %s"
                                     % (tuple(buf.shape), shp))
            x.emit_into(plan.inputs)
            xs = []
        else:
            xs = self._as_list(x)
            if len(xs) != len(plan.inputs):
                raise ValueError("Error when checking model input: expected %d arrays but got %d"
                                 % (len(plan.inputs), len(xs)))
        for buf, arr in zip(plan.inputs, xs):
            t = arr if isinstance(arr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(arr))
            if tuple(t.shape) != tuple(buf.shape):
                raise ValueError("Error when checking input: expected shape %s but got array with shape %s"
                                 % (tuple(buf.shape), tuple(t.shape)))
            buf.copy_(t.to(torch.float32), non_blocking=True)
        if y is not None and hasattr(y, "encode_into"):      # PendingTargets: SSDInputEncoder runs on the device
            if tuple(y.shape) != tuple(plan.y_true.shape):
                raise ValueError("Error when checking target: expected shape %s but got array with shape %s"
                                 % (tuple(plan.y_true.shape), tuple(y.shape)))
            side = plan.side_stream
            if side is None:
                y.encode_into(plan.y_true)
            else:
                # the matching kernel runs beside the forward pass: it may start once the previous step (whose loss
                # still reads y_true) has drained, and the loss of this step waits for it
                drained = torch.cuda.Event()
                drained.record()
                side.wait_event(drained)
                with torch.cuda.stream(side):
                    y.encode_into(plan.y_true)
                    plan.targets_event = torch.cuda.Event()
                    plan.targets_event.record(side)
        elif y is not None:
            t = y if isinstance(y, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(y))
            if tuple(t.shape) != tuple(plan.y_true.shape):
                raise ValueError("Error when checking target: expected shape %s but got array with shape %s"
                                 % (tuple(plan.y_true.shape), tuple(t.shape)))
            plan.y_true.copy_(t.to(torch.float32), non_blocking=True)

    def _apply_optimizer(self, plan=None):
        """`plan`: the training plan whose backward pass just ran (data parallel: it must carry the gradient exchange;
        None = the plan of the last run_train_step)."""
        st, opt = self._store, self.optimizer
        scale = 1.0
        if self.dist is not None:
            scale = self.dist.finish_gradients(plan if plan is not None else self._last_train_plan)
        entry, state, scalars = opt.update_call(self._optimizer_buffer)
        st["sumsq"].zero_()
        for i, (a, b, l2) in enumerate(st["segments"]):
            if b <= a:
                continue
            call(entry, st["flat"][a:b], st["grads"][a:b], *[s[a:b] if s is not None else None for s in state], b - a,
                 *scalars, l2, scale, st["sumsq"][i:i + 1] if l2 else None)
        opt.iterations += 1

    # ---- optimizer state (Optimizer.get_weights / set_weights) -----------------------------
    def _optimizer_buffer(self, name):
        """The flat fp32 state buffer `name` of the compiled optimizer, n_train elements laid out like `flat`; SGD's
        'moments' is the velocity buffer, the others are allocated zeroed when first asked for."""
        self._ensure_params()
        st = self._store
        if name == "moments":
            return st["vel"]
        bufs = st.setdefault("opt_state", {})
        if name not in bufs:
            bufs[name] = torch.zeros(st["n_train"], dtype=torch.float32, device=self._device)
        return bufs[name]

    def _placeholder_state(self, name):
        """Keras 2.2.4 keeps Adam's vhats as one zeros(1) per weight when amsgrad is off."""
        return name == "vhats" and not self.optimizer.amsgrad

    def _optimizer_state_shapes(self, name):
        return [(1,) if self._placeholder_state(name) else tuple(w.shape) for w in self.weight_specs if w.trainable]

    def _optimizer_state_arrays(self, name):
        train = [w for w in self.weight_specs if w.trainable]
        if self._placeholder_state(name):
            return [np.zeros(1, np.float32) for _ in train]
        host = self._optimizer_buffer(name).detach().cpu().numpy()
        offs = self._store["offsets"]
        return [host[offs[id(w)]:offs[id(w)] + w.size].reshape(w.shape).copy() for w in train]

    def _set_optimizer_state_arrays(self, name, arrays):
        if self._placeholder_state(name):
            return
        buf, offs = self._optimizer_buffer(name), self._store["offsets"]
        host = buf.detach().cpu()
        for w, v in zip([w for w in self.weight_specs if w.trainable], arrays):
            a = offs[id(w)]
            host[a:a + w.size] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32).reshape(-1))
        buf.copy_(host)

    def run_train_step(self, plan):
        """Forward, backward and optimizer step on buffers already resident in HBM (no host sync)."""
        self._last_train_plan = plan
        plan.run_forward()
        plan.run_backward()
        self._apply_optimizer(plan)

    def _loss_value(self, plan, with_reg=True):
        vals = plan.loss_out.detach().cpu()
        data = float(vals[0])
        reg = 0.0
        if with_reg:
            ss = self._store["sumsq"].detach().cpu()
            for i, (_, _, l2) in enumerate(self._store["segments"]):
                reg += l2 * float(ss[i])
        self.last_step_info = dict(data_loss=data, reg_loss=reg, n_positive=float(vals[1]), n_negative=float(vals[2]))
        return data + reg

    def _metric_values(self, plan):
        """Compile-time `metrics` callables, evaluated as metric(y_true, y_pred) on the device-resident batch;
        named like Keras names anonymous metric functions (`_func`, `_func_1`, ...)."""
        out, seen = {}, {}
        for m in self.metrics:
            name = getattr(m, "__name__", str(m)) if callable(m) else str(m)
            if not callable(m):
                if name in ("accuracy", "acc"):
                    from .metrics import categorical_accuracy as m
                    name = "acc"
                else:
                    continue
            n = seen.get(name, 0)
            seen[name] = n + 1
            out[name if n == 0 else "%s_%d" % (name, n)] = float(m(plan.y_true, plan.outputs[0].buf))
        return out

    def train_on_batch(self, x, y):
        b = self._as_list(x)[0].shape[0]
        plan = self._plan(b, True, True)
        self._upload(plan, x, y)
        self.run_train_step(plan)
        loss = self._loss_value(plan)
        if self.metrics:
            self.last_step_info["metrics"] = self._metric_values(plan)
        return loss

    def test_on_batch(self, x, y):
        b = self._as_list(x)[0].shape[0]
        plan = self._plan(b, False, True)
        self._upload(plan, x, y)
        plan.run_forward()
        return self._loss_value(plan, with_reg=False) + self._reg_penalty()

    def _reg_penalty(self):
        tot = 0.0
        for (a, b, l2) in self._store["segments"]:
            if l2 and b > a:
                tot += l2 * float((self._store["flat"][a:b] ** 2).sum())
        return tot

    def predict_on_batch(self, x, to_host=True):
        """`to_host=False`: the outputs as the CUDA tensors the plan owns, without a download.  The next forward pass of
        this batch size overwrites them: consume them on the launch stream before it."""
        b = self._as_list(x)[0].shape[0]
        plan = self._plan(b, False, False)
        self._upload(plan, x, None)
        plan.run_forward()
        if not to_host:
            outs = [v.buf.detach() for v in plan.outputs]
            return outs[0] if len(outs) == 1 else outs
        outs = [v.buf.detach().cpu().numpy() for v in plan.outputs]
        return outs[0] if len(outs) == 1 else outs

    def predict(self, x, batch_size=32, verbose=0):
        xs = self._as_list(x)
        n = xs[0].shape[0]
        chunks = []
        for i in range(0, n, batch_size):
            chunks.append(self.predict_on_batch([a[i:i + batch_size] for a in xs]))
        if isinstance(chunks[0], list):
            return [np.concatenate([c[j] for c in chunks], axis=0) for j in range(len(chunks[0]))]
        return np.concatenate(chunks, axis=0)

    # ---- evaluation -------------------------------------------------------------------
    @property
    def metrics_names(self):
        """['loss'] followed by the log names of the compiled metrics (`_func`, `_func_1`, `acc`, ...)."""
        from .metrics import metric_entries
        return ["loss"] + [name for name, _ in metric_entries(self.metrics)]

    def evaluate_generator(self, generator, steps=None, max_queue_size=10, workers=1, use_multiprocessing=False, verbose=0):
        """Keras `evaluate_generator` (classification_part/vgg_jpeg_keras/evaluation/evaluators.py:22): `steps` batches of
        `generator` (all of a `Sequence` when None) -> the loss, averaged over the batches weighted by their sizes plus the
        regularisation penalty, as a scalar when the model was compiled without metrics, else [loss, metric, ...] in
        `metrics_names` order.  Loss and hit counts are accumulated on the device (dj_eval_accumulate, one launch behind each
        forward pass) and downloaded once, when the pass ends.  On a data-parallel model every rank evaluates what its own
        generator yields and the values returned are the local rank's: nothing is averaged across ranks here."""
        if steps is None:
            if hasattr(generator, "__len__"):     # keras.utils.Sequence
                steps = len(generator)
            else:
                raise ValueError("`steps=None` is only valid for a generator based on the `keras.utils.Sequence`"
                                 " class. Please specify `steps` or use the `keras.utils.Sequence` class.")
        import itertools
        steps = int(steps)
        it = itertools.islice(iter(generator), steps)     # the background thread stops where the pass does
        feeder = _Prefetcher(it, max_queue_size) if workers and workers > 0 else None
        sweep = _EvalSweep(self, size_weighted=True)
        t0 = time.time()
        try:
            for _ in range(steps):
                batch = feeder.get() if feeder is not None else next(it)
                sweep.add(batch[0], batch[1])
        finally:
            if feeder is not None:
                feeder.close()
        values = sweep.finish()
        if hasattr(generator, "check_inputs"):      # a failure a device input path only finds behind the batch
            generator.check_inputs()
        out = [values[name] for name in self.metrics_names]
        if verbose:
            print("%d/%d - %.0fs - %s" % (steps, steps, time.time() - t0,
                                          " - ".join("%s: %.4f" % (n, v) for n, v in zip(self.metrics_names, out))))
        return out[0] if len(out) == 1 else out

    # ---- training loop ----------------------------------------------------------------
    def fit_generator(self, generator, steps_per_epoch=None, epochs=1, verbose=1, callbacks=None,
                      validation_data=None, validation_steps=None, class_weight=None, max_queue_size=10, workers=1,
                      use_multiprocessing=False, shuffle=True, initial_epoch=0):
        """Keras `fit_generator` contract: `generator` yields (inputs, targets) batches forever;
        one epoch = `steps_per_epoch` train_on_batch calls, then an optional validation sweep."""
        if steps_per_epoch is None:
            steps_per_epoch = len(generator)
        history = cbks.History()
        cb_list = [history] + list(callbacks or [])
        for cb in cb_list:
            cb.set_model(self)
            cb.params = {"steps": steps_per_epoch, "epochs": epochs}
            cb.on_train_begin()
        it = iter(generator)
        val_it = iter(validation_data) if validation_data is not None and not isinstance(validation_data, tuple) else None
        if val_it is not None and validation_steps is None:
            if hasattr(validation_data, "__len__"):     # keras.utils.Sequence
                validation_steps = len(validation_data)
            else:
                raise ValueError("`validation_steps=None` is only valid for a generator based on the `keras.utils.Sequence`"
                                 " class. Please specify `validation_steps` or use the `keras.utils.Sequence` class.")
        self.stop_training = False
        rank0 = self.dist is None or self.dist.rank == 0
        # Keras runs the generator in a background enqueuer (`workers`, `max_queue_size`); so does this loop, with one
        # thread (a plain generator is not thread-safe): batch production overlaps the GPU step.  (Reading a step's loss
        # one step late, to spare the per-step host sync, was measured at 1057 vs 1053 img/s and is not done: callbacks
        # see every loss before the next batch starts, as in Keras.)
        feeder = _Prefetcher(it, max_queue_size) if workers and workers > 0 else None
        for epoch in range(initial_epoch, epochs):
            for cb in cb_list:
                cb.on_epoch_begin(epoch)
            t0, run, run_metrics = time.time(), 0.0, {}
            for step in range(steps_per_epoch):
                for cb in cb_list:
                    cb.on_batch_begin(step)
                batch = feeder.get() if feeder is not None else next(it)
                x, y = batch[0], batch[1]
                loss = self.train_on_batch(x, y)
                run += loss
                logs = {"loss": loss, "batch": step, "size": self._as_list(x)[0].shape[0]}
                for mk, mv in self.last_step_info.get("metrics", {}).items():
                    logs[mk] = mv
                    run_metrics[mk] = run_metrics.get(mk, 0.0) + mv
                for cb in cb_list:
                    cb.on_batch_end(step, logs)
                if self.stop_training:
                    break
            logs = {"loss": run / max(1, step + 1), "lr": self.optimizer.current_lr()}
            for mk, mv in run_metrics.items():
                logs[mk] = mv / max(1, step + 1)
            if validation_data is not None:
                # val_loss: the plain mean over the batches of data loss + penalty (every batch weighs 1); the metrics are
                # hits / rows.  One download for the whole sweep.
                sweep = _EvalSweep(self, size_weighted=False)
                if val_it is not None:
                    for _ in range(int(validation_steps)):
                        vb = next(val_it)
                        sweep.add(vb[0], vb[1])
                else:
                    sweep.add(validation_data[0], validation_data[1])
                for mk, mv in sweep.finish().items():
                    logs["val_" + mk] = mv
            for source in (generator, validation_data):
                if hasattr(source, "check_inputs"):      # a failure a device input path only finds behind the batch
                    source.check_inputs()
            if self.dist is not None:
                logs = self.dist.average_metrics(logs)
            if verbose and rank0:
                print("Epoch %d/%d - %.0fs - %s" % (epoch + 1, epochs, time.time() - t0,
                                                    " - ".join("%s: %.4f" % kv for kv in sorted(logs.items()))))
            for cb in cb_list:
                cb.on_epoch_end(epoch, logs)
            if self.stop_training:
                break
        if feeder is not None:
            feeder.close()
        for cb in cb_list:
            cb.on_train_end()
        return history


class _EvalSweep(object):
    """One pass of a model over evaluation batches whose loss and metrics stay on the device until the pass ends.
    Per batch: the inference plan's forward pass and one dj_eval_accumulate behind it on the same stream, which adds
    weight * (the batch's mean loss) and weight to `acc` and, for a 2-D float32 probability output, the row count and the
    hits of every metric the kernel can take (keras/metrics.py:device_metric_k) to `counts`.  `size_weighted`: the weight
    is the batch size (evaluate_generator), else 1 (fit_generator's val_loss, a plain mean over batches).  Any other
    metric callable is evaluated per batch on the device tensors, as Model._metric_values does -- one host sync each --
    and averaged weighted by batch size.  The regularisation penalty does not change during a pass: it is computed once,
    in `finish`, which makes the pass's only download of the accumulators."""

    def __init__(self, model, size_weighted):
        from .metrics import metric_entries
        self.model, self.size_weighted = model, size_weighted
        self.entries = metric_entries(model.metrics)
        self.acc = None       # set up by the first batch: its plan tells whether the output can be classified on the device

    def _setup(self, plan):
        from .metrics import categorical_accuracy, device_metric_k
        buf = plan.outputs[0].buf
        classify = buf.dim() == 2 and buf.dtype == torch.float32 and buf.is_contiguous()
        c = int(buf.shape[-1])
        ks, self.slots, self.per_batch = [], {}, []
        for name, m in self.entries:
            k = device_metric_k(m) if classify else None
            if k is not None:
                k = min(k, c)                       # fewer than k classes above the target: the same for every k >= C
                if k not in ks and len(ks) == 8:    # the kernel takes 8 entries per launch
                    k = None
            if k is None:
                self.per_batch.append((name, m if callable(m) else categorical_accuracy))
            else:
                if k not in ks:
                    ks.append(k)
                self.slots[name] = 1 + ks.index(k)
        self.ks = np.asarray(ks, dtype=np.int32)
        self.classify = classify and len(ks) > 0
        self.acc = torch.zeros(2, dtype=torch.float64, device=buf.device)
        self.counts = torch.zeros(1 + len(ks), dtype=torch.int64, device=buf.device)
        self.host_sums, self.host_rows = {name: 0.0 for name, _ in self.per_batch}, 0

    def add(self, x, y):
        from .. import kernels
        model = self.model
        b = model._as_list(x)[0].shape[0]
        plan = model._plan(b, False, True)
        model._upload(plan, x, y)
        plan.run_forward()
        if self.acc is None:
            self._setup(plan)
        probs = plan.outputs[0].buf
        kernels.eval_accumulate(plan.y_true if self.classify else None, probs if self.classify else None, self.ks,
                                plan.loss_out, float(b) if self.size_weighted else 1.0, self.acc, self.counts)
        for name, m in self.per_batch:
            self.host_sums[name] += b * float(m(plan.y_true, probs))
        self.host_rows += b

    def _download(self):
        """The accumulators as one float64 host array [loss sum, weight sum, rows, hits...] (counts are exact in a double up
        to 2^53): the one device-to-host copy of a pass."""
        return torch.cat([self.acc, self.counts.to(torch.float64)]).cpu().numpy()

    def finish(self):
        """-> {'loss': ..., '<metric name>': ...} in the order of Model.metrics_names."""
        out = {}
        if self.acc is None:      # no batch at all
            out["loss"] = float("nan")
            for name, _ in self.entries:
                out[name] = float("nan")
            return out
        host = self._download()
        out["loss"] = float(host[0]) / float(host[1]) + self.model._reg_penalty()
        rows = float(host[2])
        for name, _ in self.entries:
            if name in self.slots:
                out[name] = float(host[2 + self.slots[name]]) / rows if rows else 0.0
            else:
                out[name] = self.host_sums[name] / self.host_rows if self.host_rows else 0.0
        return out


class _Prefetcher(object):
    """One background thread draining a (non thread-safe) generator into a bounded queue, like Keras'
    GeneratorEnqueuer with workers=1."""

    def __init__(self, iterator, max_queue_size=10):
        import queue
        import threading
        self.q = queue.Queue(maxsize=max(1, int(max_queue_size)))
        self.stop = threading.Event()

        def work():
            try:
                while not self.stop.is_set():
                    item = next(iterator)
                    while not self.stop.is_set():
                        try:
                            self.q.put(("item", item), timeout=0.1)
                            break
                        except queue.Full:
                            pass
            except StopIteration:
                self.q.put(("end", None))
            except BaseException as e:   # surfaces in the training thread
                self.q.put(("error", e))

        self.thread = threading.Thread(target=work, daemon=True)
        self.thread.start()

    def get(self):
        kind, item = self.q.get()
        if kind == "error":
            raise item
        if kind == "end":
            raise StopIteration
        return item

    def close(self):
        """Stop the thread and wait for it (a generator must not be resumed by two threads); batches it had already
        produced are dropped, as Keras' enqueuer does on stop()."""
        import queue
        self.stop.set()
        try:                      # a producer blocked on the full queue would only notice `stop` after its put timeout
            while True:
                self.q.get_nowait()
        except queue.Empty:
            pass
        self.thread.join()


def load_model(filepath, custom_objects=None, compile=True):
    raise NotImplementedError(
        "load_model needs the HDF5 architecture blob Keras writes; rebuild the model with its builder and call "
        "load_weights(path, by_name=True) (what the reference does right after load_model, "
        "localisation_part/training_dct_pascal_j2d_resnet.py:137-149)")
