"""The VGG-DCT SSD300 (`ssd_300DCT`, `ssd_300DCT_no_reg`) on the GPU.

The model adds no kernel, so the first part runs the existing launchers once at each geometry they meet here for the
first time -- rows of 1444 and 361 pixels per image are no multiple of a tile -- against oracle.keras_ops in float64, in
the default fp32 mix, with fp32 MFMAs only and in float16 mode.  Tolerances are the ones the existing kernel tests apply
to the same launch kind: tests/test_conv_gpu.py's `_tol` (1e-3 of the largest reference magnitude + 1e-5) in both fp32
modes, tests/test_lowp_gpu.py's relative L2 bounds (1.5e-3 forward, 8e-3 gradients) in float16 mode, tests/test_kernels_gpu.py's
`close` for L2Normalization and pooling, whose results do not depend on the mode.

The second part is the whole graph: one training step at batch 2 against an oracle written here from
oracle.ssd_resnet_dct.Net and oracle.keras_ops (computed once per process in float64 and float32 and shared), the
unregularised twin, the two inference modes, the by-name transfer from a VGG-DCT classifier checkpoint, the arithmetic
modes, both entry scripts as child processes, and one step at the full batch of 32.

Decision margins.  tests/test_vgg_dct_gpu.py picks a batch for which no ReLU input and no pooling window of the fp64
oracle is closer to a tie than fp32 arithmetic can resolve.  At full size that cannot be had: this graph takes 8.1 M ReLU
decisions per batch of 2, and with a resolution of sqrt(9 * 640) * 2^-24 = 4.5e-6 of a layer's root-mean-square 21 to 35
of them fall inside it for each of the seeds 1234 .. 1239.  What does differ between those batches is how much of the
graph they train: a predictor pair only receives a gradient when an anchor of its map is matched or mined, and the extra
layers behind the last such map receive none.  BATCH_SEED is the one of the six that reaches the most parameter tensors
in the fp64 oracle (evaluated on the CPU: 47 of 63 with 8 of the 12 head kernels and matched boxes on four maps, conv7_1 /
conv7_2 included; the others reach 31 .. 45, with 4 .. 7 head kernels); its margins (`decision_margins`) are 0.049 for
ReLU and 0.11 for pooling, with 35 ReLU inputs inside the bound (the others: 0.013 .. 0.11, 0.030 .. 0.38, 21 .. 33);
the test prints both margins and that count, and the gradient criterion of
tests/test_ssd_gpu.py (`check_gradients_and_update`) measures every tensor against the fp64 oracle with the fp32 oracle's
own deviation as the scale, which is what a flipped unit costs any fp32 evaluation."""
import functools
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import keras_ops as ko

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["float32", "float32_mfma", "float16"]
SOURCES = ["conv4_3_norm", "fc7", "conv6_2", "conv7_2", "conv8_2", "conv9_2"]
BATCH = 2
BATCH_SEED = 1234


@pytest.fixture()
def floatx():
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    yield K
    K.set_floatx("float32")


# =====================================================================================================================
# 1. the launchers at the new geometries
# =====================================================================================================================
# name -> (H = W, Cin, Cout, real filters, dilation, ReLU epilogue).  The fused predictor heads run as one GEMM over the
# conf | loc filter banks side by side, zero-padded to a multiple of 32 columns (Conv2D._lower_fused): 84 + 16 -> 128,
# 126 + 24 -> 160.
CONV_CASES = {
    "conv1_1_dct_256": (38, 64, 256, 256, 1, True),
    "conv4_1": (38, 256, 512, 512, 1, True),
    "conv4_2": (38, 512, 512, 512, 1, True),                 # = conv4_3
    "conv5_1": (19, 640, 512, 512, 1, True),
    "conv5_2": (19, 512, 512, 512, 1, True),                 # = conv5_3
    "fc6": (19, 512, 1024, 1024, 6, True),
    "conv4_3_norm_heads": (38, 512, 128, 100, 1, False),
    "fc7_heads": (19, 1024, 160, 150, 1, False),
}


@functools.lru_cache(maxsize=None)
def conv_reference(name, batch):
    """Operands (float32) and the float64 results of one convolution: computed once, shared by the three modes."""
    hw, ci, co, real, dil, _ = CONV_CASES[name]
    g = torch.Generator().manual_seed(1234 + batch)
    x = torch.randn(batch, hw, hw, ci, generator=g)
    wt = torch.randn(3, 3, ci, co, generator=g) * (2.0 / (9 * ci)) ** 0.5
    bias = torch.randn(co, generator=g)
    dy = torch.randn(batch, hw, hw, co, generator=g)
    wt[..., real:] = 0.0            # padding columns of a fused launch: zero filters, zero bias, zero gradient
    bias[real:] = 0.0
    dy[..., real:] = 0.0
    xr, wr = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    yr = ko.conv2d(xr, wr, bias.double(), (1, 1), "same", (dil, dil))
    yr.backward(dy.double())
    return x, wt, bias, dy, yr.detach(), xr.grad, wr.grad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_at_the_new_geometries(name, batch, mode, cuda, floatx):
    from jpeg_detection_resnet_ssd_amd import kernels as Kn
    from test_conv_gpu import _tol
    from test_lowp_gpu import rel_l2
    hw, ci, co, real, dil, relu = CONV_CASES[name]
    x, wt, bias, dy, yr, dxr, dwr = conv_reference(name, batch)
    desc = Kn.make_conv_desc(batch, hw, hw, ci, co, (3, 3), (1, 1), "same", (dil, dil))
    assert (desc.out_h, desc.out_w) == (hw, hw) and (batch * hw * hw) % 64 != 0
    xd, wd, bd, dyd = x.to(cuda), wt.to(cuda), bias.to(cuda), dy.to(cuda)
    y = torch.full(yr.shape, float("nan"), device=cuda)
    dx = torch.full(x.shape, float("nan"), device=cuda)
    dw = torch.full(wt.shape, float("nan"), device=cuda)
    floatx.set_floatx(mode)
    Kn.conv2d_fwd(desc, xd, wd, bd, y, None, None, False, relu)
    Kn.conv2d_dgrad(desc, dyd, wd, dx)
    Kn.conv2d_wgrad(desc, xd, dyd, dw)
    torch.cuda.synchronize()
    floatx.set_floatx("float32")
    want_y = torch.relu(yr) if relu else yr
    got = (y.cpu().double(), dx.cpu().double(), dw.cpu().double())
    errs = tuple(rel_l2(a, b) for a, b in zip(got, (want_y, dxr, dwr)))
    print("%s batch %d %s: rel-L2 fwd %.2e dgrad %.2e wgrad %.2e" % ((name, batch, mode) + errs))
    assert all(bool(torch.isfinite(t).all()) for t in got)
    if mode == "float16":
        assert errs[0] <= 1.5e-3 and errs[1] <= 8e-3 and errs[2] <= 8e-3, errs
        assert min(errs) > 1e-5, errs                  # the reduced-precision kernels did run (tests/test_lowp_gpu.py)
    else:
        for a, b in zip(got, (want_y, dxr, dwr)):
            assert float((a - b).abs().max()) <= _tol(b), errs
    assert float(got[2][..., real:].abs().max()) == 0.0 if real < co else True


POOL_CASES = {"pool4": (38, 2, 2, 0), "pool5_ssd": (19, 3, 1, 1)}       # H = W, window, stride, padding before


@functools.lru_cache(maxsize=None)
def pool_reference(name, batch):
    import torch.nn.functional as F
    hw, k, s, p = POOL_CASES[name]
    g = torch.Generator().manual_seed(77 + batch)
    x = torch.relu(torch.randn(batch, hw, hw, 512, generator=g))       # behind a ReLU: exact ties, first maximum wins
    xr = x.double().requires_grad_(True)
    yr = ko.max_pool(xr, (k, k), (s, s)) if name == "pool4" else ko.max_pool_3x3_s1_same(xr)
    dy = torch.randn(yr.shape, generator=g)
    yr.backward(dy.double())
    # the oracle's arg-max as the kernel encodes it: position inside the window, row-major
    _, idx = F.max_pool2d(x.double().permute(0, 3, 1, 2), (k, k), (s, s), padding=p, return_indices=True)
    idx = idx.permute(0, 2, 3, 1)                                       # (B, OH, OW, C) flat h * W + w
    oh = torch.arange(yr.shape[1]).view(1, -1, 1, 1)
    ow = torch.arange(yr.shape[2]).view(1, 1, -1, 1)
    code = (idx // hw - (oh * s - p)) * k + (idx % hw - (ow * s - p))
    return x, dy, yr.detach(), xr.grad, code.to(torch.uint8)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("name", list(POOL_CASES))
def test_pooling_at_the_new_geometries(name, batch, mode, cuda, floatx):
    from jpeg_detection_resnet_ssd_amd import engine as E
    from test_kernels_gpu import close
    hw, k, s, p = POOL_CASES[name]
    x, dy, yr, dxr, code = pool_reference(name, batch)
    oh = yr.shape[1]
    assert oh == 19
    floatx.set_floatx(mode)
    y = torch.full(yr.shape, float("nan"), device=cuda)
    am = torch.full((yr.numel(),), 250, dtype=torch.uint8, device=cuda)
    dx = torch.full(x.shape, float("nan"), device=cuda)
    E.call("dj_maxpool2d_fwd", x.to(cuda), y, batch, hw, hw, 512, oh, oh, k, k, s, s, p, p, 0, am)
    E.call("dj_maxpool2d_bwd", None, dy.to(cuda), dx, batch, hw, hw, 512, oh, oh, k, k, s, s, p, p, 0, 0, am)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().double(), yr)
    assert torch.equal(am.cpu().view(code.shape), code)
    assert close(dx, dxr, rel=1e-5)


@functools.lru_cache(maxsize=None)
def two_reader_reference(batch):
    """conv4_3's output x with its two readers, pool4 and conv4_3_norm: d loss / dx is the sum of both paths."""
    g = torch.Generator().manual_seed(8 + batch)
    x = torch.relu(torch.randn(batch, 38, 38, 512, generator=g)) * 4
    gamma = torch.rand(512, generator=g) * 5 + 18
    xr, gr = x.double().requires_grad_(True), gamma.double().requires_grad_(True)
    y_norm = ko.l2_normalization(xr, gr)
    y_pool = ko.max_pool(xr, (2, 2), (2, 2))
    dy_norm = torch.randn(y_norm.shape, generator=g)
    dy_pool = torch.randn(y_pool.shape, generator=g)
    ((y_norm * dy_norm.double()).sum() + (y_pool * dy_pool.double()).sum()).backward()
    return x, gamma, dy_norm, dy_pool, y_norm.detach(), xr.grad, gr.grad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("batch", [1, 2])
def test_l2norm_and_pool_gradients_accumulate(batch, mode, cuda, floatx):
    """L2Normalization at C = 512 forward and backward, and the gradient of a tensor with two readers: the later layer's
    backward pass runs first and writes (beta 0), the earlier one's adds to it (beta 1), as Plan.grad_of hands them out."""
    from jpeg_detection_resnet_ssd_amd import engine as E
    from test_kernels_gpu import close
    x, gamma, dy_norm, dy_pool, yr, dxr, dgr = two_reader_reference(batch)
    rows, c = batch * 38 * 38, 512
    floatx.set_floatx(mode)
    xd, gd = x.to(cuda), gamma.to(cuda)
    y, rn = torch.full(x.shape, float("nan"), device=cuda), torch.empty(rows, device=cuda)
    E.call("dj_l2norm_fwd", xd, c, gd, y, c, rn, rows, c)
    nr = E.query("dj_reduce_rows", rows)
    part = torch.empty(nr, 2, c, device=cuda)
    dx, dg = torch.full(x.shape, float("nan"), device=cuda), torch.empty(c, device=cuda)
    E.call("dj_l2norm_bwd", dy_norm.to(cuda), c, xd, c, gd, rn, dx, c, part, rows, c, 0)
    E.call("dj_colreduce_finalize", part, nr, c, 0, dg, 0)
    yp = torch.empty(batch, 19, 19, c, device=cuda)
    am = torch.empty(yp.numel(), dtype=torch.uint8, device=cuda)
    E.call("dj_maxpool2d_fwd", xd, yp, batch, 38, 38, c, 19, 19, 2, 2, 2, 2, 0, 0, 0, am)
    E.call("dj_maxpool2d_bwd", None, dy_pool.to(cuda), dx, batch, 38, 38, c, 19, 19, 2, 2, 2, 2, 0, 0, 0, 1, am)
    torch.cuda.synchronize()
    assert close(y, yr) and close(dx, dxr) and close(dg, dgr)


# =====================================================================================================================
# 2. the graph
# =====================================================================================================================
def vgg_ssd_forward(w, inputs, training=True, taps=None):
    """`ssd_300DCT` restated on the oracle's operations -> (y_pred (B, 8732, 33), Net).  `taps` receives ("relu",
    pre-activation) of every ReLU and ("pool2" | "pool3", input) of the two pooling layers."""
    from oracle.ssd_resnet_dct import TRAIN_SSD_ARGS as cfg, Net, anchor_boxes
    net = Net(w, training)

    def conv(t, name, reg=False, **kw):
        z = net.conv(t, name, reg=reg, **kw)
        if taps is not None:
            taps.append(("relu", z.detach()))
        return ko.relu(z)

    def pool(t, kind):
        if taps is not None:
            taps.append((kind, t.detach()))
        return ko.max_pool(t, (2, 2), (2, 2)) if kind == "pool2" else ko.max_pool_3x3_s1_same(t)

    y_in, cbcr_in = inputs
    cbcr = net.bn(cbcr_in, "b_norm_128")
    t = net.bn(y_in, "b_norm_64")
    t = conv(t, "conv1_1_dct_256", padding="same")
    t = conv(t, "conv4_1", padding="same")
    t = conv(t, "conv4_2", padding="same")
    conv4_3 = conv(t, "conv4_3", padding="same")
    t = torch.cat([pool(conv4_3, "pool2"), cbcr], dim=-1)
    for i in (1, 2, 3):
        t = conv(t, "conv5_%d" % i, padding="same")
    t = pool(t, "pool3")
    fc6 = conv(t, "fc6", reg=True, padding="same", dilation=(6, 6))
    fc7 = conv(fc6, "fc7", reg=True, padding="same")
    t = ko.zero_padding(conv(fc7, "conv6_1", reg=True, padding="same"), ((1, 1), (1, 1)))
    c62 = conv(t, "conv6_2", reg=True, strides=(2, 2))
    t = ko.zero_padding(conv(c62, "conv7_1", reg=True, padding="same"), ((1, 1), (1, 1)))
    c72 = conv(t, "conv7_2", reg=True, strides=(2, 2))
    c82 = conv(conv(c72, "conv8_1", reg=True, padding="same"), "conv8_2", reg=True)
    c92 = conv(conv(c82, "conv9_1", reg=True, padding="same"), "conv9_2", reg=True)
    sources = [ko.l2_normalization(conv4_3, w["conv4_3_norm/conv4_3_norm_gamma"]), fc7, c62, c72, c82, c92]
    n_cls, b = cfg["n_classes"] + 1, y_in.shape[0]
    confs, locs, pris = [], [], []
    for i, s in enumerate(sources):
        c = net.conv(s, "%s_mbox_conf_%d" % (SOURCES[i], n_cls), padding="same", reg=True)
        l = net.conv(s, "%s_mbox_loc" % SOURCES[i], padding="same", reg=True)
        confs.append(c.reshape(b, -1, n_cls))
        locs.append(l.reshape(b, -1, 4))
        a = anchor_boxes(s.shape[1], s.shape[2], cfg["scales"][i], cfg["scales"][i + 1], cfg["aspect_ratios"][i],
                         cfg["steps"][i], cfg["offsets"][i], cfg)
        pris.append(torch.from_numpy(a).to(c.dtype).reshape(1, -1, 8).expand(b, -1, -1))
    conf = ko.softmax(torch.cat(confs, dim=1))
    return torch.cat([conf, torch.cat(locs, dim=1), torch.cat(pris, dim=1)], dim=2), net


def decision_margins(taps):
    """-> (smallest |ReLU input|, smallest gap between the two largest entries of a pooling window with a positive maximum,
    number of ReLU inputs closer to zero than the bound), the first two in units of the bound sqrt(9 * 640) * 2^-24 times
    the tensor's root-mean-square (see the module docstring)."""
    import torch.nn.functional as F
    bound = (9 * 640) ** 0.5 * 2.0 ** -24
    relu_margin = pool_margin = float("inf")
    inside = 0
    for kind, t in taps:
        rms = float(t.double().pow(2).mean().sqrt())
        if kind == "relu":
            relu_margin = min(relu_margin, float(t.abs().min()) / (bound * rms))
            inside += int((t.abs() < bound * rms).sum())
        else:
            k, s, p = (2, 2, 0) if kind == "pool2" else (3, 1, 1)
            win = F.unfold(F.pad(t.permute(0, 3, 1, 2), (p, p, p, p), value=float("-inf")), k, stride=s)
            win = win.reshape(t.shape[0], t.shape[3], k * k, -1)
            top = win.topk(2, dim=2).values
            gaps = (top[:, :, 0] - top[:, :, 1])[top[:, :, 0] > 0]
            pool_margin = min(pool_margin, float(gaps.min()) / (bound * rms))
    return relu_margin, pool_margin, inside


def perturbed(w0, seed=3):
    """Random biases and BatchNormalization betas / gammas (Keras starts them at 0 / 1), as test_ssd_gpu.perturb_weights
    draws them; L2Normalization's gamma keeps its 20."""
    g = torch.Generator().manual_seed(seed)
    d = dict(w0)
    for k in list(d):
        if k.endswith("/bias") or k.endswith("/beta"):
            d[k] = (torch.randn(d[k].shape, generator=g) * 0.1).numpy()
        elif k.endswith("/gamma"):
            d[k] = (1.0 + 0.2 * torch.randn(d[k].shape, generator=g)).numpy()
    return d


def oracle_step(w0, x, y_true, dt, taps=None):
    """One train_on_batch of training_dct_pascal_j2d.py with --reg: SSDLoss + l2 penalties, SGD(0.001, 0.9)."""
    leaf = {}
    for k, v in w0.items():
        is_state = k.endswith("moving_mean") or k.endswith("moving_variance")
        leaf[k] = torch.from_numpy(v).to(dt).requires_grad_(not is_state)
    y_pred, net = vgg_ssd_forward(leaf, [torch.from_numpy(a).to(dt) for a in x], True, taps)
    data_loss = ko.ssd_loss(torch.from_numpy(y_true).to(dt), y_pred).mean()
    reg = sum(ko.l2_penalty(leaf[k], 0.0005) for k in net.reg_kernels)
    (data_loss + reg).backward()
    grads, new_w = {}, {}
    for k, v in leaf.items():
        if v.requires_grad:
            grads[k] = v.grad.detach()
            new_w[k], _ = ko.sgd_keras_step(v.detach(), v.grad, torch.zeros_like(v), 0.001, 0.9, 0.0, 0, False)
        else:
            new_w[k] = v.detach()
    new_w.update(net.new_state)
    return dict(loss=float((data_loss + reg).detach()), data_loss=float(data_loss.detach()), reg_loss=float(reg.detach()),
                y_pred=y_pred.detach(), grads=grads, new_weights=new_w, reg_kernels=list(net.reg_kernels))


def build(name="ssd_300DCT", seed=42, **over):
    from jpeg_detection_resnet_ssd_amd import workloads
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import SGD
    from jpeg_detection_resnet_ssd_amd.keras_loss_function.keras_ssd_loss import SSDLoss
    from jpeg_detection_resnet_ssd_amd.models.keras_ssd300_dct_j2d import ssd_300DCT
    from jpeg_detection_resnet_ssd_amd.models.keras_ssd300_dct_j2d_no_regularizer import ssd_300DCT_no_reg
    K.clear_session()
    K.set_random_seed(seed)
    model = {"ssd_300DCT": ssd_300DCT, "ssd_300DCT_no_reg": ssd_300DCT_no_reg}[name](**dict(workloads.SSD_ARGS, **over))
    model.compile(optimizer=SGD(lr=0.001, momentum=0.9, decay=0.0, nesterov=False),
                  loss=SSDLoss(neg_pos_ratio=3, alpha=1.0).compute_loss)
    return model


def make_batch(batch=BATCH, seed=BATCH_SEED):
    from test_ssd_gpu import make_batch as ssd_batch
    return ssd_batch("ssd_300DCT", [(38, 38), (19, 19), (10, 10), (5, 5), (3, 3), (1, 1)], batch, seed=seed)


@functools.lru_cache(maxsize=None)
def reference():
    """(w0, x, y_true, fp64 oracle step, fp32 oracle step, decision margins): computed once, never modified."""
    model = build()
    w0 = perturbed(model.get_weights_dict())
    x, y_true = make_batch()
    taps = []
    ref = oracle_step(w0, x, y_true, torch.float64, taps)
    margins = decision_margins(taps)
    del taps
    ref32 = oracle_step(w0, x, y_true, torch.float32)
    return w0, x, y_true, ref, ref32, margins


def rel_err(a, ref):
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    return float((a - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)


def run_step(model, w0, x, y_true):
    assert model.set_weights_dict(w0, strict=True) == len(w0)
    loss = model.train_on_batch(x, y_true)
    torch.cuda.synchronize()
    plan = model._plan(BATCH, True, True)
    y_pred = plan.outputs[0].buf.cpu()
    grads = {w.key: w.grad.detach().cpu().clone() for w in model.weight_specs if w.trainable}
    return loss, plan, y_pred, grads, model.get_weights_dict()


def check_moving_statistics(ref, w0, w1):
    """tests/test_ssd_gpu.py's bound: batch mean within 1e-4 of the layer's std, batch variance within 1e-3."""
    seen = 0
    for k, v in ref["new_weights"].items():
        if k.endswith("moving_mean"):
            kv = k.replace("moving_mean", "moving_variance")
            old_m, old_v = torch.from_numpy(w0[k]).double(), torch.from_numpy(w0[kv]).double()
            bm_ref, bm_gpu = (v - 0.99 * old_m) / 0.01, (torch.from_numpy(w1[k]).double() - 0.99 * old_m) / 0.01
            bv_ref = (ref["new_weights"][kv] - 0.99 * old_v) / 0.01
            bv_gpu = (torch.from_numpy(w1[kv]).double() - 0.99 * old_v) / 0.01
            std = float(bv_ref.clamp(min=0).max()) ** 0.5
            assert float((bm_gpu - bm_ref).abs().max()) <= 1e-4 * std + 1e-6, k
            assert float((bv_gpu - bv_ref).abs().max()) <= 1e-3 * std * std + 1e-6, kv
            seen += 1
    assert seen == 2


def test_training_step_matches_oracle(cuda):
    from test_ssd_gpu import check_gradients_and_update
    w0, x, y_true, ref, ref32, margins = reference()
    print("decision margins of the fp64 oracle (batch seed %d): ReLU %.3g, pooling %.3g, ReLU inputs inside the bound: %d"
          % ((BATCH_SEED,) + margins))
    # 8.1 M ReLU inputs, of which about 0.8 * 4.5e-6 lie inside the bound when they are spread like a normal variable of
    # their layer's root-mean-square: some 30 are expected; 100 is twelve standard deviations of that count away, and a
    # batch beyond it (a dead input plane, say) is not one this comparison should be made on
    assert margins[2] <= 100, "degenerate batch: choose another BATCH_SEED"
    model = build()
    loss, plan, y_pred, grads, w1 = run_step(model, w0, x, y_true)
    e = (rel_err(y_pred[..., :21], ref["y_pred"][..., :21]), rel_err(y_pred[..., 21:25], ref["y_pred"][..., 21:25]),
         rel_err(y_pred[..., 25:], ref["y_pred"][..., 25:]), abs(model.last_step_info["data_loss"] - ref["data_loss"])
         / abs(ref["data_loss"]), abs(loss - ref["loss"]) / abs(ref["loss"]),
         abs(model.last_step_info["reg_loss"] - ref["reg_loss"]) / abs(ref["reg_loss"]))
    print("rel. error: conf %.2e loc %.2e anchors %.2e data loss %.2e loss %.2e reg. loss %.2e" % e)
    print("masked dgrads: %r" % (plan.masked_dgrads,))
    assert e[0] <= 1e-3 and e[1] <= 1e-3 and e[2] <= 1e-6
    assert e[3] <= 1e-3 and e[4] <= 1e-3 and e[5] <= 1e-3
    assert set(ref["reg_kernels"]) == {w.key for w in model.weight_specs if w.l2}
    check_gradients_and_update(grads, ref, ref32, w0, w1, reg=set(ref["reg_kernels"]), l2=0.0005)
    check_moving_statistics(ref, w0, w1)


def test_no_reg_step_is_plain_sgd_on_the_data_gradient(cuda):
    """`ssd_300DCT_no_reg` on the weights and the batch of the test above: its gradient is the oracle's without the l2
    terms, its update plain SGD on that, and the regularisation loss is 0."""
    from test_ssd_gpu import check_gradients_and_update
    w0, x, y_true, ref, ref32, _ = reference()
    model = build("ssd_300DCT_no_reg")
    assert not [w.key for w in model.weight_specs if w.l2]
    loss, plan, y_pred, grads, w1 = run_step(model, w0, x, y_true)
    assert model.last_step_info["reg_loss"] == 0.0
    assert abs(loss - ref["data_loss"]) <= 1e-3 * abs(ref["data_loss"])
    assert rel_err(y_pred[..., :25], ref["y_pred"][..., :25]) <= 1e-3

    def without_l2(r):
        g, nw = {}, dict(r["new_weights"])
        for k, v in r["grads"].items():
            w = torch.from_numpy(w0[k]).to(v.dtype)
            g[k] = v - 2 * 0.0005 * w if k in ref["reg_kernels"] else v
            nw[k], _ = ko.sgd_keras_step(w, g[k], torch.zeros_like(w), 0.001, 0.9, 0.0, 0, False)
        return dict(grads=g, new_weights=nw)

    check_gradients_and_update(grads, without_l2(ref), without_l2(ref32), w0, w1, reg=(), l2=0.0)


@pytest.mark.parametrize("mode", ["inference", "inference_fast"])
def test_inference_modes_decode_the_training_predictions(mode, cuda):
    """predict() of the inference graphs == the host decoders on the training-mode graph's predictions of the same
    weights, compared as tests/test_decode_gpu.py compares them (rows in canonical order: class exactly, confidence 1e-5,
    pixel coordinates 5e-2)."""
    from jpeg_detection_resnet_ssd_amd.ssd_encoder_decoder.ssd_output_decoder import (decode_detections,
                                                                                     decode_detections_fast)
    from test_decode_gpu import canon
    train = build()
    weights = perturbed(train.get_weights_dict())
    g = torch.Generator().manual_seed(5)
    for k in weights:                   # random init: keep exp() of the box offsets finite and the softmax unsaturated
        if "mbox_loc" in k:
            weights[k] = weights[k] * 1e-3
        elif "mbox_conf" in k and k.endswith("kernel"):
            weights[k] = weights[k] * 0.05
        elif "mbox_conf" in k:          # biases: classes that differ in confidence, background ahead
            weights[k] = torch.randn(weights[k].shape, generator=g).numpy()
    train.set_weights_dict(weights)
    x = make_batch(seed=3)[0]
    raw = train.predict(x, batch_size=BATCH)
    assert raw.shape == (BATCH, 8732, 33) and np.isfinite(raw).all()
    infer = build(mode=mode, confidence_thresh=0.3, top_k=200)
    assert infer.layers[-1].name == "decoded_predictions" and bool(infer.layers[-1].fast) == (mode == "inference_fast")
    assert infer.set_weights_dict(weights) == len(weights)
    det = infer.predict(x, batch_size=BATCH)
    assert det.shape == (BATCH, 200, 6)
    host = decode_detections if mode == "inference" else decode_detections_fast
    ref = host(raw.astype(np.float64), confidence_thresh=0.3, iou_threshold=0.45, top_k=200, img_height=300,
               img_width=300)
    for b in range(BATCH):
        got, want = canon(det[b]), canon(ref[b])
        print("%s image %d: %d detections" % (mode, b, len(want)))
        assert 0 < len(want) and got.shape == want.shape
        np.testing.assert_array_equal(got[:, 0], want[:, 0])
        np.testing.assert_allclose(got[:, 1], want[:, 1], rtol=1e-5)
        np.testing.assert_allclose(got[:, 2:], want[:, 2:], atol=5e-2)


def test_classifier_checkpoint_loads_by_name(cuda, tmp_path):
    """A `vggd_dct` checkpoint (three convolutions per block, 10 classes; the fully-connected layers 64 wide to keep the
    file small -- they are not transferred) through the trainer's --vgg check and load_weights(by_name=True)."""
    from jpeg_detection_resnet_ssd_amd import ssd_training
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.networks import vgg_dct
    K.clear_session()
    K.set_random_seed(5)
    classifier = vgg_dct(classes=10, convs_per_block=3, fc_units=64, name="vggd_dct")
    cw = perturbed(classifier.get_weights_dict(), seed=9)
    g = torch.Generator().manual_seed(10)
    for k in cw:
        if k.endswith("moving_mean") or k.endswith("moving_variance"):
            cw[k] = (torch.rand(cw[k].shape, generator=g) + 0.5).numpy()
    classifier.set_weights_dict(cw)
    path = str(tmp_path / "vggd_dct.npz")
    classifier.save_weights(path)
    del classifier
    model = build(seed=6)
    before = model.get_weights_dict()
    names = [l.name for l in model.layers]
    ignored = ssd_training.check_checkpoint_layers(ssd_training.checkpoint_layer_names(path), names, vgg=True)
    assert ignored == ["fc1", "fc2", "predictions"]
    shared = ["b_norm_64", "b_norm_128", "conv1_1_dct_256", "conv4_1", "conv4_2", "conv4_3", "conv5_1", "conv5_2", "conv5_3"]
    n_loaded = model.load_weights(path, by_name=True)
    after = model.get_weights_dict()
    assert n_loaded == 2 * 4 + 7 * 2
    for k in after:
        if k.split("/")[0] in shared:
            assert np.array_equal(after[k], cw[k]) and not np.array_equal(after[k], before[k]), k
        else:
            assert np.array_equal(after[k], before[k]), k
    with pytest.raises(NameError, match="will not be loaded: fc1$"):
        ssd_training.check_checkpoint_layers(ssd_training.checkpoint_layer_names(path), names, ssd=True)
    bad = str(tmp_path / "unknown.npz")
    with open(bad, "wb") as f:
        np.savez(f, **dict(cw, **{"conv3_3/kernel": np.zeros((3, 3, 4, 4), np.float32)}))
    with pytest.raises(NameError, match="will not be loaded: conv3_3$"):
        ssd_training.check_checkpoint_layers(ssd_training.checkpoint_layer_names(bad), names, vgg=True)


@pytest.mark.parametrize("mode,bound,compute_mode", [("float32x3", 1e-3, 3), ("float32_mfma", 1e-3, 5), ("float16", 1e-2, 1)])
def test_arithmetic_modes(mode, bound, compute_mode, cuda, floatx):
    """One step per mode against the fp64 oracle: loss within the bound the mode gets for the ResNet detectors (1e-3 in
    tests/test_x3_gpu.py, 1e-2 for float16 in tests/test_lowp_gpu.py).  float16: which tensors of the plan are held in 16
    bits is listed; the BatchNormalization-free convolution chains are fp32."""
    w0, x, y_true, ref, _, _ = reference()
    model = build()
    floatx.set_floatx(mode)
    loss, plan, y_pred, grads, w1 = run_step(model, w0, x, y_true)
    floatx.set_floatx("float32")
    assert plan.compute_mode == compute_mode and plan.store16 == (mode == "float16")
    e_loss = abs(loss - ref["loss"]) / abs(ref["loss"])
    print("%s: loss rel. error %.2e, predictions max-norm %.2e" % (mode, e_loss, rel_err(y_pred, ref["y_pred"])))
    assert np.isfinite(loss) and e_loss <= bound
    assert max(float(np.abs(w1[k] - w0[k]).max()) for k in w0) > 0
    by_name = {}
    for lyr in model.layers:
        v = plan.values.get(id(lyr.outbound[0]))
        if v is not None and getattr(v, "buf", None) is not None:
            by_name[lyr.name] = v.buf.dtype
    narrow = sorted(n for n, dt in by_name.items() if dt != torch.float32)
    print("%s: 16-bit tensors: %r" % (mode, narrow))
    for n in ("conv1_1_dct_256", "conv4_1", "conv4_2", "conv4_3", "conv5_1", "conv5_2", "conv5_3", "fc6", "fc7", "conv6_2",
              "conv7_2", "conv8_2", "conv9_2", "conv4_3_norm", "pool4", "pool5_ssd", "predictions_ssd"):
        assert by_name[n] == torch.float32, n
    if mode != "float16":
        assert not narrow


def _child(args, env, timeout=600):
    r = subprocess.run([sys.executable] + args, capture_output=True, text=True, env=env, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r


def test_entry_scripts_end_to_end(cuda, tmp_path):
    env = dict(os.environ, LOCAL_WORK_DIR=str(tmp_path), EXPERIMENTS_OUTPUT_DIRECTORY=str(tmp_path / "out"),
               DJ_AUTOTUNE="table")
    env.pop("WORLD_SIZE", None)
    env.pop("DATASET_PATH", None)
    common = ["-vd", "0", "--vgg", "--crop", "--p07", "--epochs", "1", "--steps_per_epoch", "2", "--batch_size", "2",
              "--synthetic_images", "8"]
    trainer = os.path.join(ROOT, "training_dct_pascal_j2d.py")
    r = _child([trainer, "--reg"] + common, env)
    assert "Epoch 1/1" in r.stdout
    ckpts = sorted(glob.glob(str(tmp_path / "out" / "ssd300_pascal_07+12_epoch-*.h5")))
    assert len(ckpts) == 1, os.listdir(tmp_path / "out")
    r = _child([os.path.join(ROOT, "evaluation.py"), ckpts[0], "-sd", "--synthetic_images", "4", "--batch_size", "2"], env)
    assert [ln for ln in r.stdout.splitlines() if ln.split()[:1] == ["mAP"]], r.stdout[-1500:]
    # the detector's own checkpoint passes the --ssd check and loads
    env2 = dict(env, EXPERIMENTS_OUTPUT_DIRECTORY=str(tmp_path / "out2"))
    r = _child([trainer, "--no_reg", "--weights", ckpts[0]] + ["--ssd" if a == "--vgg" else a for a in common], env2)
    assert "Epoch 1/1" in r.stdout and glob.glob(str(tmp_path / "out2" / "*.h5"))


def generic_kernel_reason(direction, desc):
    """Why the launcher would take the generic kernel for this launch instead of the branch-free one, which alone has the
    split-bf16 and 16-bit variants (csrc/dj_conv_launch.h `fast_mode`: a tile index that names such a variant quietly runs
    its fp32 twin where a precondition fails) -- or None.  Stated on the descriptor; the remaining precondition, 16-byte
    aligned tensors, holds for every buffer a plan allocates."""
    d, kind = desc, direction & 3
    if d.batch * max(d.out_h * d.out_w, d.in_h * d.in_w) >= 1 << 22:
        return "rows"
    if d.in_c % 4 or d.ld_x % 4 or d.out_c % 4 or d.ld_y % 4:
        return "channels or pixel strides that are no multiple of 4"
    if kind == 0 and d.in_c % 32:
        return "forward: in_c % 32"
    if kind == 1 and d.out_c % 32:
        return "input gradient: out_c % 32"
    if kind == 1 and (d.stride_h, d.stride_w) != (1, 1):
        return "input gradient: stride"
    return None


def test_full_size_step(cuda):
    """One step at the trainer's batch of 32: finite loss, and no GEMM of the plan outside the branch-free kernels'
    preconditions except the two 3x3 stride-2 input gradients (conv6_2, conv7_2), which take the generic kernel in every
    SSD300 of this package."""
    from jpeg_detection_resnet_ssd_amd import workloads
    model, sizes = workloads.build_ssd("ssd_300DCT")
    x, y = workloads.synthetic_batch("ssd_300DCT", sizes, 32, fast=True)
    loss = model.train_on_batch(x, y)
    torch.cuda.synchronize()
    plan = model._plan(32, True, True)
    info = model.last_step_info
    print("batch 32: loss %.4f (data %.4f, regularisation %.4f), %d GEMM launches" % (loss, info["data_loss"],
                                                                                       info["reg_loss"], len(plan.conv_calls)))
    assert np.isfinite(loss) and loss > 0 and info["reg_loss"] > 0
    assert torch.isfinite(model.flat_gradients).all() and float(model.flat_gradients.abs().max()) > 0
    generic = [(direction, (d.in_h, d.in_c, d.out_c, d.kernel_h, d.stride_h), generic_kernel_reason(direction, d))
               for direction, d, _ in plan.conv_calls if generic_kernel_reason(direction, d)]
    print("launches on the generic kernel (direction, (H, Cin, Cout, k, stride), why): %r" % (generic,))
    assert sorted(g[:2] for g in generic) == [(1, (10, 128, 256, 3, 2)), (1, (19, 256, 512, 3, 2))], generic
    # the check can fail: an unpadded head pair (84 + 16 filters) would leave the branch-free input gradient
    from jpeg_detection_resnet_ssd_amd import kernels as Kn
    assert generic_kernel_reason(1, Kn.make_conv_desc(32, 38, 38, 512, 100, (3, 3), (1, 1), "same", (1, 1)))
    widths = sorted(d.out_c for direction, d, _ in plan.conv_calls if direction == 0 and d.out_c not in (128, 256, 512, 1024))
    assert widths == [160, 160, 160], widths          # 126 + 24 filters padded; the 84 + 16 pairs make 128
    beside = sorted(lyr.name for lyr in model.layers
                    if getattr(plan.values.get(id(lyr.outbound[0])), "side_done", None) is not None)
    print("masked dgrads: %r" % (plan.masked_dgrads,))
    print("forward launches on the side stream write: %r" % (beside,))
    assert len(plan.fused_outputs) == 12            # six conf | loc pairs, one GEMM per pair
    # 17 convolutions + 6 fused head pairs: one forward and one weight-gradient GEMM each
    kinds = [d & 3 for d, _, _ in plan.conv_calls]
    assert kinds.count(0) == 17 + 6 and kinds.count(2) == 17 + 6 and kinds.count(1) >= 17 + 6 - 1
    del model
    torch.cuda.empty_cache()
