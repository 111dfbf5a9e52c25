"""Layer-group parity at the strict 1e-3 bound: ResNet bottleneck blocks (conv -> BN -> ReLU chains with
the BatchNormalization folded into the next conv's load, residual Add+ReLU), the deconv / up-sampling
input stages and the SSD prediction assembly, forward AND backward from an externally supplied
output gradient, against the fp64 CPU oracle.  Batch 4 on 19x19 maps keeps every gradient
well-conditioned (cf. tests/test_ssd_gpu.py for why the full batch-2 graph is not)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel_err(a, ref):
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    return float((a - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)


def _perturb(model, seed=3):
    g = torch.Generator().manual_seed(seed)
    d = model.get_weights_dict()
    for k in list(d):
        if k.endswith("/bias") or k.endswith("/beta"):
            d[k] = (torch.randn(d[k].shape, generator=g) * 0.1).numpy()
        elif k.endswith("/gamma"):
            d[k] = (1.0 + 0.2 * torch.randn(d[k].shape, generator=g)).numpy()
    model.set_weights_dict(d)
    return d


def _run(model, xs, dy, cuda):
    b = xs[0].shape[0]
    plan = model._plan(b, True, False, external_grad=True)
    model._upload(plan, xs, None)
    plan.external_grad.copy_(torch.from_numpy(dy))
    plan.run_forward()
    plan.run_backward()
    torch.cuda.synchronize()
    grads = {w.key: w.grad.detach().cpu().clone() for w in model.weight_specs if w.trainable}
    return plan.outputs[0].buf.cpu(), grads, model.get_weights_dict()


def rel_l2(a, ref):
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    return float((a - ref).norm()) / (float(ref.norm()) + 1e-30)


def _check(out, grads, ref_out, ref_grads, tol=1e-3):
    """Forward in max-norm at 1e-3; gradients in relative L2 norm at 2e-3 plus a loose 5e-2 max-norm bound.
    Max-norm alone is not a stable criterion for gradients: one ReLU whose pre-activation is ~1e-7
    (it happens for roughly one element in 10^6) is clamped on one side and not on the other, which
    moves single gradient entries by a few 1e-3 of the tensor's maximum in ANY two fp32 runs, while
    every other entry agrees to ~1e-6 (measured; see DESIGN.md 'parity')."""
    assert rel_err(out, ref_out) <= tol
    gmax = max(float(v.abs().max()) for v in ref_grads.values())
    bad = []
    for k, gref in ref_grads.items():
        scale = float(gref.abs().max())
        if scale <= 1e-6 * gmax:      # analytically-zero gradients (conv bias / beta in front of a BN)
            if float(grads[k].abs().max()) > 1e-5 * gmax:
                bad.append((k, "nonzero", float(grads[k].abs().max())))
            continue
        e2, emax = rel_l2(grads[k], gref), rel_err(grads[k], gref)
        if e2 > 2 * tol or emax > 5e-2:
            bad.append((k, e2, emax))
    assert not bad, bad


@pytest.mark.parametrize("kind", ["conv_s1_k1", "conv_s2_k3", "identity_k2", "identity_k3", "conv_s2_k3+autotune"])
def test_bottleneck_blocks(kind, cuda, monkeypatch):
    if kind.endswith("+autotune"):
        # the production path for geometries the in-tree table does not hold: every tile variant is timed at plan time
        # (on garbage buffers; the timed launches write no weight or BatchNormalization state) and the fastest one is used
        monkeypatch.setenv("DJ_AUTOTUNE", "1")
        kind = kind[:-len("+autotune")]
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras.layers import BatchNormalization, Input
    from jpeg_detection_resnet_ssd_amd.keras.models import Model
    from jpeg_detection_resnet_ssd_amd.models.resnet_dct_blocks import conv_block, identity_block
    from oracle import ssd_resnet_dct as oracle
    K.clear_session()
    K.set_random_seed(5)
    b, hw, cin = 4, 19, 128
    inp = Input((hw, hw, cin))
    x = BatchNormalization()(inp)            # input BN folded into the first convs, like the DCT inputs
    x = conv_block(x, 3, [64, 64, 128], stage=9, block="p", strides=(1, 1))
    if kind == "conv_s1_k1":
        y = conv_block(x, 1, [64, 64, 192], stage=1, block="a", strides=(1, 1))
    elif kind == "conv_s2_k3":
        y = conv_block(x, 3, [64, 64, 192], stage=1, block="a")
    elif kind == "identity_k2":
        y = identity_block(x, 2, [64, 64, 128], stage=1, block="a")
    else:
        y = identity_block(x, 3, [64, 64, 128], stage=1, block="a")
    model = Model(inp, y)
    w0 = _perturb(model)
    g = torch.Generator().manual_seed(1)
    xin = (torch.randn(b, hw, hw, cin, generator=g) * 20).numpy()
    dy = torch.randn(b, *model.outputs[0].shape[1:], generator=g).numpy()
    out, grads, w1 = _run(model, [xin], dy, cuda)

    wt = {k: torch.from_numpy(v).double().requires_grad_(not k.endswith(("moving_mean", "moving_variance")))
          for k, v in w0.items()}
    net = oracle.Net(wt, True)
    t = net.bn(torch.from_numpy(xin).double())
    t = net.conv_block(t, 3, 9, "p", (1, 1))
    if kind == "conv_s1_k1":
        ref = net.conv_block(t, 1, 1, "a", (1, 1))
    elif kind == "conv_s2_k3":
        ref = net.conv_block(t, 3, 1, "a")
    else:
        ref = net.identity_block(t, 2 if kind == "identity_k2" else 3, 1, "a")
    ref.backward(torch.from_numpy(dy).double())
    _check(out, grads, ref.detach(), {k: v.grad for k, v in wt.items() if v.grad is not None})
    for k, v in net.new_state.items():
        assert rel_err(w1[k], v) <= 1e-3, k


@pytest.mark.parametrize("archi", ["deconv", "up_sampling"])
def test_chroma_fusion_stage(archi, cuda):
    """Conv2DTranspose x2 (or UpSampling2D) -> Concatenate -> BatchNormalization(192) -> first RFA conv block."""
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras.layers import (BatchNormalization, Concatenate, Conv2DTranspose, Input,
                                                            UpSampling2D)
    from jpeg_detection_resnet_ssd_amd.keras.models import Model
    from jpeg_detection_resnet_ssd_amd.models.resnet_dct_blocks import conv_block
    from oracle import keras_ops as ko
    from oracle import ssd_resnet_dct as oracle
    K.clear_session()
    K.set_random_seed(6)
    b, gsz = 3, 38
    g = torch.Generator().manual_seed(2)
    iy = Input((gsz, gsz, 64))
    if archi == "deconv":
        icb, icr = Input((gsz // 2, gsz // 2, 64)), Input((gsz // 2, gsz // 2, 64))
        cb = Conv2DTranspose(64, 2, strides=(2, 2))(icb)
        cr = Conv2DTranspose(64, 2, strides=(2, 2))(icr)
        cat = Concatenate(axis=-1)([iy, Concatenate(axis=-1)([cb, cr])])
        ins = [iy, icb, icr]
        xs = [(torch.randn(b, gsz, gsz, 64, generator=g) * 30).numpy(),
              (torch.randn(b, gsz // 2, gsz // 2, 64, generator=g) * 10).numpy(),
              (torch.randn(b, gsz // 2, gsz // 2, 64, generator=g) * 10).numpy()]
    else:
        icc = Input((gsz // 2, gsz // 2, 128))
        cat = Concatenate(axis=-1)([iy, UpSampling2D()(icc)])
        ins = [iy, icc]
        xs = [(torch.randn(b, gsz, gsz, 64, generator=g) * 30).numpy(),
              (torch.randn(b, gsz // 2, gsz // 2, 128, generator=g) * 10).numpy()]
    x = BatchNormalization(input_shape=(gsz, gsz, 64))(cat)
    y = conv_block(x, 1, [64, 64, 128], stage=4, block="a2", strides=(1, 1))
    model = Model(ins, y)
    w0 = _perturb(model)
    dy = torch.randn(b, gsz, gsz, 128, generator=g).numpy()
    out, grads, _ = _run(model, xs, dy, cuda)

    wt = {k: torch.from_numpy(v).double().requires_grad_(not k.endswith(("moving_mean", "moving_variance")))
          for k, v in w0.items()}
    net = oracle.Net(wt, True)
    tx = [torch.from_numpy(a).double() for a in xs]
    if archi == "deconv":
        c = torch.cat([tx[0], torch.cat([net.deconv2x(tx[1]), net.deconv2x(tx[2])], dim=-1)], dim=-1)
    else:
        c = torch.cat([tx[0], ko.upsampling_nearest_2x(tx[1])], dim=-1)
    ref = net.conv_block(net.bn(c), 1, 4, "a2", (1, 1))
    ref.backward(torch.from_numpy(dy).double())
    _check(out, grads, ref.detach(), {k: v.grad for k, v in wt.items() if v.grad is not None})
