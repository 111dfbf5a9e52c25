"""Lowering of the ReLU mask of a residual block's output into the input-gradient GEMM that completes the block output's
gradient (keras/layers.py `_relu_mask_in_dgrad`, DJ_MASK_IN_DGRAD): a chain of one conv-shortcut and two identity bottleneck
blocks, lowered with the knob on and off.  The same values are masked by the same predicate and every sum runs over the same
numbers in the same order, so the two plans must agree exactly on the chain's input gradient, on every BatchNormalization's
dgamma / dbeta and on every dz; the weight gradients (which may be summed with atomics) within the bound
tests/test_blocks_gpu.py applies to them.  The plan with the knob on must really contain masked input gradients, and no
BatchNormalization of a block whose output gradient is pre-masked may read the block output (mask_mode 1)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rel_l2(a, ref):
    a, ref = a.double(), ref.double()
    return float((a - ref).norm()) / (float(ref.norm()) + 1e-30)


def _rel_max(a, ref):
    a, ref = a.double(), ref.double()
    return float((a - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)


def _lower_and_run(knob, monkeypatch):
    from jpeg_detection_resnet_ssd_amd import kernels as Kn
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras.layers import BatchNormalization, Conv2D, Input
    from jpeg_detection_resnet_ssd_amd.keras.models import Model
    from jpeg_detection_resnet_ssd_amd.models.resnet_dct_blocks import conv_block, identity_block
    from test_blocks_gpu import _perturb
    monkeypatch.setenv("DJ_MASK_IN_DGRAD", knob)
    K.clear_session()
    K.set_random_seed(5)
    b, hw, cin = 2, 9, 128
    inp = Input((hw, hw, cin))
    x0 = BatchNormalization()(inp)
    x = conv_block(x0, 3, [32, 32, 128], stage=1, block="a", strides=(1, 1))
    x = identity_block(x, 3, [32, 32, 128], stage=1, block="b")
    y = identity_block(x, 3, [32, 32, 128], stage=1, block="c")
    model = Model(inp, y)
    _perturb(model)
    # mask_mode of every BatchNormalization backward launch, by the address of the layer's input z
    modes = {"reduce": {}, "apply": {}}
    real_reduce, real_apply = Kn.bn_bwd_reduce_call, Kn.bn_bwd_apply_call

    def reduce_call(dy, ld_dy, z, ld_z, mask_y, ld_y, mean, invstd, scale, shift, mode, rows, c, part):
        modes["reduce"][z.data_ptr()] = int(mode)
        return real_reduce(dy, ld_dy, z, ld_z, mask_y, ld_y, mean, invstd, scale, shift, mode, rows, c, part)

    def apply_call(dy, ld_dy, z, ld_z, mask_y, ld_y, scale, shift, mode, *rest):
        modes["apply"][z.data_ptr()] = (int(mode), rest[7] is not None)     # rest[7]: the `dmasked` side output
        return real_apply(dy, ld_dy, z, ld_z, mask_y, ld_y, scale, shift, mode, *rest)

    monkeypatch.setattr(Kn, "bn_bwd_reduce_call", reduce_call)
    monkeypatch.setattr(Kn, "bn_bwd_apply_call", apply_call)
    plan = model._plan(b, True, False, external_grad=True)
    g = torch.Generator().manual_seed(1)
    xin = (torch.randn(b, hw, hw, cin, generator=g) * 20).numpy()
    dy = torch.randn(b, hw, hw, 128, generator=g)
    model._upload(plan, [xin], None)
    for _ in range(2):      # twice: the shared gradient buffers are rewritten from their first writer on every step
        plan.external_grad.copy_(dy)
        plan.run_forward()
        plan.run_backward()
    torch.cuda.synchronize()
    out = dict(grads={w.key: w.grad.detach().cpu().clone() for w in model.weight_specs if w.trainable}, dz={}, modes={})
    out["dx"] = plan.values[id(x0)].grad.buf.cpu().clone()
    for lyr in model.layers:
        if isinstance(lyr, Conv2D):
            out["dz"][lyr.name] = plan.values[id(lyr.outbound[0])].grad.buf.cpu().clone()
        if isinstance(lyr, BatchNormalization) and lyr.inbound[0] is not inp:
            zp = plan.values[id(lyr.inbound[0])].buf.data_ptr()
            out["modes"][lyr.name] = (modes["reduce"].get(zp), modes["apply"].get(zp))
    out["masked"] = list(plan.masked_dgrads)
    return out


def test_chain_of_blocks_is_the_same_with_the_mask_in_the_dgrad(cuda, monkeypatch):
    on = _lower_and_run("1", monkeypatch)
    off = _lower_and_run("0", monkeypatch)
    # not vacuous: the first conv of both identity blocks completes and masks the gradient of the block output it reads ...
    assert off["masked"] == [] and len(on["masked"]) >= 2, on["masked"]
    assert set(on["masked"]) == {"res1b_branch2a", "res1c_branch2a"}, on["masked"]
    # ... so no BatchNormalization at the end of blocks a and b masks by the block output any more (reduce: mode; apply:
    # (mode, writes the shortcut's masked gradient)), where the plain plan does; block c's output gradient comes from outside
    for name in ("bn1a_branch2c", "bn1a_branch1", "bn1b_branch2c"):
        assert on["modes"][name] == (0, (0, False)), (name, on["modes"][name])
        assert off["modes"][name][0] == 1 and off["modes"][name][1][0] == 1, (name, off["modes"][name])
    assert off["modes"]["bn1b_branch2c"][1] == (1, True)
    assert on["modes"]["bn1c_branch2c"] == off["modes"]["bn1c_branch2c"] == (1, (1, True))
    assert torch.equal(on["dx"], off["dx"]) and float(on["dx"].abs().max()) > 0
    assert set(on["dz"]) == set(off["dz"]) and len(on["dz"]) == 10
    for name in on["dz"]:
        assert torch.equal(on["dz"][name], off["dz"][name]), name
    for key, ref in off["grads"].items():
        got = on["grads"][key]
        if key.endswith("/gamma") or key.endswith("/beta"):
            assert torch.equal(got, ref), key
        elif float(ref.abs().max()) > 0:
            # weight gradients: the rel-L2 / max-norm bound of tests/test_blocks_gpu.py::_check
            assert _rel_l2(got, ref) <= 2e-3 and _rel_max(got, ref) <= 5e-2, key
