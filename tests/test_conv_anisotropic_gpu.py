"""Convolution geometries that differ between the two axes (tests/conv_geometry_cases.py: kernels 1x3 / 3x1 / 2x3 / 3x2,
strides (2,1) / (1,2), dilations (1,3) / (2,1), one-sided pads, non-square maps) through every kernel family and every
configuration index, against the fp64 oracle.  The kernels carry KH / KW, sH / sW, dH / dW and pT / pL apart; every other
convolution test of the suite passes equal pairs, which a swapped pair survives.  tests/test_conv_geometry_cases_cpu.py shows
that each case here is moved by order 1 when one of its pairs is swapped, so the bounds -- the project's existing ones, per
arithmetic mode -- are not delicate.

Also: Conv2DTranspose with unequal kernel / strides as the input gradient of the convolution it transposes, and a small
model (Conv2D 1x3 -> BN -> ReLU -> Conv2D 3x2 strides (2,1) -> Conv2DTranspose 2x3 strides (2,3) -> MaxPooling2D 2x3 strides
(1,2)) forward and backward, which pins compute_output_shape, conv_geometry and the lowering as well."""
import functools

import numpy as np
import pytest
import torch

import conv_geometry_cases as cg

pytestmark = pytest.mark.gpu

# rel-L2 against the fp64 oracle per arithmetic mode: (forward, gradients) -- tests/test_gather_variants_gpu.py (float32 takes
# the fp32-result bound of float32_mfma / float32x6: its index range holds both families), tests/test_lowp_gpu.py (float16)
TOL = {"float32": (2e-6, 2e-6), "float32x3": (3e-5, 3e-5), "float16": (1.5e-3, 8e-3)}
IDS = cg.case_id


@pytest.fixture()
def floatx():
    from jpeg_detection_resnet_ssd_amd import _lib
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    yield K
    K.set_floatx("float32")
    _lib.load().dj_set_gather_variants(1)
    _lib.load().dj_set_fast_path(1)


def _tol(ref):
    return 1e-3 * float(ref.abs().max()) + 1e-5


@functools.lru_cache(maxsize=None)
def device_case(geom):
    """Descriptor, device operands and the oracle's results of one geometry: made once, never written to."""
    from jpeg_detection_resnet_ssd_amd import kernels as Kn
    b, h, w, ci, co, k, s, pad, d = cg.norm(geom)
    host, ref = cg.reference(geom)
    desc = Kn.make_conv_desc(b, h, w, ci, co, k, s, pad, d)
    dev = {n: t.cuda() for n, t in host.items()}
    g = torch.Generator().manual_seed(5)
    dev["dx0"] = (torch.randn(b, h, w, ci, generator=g) * 1e-3).cuda()      # what the accumulating input gradient adds to
    return desc, dev, ref


def run_all(lib, desc, dev, cfg, y_shape):
    """Every launch form of one configuration index -> {name: tensor}."""
    from jpeg_detection_resnet_ssd_amd import _lib
    from jpeg_detection_resnet_ssd_amd import kernels as Kn
    x, wt, dy, sc, sh = dev["x"], dev["w"], dev["dy"], dev["sc"], dev["sh"]
    co = wt.shape[3]
    out = {}

    def pin(direction, splits):
        _lib.check(lib.dj_conv2d_tune_set(direction, desc, cfg, splits), "tune_set")

    # forward: plain; BN prologue + ReLU prologue with the statistics rows; the same through two slabs
    pin(0, 1)
    out["y"] = Kn.conv2d_fwd(desc, x, wt, None, torch.empty(y_shape, device="cuda"))
    pin(4, 1)
    out["stats"] = torch.zeros(Kn.conv2d_stats_rows(desc), 2, co, device="cuda")
    out["y_pro"] = Kn.conv2d_fwd(desc, x, wt, None, torch.empty(y_shape, device="cuda"), sc, sh, True, False, out["stats"])
    pin(0, 2)
    ws = torch.empty(2 * out["y"].numel(), device="cuda")
    out["y_pro_slabs"] = Kn.conv2d_fwd(desc, x, wt, None, torch.empty(y_shape, device="cuda"), sc, sh, True, False, None,
                                       workspace=ws)
    # input gradient: one K range, two K ranges, accumulating
    for splits in (1, 2):
        pin(1, splits)
        out["dx_%d" % splits] = Kn.conv2d_dgrad(desc, dy, wt, torch.empty(x.shape, device="cuda"))
    pin(1, 1)
    out["dx_beta"] = Kn.conv2d_dgrad(desc, dy, wt, dev["dx0"].clone(), beta=True)
    # weight gradient: one K range with and without prologue, three K ranges with prologue
    pin(2, 1)
    out["dw"] = Kn.conv2d_wgrad(desc, x, dy, torch.full(wt.shape, 7.0, device="cuda"))
    out["dw_pro"] = Kn.conv2d_wgrad(desc, x, dy, torch.zeros(wt.shape, device="cuda"), sc, sh, True, dw_zeroed=True)
    pin(2, 3)
    out["dw_pro_3"] = Kn.conv2d_wgrad(desc, x, dy, torch.zeros(wt.shape, device="cuda"), sc, sh, True, dw_zeroed=True)
    return out


FORMS = (("y", "y", 0), ("y_pro", "y_pro", 0), ("y_pro_slabs", "y_pro", 0), ("dx_1", "dx", 1), ("dx_2", "dx", 1),
         ("dx_beta", "dx_beta", 1), ("dw", "dw", 1), ("dw_pro", "dw_pro", 1), ("dw_pro_3", "dw_pro", 1))


@pytest.mark.parametrize("mode", ["float32", "float32x3", "float16"])
@pytest.mark.parametrize("case", cg.ANISOTROPIC, ids=IDS)
def test_anisotropic_geometry_every_configuration(case, mode, floatx):
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    desc, dev, ref = device_case(case.geom)
    ref = dict(ref, dx_beta=ref["dx"] + dev["dx0"].cpu().double())
    raw = ref["y_pro"].reshape(-1, ref["y_pro"].shape[3])
    ref_s, ref_q = raw.sum(0), (raw * raw).sum(0)
    floatx.set_floatx(mode)
    try:
        for cfg in range(lib.dj_conv2d_tune_configs()):
            out = run_all(lib, desc, dev, cfg, ref["y"].shape)
            torch.cuda.synchronize()
            errs = {name: cg.rel_l2(out[name].cpu(), ref[r]) for name, r, _ in FORMS}
            bad = {name: errs[name] for name, _, grad in FORMS if not errs[name] <= TOL[mode][grad]}
            assert not bad, ("cfg %d" % cfg, bad)
            st = out["stats"].cpu().double().sum(dim=0)
            assert (st[0] - ref_s).abs().max() <= 1e-3 * ref_s.abs().max() + 1e-3, ("cfg %d" % cfg, "column sums")
            assert (st[1] - ref_q).abs().max() <= 1e-3 * ref_q.abs().max(), ("cfg %d" % cfg, "column sums of squares")
    finally:
        for direction in (0, 4, 1, 2):
            _lib.check(lib.dj_conv2d_tune_set(direction, desc, -1, 1), "tune_set")


@pytest.mark.parametrize("tcase", cg.TRANSPOSE, ids=lambda t: "k%dx%d-s%dx%d" % (t[5] + t[6]))
def test_conv_transpose_with_unequal_kernel_and_strides_via_dgrad(tcase, floatx):
    """Conv2DTranspose(filters, (kh, kw), strides (sh, sw)) forward == the input gradient of the convolution with the same
    kernel, with its bias, in one K range, into a channel slice -- every configuration index."""
    from jpeg_detection_resnet_ssd_amd import _lib
    from jpeg_detection_resnet_ssd_amd import kernels as Kn
    from oracle import keras_ops as ko
    lib = _lib.load()
    b, h, w, ci, co, k, s = tcase
    g = torch.Generator().manual_seed(3)
    x = torch.randn(b, h, w, ci, generator=g)
    kern = torch.randn(k[0], k[1], co, ci, generator=g) * 0.1   # (kh, kw, out, in)
    bias = torch.randn(co, generator=g)
    yr = ko.conv2d_transpose(x.double(), kern.double(), bias.double(), s)
    geom = cg.transpose_conv_geom(tcase)
    desc = Kn.make_conv_desc(*cg.norm(geom))
    assert (desc.out_h, desc.out_w) == (h, w) and tuple(yr.shape) == (b, desc.in_h, desc.in_w, co)
    xd, kd, bd = x.cuda(), kern.cuda(), bias.cuda()
    try:
        for cfg in range(lib.dj_conv2d_tune_configs()):
            _lib.check(lib.dj_conv2d_tune_set(1, desc, cfg, 1), "tune_set")
            ybuf = torch.full((b, desc.in_h, desc.in_w, co + 16), float("nan"), device="cuda")
            Kn.conv2d_dgrad(desc, xd, kd, ybuf[..., 8:8 + co], bias=bd, no_split=True)
            torch.cuda.synchronize()
            y = ybuf[..., 8:8 + co].cpu().double()
            assert cg.rel_l2(y, yr) <= 2e-6 and (y - yr).abs().max() <= _tol(yr), ("cfg %d" % cfg, cg.rel_l2(y, yr))
            assert torch.isnan(ybuf[..., :8]).all() and torch.isnan(ybuf[..., 8 + co:]).all(), cfg
    finally:
        _lib.check(lib.dj_conv2d_tune_set(1, desc, -1, 1), "tune_set")


def test_model_with_unequal_pairs_in_every_layer(floatx):
    """Conv2D (1,3) 'same' -> BN -> ReLU -> Conv2D (3,2) strides (2,1) 'same' -> Conv2DTranspose (2,3) strides (2,3) ->
    MaxPooling2D (2,3) strides (1,2): output and every weight gradient from an external output gradient against the same
    chain of oracle calls under autograd in fp64, at the bounds of tests/test_blocks_gpu.py."""
    from test_blocks_gpu import _check, _perturb, _run
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras.layers import (Activation, BatchNormalization, Conv2D, Conv2DTranspose, Input,
                                                            MaxPooling2D)
    from jpeg_detection_resnet_ssd_amd.keras.models import Model
    from oracle import keras_ops as ko
    K.clear_session()
    K.set_random_seed(8)
    b = 3
    inp = Input((9, 12, 32))
    t = Conv2D(32, (1, 3), padding="same", name="an_c1")(inp)
    t = BatchNormalization(name="an_bn")(t)
    t = Activation("relu", name="an_relu")(t)
    t = Conv2D(32, (3, 2), strides=(2, 1), padding="same", name="an_c2")(t)
    t = Conv2DTranspose(16, (2, 3), strides=(2, 3), name="an_t")(t)
    out_t = MaxPooling2D((2, 3), strides=(1, 2), name="an_pool")(t)
    model = Model(inp, out_t)
    assert tuple(model.outputs[0].shape[1:]) == (9, 17, 16)
    w0 = _perturb(model)
    g = torch.Generator().manual_seed(1)
    xin = torch.randn(b, 9, 12, 32, generator=g).numpy()
    dy = torch.randn(b, 9, 17, 16, generator=g).numpy()
    out, grads, _ = _run(model, [xin], dy, "cuda")

    wt = {k: torch.from_numpy(v).double().requires_grad_(not k.endswith(("moving_mean", "moving_variance")))
          for k, v in w0.items()}
    r = ko.conv2d(torch.from_numpy(xin).double(), wt["an_c1/kernel"], wt["an_c1/bias"], (1, 1), "same")
    r = ko.relu(ko.batch_norm_train(r, wt["an_bn/gamma"], wt["an_bn/beta"])[0])
    r = ko.conv2d(r, wt["an_c2/kernel"], wt["an_c2/bias"], (2, 1), "same")
    assert tuple(r.shape[1:]) == (5, 12, 32)
    r = ko.conv2d_transpose(r, wt["an_t/kernel"], wt["an_t/bias"], (2, 3))
    assert tuple(r.shape[1:]) == (10, 36, 16)
    r = ko.max_pool(r, (2, 3), (1, 2))
    assert tuple(r.shape) == tuple(out.shape) == (b, 9, 17, 16)
    r.backward(torch.from_numpy(dy).double())
    ref_grads = {k: v.grad for k, v in wt.items() if v.grad is not None}
    assert set(ref_grads) >= {"an_c1/kernel", "an_c2/kernel", "an_t/kernel", "an_bn/gamma"}
    _check(out, grads, r.detach(), ref_grads)
    assert np.isfinite(out.numpy()).all()
