"""Both branch-free kernel families -- the split-bf16 kernels of dj_igemm_h16.h (float32x3 / float32x6) and the fp32 MFMA
kernels of dj_igemm_fast.h (float32_mfma: compute mode 5, configuration indices [0, N)) --: their gather variants --
per-tap row offsets cached across the K-steps of a tap (NP 2: forward, input gradient) and the incremental pixel walk
(NP 3: weight gradient, dj_walk.h) -- against their plain twins (NP 0), which redo the bounds and address arithmetic
every K-step.  A twin pair sums the same products in the same order, so every comparison is torch.equal;
`dj_set_gather_variants` picks the twin of either family inside one process.

Geometries: the smallest at which each carry and edge of the walk / each tap edge occurs, and three whose kernel, strides or
dilation differ between the axes (see GEOMS).  The prologue's
shift is larger in magnitude than the data, so a padding pixel that is not zeroed AFTER the prologue shows.

Split-K in the bit-equality test: the forward pass goes through slabs + the fixed-order reduction; the gradients have
atomics only, and are compared at TWO K ranges -- two commutative additions onto a zeroed tensor, the same bits in either
arrival order -- which is what makes a K range that starts in the middle of the reduction comparable at all.  The
fp64-oracle test runs the weight gradient at three K ranges (atomics) at the bounds of tests/test_x3_gpu.py;
float32_mfma takes the float32x6 bound: against the fp64 oracle the fp32 MFMA kernels and the float32x6 kernels lie
equally far from it (include/dj_hip.h, dj_set_compute_mode)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = {"float32x3": 3e-5, "float32x6": 2e-6}   # rel-L2 per GEMM: the bounds of tests/test_x3_gpu.py
TOL["float32_mfma"] = TOL["float32x6"]
MODES = ["float32x6", "float32x3", "float32_mfma"]

# (batch, H, W, Cin, Cout, k, stride, padding, dilation); k, stride and dilation: one int for both axes, or an (h, w) pair
GEOMS = [
    (2, 7, 5, 128, 96, 3, 1, "same", 1),      # non-square map, a row shorter than a K-step
    (3, 3, 3, 128, 64, 3, 1, "same", 1),      # a map smaller than a K-step: an image carry every step
    (2, 1, 1, 256, 64, 3, 1, "same", 1),      # one-pixel map
    (2, 9, 9, 128, 160, 3, 2, "same", 1),     # stride 2 and an N tail
    (1, 12, 12, 128, 64, 3, 1, "same", 6),    # dilated: most taps outside the image
    (2, 6, 6, 128, 64, 3, 1, "valid", 1),
    (2, 8, 8, 256, 64, 1, 2, "valid", 1),     # strided 1x1: the weight gradient walks
    (2, 6, 6, 192, 64, 3, 1, "same", 1),      # Cin % 128 != 0: the 128-row tiles fall back to the plain kernel
    # geometries that differ between the axes (tests/conv_geometry_cases.py): the tap cache's (kh, kw) wrap at KW != KH, the
    # walk's carries at sH != sW, the tap offsets at dH != dW and pads 1 / 3
    (2, 9, 12, 128, 64, (2, 3), 1, "same", 1),
    (2, 11, 9, 128, 64, 3, (2, 1), "same", 1),     # (an output row of 9 pixels: every K-step of the walk carries)
    (1, 12, 9, 128, 64, 3, 1, "same", (1, 3)),
]


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


@pytest.fixture()
def floatx():
    from jpeg_detection_resnet_ssd_amd import _lib
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    yield K
    K.set_floatx("float32")
    _lib.load().dj_set_gather_variants(1)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@functools.lru_cache(maxsize=None)
def case(geom):
    """Operands (host and device) and the fp64 oracle's results of one geometry: computed once, never written to."""
    from jpeg_detection_resnet_ssd_amd import kernels as Kn
    from oracle import keras_ops as ko
    b, h, w, ci, co, k, s, pad, dil = geom
    k, s, dil = _pair(k), _pair(s), _pair(dil)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(b, h, w, ci, generator=g)
    wt = torch.randn(k[0], k[1], ci, co, generator=g) * (2.0 / (k[0] * k[1] * ci)) ** 0.5
    sc = torch.rand(ci, generator=g) + 0.5
    # |shift| in [8, 9): above |x * scale| (< 1.5 * 5.5), both signs -- a padding pixel left at `shift` would be seen
    sh = (8.0 + torch.rand(ci, generator=g)) * torch.where(torch.rand(ci, generator=g) < 0.75, 1.0, -1.0)
    xa = torch.relu(x * sc + sh)
    xr, wr = xa.double().requires_grad_(True), wt.double().requires_grad_(True)
    yr = ko.conv2d(xr, wr, None, s, pad, dil)
    dy = torch.randn(*yr.shape, generator=g) * 1e-3
    yr.backward(dy.double())
    w_plain, x_plain = wt.double().requires_grad_(True), x.double().requires_grad_(True)
    y_plain = ko.conv2d(x_plain, w_plain, None, s, pad, dil)
    y_plain.backward(dy.double())
    desc = Kn.make_conv_desc(b, h, w, ci, co, k, s, pad, dil)
    dev = {n: t.cuda() for n, t in (("x", x), ("w", wt), ("dy", dy), ("sc", sc), ("sh", sh))}
    ref = {"y_pro": yr.detach(), "y": y_plain.detach(), "dx": x_plain.grad, "dw_pro": wr.grad, "dw": w_plain.grad}
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

    # forward: plain; BN prologue + ReLU with the statistics rows; BN prologue + ReLU through two slabs
    pin(0, 1)
    out["y"] = Kn.conv2d_fwd(desc, x, wt, None, torch.empty(y_shape, device="cuda"))
    pin(4, 1)
    out["stats"] = torch.zeros(Kn.conv2d_stats_rows(desc), 2, co, device="cuda")
    out["y_pro"] = Kn.conv2d_fwd(desc, x, wt, None, torch.empty(y_shape, device="cuda"), sc, sh, True, False, out["stats"])
    pin(0, 2)
    ws = torch.empty(2 * out["y"].numel(), device="cuda")
    out["y_pro_slabs"] = Kn.conv2d_fwd(desc, x, wt, None, torch.empty(y_shape, device="cuda"), sc, sh, True, False, None,
                                       workspace=ws)
    # input gradient: one K range, two K ranges
    for splits in (1, 2):
        pin(1, splits)
        out["dx_%d" % splits] = Kn.conv2d_dgrad(desc, dy, wt, torch.empty(x.shape, device="cuda"))
    # weight gradient: one K range with and without prologue, two K ranges with prologue
    pin(2, 1)
    out["dw"] = Kn.conv2d_wgrad(desc, x, dy, torch.full(wt.shape, 7.0, device="cuda"))
    out["dw_pro"] = Kn.conv2d_wgrad(desc, x, dy, torch.zeros(wt.shape, device="cuda"), sc, sh, True, dw_zeroed=True)
    pin(2, 2)
    out["dw_pro_2"] = Kn.conv2d_wgrad(desc, x, dy, torch.zeros(wt.shape, device="cuda"), sc, sh, True, dw_zeroed=True)
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", GEOMS)
def test_gather_variants_equal_their_plain_twins_bit_for_bit(geom, mode, floatx):
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    desc, dev, ref = case(geom)
    floatx.set_floatx(mode)
    try:
        for cfg in range(lib.dj_conv2d_tune_configs()):
            lib.dj_set_gather_variants(1)
            new = run_all(lib, desc, dev, cfg, ref["y"].shape)
            lib.dj_set_gather_variants(0)
            plain = run_all(lib, desc, dev, cfg, ref["y"].shape)
            torch.cuda.synchronize()
            for name in new:
                assert torch.equal(new[name], plain[name]), ("cfg %d" % cfg, name,
                                                             float((new[name] - plain[name]).abs().max()))
            if cfg == 0:     # (once: the twins are equal, so are their distances to the oracle)
                for name, r in (("y", "y"), ("y_pro", "y_pro"), ("y_pro_slabs", "y_pro"), ("dx_1", "dx"), ("dx_2", "dx"),
                                ("dw", "dw"), ("dw_pro", "dw_pro"), ("dw_pro_2", "dw_pro")):
                    assert rel_l2(new[name].cpu(), ref[r]) <= TOL[mode], (name, rel_l2(new[name].cpu(), ref[r]))
    finally:
        lib.dj_set_gather_variants(1)
        for direction in (0, 4, 1, 2):
            _lib.check(lib.dj_conv2d_tune_set(direction, desc, -1, 1), "tune_set")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", GEOMS)
def test_gather_variants_against_the_fp64_oracle(geom, mode, floatx):
    """Forward (BN prologue + ReLU), input gradient and the weight gradient at three K ranges (atomics), every
    configuration index, at the mode's bound."""
    from jpeg_detection_resnet_ssd_amd import _lib
    from jpeg_detection_resnet_ssd_amd import kernels as Kn
    lib = _lib.load()
    desc, dev, ref = case(geom)
    x, wt, dy, sc, sh = dev["x"], dev["w"], dev["dy"], dev["sc"], dev["sh"]
    floatx.set_floatx(mode)
    lib.dj_set_gather_variants(1)
    try:
        for cfg in range(lib.dj_conv2d_tune_configs()):
            for direction, splits in ((0, 1), (1, 1), (2, 3)):
                _lib.check(lib.dj_conv2d_tune_set(direction, desc, cfg, splits), "tune_set")
            y = Kn.conv2d_fwd(desc, x, wt, None, torch.empty(ref["y"].shape, device="cuda"), sc, sh, True)
            dx = Kn.conv2d_dgrad(desc, dy, wt, torch.empty(x.shape, device="cuda"))
            dw_pro = Kn.conv2d_wgrad(desc, x, dy, torch.zeros(wt.shape, device="cuda"), sc, sh, True, dw_zeroed=True)
            dw = Kn.conv2d_wgrad(desc, x, dy, torch.full(wt.shape, 7.0, device="cuda"))
            torch.cuda.synchronize()
            errs = [rel_l2(o.cpu(), ref[r]) for o, r in ((y, "y_pro"), (dx, "dx"), (dw_pro, "dw_pro"), (dw, "dw"))]
            assert max(errs) <= TOL[mode], ("cfg %d" % cfg, errs)
    finally:
        for direction in (0, 1, 2):
            _lib.check(lib.dj_conv2d_tune_set(direction, desc, -1, 1), "tune_set")
