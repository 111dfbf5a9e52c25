"""dj_conv2d_nhwc_dgrad with `mask_x` (kernels.conv2d_dgrad(relu_mask=...)): the input gradient whose epilogue applies the ReLU mask
of the tensor it differentiates, against the two launches it replaces -- the plain (accumulating) input gradient followed by
dj_relu_bwd in place, on the same previous contents of dx.  One K range per tile in both, the same tile variant, the same
accumulation order: the results must agree BIT FOR BIT, under every tile variant the tuner may register and in every
arithmetic mode that works on fp32 tensors."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (name, batch, h, w, in_c, out_c, kernel, padding, beta, channel slices of wider buffers)
CASES = [
    # M = 338: two full 128-row tiles and a partial one; N = 160: partial for 128- and for 64-column tiles
    ("1x1_partial_tiles", 2, 13, 13, 160, 64, 1, "valid", 1, False),
    ("3x3_same", 1, 7, 5, 96, 32, 3, "same", 1, False),
    ("1x1_channel_slices", 2, 13, 13, 160, 64, 1, "valid", 1, True),
    ("1x1_beta0", 2, 13, 13, 160, 64, 1, "valid", 0, False),
    # outside the branch-free kernels' preconditions (channels % 32): the generic kernel's twin does the same
    ("3x3_generic_kernel", 2, 6, 7, 24, 20, 3, "same", 1, False),
]


def _slice_of_wider(t, lead, total):
    """The same values as `t` (B, H, W, C), held as channels [lead, lead + C) of a (B, H, W, total) buffer of NaNs."""
    wide = torch.full(t.shape[:3] + (total,), float("nan"), device=t.device)
    wide[..., lead:lead + t.shape[3]] = t
    return wide, wide[..., lead:lead + t.shape[3]]


@pytest.mark.parametrize("floatx", ["float32", "float32_mfma", "float32x6"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_masked_accumulate_equals_dgrad_then_relu_bwd(case, floatx, cuda):
    from jpeg_detection_resnet_ssd_amd import _lib
    from jpeg_detection_resnet_ssd_amd import kernels as Kn
    from jpeg_detection_resnet_ssd_amd.engine import call
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    _, b, h, w, ci, co, k, pad, beta, sliced = case
    g = torch.Generator().manual_seed(11)
    dy = torch.randn(b, h, w, co, generator=g).to(cuda)
    wt = (torch.randn(k, k, ci, co, generator=g) * 0.1).to(cuda)
    mask = torch.randn(b, h, w, ci, generator=g)
    mask[torch.rand(mask.shape, generator=g) < 0.25] = 0.0      # exact zeros beside the negatives: `> 0`, not `>= 0`
    mask = mask.to(cuda)
    assert int((mask == 0).sum()) > 0 and int((mask < 0).sum()) > 0 and int((mask > 0).sum()) > 0
    # beta = 0: the previous contents must not be read -- NaNs would show (NaN != NaN)
    old = torch.randn(b, h, w, ci, generator=g).to(cuda) if beta else torch.full((b, h, w, ci), float("nan"), device=cuda)
    desc = Kn.make_conv_desc(b, h, w, ci, co, (k, k), (1, 1), pad, (1, 1))
    lib = _lib.load()
    K.set_floatx(floatx)
    try:
        n_cfg = lib.dj_conv2d_tune_configs()
        assert n_cfg >= 14
        for cfg in range(n_cfg):
            _lib.check(lib.dj_conv2d_tune_set(1, desc, cfg, 1), "tune_set")
            assert Kn.conv2d_dgrad_relumask_supported(desc)
            if sliced:
                ref_all, ref = _slice_of_wider(old, 16, 224)
                got_all, got = _slice_of_wider(old, 16, 224)
                _, m = _slice_of_wider(mask, 32, 200)
            else:
                ref_all = ref = old.clone()
                got_all = got = old.clone()
                m = mask
            Kn.conv2d_dgrad(desc, dy, wt, ref, None, bool(beta))
            rows, ld, ld_m = b * h * w, ref.stride(2), m.stride(2)
            call("dj_relu_bwd", ref, ld, m, ld_m, ref, ld, rows, ci, 0)
            Kn.conv2d_dgrad(desc, dy, wt, got, None, bool(beta), relu_mask=m)
            torch.cuda.synchronize()
            assert not torch.isnan(ref).any(), "cfg %d" % cfg
            # the whole buffers: what lies beside a channel slice stays as it was (NaN there on both sides)
            assert torch.equal(torch.nan_to_num(got_all, nan=-7.0), torch.nan_to_num(ref_all, nan=-7.0)), "cfg %d" % cfg
            assert float(ref.abs().max()) > 0 and int((ref == 0).sum()) >= int((m <= 0).sum()), "cfg %d" % cfg
    finally:
        _lib.check(lib.dj_conv2d_tune_set(1, desc, -1, 1), "tune_set")
        K.set_floatx("float32")


def test_what_the_masked_accumulate_refuses(cuda):
    """Split-K entries, the strided 1x1 scatter form and the 16-bit arithmetic modes: `_supported` says 0 and the call
    returns DJ_ERR_ARG before it launches anything."""
    from jpeg_detection_resnet_ssd_amd import _lib
    from jpeg_detection_resnet_ssd_amd import kernels as Kn
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    lib = _lib.load()
    b, h, w, ci, co = 2, 8, 8, 64, 32
    dy, wt = torch.randn(b, h, w, co, device=cuda), torch.randn(1, 1, ci, co, device=cuda)
    dx, m = torch.zeros(b, h, w, ci, device=cuda), torch.randn(b, h, w, ci, device=cuda)
    desc = Kn.make_conv_desc(b, h, w, ci, co, (1, 1))
    assert Kn.conv2d_dgrad_relumask_supported(desc)
    try:
        _lib.check(lib.dj_conv2d_tune_set(1, desc, 0, 2), "tune_set")
        assert not Kn.conv2d_dgrad_relumask_supported(desc)
        with pytest.raises(_lib.DjError, match="splits"):
            Kn.conv2d_dgrad(desc, dy, wt, dx, None, True, relu_mask=m)
    finally:
        _lib.check(lib.dj_conv2d_tune_set(1, desc, -1, 1), "tune_set")
    strided = Kn.make_conv_desc(b, h, w, ci, co, (1, 1), (2, 2))
    assert not Kn.conv2d_dgrad_relumask_supported(strided)
    with pytest.raises(_lib.DjError, match="strided"):
        Kn.conv2d_dgrad(strided, dy[:, :4, :4].contiguous(), wt, dx, None, True, relu_mask=m)
    K.set_floatx("float16")
    try:
        assert not Kn.conv2d_dgrad_relumask_supported(desc)
        with pytest.raises(_lib.DjError, match="16-bit"):
            Kn.conv2d_dgrad(desc, dy, wt, dx, None, True, relu_mask=m)
    finally:
        K.set_floatx("float32")
    torch.cuda.synchronize()
    assert float(dx.abs().max()) == 0.0      # nothing was launched
