"""GPU: csrc/dj_rgb2dct.hip turns uint8 pixels into exactly the coefficients the in-tree reader gets out of the JPEG
PIL wrote of them (tests/golden/rgb_dct.npz: pixels + bytes), whatever the batch, the output strides or the stream, and
a model fed with pixels computes what the model fed with the decoded file computes.  Equality throughout: the
arithmetic is integer only."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rgb_dct.npz")
CASES = ["smooth_300x300_q75", "patches_300x300_q75", "noise_300x300_q30", "saturated_300x300_q90",
         "smooth_224x224_q75", "smooth_301x299_q75", "smooth_296x300_q75", "noise_37x53_q75", "noise_17x16_q75",
         "noise_8x8_q75", "noise_1x1_q100", "noise_300x20_q50", "noise_15x33_q10"]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _device_planes(rgb_batch, tables, normalized=True, dev="cuda:0"):
    from jpeg_detection_resnet_ssd_amd import kernels
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import blocks_for
    b, h, w, _ = rgb_batch.shape
    (yh, yw), (ch, cw) = blocks_for(h, w)
    outs = (torch.full((b, yh, yw, 64), float("nan"), device=dev), torch.full((b, ch, cw, 64), float("nan"), device=dev),
            torch.full((b, ch, cw, 64), float("nan"), device=dev))
    kernels.rgb_to_dct(torch.from_numpy(np.ascontiguousarray(rgb_batch)).to(dev), tables, outs, normalized=normalized)
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("normalized", [True, False])
def test_kernel_equals_the_reader_on_the_jpeg_pil_wrote(cuda, golden, case, normalized):
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import quant_tables
    from jpeg_detection_resnet_ssd_amd.jpeg2dct import numpy as j2d
    rgb, data, quality = golden[case + "/rgb"], golden[case + "/jpeg"].tobytes(), int(golden[case + "/quality"])
    want = j2d.loads(data, normalized=normalized)
    got = _device_planes(rgb[None], quant_tables(quality), normalized)
    for name, w, g in zip(("y", "cb", "cr"), want, got):
        w = torch.from_numpy(w.astype(np.float32))[None]
        g = g.cpu()
        assert g.shape == w.shape, (name, g.shape, w.shape)
        bad = (g != w) | torch.isnan(g)
        print(case, name, "mismatching coefficients:", int(bad.sum()), "of", w.numel(),
              "first blocks:", bad.any(-1).nonzero()[:4].tolist())
        assert torch.equal(g, w), (case, name)


def test_host_twin_equals_the_kernel_on_fresh_pixels(cuda):
    """Sizes and contents the fixture does not hold, against the numpy statement of the contract."""
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import quant_tables, rgb_to_dct_host
    rng = np.random.default_rng(77)
    for h, w, q in ((2, 3, 1), (16, 16, 50), (298, 298, 95), (302, 302, 100), (150, 300, 10), (20, 300, 75), (31, 47, 90)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        img[rng.random((h, w)) < 0.3] = 255
        img[rng.random((h, w)) < 0.3] = 0
        for name, a, b in zip(("y", "cb", "cr"), rgb_to_dct_host(img, q), _device_planes(img[None], quant_tables(q))):
            assert torch.equal(b.cpu()[0], torch.from_numpy(a.astype(np.float32))), (h, w, q, name)


def test_batch_of_32_equals_its_single_image_runs(cuda):
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import quant_tables
    rng = np.random.default_rng(5)
    batch = rng.integers(0, 256, (32, 300, 300, 3), dtype=np.uint8)
    batch[16:] = np.kron(rng.integers(0, 256, (16, 50, 50, 3)), np.ones((1, 6, 6, 1), dtype=np.int64)).astype(np.uint8)
    tabs = quant_tables(75)
    whole = _device_planes(batch, tabs)
    for i in range(32):
        single = _device_planes(batch[i:i + 1], tabs)
        for a, b in zip(whole, single):
            assert torch.equal(a[i:i + 1], b), i


def test_strided_outputs_leave_everything_else_untouched(cuda, golden):
    """Cb and Cr as the two halves of one 128-channel buffer, Y as channels 8..71 of a 96-channel one; sentinels in the
    unwritten channels and in a guard band after each tensor stay."""
    from jpeg_detection_resnet_ssd_amd import kernels
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import quant_tables
    from jpeg_detection_resnet_ssd_amd.jpeg2dct import numpy as j2d
    names = ["smooth_301x299_q75", "smooth_301x299_q75"]
    rgb = np.stack([golden[n + "/rgb"] for n in names])
    want = [j2d.loads(golden[n + "/jpeg"].tobytes()) for n in names]
    guard, sentinel = 4096, -12345.0
    flat_y = torch.full((2 * 38 * 38 * 96 + guard,), sentinel, device=cuda)
    flat_c = torch.full((2 * 19 * 19 * 128 + guard,), sentinel, device=cuda)
    wide_y = flat_y[:2 * 38 * 38 * 96].view(2, 38, 38, 96)
    cbcr = flat_c[:2 * 19 * 19 * 128].view(2, 19, 19, 128)
    kernels.rgb_to_dct(torch.from_numpy(rgb).to(cuda), quant_tables(75), (wide_y[..., 8:72], cbcr[..., :64], cbcr[..., 64:]))
    torch.cuda.synchronize()
    for i in range(2):
        assert torch.equal(wide_y[i, ..., 8:72].cpu(), torch.from_numpy(want[i][0].astype(np.float32)))
        assert torch.equal(cbcr[i, ..., :64].cpu(), torch.from_numpy(want[i][1].astype(np.float32)))
        assert torch.equal(cbcr[i, ..., 64:].cpu(), torch.from_numpy(want[i][2].astype(np.float32)))
    assert bool((wide_y[..., :8] == sentinel).all()) and bool((wide_y[..., 72:] == sentinel).all())
    assert bool((flat_y[-guard:] == sentinel).all()) and bool((flat_c[-guard:] == sentinel).all())


def test_row_stride_of_the_pixels_is_honoured(cuda, golden):
    """The batch as a window of a wider image buffer (row stride above 3 * width)."""
    from jpeg_detection_resnet_ssd_amd import kernels
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import quant_tables, rgb_to_dct_host
    rgb = golden["noise_37x53_q75/rgb"]
    wide = torch.zeros((1, 37, 64, 3), dtype=torch.uint8, device=cuda)
    wide[0, :, :53] = torch.from_numpy(rgb).to(cuda)
    window = wide[:, :, :53]
    assert window.stride(1) == 192
    outs = (torch.empty((1, 5, 7, 64), device=cuda), torch.empty((1, 3, 4, 64), device=cuda),
            torch.empty((1, 3, 4, 64), device=cuda))
    kernels.rgb_to_dct(window, quant_tables(75), outs)
    for a, b in zip(rgb_to_dct_host(rgb, 75), outs):
        assert torch.equal(b.cpu()[0], torch.from_numpy(a.astype(np.float32)))


def test_launch_on_a_side_stream(cuda, golden):
    from jpeg_detection_resnet_ssd_amd import kernels
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import quant_tables
    from jpeg_detection_resnet_ssd_amd.jpeg2dct import numpy as j2d
    rgb = torch.from_numpy(golden["smooth_224x224_q75/rgb"][None]).to(cuda)
    outs = (torch.zeros((1, 28, 28, 64), device=cuda), torch.zeros((1, 14, 14, 64), device=cuda),
            torch.zeros((1, 14, 14, 64), device=cuda))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    kernels.rgb_to_dct(rgb, quant_tables(75), outs, stream=side.cuda_stream)
    side.synchronize()
    for w, g in zip(j2d.loads(golden["smooth_224x224_q75/jpeg"].tobytes()), outs):
        assert torch.equal(g.cpu()[0], torch.from_numpy(w.astype(np.float32)))


def test_custom_all_ones_table(cuda, golden):
    """Table entries of 1: the levels are the DCT coefficients rounded from their 8x scale, and equal the values."""
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import rgb_to_dct_host
    ones = (np.ones(64, np.int32), np.ones(64, np.int32))
    rgb = golden["noise_37x53_q75/rgb"]
    want = rgb_to_dct_host(rgb, tables=ones)
    got = _device_planes(rgb[None], ones)
    levels = _device_planes(rgb[None], ones, normalized=False)
    for w, g, l in zip(want, got, levels):
        assert torch.equal(g.cpu()[0], torch.from_numpy(w.astype(np.float32))) and torch.equal(g, l)


def test_emit_dct_inputs_device_equals_emit_dct_inputs(cuda, golden):
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import emit_dct_inputs, emit_dct_inputs_device
    names = ["smooth_300x300_q75", "patches_300x300_q75"]
    rgb = np.stack([golden[n + "/rgb"] for n in names])
    data = [golden[n + "/jpeg"].tobytes() for n in names]
    for deconv in (False, True):
        want = emit_dct_inputs(None, deconv=deconv, jpeg_bytes=data)
        got = emit_dct_inputs_device(rgb, deconv=deconv)
        assert len(want) == len(got) == (3 if deconv else 2)
        for w, g in zip(want, got):
            assert g.is_cuda and g.dtype == torch.float32 and torch.equal(g.cpu(), torch.from_numpy(w))


@pytest.mark.parametrize("archi", ["deconv", "ssd_custom"])
def test_model_fed_with_pixels_equals_model_fed_with_the_decoded_file(cuda, golden, archi):
    """train_on_batch(PendingDCTInputs, y) leaves the plan's inputs bit-identical to train_on_batch(emit_dct_inputs(...
    jpeg_bytes), y), its loss differs from the host-fed loss by no more than two host-fed runs differ from each other
    (measured here), and predict_on_batch / predict return the same y_pred either way.

    The bound is applied to the data loss, the mining counts included: the part of the reported loss that the inputs
    reach.  Measured on an MI355X: data loss 67.548095703125 (deconv) / 32.575592041015625 (ssd_custom) in all three
    runs, spread 0, difference 0.  The other part, the l2 report, is sum(w^2) of the weights BEFORE the step -- the same
    weights in all three runs, whatever is fed -- accumulated by dj_sgd_momentum_update: per segment the workgroups' sums
    are added with fp64 atomics, whose order is free, and rounded once to fp32, and float(l2 * sum) is added over the
    segments, so its last digit may move from run to run on its own (with the fp32 atomics of an earlier kernel: 4.72073779 / 4.72073877 between the two host-fed deconv runs; 3.69233496
    twice, then 3.69233594, for ssd_custom): on the sum, "no more than two host-fed runs differ" is a comparison of
    three draws of that noise and fails about every other time with identical inputs.  The sums are printed."""
    from jpeg_detection_resnet_ssd_amd import workloads
    from jpeg_detection_resnet_ssd_amd.data import synthetic_dct as sd
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import DeviceDCTEmitter, emit_dct_inputs
    names = ["smooth_300x300_q75", "patches_300x300_q75"]
    rgb = np.stack([golden[n + "/rgb"] for n in names])
    deconv = archi == "deconv"
    host_x = emit_dct_inputs(None, deconv=deconv, jpeg_bytes=[golden[n + "/jpeg"].tobytes() for n in names])
    pending = DeviceDCTEmitter(quality=75, deconv=deconv)(rgb)
    gt = sd.random_ground_truth(2, seed=5)
    runs = []
    for x in (host_x, host_x, pending):
        model, sizes = workloads.build_ssd(archi)
        y = workloads.make_encoder(sizes)(gt).astype(np.float32)
        pred = model.predict_on_batch(x)
        if x is pending:
            assert np.array_equal(model.predict(x, batch_size=2), pred)      # `predict` slices the batch
        loss = model.train_on_batch(x, y)
        torch.cuda.synchronize()
        print(archi, "pixel-fed" if x is pending else "host-fed", "loss", repr(loss), model.last_step_info)
        runs.append((dict(model.last_step_info), pred, [t.detach().cpu().clone() for t in model._plan(2, True, True).inputs]))
    (info_a, pred_a, in_a), (info_b, pred_b, in_b), (info_d, pred_d, in_d) = runs
    assert len(in_a) == len(in_d) == (3 if deconv else 2)
    for a, d, h in zip(in_a, in_d, host_x):
        assert torch.equal(a, torch.from_numpy(h)) and torch.equal(a, d)
    for key in ("data_loss", "n_positive", "n_negative"):
        spread = abs(info_a[key] - info_b[key])
        print(archi, key, "host-fed", repr(info_a[key]), repr(info_b[key]), "spread", spread, "pixel-fed", repr(info_d[key]),
              "difference", abs(info_d[key] - info_a[key]))
        assert np.isfinite(info_d[key]) and abs(info_d[key] - info_a[key]) <= spread, key
    assert np.array_equal(pred_a, pred_b) and np.array_equal(pred_a, pred_d)
