"""GPU: csrc/dj_imgprep.hip resizes, crops and flips a ragged batch of decoded images into exactly the bytes Pillow
leaves (tests/golden/image_prep.npz) and the numpy twin states (data/image_prep.py:prep_host), whatever the batch, the
output stride or the stream, and a classifier fed the decoded images computes what it computes when fed the host-made
inputs.  Equality throughout: the arithmetic is integer only."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_prep.npz")
CASES = ["down1p1_noise_bicubic", "down1p1_noise_bilinear", "down2_smooth_bicubic", "down3p1_saturated_bilinear",
         "down9p4_noise_bicubic", "down5_portrait_smooth_bilinear", "down5_portrait_saturated_bicubic", "up3p2_noise_bicubic",
         "up2p9_portrait_noise_bilinear", "unchanged_height_noise_bicubic", "unchanged_both_smooth_bilinear",
         "squash_saturated_bicubic", "square_saturated_bilinear", "one_pixel_bicubic", "two_by_three_bilinear",
         "two_by_three_bicubic"]
BILINEAR, BICUBIC = 2, 3


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _ragged_batch(rng, shapes, target):
    from jpeg_detection_resnet_ssd_amd.data.image_prep import max_offset
    images, params = [], []
    for i, (h, w) in enumerate(shapes):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if i % 3 == 1:
            img[rng.random((h, w)) < 0.4] = 255
            img[rng.random((h, w)) < 0.4] = 0
        scale = i % 5 != 4
        top = max_offset(h, w, target, scale)
        images.append(img)
        params.append((scale, (0, top, top // 2, top // 3)[i % 4], i % 2 == 1))
    return images, params


def test_fixture_lists_the_cases(golden):
    assert sorted(CASES) == sorted(str(n) for n in golden["names"])


@pytest.mark.parametrize("case", CASES)
def test_kernel_equals_what_pillow_made_of_the_fixture(cuda, golden, case):
    from jpeg_detection_resnet_ssd_amd.data.image_prep import prep_device
    t, scale, offset, flip, resample = (int(v) for v in golden[case + "/params"])
    got = prep_device([golden[case + "/src"]], [(bool(scale), offset, bool(flip))], t, resample, device=cuda).cpu().numpy()
    want = golden[case + "/out"]
    bad = got[0] != want
    print(case, "mismatching bytes:", int(bad.sum()), "of", want.size, "first:", np.argwhere(bad)[:4].tolist())
    assert got.shape == (1,) + want.shape and np.array_equal(got[0], want)


@pytest.mark.parametrize("resample", [BICUBIC, BILINEAR])
def test_kernel_equals_the_host_twin_on_fresh_ragged_batches(cuda, resample):
    """Sizes and contents the fixture does not hold, a 2000 x 30 and a 30 x 2000 source among them."""
    from jpeg_detection_resnet_ssd_amd.data.image_prep import prep_device, prep_host
    rng = np.random.default_rng(31)
    for target, shapes in ((224, [(375, 500), (500, 375), (2000, 30), (30, 2000), (224, 224), (224, 300), (100, 80), (1, 1),
                                 (333, 500), (768, 1024)]),
                           (64, [(64, 64), (65, 64), (64, 63), (2, 3), (3, 2), (700, 500), (48, 1000)]),
                           (1, [(5, 7), (1, 1)]),
                           (300, [(120, 160), (481, 321)])):
        images, params = _ragged_batch(rng, shapes, target)
        got = prep_device(images, params, target, resample, device=cuda).cpu().numpy()
        for i, (im, (s, o, f)) in enumerate(zip(images, params)):
            want = prep_host(im, target, s, o, f, resample)
            assert np.array_equal(got[i], want), (target, shapes[i], s, o, f, int((got[i] != want).sum()))


def test_ragged_batch_of_64_equals_its_single_image_runs(cuda):
    from jpeg_detection_resnet_ssd_amd.data.image_prep import prep_device
    rng = np.random.default_rng(32)
    shapes = [(int(rng.integers(120, 420)), int(rng.integers(120, 520))) for _ in range(64)]
    shapes[7], shapes[40] = (375, 500), (375, 500)
    images, params = _ragged_batch(rng, shapes, 224)
    whole = prep_device(images, params, 224, device=cuda)
    assert whole.shape == (64, 224, 224, 3) and whole.dtype == torch.uint8
    for i in range(64):
        single = prep_device(images[i:i + 1], params[i:i + 1], 224, device=cuda)
        assert torch.equal(whole[i:i + 1], single), i


def _staged(plan, images, cuda):
    blob_host = np.zeros(plan.nbytes, dtype=np.uint8)
    plan.fill(blob_host, images)
    return blob_host, torch.from_numpy(blob_host).to(cuda)


def test_strided_output_leaves_everything_else_untouched(cuda):
    """Rows of 3 * T bytes inside rows of 3 * T + 40: the bytes between rows, a guard band behind the tensor, the scratch
    past what the plan uses and the staged inputs keep their sentinel / their content."""
    from jpeg_detection_resnet_ssd_amd import kernels
    from jpeg_detection_resnet_ssd_amd.data.image_prep import BatchPlan, prep_host
    rng = np.random.default_rng(33)
    t, pitch, guard, sentinel = 96, 3 * 96 + 40, 4096, 0xA5
    images, params = _ragged_batch(rng, [(150, 200), (200, 150), (96, 96), (90, 300)], t)
    plan = BatchPlan([im.shape[:2] for im in images], params, t)
    blob_host, blob = _staged(plan, images, cuda)
    flat = torch.full((4 * t * pitch + guard,), sentinel, dtype=torch.uint8, device=cuda)
    out = flat[:4 * t * pitch].view(4, t, pitch)[:, :, :3 * t].unflatten(2, (t, 3))
    assert out.stride() == (t * pitch, pitch, 3, 1)
    scratch = torch.full((plan.scratch_bytes + guard,), sentinel, dtype=torch.uint8, device=cuda)
    src_h, desc_h, pool_h = plan.views(blob_host)
    src_d, desc_d, pool_d = plan.views(blob)
    assert kernels.image_prep_scratch_bytes(desc_h, t) == plan.scratch_bytes
    kernels.image_prep(src_d, desc_d, desc_h, pool_d, pool_h, t, out, scratch)
    torch.cuda.synchronize()
    for i, (im, (s, o, f)) in enumerate(zip(images, params)):
        assert np.array_equal(out[i].cpu().numpy(), prep_host(im, t, s, o, f)), i
    rows = flat[:4 * t * pitch].view(4 * t, pitch)
    assert bool((rows[:, 3 * t:] == sentinel).all()) and bool((flat[-guard:] == sentinel).all())
    assert bool((scratch[plan.scratch_bytes:] == sentinel).all())
    for d in plan.desc:      # the 64-byte rounding between two images' scratch regions stays too
        end = int(d["scratch_offset"]) + 3 * t * int(d["n_rows"])
        assert bool((scratch[end:-(-end // 64) * 64] == sentinel).all())
    assert np.array_equal(blob.cpu().numpy(), blob_host)


def test_launch_on_a_side_stream(cuda, golden):
    from jpeg_detection_resnet_ssd_amd.data.image_prep import prep_device
    names = ["down2_smooth_bicubic", "squash_saturated_bicubic"]
    t = 40
    images = [golden[n + "/src"] for n in names]
    params = [(True, 3, True), (False, 0, False)]
    want = prep_device(images, params, t, device=cuda)
    out = torch.zeros((2, t, t, 3), dtype=torch.uint8, device=cuda)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):        # the upload goes to the same stream as the two passes
        prep_device(images, params, t, device=cuda, out=out, stream=side.cuda_stream)
    side.synchronize()
    assert torch.equal(out, want)


@pytest.mark.parametrize("field, image, value", [
    ("crop_x", 0, 60), ("crop_y", 1, -1), ("res_w", 0, 10), ("src_h", 1, 0), ("src_w", 0, -7), ("n_rows", 0, 0),
    ("row0", 1, 9), ("scratch_offset", 1, 0), ("src_offset", 1, 1 << 40), ("h_ksize", 0, 1), ("v_bounds", 1, 1 << 30),
])
def test_rejected_arguments_return_an_error_and_write_nothing(cuda, field, image, value):
    from jpeg_detection_resnet_ssd_amd import _lib, kernels
    from jpeg_detection_resnet_ssd_amd.data.image_prep import BatchPlan
    rng = np.random.default_rng(34)
    t, sentinel = 32, 0x5A
    images, params = _ragged_batch(rng, [(50, 70), (70, 50)], t)
    plan = BatchPlan([im.shape[:2] for im in images], params, t)
    blob_host, blob = _staged(plan, images, cuda)
    out = torch.full((2, t, t, 3), sentinel, dtype=torch.uint8, device=cuda)
    scratch = torch.full((plan.scratch_bytes,), sentinel, dtype=torch.uint8, device=cuda)
    src_h, desc_h, pool_h = plan.views(blob_host)
    src_d, desc_d, pool_d = plan.views(blob)
    desc_h = desc_h.copy()
    desc_h[field][image] = value
    with pytest.raises(_lib.DjError) as e:
        kernels.image_prep(src_d, desc_d, desc_h, pool_d, pool_h, t, out, scratch)
    assert "image %d" % image in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == sentinel).all()) and bool((scratch == sentinel).all())


def test_emitter_reuses_its_buffers_and_batches_do_not_disturb_each_other(cuda):
    """Several batches of different sizes through one DeviceImagePrep, queued without a synchronise in between: each
    lands in the caller's buffers as its own host statement, and the steady state allocates nothing."""
    from jpeg_detection_resnet_ssd_amd.data.image_prep import DeviceImagePrep
    rng = np.random.default_rng(35)
    prep = DeviceImagePrep(target_length=64, deconv=True)
    batches = [prep(*_ragged_batch(rng, shapes, 64)) for shapes in
               ([(150, 200)] * 3 + [(90, 70)], [(300, 400), (64, 64), (100, 64), (64, 100)], [(80, 120)] * 4,
                [(150, 200), (200, 150), (33, 44), (500, 300)], [(70, 90), (91, 71), (64, 80), (128, 128)])]
    outs = [[torch.full(s, float("nan"), device=cuda) for s in b.shapes] for b in batches]
    for b, o in zip(batches, outs):
        b.emit_into(o)
    torch.cuda.synchronize()
    for b, o in zip(batches, outs):
        for got, want in zip(o, b.numpy()):
            assert torch.equal(got.cpu(), torch.from_numpy(want))
    st = prep._state[str(cuda)]

    def held():
        return [st["blob"].data_ptr(), st["scratch"].data_ptr(), st["out"].data_ptr()] + [s[0].data_ptr() for s in st["slots"]]
    for b, o in zip(batches, outs):      # five batches over two staging buffers: after this round each has held the largest
        b.emit_into(o)
    before = held()
    for _ in range(2):
        for b, o in zip(batches, outs):
            b.emit_into(o)
    torch.cuda.synchronize()
    assert held() == before
    for got, want in zip(outs[-1], batches[-1].numpy()):
        assert torch.equal(got.cpu(), torch.from_numpy(want))


def test_call_is_capturable_in_a_graph(cuda):
    """No synchronisation inside dj_image_prep: the two passes can be captured and replayed on new pixels."""
    from jpeg_detection_resnet_ssd_amd import kernels
    from jpeg_detection_resnet_ssd_amd.data.image_prep import BatchPlan, prep_host
    rng = np.random.default_rng(36)
    t = 48
    images, params = _ragged_batch(rng, [(100, 140), (140, 100), (60, 60)], t)
    plan = BatchPlan([im.shape[:2] for im in images], params, t)
    blob_host, blob = _staged(plan, images, cuda)
    out = torch.zeros((3, t, t, 3), dtype=torch.uint8, device=cuda)
    scratch = torch.zeros(plan.scratch_bytes, dtype=torch.uint8, device=cuda)
    src_h, desc_h, pool_h = plan.views(blob_host)
    src_d, desc_d, pool_d = plan.views(blob)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kernels.image_prep(src_d, desc_d, desc_h, pool_d, pool_h, t, out, scratch,
                           stream=torch.cuda.current_stream().cuda_stream)
    fresh = [rng.integers(0, 256, im.shape, dtype=np.uint8) for im in images]       # same sizes: the plan still holds
    plan.fill(blob_host, fresh)
    blob.copy_(torch.from_numpy(blob_host))
    graph.replay()
    torch.cuda.synchronize()
    for i, (im, (s, o, f)) in enumerate(zip(fresh, params)):
        assert np.array_equal(out[i].cpu().numpy(), prep_host(im, t, s, o, f)), i


def test_classifier_fed_with_decoded_images_equals_classifier_fed_with_host_inputs(cuda):
    """Batch 4, ResNet50-DCT classifier: predict_on_batch(PendingImageInputs) returns exactly what
    predict_on_batch(pending.numpy()) returns, and `predict` (which slices the batch) agrees."""
    from jpeg_detection_resnet_ssd_amd.data.image_prep import DeviceImagePrep
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras.losses import categorical_crossentropy
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import SGD
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.networks.resnet_dct import ResNet50Custom
    K.clear_session()
    K.set_random_seed(11)
    rng = np.random.default_rng(37)
    shapes = [(375, 500), (500, 375), (300, 300), (256, 341)]
    images = []
    for h, w in shapes:
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([127 + 110 * np.sin(xx / (9.0 + c) + c) * np.cos(yy / (7.0 + 2 * c)) for c in range(3)], axis=-1)
        images.append(np.clip(img + rng.normal(0, 10, img.shape), 0, 255).astype(np.uint8))
    params = [(True, 40, True), (True, 0, False), (True, 0, True), (False, 0, False)]
    pending = DeviceImagePrep(target_length=224, deconv=False)(images, params)
    host_x = pending.numpy()
    model = ResNet50Custom(weights=None, archi="late_concat_rfa_thinner")
    model.compile(loss=categorical_crossentropy, optimizer=SGD(lr=0.1, momentum=0.9, decay=1e-4, nesterov=True))
    want = model.predict_on_batch(host_x)
    got = model.predict_on_batch(pending)
    torch.cuda.synchronize()
    for buf, h in zip(model._plan(4, False, False).inputs, host_x):
        assert torch.equal(buf.detach().cpu(), torch.from_numpy(h))
    assert want.shape == (4, 1000) and np.isfinite(want).all()
    assert np.array_equal(got, want)
    assert np.array_equal(model.predict(pending, batch_size=4), want)
    assert np.array_equal(model.predict_on_batch(host_x), want)
