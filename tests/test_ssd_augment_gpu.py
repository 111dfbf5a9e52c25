"""GPU: csrc/dj_patchresize.hip takes a window of each image of a ragged batch on a background, mirrors and resizes it
into exactly the bytes the numpy + Pillow statement gives (data/patch_resize.py:patch_resize_host), whatever the window,
the filter or the output stride; rejected arguments write nothing; and a model fed the decoded images and their geometries
computes what it computes when fed the host-made inputs.  Equality throughout: the arithmetic is integer only."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX = 0, 1, 2, 3, 4
FILTERS = [NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX]
BG = (123, 117, 104)
SHAPES = [(64, 48), (1, 1), (37, 53), (48, 64), (20, 21), (5, 3)]


def _images(seed, shapes=SHAPES):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def _windows(h, w):
    """Inside the image, starting negative, past both far edges, wholly larger (an expand), one pixel, and off the image."""
    return [(h // 4, w // 5, max(1, h // 2), max(1, w // 2)), (-3, -5, h + 1, w + 2), (h // 2, w // 3, h, w + 4),
            (-h - 7, -2 * w, 3 * h + 9, 4 * w + 1), (h - 1, w // 2, 1, 1), (h + 2, -9, 4, 6)]


def _main_cases():
    """Batches of the six images; batch k gives image i its window of kind (i + k) mod 6, filter i mod 5 and alternating
    flips, so that six batches pair every image, and with it every filter, with every kind of window."""
    for k in range(6):
        yield [_windows(h, w)[(i + k) % 6] + (bool((i + k // 2) % 2), FILTERS[i % 5], BG if i % 2 else (7, 250, 0))
               for i, (h, w) in enumerate(SHAPES)]


def test_ragged_batch_equals_the_host_twin(cuda):
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import patch_resize_device, patch_resize_host
    images = _images(41)
    seen = set()
    for k, geometries in enumerate(_main_cases()):
        got = patch_resize_device(images, geometries, 24, 20, device=cuda).cpu().numpy()
        assert got.shape == (6, 24, 20, 3)
        for i, (im, g) in enumerate(zip(images, geometries)):
            want = patch_resize_host(im, g, 24, 20)
            bad = got[i] != want
            assert not bad.any(), (im.shape, g, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            seen.add(((i + k) % 6, g[4], g[5]))
    assert {(w, f) for w, _, f in seen} == {(w, f) for w in range(6) for f in FILTERS} and {fl for _, fl, _ in seen} == {False, True}


@pytest.mark.parametrize("resample, flip", [(NEAREST, False), (LANCZOS, True), (BILINEAR, True), (BICUBIC, False), (BOX, True)])
def test_expanded_full_size_image_equals_the_host_twin(cuda, resample, flip):
    """375 x 500 on a canvas four times its size, to 300 x 300: 1500 window rows of up to 41 taps, most of them background."""
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import patch_resize_device, patch_resize_host
    image = _images(42, [(375, 500)])[0]
    geometry = (-700, -1100, 1500, 2000, flip, resample, BG)
    got = patch_resize_device([image], [geometry], 300, 300, device=cuda).cpu().numpy()[0]
    want = patch_resize_host(image, geometry, 300, 300)
    assert (want != np.array(BG, dtype=np.uint8)).any(axis=-1).sum() > 5000      # the image is in the picture
    assert np.array_equal(got, want), int((got != want).sum())


def _staged(plan, images, cuda):
    blob_host = np.zeros(plan.nbytes, dtype=np.uint8)
    plan.fill(blob_host, images)
    return blob_host, torch.from_numpy(blob_host).to(cuda)


def test_strided_output_leaves_everything_else_untouched(cuda):
    """Rows of 3 * 20 bytes inside rows of 100: the bytes between rows, a guard band behind the tensor, the scratch past
    what the plan uses and the staged inputs keep their sentinel / their content."""
    from jpeg_detection_resnet_ssd_amd import kernels
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import PatchPlan, patch_resize_host
    images = _images(43)
    geometries = list(_main_cases())[1]
    oh, ow, pitch, guard, sentinel = 24, 20, 100, 4096, 0xA5
    plan = PatchPlan([im.shape[:2] for im in images], geometries, oh, ow)
    blob_host, blob = _staged(plan, images, cuda)
    flat = torch.full((6 * oh * pitch + guard,), sentinel, dtype=torch.uint8, device=cuda)
    out = flat[:6 * oh * pitch].view(6, oh, pitch)[:, :, :3 * ow].unflatten(2, (ow, 3))
    assert out.stride() == (oh * pitch, pitch, 3, 1)
    scratch = torch.full((plan.scratch_bytes + guard,), sentinel, dtype=torch.uint8, device=cuda)
    src_h, desc_h, pool_h = plan.views(blob_host)
    src_d, desc_d, pool_d = plan.views(blob)
    assert kernels.patch_resize_scratch_bytes(desc_h, ow) == plan.scratch_bytes
    kernels.patch_resize(src_d, desc_d, desc_h, pool_d, pool_h, out, scratch)
    torch.cuda.synchronize()
    for i, (im, g) in enumerate(zip(images, geometries)):
        assert np.array_equal(out[i].cpu().numpy(), patch_resize_host(im, g, oh, ow)), i
    rows = flat[:6 * oh * pitch].view(6 * oh, pitch)
    assert bool((rows[:, 3 * ow:] == sentinel).all()) and bool((flat[-guard:] == sentinel).all())
    assert bool((scratch[plan.scratch_bytes:] == sentinel).all())
    assert np.array_equal(blob.cpu().numpy(), blob_host)


@pytest.mark.parametrize("field, image, value, short_scratch", [
    ("win_h", 0, 0, False), ("win_w", 1, 0, False), ("win_w", 0, -3, False), ("h_bounds", 1, 1 << 30, False),
    ("v_taps", 0, 1 << 30, False), ("h_taps", 1, -1, False), ("scratch_offset", 1, 0, False), ("src_offset", 1, 1 << 40, False),
    ("src_h", 0, 500, False), ("win_w", 0, 25, False), ("win_y0", 1, 1 << 28, False), (None, 1, 0, True),
])
def test_rejected_arguments_return_an_error_and_write_nothing(cuda, field, image, value, short_scratch):
    from jpeg_detection_resnet_ssd_amd import _lib, kernels
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import PatchPlan
    images = _images(44, [(50, 70), (70, 50)])
    geometries = [(-5, 3, 40, 60, True, BICUBIC, BG), (10, -8, 70, 66, False, LANCZOS, BG)]
    sentinel = 0x5A
    plan = PatchPlan([im.shape[:2] for im in images], geometries, 24, 20)
    blob_host, blob = _staged(plan, images, cuda)
    out = torch.full((2, 24, 20, 3), sentinel, dtype=torch.uint8, device=cuda)
    scratch = torch.full((plan.scratch_bytes - (64 if short_scratch else 0),), sentinel, dtype=torch.uint8, device=cuda)
    src_h, desc_h, pool_h = plan.views(blob_host)
    src_d, desc_d, pool_d = plan.views(blob)
    desc_h = desc_h.copy()
    if field is not None:
        desc_h[field][image] = value
    with pytest.raises(_lib.DjError) as e:
        kernels.patch_resize(src_d, desc_d, desc_h, pool_d, pool_h, out, scratch)
    assert "image %d" % image in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == sentinel).all()) and bool((scratch == sentinel).all())


@pytest.mark.parametrize("deconv", [False, True])
def test_emission_into_model_buffers_equals_the_host_statement(cuda, deconv):
    """Batches of different sizes through one DevicePatchResize, queued without a synchronise in between, then a slice."""
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import DevicePatchResize
    images = _images(45)
    prep = DevicePatchResize(out_height=24, out_width=20, deconv=deconv)
    cases = list(_main_cases())
    batches = [prep(images, cases[0]), prep(images[:3], cases[3][:3]), prep(images, cases[4])[2:5]]
    assert len(batches[2]) == 3 and batches[2].shape == (3, 24, 20, 3)
    outs = [[torch.full(s, float("nan"), device=cuda) for s in b.shapes] for b in batches]
    for b, o in zip(batches, outs):
        b.emit_into(o)
    torch.cuda.synchronize()
    for b, o in zip(batches, outs):
        for got, want in zip(o, b.numpy()):
            assert torch.equal(got.cpu(), torch.from_numpy(want))
    whole = prep(images, cases[4]).numpy()
    assert all(np.array_equal(w[2:5], s) for w, s in zip(whole, batches[2].numpy()))
    with pytest.raises(ValueError):
        batches[0].emit_into(outs[1])


def test_classifier_fed_with_images_and_geometries_equals_classifier_fed_with_host_inputs(cuda):
    """Batch 2, ResNet50-DCT classifier (the small model the image-prep facade test builds): predict_on_batch(PendingPatchInputs)
    returns exactly what predict_on_batch(pending.numpy()) returns, and `predict`, which slices the batch, agrees."""
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import DevicePatchResize
    from jpeg_detection_resnet_ssd_amd.data.ssd_augment import SSDDataAugmentation
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras.losses import categorical_crossentropy
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import SGD
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.networks.resnet_dct import ResNet50Custom
    K.clear_session()
    K.set_random_seed(11)
    rng = np.random.default_rng(46)
    images = []
    for h, w in [(375, 500), (333, 250)]:
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([127 + 110 * np.sin(xx / (9.0 + c) + c) * np.cos(yy / (7.0 + 2 * c)) for c in range(3)], axis=-1)
        images.append(np.clip(img + rng.normal(0, 10, img.shape), 0, 255).astype(np.uint8))
    chain = SSDDataAugmentation(224, 224)
    np.random.seed(3)
    geometries = [chain.plan(im.shape[0], im.shape[1], np.array([[1, 50, 60, 200, 220]]))[0] for im in images]
    pending = DevicePatchResize(224, 224, deconv=False)(images, geometries)
    host_x = pending.numpy()
    model = ResNet50Custom(weights=None, archi="late_concat_rfa_thinner")
    model.compile(loss=categorical_crossentropy, optimizer=SGD(lr=0.1, momentum=0.9, decay=1e-4, nesterov=True))
    want = model.predict_on_batch(host_x)
    got = model.predict_on_batch(pending)
    torch.cuda.synchronize()
    for buf, h in zip(model._plan(2, False, False).inputs, host_x):
        assert torch.equal(buf.detach().cpu(), torch.from_numpy(h))
    assert want.shape == (2, 1000) and np.isfinite(want).all()
    assert np.array_equal(got, want)
    assert np.array_equal(model.predict(pending, batch_size=2), want)
