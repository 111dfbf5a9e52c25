"""GPU: `device_decode` for the two classifier input pipelines -- dj_jpeg_pixels in front of dj_image_prep (`BatchPlan`) and
in front of dj_patch_resize and dj_rgb_warp (`PendingRGBFileInputs`), against the host statements and Pillow's pixels, and
through one small model per pipeline.  No tolerance anywhere: every comparison is equality."""
import math
import random

import numpy as np
import pytest
import torch

import classifier_decode_cases as K

pytestmark = pytest.mark.gpu

FILL = 0xA5
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def jp():
    from jpeg_detection_resnet_ssd_amd.data import jpeg_pixels
    return jpeg_pixels


@pytest.fixture(scope="module")
def batch(jp):
    """(the shared batch as a `device_decode` generator hands it over, Pillow's pixels of the same files)."""
    _, mixed, arrays = K.items(jp)
    assert K.coefficient_items(mixed) == K.BASELINE == [0, 1, 2, 3, 4] and isinstance(mixed[5], np.ndarray)
    return mixed, arrays


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    return (K.write_tree(str(tmp_path_factory.mktemp("dct_tree_gpu"))),
            K.write_tree(str(tmp_path_factory.mktemp("rgb_tree_gpu")), png=True))


# ---- BatchPlan: dj_jpeg_pixels, dj_image_prep, dj_photometric --------------------------------------------------------------
def _launch_prefilled(plan, images, cuda):
    """Stage `plan` in a pinned blob pre-filled with FILL (scratch too), upload and launch: a byte dj_image_prep reads that
    neither the host nor dj_jpeg_pixels wrote shows in the output."""
    staging = torch.full((plan.nbytes,), FILL, dtype=torch.uint8).pin_memory()
    host = staging.numpy()
    plan.fill(host, images, 2)
    blob = staging.to(cuda)
    out = torch.full(plan.out_shape, FILL, dtype=torch.uint8, device=cuda)
    scratch = torch.full((plan.scratch_bytes,), FILL, dtype=torch.uint8, device=cuda)
    plan.launch(host, blob, out, scratch)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _param_sets(arrays):
    from jpeg_detection_resnet_ssd_amd.data import photometric as ph
    from jpeg_detection_resnet_ssd_amd.data.image_prep import max_offset
    far = [max_offset(a.shape[0], a.shape[1], K.TARGET) for a in arrays]
    assert far == [0, 6, 0, 6, 3, 6]           # 1x1 and 16x16 have no room; the others crop along their longer side
    ops = [[(ph.LIGHTING, (0.1, 0.2, -0.1)), (ph.CONTRAST, (0.9,))], [], [(ph.SATURATION, (1.3,))], [(ph.BRIGHTNESS, (0.7,))],
           [(ph.CONTRAST, (1.2,)), (ph.SATURATION, (0.6,)), (ph.BRIGHTNESS, (1.1,)), (ph.LIGHTING, (-0.3, 0.0, 0.2))], []]
    return {"scale": ([(True, 0, False)] * 6, None),
            "far_offset_flip": ([(True, o, True) for o in far], None),
            "no_scale": ([(False, 0, bool(i % 2)) for i in range(6)], None),
            "photometric": ([(True, o // 2, bool(i % 2)) for i, o in enumerate(far)], ops)}


@pytest.mark.parametrize("case", ["scale", "far_offset_flip", "no_scale", "photometric"])
def test_prep_device_on_coefficient_items_equals_prep_host_of_pillows_pixels(cuda, batch, case):
    from jpeg_detection_resnet_ssd_amd.data import device_staging as ds, image_prep as ip
    from jpeg_detection_resnet_ssd_amd.data.photometric import photometric_host
    mixed, arrays = batch
    params, ops = _param_sets(arrays)[case]
    want = np.stack([ip.prep_host(a, K.TARGET, s, o, f) for a, (s, o, f) in zip(arrays, params)])
    if ops is not None:
        want = photometric_host(want, ops)
    plan = ip.BatchPlan(ds.plan_items(mixed), params, K.TARGET, ops=ops)
    assert plan.decode_items == K.BASELINE
    got = _launch_prefilled(plan, mixed, cuda)
    bad = got != want
    assert not bad.any(), (case, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert np.array_equal(ip.prep_device(mixed, params, K.TARGET, device=cuda, ops=ops, n_threads=2).cpu().numpy(), want)
    # all coefficients, and a batch of one
    assert np.array_equal(ip.prep_device(mixed[:5], params[:5], K.TARGET, device=cuda, n_threads=1,
                                         ops=None if ops is None else ops[:5]).cpu().numpy(), want[:5])
    assert np.array_equal(ip.prep_device(mixed[3:4], params[3:4], K.TARGET, device=cuda,
                                         ops=None if ops is None else ops[3:4]).cpu().numpy(), want[3:4])


def test_two_dct_batches_through_the_same_resident_buffers(cuda, batch):
    """The second batch is larger: the blob grows and both pinned slots are used; nothing synchronises in between."""
    from jpeg_detection_resnet_ssd_amd.data.image_prep import DeviceImagePrep
    mixed, arrays = batch
    params = _param_sets(arrays)["far_offset_flip"][0]
    prep = DeviceImagePrep(K.TARGET, deconv=True, n_threads=2)
    first, second = prep(mixed[:2], params[:2]), prep(mixed[::-1], params[::-1])
    assert second.plan.nbytes > first.plan.nbytes
    pendings = [first, second, first]
    outs = [[torch.full(s, float("nan"), device=cuda) for s in p.shapes] for p in pendings]
    for p, o in zip(pendings, outs):
        p.emit_into(o)
    torch.cuda.synchronize()
    st = prep._state[str(cuda)]
    assert all(slot[0] is not None for slot in st["slots"]) and st["blob"].numel() >= second.plan.nbytes
    for p, o, images in zip(pendings, outs, (arrays[:2], arrays[::-1], arrays[:2])):
        want = prep(images, p.params).numpy()           # the statement from Pillow's pixels
        for got, w in zip(o, want):
            assert torch.equal(got.cpu(), torch.from_numpy(w))


# ---- the RGB pending inputs: dj_jpeg_pixels, dj_patch_resize, dj_rgb_warp --------------------------------------------------
def _records(n):
    """Identity, warps whose coordinates leave the image, each flip alone and both together, cycled to `n`."""
    from jpeg_detection_resnet_ssd_amd.data.rgb_warp import make_record, pack_records
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import affine_matrix
    shape = K.RGB_TARGET + (3,)
    kinds = [make_record(None),
             make_record(affine_matrix(shape, theta=0.15, shear=-0.1, zx=0.9, zy=1.15)),
             make_record(affine_matrix(shape, zx=0.8, zy=0.8), flip_rows=True),
             make_record(None, flip_cols=True),
             make_record(affine_matrix(shape, theta=45, shear=20), flip_cols=True, flip_rows=True),
             make_record(affine_matrix(shape, tx=3.5, ty=-2.25)),
             make_record(None, flip_cols=True, flip_rows=True)]
    return pack_records([kinds[k % len(kinds)] for k in range(n)])


def _rgb_items(batch):
    """The shared batch plus an array of the target's size, which the resize must leave as it is."""
    import jpeg_pixels_cases as C
    mixed, arrays = batch
    same = C.content("noise", K.RGB_TARGET[0], K.RGB_TARGET[1], seed=9)
    return mixed + [same], arrays + [same]


def _out_buffer(cuda, shape, layout):
    """-> (whole buffer, the (B, H, W, 3) view written): 'dense' is 16-byte aligned and contiguous, 'offset' contiguous
    from 4 bytes past such an address, 'rows' has 5 floats of padding behind every row."""
    b, h, w, _ = shape
    if layout == "rows":
        whole = torch.full((b, h, 3 * w + 5), SENTINEL, dtype=torch.float32, device=cuda)
        return whole, whole[:, :, :3 * w].unflatten(2, (w, 3))
    lead = 0 if layout == "dense" else 1
    whole = torch.full((lead + b * h * w * 3 + 8,), SENTINEL, dtype=torch.float32, device=cuda)
    view = whole[lead:lead + b * h * w * 3].view(b, h, w, 3)
    assert view.data_ptr() % 16 == (0 if layout == "dense" else 4)
    return whole, view


def _untouched(whole, view, layout):
    host = whole.cpu().numpy()
    if layout == "rows":
        return bool((host[:, :, 3 * view.shape[2]:] == SENTINEL).all())
    lead = 0 if layout == "dense" else 1
    return bool((host[:lead] == SENTINEL).all() and (host[lead + view.numel():] == SENTINEL).all())


@pytest.mark.parametrize("interpolation", ["nearest", "bilinear"])
def test_rgb_pending_inputs_equal_their_host_statement(cuda, batch, interpolation):
    from jpeg_detection_resnet_ssd_amd.data import device_staging as ds
    from jpeg_detection_resnet_ssd_amd.data.rgb_warp import PendingRGBFileInputs, rgb_warp_host
    images, arrays = _rgb_items(batch)
    records = _records(len(images))
    stager = ds.StagingBuffers(2)
    for preprocess, rescale in ((0, None), (1, None), (0, 1 / 255.), (1, 1 / 64.)):
        pending = PendingRGBFileInputs(images, records, K.RGB_TARGET, interpolation, preprocess, rescale, stager)
        assert K.coefficient_items(pending.images) == K.BASELINE and pending.plan.decode_items == K.BASELINE
        # the statement, from Pillow's pixels and Pillow's resize
        from PIL import Image
        pillow = np.stack([np.asarray(Image.fromarray(a).resize(K.RGB_TARGET[::-1], pending.resample))
                           if a.shape[:2] != K.RGB_TARGET else a for a in arrays])
        assert np.array_equal(pending.pixels(), pillow)
        want = pending.numpy()[0]
        assert np.array_equal(want, rgb_warp_host(pillow, records, preprocess, rescale))
        for layout in ("dense", "rows", "offset"):
            whole, view = _out_buffer(cuda, pending.shape, layout)
            pending.emit_into([view])
            got = view.cpu().numpy()
            bad = got != want
            assert not bad.any(), (preprocess, rescale, layout, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            assert _untouched(whole, view, layout)
    with pytest.raises(ValueError, match="emit_into"):
        pending.emit_into([torch.empty((2,) + K.RGB_TARGET + (3,), device=cuda)])


def test_two_rgb_batches_through_the_same_resident_buffers(cuda, batch):
    from jpeg_detection_resnet_ssd_amd.data import device_staging as ds
    from jpeg_detection_resnet_ssd_amd.data.rgb_warp import PendingRGBFileInputs
    images, _ = _rgb_items(batch)
    records = _records(len(images))
    stager = ds.StagingBuffers(2)
    whole = PendingRGBFileInputs(images, records, K.RGB_TARGET, "bilinear", 1, None, stager)
    first, second = whole[5:7], whole[::-1]
    assert second.plan.nbytes > first.plan.nbytes and K.coefficient_items(first.images) == []
    pendings = [first, second, whole[1:3]]
    outs = [torch.full(p.shape, float("nan"), device=cuda) for p in pendings]
    for p, o in zip(pendings, outs):
        p.emit_into([o])
    torch.cuda.synchronize()
    st = stager._state[str(cuda)]
    assert all(slot[0] is not None for slot in st["slots"]) and st["blob"].numel() >= second.plan.nbytes
    for p, o in zip(pendings, outs):
        assert np.array_equal(o.cpu().numpy(), p.numpy()[0])


# ---- one small model per pipeline -------------------------------------------------------------------------------------------
def _compiled(inputs, features):
    from jpeg_detection_resnet_ssd_amd.keras import layers as L
    from jpeg_detection_resnet_ssd_amd.keras.models import Model
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import SGD
    h = L.Conv2D(8, (3, 3), padding="same", activation="relu", name="conv")(features)
    y = L.Dense(3, activation="softmax", name="probs")(L.GlobalAveragePooling2D(name="pool")(h))
    model = Model(inputs, y)
    model.compile(optimizer=SGD(lr=0.05, momentum=0.9), loss="categorical_crossentropy")
    return model


def _finite_training(model, generator, steps):
    from jpeg_detection_resnet_ssd_amd.keras.callbacks import Callback

    class Steps(Callback):
        def on_train_begin(self, logs=None):
            self.seen = []

        def on_batch_end(self, batch, logs=None):
            self.seen.append(logs["loss"])

    seen = Steps()
    history = model.fit_generator(generator, steps_per_epoch=steps, epochs=1, verbose=0, callbacks=[seen])
    assert len(seen.seen) == steps and all(math.isfinite(v) for v in seen.seen) and math.isfinite(history.history["loss"][0])
    assert math.isfinite(model.evaluate_generator(generator))


def test_dct_model_fed_by_device_decode_equals_device_prep(cuda, trees):
    from jpeg_detection_resnet_ssd_amd.keras import backend as B
    from jpeg_detection_resnet_ssd_amd.keras import layers as L
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import DCTGeneratorJPEG2DCT
    directory, index_file = trees[0]

    def generator(**kw):
        return DCTGeneratorJPEG2DCT(directory, index_file, batch_size=3, shuffle=False, target_length=K.TARGET,
                                    device_prep=True, **kw)
    B.clear_session()
    B.set_random_seed(5)
    iy, icc = L.Input(shape=(2, 2, 64)), L.Input(shape=(1, 1, 128))
    model = _compiled([iy, icc], L.Concatenate(axis=-1)([iy, L.UpSampling2D()(icc)]))
    decode, prep = generator(device_decode=True, decode_threads=2), generator()
    for index in (0, 1):
        random.seed(21 + index)
        x_decode, y_decode = decode[index]
        random.seed(21 + index)
        x_prep, y_prep = prep[index]
        # batch 0 reads files 0, 3, 1 and batch 1 files 4, 2 and the progressive one, which alone is decoded on the host
        assert K.coefficient_items(x_decode.images) == ([0, 1, 2] if index == 0 else [0, 1])
        assert K.coefficient_items(x_prep.images) == [] and np.array_equal(y_decode, y_prep)
        buffers = []
        for x in (x_decode, x_prep):
            model.predict_on_batch(x)
            torch.cuda.synchronize()
            buffers.append([b.detach().cpu().numpy().copy() for b in model._plan(3, False, False).inputs])
        for got, want, host in zip(buffers[0], buffers[1], x_prep.numpy()):
            assert np.array_equal(got, want) and np.array_equal(got, host)
    _finite_training(model, decode, 2)


def test_rgb_model_fed_by_device_decode_equals_device_prep(cuda, trees):
    from jpeg_detection_resnet_ssd_amd.keras import backend as B
    from jpeg_detection_resnet_ssd_amd.keras import layers as L
    from jpeg_detection_resnet_ssd_amd.keras.applications.vgg16 import preprocess_input
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import ImageDataGenerator
    tree = trees[1][0]

    def iterator(**kw):
        gen = ImageDataGenerator(rotation_range=20, shear_range=10, zoom_range=0.2, width_shift_range=0.1, vertical_flip=True,
                                 horizontal_flip=True, rescale=1 / 64., preprocessing_function=preprocess_input)
        return gen.flow_from_directory(tree, target_size=K.RGB_TARGET, batch_size=4, seed=17, shuffle=False,
                                       interpolation="bilinear", device_prep=True, **kw)
    B.clear_session()
    B.set_random_seed(5)
    x = L.Input(shape=K.RGB_TARGET + (3,))
    model = _compiled(x, x)
    decode, prep = iterator(device_decode=True, decode_threads=2), iterator()
    assert len(decode) == 2
    for index, coefficients in ((0, [0, 1, 3]), (1, [0, 1])):          # the PNG is item 2 of batch 0, the progressive file the last
        x_decode, y_decode = decode[index]
        x_prep, y_prep = prep[index]
        assert K.coefficient_items(x_decode.images) == coefficients and np.array_equal(y_decode, y_prep)
        buffers = []
        for pending in (x_decode, x_prep):
            model.predict_on_batch(pending)
            torch.cuda.synchronize()
            buffers.append(model._plan(len(pending), False, False).inputs[0].detach().cpu().numpy().copy())
        assert np.array_equal(buffers[0], buffers[1]) and np.array_equal(buffers[0], x_prep.numpy()[0])
    _finite_training(model, decode, 2)
