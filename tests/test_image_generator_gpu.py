"""dj_rgb_warp and the device path of keras.preprocessing.image on the GPU: everything bit for bit against the in-tree
statement (data/rgb_warp.py), which tests/test_image_generator_cpu.py compares with scipy."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def _records(shape, n):
    """`n` records for images of `shape`: identity, the reference's ranges, zoom 0.8 (coordinates leave the image on all
    sides), zoom 1.2, 45 degrees with 20 degrees of shear, a fractional shift, each flip alone and both together -- in
    that order, cut or cycled to `n`."""
    from jpeg_detection_resnet_ssd_amd.data.rgb_warp import make_record, pack_records
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import affine_matrix
    rng = np.random.default_rng(1000 * shape[0] + shape[1])

    def reference_draw():
        return affine_matrix(shape, rng.uniform(-0.2, 0.2), 0, 0, rng.uniform(-0.2, 0.2), rng.uniform(0.8, 1.2),
                             rng.uniform(0.8, 1.2))

    kinds = [
        lambda: make_record(None),
        lambda: make_record(reference_draw()),
        lambda: make_record(affine_matrix(shape, zx=0.8, zy=0.8)),
        lambda: make_record(affine_matrix(shape, zx=1.2, zy=1.2)),
        lambda: make_record(affine_matrix(shape, theta=45, shear=20)),
        lambda: make_record(affine_matrix(shape, tx=3.5, ty=-2.25)),
        lambda: make_record(None, flip_cols=True),
        lambda: make_record(reference_draw(), flip_rows=True),
        lambda: make_record(affine_matrix(shape, theta=-30, zx=0.9, zy=1.1), flip_cols=True, flip_rows=True),
        lambda: make_record(None, flip_cols=True, flip_rows=True),
        lambda: make_record(reference_draw(), flip_cols=True),
    ]
    return pack_records([kinds[k % len(kinds)]() for k in range(n)])


def _out_buffer(cuda, shape, layout):
    """-> (whole buffer, the (B, H, W, 3) view the kernel writes): 'dense' is 16-byte aligned and contiguous, 'offset' is
    contiguous from a base 4 bytes past such an address, 'rows4' / 'rows5' have 4 / 5 floats of padding behind every row."""
    b, h, w, _ = shape
    if layout in ("dense", "offset"):
        lead = 0 if layout == "dense" else 1
        whole = torch.full((lead + b * h * w * 3 + 8,), SENTINEL, dtype=torch.float32, device=cuda)
        view = whole[lead:lead + b * h * w * 3].view(b, h, w, 3)
        assert view.data_ptr() % 16 == (0 if layout == "dense" else 4)
        return whole, view
    pad = 4 if layout == "rows4" else 5
    row = 3 * w + pad
    row += (-row) % 4 if layout == "rows4" else 0          # rows4: every row starts 16-byte aligned
    if layout == "rows5" and row % 4 == 0:
        row += 1
    whole = torch.full((b, h, row), SENTINEL, dtype=torch.float32, device=cuda)
    return whole, whole[:, :, :3 * w].unflatten(2, (w, 3))


def _check_untouched(whole, view, layout):
    host = whole.cpu().numpy()
    if layout in ("dense", "offset"):
        lead = 0 if layout == "dense" else 1
        assert (host[:lead] == SENTINEL).all() and (host[lead + view.numel():] == SENTINEL).all()
    else:
        assert (host[:, :, 3 * view.shape[2]:] == SENTINEL).all()


SHAPES = [(1, 1), (1, 7), (2, 3), (5, 7), (17, 23), (16, 16)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_kernel_equals_the_statement(cuda, shape):
    """Eleven images per batch (17 x 23: 4301 pixels, a scalar tail behind the 16-byte stores; 16 x 16: none), preprocessing
    code 0 and 1, with and without rescale, into each output layout."""
    from jpeg_detection_resnet_ssd_amd import kernels
    from jpeg_detection_resnet_ssd_amd.data.rgb_warp import rgb_warp_host
    n = 11 if shape != (16, 16) else 12
    pixels = np.random.default_rng(shape[0] * 31 + shape[1]).integers(0, 256, size=(n,) + shape + (3,)).astype(np.uint8)
    recs = _records(shape, n)
    pix_dev = torch.from_numpy(pixels).to(cuda)
    rec_dev = torch.from_numpy(recs.view(np.uint8).reshape(-1)).to(cuda)
    for prep in (0, 1):
        for rescale in (None, 1 / 255.):
            want = rgb_warp_host(pixels, recs, prep, rescale)
            for layout in ("dense", "offset", "rows4", "rows5"):
                whole, view = _out_buffer(cuda, pixels.shape, layout)
                kernels.rgb_warp(pix_dev, rec_dev, recs, view, prep, rescale)
                got = view.cpu().numpy()
                bad = got != want
                assert not bad.any(), (prep, rescale, layout, int(bad.sum()), np.argwhere(bad)[:4].tolist())
                _check_untouched(whole, view, layout)


def test_kernel_equals_the_statement_at_224(cuda):
    from jpeg_detection_resnet_ssd_amd import kernels
    from jpeg_detection_resnet_ssd_amd.data.rgb_warp import rgb_warp_device, rgb_warp_host
    shape = (224, 224)
    pixels = np.random.default_rng(224).integers(0, 256, size=(4,) + shape + (3,)).astype(np.uint8)
    recs = _records(shape, 11)[[1, 2, 4, 8]]
    want = rgb_warp_host(pixels, recs, 1, None)
    got = rgb_warp_device(pixels, recs, 1, None, device=cuda)
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want)
    whole, view = _out_buffer(cuda, pixels.shape, "rows4")
    rgb_warp_device(pixels, recs, 0, 1 / 255., out=view)
    assert np.array_equal(view.cpu().numpy(), rgb_warp_host(pixels, recs, 0, 1 / 255.))
    _check_untouched(whole, view, "rows4")
    with pytest.raises(AssertionError, match="out"):
        kernels.rgb_warp(torch.from_numpy(pixels).to(cuda), torch.zeros(256, dtype=torch.uint8, device=cuda), recs,
                         torch.empty((4, 224, 224, 4), device=cuda))


# ---- through the model --------------------------------------------------------------------------------------------------
def _write_tree(root):
    from PIL import Image
    rng = np.random.default_rng(5)
    sizes = [(14, 10), (20, 13), (9, 31), (40, 30), (7, 5), (15, 11), (33, 18)]
    for k, size in enumerate(sizes):
        directory = os.path.join(root, "class%d" % (k % 3))
        os.makedirs(directory, exist_ok=True)
        mode = "L" if k == 1 else "RGB"
        shape = (size[1], size[0]) + ((3,) if mode == "RGB" else ())
        Image.fromarray(rng.integers(0, 256, size=shape).astype(np.uint8), mode).save(os.path.join(directory, "img%d.png" % k))
    return root


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return _write_tree(str(tmp_path_factory.mktemp("rgb_tree_gpu")))


def _iterator(tree, device_prep, target=(10, 14), batch_size=4, seed=17):
    from jpeg_detection_resnet_ssd_amd.keras.applications.vgg16 import preprocess_input
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import ImageDataGenerator
    gen = ImageDataGenerator(rotation_range=20, shear_range=10, zoom_range=0.2, width_shift_range=0.1, vertical_flip=True,
                             horizontal_flip=True, rescale=1 / 64., preprocessing_function=preprocess_input)
    return gen.flow_from_directory(tree, target_size=target, batch_size=batch_size, seed=seed, device_prep=device_prep)


def _small_model(seed=5):
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras import layers as L
    from jpeg_detection_resnet_ssd_amd.keras.models import Model
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import SGD
    K.clear_session()
    K.set_random_seed(seed)
    x = L.Input(shape=(10, 14, 3))
    h = L.Conv2D(8, (3, 3), padding="same", activation="relu", name="conv")(x)
    y = L.Dense(3, activation="softmax", name="probs")(L.GlobalAveragePooling2D(name="pool")(h))
    model = Model(x, y)
    model.compile(optimizer=SGD(lr=0.05, momentum=0.9), loss="categorical_crossentropy")
    return model


@pytest.fixture
def one_k_range():
    """The weight gradient of the small model's convolution sums over 4 * 10 * 14 = 560 pixels; the launcher would split
    that range over workgroups that add their parts with fp32 atomics (DESIGN: wgrad), in an order that differs from run
    to run.  Registered with one K range, the step is a function of its input, and two steps can be compared bit for bit."""
    import ctypes
    from jpeg_detection_resnet_ssd_amd import _lib, kernels
    lib = _lib.load()
    desc = kernels.make_conv_desc(4, 10, 14, 3, 8, (3, 3), (1, 1), "same")
    cfg, splits = ctypes.c_int(), ctypes.c_int()
    _lib.check(lib.dj_conv2d_default_config(2, desc, ctypes.byref(cfg), ctypes.byref(splits)), "default_config")
    _lib.check(lib.dj_conv2d_tune_set(2, desc, cfg.value, 1), "tune_set")
    yield
    _lib.check(lib.dj_conv2d_tune_set(2, desc, -1, 1), "tune_set")


def test_training_step_fed_by_the_device_path_equals_the_host_path(cuda, tree, one_k_range):
    from jpeg_detection_resnet_ssd_amd.data.rgb_warp import PendingRGBInputs
    x_host, y_host = _iterator(tree, False)[0]
    x_dev, y_dev = _iterator(tree, True)[0]
    assert isinstance(x_dev, PendingRGBInputs) and np.array_equal(y_dev, y_host) and x_host.shape == (4, 10, 14, 3)
    results = []
    for x in (x_host, x_dev, x_host):
        model = _small_model()
        loss = model.train_on_batch(x, y_host)
        torch.cuda.synchronize()
        results.append((loss, model.get_weights_dict(), model._plan(4, True, True).inputs[0].cpu().numpy()))
    again = results.pop()                      # the host path a second time: the step itself repeats bit for bit
    assert again[0] == results[0][0] and all(np.array_equal(again[1][k], v) for k, v in results[0][1].items())
    (loss_h, w_h, in_h), (loss_d, w_d, in_d) = results
    assert np.array_equal(in_h, x_host) and np.array_equal(in_d, x_host)       # the plan's input buffer is the host array
    assert math.isfinite(loss_h) and loss_d == loss_h
    assert sorted(w_d) == sorted(w_h)
    for key in w_h:
        assert np.array_equal(w_d[key], w_h[key]), key


def test_fit_generator_over_the_device_iterator(cuda, tree):
    from jpeg_detection_resnet_ssd_amd.keras.callbacks import Callback

    class Steps(Callback):
        def on_train_begin(self, logs=None):
            self.seen = []

        def on_batch_end(self, batch, logs=None):
            self.seen.append((logs["size"], logs["loss"]))

    steps = Steps()
    it = _iterator(tree, True, batch_size=3)
    assert len(it) == 3
    history = _small_model().fit_generator(it, epochs=1, verbose=0, callbacks=[steps])
    assert [s for s, _ in steps.seen] == [3, 3, 1]                  # the short last batch went through
    assert all(math.isfinite(v) for _, v in steps.seen) and math.isfinite(history.history["loss"][0])


def test_resnet50_rgb_predicts_the_same_from_both_paths(cuda, tree):
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.networks.resnet_dct import ResNet50RGB
    x_host, _ = _iterator(tree, False, target=(224, 224))[0]
    x_dev, _ = _iterator(tree, True, target=(224, 224))[0]
    K.clear_session()
    K.set_random_seed(3)
    model = ResNet50RGB(weights=None)
    from_host = model.predict(x_host, batch_size=4)
    from_dev = model.predict(x_dev, batch_size=4)
    assert from_host.shape == (4, 1000) and np.isfinite(from_host).all()
    assert np.array_equal(from_dev, from_host)
    assert np.array_equal(model._plan(4, False, False).inputs[0].cpu().numpy(), x_host)
