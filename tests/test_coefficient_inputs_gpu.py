"""GPU: dj_jpeg_dct_inputs (csrc/dj_jpegdct.hip) writes, bit for bit, what data/coefficient_inputs.py states -- at the smallest
shapes where it can go wrong --, refuses bad descriptors before launching, and carries batches into a model's resident
inputs.  No tolerance anywhere: every comparison is equality, and outputs are pre-filled with NaN so that an element the
kernel did not write shows."""
import math
import random

import numpy as np
import pytest
import torch

import coefficient_inputs_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ci():
    from jpeg_detection_resnet_ssd_amd.data import coefficient_inputs
    return coefficient_inputs


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return K.write_tree(str(tmp_path_factory.mktemp("coefficient_tree_gpu")))


def _nan(cuda, shapes):
    return [torch.full(tuple(s), float("nan"), device=cuda) for s in shapes]


def _staged(pending, cuda):
    """-> (host blob, device blob) of the batch's plan, filled on 2 threads into a blob pre-filled with 0xA5."""
    staging = np.full(pending.plan.nbytes, 0xA5, dtype=np.uint8)
    pending.plan.fill(staging, pending.images, 2)
    return staging, torch.from_numpy(staging).to(cuda)


def _kernel_equals_statement(ci, cuda, files, windows=None, flips=None, deconv=False):
    pending = ci.DeviceCoefficientInputs(deconv=deconv)(files, windows, flips)
    host, blob = _staged(pending, cuda)
    outs = _nan(cuda, pending.shapes)
    pending.plan.launch(host, blob, outs)
    torch.cuda.synchronize()
    want = pending.numpy()
    for k, (got, w) in enumerate(zip(outs, want)):
        got = got.cpu().numpy()
        bad = ~((got == w) & (np.signbit(got) == np.signbit(w)))
        assert not bad.any(), (k, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return want


# ---- the kernel against the statement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(8, 8), (16, 16), (24, 40), (17, 33)])
@pytest.mark.parametrize("deconv", [False, True])
def test_whole_small_files(ci, cuda, size, deconv):
    h, w = size
    for quality, kind in ((1, "noise"), (75, "saturated"), (100, "noise")):
        _kernel_equals_statement(ci, cuda, [K.jpeg(h, w, quality, kind)], deconv=deconv)


@pytest.mark.parametrize("origin", [(0, 0), (16, 32), (16, 16)])
@pytest.mark.parametrize("flip", [False, True])
def test_windows_of_a_48_x_64_file(ci, cuda, origin, flip):
    data = K.jpeg(48, 64, 75)
    for deconv in (False, True):
        _kernel_equals_statement(ci, cuda, [data], [origin + (32, 32)], [flip], deconv=deconv)


def test_whole_300_x_300_file_equals_the_host_reader_too(ci, cuda):
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import emit_dct_inputs
    data = [K.jpeg(300, 300, 90, "smooth"), K.jpeg(300, 300, 50, "noise")]
    want = _kernel_equals_statement(ci, cuda, data)
    assert [w.shape for w in want] == [(2, 38, 38, 64), (2, 19, 19, 128)]
    assert all(np.array_equal(a, b) for a, b in zip(want, emit_dct_inputs(None, jpeg_bytes=data)))


def test_gray_file_and_mixed_batches(ci, cuda):
    gray = K.jpeg(33, 47, 50, layout="gray")
    want = _kernel_equals_statement(ci, cuda, [gray], [(0, 0, 32, 32)], deconv=True)
    assert want[0].any() and not want[1].any() and not want[2].any()
    files = [K.jpeg(48, 64, 75), gray, K.jpeg(32, 32, 100, "saturated"), K.jpeg(64, 48, 10, layout="gray"),
             K.jpeg(40, 56, 90, "smooth")]
    windows = [(16, 32, 32, 32), (0, 0, 32, 32), (0, 0, 32, 32), (32, 16, 32, 32), (0, 16, 32, 32)]
    flips = [True, True, False, False, True]
    for deconv in (False, True):
        _kernel_equals_statement(ci, cuda, files, windows, flips, deconv=deconv)
        _kernel_equals_statement(ci, cuda, files[4:], windows[4:], flips[4:], deconv=deconv)          # a batch of 1


def _hand_made(ci, cuda, flip):
    """Descriptors, tables and planes of `wrap_planes` as one blob, laid out as the plan lays a file out."""
    planes, tables = K.wrap_planes()
    desc = np.zeros(1, dtype=ci.DESC_DTYPE)
    offsets = [0, 512, 640]
    desc["coef_offset"][0], desc["blocks_h"][0], desc["blocks_w"][0] = offsets, [2, 1, 1], [2, 1, 1]
    desc["n_components"], desc["flip"], desc["table_offset"] = 3, int(flip), 0
    coef = np.zeros(768, dtype=np.uint8)
    for off, plane in zip(offsets, planes):
        coef[off:off + plane.nbytes] = plane.reshape(-1).view(np.uint8)
    dev = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(cuda) for a in (coef, desc, tables)]
    return planes, tables, desc, dev


@pytest.mark.parametrize("flip", [False, True])
def test_products_that_leave_int16_wrap(ci, cuda, flip):
    from jpeg_detection_resnet_ssd_amd import kernels
    planes, tables, desc, (coef_d, desc_d, tables_d) = _hand_made(ci, cuda, flip)
    outs = _nan(cuda, [(1, 2, 2, 64), (1, 1, 1, 64), (1, 1, 1, 64)])
    kernels.jpeg_dct_inputs(coef_d, desc_d, desc, tables_d, tables, outs)
    for c, out in enumerate(outs):
        want = K.wrapped(planes[c], tables[c])
        want = (K.mirror_restated(want) if flip else want).astype(np.float32)
        assert np.array_equal(out.cpu().numpy()[0], want), c
        assert np.array_equal(want, ci.window_blocks(planes[c], tables[c], 0, 0, want.shape[0], want.shape[1], flip))


def test_output_layouts(ci, cuda):
    """CbCr as the halves of one 128-channel tensor and as two tensors; a Y output that is not 16-byte aligned and chroma
    with a stride that is no multiple of 4, which take the element-by-element stores; nothing outside the views is written."""
    from jpeg_detection_resnet_ssd_amd import kernels
    pending = ci.DeviceCoefficientInputs(deconv=True)([K.jpeg(48, 64, 75), K.jpeg(48, 64, 10, "smooth")],
                                                      [(16, 32, 32, 32), (0, 16, 32, 32)], [True, False])
    host, blob = _staged(pending, cuda)
    desc_h, tables_h, _ = pending.plan.views(host)
    desc_d, tables_d, coef_d = pending.plan.views(blob)
    want = pending.numpy()
    # halves of (2, 2, 2, 128), through the plan
    halves = _nan(cuda, [(2, 4, 4, 64), (2, 2, 2, 128)])
    pending.plan.launch(host, blob, halves)
    assert np.array_equal(halves[1].cpu().numpy(), np.concatenate(want[1:], axis=-1))
    # Y one float past a 16-byte boundary; Cb and Cr blocks 67 floats apart
    whole_y = torch.full((1 + 2 * 4 * 4 * 64 + 7,), float("nan"), device=cuda)
    y = whole_y[1:1 + 2 * 4 * 4 * 64].view(2, 4, 4, 64)
    assert y.data_ptr() % 16 == 4
    whole_c = [torch.full((2, 2, 2, 67), float("nan"), device=cuda) for _ in range(2)]
    kernels.jpeg_dct_inputs(coef_d, desc_d, desc_h, tables_d, tables_h, (y, whole_c[0][..., :64], whole_c[1][..., :64]))
    assert np.array_equal(y.cpu().numpy(), want[0]) and np.array_equal(halves[0].cpu().numpy(), want[0])
    edge = whole_y.cpu().numpy()
    assert np.isnan(edge[:1]).all() and np.isnan(edge[-7:]).all()
    for c in (0, 1):
        got = whole_c[c].cpu().numpy()
        assert np.array_equal(got[..., :64], want[1 + c]) and np.isnan(got[..., 64:]).all()


# ---- entry-point checks --------------------------------------------------------------------------------------------------------
def test_bad_descriptors_launch_nothing(ci, cuda):
    from jpeg_detection_resnet_ssd_amd import kernels
    from jpeg_detection_resnet_ssd_amd._lib import DjError
    pending = ci.DeviceCoefficientInputs(deconv=True)([K.jpeg(48, 64, 75), K.jpeg(48, 64, 50)], [(16, 32, 32, 32)] * 2)
    host, blob = _staged(pending, cuda)
    desc_h, tables_h, _ = pending.plan.views(host)
    desc_d, tables_d, coef_d = pending.plan.views(blob)
    outs = _nan(cuda, pending.shapes)

    def refused(word, **fields):
        desc = desc_h.copy()
        for name, value in fields.items():
            desc[name][1] = value
        with pytest.raises(DjError, match=word):
            kernels.jpeg_dct_inputs(coef_d, desc_d, desc, tables_d, tables_h, outs)
    refused("leave the buffer", coef_offset=[0, 6144, pending.plan.coef_bytes - 64])      # a bad offset
    refused("multiple of 16", coef_offset=[8, 6144, 7680])
    refused("leaves the grid", by0=[3, 1, 1])                                             # a window outside the grid
    refused("leaves the grid", bx0=[4, 2, 3])
    refused("tables at", table_offset=2 * 192)                                            # a table offset past the tables
    refused("components", n_components=0)
    refused("flip", flip=-1)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs)
    kernels.jpeg_dct_inputs(coef_d, desc_d, desc_h, tables_d, tables_h, outs)             # the good descriptors do run
    assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(outs, pending.numpy()))


# ---- upload and models -----------------------------------------------------------------------------------------------------------
def test_emit_into_equals_numpy_over_both_staging_slots(ci, cuda):
    """Three batches through one emitter, nothing synchronising in between: both pinned slots are used, the blob grows,
    and the second batch holds a gray file whose chroma must not keep the first batch's values."""
    emit = ci.DeviceCoefficientInputs(n_threads=2)
    colour = [K.jpeg(48, 64, 75, seed=s) for s in range(3)]
    first = emit(colour[:2], [(0, 0, 32, 32), (16, 32, 32, 32)], [False, True])
    second = emit([colour[2], K.jpeg(64, 48, 50, layout="gray"), colour[0]],
                  [(16, 16, 32, 32), (32, 16, 32, 32), (0, 32, 32, 32)], [True, True, False])
    assert second.plan.nbytes > first.plan.nbytes
    buffers = _nan(cuda, second.shapes)                      # one set of resident buffers, reused as a model's are
    results = []
    for pending in (first, second, first):
        n = len(pending)
        pending.emit_into([b[:n] for b in buffers])
        results.append([b[:n].clone() for b in buffers])
    torch.cuda.synchronize()
    st = emit._state[str(cuda)]
    assert all(slot[0] is not None for slot in st["slots"]) and st["blob"].numel() >= second.plan.nbytes
    for pending, got in zip((first, second, first), results):
        for g, w in zip(got, pending.numpy()):
            assert np.array_equal(g.cpu().numpy(), w)
    assert not results[1][1][1].any() and results[0][1][1].any()       # the gray file's chroma, where colour was before
    with pytest.raises(ValueError, match="emit_into"):
        first.emit_into(_nan(cuda, second.shapes))


def _compiled():
    """The smallest DCT classifier of tests/test_classifier_decode_gpu.py, at a 32 x 32 window."""
    from jpeg_detection_resnet_ssd_amd.keras import backend as B
    from jpeg_detection_resnet_ssd_amd.keras import layers as L
    from jpeg_detection_resnet_ssd_amd.keras.models import Model
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import SGD
    B.clear_session()
    B.set_random_seed(5)
    iy, icc = L.Input(shape=(4, 4, 64)), L.Input(shape=(2, 2, 128))
    features = L.Concatenate(axis=-1)([iy, L.UpSampling2D()(icc)])
    h = L.Conv2D(8, (3, 3), padding="same", activation="relu", name="conv")(features)
    y = L.Dense(3, activation="softmax", name="probs")(L.GlobalAveragePooling2D(name="pool")(h))
    model = Model([iy, icc], y)
    model.compile(optimizer=SGD(lr=1e-4, momentum=0.9), loss="categorical_crossentropy")
    return model


def test_model_fed_the_pending_batch_equals_model_fed_the_statement(ci, cuda):
    model = _compiled()
    pending = ci.DeviceCoefficientInputs(n_threads=2)([K.jpeg(48, 64, 75), K.jpeg(33, 47, 50, layout="gray"), K.jpeg(32, 32, 90)],
                                                      [(16, 32, 32, 32), (0, 0, 32, 32), (0, 0, 32, 32)], [True, False, True])
    got = model.predict(pending, batch_size=3)
    torch.cuda.synchronize()
    inputs = [b.detach().cpu().numpy().copy() for b in model._plan(3, False, False).inputs]
    want = model.predict(pending.numpy(), batch_size=3)
    assert got.shape == (3, 3) and np.isfinite(got).all() and np.array_equal(got, want)
    assert all(np.array_equal(a, b) for a, b in zip(inputs, pending.numpy()))
    # sliced along the batch: chunks of 2 and 1
    assert np.array_equal(model.predict(pending, batch_size=2), model.predict(pending.numpy(), batch_size=2))


def test_fit_and_evaluate_from_the_generator(cuda, tree):
    from jpeg_detection_resnet_ssd_amd.keras.callbacks import Callback
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import DCTGeneratorCoefficients
    model = _compiled()
    generator = DCTGeneratorCoefficients(tree[0], tree[1], batch_size=3, shuffle=False, target_length=32, device=True,
                                         decode_threads=2)

    class Steps(Callback):
        def on_train_begin(self, logs=None):
            self.seen = []

        def on_batch_end(self, batch, logs=None):
            self.seen.append(logs["loss"])

    seen = Steps()
    random.seed(3)
    history = model.fit_generator(generator, steps_per_epoch=2, epochs=1, verbose=0, callbacks=[seen])
    assert len(seen.seen) == 2 and all(math.isfinite(v) for v in seen.seen) and math.isfinite(history.history["loss"][0])
    assert math.isfinite(model.evaluate_generator(generator))
