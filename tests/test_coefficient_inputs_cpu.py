"""CPU: data/coefficient_inputs.py -- the numpy statement of feeding a JPEG file's own coefficients to the networks --
against the existing host reader, its windows and mirror, its refusals, the staging plan, the generators and the switch."""
import ctypes
import random

import numpy as np
import pytest

import coefficient_inputs_cases as K
import jpeg_pixels_cases as C


@pytest.fixture(scope="module")
def ci():
    from jpeg_detection_resnet_ssd_amd.data import coefficient_inputs
    return coefficient_inputs


@pytest.fixture(scope="module")
def reader():
    from jpeg_detection_resnet_ssd_amd.jpeg2dct import numpy as reader
    return reader


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return K.write_tree(str(tmp_path_factory.mktemp("coefficient_tree")))


def _equal(got, want):
    return len(got) == len(want) and all(g.dtype == np.float32 and g.shape == w.shape and np.array_equal(g, w)
                                         for g, w in zip(got, want))


# ---- the statement against the existing reader -------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(16, 16), (24, 40), (17, 33), (48, 64), (300, 300)])
def test_whole_file_statement_equals_the_host_reader(ci, size):
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import emit_dct_inputs, input_shapes
    h, w = size
    for quality in (1, 75, 100):
        for kind in (C.CONTENTS if h < 300 else ("noise",)):
            data = [K.jpeg(h, w, quality, kind), K.jpeg(h, w, quality, kind, seed=1)]
            for deconv in (False, True):
                got = ci.coefficient_inputs_host(data, deconv=deconv)
                assert [g.shape for g in got] == [tuple(s) for s in input_shapes(2, h, w, deconv)]
                assert _equal(got, emit_dct_inputs(None, jpeg_bytes=data, deconv=deconv)), (size, quality, kind, deconv)
    if size == (300, 300):
        assert [g.shape[1:] for g in got] == [(38, 38, 64), (19, 19, 64), (19, 19, 64)]


def test_gray_file_gives_its_luma_and_zero_chroma(ci, reader):
    data = K.jpeg(24, 40, 50, layout="gray")
    for deconv in (False, True):
        got = ci.coefficient_inputs_host([data], deconv=deconv)
        assert np.array_equal(got[0][0], reader.loads(data)[0].astype(np.float32))
        assert got[0].shape == (1, 3, 5, 64) and got[1].shape == (1, 2, 3, 64 if deconv else 128)
        assert all(not g.any() for g in got[1:])


def test_the_product_wraps_to_int16(ci):
    planes, tables = K.wrap_planes()
    for plane, table in zip(planes, tables):
        want = K.wrapped(plane, table)
        assert (want.astype(np.int64) != plane.astype(np.int64) * table).any()          # the case does leave int16
        assert np.array_equal(ci.dequantised(plane, table), want)
        rows, cols = plane.shape[:2]
        got = ci.window_blocks(plane, table, 0, 0, rows, cols)
        assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
        flipped = ci.window_blocks(plane, table, 0, 0, rows, cols, flip=True)
        assert np.array_equal(flipped, K.mirror_restated(want).astype(np.float32))
    assert ci.window_blocks(planes[0], tables[0], 0, 0, 1, 1)[0, 0, 0] == 32513.0      # 32767 * 255 = 0x7F7F01
    assert ci.window_blocks(planes[0], tables[0], 0, 0, 1, 1)[0, 0, 2] == 0.0            # -32768 * 2
    assert ci.window_blocks(planes[0], tables[0], 0, 0, 1, 1, flip=True)[0, 0, 5] == -32768.0   # the negation wraps too


# ---- windows and mirror --------------------------------------------------------------------------------------------------------
def test_a_window_equals_slicing_the_whole_file(ci):
    data = K.jpeg(48, 64, 75)
    whole = ci.coefficient_inputs_host([data], deconv=True)
    origins = K.legal_origins(48, 64, 32, 32)
    assert origins == [(0, 0), (0, 16), (0, 32), (16, 0), (16, 16), (16, 32)]
    got = ci.coefficient_inputs_host([data] * len(origins), [(y0, x0, 32, 32) for y0, x0 in origins], deconv=True)
    for i, (y0, x0) in enumerate(origins):
        assert np.array_equal(got[0][i], whole[0][0, y0 // 8:y0 // 8 + 4, x0 // 8:x0 // 8 + 4])
        for c in (1, 2):
            assert np.array_equal(got[c][i], whole[c][0, y0 // 16:y0 // 16 + 2, x0 // 16:x0 // 16 + 2])


def test_windows_that_end_at_a_ragged_edge(ci):
    data = K.jpeg(17, 33, 90, "smooth")
    assert _equal(ci.coefficient_inputs_host([data], [(0, 0, 17, 33)]), ci.coefficient_inputs_host([data]))
    assert [g.shape for g in ci.coefficient_inputs_host([data])] == [(1, 3, 5, 64), (1, 2, 3, 128)]
    data = K.jpeg(24, 40, 90)
    whole = ci.coefficient_inputs_host([data], deconv=True)
    got = ci.coefficient_inputs_host([data], [(16, 32, 8, 8)], deconv=True)
    assert [g.shape for g in got] == [(1, 1, 1, 64)] * 3
    assert np.array_equal(got[0][0], whole[0][0, 2:, 4:]) and np.array_equal(got[1][0], whole[1][0, 1:, 2:])
    assert np.array_equal(got[2][0], whole[2][0, 1:, 2:])


def test_mirror_is_an_involution_and_follows_the_sign_rule(ci):
    data = K.jpeg(48, 64, 75, "saturated")
    for window in ((0, 0, 48, 64), (16, 32, 32, 32), (16, 16, 32, 48)):
        plain = ci.coefficient_inputs_host([data], [window], deconv=True)
        flipped = ci.coefficient_inputs_host([data], [window], [True], deconv=True)
        for p, f in zip(plain, flipped):
            assert np.array_equal(f[0], K.mirror_restated(p[0])) and not np.array_equal(f, p)
            assert np.array_equal(ci.mirrored(ci.mirrored(p[0].astype(np.int16))), p[0].astype(np.int16))
        concat = ci.coefficient_inputs_host([data], [window], [True])
        assert np.array_equal(concat[1], np.concatenate(flipped[1:], axis=-1))


def test_mirrored_coefficients_are_the_mirrored_pixels(ci):
    """In float64, the orthonormal inverse DCT of a mirrored block is the mirrored inverse DCT of the block.  Each pixel is
    a sum of 64 products B[u, v] M[y, u] M[x, v] with |M| <= 1/2, computed on both sides from the same rounded M: the
    rounding of the two constants and the product (4 eps) and of at most 63 additions bound either side's error by
    68 eps sum|B| / 4, so the two sides differ by no more than 34 eps sum|B| of the block."""
    u = np.arange(8)
    m = np.cos((2 * u[:, None] + 1) * u[None, :] * np.pi / 16) * np.where(u == 0, np.sqrt(1 / 8), np.sqrt(2 / 8))[None, :]
    data = K.jpeg(48, 64, 75)
    for c, (plain, flipped) in enumerate(zip(ci.coefficient_inputs_host([data], deconv=True),
                                             ci.coefficient_inputs_host([data], flips=[True], deconv=True))):
        def pixels(blocks):
            b = blocks[0].astype(np.float64).reshape(blocks.shape[1], blocks.shape[2], 8, 8)
            px = np.einsum("yu,rcuv,xv->rcyx", m, b, m)
            return px.transpose(0, 2, 1, 3).reshape(8 * blocks.shape[1], 8 * blocks.shape[2])
        tol = 34 * np.finfo(np.float64).eps * np.abs(plain[0].astype(np.float64)).sum(axis=-1).max()
        assert tol < 1e-8
        assert np.abs(pixels(flipped) - pixels(plain)[:, ::-1]).max() <= tol, c


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_files_that_are_not_eligible_are_refused(ci):
    for layout, word in (("444", "4:2:0"), ("422", "4:2:0")):
        with pytest.raises(ValueError, match=word):
            ci.coefficient_inputs_host([K.jpeg(32, 32, layout=layout)])
    with pytest.raises(ValueError, match="SOF2"):
        ci.coefficient_inputs_host([C.golden_jpegs()["progressive"]])
    good = K.jpeg(48, 64, 75)
    with pytest.raises(ValueError, match="could not be read"):
        ci.coefficient_inputs_host([good[:len(good) * 2 // 3]])
    with pytest.raises(ValueError):
        ci.coefficient_inputs_host([])


def test_windows_that_are_not_legal_are_refused(ci):
    data = K.jpeg(48, 64, 75)
    for window, word in (((8, 0, 32, 32), "origin"), ((0, 24, 32, 32), "origin"), ((-16, 0, 32, 32), "origin"),
                         ((32, 0, 32, 32), "leave"), ((0, 48, 32, 32), "leave"), ((0, 0, 64, 64), "leave"),
                         ((0, 0, 24, 32), "neither"), ((0, 0, 32, 40), "neither"), ((0, 0, 0, 32), "positive")):
        with pytest.raises(ValueError, match=word):
            ci.coefficient_inputs_host([data], [window])
    ragged = K.jpeg(24, 40, 75)
    assert ci.check_window(ci.check_file(ragged), (16, 0, 8, 40)) == (16, 0, 8, 40)
    with pytest.raises(ValueError, match="mirror"):
        ci.coefficient_inputs_host([ragged], flips=[True])                       # 40 % 16 != 0
    with pytest.raises(ValueError, match="mixed window shapes"):
        ci.coefficient_inputs_host([data, ragged])
    with pytest.raises(ValueError, match="mixed window shapes"):
        ci.coefficient_inputs_host([data, data], [(0, 0, 32, 32), (0, 0, 32, 48)])
    with pytest.raises(ValueError, match="one window and one flip"):
        ci.coefficient_inputs_host([data, data], [(0, 0, 32, 32)])


# ---- the staging plan --------------------------------------------------------------------------------------------------------
def test_plan_layout_and_fill(ci, reader):
    files = [K.jpeg(48, 64, 75), K.jpeg(33, 47, 50, layout="gray")]
    emit = ci.DeviceCoefficientInputs(n_threads=2)
    pending = emit(files, [(16, 16, 32, 32), (0, 0, 32, 32)], [True, False])
    plan = pending.plan
    assert len(pending) == 2 and pending.shape == (2, 32, 32, 3) and pending.shapes == [(2, 4, 4, 64), (2, 2, 2, 128)]
    assert plan.desc.dtype.itemsize == 88 and plan.desc_offset == 0 and plan.tables_offset == 192
    assert plan.coef_offset == 192 + 2 * 768
    planes = [6 * 8 * 128, 3 * 4 * 128, 3 * 4 * 128, 5 * 6 * 128]
    assert plan.coef_bytes == sum(planes) and plan.nbytes == plan.coef_offset + plan.coef_bytes
    offsets = np.concatenate([plan.desc["coef_offset"][0], plan.desc["coef_offset"][1][:1]])
    assert offsets.tolist() == [0] + np.cumsum(planes)[:-1].tolist() and not (offsets % 64).any()
    assert plan.desc["by0"].tolist() == [[2, 1, 1], [0, 0, 0]] and plan.desc["flip"].tolist() == [1, 0]
    assert plan.desc["n_components"].tolist() == [3, 1] and plan.desc["table_offset"].tolist() == [0, 192]
    staging = np.full(plan.nbytes + 64, 0xA5, dtype=np.uint8)
    plan.fill(staging, pending.images, 2)
    assert (staging[plan.nbytes:] == 0xA5).all()
    desc, tables, coef = plan.views(staging)
    assert np.array_equal(desc, plan.desc) and np.array_equal(tables.reshape(2, 3, 64), plan.tables)
    values = coef.view(np.int16)
    want = list(reader.loads(files[0], normalized=False)) + [reader.loads(files[1], normalized=False)[0]]
    for off, w in zip(offsets, want):
        assert np.array_equal(values[off // 2:off // 2 + w.size].reshape(w.shape), w)
    # slicing along the batch keeps windows and flips; the host statement is numpy()
    assert _equal(pending[1:].numpy(), [a[1:] for a in pending.numpy()])
    assert _equal(pending.numpy(), ci.coefficient_inputs_host(files, pending.windows, pending.flips))
    with pytest.raises(TypeError):
        pending[0]


def test_a_file_that_fails_in_fill_is_named_by_its_index(ci):
    good = K.jpeg(48, 64, 75)
    pending = ci.DeviceCoefficientInputs()([good, good[:len(good) * 2 // 3], good])      # the header is whole
    staging = np.zeros(pending.plan.nbytes, dtype=np.uint8)
    with pytest.raises(ValueError, match=r"items \[1\] of the batch"):
        pending.plan.fill(staging, pending.images, 2)
    with pytest.raises(ValueError):
        pending.numpy()


# ---- generators -----------------------------------------------------------------------------------------------------------------
ORDER = (0, 3, 1, 4, 2, 5)          # of the tree's files in sorted path order


def _generator(tree, cls="DCTGeneratorCoefficients", **kw):
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras import generators
    kw.setdefault("batch_size", 3)
    kw.setdefault("shuffle", False)
    kw.setdefault("target_length", 32)
    return getattr(generators, cls)(tree[0], tree[1], **kw)


@pytest.mark.parametrize("cls", ["DCTGeneratorCoefficients", "DCTGeneratorCoefficientsDeconv"])
def test_generators_draw_in_the_stated_order(ci, tree, cls):
    deconv = cls.endswith("Deconv")
    host, device = _generator(tree, cls, device=False), _generator(tree, cls, device=True, decode_threads=2)
    assert len(host) == 2 and host.number_of_classes == 3
    for index in (0, 1, 2):                                  # batch 2 wraps around to batch 0
        files = [open(tree[2][k], "rb").read() for k in range(3 * (index % 2), 3 * (index % 2) + 3)]
        sizes = [K.TREE_SIZES[k] for k in ORDER[3 * (index % 2):3 * (index % 2) + 3]]
        random.seed(40 + index)
        draws = K.restated_draws(sizes, 32)
        state = random.getstate()
        random.seed(40 + index)
        x_host, y_host = host[index]
        assert random.getstate() == state
        random.seed(40 + index)
        x_device, y_device = device[index]
        assert random.getstate() == state
        assert [tuple(s) for s in x_device.shapes] == [x.shape for x in x_host] == \
            [(3, 4, 4, 64)] + ([(3, 2, 2, 64)] * 2 if deconv else [(3, 2, 2, 128)])
        assert x_device.windows == [d[0] for d in draws] and x_device.flips == [d[1] for d in draws]
        want = ci.coefficient_inputs_host(files, [d[0] for d in draws], [d[1] for d in draws], deconv=deconv)
        assert _equal(x_host, want) and _equal(x_device.numpy(), want)
        labels = np.zeros((3, 3), dtype=np.float32)
        labels[np.arange(3), [k % 3 for k in ORDER[3 * (index % 2):3 * (index % 2) + 3]]] = 1
        assert np.array_equal(y_host, labels) and np.array_equal(y_device, labels) and y_host.dtype == np.float32
    # the draws above did move: some origin is not zero and some image is mirrored over the seeds used
    random.seed(40)
    assert any(d[0][:2] != (0, 0) for d in K.restated_draws([K.TREE_SIZES[k] for k in ORDER], 32))


def test_generator_without_draws_takes_the_centred_window(tree):
    gen = _generator(tree, device=True, random_crop=False, flip=False, batch_size=6)
    state = random.getstate()
    x, _ = gen[0]
    assert random.getstate() == state
    sizes = [K.TREE_SIZES[k] for k in ORDER]
    assert x.windows == [d[0] for d in K.restated_draws(sizes, 32, random_crop=False, flip=False)]
    assert x.windows[0] == (0, 16, 32, 32) and x.windows[1] == (16, 0, 32, 32) and x.flips == [False] * 6


def test_generator_refuses_small_and_ineligible_files_by_path(tree, tmp_path):
    with pytest.raises(ValueError, match="multiple of 16"):
        _generator(tree, target_length=40)
    gen = _generator(tree, target_length=48, device=False)
    with pytest.raises(ValueError, match="img1.jpg"):             # 32 x 32 holds no 48 x 48 window
        gen[0]
    import json
    import os
    directory = tmp_path / "train" / "n_cat"
    os.makedirs(str(directory))
    (directory / "full.jpg").write_bytes(K.jpeg(32, 32, layout="444"))
    (tmp_path / "index.json").write_text(json.dumps(K.CLASSES))
    gen = _generator((str(tmp_path / "train"), str(tmp_path / "index.json")), batch_size=1)
    with pytest.raises(ValueError, match="full.jpg"):
        gen[0]


def test_coefficient_switch():
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import coefficient_switch, device_switches
    assert coefficient_switch({}) is False and coefficient_switch({"DJ_COEFFICIENT_INPUTS": "0", "DJ_DEVICE_PREP": "1"}) is False
    assert coefficient_switch({"DJ_COEFFICIENT_INPUTS": "1"}) is True
    assert coefficient_switch({"DJ_COEFFICIENT_INPUTS": "1", "DJ_DEVICE_PREP": "0", "DJ_DECODE_THREADS": "4"}) is True
    for other in ("DJ_DEVICE_PREP", "DJ_DEVICE_DECODE", "DJ_PHOTOMETRIC"):
        with pytest.raises(ValueError, match=other):
            coefficient_switch({"DJ_COEFFICIENT_INPUTS": "1", other: "1"})
    assert device_switches({"DJ_COEFFICIENT_INPUTS": "1"}) == {"device_prep": False, "device_decode": False,
                                                                "decode_threads": 16}


def test_configurations_honour_the_switch(tree, monkeypatch):
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras import generators
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.vgg_dct_configuration import VGGDCTTrainingConfiguration
    for key in ("DJ_TRAIN_DIR", "DJ_VAL_DIR", "DJ_TEST_DIR"):
        monkeypatch.setenv(key, tree[0])
    monkeypatch.setenv("DJ_INDEX_FILE", tree[1])
    for key in ("DJ_DEVICE_PREP", "DJ_DEVICE_DECODE", "DJ_PHOTOMETRIC"):
        monkeypatch.delenv(key, raising=False)
    config = VGGDCTTrainingConfiguration(lambda classes: None, "test")
    config._batch_size, config.img_size = 2, (32, 32)
    monkeypatch.setenv("DJ_COEFFICIENT_INPUTS", "1")
    config.prepare_training_generators()
    config.prepare_testing_generator()
    train, val, test = config.train_generator, config.validation_generator, config.test_generator
    assert all(type(g) is generators.DCTGeneratorCoefficients and g.device and g.target_length == 32 for g in (train, val, test))
    assert train.random_crop and train.flip and not (val.random_crop or val.flip or test.random_crop or test.flip)
    monkeypatch.setenv("DJ_PHOTOMETRIC", "1")
    with pytest.raises(ValueError, match="DJ_PHOTOMETRIC"):
        config.prepare_training_generators()
    monkeypatch.delenv("DJ_PHOTOMETRIC")
    monkeypatch.delenv("DJ_COEFFICIENT_INPUTS")
    config.prepare_training_generators()
    assert type(config.train_generator) is generators.DCTGeneratorJPEG2DCT


def test_presize_tool_writes_eligible_files(ci, tmp_path):
    import importlib.util
    import os
    from PIL import Image
    spec = importlib.util.spec_from_file_location(
        "presize_dataset", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "presize_dataset.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src, dst = tmp_path / "src", tmp_path / "dst"
    os.makedirs(str(src / "n_cat"))
    os.makedirs(str(src / "n_dog"))
    Image.fromarray(C.content("smooth", 40, 70)).save(str(src / "n_cat" / "wide.png"))
    (src / "n_dog" / "tall.jpeg").write_bytes(K.jpeg(50, 33, layout="444"))
    (src / "n_dog" / "broken.jpg").write_bytes(b"no image")
    assert tool.main([str(src), str(dst), "--side", "32", "--workers", "2"]) == 1          # one file skipped
    assert sorted(os.listdir(str(dst / "n_dog"))) == ["tall.jpg"] and os.listdir(str(dst / "n_cat")) == ["wide.jpg"]
    for path in (dst / "n_cat" / "wide.jpg", dst / "n_dog" / "tall.jpg"):
        image = ci.check_file(path.read_bytes())
        assert image.shape == (32, 32, 3) and image.sampling == (2, 2) and image.info.base.sof == 0
    assert [a.shape for a in ci.coefficient_inputs_host([(dst / "n_cat" / "wide.jpg").read_bytes()])] == [(1, 4, 4, 64), (1, 2, 2, 128)]


# ---- the library ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_point_and_keeps_its_abi_version(ci):
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "dj_jpeg_dct_inputs") and "dj_jpeg_dct_inputs" in _lib.SIGNATURES
    assert lib.dj_abi_version() == _lib.ABI_VERSION == 5
    assert ctypes.sizeof(_lib.JpegDctDesc) == ci.DESC_DTYPE.itemsize == 88
    for name in ci.DESC_DTYPE.names:
        assert getattr(_lib.JpegDctDesc, name).offset == ci.DESC_DTYPE.fields[name][1]


def test_entry_point_refuses_bad_descriptors_on_the_host(ci):
    """Every check runs before the launch, on the host copy of the descriptors: the pointers are never dereferenced."""
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    fake = 0x10000
    pending = ci.DeviceCoefficientInputs()([K.jpeg(48, 64, 75)], [(16, 16, 32, 32)])
    coef_bytes = pending.plan.coef_bytes

    def call(desc, coef=fake, coef_bytes=coef_bytes, table_ints=192, grids=(4, 4, 2, 2), ld=(64, 128, 128),
             floats=(1024, 512 - 64, 512 - 64), outs=(fake, fake, fake + 256)):
        args = []
        for o, l, f in zip(outs, ld, floats):
            args += [o, l, f]
        return lib.dj_jpeg_dct_inputs(coef, coef_bytes, fake, desc.ctypes.data, len(desc), fake, table_ints, *grids, *args,
                                      None)

    def changed(**fields):
        desc = pending.plan.desc.copy()
        for name, value in fields.items():
            desc[name][0] = value
        return desc
    cases = [(changed(coef_offset=[8, 6144, 7680]), {}, "multiple of 16"), (changed(coef_offset=[0, 6144, 7680 + 64]), {}, "leave the buffer"),
             (changed(coef_offset=[-16, 6144, 7680]), {}, "leave the buffer"), (changed(by0=[3, 1, 1]), {}, "leaves the grid"),
             (changed(bx0=[2, 3, 2]), {}, "leaves the grid"), (changed(by0=[-1, 0, 0]), {}, "leaves the grid"),
             (changed(blocks_h=[10, 3, 3]), {}, "leave the buffer"), (changed(table_offset=64), {}, "tables at 64"),
             (changed(table_offset=2), {"table_ints": 400}, "multiple of 4"), (changed(n_components=2), {}, "components"),
             (changed(flip=2), {}, "flip"), (changed(), {"ld": (32, 128, 128)}, "ld_y"),
             (changed(), {"floats": (1023, 448, 448)}, "out_y"), (changed(), {"floats": (1024, 447, 448)}, "out_cb"),
             (changed(), {"grids": (4, 4, 2, 3)}, "out_cb"), (changed(), {"grids": (0, 4, 2, 2)}, "block grids"),
             (changed(), {"coef": fake + 2}, "aligned"), (changed(), {"outs": (fake + 2, fake, fake)}, "4-byte aligned")]
    for desc, kw, word in cases:
        assert call(desc, **kw) < 0, word
        assert word.encode() in lib.dj_last_error(), (word, lib.dj_last_error())
