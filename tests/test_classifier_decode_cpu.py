"""CPU: `device_decode` for the two classifier input pipelines -- `BatchPlan` with `CoefficientImage` items, the DCT
generators and the RGB directory iterator handing files over undecoded, their host statements against the `device_prep`
path and the plain host path, and the errors.  No tolerance anywhere: every comparison is equality."""
import importlib.util
import os
import random

import numpy as np
import pytest

import classifier_decode_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = [(True, 0, False), (True, 2, True), (False, 0, True), (True, 0, True), (True, 3, False), (False, 0, False)]


@pytest.fixture(scope="module")
def jp():
    from jpeg_detection_resnet_ssd_amd import _build
    _build.build_jpeg_library()
    from jpeg_detection_resnet_ssd_amd.data import jpeg_pixels
    return jpeg_pixels


@pytest.fixture(scope="module")
def trees(jp, tmp_path_factory):
    """(directory, index file) of the DCT generators' tree and of the RGB iterator's (the same files plus a PNG)."""
    pytest.importorskip("PIL.Image")
    return (K.write_tree(str(tmp_path_factory.mktemp("dct_tree"))),
            K.write_tree(str(tmp_path_factory.mktemp("rgb_tree")), png=True))


# ---- the plan -----------------------------------------------------------------------------------------------------------
def test_batch_plan_layout_and_fill(jp):
    from jpeg_detection_resnet_ssd_amd.data import device_staging as ds, image_prep as ip
    from jpeg_detection_resnet_ssd_amd.jpeg2dct import numpy as reader
    data, mixed, arrays = K.items(jp)
    assert K.coefficient_items(mixed) == K.BASELINE == [0, 1, 2, 3, 4]
    assert ds.check_images(mixed)[0] is mixed[0]
    ops = [[(2, (1.25,))] if i % 2 else [] for i in range(len(mixed))]
    for with_ops in (None, ops):
        plan = ip.BatchPlan(ds.plan_items(mixed), PARAMS, K.TARGET, ops=with_ops)
        plain = ip.BatchPlan([a.shape[:2] for a in arrays], PARAMS, K.TARGET, ops=with_ops)
        assert np.array_equal(plan.desc, plain.desc) and np.array_equal(plan.pool, plain.pool)
        assert plan.shapes == plain.shapes and plan.src_bytes == plain.src_bytes and plan.out_shape == plain.out_shape
        own = ("desc", "pool", "ops", "src")
        assert [getattr(plan, n + "_offset") for n in own] == [getattr(plain, n + "_offset") for n in own]
        behind = [getattr(plan, n + "_offset") for n in ("decode", "tables", "coef")]
        assert all(o % 64 == 0 for o in behind) and behind == sorted(behind) and behind[0] >= plain.nbytes
        assert plan.nbytes == plan.coef_offset + plan.coef_bytes
        assert plan.decode_items == K.BASELINE and plan.decode.dtype == ds.DECODE_DTYPE
        # every item is staged whole, where its pixels would have been copied to
        for j, i in enumerate(plan.decode_items):
            h, w = arrays[i].shape[:2]
            d = plan.decode[j]
            assert (d["ya"], d["yb"], d["xa"], d["xb"], d["height"], d["width"]) == (0, h, 0, w, h, w)
            assert (d["dst_offset"], d["dst_stride"]) == (plan.desc[i]["src_offset"], 3 * w)
        assert plan.scratch_bytes > plain.scratch_bytes
        for d in plan.decode:                                 # the sample planes lie behind the resize's own scratch
            assert (d["sample_offset"][:d["n_components"]] >= plain.scratch_bytes).all()
        assert (plan.decode["sample_offset"] % 64 == 0).all() and (plan.decode["coef_offset"] % 64 == 0).all()
        staging = np.full(plan.nbytes + 64, 0xCD, dtype=np.uint8)
        plan.fill(staging, mixed, n_threads=3)
        assert (staging[plan.nbytes:] == 0xCD).all()
        full = np.full(plain.nbytes, 0xCD, dtype=np.uint8)
        plain.fill(full, arrays)
        assert np.array_equal(staging[:plan.src_offset], full[:plain.src_offset])      # descriptors, pool and lists
        src = plan.views(staging)[0]
        for i, a in enumerate(arrays):
            o = int(plan.desc[i]["src_offset"])
            if i in plan.decode_items:                        # left for the GPU to write
                assert (src[o:o + a.size] == 0xCD).all()
            else:                                             # the fallback's pixels are staged as ever
                assert np.array_equal(src[o:o + a.size], a.reshape(-1))
        decode, tables, coef = plan.decode_views(staging)
        assert np.array_equal(decode, plan.decode)
        for j, i in enumerate(plan.decode_items):
            n = mixed[i].n_components
            planes = reader.loads(data[i], normalized=False, channels=3 if n == 3 else 1)
            for c in range(n):
                assert decode[j]["coef_offset"][c] == plan.plane_offsets[j, c]
                o = int(plan.plane_offsets[j, c])
                assert np.array_equal(coef[o:o + planes[c].size * 2].view(np.int16), planes[c].reshape(-1))
                q = np.array(mixed[i].info.base.quant[c][:])
                assert np.array_equal(tables[int(decode[j]["table_offset"]) + 64 * c:][:64], q)


def test_all_array_batch_plan_is_the_plan_it_was(jp):
    """Without `CoefficientImage`s there is no new part: offsets by the four-part rule restated here, no decode state."""
    from jpeg_detection_resnet_ssd_amd.data import device_staging as ds, image_prep as ip
    _, _, arrays = K.items(jp)
    plan = ip.BatchPlan(ds.plan_items(arrays), PARAMS, K.TARGET)
    up = lambda n: -(-n // 64) * 64
    assert plan.decode is None and not hasattr(plan, "coef_offset")
    assert plan.pool_offset == up(plan.desc.nbytes)
    assert plan.ops_offset == plan.src_offset == up(plan.pool_offset + plan.pool.nbytes)
    assert plan.nbytes == plan.src_offset + plan.src_bytes
    assert plan.src_bytes == sum(up(a.size) for a in arrays)


def test_truncated_file_raises_from_fill_naming_the_item(jp):
    from jpeg_detection_resnet_ssd_amd.data import device_staging as ds, image_prep as ip
    data, mixed, _ = K.items(jp)
    plan = ip.BatchPlan(ds.plan_items(mixed), PARAMS, K.TARGET)
    cut = jp.CoefficientImage(data[4])               # a baseline file that shrank between planning and filling
    cut.data = data[4][:len(data[4]) - 30]
    staging = np.zeros(plan.nbytes, dtype=np.uint8)
    with pytest.raises(ValueError) as e:
        plan.fill(staging, mixed[:4] + [cut] + mixed[5:])
    assert "[4]" in str(e.value)


def test_pending_image_inputs_host_statement(jp):
    from jpeg_detection_resnet_ssd_amd.data import image_prep as ip
    _, mixed, arrays = K.items(jp)
    ops = [[(2, (1.25,)), (3, (0.8,))] if i % 2 else [] for i in range(len(mixed))]
    prep = ip.DeviceImagePrep(K.TARGET, deconv=True, n_threads=2)
    assert prep.n_threads == 2 and ip.DeviceImagePrep(K.TARGET).n_threads is None
    for with_ops in (None, ops):
        want = ip.PendingImageInputs(prep, arrays, PARAMS, with_ops)
        pending = prep(mixed, PARAMS, with_ops)
        assert K.coefficient_items(pending.images) == K.BASELINE and pending.plan.decode_items == K.BASELINE
        assert np.array_equal(pending.pixels(), want.pixels()) and np.array_equal(pending.host_pixels(), want.pixels())
        part = pending[1:4]
        assert K.coefficient_items(part.images) == [0, 1, 2] and np.array_equal(part.pixels(), want.pixels()[1:4])
        for a, b in zip(pending.numpy(), want.numpy()):
            assert np.array_equal(a, b)


# ---- the DCT generators ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deconv", [False, True])
@pytest.mark.parametrize("scale, transformations", [(True, False), (False, False), (True, True)])
def test_dct_generators_hand_over_the_same_batch_undecoded(trees, deconv, scale, transformations):
    from jpeg_detection_resnet_ssd_amd.data.image_prep import PendingImageInputs
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras import generators as G
    directory, index_file = trees[0]
    cls = G.DCTGeneratorJPEG2DCTDeconv if deconv else G.DCTGeneratorJPEG2DCT

    def batch(**kw):
        t = [G.lighting, G.contrast, G.brightness, G.saturation] if transformations else None
        gen = cls(directory, index_file, batch_size=6, shuffle=False, scale=scale, target_length=K.TARGET, transformations=t,
                  device_prep=True, **kw)
        random.seed(11)
        np.random.seed(12)
        pending, y = gen[0]
        return gen, pending, y, random.getstate(), np.random.get_state()
    _, want, want_y, want_random, want_np = batch()
    gen, got, got_y, got_random, got_np = batch(device_decode=True, decode_threads=2)
    assert gen._prep.n_threads == 2
    assert isinstance(got, PendingImageInputs) and len(got) == 6
    # class directories are read in sorted order: n_cat (files 0, 3), n_dog (1, 4), n_eel (2 and the progressive file)
    assert [os.path.basename(p)[:4] for p in gen.images_path] == ["img0", "img3", "img1", "img4", "img2", "img5"]
    assert K.coefficient_items(got.images) == [0, 1, 2, 3, 4] and isinstance(got.images[5], np.ndarray)
    assert got.params == want.params and np.array_equal(got_y, want_y)
    assert (got.ops is None) == (not transformations) and repr(got.ops) == repr(want.ops)
    assert got_random == want_random
    assert all(np.array_equal(a, b) for a, b in zip(got_np, want_np))
    assert np.array_equal(got.pixels(), want.pixels())
    assert np.array_equal(got.plan.desc, want.plan.desc)
    for a, b in zip(got.numpy(), want.numpy()):
        assert a.dtype == np.float32 and np.array_equal(a, b)


# ---- the RGB iterator -----------------------------------------------------------------------------------------------------
def _iterator(tree, interpolation="nearest", batch_size=7, **kw):
    from jpeg_detection_resnet_ssd_amd.keras.applications.vgg16 import preprocess_input
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import ImageDataGenerator
    gen = ImageDataGenerator(rotation_range=20, shear_range=10, zoom_range=0.2, width_shift_range=0.1, vertical_flip=True,
                             horizontal_flip=True, rescale=1 / 64., preprocessing_function=preprocess_input)
    return gen.flow_from_directory(tree, target_size=K.RGB_TARGET, batch_size=batch_size, seed=17, shuffle=False,
                                   interpolation=interpolation, **kw)


@pytest.mark.parametrize("interpolation", ["nearest", "bilinear"])
def test_rgb_iterator_hands_over_the_same_batch_undecoded(trees, interpolation):
    from jpeg_detection_resnet_ssd_amd.data.rgb_warp import PendingRGBFileInputs, PendingRGBInputs
    tree = trees[1][0]

    def batch(**kw):
        x, y = _iterator(tree, interpolation, **kw)[0]
        return x, y, np.random.get_state()
    host, host_y, host_np = batch()
    want, want_y, want_np = batch(device_prep=True)
    got, got_y, got_np = batch(device_prep=True, device_decode=True, decode_threads=2)
    assert isinstance(want, PendingRGBInputs) and isinstance(got, PendingRGBFileInputs)
    assert got.stager.n_threads == 2
    # n_cat holds files 0, 3 and the PNG, n_dog 1 and 4, n_eel 2 and the progressive file
    assert K.coefficient_items(got.images) == [0, 1, 3, 4, 5]
    assert got.images[2].shape == K.RGB_TARGET + (3,) and got.images[6].shape == (23, 17, 3)      # full size: not resized
    assert got.shape == want.shape == (7,) + K.RGB_TARGET + (3,) and got.shapes == want.shapes and len(got) == 7
    assert np.array_equal(got.records, want.records) and got.preprocess == want.preprocess and got.rescale == want.rescale
    assert np.array_equal(got_y, want_y) and np.array_equal(got_y, host_y)
    for state in (want_np, host_np):
        assert all(np.array_equal(a, b) for a, b in zip(got_np, state))
    assert np.array_equal(got.pixels(), want.pixels)
    from PIL import Image
    with Image.open(os.path.join(tree, "n_cat", "img6_same_size.png")) as png:
        assert np.array_equal(got.pixels()[2], np.asarray(png))            # a file of the target's size comes through unchanged
    x = got.numpy()
    assert len(x) == 1 and x[0].dtype == np.float32
    assert np.array_equal(x[0], want.numpy()[0]) and np.array_equal(x[0], host)
    part = got[2:5]
    assert isinstance(part, PendingRGBFileInputs) and part.stager is got.stager and part.shape == (3,) + K.RGB_TARGET + (3,)
    assert K.coefficient_items(part.images) == [1, 2] and np.array_equal(part.numpy()[0], host[2:5])
    assert part.plan.records_offset % 64 == 0 and part.plan.records_offset < part.plan.decode_offset
    with pytest.raises(TypeError):
        got[0]


def test_rgb_plan_carries_the_records_in_the_blob(trees):
    got = _iterator(trees[1][0], "bilinear", device_prep=True, device_decode=True)[0][0]
    plan = got.plan
    offsets = [getattr(plan, n + "_offset") for n in ("desc", "pool", "src", "records", "decode", "tables", "coef")]
    assert offsets == sorted(offsets) and all(o % 64 == 0 for o in offsets)
    staging = np.zeros(plan.nbytes, dtype=np.uint8)
    plan.fill(staging, got.images, 2)
    assert np.array_equal(plan.part(staging, plan.records_offset, got.records, got.records.dtype), got.records)
    # the PNG has the target's size: both passes take the identity taps
    d = plan.desc[2]
    assert (d["src_h"], d["src_w"], d["win_h"], d["win_w"]) == K.RGB_TARGET * 2 and d["h_ksize"] == d["v_ksize"] == 1


# ---- errors -------------------------------------------------------------------------------------------------------------
def test_device_decode_needs_device_prep(trees):
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import DirectoryIterator, ImageDataGenerator
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras import generators as G
    (directory, index_file), (tree, _) = trees
    for cls in (G.DCTGeneratorJPEG2DCT, G.DCTGeneratorJPEG2DCTDeconv):
        with pytest.raises(ValueError, match="device_prep"):
            cls(directory, index_file, batch_size=6, device_decode=True)
    with pytest.raises(ValueError, match="device_prep"):
        ImageDataGenerator().flow_from_directory(tree, target_size=K.RGB_TARGET, device_decode=True)
    with pytest.raises(ValueError, match="device_prep"):
        DirectoryIterator(tree, ImageDataGenerator(), target_size=K.RGB_TARGET, device_decode=True)


def test_unrestated_interpolation_raises_naming_the_argument(trees):
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import ImageDataGenerator
    tree = trees[1][0]
    with pytest.raises(NotImplementedError) as e:
        ImageDataGenerator().flow_from_directory(tree, target_size=K.RGB_TARGET, interpolation="hamming", device_prep=True,
                                                 device_decode=True)
    assert "interpolation" in str(e.value) and "hamming" in str(e.value)
    # without device_decode the filter is Pillow's own, as before
    it = ImageDataGenerator().flow_from_directory(tree, target_size=K.RGB_TARGET, interpolation="hamming", device_prep=True)
    assert it[0][0].shape == (7,) + K.RGB_TARGET + (3,)


def _config(folder):
    spec = importlib.util.spec_from_file_location("cfg_decode_" + folder, os.path.join(ROOT, "config", folder, "config_file.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bare(mod, archi, deconv=False):
    config = mod.TrainingConfiguration.__new__(mod.TrainingConfiguration)      # the generators need no network
    config._horovod, config.archi, config.deconv, config._batch_size, config.num_classes = None, archi, deconv, 4, 1000
    config.img_size = K.RGB_TARGET
    return config


SWITCHES = ("DJ_TRAIN_DIR", "DJ_VAL_DIR", "DJ_TEST_DIR", "DJ_INDEX_FILE", "DJ_DEVICE_PREP", "DJ_DEVICE_DECODE", "DJ_DECODE_THREADS")


def test_config_honours_the_switches(trees, monkeypatch):
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras import generators as G
    (directory, index_file), (tree, _) = trees
    mod = _config("resnet")

    def env(**values):
        for key in SWITCHES:
            monkeypatch.delenv(key, raising=False)
        for key, value in values.items():
            monkeypatch.setenv(key, value)
    every = dict(DJ_TRAIN_DIR=directory, DJ_VAL_DIR=directory, DJ_INDEX_FILE=index_file)
    # the DCT family: training, validation and test generators
    env(DJ_DEVICE_PREP="1", DJ_DEVICE_DECODE="1", **every)
    config = _bare(mod, "deconv", deconv=True)
    config.prepare_training_generators()
    config.prepare_testing_generator()
    for gen in (config.train_generator, config.validation_generator, config.test_generator):
        assert type(gen) is G.DCTGeneratorJPEG2DCTDeconv and gen.device_prep and gen.device_decode
        assert gen._prep.n_threads == 16                        # the default, whatever the CPU count
    env(DJ_DEVICE_PREP="1", DJ_DEVICE_DECODE="1", DJ_DECODE_THREADS="3", **every)
    config = _bare(mod, "deconv")
    config.prepare_training_generators()
    assert config.train_generator._prep.n_threads == 3 and config.validation_generator.device_decode
    env(DJ_DEVICE_PREP="1", **every)
    config = _bare(mod, "deconv")
    config.prepare_training_generators()
    config.prepare_testing_generator()
    for gen in (config.train_generator, config.validation_generator, config.test_generator):
        assert gen.device_prep and not gen.device_decode
    # resnet_rgb
    env(DJ_TRAIN_DIR=tree, DJ_VAL_DIR=tree, DJ_DEVICE_PREP="1", DJ_DEVICE_DECODE="1")
    config = _bare(mod, "resnet_rgb")
    config.prepare_training_generators()
    config.prepare_testing_generator()
    for gen in (config.train_generator, config.validation_generator, config.test_generator):
        assert gen.device_prep and gen.device_decode and gen._stager.n_threads == 16
    # the decode switch alone fails with the SSD trainer's message, for either family and for the test generator
    for archi, values in (("deconv", every), ("resnet_rgb", dict(DJ_TRAIN_DIR=tree, DJ_VAL_DIR=tree))):
        env(DJ_DEVICE_DECODE="1", **values)
        for prepare in ("prepare_training_generators", "prepare_testing_generator"):
            with pytest.raises(ValueError) as e:
                getattr(_bare(mod, archi), prepare)()
            assert str(e.value) == "DJ_DEVICE_DECODE=1 needs DJ_DEVICE_PREP=1"


@pytest.mark.parametrize("folder", ["vggA_dct", "vggD_dct", "resnetRGB"])
def test_the_other_configs_get_the_switches_through_the_resnet_config(folder, trees, monkeypatch):
    (directory, index_file), (tree, _) = trees
    mod = _config(folder)
    for key in SWITCHES:
        monkeypatch.delenv(key, raising=False)
    rgb = folder == "resnetRGB"
    for key, value in (("DJ_TRAIN_DIR", tree if rgb else directory), ("DJ_VAL_DIR", tree if rgb else directory),
                       ("DJ_INDEX_FILE", index_file), ("DJ_DEVICE_PREP", "1"), ("DJ_DEVICE_DECODE", "1")):
        monkeypatch.setenv(key, value)
    config = _bare(mod, "resnet_rgb" if rgb else "vgga_dct")
    config.prepare_training_generators()
    assert config.train_generator.device_decode and config.validation_generator.device_decode
    monkeypatch.delenv("DJ_DEVICE_PREP")
    with pytest.raises(ValueError, match="DJ_DEVICE_DECODE=1 needs DJ_DEVICE_PREP=1"):
        _bare(mod, "resnet_rgb" if rgb else "vgga_dct").prepare_training_generators()
