"""keras.preprocessing.image / keras.applications.vgg16 on the host: the warp against scipy, the draws, the matrices, the
directory iterator, the RGB configuration's switch and the host checks of dj_rgb_warp.  Nothing here needs a GPU."""
import ctypes
import importlib.util
import itertools
import os
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WARP_SHAPES = [(1, 1), (1, 7), (2, 3), (5, 7), (8, 8), (17, 23), (31, 5), (64, 64), (224, 224)]
# (theta, shear, zx, zy, tx, ty)
WARP_PARAMS = [(0.2, -0.2, 0.8, 0.8, 0, 0), (-0.2, 0.2, 1.2, 1.2, 0, 0), (45, 20, 0.5, 2.0, 0, 0), (0, 0, 1, 1, 3.5, -2.25),
               (179.9, 0, 1, 1, 0, 0)]
REFERENCE_ARGS = dict(featurewise_center=True, rotation_range=0.2, shear_range=0.2, zoom_range=0.2, vertical_flip=True,
                      validation_split=0)


def _image(shape, seed, channels=3):
    return np.random.default_rng(seed).integers(0, 256, size=shape + (channels,)).astype(np.float32)


def _reference_draws(n, seed):
    rng = np.random.default_rng(seed)
    return [(rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.8, 1.2), rng.uniform(0.8, 1.2), 0, 0)
            for _ in range(n)]


# ---- the warp -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", WARP_SHAPES, ids=lambda s: "%dx%d" % s)
def test_warp_equals_scipy_bit_for_bit(shape):
    ndimage = pytest.importorskip("scipy").ndimage
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import affine_matrix, affine_warp_host
    x = _image(shape, 7 * shape[0] + shape[1])
    for k, (theta, shear, zx, zy, tx, ty) in enumerate(WARP_PARAMS + _reference_draws(3, shape[0] * 1000 + shape[1])):
        M = affine_matrix(shape, theta, tx, ty, shear, zx, zy)
        got = affine_warp_host(x, M)
        assert got.dtype == np.float32 and got.shape == x.shape
        for ch in range(3):
            want = ndimage.affine_transform(x[:, :, ch], M[:2, :2], M[:2, 2], order=1, mode="nearest", cval=0.)
            assert want.dtype == np.float32
            assert np.array_equal(got[:, :, ch], want), (k, ch, int((got[:, :, ch] != want).sum()))
        assert np.array_equal(affine_warp_host(x.astype(np.uint8), M), got)      # uint8 pixels are the same values


def test_warp_fills_with_the_nearest_edge():
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import affine_warp_host
    x = _image((4, 5), 3)
    far = np.array([[1.0, 0.0, -100.0], [0.0, 1.0, 100.0], [0.0, 0.0, 1.0]])
    got = affine_warp_host(x, far)
    assert np.array_equal(got, np.broadcast_to(x[0, 4], x.shape))
    half = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    got = affine_warp_host(x, half)
    assert np.array_equal(got[:3], ((x[:3].astype(np.float64) * 0.5) * 1.0 + (x[1:].astype(np.float64) * 0.5) * 1.0)
                          .astype(np.float32))
    assert np.array_equal(got[3], x[3])


# ---- the draws ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enabled", list(itertools.product([False, True], repeat=7)),
                         ids=lambda e: "".join("1" if v else "0" for v in e))
def test_draw_order(enabled):
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import ImageDataGenerator
    rot, hs, ws, sh, zoom, hf, vf = enabled
    gen = ImageDataGenerator(rotation_range=30 if rot else 0, height_shift_range=0.25 if hs else 0.,
                             width_shift_range=1.5 if ws else 0., shear_range=12.5 if sh else 0.,
                             zoom_range=(0.5, 1.75) if zoom else 0., horizontal_flip=hf, vertical_flip=vf)
    shape = (11, 29, 3)
    got = gen.get_random_transform(shape, seed=1234)
    after = np.random.random()
    rs = np.random.RandomState(1234)
    want = {"theta": rs.uniform(-30, 30) if rot else 0}
    want["tx"] = rs.uniform(-0.25, 0.25) * 11 if hs else 0          # below 1: a fraction of the height
    want["ty"] = rs.uniform(-1.5, 1.5) if ws else 0                  # 1 and above: pixels
    want["shear"] = rs.uniform(-12.5, 12.5) if sh else 0
    want["zx"], want["zy"] = rs.uniform(0.5, 1.75, 2) if zoom else (1, 1)
    want["flip_horizontal"] = (rs.random_sample() < 0.5) * hf
    want["flip_vertical"] = (rs.random_sample() < 0.5) * vf
    want["channel_shift_intensity"], want["brightness"] = None, None
    assert set(got) == set(want)
    for key, value in want.items():
        assert got[key] == value, key
    assert after == rs.random_sample()           # as many draws consumed, no more


def test_zoom_range_forms():
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import ImageDataGenerator
    assert ImageDataGenerator(zoom_range=0.2).zoom_range == [0.8, 1.2]
    assert ImageDataGenerator(zoom_range=(0.5, 2.0)).zoom_range == [0.5, 2.0]
    with pytest.raises(ValueError, match="zoom_range"):
        ImageDataGenerator(zoom_range=(1, 2, 3))
    np.random.seed(5)
    ImageDataGenerator(zoom_range=[1, 1]).get_random_transform((4, 4, 3))       # [1, 1]: no zoom draw, the two flips only
    after = np.random.random()
    rs = np.random.RandomState(5)
    rs.random_sample(2)
    assert after == rs.random_sample()


# ---- matrices -----------------------------------------------------------------------------------------------------------
def test_pure_zoom_about_the_centre():
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import affine_matrix, apply_affine_transform
    M = affine_matrix((4, 6, 3), zx=2, zy=2)
    assert np.array_equal(M, [[2, 0, -2.5], [0, 2, -3.5], [0, 0, 1]])         # o = dim / 2 + 0.5: x -> 2 x - o
    x = _image((4, 6), 11)
    got = apply_affine_transform(x, zx=2, zy=2)
    # rows 2 i - 2.5 -> clipped 0, 0, 1.5, 3 ; columns 2 j - 3.5 -> 0, 0, 0.5, 2.5, 4.5, 5
    xd = x.astype(np.float64)
    assert np.array_equal(got[0, 0], x[0, 0]) and np.array_equal(got[3, 5], x[3, 5])
    assert np.array_equal(got[3, 2], ((xd[3, 0] * 1.0) * 0.5 + (xd[3, 1] * 1.0) * 0.5).astype(np.float32))
    assert np.array_equal(got[2, 0], ((xd[1, 0] * 0.5) * 1.0 + (xd[2, 0] * 0.5) * 1.0).astype(np.float32))
    assert np.array_equal(got[2, 3], (xd[1, 2] * 0.25 + xd[1, 3] * 0.25 + xd[2, 2] * 0.25 + xd[2, 3] * 0.25).astype(np.float32))


def test_rotation_by_90_degrees_of_a_3x3_image():
    """o = 3 / 2 + 0.5 = 2 on both axes, so the turn is about the last pixel: output (i, j) reads row 4 - j, clipped to 2,
    and column i (cos 90 degrees is 6e-17 in float64; float32 absorbs what it adds)."""
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import apply_affine_transform
    x = np.arange(27, dtype=np.float32).reshape(3, 3, 3)
    got = apply_affine_transform(x, theta=90)
    want = np.empty_like(x)
    for i in range(3):
        for j in range(3):
            want[i, j] = x[min(4 - j, 2), i]
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_trivial_parameters_return_the_input():
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import ImageDataGenerator, affine_matrix
    x = _image((5, 7), 2)
    gen = ImageDataGenerator()
    params = gen.get_random_transform(x.shape, seed=3)
    assert affine_matrix(x.shape) is None
    assert gen.apply_transform(x, params) is x
    flipped = gen.apply_transform(x, dict(params, flip_horizontal=True, flip_vertical=True))
    assert np.array_equal(flipped, x[::-1, ::-1])
    only_cols = gen.apply_transform(x, dict(params, flip_horizontal=True))
    assert np.array_equal(only_cols, x[:, ::-1])
    rec = gen.transform_record(x.shape, params)
    assert rec["identity"] == 1 and rec["flip_cols"] == 0 and rec["flip_rows"] == 0


def test_factors_compose_in_keras_order():
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import affine_matrix, transform_matrix_offset_center
    t, s = np.deg2rad(10.0), np.deg2rad(-7.0)
    rot = np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])
    shift = np.array([[1, 0, 1.5], [0, 1, -2.0], [0, 0, 1]])
    shear = np.array([[1, -np.sin(s), 0], [0, np.cos(s), 0], [0, 0, 1]])
    zoom = np.array([[0.9, 0, 0], [0, 1.1, 0], [0, 0, 1]])
    want = transform_matrix_offset_center(rot.dot(shift).dot(shear).dot(zoom), 9, 12)
    assert np.array_equal(affine_matrix((9, 12, 3), 10.0, 1.5, -2.0, -7.0, 0.9, 1.1), want)
    assert np.array_equal(affine_matrix((9, 12, 3), shear=-7.0), transform_matrix_offset_center(shear, 9, 12))


# ---- preprocess_input ---------------------------------------------------------------------------------------------------
def test_preprocess_input_known_answers():
    from jpeg_detection_resnet_ssd_amd.keras.applications.imagenet_utils import preprocess_input as from_utils
    from jpeg_detection_resnet_ssd_amd.keras.applications.vgg16 import preprocess_input
    assert from_utils is preprocess_input
    x = np.array([[[1, 2, 3], [255, 0, 128]]], dtype=np.float32)
    keep = x.copy()
    got = preprocess_input(x)
    f = np.float32
    want = np.array([[[f(3) - f(103.939), f(2) - f(116.779), f(1) - f(123.68)],
                      [f(128) - f(103.939), f(0) - f(116.779), f(255) - f(123.68)]]], dtype=np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want) and np.array_equal(x, keep)
    # the float32 difference is what is returned: the float64 one is another number
    assert float(got[0, 0, 0]) != 3 - 103.939 and float(got[0, 0, 0]) == float(np.float32(np.float32(3) - np.float32(103.939)))
    assert np.array_equal(preprocess_input(x.astype(np.uint8)), want)
    batch = np.stack([x, x + 1])
    assert np.array_equal(preprocess_input(batch)[1], preprocess_input(x + 1))
    with pytest.raises(NotImplementedError, match="mode"):
        preprocess_input(x, mode="tf")


# ---- files --------------------------------------------------------------------------------------------------------------
def _write_tree(root):
    """3 classes, 7 files: several sizes and modes (RGB, L, RGBA as PNG, one JPEG), one file in a nested directory, two
    files the white list leaves out."""
    from PIL import Image
    rng = np.random.default_rng(99)

    def save(rel, mode, size, fmt=None):
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        shape = (size[1], size[0]) + ({"RGB": (3,), "RGBA": (4,), "L": ()}[mode])
        Image.fromarray(rng.integers(0, 256, size=shape).astype(np.uint8), mode).save(path, format=fmt)

    save("cats/b.png", "RGB", (14, 10))            # already the target size
    save("cats/a.png", "L", (20, 13))
    save("cats/deep/c.PNG", "RGBA", (9, 31))
    save("birds/z.jpg", "RGB", (40, 30), "JPEG")
    save("birds/y.bmp", "RGB", (7, 5))
    save("ants/one.png", "RGB", (15, 11))
    save("ants/two.png", "L", (3, 2))
    with open(os.path.join(root, "ants", "notes.txt"), "w") as f:
        f.write("not an image")
    with open(os.path.join(root, "README"), "w") as f:
        f.write("not a class")
    return root


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return _write_tree(str(tmp_path_factory.mktemp("rgb_tree")))


EXPECTED_FILES = ["ants/one.png", "ants/two.png", "birds/y.bmp", "birds/z.jpg", "cats/a.png", "cats/b.png", "cats/deep/c.PNG"]


def test_load_img_converts_and_resizes(tree):
    from PIL import Image
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import img_to_array, load_img
    plain = load_img(os.path.join(tree, "cats", "b.png"))
    assert plain.mode == "RGB" and plain.size == (14, 10)
    arr = img_to_array(plain)
    assert arr.dtype == np.float32 and arr.shape == (10, 14, 3)
    assert np.array_equal(arr, np.asarray(Image.open(os.path.join(tree, "cats", "b.png"))).astype(np.float32))
    for rel, mode in (("cats/a.png", "L"), ("cats/deep/c.PNG", "RGBA"), ("birds/z.jpg", "RGB")):
        with Image.open(os.path.join(tree, rel)) as raw:
            assert raw.mode == mode
            want = raw.convert("RGB").resize((14, 10), Image.NEAREST)
            want_bilinear = raw.convert("RGB").resize((14, 10), Image.BILINEAR)
        got = load_img(os.path.join(tree, rel), target_size=(10, 14))
        assert got.mode == "RGB" and got.size == (14, 10) and np.array_equal(np.asarray(got), np.asarray(want))
        got = load_img(os.path.join(tree, rel), target_size=(10, 14), interpolation="bilinear")
        assert np.array_equal(np.asarray(got), np.asarray(want_bilinear))
    with pytest.raises(NotImplementedError, match="color_mode"):
        load_img(os.path.join(tree, "cats", "b.png"), color_mode="grayscale")
    with pytest.raises(ValueError, match="interpolation"):
        load_img(os.path.join(tree, "cats", "b.png"), target_size=(4, 4), interpolation="cubic")


def test_directory_iterator_lists_classes_and_files(tree, capsys):
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import DirectoryIterator, ImageDataGenerator
    from jpeg_detection_resnet_ssd_amd.keras.utils import Sequence
    it = ImageDataGenerator().flow_from_directory(tree, target_size=(10, 14), batch_size=3, shuffle=False)
    assert "Found 7 images belonging to 3 classes." in capsys.readouterr().out
    assert isinstance(it, DirectoryIterator) and isinstance(it, Sequence)
    assert it.class_indices == {"ants": 0, "birds": 1, "cats": 2} and it.num_classes == 3 and it.samples == 7
    assert [f.replace(os.sep, "/") for f in it.filenames] == EXPECTED_FILES
    assert it.classes.tolist() == [0, 0, 1, 1, 2, 2, 2]
    assert len(it) == 3
    batches = [it[k] for k in range(3)]
    assert [b[0].shape for b in batches] == [(3, 10, 14, 3), (3, 10, 14, 3), (1, 10, 14, 3)]      # the last batch is short
    for k, (x, y) in enumerate(batches):
        assert x.dtype == np.float32 and y.dtype == np.float32
        want = np.zeros((len(x), 3), dtype=np.float32)
        want[np.arange(len(x)), it.classes[3 * k:3 * k + 3]] = 1
        assert np.array_equal(y, want)
    with pytest.raises(ValueError, match="length 3"):
        it[3]
    # as an iterator: the same batches in order, and round again after the short one
    seq = [next(it) for _ in range(4)]
    for got, want in zip(seq, batches + batches[:1]):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert iter(it) is it
    only_x = ImageDataGenerator().flow_from_directory(tree, target_size=(10, 14), batch_size=7, shuffle=False, class_mode=None)
    assert isinstance(only_x[0], np.ndarray) and only_x[0].shape == (7, 10, 14, 3)
    named = ImageDataGenerator().flow_from_directory(tree, target_size=(10, 14), classes=["cats", "ants"])
    assert named.class_indices == {"cats": 0, "ants": 1} and named.samples == 5


def test_getitem_is_the_per_image_composition(tree):
    from jpeg_detection_resnet_ssd_amd.keras.applications.vgg16 import preprocess_input
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import ImageDataGenerator, img_to_array, load_img
    kwargs = dict(rotation_range=25, width_shift_range=0.1, height_shift_range=2.5, shear_range=10, zoom_range=0.3,
                  horizontal_flip=True, vertical_flip=True, rescale=1 / 255., preprocessing_function=preprocess_input)
    it = ImageDataGenerator(**kwargs).flow_from_directory(tree, target_size=(10, 14), batch_size=4, shuffle=True, seed=21)
    x, y = it[1]
    gen = ImageDataGenerator(**kwargs)
    np.random.seed(21)                         # seed + total_batches_seen, and no batch was seen before
    order = np.random.permutation(7)[4:8]      # the epoch's permutation is drawn behind the per-batch seed
    assert len(x) == 3
    for k, j in enumerate(order):
        img = img_to_array(load_img(os.path.join(tree, EXPECTED_FILES[j]), target_size=(10, 14)))
        params = gen.get_random_transform(img.shape)
        want = gen.standardize(gen.apply_transform(img, params))
        assert want.dtype == np.float32 and np.array_equal(x[k], want), k
        assert y[k].argmax() == it.classes[j] and y[k].sum() == 1
    after = np.random.random()
    again = ImageDataGenerator(**kwargs).flow_from_directory(tree, target_size=(10, 14), batch_size=4, shuffle=True, seed=21,
                                                             device_prep=True)
    px, py = again[1]
    assert after == np.random.random()         # the device path leaves np.random where the host path does
    assert px.shape == (3, 10, 14, 3) and px.shapes == [(3, 10, 14, 3)] and np.array_equal(py, y)
    assert np.array_equal(px.numpy()[0], x)    # its host statement is the host path, bit for bit
    assert np.array_equal(px[1:].numpy()[0], x[1:]) and len(px[1:]) == 2


def test_seed_reproduces_and_every_epoch_is_permuted(tree):
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import ImageDataGenerator

    def run(seed):
        gen = ImageDataGenerator(rotation_range=10, zoom_range=0.1, vertical_flip=True)
        it = gen.flow_from_directory(tree, target_size=(10, 14), batch_size=3, seed=seed)
        return [next(it) for _ in range(6)]        # two epochs of three batches

    a, b = run(4), run(4)
    for (xa, ya), (xb, yb) in zip(a, b):
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb)
    assert any(not np.array_equal(xa, xc) for (xa, _), (xc, _) in zip(a, run(5)))
    labels = [np.concatenate([y.argmax(1) for _, y in epoch]) for epoch in (a[:3], a[3:])]
    for lab in labels:                              # each epoch sees every file once ...
        assert sorted(lab.tolist()) == [0, 0, 1, 1, 2, 2, 2]
    assert labels[0].tolist() != labels[1].tolist()          # ... in a permutation of its own (seeds 4 and 7 differ here)
    np.random.seed(4)
    assert labels[0].tolist() == [[0, 0, 1, 1, 2, 2, 2][j] for j in np.random.permutation(7)]


def test_featurewise_center_without_fit_warns_and_does_nothing(tree):
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import ImageDataGenerator
    plain = ImageDataGenerator().flow_from_directory(tree, target_size=(10, 14), batch_size=7, shuffle=False)
    centred = ImageDataGenerator(featurewise_center=True).flow_from_directory(tree, target_size=(10, 14), batch_size=7,
                                                                              shuffle=False)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        x = centred[0][0]
    assert any("featurewise_center" in str(w.message) for w in seen)
    assert np.array_equal(x, plain[0][0])
    with pytest.raises(NotImplementedError, match="fit"):
        ImageDataGenerator(featurewise_center=True).fit(x)


# ---- what is not built says so ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,value", [
    ("samplewise_center", True), ("featurewise_std_normalization", True), ("samplewise_std_normalization", True),
    ("zca_whitening", True), ("zca_epsilon", 1e-3), ("brightness_range", (0.5, 1.5)), ("channel_shift_range", 10.),
    ("fill_mode", "constant"), ("fill_mode", "reflect"), ("fill_mode", "wrap"), ("cval", 1.), ("interpolation_order", 0),
    ("interpolation_order", 3), ("data_format", "channels_first"), ("validation_split", 0.2), ("dtype", "float64"),
    ("width_shift_range", 3), ("height_shift_range", [1, 2]),
])
def test_unsupported_generator_arguments_name_themselves(name, value):
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import ImageDataGenerator
    with pytest.raises(NotImplementedError, match=name):
        ImageDataGenerator(**{name: value})


def test_unsupported_flow_arguments_name_themselves(tree, tmp_path):
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import ImageDataGenerator
    gen = ImageDataGenerator()
    for kw, needle in ((dict(class_mode="binary"), "class_mode"), (dict(class_mode="sparse"), "class_mode"),
                       (dict(class_mode="input"), "class_mode"), (dict(save_to_dir=str(tmp_path)), "save_to_dir"),
                       (dict(color_mode="grayscale"), "color_mode"), (dict(subset="training"), "subset")):
        with pytest.raises(NotImplementedError, match=needle):
            gen.flow_from_directory(tree, **kw)
    for method in ("flow", "flow_from_dataframe"):
        with pytest.raises(NotImplementedError, match=method):
            getattr(gen, method)(None)
    with pytest.raises(NotImplementedError, match="preprocessing_function"):
        ImageDataGenerator(preprocessing_function=lambda x: x).flow_from_directory(tree, device_prep=True)
    ImageDataGenerator(preprocessing_function=lambda x: x).flow_from_directory(tree)          # fine on the host


# ---- the configuration --------------------------------------------------------------------------------------------------
def _rgb_config(name):
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "config", "resnetRGB", "config_file.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    K.clear_session()
    cfg = mod.TrainingConfiguration(load_pretrained_weights=False)
    cfg._batch_size = 2
    return cfg, mod._mod


@pytest.mark.parametrize("device_prep", [False, True])
def test_rgb_config_reads_directories_as_the_reference_does(tree, monkeypatch, device_prep):
    from jpeg_detection_resnet_ssd_amd.keras.applications.vgg16 import preprocess_input
    from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import DirectoryIterator
    monkeypatch.setenv("DJ_TRAIN_DIR", tree)
    monkeypatch.setenv("DJ_VAL_DIR", tree)
    monkeypatch.delenv("DJ_TEST_DIR", raising=False)
    monkeypatch.delenv("DJ_INDEX_FILE", raising=False)
    monkeypatch.setenv("DJ_DEVICE_PREP", "1" if device_prep else "0")
    cfg, _ = _rgb_config("cfg_rgb_directories_%d" % device_prep)
    cfg.prepare_training_generators()
    cfg.prepare_testing_generator()
    train, val, test = cfg.train_generator, cfg.validation_generator, cfg.test_generator
    for it in (train, val, test):
        assert isinstance(it, DirectoryIterator) and it.device_prep is device_prep
        assert it.target_size == (224, 224) and it.batch_size == 2 and it.shuffle and it.seed is None
        assert it.interpolation == "nearest" and it.class_mode == "categorical" and it.samples == 7
        assert it.image_data_generator.preprocessing_function is preprocess_input
    g = train.image_data_generator
    assert (g.featurewise_center, g.rotation_range, g.shear_range, g.zoom_range, g.vertical_flip, g.horizontal_flip,
            g.width_shift_range, g.height_shift_range, g.rescale) == (True, 0.2, 0.2, [0.8, 1.2], True, False, 0., 0., None)
    for it in (val, test):
        g = it.image_data_generator
        assert (g.featurewise_center, g.rotation_range, g.shear_range, g.zoom_range, g.vertical_flip, g.horizontal_flip,
                g.rescale) == (False, 0, 0., [1, 1], False, False, None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x, y = train[0]
    assert tuple(x.shape) == (2, 224, 224, 3) and y.shape == (2, 3)
    assert cfg.train_directory == tree and cfg.validation_directory == tree
    monkeypatch.setenv("DJ_TEST_DIR", os.path.join(tree, "cats"))          # the test directory wins over DJ_VAL_DIR
    cfg.prepare_testing_generator()
    assert cfg.test_generator.directory == os.path.join(tree, "cats")


def test_rgb_config_without_directories_stays_synthetic(monkeypatch):
    for var in ("DJ_TRAIN_DIR", "DJ_VAL_DIR", "DJ_TEST_DIR", "DJ_INDEX_FILE"):
        monkeypatch.delenv(var, raising=False)
    cfg, base = _rgb_config("cfg_rgb_synthetic")
    cfg.prepare_training_generators()
    cfg.prepare_testing_generator()
    for it in (cfg.train_generator, cfg.validation_generator, cfg.test_generator):
        assert isinstance(it, base.SyntheticRGBGenerator)
    monkeypatch.setenv("DJ_TRAIN_DIR", "/nowhere")         # one of the two alone changes nothing
    cfg.prepare_training_generators()
    assert isinstance(cfg.train_generator, base.SyntheticRGBGenerator)


# ---- the C entry point --------------------------------------------------------------------------------------------------
def test_record_layout_is_the_c_struct():
    from jpeg_detection_resnet_ssd_amd import _lib
    from jpeg_detection_resnet_ssd_amd.data.rgb_warp import RECORD_DTYPE, make_record, pack_records
    assert RECORD_DTYPE.itemsize == ctypes.sizeof(_lib.RgbWarpRecord) == 64
    for name in ("m", "identity", "flip_cols", "flip_rows", "reserved"):
        assert RECORD_DTYPE.fields[name][1] == getattr(_lib.RgbWarpRecord, name).offset, name
    recs = pack_records([make_record(None), make_record(np.arange(9.).reshape(3, 3), flip_rows=True)])
    assert recs["identity"].tolist() == [1, 0] and recs["flip_rows"].tolist() == [0, 1]
    assert recs["m"][1].tolist() == [0, 1, 2, 3, 4, 5]
    with pytest.raises(ValueError, match="finite"):
        make_record(np.full((3, 3), np.nan))


def test_library_exports_the_entry_point_and_keeps_its_abi_version():
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    assert "dj_rgb_warp" in _lib.SIGNATURES and hasattr(lib, "dj_rgb_warp")
    assert lib.dj_abi_version() == _lib.ABI_VERSION == 5


def _records(n=2):
    from jpeg_detection_resnet_ssd_amd.data.rgb_warp import make_record, pack_records
    return pack_records([make_record(np.eye(3)) for _ in range(n)])


def _call(lib, recs, **kw):
    """Device pointers are made up and never dereferenced: every call made through here must fail in the host checks."""
    a = dict(pixels=0x10000, batch=len(recs), height=24, width=40, rec_dev=0x20000, rec_host=recs.ctypes.data, preprocess=1,
             has_rescale=0, rescale=1.0, out=0x30000, stride=120)
    a.update(kw)
    return lib.dj_rgb_warp(a["pixels"], a["batch"], a["height"], a["width"], a["rec_dev"], a["rec_host"], a["preprocess"],
                           a["has_rescale"], a["rescale"], a["out"], a["stride"], None)


@pytest.mark.parametrize("kw,needle", [
    (dict(pixels=None), "pixels is null"), (dict(rec_dev=None), "rec_dev is null"), (dict(rec_host=None), "rec_host is null"),
    (dict(out=None), "out is null"), (dict(batch=0), "batch"), (dict(batch=-2), "batch"), (dict(height=0), "height"),
    (dict(width=-1), "width"), (dict(width=40000, stride=120000), "width"), (dict(stride=119), "out_row_stride"),
    (dict(preprocess=2), "preprocess"), (dict(preprocess=-1), "preprocess"),
    (dict(has_rescale=1, rescale=float("inf")), "rescale"),
])
def test_argument_errors_are_refused_on_the_host(kw, needle):
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    rc = _call(lib, _records(), **kw)
    assert rc < 0
    msg = lib.dj_last_error().decode()
    assert needle in msg, msg


@pytest.mark.parametrize("image,entry,value", [(0, 0, float("nan")), (1, 5, float("inf")), (1, 2, -float("inf"))])
def test_non_finite_matrix_entries_are_refused_on_the_host(image, entry, value):
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    recs = _records()
    recs["m"][image, entry] = value
    assert _call(lib, recs) < 0
    msg = lib.dj_last_error().decode()
    assert "not finite" in msg and "image %d" % image in msg and "entry %d" % entry in msg, msg
