"""CPU: the photometric augmentations (saturation, brightness, contrast, lighting) as the machine-independent statement
of data/photometric.py (`photometric_host`, the twin of csrc/dj_photometric.hip) and as the numpy callables of
vgg_jpeg_keras/generators/helper.py, against tests/golden/photometric.npz (what the reference's own functions returned),
the restated numpy sum against the installed numpy, the generators' device path against their host path, and the argument
checks of the C entry point.  Equality throughout."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "photometric.npz")
SIZES = [(1, 1), (1, 5), (8, 16), (3, 43), (24, 40), (33, 47)]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _cases(golden, *prefixes):
    return [str(n) for n in golden["names"] if str(n).split("/")[0] in prefixes]


def _ops_of(golden, name):
    from jpeg_detection_resnet_ssd_amd.data.photometric import LIGHTING
    return [(int(c), golden[name + "/draws"][i, :3] if c == LIGHTING else golden[name + "/draws"][i, :1])
            for i, c in enumerate(golden[name + "/ops"])]


# ---- the twin -----------------------------------------------------------------------------------------------------------
def test_fixture_covers_what_it_says(golden):
    names = [str(n) for n in golden["names"]]
    for fn in ("saturation", "brightness", "contrast"):
        mine = [n for n in names if n.startswith(fn + "/")]
        for h, w in SIZES:
            assert any("/%dx%d_noise" % (h, w) in n for n in mine), (fn, h, w)
        for kind in ("white", "black", "ramp", "patches"):
            assert any(kind in n for n in mine), (fn, kind)
        alphas = np.array([golden[n + "/draws"][0, 0] for n in mine])
        assert alphas.min() < 0.52 and alphas.max() > 1.48          # both ends of [0.5, 1.5]
    assert len(_cases(golden, "chain")) >= 4 and len(_cases(golden, "lighting")) >= 10
    assert golden["probe/pixels"].shape == (4096, 3) and golden["probe/grey"].shape == (4096,)
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_exact_grey_value_equals_the_probe(golden):
    from jpeg_detection_resnet_ssd_amd.data.photometric import grey_exact
    assert np.array_equal(grey_exact(golden["probe/pixels"]), golden["probe/grey"])


@pytest.mark.parametrize("family", ["saturation", "brightness", "contrast", "chain"])
def test_twin_equals_the_fixture(golden, family):
    from jpeg_detection_resnet_ssd_amd.data.photometric import photometric_host
    names = _cases(golden, family)
    assert names
    for name in names:
        got = photometric_host(golden[name + "/src"][None], [_ops_of(golden, name)])[0]
        want = golden[name + "/out"]
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, int((got != want).sum()))


def test_twin_lighting_equals_the_fixture_where_lapack_followed_the_sign_rule(golden):
    """The reference leaves the eigenvectors' signs to LAPACK; the cases whose signs happened to follow the port's rule
    compare byte for byte, the others change when the rule is applied to the recorded shift's decomposition."""
    from jpeg_detection_resnet_ssd_amd.data.photometric import lighting_shift, photometric_host
    names = _cases(golden, "lighting")
    followed = [n for n in names if bool(golden[n + "/signs_follow_rule"])]
    assert len(followed) >= 5
    for name in followed:
        src, normals = golden[name + "/src"], golden[name + "/draws"][0]
        shift = lighting_shift(src, normals)
        scale = max(np.abs(golden[name + "/shift"]).max(), 1e-300)
        assert np.abs(shift - golden[name + "/shift"]).max() <= 1e-9 * scale, name
        got = photometric_host(src[None], [[(4, normals)]])[0]
        assert np.array_equal(got, golden[name + "/out"]), name


def _skip_unless_the_live_dot_is_the_fixtures(golden):
    """The numpy callables go through the installed `dot`; where it rounds the grey value differently from the BLAS that
    made the fixture, their bytes cannot be compared with it."""
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras import generators
    live = generators.grayscale(golden["probe/pixels"].reshape(64, 64, 3)).reshape(-1)
    if np.array_equal(live, golden["probe/grey"]):
        return
    try:
        blas = np.show_config(mode="dicts")["Build Dependencies"]["blas"]
        blas = "%s %s" % (blas.get("name"), blas.get("version"))
    except Exception:
        blas = "unknown"
    pytest.skip("the installed BLAS (%s, numpy %s) evaluates `dot` differently from the fixture's (%s, numpy %s): %d of 4096 "
                "grey values differ" % (blas, np.__version__, golden["blas"], golden["numpy_version"],
                                        int((live != golden["probe/grey"]).sum())))


# ---- the callables ------------------------------------------------------------------------------------------------------
def test_callables_equal_the_fixture(golden):
    from jpeg_detection_resnet_ssd_amd.data.photometric import NAMES
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras import generators
    _skip_unless_the_live_dot_is_the_fixtures(golden)
    checked = 0
    for name in (str(n) for n in golden["names"]):
        if name.startswith("lighting/") and not bool(golden[name + "/signs_follow_rule"]):
            continue
        np.random.seed(int(golden[name + "/seed"]))
        out = golden[name + "/src"]
        for code in golden[name + "/ops"]:
            out = getattr(generators, NAMES[int(code)])(out)
        assert out.dtype == np.uint8 and np.array_equal(out, golden[name + "/out"]), name
        checked += 1
    assert checked >= 100


def test_draw_parameters_makes_the_draws_of_the_callables(golden):
    from jpeg_detection_resnet_ssd_amd.data.photometric import NAMES
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import helper
    for name in _cases(golden, "chain") + _cases(golden, "lighting")[:3]:
        np.random.seed(int(golden[name + "/seed"]))
        for i, code in enumerate(golden[name + "/ops"]):
            got_code, params = helper.draw_parameters(getattr(helper, NAMES[int(code)]))
            assert got_code == int(code) and np.array_equal(np.array(params), golden[name + "/draws"][i, :len(params)])
    assert helper.photometric_code(lambda x: x) is None and helper.photometric_code(helper.grayscale) is None
    with pytest.raises(ValueError):
        helper.draw_parameters(helper.grayscale)


# ---- numpy's sum, restated ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SIZES + [(224, 224), (56, 56), (17, 23), (8, 8), (3, 5), (129, 64), (300, 300)])
def test_restated_sum_equals_numpy(shape):
    from jpeg_detection_resnet_ssd_amd.data.photometric import grey_mean, numpy_sum, pairwise_sum
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    for trial in range(3):
        img = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
        gs = img.dot([0.299, 0.587, 0.114])
        assert numpy_sum(gs) == float(np.sum(gs)) and numpy_sum(gs) == float(gs.reshape(-1).sum()), (shape, trial)
        assert float(np.float64(numpy_sum(gs)) / gs.size) == float(gs.mean())
        if gs.size <= 8192:
            assert pairwise_sum(gs) == float(np.sum(gs))
    small = rng.integers(0, 256, (min(shape[0], 40), min(shape[1], 40), 3), dtype=np.uint8)
    from jpeg_detection_resnet_ssd_amd.data.photometric import grey_exact
    if np.array_equal(grey_exact(small), small.dot([0.299, 0.587, 0.114])):      # the live `dot` is the fused form here
        assert grey_mean(small) == float(small.dot([0.299, 0.587, 0.114]).mean())


def test_sum_above_the_reduction_buffer_is_not_one_pairwise_tree():
    """Above 8192 elements numpy adds the sums of 8192-element chunks in order; a single tree gives other bits."""
    from jpeg_detection_resnet_ssd_amd.data.photometric import numpy_sum, pairwise_sum
    rng = np.random.default_rng(12)
    differ = 0
    for _ in range(8):
        a = rng.random(50176) * 255
        assert numpy_sum(a) == float(a.sum())
        differ += pairwise_sum(a) != float(a.sum())
    assert differ > 0


# ---- lists, layout, plan ------------------------------------------------------------------------------------------------
def test_operation_list_layout_is_the_c_struct():
    from jpeg_detection_resnet_ssd_amd import _lib
    from jpeg_detection_resnet_ssd_amd.data.photometric import OPS_DTYPE, pack_ops
    assert OPS_DTYPE.itemsize == ctypes.sizeof(_lib.PhotometricOps) == 120
    for name, _ in _lib.PhotometricOps._fields_:
        assert getattr(_lib.PhotometricOps, name).offset == OPS_DTYPE.fields[name][1], name
    arr = pack_ops([[(1, 0.75), (4, (0.1, -0.2, 0.3))], []])
    assert arr["n_ops"].tolist() == [2, 0] and arr["code"][0].tolist() == [1, 4, 0, 0]
    assert arr["param"][0, 0].tolist() == [0.75, 0.0, 0.0] and arr["param"][0, 1].tolist() == [0.1, -0.2, 0.3]
    for bad in ([[(5, 1.0)]], [[(1, 1.0)] * 5], [[(4, (1.0,))]], [[(1, float("nan"))]], [[(2, (1.0, 2.0))]]):
        with pytest.raises(ValueError):
            pack_ops(bad)


def test_pending_inputs_carry_the_lists_and_slices_keep_them_aligned():
    from jpeg_detection_resnet_ssd_amd.data.image_prep import BatchPlan, DeviceImagePrep, prep_host
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import rgb_to_dct_host
    from jpeg_detection_resnet_ssd_amd.data.photometric import OPS_DTYPE, photometric_host
    rng = np.random.default_rng(21)
    images = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((40, 60), (60, 40), (50, 50), (45, 45))]
    params = [(True, 5, True), (True, 0, False), (False, 0, True), (True, 0, False)]
    ops = [[(1, 0.7), (4, (0.1, -0.2, 0.3))], [], [(3, 1.3), (2, 0.6), (1, 1.45), (4, (0.5, 0.4, -0.3))], [(2, 1.5)]]
    prep = DeviceImagePrep(target_length=32)
    pending = prep(images, params, ops)
    plain = prep(images, params)
    assert plain.ops is None and plain.plan.ops is None and plain.plan.src_offset == plain.plan.ops_offset
    plan = pending.plan
    assert plan.ops.dtype == OPS_DTYPE and plan.ops.shape == (4,) and plan.ops["n_ops"].tolist() == [2, 0, 4, 1]
    assert plan.ops_offset % 64 == 0 and plan.src_offset == plan.ops_offset + 512 and plan.nbytes == plain.plan.nbytes + 512
    blob = np.zeros(plan.nbytes, dtype=np.uint8)
    plan.fill(blob, images)
    assert np.array_equal(blob[plan.ops_offset:plan.ops_offset + 480].view(OPS_DTYPE), plan.ops)
    src, desc, pool = plan.views(blob)
    assert np.array_equal(desc, BatchPlan([im.shape[:2] for im in images], params, 32).desc)
    want = photometric_host(np.stack([prep_host(im, 32, *p) for im, p in zip(images, params)]), ops)
    assert np.array_equal(pending.pixels(), want) and not np.array_equal(want, plain.pixels())
    assert np.array_equal(pending.pixels()[1], plain.pixels()[1])                  # the empty list changes nothing
    arrays = pending.numpy()
    for i in range(4):
        y, cb, cr = rgb_to_dct_host(want[i])
        assert np.array_equal(arrays[0][i], y) and np.array_equal(arrays[1][i], np.concatenate([cb, cr], axis=-1))
    tail = pending[2:]
    assert len(tail) == 2 and [[c for c, _ in lst] for lst in tail.ops] == [[3, 2, 1, 4], [2]]
    assert all(np.array_equal(a[2:], b) for a, b in zip(arrays, tail.numpy()))
    assert prep(images, params)[1:].ops is None
    with pytest.raises(ValueError):
        prep(images, params, ops[:3])
    with pytest.raises(ValueError):
        prep(images, params, [[(9, 1.0)], [], [], []])


# ---- the generators -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def image_directory(tmp_path_factory):
    Image = pytest.importorskip("PIL.Image")
    root = tmp_path_factory.mktemp("imagenet_photometric")
    rng = np.random.default_rng(18)
    sizes = [(60, 80), (80, 60), (64, 64), (50, 90), (90, 50), (72, 72), (45, 70), (70, 45)]
    index = {"0": ["n_cat", "cat"], "1": ["n_dog", "dog"], "2": ["n_eel", "eel"]}
    for i, (h, w) in enumerate(sizes):
        directory = root / "train" / index[str(i % 3)][0]
        directory.mkdir(parents=True, exist_ok=True)
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([127 + (60 + 25 * c) * np.sin(xx / (4.0 + i) + c) * np.cos(yy / (3.0 + c)) for c in range(3)], axis=-1)
        img = np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(str(directory / ("img%d.png" % i)))
    index_file = root / "index.json"
    index_file.write_text(json.dumps(index))
    return str(root / "train"), str(index_file)


def _four():
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import brightness, contrast, lighting, saturation
    return [lighting, contrast, brightness, saturation]


@pytest.mark.parametrize("deconv", [False, True])
def test_device_batch_with_the_four_callables_equals_the_host_batch(image_directory, golden, deconv):
    """Equal seeds of `random` and `np.random`: both paths make the same draws in the same order, and the pending
    batch's host statement (prep_host, photometric_host, rgb_to_dct_host) equals the PIL + callables + JPEG batch.  The
    host callables go through the installed `dot`, `np.cov` and LAPACK, the twin through exact arithmetic: the images and
    seeds are such that the two lightings agree on every pixel (checked when they were chosen)."""
    from jpeg_detection_resnet_ssd_amd.data.image_prep import PendingImageInputs
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras import generators
    _skip_unless_the_live_dot_is_the_fixtures(golden)
    directory, index_file = image_directory
    cls = generators.DCTGeneratorJPEG2DCTDeconv if deconv else generators.DCTGeneratorJPEG2DCT
    kw = dict(batch_size=4, shuffle=False, scale=True, target_length=32, flip=True)
    host = cls(directory, index_file, transformations=_four(), **kw)
    device = cls(directory, index_file, transformations=_four(), device_prep=True, **kw)
    seen = set()
    for index in (0, 1, 2):
        random.seed(300 + index)
        np.random.seed(400 + index)
        got_x, got_y = host[index]
        state, np_state = random.getstate(), np.random.get_state()[1].copy()
        random.seed(300 + index)
        np.random.seed(400 + index)
        pending, dev_y = device[index]
        assert random.getstate() == state and np.array_equal(np.random.get_state()[1], np_state)
        assert host.transformations == device.transformations           # shuffled alike
        assert isinstance(pending, PendingImageInputs) and pending.ops is not None and len(pending.ops) == 4
        seen.update(c for lst in pending.ops for c, _ in lst)
        assert np.array_equal(dev_y, got_y)
        for p, g in zip(pending.numpy(), got_x):
            assert p.dtype == np.float32 and p.shape == g.shape and np.array_equal(p, g), index
    assert seen == {1, 2, 3, 4}


def test_device_prep_refuses_unknown_callables_and_accepts_the_four(image_directory):
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import (DCTGeneratorJPEG2DCT, DCTGeneratorJPEG2DCTDeconv,
                                                                         grayscale, saturation)
    directory, index_file = image_directory
    for cls in (DCTGeneratorJPEG2DCT, DCTGeneratorJPEG2DCTDeconv):
        for bad in ([lambda x: x], [saturation, lambda x: x], [grayscale], [lambda x, f=saturation: f(x)]):
            with pytest.raises(NotImplementedError) as e:
                cls(directory, index_file, batch_size=4, transformations=bad, device_prep=True)
            assert "transformations" in str(e.value) and "device_prep" in str(e.value)
        gen = cls(directory, index_file, batch_size=4, transformations=_four(), device_prep=True, target_length=32)
        assert gen.device_prep and len(gen.transformations) == 4
        plain = cls(directory, index_file, batch_size=4, device_prep=True, target_length=32)
        assert plain[0][0].ops is None


def test_config_switch_gives_the_training_generator_the_four_callables(image_directory, monkeypatch):
    import importlib.util as iu
    directory, index_file = image_directory
    spec = iu.spec_from_file_location("resnet_config_file_photometric",
                                      os.path.join(os.path.dirname(HERE), "config", "resnet", "config_file.py"))
    mod = iu.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def generators(**env):
        for key in ("DJ_TRAIN_DIR", "DJ_VAL_DIR", "DJ_INDEX_FILE", "DJ_DEVICE_PREP", "DJ_PHOTOMETRIC"):
            monkeypatch.delenv(key, raising=False)
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        config = mod.TrainingConfiguration.__new__(mod.TrainingConfiguration)
        config._horovod, config.archi, config.deconv, config._batch_size, config.num_classes = None, "deconv", True, 4, 1000
        config.prepare_training_generators()
        return config.train_generator, config.validation_generator
    every = dict(DJ_TRAIN_DIR=directory, DJ_VAL_DIR=directory, DJ_INDEX_FILE=index_file)
    train, val = generators(**every)
    assert train.transformations is None and val.transformations is None            # the default stays
    for device_prep in ("0", "1"):
        train, val = generators(DJ_PHOTOMETRIC="1", DJ_DEVICE_PREP=device_prep, **every)
        assert train.transformations is not None and sorted(t.__name__ for t in train.transformations) == \
            ["brightness", "contrast", "lighting", "saturation"]
        assert train.device_prep == (device_prep == "1") and val.transformations is None


# ---- the C entry point --------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_point_and_keeps_its_abi_version():
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    assert "dj_photometric" in _lib.SIGNATURES and hasattr(lib, "dj_photometric")
    assert lib.dj_abi_version() == 5 and _lib.ABI_VERSION == 5


def _call(lib, ops, **kw):
    """Device pointers are made up and never dereferenced: every call made through here must fail in the host checks."""
    a = dict(pixels=0x10000, batch=len(ops), height=24, width=40, stride=120, ops_dev=0x20000, ops_host=ops.ctypes.data,
             shift_out=0x30000)
    a.update(kw)
    return lib.dj_photometric(a["pixels"], a["batch"], a["height"], a["width"], a["stride"], a["ops_dev"], a["ops_host"],
                              a["shift_out"], None)


@pytest.mark.parametrize("what, needle", [
    (dict(pixels=None), "pixels is null"), (dict(ops_dev=None), "ops_dev"), (dict(ops_host=None), "ops_host"),
    (dict(batch=0), "batch"), (dict(batch=-2), "batch"), (dict(height=0), "size"), (dict(width=-1), "size"),
    (dict(height=9000), "size"), (dict(height=600, width=600, stride=1800), "pixels per image"),
    (dict(stride=119), "stride_bytes"),
    (("n_ops", 1, 5), "operations"), (("n_ops", 0, -1), "operations"), (("code", 1, 0), "unknown code"),
    (("code", 0, 5), "unknown code"), (("code", 1, -3), "unknown code"), (("param", 0, float("nan")), "not finite"),
    (("param", 1, float("inf")), "not finite"),
])
def test_argument_errors_are_refused_on_the_host(what, needle):
    from jpeg_detection_resnet_ssd_amd import _lib
    from jpeg_detection_resnet_ssd_amd.data.photometric import pack_ops
    lib = _lib.load()
    ops = pack_ops([[(1, 0.8), (4, (0.1, 0.2, 0.3))], [(3, 1.2), (2, 0.9)]])
    kw = {}
    if isinstance(what, tuple):
        field, image, value = what
        if field == "n_ops":
            ops[field][image] = value
        else:
            ops[field][image, 1] = value           # the second operation of that image
    else:
        kw = what
    rc = _call(lib, ops, **kw)
    assert rc < 0
    msg = lib.dj_last_error().decode()
    assert needle in msg, msg
    if isinstance(what, tuple):
        assert "image %d" % what[1] in msg, msg
    with pytest.raises(_lib.DjError):
        _lib.check(rc, "dj_photometric")
