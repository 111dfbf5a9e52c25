"""CPU: resize + crop + flip of decoded images as a statement in numpy (data/image_prep.py, the twin of
csrc/dj_imgprep.hip) against the installed Pillow and against tests/golden/image_prep.npz, the batch plan the kernel reads,
the argument checks of the C entry point, and the classifier generators built on top.  Equality throughout: the arithmetic
is integer only.  The comparisons with the installed Pillow skip where Pillow is missing; the fixture comparisons always
run."""
import ctypes
import importlib.util
import json
import os
import random

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "image_prep.npz")
BILINEAR, BICUBIC = 2, 3

# (source height, source width, output width, output height): up, down by 1.02 .. 12, unchanged dimensions, tiny sources
SIZES = [(375, 500, 299, 224), (500, 375, 224, 299), (333, 500, 336, 224), (300, 300, 224, 224), (224, 224, 224, 224),
         (224, 300, 224, 224), (300, 224, 224, 224), (224, 300, 300, 100), (64, 64, 65, 63), (50, 70, 49, 71),
         (100, 100, 98, 98), (100, 110, 100, 91), (480, 640, 80, 60), (600, 37, 5, 50), (37, 600, 50, 5),
         (512, 512, 43, 43), (97, 131, 9, 7), (1, 1, 8, 8), (1, 1, 1, 5), (2, 3, 10, 7), (3, 2, 7, 11), (1, 40, 13, 4),
         (40, 1, 4, 13), (5, 5, 1, 1), (17, 23, 170, 230), (10, 10, 300, 7), (31, 17, 27, 50), (20, 30, 96, 64),
         (7, 9, 224, 224), (128, 128, 127, 129), (255, 257, 256, 256), (400, 30, 224, 224), (30, 400, 224, 224),
         (199, 301, 150, 99)]


def _content(rng, kind, h, w):
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w]
        planes = [127.5 + 127.5 * np.sin(xx / (3.0 + c) + yy / (5.0 + 2 * c) + c) for c in range(3)]
        return np.stack(planes, axis=-1).astype(np.uint8)
    img = (rng.integers(0, 2, (-(-h // 4), -(-w // 4), 3)) * 255).astype(np.uint8)      # saturated 4x4 patches
    return np.ascontiguousarray(np.kron(img, np.ones((4, 4, 1), dtype=np.uint8))[:h, :w])


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _fixture_script():
    spec = importlib.util.spec_from_file_location("make_image_prep_fixture",
                                                  os.path.join(HERE, "golden", "make_image_prep_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the host twin against Pillow ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("resample", [BICUBIC, BILINEAR])
def test_resize_host_equals_pillow_on_a_table_of_sizes(resample):
    Image = pytest.importorskip("PIL.Image")
    from jpeg_detection_resnet_ssd_amd.data.image_prep import resize_host
    assert len(SIZES) >= 30
    rng = np.random.default_rng(11)
    for i, (h, w, ow, oh) in enumerate(SIZES):
        img = _content(rng, ("noise", "smooth", "saturated")[i % 3], h, w)
        want = np.asarray(Image.fromarray(img).resize((ow, oh), resample))
        got = resize_host(img, (ow, oh), resample)
        assert got.shape == want.shape and got.dtype == np.uint8
        assert np.array_equal(got, want), (h, w, ow, oh, int(np.abs(got.astype(int) - want).max()))


@pytest.mark.parametrize("resample", [BICUBIC, BILINEAR])
def test_resize_host_equals_pillow_under_the_classifier_rule(resample):
    Image = pytest.importorskip("PIL.Image")
    from jpeg_detection_resnet_ssd_amd.data.image_prep import resize_host
    rng = np.random.default_rng(12)
    for i in range(24):
        short = int(rng.integers(20, 520))
        long_ = int(short * rng.uniform(1.0, 3.0))
        h, w = (short, long_) if i % 2 else (long_, short)
        ratio = 224 / min(h, w)
        size = (int(round(w * ratio)), int(round(h * ratio)))
        img = _content(rng, ("noise", "smooth", "saturated")[i % 3], h, w)
        want = np.asarray(Image.fromarray(img).resize(size, resample))
        assert np.array_equal(resize_host(img, size, resample), want), (h, w, size)


def test_box_filter_equals_pillow_too():
    """BOX is the one optional filter restated: no transcendental in its weights."""
    Image = pytest.importorskip("PIL.Image")
    from jpeg_detection_resnet_ssd_amd.data.image_prep import BOX, resize_host
    rng = np.random.default_rng(13)
    for h, w, ow, oh in SIZES[::2]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert np.array_equal(resize_host(img, (ow, oh), BOX), np.asarray(Image.fromarray(img).resize((ow, oh), BOX))), (h, w, ow, oh)


def test_default_filter_is_the_one_pillow_uses_by_default():
    Image = pytest.importorskip("PIL.Image")
    from jpeg_detection_resnet_ssd_amd.data.image_prep import resize_host
    img = np.random.default_rng(14).integers(0, 256, (75, 100, 3), dtype=np.uint8)
    assert np.array_equal(resize_host(img, (60, 45)), np.asarray(Image.fromarray(img).resize((60, 45))))


def test_prep_host_equals_the_pil_statement_of_steps_2_to_4():
    Image = pytest.importorskip("PIL.Image")
    from jpeg_detection_resnet_ssd_amd.data.image_prep import max_offset, prep_host
    rng = np.random.default_rng(15)
    for i, (h, w, t) in enumerate([(375, 500, 224), (500, 375, 224), (300, 300, 224), (100, 260, 64), (260, 100, 64),
                                   (33, 47, 50), (224, 225, 224), (2, 3, 7), (1, 1, 4)]):
        img = _content(rng, ("noise", "smooth", "saturated")[i % 3], h, w)
        for scale in (True, False):
            top = max_offset(h, w, t, scale)
            for offset in sorted({0, top // 2, top}):
                for flip in (False, True):
                    for resample in (BICUBIC, BILINEAR):
                        im = Image.fromarray(img)
                        if scale:
                            ratio = t / min(im.size)
                            width, height = im.size
                            im = im.resize((int(round(width * ratio)), int(round(height * ratio))), resample)
                            assert top == max(im.size) - t
                            if im.size[0] > im.size[1]:
                                im = im.crop((offset, 0, t + offset, t))
                            else:
                                im = im.crop((0, offset, t, t + offset))
                        else:
                            im = im.resize((t, t), resample)
                        if flip:
                            im = im.transpose(Image.FLIP_LEFT_RIGHT)
                        got = prep_host(img, t, scale, offset, flip, resample)
                        assert got.shape == (t, t, 3) and got.dtype == np.uint8 and got.flags.c_contiguous
                        assert np.array_equal(got, np.asarray(im)), (h, w, t, scale, offset, flip, resample)


def test_prep_host_refuses_an_offset_outside_the_range():
    from jpeg_detection_resnet_ssd_amd.data.image_prep import max_offset, prep_host
    img = np.zeros((30, 50, 3), dtype=np.uint8)
    top = max_offset(30, 50, 24)
    assert top == 16
    prep_host(img, 24, True, top, False)
    for bad in (-1, top + 1):
        with pytest.raises(ValueError):
            prep_host(img, 24, True, bad, False)
    with pytest.raises(ValueError):
        prep_host(img, 24, False, 1, False)
    with pytest.raises(ValueError):
        prep_host(img[..., :2], 24, True, 0, False)


# ---- the fixture --------------------------------------------------------------------------------------------------------
def test_prep_host_equals_the_fixture(golden):
    """The same assertion without Pillow: the fixture holds what Pillow made of each case."""
    from jpeg_detection_resnet_ssd_amd.data.image_prep import prep_host
    names = [str(n) for n in golden["names"]]
    assert len(names) >= 12
    for name in names:
        t, scale, offset, flip, resample = (int(v) for v in golden[name + "/params"])
        got = prep_host(golden[name + "/src"], t, bool(scale), offset, bool(flip), resample)
        assert np.array_equal(got, golden[name + "/out"]), name


def test_fixture_covers_what_it_says(golden):
    names = [str(n) for n in golden["names"]]
    params = np.array([golden[n + "/params"] for n in names])
    shapes = [golden[n + "/src"].shape for n in names]
    factors = [min(s[:2]) / p[0] for s, p in zip(shapes, params) if p[1]]
    assert min(factors) < 0.5 and max(factors) > 8 and any(1.05 < f < 1.15 for f in factors)
    assert (1, 1, 3) in shapes and (2, 3, 3) in shapes
    assert set(params[:, 3]) == {0, 1} and set(params[:, 4]) == {BILINEAR, BICUBIC} and set(params[:, 1]) == {0, 1}
    assert (params[:, 2] == 0).any() and (params[:, 2] > 0).any()
    assert all(s[0] <= 200 and s[1] <= 200 and s[0] * s[1] * 3 < 100000 for s in shapes)
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(HERE, "golden", "rgb_dct.npz"))


def test_fixture_regenerates_identically_from_its_script(golden):
    pil = pytest.importorskip("PIL")
    fresh = _fixture_script().make_cases()
    assert sorted(fresh) == sorted(golden)
    same_pillow = str(golden["pillow_version"]) == pil.__version__
    for key in fresh:
        if key.endswith("/out") and not same_pillow:
            continue            # another Pillow than the recorded one: the fixture is the contract, not this one
        assert np.array_equal(fresh[key], golden[key]), key


# ---- the taps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resample", [BICUBIC, BILINEAR])
def test_taps_sum_to_one_and_bounds_stay_inside_the_source(resample):
    from jpeg_detection_resnet_ssd_amd.data.image_prep import resample_coeffs
    pairs = {(h, oh) for h, _, _, oh in SIZES} | {(w, ow) for _, w, ow, _ in SIZES}
    for in_size, out_size in sorted(pairs):
        if in_size == out_size:
            continue
        bounds, taps = resample_coeffs(in_size, out_size, resample)
        assert bounds.shape == (out_size, 2) and taps.shape[0] == out_size
        assert bounds.dtype == np.int32 and taps.dtype == np.int32
        first, count = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
        assert (first >= 0).all() and (count >= 1).all() and (first + count <= in_size).all()
        assert (count <= taps.shape[1]).all()
        assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all()      # what the row window relies on
        live = np.arange(taps.shape[1])[None, :] < count[:, None]
        assert (taps[~live] == 0).all()
        # each tap is within half a unit of its exact value, and the exact values sum to 2^22
        assert (np.abs(taps.astype(np.int64).sum(axis=1) - (1 << 22)) <= count).all(), (in_size, out_size)


def test_unsupported_filters_raise_and_name_the_supported_ones():
    from jpeg_detection_resnet_ssd_amd.data import image_prep as ip
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    for code in (ip.NEAREST, ip.LANCZOS, ip.HAMMING, 17, "lanczos"):
        for call in (lambda: ip.resample_coeffs(8, 4, code), lambda: ip.resize_host(img, (4, 4), code),
                     lambda: ip.prep_host(img, 4, True, 0, False, code), lambda: ip.DeviceImagePrep(resample=code)):
            with pytest.raises(ValueError) as e:
                call()
            assert "BICUBIC" in str(e.value) and "BILINEAR" in str(e.value)
    assert ip.resolve_resample(None) == ip.BICUBIC and ip.resolve_resample("bilinear") == ip.BILINEAR


# ---- what the kernel is given -------------------------------------------------------------------------------------------
def test_descriptor_layout_is_the_c_struct():
    from jpeg_detection_resnet_ssd_amd import _lib
    from jpeg_detection_resnet_ssd_amd.data.image_prep import DESC_DTYPE
    assert DESC_DTYPE.itemsize == ctypes.sizeof(_lib.ImagePrepDesc)
    assert [n for n, _ in _lib.ImagePrepDesc._fields_] == list(DESC_DTYPE.names)
    for name, _ in _lib.ImagePrepDesc._fields_:
        assert getattr(_lib.ImagePrepDesc, name).offset == DESC_DTYPE.fields[name][1], name


def _run_plan_on_the_host(plan, blob):
    """The two passes of csrc/dj_imgprep.hip, read off the staging buffer with the kernel's own index arithmetic."""
    src, desc, pool = plan.views(blob)
    t = plan.target
    outs = []
    for d in desc:
        d = {k: int(d[k]) for k in desc.dtype.names}
        pix = src[d["src_offset"]:d["src_offset"] + d["src_h"] * d["src_stride"]].reshape(d["src_h"], d["src_w"], 3)
        scratch = np.zeros((d["n_rows"], t, 3), dtype=np.uint8)
        for j in range(t):
            c = d["crop_x"] + j
            first, n = pool[d["h_bounds"] + 2 * c], pool[d["h_bounds"] + 2 * c + 1]
            taps = pool[d["h_taps"] + c * d["h_ksize"]:][:n].astype(np.int64)
            rows = pix[d["row0"]:d["row0"] + d["n_rows"], first:first + n].astype(np.int64)
            scratch[:, j] = np.clip(((rows * taps[None, :, None]).sum(1) + (1 << 21)) >> 22, 0, 255)
        out = np.zeros((t, t, 3), dtype=np.uint8)
        for y in range(t):
            r = d["crop_y"] + y
            first, n = pool[d["v_bounds"] + 2 * r] - d["row0"], pool[d["v_bounds"] + 2 * r + 1]
            assert first >= 0 and first + n <= d["n_rows"]
            taps = pool[d["v_taps"] + r * d["v_ksize"]:][:n].astype(np.int64)
            out[y] = np.clip(((scratch[first:first + n].astype(np.int64) * taps[:, None, None]).sum(0) + (1 << 21)) >> 22, 0, 255)
        outs.append(out[:, ::-1] if d["flip"] else out)
    return np.stack(outs)


def test_batch_plan_holds_what_the_two_passes_need():
    from jpeg_detection_resnet_ssd_amd.data.image_prep import BatchPlan, max_offset, prep_host
    rng = np.random.default_rng(16)
    shapes = [(75, 100), (100, 75), (60, 60), (9, 400), (75, 100), (48, 64)]
    images = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]
    params = [(i != 5, max_offset(h, w, 48, i != 5) // (1 + i % 2), i % 2 == 0) for i, (h, w) in enumerate(shapes)]
    plan = BatchPlan(shapes, params, 48, BILINEAR)
    blob = np.full(plan.nbytes, 0xAB, dtype=np.uint8)
    plan.fill(blob, images)
    d = plan.desc
    assert plan.nbytes % 64 == 0 and plan.pool_offset % 64 == 0 and plan.src_offset % 64 == 0
    assert (d["src_offset"] % 64 == 0).all() and (d["scratch_offset"] % 64 == 0).all()
    assert d["h_bounds"][0] == d["h_bounds"][4] and d["v_taps"][0] == d["v_taps"][4]      # equal sizes share their taps
    assert (d["row0"] >= 0).all() and (d["row0"] + d["n_rows"] <= d["src_h"]).all()
    assert d["n_rows"][1] < d["src_h"][1]                  # a portrait image: only the rows under the window
    assert d["h_ksize"][5] > 1 and d["v_ksize"][5] == 1    # 48 x 64 squashed to 48 x 48: the vertical pass is the identity
    want = np.stack([prep_host(im, 48, s, o, f, BILINEAR) for im, (s, o, f) in zip(images, params)])
    assert np.array_equal(_run_plan_on_the_host(plan, blob), want)


# ---- the C entry point --------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points_and_keeps_its_abi_version():
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    for name in ("dj_image_prep", "dj_image_prep_scratch_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.dj_abi_version() == 5


def _good_plan():
    from jpeg_detection_resnet_ssd_amd.data.image_prep import BatchPlan
    plan = BatchPlan([(30, 40), (40, 30)], [(True, 3, False), (True, 0, True)], 24, BICUBIC)
    return plan, plan.desc.copy(), plan.pool.copy()


def _call(lib, plan, desc, pool, **kw):
    """Device pointers are made up and never dereferenced: every call made through here must fail in the host checks."""
    a = dict(src=0x10000, src_bytes=plan.src_bytes, desc_dev=0x20000, desc_host=desc.ctypes.data, batch=len(desc), pool_dev=0x30000,
             pool_host=pool.ctypes.data, pool_ints=pool.size, target=plan.target, out=0x40000, out_stride=3 * plan.target,
             scratch=0x50000, scratch_bytes=plan.scratch_bytes)
    a.update(kw)
    return lib.dj_image_prep(a["src"], a["src_bytes"], a["desc_dev"], a["desc_host"], a["batch"], a["pool_dev"], a["pool_host"],
                             a["pool_ints"], a["target"], a["out"], a["out_stride"], a["scratch"], a["scratch_bytes"], None)


@pytest.mark.parametrize("what, needle", [
    (dict(src=None), "src is null"), (dict(desc_dev=None), "desc_dev"), (dict(desc_host=None), "desc_host"),
    (dict(pool_dev=None), "pool_dev"), (dict(pool_host=None), "pool_host"), (dict(out=None), "out is null"),
    (dict(scratch=None), "scratch is null"), (dict(batch=0), "batch"), (dict(target=0), "target"), (dict(target=-5), "target"),
    (dict(out_stride=71), "out_stride_bytes"), (dict(src_bytes=1000), "leave the source buffer"),
    (dict(scratch_bytes=100), "scratch"), (dict(pool_ints=50), "leave the pool"),
    (("src_h", 0, 0), "source size"), (("src_w", 1, -4), "source size"), (("res_h", 0, 0), "resized size"),
    (("src_stride", 0, 100), "src_stride"), (("src_offset", 0, -1), "leave the source buffer"),
    (("crop_x", 0, 9), "window"), (("crop_y", 1, 9), "window"), (("crop_x", 0, -1), "window"), (("res_w", 0, 20), "window"),
    (("n_rows", 0, 0), "source rows"), (("row0", 1, 30), "source rows"), (("row0", 1, 3), "reads source rows"),
    (("h_ksize", 0, 0), "tap row length"), (("v_ksize", 1, 2), "reads source rows"), (("h_taps", 0, -8), "leave the pool"),
    (("scratch_offset", 1, 0), "overlaps"), (("src_w", 0, 35), "reads source columns"),
])
def test_argument_errors_are_refused_on_the_host(what, needle):
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    plan, desc, pool = _good_plan()
    kw = {}
    if isinstance(what, tuple):
        field, image, value = what
        desc[field][image] = value
        if field == "src_w":
            desc["src_stride"][image] = max(3 * value, 3)
    else:
        kw = what
    rc = _call(lib, plan, desc, pool, **kw)
    assert rc < 0
    msg = lib.dj_last_error().decode()
    assert needle in msg, msg
    with pytest.raises(_lib.DjError):
        _lib.check(rc, "dj_image_prep")


def test_a_bound_that_leaves_the_source_is_refused_on_the_host():
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    plan, desc, pool = _good_plan()
    col = int(desc["h_bounds"][0]) + 2 * (int(desc["crop_x"][0]) + 5)
    pool[col] = int(desc["src_w"][0]) - 1          # first index at the last column, with the full tap count behind it
    assert _call(lib, plan, desc, pool) < 0 and "reads source columns" in lib.dj_last_error().decode()


def test_scratch_size_query():
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    plan, desc, _ = _good_plan()
    assert lib.dj_image_prep_scratch_bytes(desc.ctypes.data, len(desc), plan.target) == plan.scratch_bytes
    assert plan.scratch_bytes == sum(-(-3 * plan.target * int(n) // 64) * 64 for n in desc["n_rows"])
    assert lib.dj_image_prep_scratch_bytes(None, 2, 24) < 0
    desc["n_rows"][1] = 0
    assert lib.dj_image_prep_scratch_bytes(desc.ctypes.data, len(desc), plan.target) < 0


# ---- the pending batch, without a device --------------------------------------------------------------------------------
def test_pending_inputs_follow_the_protocol_of_the_model():
    from jpeg_detection_resnet_ssd_amd.data.image_prep import DeviceImagePrep, PendingImageInputs, prep_host
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import rgb_to_dct_host
    rng = np.random.default_rng(17)
    images = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((40, 60), (60, 40), (50, 50))]
    params = [(True, 5, True), (True, 0, False), (False, 0, True)]
    for deconv in (False, True):
        pending = DeviceImagePrep(target_length=32, deconv=deconv)(images, params)
        assert isinstance(pending, PendingImageInputs) and hasattr(pending, "emit_into")
        assert len(pending) == 3 and pending.shape == (3, 32, 32, 3)
        assert pending.shapes == ([(3, 4, 4, 64), (3, 2, 2, 64), (3, 2, 2, 64)] if deconv else [(3, 4, 4, 64), (3, 2, 2, 128)])
        tail = pending[1:]
        assert len(tail) == 2 and tail.shape[0] == 2 and tail.params == pending.params[1:]
        with pytest.raises(TypeError):
            pending[0]
        arrays = pending.numpy()
        assert [a.shape for a in arrays] == pending.shapes and all(a.dtype == np.float32 for a in arrays)
        for i, (im, (s, o, f)) in enumerate(zip(images, params)):
            y, cb, cr = rgb_to_dct_host(prep_host(im, 32, s, o, f))
            assert np.array_equal(arrays[0][i], y)
            chroma = [cb, cr] if deconv else [np.concatenate([cb, cr], axis=-1)]
            for a, c in zip(arrays[1:], chroma):
                assert np.array_equal(a[i], c)
        assert all(np.array_equal(a[1:], b) for a, b in zip(arrays, tail.numpy()))
    with pytest.raises(ValueError):
        DeviceImagePrep(target_length=32)(images, params[:2])
    with pytest.raises(ValueError):
        DeviceImagePrep(target_length=32)([images[0].astype(np.float32)], params[:1])


# ---- the generators -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def image_directory(tmp_path_factory):
    Image = pytest.importorskip("PIL.Image")
    root = tmp_path_factory.mktemp("imagenet")
    rng = np.random.default_rng(18)
    sizes = [(60, 80), (80, 60), (64, 64), (50, 90), (90, 50), (72, 72), (45, 70), (70, 45)]
    index = {"0": ["n_cat", "cat"], "1": ["n_dog", "dog"], "2": ["n_eel", "eel"]}
    for i, (h, w) in enumerate(sizes):
        directory = root / "train" / index[str(i % 3)][0]
        directory.mkdir(parents=True, exist_ok=True)
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([127 + 120 * np.sin(xx / (4.0 + i) + c) * np.cos(yy / (3.0 + c)) for c in range(3)], axis=-1)
        img = np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8)
        if i % 2:
            Image.fromarray(img).save(str(directory / ("img%d.png" % i)))
        elif i == 4:
            Image.fromarray(img[..., 0]).save(str(directory / ("img%d.jpg" % i)), quality=90)      # a greyscale file
        else:
            Image.fromarray(img).save(str(directory / ("img%d.jpg" % i)), quality=90)
    index_file = root / "index.json"
    index_file.write_text(json.dumps(index))
    return str(root / "train"), str(index_file)


def _pil_loop(paths, association, n_classes, target, scale, flip, deconv):
    """The reference's per-image loop (generators.py:133-192), with the in-tree coefficient reader."""
    import io

    from PIL import Image

    from jpeg_detection_resnet_ssd_amd.jpeg2dct import numpy as j2d
    xs, y = [], np.zeros((len(paths), n_classes))
    for i, path in enumerate(paths):
        with Image.open(path) as im:
            im = im.convert("RGB")
            if scale:
                ratio = target / min(im.size)
                width, height = im.size
                im = im.resize((int(round(width * ratio)), int(round(height * ratio))))
                offset = random.randint(0, max(im.size) - target)
                if im.size[0] > im.size[1]:
                    im = im.crop((offset, 0, target + offset, target))
                else:
                    im = im.crop((0, offset, target, target + offset))
            else:
                im = im.resize((target, target))
            if flip and random.uniform(0, 1) > 0.5:
                im = im.transpose(Image.FLIP_LEFT_RIGHT)
            fake_file = io.BytesIO()
            im.save(fake_file, format="jpeg")
        dct_y, dct_cb, dct_cr = j2d.loads(fake_file.getvalue())
        xs.append([dct_y, dct_cb, dct_cr] if deconv else [dct_y, np.concatenate([dct_cb, dct_cr], axis=-1)])
        y[i, int(association[os.path.basename(os.path.dirname(path))])] = 1
    return [np.stack([x[k] for x in xs]) for k in range(len(xs[0]))], y


@pytest.mark.parametrize("deconv", [False, True])
@pytest.mark.parametrize("scale, flip", [(True, True), (False, True), (True, False)])
def test_generators_equal_a_pil_loop_and_the_device_batch_equals_the_host_batch(image_directory, deconv, scale, flip):
    from jpeg_detection_resnet_ssd_amd.data.image_prep import PendingImageInputs
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import DCTGeneratorJPEG2DCT, DCTGeneratorJPEG2DCTDeconv
    directory, index_file = image_directory
    cls = DCTGeneratorJPEG2DCTDeconv if deconv else DCTGeneratorJPEG2DCT
    kw = dict(batch_size=4, shuffle=False, scale=scale, target_length=32, flip=flip)
    host, device = cls(directory, index_file, **kw), cls(directory, index_file, device_prep=True, **kw)
    assert len(host) == len(device) == 2 and host.number_of_classes == 3 and host.number_of_data_samples == 8
    for index in (0, 1, 3):              # 3 wraps around to batch 1
        paths = [host.images_path[k] for k in host.indexes[(index % 2) * 4:(index % 2) * 4 + 4]]
        random.seed(100 + index)
        want_x, want_y = _pil_loop(paths, host.association, 3, 32, scale, flip, deconv)
        state = random.getstate()
        random.seed(100 + index)
        got_x, got_y = host[index]
        assert random.getstate() == state                       # the same number of draws, in the same order
        random.seed(100 + index)
        pending, dev_y = device[index]
        assert random.getstate() == state
        assert len(got_x) == len(want_x) == (3 if deconv else 2)
        for g, w in zip(got_x, want_x):
            assert g.dtype == np.float32 and g.shape == w.shape and np.array_equal(g, w)
        assert np.array_equal(got_y, want_y) and np.array_equal(dev_y, want_y)
        assert (got_y.sum(axis=1) == 1).all() and got_y.sum(axis=0).max() <= 3
        assert isinstance(pending, PendingImageInputs) and len(pending) == 4
        assert [tuple(s) for s in pending.shapes] == [g.shape for g in got_x]
        for p, g in zip(pending.numpy(), got_x):
            assert p.dtype == np.float32 and np.array_equal(p, g)


def test_shuffle_reorders_at_the_end_of_an_epoch(image_directory):
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import DCTGeneratorJPEG2DCT
    directory, index_file = image_directory
    np.random.seed(3)
    gen = DCTGeneratorJPEG2DCT(directory, index_file, batch_size=4, shuffle=True, target_length=32)
    orders = set()
    for _ in range(6):
        assert sorted(gen.indexes) == list(range(8))
        orders.add(tuple(gen.indexes))
        gen.on_epoch_end()
    assert len(orders) > 1


def test_device_prep_with_transformations_raises(image_directory):
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import DCTGeneratorJPEG2DCT, DCTGeneratorJPEG2DCTDeconv
    directory, index_file = image_directory
    for cls in (DCTGeneratorJPEG2DCT, DCTGeneratorJPEG2DCTDeconv):
        with pytest.raises(NotImplementedError) as e:
            cls(directory, index_file, batch_size=4, transformations=[lambda x: x], device_prep=True)
        assert "transformations" in str(e.value) and "device_prep" in str(e.value)


def test_host_path_applies_the_transformations_in_the_reference_order(image_directory):
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import DCTGeneratorJPEG2DCT
    directory, index_file = image_directory
    calls = []

    def invert(x):
        calls.append("invert")
        return 255 - x

    def darken(x):
        calls.append("darken")
        return x // 2
    kw = dict(batch_size=8, shuffle=False, target_length=32)
    random.seed(5)
    plain_x, _ = DCTGeneratorJPEG2DCT(directory, index_file, **kw)[0]
    random.seed(5)
    x, _ = DCTGeneratorJPEG2DCT(directory, index_file, transformations=[invert, darken], **kw)[0]
    assert calls and set(calls) == {"invert", "darken"} and len(calls) < 16      # each drawn with probability 1/2
    assert x[0].shape == plain_x[0].shape and not np.array_equal(x[0], plain_x[0])


def test_config_uses_the_real_generators_only_when_all_three_switches_are_set(image_directory, monkeypatch):
    import importlib.util as iu
    directory, index_file = image_directory
    spec = iu.spec_from_file_location("resnet_config_file", os.path.join(os.path.dirname(HERE), "config", "resnet", "config_file.py"))
    mod = iu.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import DCTGeneratorJPEG2DCT, DCTGeneratorJPEG2DCTDeconv

    def generators(deconv, **env):
        for key in ("DJ_TRAIN_DIR", "DJ_VAL_DIR", "DJ_INDEX_FILE", "DJ_DEVICE_PREP"):
            monkeypatch.delenv(key, raising=False)
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        config = mod.TrainingConfiguration.__new__(mod.TrainingConfiguration)      # the generators need no network
        config._horovod, config.archi, config.deconv, config._batch_size, config.num_classes = None, "deconv", deconv, 4, 1000
        config.prepare_training_generators()
        return config.train_generator, config.validation_generator
    train, val = generators(False)
    assert isinstance(train, mod.SyntheticDCTClassificationGenerator) and isinstance(val, mod.SyntheticDCTClassificationGenerator)
    train, _ = generators(False, DJ_TRAIN_DIR=directory, DJ_INDEX_FILE=index_file, DJ_DEVICE_PREP="1")
    assert isinstance(train, mod.SyntheticDCTClassificationGenerator)
    every = dict(DJ_TRAIN_DIR=directory, DJ_VAL_DIR=directory, DJ_INDEX_FILE=index_file)
    train, val = generators(False, **every)
    assert type(train) is DCTGeneratorJPEG2DCT and not train.device_prep and train.scale and not val.scale
    train, val = generators(True, DJ_DEVICE_PREP="1", **every)
    assert type(train) is DCTGeneratorJPEG2DCTDeconv and train.device_prep and val.device_prep
