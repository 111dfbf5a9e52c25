"""CPU: the photometric stage of the SSD augmentation chain as data/ssd_photometric.py states it.  (a) the restated 8-bit
colour conversions against the real-valued definition of HSV, (b) the order of `np.random` draws, (c) pixels whose path
through the statement is special, pinned, (d) the chain: `chain(image, labels)` against `plan(..., return_photometric=True)`
+ `apply` + `patch_resize_host`, (e) the records through `PatchPlan`, `PendingPatchInputs` and the VOC generator's planned
path, (f) the C ABI's record layout."""
import os

import numpy as np
import pytest

F = np.float32
# each channel on 64 levels that include 0 and 255: 2^18 colours
LEVELS = np.round(np.linspace(0, 255, 64)).astype(np.uint8)


def colour_grid():
    r, g, b = np.meshgrid(LEVELS, LEVELS, LEVELS, indexing="ij")
    return np.stack([r, g, b], axis=-1).reshape(-1, 3)


def _noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _exact_hsv(rgb):
    """The real-valued definition in float64: V = max, S = 255 (max - min) / max, H = 30 * (sextant offset) in 0..180."""
    f = rgb.astype(np.float64)
    r, g, b = f[:, 0], f[:, 1], f[:, 2]
    v = f.max(axis=1)
    d = v - f.min(axis=1)
    s = np.where(v > 0, 255.0 * d / np.maximum(v, 1), 0.0)
    dd = np.maximum(d, 1)
    h = np.where(v == r, 30.0 * (g - b) / dd, np.where(v == g, 60.0 + 30.0 * (b - r) / dd, 120.0 + 30.0 * (r - g) / dd))
    h = np.where(d == 0, 0.0, h)
    return np.where(h < 0, h + 180.0, h), s, v


# ---- (a) the colour conversions ---------------------------------------------------------------------------------------------
def test_conversions_stay_within_one_level_of_the_real_valued_definition():
    """One rounding plus one level of table error: |S - exact| <= 1 and circular |H - exact| <= 1, V exact, H in 0..179;
    the uint8 round trip is off by at most 5 levels.  Over all 2^24 colours the maxima are 0.522, 0.640 and 5 (mean 1.046),
    over this grid of 2^18 they are printed."""
    from jpeg_detection_resnet_ssd_amd.data.ssd_photometric import HDIV, SDIV, hsv_to_rgb_host, rgb_to_hsv_host
    assert SDIV[0] == 0 and HDIV[0] == 0 and SDIV[255] == 4096 and SDIV[1] == 255 << 12 and HDIV[1] == 122880
    assert SDIV[7] == 149211 and (255 << 12) // 7 == 149211 and SDIV[11] == 94953 and (255 << 12) // 11 == 94952      # rounded, not truncated
    rgb = colour_grid()
    assert rgb.shape == (1 << 18, 3) and rgb.min() == 0 and rgb.max() == 255
    hsv = rgb_to_hsv_host(rgb)
    h, s, v = _exact_hsv(rgb)
    assert hsv.dtype == np.uint8 and hsv[:, 0].max() <= 179
    assert np.array_equal(hsv[:, 2], v)
    err_s = np.abs(hsv[:, 1] - s).max()
    dh = np.abs(hsv[:, 0] - h)
    err_h = np.minimum(dh, 180.0 - dh).max()
    back = hsv_to_rgb_host(hsv)
    trip = np.abs(back.astype(np.int32) - rgb.astype(np.int32))
    print("max |S - exact| %.3f, max circular |H - exact| %.3f, round trip max %d mean %.3f"
          % (err_s, err_h, trip.max(), trip.max(axis=1).mean()))
    assert err_s <= 1.0 and err_h <= 1.0
    assert back.dtype == np.uint8 and trip.max() <= 5


def test_conversions_equal_opencv_where_it_is_installed():
    cv2 = pytest.importorskip("cv2")
    from jpeg_detection_resnet_ssd_amd.data.ssd_photometric import hsv_to_rgb_host, rgb_to_hsv_host
    rgb = colour_grid().reshape(512, 512, 3)
    hsv = cv2.cvtColor(rgb, cv2.COLOR_RGB2HSV)
    assert np.array_equal(rgb_to_hsv_host(rgb), hsv)
    assert np.array_equal(hsv_to_rgb_host(hsv), cv2.cvtColor(hsv, cv2.COLOR_HSV2RGB))
    odd = np.stack([np.full(256, 180, np.uint8), np.arange(256, dtype=np.uint8), np.arange(255, -1, -1, dtype=np.uint8)], -1)[None]
    assert np.array_equal(hsv_to_rgb_host(odd), cv2.cvtColor(odd, cv2.COLOR_HSV2RGB))


def test_the_restated_classes_keep_the_references_arguments_and_errors():
    from jpeg_detection_resnet_ssd_amd.data import ssd_photometric as sp
    image = _noise(1, 6, 7)
    hsv = sp.ConvertColor()(image)
    assert np.array_equal(hsv, sp.rgb_to_hsv_host(image))
    back, labels = sp.ConvertColor(current='HSV', to='RGB')(hsv, "labels")
    assert labels == "labels" and np.array_equal(back, sp.hsv_to_rgb_host(hsv))
    for kwargs in ({"to": "GRAY"}, {"current": "HSV", "to": "GRAY"}, {"current": "BGR"}):
        with pytest.raises(NotImplementedError):
            sp.ConvertColor(**kwargs)
    with pytest.raises(ValueError):
        sp.ConvertDataType(to='float64')
    halves = np.array([[[0.5, 1.5, 2.5]]], dtype=F)
    assert sp.ConvertDataType()(halves).tolist() == [[[0, 2, 2]]] and sp.ConvertDataType('float32')(image).dtype == F
    c3 = sp.ConvertTo3Channels()
    assert c3(image[:, :, 0]).shape == (6, 7, 3) and c3(image[:, :, :1]).shape == (6, 7, 3) and c3(image) is image
    assert np.array_equal(c3(np.concatenate([image, image[:, :, :1]], axis=-1)), image)
    x = image.astype(F)
    assert np.array_equal(sp.Brightness(delta=40)(x), np.clip(x + F(40), 0, 255))
    assert np.array_equal(sp.Contrast(factor=1.25)(x), np.clip(F(127.5) + F(1.25) * (x - F(127.5)), 0, 255))
    assert np.array_equal(sp.Saturation(factor=3.0)(x.copy())[:, :, 1], np.clip(x[:, :, 1] * F(3), 0, 255))
    assert sp.Hue(delta=-1e-9)(np.zeros((1, 1, 3), dtype=F))[0, 0, 0] == 180.0
    assert np.array_equal(sp.ChannelSwap(order=(2, 0, 1))(image), image[:, :, [2, 0, 1]])
    for make in (lambda: sp.Hue(181), lambda: sp.RandomHue(max_delta=181), lambda: sp.Saturation(0.0), lambda: sp.Contrast(-1.0),
                 lambda: sp.RandomSaturation(2.0, 1.0), lambda: sp.RandomBrightness(3, 3), lambda: sp.RandomContrast(1.5, 0.5)):
        with pytest.raises(ValueError):
            make()
    assert (sp.RandomBrightness().lower, sp.RandomBrightness().upper, sp.RandomSaturation().lower, sp.RandomSaturation().upper,
            sp.RandomContrast().lower, sp.RandomContrast().upper, sp.RandomHue().max_delta, sp.RandomChannelSwap().prob) \
        == (-84.0, 84.0, 0.3, 2.0, 0.5, 1.5, 18, 0.5)
    np.random.seed(2)
    swapped = sp.RandomChannelSwap(prob=1.0)(image)
    np.random.seed(2)
    np.random.uniform(0, 1)
    assert np.array_equal(swapped, image[:, :, list(sp.RandomChannelSwap().permutations[np.random.randint(5)])])


# ---- (b) the draws ----------------------------------------------------------------------------------------------------------
def _replay(seed):
    """The reference's calls, written out: choice(2), then per random operation of the chosen sequence uniform(0, 1) and,
    when p >= 1 - 0.5, the parameter; the channel swap's coin last (prob 0: p >= 1 never holds)."""
    rs = np.random.RandomState(seed)
    out = {}
    if rs.choice(2):
        sequence = 1
        if rs.uniform(0, 1) >= 0.5:
            out["brightness"] = F(rs.uniform(-32.0, 32.0))
        if rs.uniform(0, 1) >= 0.5:
            out["contrast"] = F(rs.uniform(0.5, 1.5))
        if rs.uniform(0, 1) >= 0.5:
            out["saturation"] = F(rs.uniform(0.5, 1.5))
        if rs.uniform(0, 1) >= 0.5:
            out["hue"] = F(rs.uniform(-18, 18))
    else:
        sequence = 2
        if rs.uniform(0, 1) >= 0.5:
            out["brightness"] = F(rs.uniform(-32.0, 32.0))
        if rs.uniform(0, 1) >= 0.5:
            out["saturation"] = F(rs.uniform(0.5, 1.5))
        if rs.uniform(0, 1) >= 0.5:
            out["hue"] = F(rs.uniform(-18, 18))
        if rs.uniform(0, 1) >= 0.5:
            out["contrast"] = F(rs.uniform(0.5, 1.5))
    assert not rs.uniform(0, 1) >= 1.0
    return (sequence, out.get("brightness"), out.get("contrast"), out.get("saturation"), out.get("hue"), (0, 1, 2)), rs.get_state()


def test_draw_makes_the_references_calls_in_the_references_order():
    from jpeg_detection_resnet_ssd_amd.data import ssd_augment as sa
    from jpeg_detection_resnet_ssd_amd.data.ssd_photometric import PhotoParams, SSDPhotometricDistortions
    stage = SSDPhotometricDistortions()
    image, labels = _noise(2, 30, 40), np.array([[3, 5, 6, 30, 25]])
    seen = set()
    for seed in range(40):
        want, state = _replay(seed)
        np.random.seed(seed)
        got = stage.draw()
        assert isinstance(got, PhotoParams) and tuple(got) == want, (seed, got, want)
        assert all(v is None or type(v) is np.float32 for v in got[1:5])
        assert _same_state(np.random.get_state(), state)
        np.random.seed(seed)
        out, same_labels = stage(image, labels)
        assert _same_state(np.random.get_state(), state) and same_labels is labels
        assert out.dtype == np.uint8 and np.array_equal(out, stage.apply(image, got)), seed
        seen.add((got.sequence,) + tuple(v is not None for v in got[1:5]))
        # a full chain: the stage's draws come first, then the geometric ones, on both routes
        np.random.seed(seed)
        sa.SSDDataAugmentation(24, 20, photometric_distortions=stage)(image, labels)
        after_call = np.random.get_state()
        np.random.seed(seed)
        planned = sa.SSDDataAugmentation(24, 20, photometric_distortions=stage).plan(30, 40, labels, return_photometric=True)
        assert _same_state(np.random.get_state(), after_call) and tuple(planned[-1]) == want
    assert {s[0] for s in seen} == {1, 2} and len(seen) > 16


# ---- (c) pixels with a path of their own ------------------------------------------------------------------------------------
# black, grey (s = 0), white, v == r == g, v == g == b, red (H = 0), blue, and one of no kind
SPECIAL = np.array([[[0, 0, 0], [128, 128, 128], [255, 255, 255], [200, 200, 10], [10, 200, 200], [255, 0, 0], [0, 0, 255],
                     [37, 201, 99]]], dtype=np.uint8)


@pytest.mark.parametrize("params, want", [
    ((1, None, None, None, None, (0, 1, 2)),
     [[0, 0, 0], [128, 128, 128], [255, 255, 255], [200, 200, 10], [10, 200, 200], [255, 0, 0], [0, 0, 255], [37, 201, 97]]),
    # H = 0 and a tiny negative delta: the hue byte is 180 for the first three and for red, and reads as 0
    ((1, None, None, None, F(-1e-9), (0, 1, 2)),
     [[0, 0, 0], [128, 128, 128], [255, 255, 255], [200, 200, 10], [10, 200, 200], [255, 0, 0], [0, 0, 255], [37, 201, 97]]),
    ((2, F(-32), F(1.5), F(0.5), F(18), (2, 0, 1)),
     [[0, 0, 0], [80, 80, 80], [255, 255, 255], [62, 112, 188], [188, 62, 112], [103, 255, 203], [255, 203, 103], [185, 67, 190]]),
    ((1, F(32), F(0.5), F(1.5), F(-18), (1, 2, 0)),
     [[80, 80, 80], [144, 144, 144], [191, 191, 191], [94, 37, 180], [180, 94, 37], [25, 124, 191], [124, 191, 25], [180, 57, 86]]),
    ((2, None, F(1.5), None, F(-1e-9), (0, 2, 1)),
     [[0, 0, 0], [128, 128, 128], [255, 255, 255], [236, 0, 236], [0, 236, 236], [255, 0, 0], [0, 255, 0], [0, 82, 238]]),
])
def test_special_pixels_are_pinned(params, want):
    from jpeg_detection_resnet_ssd_amd.data.ssd_photometric import ssd_photometric_host
    got = ssd_photometric_host(SPECIAL, params)
    assert got.dtype == np.uint8 and got.flags.c_contiguous and got.tolist() == [want]


def test_hue_byte_180_is_a_legal_input_and_the_round_trip_is_never_skipped():
    from jpeg_detection_resnet_ssd_amd.data import ssd_photometric as sp
    hsv = sp.rgb_to_hsv_host(SPECIAL).astype(F)
    lifted = np.remainder(hsv[..., 0] + F(-1e-9), F(180.0))
    assert lifted.dtype == F and lifted[0].tolist() == [180.0, 180.0, 180.0, 30.0, 90.0, 180.0, 120.0, 71.0]
    assert sp.hsv_to_rgb_host(np.array([[180, 200, 150], [0, 200, 150], [179, 255, 255], [255, 10, 10]], dtype=np.uint8)).tolist() \
        == [[150, 32, 32], [150, 32, 32], [255, 0, 8], [10, 10, 10]]
    image = colour_grid().reshape(512, 512, 3)
    nothing_drawn = sp.ssd_photometric_host(image, (1, None, None, None, None, (0, 1, 2)))
    assert np.array_equal(nothing_drawn, sp.hsv_to_rgb_host(sp.rgb_to_hsv_host(image))) and (nothing_drawn != image).any()
    assert np.array_equal(sp.ssd_photometric_host(image, (2, None, None, None, None, (0, 1, 2))), nothing_drawn)


def test_params_are_checked_and_packed():
    import ctypes

    from jpeg_detection_resnet_ssd_amd import _lib
    from jpeg_detection_resnet_ssd_amd.data import ssd_photometric as sp
    good = (1, None, F(1.25), None, F(-3), (1, 0, 2))
    for bad in ((0,) + good[1:], (3,) + good[1:], good[:1] + (float("nan"),) + good[2:], good[:4] + (float("inf"),) + good[5:],
                good[:5] + ((0, 0, 1),), good[:5] + ((0, 1, 3),), good[:5] + ((0, 1),)):
        with pytest.raises(ValueError):
            sp.check_params(bad)
        with pytest.raises(ValueError):
            sp.ssd_photometric_host(SPECIAL, bad)
    arr = sp.pack_params([good, (2, F(-32), None, F(0.5), None, (0, 1, 2))])
    assert arr.dtype == sp.PARAMS_DTYPE and arr.dtype.itemsize == ctypes.sizeof(_lib.SsdPhotoParams) == 40
    for name, kind in _lib.SsdPhotoParams._fields_:
        assert sp.PARAMS_DTYPE.fields[name][1] == getattr(_lib.SsdPhotoParams, name).offset, name
    assert arr["sequence"].tolist() == [1, 2] and arr["flags"].tolist() == [sp.CONTRAST | sp.HUE, sp.BRIGHTNESS | sp.SATURATION]
    assert arr["contrast"].tolist() == [1.25, 0.0] and arr["hue"].tolist() == [-3.0, 0.0] and arr["brightness"].tolist() == [0.0, -32.0]
    assert arr["order"].tolist() == [[1, 0, 2], [0, 1, 2]] and arr["reserved"].tolist() == [0, 0]


def test_library_exports_the_entry_point():
    from jpeg_detection_resnet_ssd_amd import _lib, kernels
    lib = _lib.load()
    assert "dj_ssd_photometric" in _lib.SIGNATURES and hasattr(lib, "dj_ssd_photometric") and callable(kernels.ssd_photometric)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dj_hip.h")).read()
    assert "dj_ssd_photo_params" in header and "int dj_ssd_photometric(" in header


# ---- (d) the chain ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain_name", ["SSDDataAugmentation", "SSDDataAugmentationNoCrop"])
def test_chain_call_equals_plan_apply_and_patch_resize(chain_name):
    from jpeg_detection_resnet_ssd_amd.data import ssd_augment as sa
    image = _noise(3, 60, 80)
    labels = np.array([[7, 10, 20, 50, 40], [2, 0, 0, 80, 60]])
    stage = sa.SSDPhotometricDistortions()
    make = getattr(sa, chain_name)
    distorted = 0
    for seed in range(12):
        np.random.seed(seed)
        pixels, boxes = make(30, 40, photometric_distortions=stage)(image, labels)
        state = np.random.get_state()
        np.random.seed(seed)
        chain = make(30, 40, photometric_distortions=stage)
        assert chain.plans_photometric
        geometry, planned_boxes, record = chain.plan(60, 80, labels, return_photometric=True)
        assert _same_state(np.random.get_state(), state)
        assert np.array_equal(planned_boxes, boxes)
        twin = sa.patch_resize_host(stage.apply(image, record), geometry, 30, 40)
        assert np.array_equal(twin, pixels), (seed, record, geometry)
        distorted += not np.array_equal(twin, sa.patch_resize_host(image, geometry, 30, 40))
        # with inverters, the record stays the last element
        np.random.seed(seed)
        out = chain.plan(60, 80, labels, return_inverter=True, return_photometric=True)
        assert len(out) == 4 and out[0] == geometry and tuple(out[3]) == tuple(record) and isinstance(out[2], list)
    assert distorted == 12


def test_plan_without_the_argument_returns_what_it_returned():
    from jpeg_detection_resnet_ssd_amd.data import ssd_augment as sa
    labels = np.array([[7, 10, 20, 50, 40], [2, 0, 0, 80, 60]])
    image = _noise(4, 60, 80)
    for seed in range(6):
        # a chain without the stage: the geometric draws alone, (geometry, labels), and the pixel call consumes the same
        np.random.seed(seed)
        plain = sa.SSDDataAugmentation(30, 40)
        assert not plain.plans_photometric
        out = plain.plan(60, 80, labels)
        state = np.random.get_state()
        assert len(out) == 2 and len(out[0]) == 7
        np.random.seed(seed)
        pixels, boxes = sa.SSDDataAugmentation(30, 40)(image, labels)
        assert _same_state(np.random.get_state(), state) and np.array_equal(boxes, out[1])
        assert np.array_equal(pixels, sa.patch_resize_host(image, out[0], 30, 40))
        # asked for a record, an empty slot gives None and draws nothing more
        np.random.seed(seed)
        with_none = plain.plan(60, 80, labels, return_photometric=True)
        assert _same_state(np.random.get_state(), state)
        assert len(with_none) == 3 and with_none[0] == out[0] and np.array_equal(with_none[1], out[1]) and with_none[2] is None
        # a chain WITH the stage, planned without the argument, leaves the stage out as it always did
        np.random.seed(seed)
        staged = sa.SSDDataAugmentation(30, 40, photometric_distortions=sa.SSDPhotometricDistortions()).plan(60, 80, labels)
        assert _same_state(np.random.get_state(), state) and len(staged) == 2 and staged[0] == out[0]
    with pytest.raises(ValueError):
        sa.SSDDataAugmentation(30, 40, photometric_distortions=lambda i, l: (i, l)).plan(60, 80, labels, return_photometric=True)


# ---- (e) records through the plan, the pending batch and the generator --------------------------------------------------------
def test_patch_plan_gets_a_fourth_part_only_with_records():
    from jpeg_detection_resnet_ssd_amd.data import ssd_photometric as sp
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import DevicePatchResize, PatchPlan, patch_resize_host
    images = [_noise(5, 20, 30), _noise(6, 9, 7), _noise(7, 12, 12)]
    geometries = [(2, 3, 10, 12, True, 3, (1, 2, 3)), (-4, -4, 20, 20, False, 0, (9, 9, 9)), (30, 0, 4, 4, False, 2, (0, 0, 0))]
    records = [(1, F(5), None, None, None, (0, 1, 2)), (2, None, F(0.75), F(1.5), None, (2, 1, 0)), (1, None, None, None, F(9), (0, 1, 2))]
    shapes = [im.shape[:2] for im in images]
    plain, full = PatchPlan(shapes, geometries, 8, 6), PatchPlan(shapes, geometries, 8, 6, records)
    assert plain.photo is None and plain.photo_offset is None and plain.photo_view(np.zeros(plain.nbytes, np.uint8)) is None
    assert plain.nbytes == plain.src_offset + plain.src_bytes
    assert (full.pool_offset, full.src_offset, full.src_bytes) == (plain.pool_offset, plain.src_offset, plain.src_bytes)
    assert full.photo_offset == plain.nbytes and full.photo_offset % 64 == 0 and full.nbytes == plain.nbytes + 3 * 40
    a, b = np.full(plain.nbytes, 0xEE, np.uint8), np.full(full.nbytes, 0xEE, np.uint8)
    plain.fill(a, images)
    full.fill(b, images)
    assert np.array_equal(a, b[:plain.nbytes])
    assert np.array_equal(full.photo_view(b), sp.pack_params(records)) and np.array_equal(full.desc, plain.desc)
    with pytest.raises(ValueError):
        PatchPlan(shapes, geometries, 8, 6, records[:2])
    prep = DevicePatchResize(8, 6)
    pending = prep(images, geometries, photometric=records)
    want = np.stack([patch_resize_host(sp.ssd_photometric_host(im, r), g, 8, 6) for im, r, g in zip(images, records, geometries)])
    assert np.array_equal(pending.pixels(), want) and not np.array_equal(want, prep(images, geometries).pixels())
    tail = pending[1:]
    assert len(tail) == 2 and [tuple(r) for r in tail.photometric] == [tuple(sp.check_params(r)) for r in records[1:]]
    assert np.array_equal(tail.pixels(), want[1:]) and tail.plan.photo is not None
    assert all(np.array_equal(x[1:], y) for x, y in zip(pending.numpy(), tail.numpy()))
    assert prep(images, geometries).photometric is None and prep(images, geometries)[1:].plan.photo is None


XML = """<annotation><folder>VOC2007</folder><filename>%s.jpg</filename>
<size><width>%d</width><height>%d</height><depth>3</depth></size>%s</annotation>"""
OBJ = """<object><name>%s</name><pose>Left</pose><truncated>0</truncated><difficult>0</difficult>
<bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>"""


def write_voc_tree(root):
    """Three small JPEGs with one or two boxes each -> a parsed DataGeneratorDCT."""
    from PIL import Image

    from jpeg_detection_resnet_ssd_amd.data.voc_generator import DataGeneratorDCT
    base = os.path.join(str(root), "VOC2007")
    for sub in ("JPEGImages", "Annotations", "ImageSets/Main"):
        os.makedirs(os.path.join(base, sub))
    items = [("000001", 60, 80, [("dog", 10, 12, 50, 44), ("person", 30, 5, 70, 55)]), ("000002", 48, 64, [("cat", 4, 4, 60, 40)]),
             ("000003", 75, 50, [("car", 5, 20, 45, 70)])]
    rng = np.random.default_rng(12)
    for image_id, h, w, objects in items:
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(3 * xx + yy) % 256, (2 * yy + 5 * xx) % 256, (xx * yy) % 256], axis=-1) + rng.integers(0, 20, (h, w, 3))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(base, "JPEGImages", image_id + ".jpg"), quality=95)
        with open(os.path.join(base, "Annotations", image_id + ".xml"), "w") as f:
            f.write(XML % (image_id, w, h, "".join(OBJ % o for o in objects)))
    with open(os.path.join(base, "ImageSets", "Main", "trainval.txt"), "w") as f:
        f.write("".join(i[0] + "\n" for i in items))
    gen = DataGeneratorDCT()
    gen.parse_xml([os.path.join(base, "JPEGImages")], [os.path.join(base, "ImageSets", "Main", "trainval.txt")],
                  [os.path.join(base, "Annotations")])
    return gen


def test_generator_host_path_equals_the_planned_path_with_the_stage(tmp_path):
    from jpeg_detection_resnet_ssd_amd.data import ssd_augment as sa
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import DevicePatchResize, PendingPatchInputs
    gen = write_voc_tree(tmp_path)
    for make in (sa.SSDDataAugmentation, sa.SSDDataAugmentationNoCrop):
        for seed in (0, 1):
            chain = make(48, 40, photometric_distortions=sa.SSDPhotometricDistortions())
            np.random.seed(seed)
            host_x, host_y = next(gen.generate(batch_size=3, shuffle=False, transformations=[chain],
                                               returns=["processed_images", "processed_labels"]))
            state = np.random.get_state()
            np.random.seed(seed)
            pending, dev_y = next(gen.generate(batch_size=3, shuffle=False, transformations=[chain],
                                               returns=["processed_images", "processed_labels"],
                                               device_prep=DevicePatchResize(48, 40)))
            assert _same_state(np.random.get_state(), state)
            assert isinstance(pending, PendingPatchInputs) and len(pending) == 3 and len(pending.photometric) == 3
            assert all(np.array_equal(a, b) for a, b in zip(host_y, dev_y))
            assert all(np.array_equal(a, b) for a, b in zip(host_x, pending.numpy()))
    # without the stage the generator calls device_prep as it always did
    calls = []

    def prep(images, geometries):
        calls.append(len(images))
        return "pending"
    prep.out_height, prep.out_width = 48, 40
    np.random.seed(0)
    assert next(gen.generate(batch_size=3, shuffle=False, transformations=[sa.SSDDataAugmentation(48, 40)],
                             returns=["processed_images"], device_prep=prep)) == ["pending"] and calls == [3]
