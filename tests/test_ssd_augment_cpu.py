"""Host: the SSD augmentation chain restated in data/ssd_augment.py makes the reference's draws and boxes
(tests/golden/ssd_augment.npz, made from the reference's own modules), its planning mode makes the same draws without
touching a pixel, the window it plans is the picture the reference hands to its resize, the resize is Pillow's for all
five filters, and the Pascal-VOC generator built on it keeps the reference's batch rules on both of its paths.
Equality throughout: everything here is integer arithmetic or a replay of seeded draws."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssd_augment.npz")
NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX = 0, 1, 2, 3, 4
FILTERS = [NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX]
BG = (123, 117, 104)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- (a) the two added filters against the installed Pillow -----------------------------------------------------------------
@pytest.mark.parametrize("resample", [NEAREST, LANCZOS])
def test_nearest_and_lanczos_equal_pillow(resample):
    from PIL import Image
    from jpeg_detection_resnet_ssd_amd.data.ssd_augment import resize_host
    pairs = [((37, 53), (80, 111)), ((37, 53), (20, 24)), ((37, 53), (37, 20)), ((37, 53), (90, 53)), ((37, 53), (10, 200)),
             ((1, 1), (7, 5)), ((7, 5), (1, 1)), ((1, 9), (6, 9)), ((64, 48), (24, 20)), ((375, 500), (300, 300)),
             ((300, 8), (3, 300)), ((33, 47), (33, 47)), ((1500, 3), (300, 3)), ((3, 2000), (3, 300))]
    for k, ((h, w), (oh, ow)) in enumerate(pairs):
        x = _noise(100 + k, h, w)
        want = np.asarray(Image.fromarray(x).resize((ow, oh), resample))
        got = resize_host(x, (ow, oh), resample)
        assert got.shape == want.shape and np.array_equal(got, want), (resample, (h, w), (oh, ow), int((got != want).sum()))


def test_image_prep_still_refuses_the_two_filters():
    """The widened table lives in data/patch_resize.py; the classifier path's entry points keep their contract."""
    from jpeg_detection_resnet_ssd_amd.data import image_prep as ip, patch_resize as pr
    assert ip.SUPPORTED == (ip.BILINEAR, ip.BICUBIC, ip.BOX)
    for code in (ip.NEAREST, ip.LANCZOS):
        with pytest.raises(ValueError):
            ip.resolve_resample(code)
        assert pr.resolve_filter(code) == code
    with pytest.raises(ValueError):
        pr.resolve_filter(ip.HAMMING)
    assert pr.resolve_filter("lanczos") == ip.LANCZOS and pr.resolve_filter(None) == ip.BICUBIC


# ---- (b) patch_resize_host against a numpy canvas + Pillow ------------------------------------------------------------------
WINDOWS = {"inside": (5, 7, 20, 30), "starting_negative": (-6, -9, 25, 31), "past_both_far_edges": (20, 30, 40, 50),
           "expand": (-30, -45, 120, 170), "one_pixel": (11, 13, 1, 1), "one_pixel_outside": (-3, -2, 1, 1),
           "column_past_the_right_edge": (0, 52, 37, 4)}


def _canvas(image, y0, x0, h, w, background):
    """Pixel by pixel, from the definition: the window shows the image where it lies on it, the background elsewhere."""
    out = np.empty((h, w, 3), dtype=np.uint8)
    for y in range(h):
        for x in range(w):
            inside = 0 <= y0 + y < image.shape[0] and 0 <= x0 + x < image.shape[1]
            out[y, x] = image[y0 + y, x0 + x] if inside else background
    return out


@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_patch_resize_host_equals_canvas_then_pillow(name):
    from PIL import Image
    from jpeg_detection_resnet_ssd_amd.data.ssd_augment import patch_resize_host, window_host
    image = _noise(7, 37, 53)
    y0, x0, h, w = WINDOWS[name]
    canvas = _canvas(image, y0, x0, h, w, BG)
    for flip in (False, True):
        pre = np.ascontiguousarray(canvas[:, ::-1]) if flip else canvas
        for resample in FILTERS:
            geometry = (y0, x0, h, w, flip, resample, BG)
            assert np.array_equal(window_host(image, geometry), pre)
            want = np.asarray(Image.fromarray(pre).resize((20, 24), resample))
            got = patch_resize_host(image, geometry, 24, 20)
            assert got.shape == (24, 20, 3) and np.array_equal(got, want), (name, flip, resample)


def test_geometry_errors():
    from jpeg_detection_resnet_ssd_amd.data.ssd_augment import patch_resize_host
    image = _noise(8, 10, 12)
    for bad in ((0, 0, 0, 5, False, BILINEAR, BG), (0, 0, 5, -1, False, BILINEAR, BG), (0, 0, 5, 5, False, 5, BG),
                (0, 0, 5, 5, False, BILINEAR, (1, 2)), (0, 0, 5, 5, False, BILINEAR, (1, 2, 256))):
        with pytest.raises(ValueError):
            patch_resize_host(image, bad, 4, 4)


# ---- (c) the chain against the reference's own run --------------------------------------------------------------------------
def _case_names(golden):
    return [str(n) for n in golden["names"]]


def _transform_for(name, golden, degenerate_filter=False):
    """The chain as the fixture's maker ran the reference: its `ResizeRandomInterp` had no box filter."""
    from jpeg_detection_resnet_ssd_amd.data import ssd_augment as sa
    oh, ow = (int(v) for v in golden["out_size"])
    if not name.startswith("resize/"):
        chain = (sa.SSDDataAugmentation if name.startswith("full/") else sa.SSDDataAugmentationNoCrop)(img_height=oh, img_width=ow)
        assert isinstance(chain.resize.resize.box_filter, sa.BoxFilter) and chain.resize.resize.box_filter.check_degenerate
        if not degenerate_filter:
            chain.resize.box_filter = chain.resize.resize.box_filter = None
        return chain, lambda t: t.resize.resize.interpolation_mode
    assert name.startswith("resize/")
    code = int(golden[name + "/interpolation"])
    return sa.Resize(height=oh, width=ow, interpolation_mode=code), lambda t: t.interpolation_mode


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_fixture_holds_every_group_filter_and_stage(golden):
    names = _case_names(golden)
    assert len(names) == 55 and sum(n.startswith("full/") for n in names) == 40
    assert {int(golden[n + "/interpolation"]) for n in names} == {0, 1, 2, 3, 4}
    grown = [n for n in names if golden[n + "/pre_resize"].shape[0] > golden[n + "/image"].shape[0]]
    shrunk = [n for n in names if golden[n + "/pre_resize"].shape[0] < golden[n + "/image"].shape[0]]
    assert len(grown) >= 5 and len(shrunk) >= 5
    assert any(golden[n + "/labels"].dtype == np.float64 for n in names) and any(golden[n + "/labels"].dtype == np.int64 for n in names)


def test_chain_reproduces_the_reference_run_and_plan_makes_the_same_draws(golden):
    from jpeg_detection_resnet_ssd_amd.data import ssd_augment as sa
    oh, ow = (int(v) for v in golden["out_size"])
    checked = flipped = 0
    for name in _case_names(golden):
        image, labels = golden[name + "/image"], golden[name + "/labels"]
        seed, interpolation = int(golden[name + "/seed"]), int(golden[name + "/interpolation"])
        transform, drawn_mode = _transform_for(name, golden)

        np.random.seed(seed)
        pixels, out_labels = transform(image, labels)
        state_pixels = np.random.get_state()
        assert int(drawn_mode(transform)) == interpolation, name
        assert out_labels.dtype == golden[name + "/out_labels"].dtype and np.array_equal(out_labels, golden[name + "/out_labels"]), name
        assert pixels.shape == (oh, ow, 3) and pixels.dtype == np.uint8

        np.random.seed(seed)
        geometry, plan_labels = transform.plan(image.shape[0], image.shape[1], labels)
        assert _same_state(np.random.get_state(), state_pixels), name
        assert plan_labels.dtype == out_labels.dtype and np.array_equal(plan_labels, out_labels), name
        assert geometry[5] == sa.CV2_TO_PILLOW[interpolation], name
        assert np.array_equal(sa.window_host(image, geometry), golden[name + "/pre_resize"]), name
        assert np.array_equal(sa.patch_resize_host(image, geometry, oh, ow), pixels), name
        np.array_equal(labels, golden[name + "/labels"])      # the inputs are left as they were
        checked += 1
        flipped += bool(geometry[4])
    assert checked == len(golden["names"]) and 10 <= flipped <= checked - 10


def test_chain_drops_the_boxes_its_resize_flattens(golden):
    """With the chain's own box filter on the resize stage the boxes are the fixture's minus the degenerate ones (the
    filter draws nothing, so everything else is unchanged)."""
    from jpeg_detection_resnet_ssd_amd.data import ssd_augment as sa
    dropped = 0
    for name in _case_names(golden):
        if name.startswith("resize/"):
            continue
        np.random.seed(int(golden[name + "/seed"]))
        image, labels = golden[name + "/image"], golden[name + "/labels"]
        _, out = _transform_for(name, golden, degenerate_filter=True)[0].plan(image.shape[0], image.shape[1], labels)
        want = golden[name + "/out_labels"]
        keep = (want[:, 3] > want[:, 1]) & (want[:, 4] > want[:, 2])
        assert np.array_equal(out, want[keep]), name
        dropped += int((~keep).sum())
    assert dropped >= 1


def test_plan_of_single_stages_composes_like_the_chain(golden):
    """Planned one transform at a time, each handed the geometry so far (what the generator's device path does with a list
    of transformations), the stages give the chain's geometry and boxes."""
    from jpeg_detection_resnet_ssd_amd.data import ssd_augment as sa
    oh, ow = (int(v) for v in golden["out_size"])
    for name in _case_names(golden)[:12]:
        image, labels = golden[name + "/image"], golden[name + "/labels"]
        seed = int(golden[name + "/seed"])
        h, w = image.shape[:2]
        np.random.seed(seed)
        want_geometry, want_labels = sa.SSDDataAugmentation(oh, ow).plan(h, w, labels)
        np.random.seed(seed)
        geometry, out = None, labels
        resize = sa.ResizeRandomInterp(oh, ow, box_filter=sa.BoxFilter(check_overlap=False, check_min_area=False,
                                                                       check_degenerate=True))
        for stage in (sa.SSDExpand(), sa.SSDRandomCrop(), sa.RandomFlip(), resize):
            geometry, out = stage.plan(h, w, out, geometry=geometry)
        assert geometry == want_geometry and np.array_equal(out, want_labels), name


def test_what_cannot_be_one_window_raises():
    from jpeg_detection_resnet_ssd_amd.data import ssd_augment as sa
    crop = sa.CropPad(2, 2, 10, 10)
    pad = sa.CropPad(-5, -5, 40, 40, background=BG)
    geometry = crop.plan(20, 30)
    assert geometry[:5] == (2, 2, 10, 10, False)
    with pytest.raises(ValueError):
        pad.plan(20, 30, geometry=geometry)                    # padding after a crop: the source would show through
    padded = pad.plan(20, 30)
    with pytest.raises(ValueError):
        sa.CropPad(-1, -1, 50, 50, background=(0, 0, 0)).plan(20, 30, geometry=padded)      # a second colour
    resized = sa.Resize(8, 8).plan(20, 30)
    for late in (crop, sa.Flip(), sa.Resize(4, 4)):
        with pytest.raises(ValueError):
            late.plan(20, 30, geometry=resized)
    with pytest.raises(ValueError):
        sa.Flip(dim="vertical").plan(20, 30)
    # a crop of a mirrored picture is taken from the other side of the source
    mirrored = sa.Flip().plan(20, 30)
    assert sa.CropPad(0, 3, 20, 10).plan(20, 30, geometry=mirrored)[:5] == (0, 17, 20, 10, True)
    image = _noise(9, 20, 30)
    assert np.array_equal(sa.window_host(image, sa.CropPad(0, 3, 20, 10).plan(20, 30, geometry=mirrored)),
                          sa.CropPad(0, 3, 20, 10)(sa.Flip()(image)))


def test_can_fail_patch_plans_to_none():
    from jpeg_detection_resnet_ssd_amd.data import ssd_augment as sa
    never = sa.ImageValidator(overlap_criterion="iou", bounds=(0.99, 1.0), n_boxes_min=1)
    patch = sa.RandomPatch(sa.PatchCoordinateGenerator(min_scale=0.3, max_scale=0.4), image_validator=never, n_trials_max=2,
                           can_fail=True)
    labels = np.array([[1, 1, 1, 3, 3]])
    np.random.seed(0)
    assert patch(_noise(1, 40, 40), labels) == (None, None)
    np.random.seed(0)
    assert patch.plan(40, 40, labels) is None


def test_photometric_callable_runs_first_and_only_in_pixel_mode():
    from jpeg_detection_resnet_ssd_amd.data import ssd_augment as sa
    seen = []

    def invert(image, labels):
        seen.append(image.shape)
        return 255 - image, labels
    image, labels = _noise(3, 40, 50), np.array([[3, 5, 6, 30, 31]])
    np.random.seed(5)
    with_callable, l1 = sa.SSDDataAugmentation(24, 20, photometric_distortions=invert)(image, labels)
    np.random.seed(5)
    plain, l2 = sa.SSDDataAugmentation(24, 20)(255 - image, labels)
    assert seen == [(40, 50, 3)] and np.array_equal(with_callable, plain) and np.array_equal(l1, l2)
    np.random.seed(5)
    geometry, l3 = sa.SSDDataAugmentation(24, 20, photometric_distortions=invert).plan(40, 50, labels)
    assert len(seen) == 1 and np.array_equal(l3, l1)
    with pytest.raises(ValueError):
        sa.SSDDataAugmentation(photometric_distortions="yes")


# ---- (d) inverters ----------------------------------------------------------------------------------------------------------
def test_inverters_round_trip_resize_and_expand():
    from jpeg_detection_resnet_ssd_amd.data import ssd_augment as sa
    image = _noise(4, 60, 80)
    labels = np.array([[7, 10, 20, 50, 40], [2, 0, 0, 80, 60]], dtype=np.float64)
    # predictions carry one more leading column (class, confidence, box), which is what the inverters shift
    as_prediction = lambda y: np.concatenate([y[:, :1], np.full((len(y), 1), 0.5), y[:, 1:]], axis=1)   # noqa: E731
    _, resized, inverter = sa.Resize(30, 20)(image, labels, return_inverter=True)
    assert np.array_equal(resized, [[7, 2, 10, 12, 20], [2, 0, 0, 20, 30]])
    assert np.array_equal(inverter(as_prediction(resized))[:, 2:], [[8, 20, 48, 40], [0, 0, 80, 60]])      # 2 * 4, 12 * 4: multiples of the scale
    np.random.seed(1)      # first draw 0.417 < 0.5 keeps the image; seed 3 (0.55) expands
    np.random.seed(3)
    expanded, moved, inverter = sa.SSDExpand()(image, labels, return_inverter=True)
    assert expanded.shape[0] > 60 and not np.array_equal(moved, labels)
    assert np.array_equal(inverter(as_prediction(moved))[:, 2:], labels[:, 1:])
    np.random.seed(3)
    geometry, moved_plan, inverter = sa.SSDExpand().plan(60, 80, labels, return_inverter=True)
    assert np.array_equal(moved_plan, moved) and np.array_equal(inverter(as_prediction(moved))[:, 2:], labels[:, 1:])
    # the whole chain: inverters come last stage first and undo resize, crop and expand up to the resize's rounding
    np.random.seed(11)
    _, out, inverters = sa.SSDDataAugmentation(30, 40)(image, labels, return_inverter=True)
    assert len(inverters) == 3


# ---- (e) the generator on a tiny VOC tree -----------------------------------------------------------------------------------
XML = """<annotation><folder>VOC2007</folder><filename>%s.jpg</filename>
<size><width>%d</width><height>%d</height><depth>3</depth></size>%s</annotation>"""
OBJ = """<object><name>%s</name><pose>Left</pose><truncated>%d</truncated><difficult>%d</difficult>
<bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox>
<part><name>head</name><bndbox><xmin>1</xmin><ymin>1</ymin><xmax>2</xmax><ymax>2</ymax></bndbox></part></object>"""


@pytest.fixture(scope="module")
def voc_tree(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("voc")
    for sub in ("JPEGImages", "Annotations", "ImageSets/Main"):
        os.makedirs(os.path.join(root, "VOC2007", sub))
    items = [("000001", 60, 80, [("dog", 0, 0, 10, 12, 50, 44), ("person", 1, 1, 30, 5, 70, 55)]),
             ("000002", 48, 64, []),
             ("000003", 75, 50, [("car", 0, 0, 5, 20, 45, 70)])]
    rng = np.random.default_rng(12)
    for image_id, h, w, objects in items:
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(3 * xx + yy) % 256, (2 * yy + 5 * xx) % 256, (xx * yy) % 256], axis=-1) + rng.integers(0, 20, (h, w, 3))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(
            os.path.join(root, "VOC2007", "JPEGImages", image_id + ".jpg"), quality=95)
        with open(os.path.join(root, "VOC2007", "Annotations", image_id + ".xml"), "w") as f:
            f.write(XML % (image_id, w, h, "".join(OBJ % o for o in objects)))
    with open(os.path.join(root, "VOC2007", "ImageSets", "Main", "trainval.txt"), "w") as f:
        f.write("".join(i[0] + "\n" for i in items))
    return str(root)


def _parsed(voc_tree, **kwargs):
    from jpeg_detection_resnet_ssd_amd.data.voc_generator import DataGeneratorDCT
    base = os.path.join(voc_tree, "VOC2007")
    gen = DataGeneratorDCT()
    out = gen.parse_xml([os.path.join(base, "JPEGImages")], [os.path.join(base, "ImageSets", "Main", "trainval.txt")],
                        [os.path.join(base, "Annotations")], ret=True, **kwargs)
    return gen, out


def test_parse_xml(voc_tree):
    gen, (images, filenames, labels, image_ids, eval_neutral) = _parsed(voc_tree)
    assert images is None and image_ids == ["000001", "000002", "000003"] and gen.get_dataset_size() == 3
    assert [os.path.basename(f) for f in filenames] == ["000001.jpg", "000002.jpg", "000003.jpg"]
    assert labels == [[[12, 10, 12, 50, 44], [15, 30, 5, 70, 55]], [], [[7, 5, 20, 45, 70]]]      # the part's box is no object's
    assert eval_neutral == [[False, True], [], [False]]
    gen, out = _parsed(voc_tree, exclude_difficult=True)
    assert out[2] == [[[12, 10, 12, 50, 44]], [], [[7, 5, 20, 45, 70]]] and out[4] == [[False], [], [False]]
    gen, out = _parsed(voc_tree, exclude_truncated=True, include_classes=[12, 15])
    assert out[2] == [[[12, 10, 12, 50, 44]], [], []]


def test_generator_batch_rules_and_order_of_returns(voc_tree):
    from jpeg_detection_resnet_ssd_amd.data import ssd_augment as sa
    from jpeg_detection_resnet_ssd_amd.data.voc_generator import DegenerateBatchError
    gen, _ = _parsed(voc_tree)
    returns = {"processed_images", "encoded_labels", "processed_labels", "filenames", "image_ids", "evaluation-neutral",
               "inverse_transform", "original_images", "original_labels"}
    g = gen.generate(batch_size=3, shuffle=False, transformations=[sa.Resize(32, 48)], label_encoder=lambda y: ("encoded", len(y)),
                     returns=returns, keep_images_without_gt=False)
    x, encoded, y, filenames, ids, neutral, inverse, original_images, original_labels = next(g)
    assert ids == ["000001", "000003"] and [os.path.basename(f) for f in filenames] == ["000001.jpg", "000003.jpg"]
    assert encoded == ("encoded", 2) and neutral == [[False, True], [False]]
    assert [a.shape for a in x] == [(2, 4, 6, 64), (2, 2, 3, 128)] and all(a.dtype == np.float32 for a in x)
    assert np.array_equal(y[0], [[12, 6, 6, 30, 23], [15, 18, 3, 42, 29]]) and np.array_equal(y[1], [[7, 5, 9, 43, 30]])
    assert [im.shape for im in original_images] == [(60, 80, 3), (75, 50, 3)]
    assert original_labels == [[[12, 10, 12, 50, 44], [15, 30, 5, 70, 55]], [[7, 5, 20, 45, 70]]]
    assert [len(i) for i in inverse] == [1, 1]
    assert next(g)[4] == ["000001", "000003"]                # wraps around
    kept = next(gen.generate(batch_size=3, shuffle=False, transformations=[sa.Resize(32, 48)],
                             returns=["image_ids", "processed_labels", "processed_images"], keep_images_without_gt=True,
                             deconv=True))
    assert [a.shape for a in kept[0]] == [(3, 4, 6, 64), (3, 2, 3, 64), (3, 2, 3, 64)]
    assert kept[2] == ["000001", "000002", "000003"] and kept[1][1].shape == (0, 5)
    # a box a transformation flattens is removed, and the image with it when it was its last one
    def flatten_dogs(image, labels):
        labels = labels.copy()
        labels[labels[:, 0] == 12, 4] = labels[labels[:, 0] == 12, 2]
        return image[:32, :48], labels
    out = next(gen.generate(batch_size=3, shuffle=False, transformations=[flatten_dogs], returns=["image_ids", "processed_labels"]))
    assert out[1] == ["000001", "000003"] and [y[:, 0].tolist() for y in out[0]] == [[15], [7]]

    def flatten_all(image, labels):
        return image[:32, :48], labels * np.array([1, 1, 0, 1, 0])
    out = next(gen.generate(batch_size=3, shuffle=False, transformations=[flatten_all], returns=["image_ids", "processed_labels"],
                            keep_images_without_gt=True))
    assert out[1] == ["000001", "000002", "000003"] and [len(y) for y in out[0]] == [0, 0, 0]
    with pytest.raises(DegenerateBatchError):
        next(gen.generate(batch_size=3, shuffle=False, transformations=[flatten_all], returns=["image_ids"]))
    with pytest.raises(ValueError) as e:
        next(gen.generate(batch_size=3, transformations=[lambda image, labels: (image, labels)], device_prep=object()))
    assert "plan" in str(e.value)


@pytest.mark.parametrize("deconv", [False, True])
def test_generator_host_path_equals_the_planned_path(voc_tree, deconv):
    """Under one seed the host path (pixel-mode chain, then the JPEG round trip) and the device path's host twin (planned
    geometries, `patch_resize_host`, then either statement of the JPEG transform) give the same inputs and boxes."""
    from jpeg_detection_resnet_ssd_amd.data import ssd_augment as sa
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import emit_dct_inputs
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import DevicePatchResize, PendingPatchInputs
    gen, _ = _parsed(voc_tree)
    for chain in (sa.SSDDataAugmentation, sa.SSDDataAugmentationNoCrop):
        for seed in (0, 1, 2):
            np.random.seed(seed)
            host_x, host_y = next(gen.generate(batch_size=3, shuffle=False, transformations=[chain(48, 40)],
                                               returns=["processed_images", "processed_labels"], deconv=deconv))
            np.random.seed(seed)
            pending, dev_y = next(gen.generate(batch_size=3, shuffle=False, transformations=[chain(48, 40)],
                                               returns=["processed_images", "processed_labels"], deconv=deconv,
                                               device_prep=DevicePatchResize(48, 40, deconv=deconv)))
            assert isinstance(pending, PendingPatchInputs) and len(pending) == 2 and pending.shape == (2, 48, 40, 3)
            assert pending.shapes == [tuple(a.shape) for a in host_x]
            assert all(np.array_equal(a, b) for a, b in zip(host_y, dev_y))
            images = [gen._decode(f) for f in (gen.filenames[0], gen.filenames[2])]
            pixels = np.stack([sa.patch_resize_host(im, g, 48, 40) for im, g in zip(images, pending.geometries)])
            assert np.array_equal(pending.pixels(), pixels)
            for a, b, c in zip(host_x, emit_dct_inputs(pixels, deconv=deconv), pending.numpy()):
                assert a.dtype == np.float32 and np.array_equal(a, b) and np.array_equal(a, c)
            tail = pending[1:]
            assert len(tail) == 1 and all(np.array_equal(a[1:], b) for a, b in zip(pending.numpy(), tail.numpy()))
            with pytest.raises(TypeError):
                pending[0]
    with pytest.raises(ValueError):
        next(gen.generate(batch_size=3, transformations=[sa.SSDDataAugmentation(48, 40)], device_prep=DevicePatchResize(40, 48)))


def test_patch_plan_stages_only_what_the_window_covers():
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import DESC_DTYPE, PatchPlan
    images = [_noise(20, 100, 120), _noise(21, 50, 60), _noise(22, 10, 10)]
    geometries = [(10, 20, 30, 40, True, BICUBIC, BG), (-20, -30, 200, 240, False, NEAREST, BG), (40, 40, 5, 5, False, BOX, BG)]
    plan = PatchPlan([im.shape[:2] for im in images], geometries, 24, 20)
    d = plan.desc
    assert d.dtype == DESC_DTYPE and DESC_DTYPE.itemsize == 80
    assert [(int(a), int(b)) for a, b in zip(d["src_h"], d["src_w"])] == [(30, 40), (50, 60), (0, 0)]
    assert [(int(a), int(b)) for a, b in zip(d["win_y0"], d["win_x0"])] == [(0, 0), (-20, -30), (40, 40)]
    assert plan.src_bytes == 3 * 30 * 40 + 3 * 50 * 60 + (-(3 * 30 * 40) % 64) + (-(3 * 50 * 60) % 64)
    assert int(d["background"][0]) == 123 | (117 << 8) | (104 << 16) and list(d["flip"]) == [1, 0, 0]
    staging = np.zeros(plan.nbytes, dtype=np.uint8)
    plan.fill(staging, images)
    src, desc, pool = plan.views(staging)
    assert np.array_equal(src[:3600].reshape(30, 40, 3), images[0][10:40, 20:60]) and np.array_equal(desc, plan.desc)
    assert np.array_equal(pool, plan.pool) and int(d["scratch_offset"][1]) == -(-(3 * 20 * 30) // 64) * 64
