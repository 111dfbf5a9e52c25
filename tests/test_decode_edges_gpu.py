"""DecodeDetections / DecodeDetectionsFast on the device (`dj_decode_detections`, `dj_decode_detections_fast` through
the C ABI) against the plain restatement of the two TF layers in tests/decode_reference.py: which box, in which row.

Every call gets a workspace filled with NaN, an output filled with a sentinel and at least three images with different
content.  Two families of inputs:

* lattice inputs (zero offsets, unit variances, anchors with dyadic corners, power-of-two canvas, scores k/1024 or
  k/2048): every decoded coordinate, area, intersection and union is exact in float32, so the float32 statement IS the
  answer and the whole output tensor is compared bit for bit.  `expf(0) == 1` is assumed of the device;
* seeded SSD-like inputs: the test first asserts from the restatement alone that no decision (confidence threshold,
  IoU threshold, order of two scores) is closer than 1e-4 to going the other way, then demands the same rows in the same
  order: class exactly, confidence bit for bit, coordinates within 1e-5 * max(|coord|, canvas side) of the float64
  statement (at most six float32 operations, one of them expf, per coordinate: ~1e-6 relative, 8x headroom).

The rules stated here are TF's (`tf.image.non_max_suppression`, `tf.nn.top_k`, `tf.argmax`), not those of the host numpy
decoder, which differs by design for zero-area boxes (it drops a NaN IoU) and leaves the order of ties unspecified.

Measured on an MI355X (N = 2000, 6 classes, batch 3, canvas 300 x 500, the seeds of decode_reference.RANDOM_SEED):

    entry   min |conf - thresh|   min |IoU - thr|   min score gap   worst coordinate error
    full    5.8e-2                1.3e-3            4.3e-4          3.9e-5 px = 0.008 of the bound
    fast    5.4e-2                8.5e-4            2.2e-4          4.2e-5 px = 0.008 of the bound

Every lattice case was bit-exact, `expf(0) == 1` included."""
import numpy as np
import pytest

import decode_reference as R

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
ENTRIES = {"full": "dj_decode_detections", "fast": "dj_decode_detections_fast"}
U = 128.0                                   # lattice unit of box corners: 1/128 of the canvas


# ---- device call ---------------------------------------------------------------------------------------------------------
def workspace_floats(kind, b, n, n_classes, nms_max):
    from jpeg_detection_resnet_ssd_amd.engine import query
    if kind == "fast":
        return query("dj_decode_detections_fast_workspace_floats", b, n, nms_max)
    return query("dj_decode_detections_workspace_floats", b, n, n_classes, nms_max)


def device(kind, y, confidence_thresh, iou_threshold, top_k, nms_max_output_size, normalize_coords, img_height, img_width):
    """-> (out (b, top_k, 6), workspace) as numpy; the workspace starts as NaN, the output as SENTINEL."""
    import torch
    from jpeg_detection_resnet_ssd_amd.engine import call
    yt = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).cuda()
    b, n, width = yt.shape
    ws = torch.full((workspace_floats(kind, b, n, width - 12, nms_max_output_size),), float("nan"), device="cuda")
    out = torch.full((b, top_k, 6), SENTINEL, device="cuda")
    try:
        call(ENTRIES[kind], yt, b, n, width - 12, float(confidence_thresh), float(iou_threshold), int(top_k),
             int(nms_max_output_size), int(normalize_coords), int(img_height), int(img_width), ws, out)
    finally:
        torch.cuda.synchronize()
        device.last = (out.cpu().numpy(), ws.cpu().numpy())
    return device.last


def reference(kind, y, dtype, **args):
    fn = R.decode_detections if kind == "full" else R.decode_detections_fast
    return fn(y, dtype=dtype, **args)


def assert_bits_equal(out, rows):
    """The whole output tensor, bit for bit (NaN and the sign of zero included)."""
    want = np.ascontiguousarray(rows, dtype=np.float32)
    assert out.shape == want.shape
    same = out.view(np.uint32) == want.view(np.uint32)
    if not same.all():
        b, r = np.argwhere(~same.all(axis=-1))[0]
        raise AssertionError("image %d row %d: device %r, statement %r (%d rows differ)"
                             % (b, r, out[b, r].tolist(), want[b, r].tolist(), int((~same.all(axis=-1)).sum())))


def check_lattice(kind, y, ref=None, **args):
    """Run the device on a lattice input and compare the whole tensor with the float32 statement.  `ref` may hold the
    statement computed with a larger top_k: top-k rows are a prefix of it."""
    if ref is None:
        ref = reference(kind, y, np.float32, **args)
    out, ws = device(kind, y, **args)
    k = args["top_k"]
    rows = np.zeros((y.shape[0], k, 6))
    rows[:, :min(k, ref.rows.shape[1])] = ref.rows[:, :k]
    assert_bits_equal(out, rows)
    return ref, out, ws


# ---- lattice inputs ------------------------------------------------------------------------------------------------------
def blank(batch, n, n_classes):
    y = np.zeros((batch, n, n_classes + 12), dtype=np.float32)
    y[..., -4:] = 1.0                        # variances; offsets stay 0: the decoded box is the anchor
    return y


def put_boxes(y, b, corners):
    """Anchors of image b from corners (xmin, ymin, xmax, ymax) in units of 1/128."""
    c = np.asarray(corners, dtype=np.float64).reshape(-1, 4)
    y[b, :c.shape[0], -8] = (c[:, 0] + c[:, 2]) / (2 * U)
    y[b, :c.shape[0], -7] = (c[:, 1] + c[:, 3]) / (2 * U)
    y[b, :c.shape[0], -6] = (c[:, 2] - c[:, 0]) / U
    y[b, :c.shape[0], -5] = (c[:, 3] - c[:, 1]) / U
    return y


def disjoint(n, shift=0):
    """n boxes in n different cells of the 128 x 128 grid (touching at most): no pair overlaps."""
    assert n <= 128 * 128
    cell = (np.arange(n) + shift) % (128 * 128)
    x, yy = cell % 128, cell // 128
    return np.stack([x, yy, x + 1, yy + 1], axis=1)


def lattice_random(seed, batch, n, n_classes):
    """Overlapping boxes with corners on the 1/128 lattice, confidences k/1024 in every column (background included):
    equal scores, scores equal to a threshold of 0.5 and IoUs of exactly 0.5 all occur."""
    rng = np.random.RandomState(seed)
    y = blank(batch, n, n_classes)
    for b in range(batch):
        cx, cy = rng.randint(16, 113, size=n) * 2, rng.randint(16, 113, size=n) * 2          # centre * 256
        w, h = rng.randint(2, 25, size=n) * 2, rng.randint(2, 25, size=n) * 2                # size * 128
        put_boxes(y, b, np.stack([(cx - w) / 2, (cy - h) / 2, (cx + w) / 2, (cy + h) / 2], axis=1))
    y[..., :n_classes] = rng.randint(0, 1025, size=(batch, n, n_classes)) / 1024.0
    return y


LATTICE_ARGS = dict(confidence_thresh=0.5, iou_threshold=0.5, top_k=64, nms_max_output_size=20, normalize_coords=1,
                    img_height=256, img_width=512)


# ---- case 1: strided loops, wave reduction with idle lanes ---------------------------------------------------------------
@pytest.mark.parametrize("kind", ["full", "fast"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 600])
def test_sizes(kind, n):
    y = lattice_random(100 + n, 3, n, 3)
    ref, out, _ = check_lattice(kind, y, **LATTICE_ARGS)
    if n >= 63:
        assert (ref.index >= 0).sum() > 3                                   # the case is not empty


# ---- case 2: the three tie merges ----------------------------------------------------------------------------------------
def tie_input():
    n = 600
    rng = np.random.RandomState(2)
    y = blank(3, n, 3)
    for b in range(3):
        put_boxes(y, b, disjoint(n, shift=131 * b))
        for c in (1, 2):
            y[b, :, c] = 0.5 + (rng.permutation(n) + 1) / 2048.0             # all different, all above 0.5
    ties = {(0, 1): [(10, 11), (100, 164), (7, 263)],                         # adjacent lanes, two waves, same thread
            (0, 2): [(300, 301), (2, 66), (40, 296), (40, 552), (599, 87)],   # ... and a triple in one thread
            (2, 1): [(5, 133), (5, 517), (63, 64), (255, 256)],               # waves 0 and 2; lanes 63|0 of two waves
            (2, 2): [(0, 599), (191, 192), (20, 276)]}
    for (b, c), pairs in ties.items():
        for i, j in pairs:
            y[b, j, c] = y[b, i, c]
    for (b, c), pairs in ties.items():                                        # make the ties the best scores of their class
        for k, (i, j) in enumerate(pairs):
            members = np.nonzero(y[b, :, c] == y[b, i, c])[0]
            y[b, members, c] = 0.875 + (k + 1) / 2048.0
    y[1, :, 1:3] = 0.75                                                       # image 1: all N equal, in both classes
    return y


@pytest.mark.parametrize("kind", ["full", "fast"])
def test_equal_scores_go_by_box_index(kind):
    y = tie_input()
    args = dict(LATTICE_ARGS, top_k=1300, nms_max_output_size=600)
    ref, out, _ = check_lattice(kind, y, **args)
    # what the statement says, spelled out: among equal confidences of one class the box indices ascend
    for b in range(3):
        live = ref.index[b] >= 0
        cls, conf, idx = ref.rows[b][live, 0], ref.rows[b][live, 1], ref.index[b][live]
        assert live.sum() == (1200 if kind == "full" else 600)
        same = (cls[1:] == cls[:-1]) & (conf[1:] == conf[:-1])
        assert same.sum() >= (3 if b != 1 else 598) and np.all(idx[1:][same] > idx[:-1][same])
    if kind == "full":
        np.testing.assert_array_equal(ref.index[1][:1200], np.concatenate([np.arange(600), np.arange(600)]))


# ---- cases 3, 4, 5: strict IoU, strict confidence, zero-area boxes -------------------------------------------------------
def strict_iou_input():
    # width 48: a shift of 16 gives IoU 32/64 == 0.5, a shift of 15 gives 33/63, the next lattice value above
    y = blank(3, 6, 3)
    put_boxes(y, 0, [[0, 0, 48, 16], [16, 0, 64, 16], [0, 40, 48, 56], [15, 40, 63, 56], [0, 80, 16, 128], [0, 96, 16, 144]])
    y[0, :, 1] = [0.9375, 0.875, 0.8125, 0.75, 0.6875, 0.625]                 # pairs 0-1, 4-5 at 0.5: kept; 3 dropped
    put_boxes(y, 1, [[8, 8, 56, 24], [23, 8, 71, 24], [8, 8, 56, 24], [39, 8, 87, 24]])
    y[1, :4, 2] = [0.75, 0.875, 0.0, 0.625]                                   # 0 dropped by 1 (33/63); 3 at 0.5 with 1: kept
    y[1, 2, 1] = 0.75                                                         # same box, other class: not compared
    # chain: B (1) is suppressed by A (0); C (2) overlaps only B and is kept
    put_boxes(y, 2, [[0, 0, 48, 16], [10, 0, 58, 16], [20, 0, 68, 16]])
    y[2, :3, 1] = [0.875, 0.75, 0.625]
    return y


@pytest.mark.parametrize("kind", ["full", "fast"])
def test_iou_threshold_is_strict(kind):
    y = strict_iou_input()
    ref, out, _ = check_lattice(kind, y, **dict(LATTICE_ARGS, top_k=8))
    assert ref.margins["iou"] == 0.0                                          # a pair sat exactly on the threshold
    np.testing.assert_array_equal(ref.index[0], [0, 1, 2, 4, 5, -1, -1, -1])
    np.testing.assert_array_equal(ref.index[2], [0, 2, -1, -1, -1, -1, -1, -1])
    if kind == "full":
        np.testing.assert_array_equal(ref.index[1], [1, 2, 3, -1, -1, -1, -1, -1])


def strict_conf_input():
    up, down = np.nextafter(np.float32(0.5), np.float32(1)), np.nextafter(np.float32(0.5), np.float32(0))
    y = blank(3, 70, 3)
    for b in range(3):
        put_boxes(y, b, disjoint(70, shift=7 * b))
    y[0, :5, 1] = [0.5, up, np.nan, 0.75, down]
    y[0, 64:69, 2] = [np.nan, 0.5, 0.5, up, down]
    y[1, :, 1] = 0.5                                                          # image 1: nothing strictly above
    y[1, ::3, 2] = np.nan
    y[1, 1::3, 2] = down
    y[2, 69, 1] = up
    y[2, 0, 2] = np.nan
    return y


@pytest.mark.parametrize("kind", ["full", "fast"])
def test_confidence_threshold_is_strict(kind):
    y = strict_conf_input()
    ref, out, _ = check_lattice(kind, y, **dict(LATTICE_ARGS, top_k=5))
    np.testing.assert_array_equal(ref.index, [[3, 1, 67, -1, -1], [-1] * 5, [69, -1, -1, -1, -1]])
    assert np.all(out[1] == 0.0) and ref.margins["conf"] == 0.0


@pytest.mark.parametrize("kind", ["full", "fast"])
def test_zero_area_boxes_do_not_suppress(kind):
    """TF's rule: a pair with a box of no area has IoU 0 (on the device 0/0 = NaN, which is not above the threshold), so
    two identical degenerate boxes are both kept.  The host numpy decoder keeps one of them, by design: it filters with
    `iou <= threshold` and drops the NaN."""
    y = blank(3, 4, 2)
    put_boxes(y, 0, [[32, 32, 32, 32], [32, 32, 32, 32], [0, 0, 64, 64], [0, 0, 64, 64]])     # points in a box
    y[0, :, 1] = [0.9375, 0.875, 0.75, 0.625]
    put_boxes(y, 1, [[16, 0, 16, 64], [16, 0, 16, 64], [0, 8, 64, 8], [0, 8, 64, 8]])         # zero width, zero height
    y[1, :, 1] = [0.75, 0.75, 0.875, 0.625]
    put_boxes(y, 2, [[0, 0, 64, 64], [8, 8, 8, 8], [0, 0, 64, 64], [8, 8, 8, 8]])
    y[2, :, 1] = [0.625, 0.75, 0.9375, 0.875]
    ref, out, _ = check_lattice(kind, y, **dict(LATTICE_ARGS, top_k=5))
    np.testing.assert_array_equal(ref.index, [[0, 1, 2, -1, -1], [2, 0, 1, 3, -1], [2, 3, 1, -1, -1]])


# ---- case 6: NMS cap -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["full", "fast"])
def test_nms_cap_keeps_the_best(kind):
    rng = np.random.RandomState(6)
    b, n, nms_max = 3, 40, 7
    y = blank(b, n, 3)
    for i in range(b):
        put_boxes(y, i, disjoint(n, shift=50 * i))
        y[i, :, 1] = 0.5 + (rng.permutation(n) + 1) / 1024.0
        y[i, :, 2] = 0.5 + (rng.permutation(n) // 2 + 1) / 1024.0            # pairs of equal scores across the cut
    ref, out, ws = check_lattice(kind, y, **dict(LATTICE_ARGS, top_k=20, nms_max_output_size=nms_max))
    n_fg = 2 if kind == "full" else 1
    assert np.all((ref.index >= 0).sum(axis=1) == n_fg * nms_max)
    counts_at = b * n * (4 if kind == "full" else 6) + b * n_fg * nms_max * 6
    np.testing.assert_array_equal(ws[counts_at:counts_at + b * n_fg].view(np.int32), nms_max)
    if kind == "full":
        for i in range(b):
            rows = out[i][out[i][:, 0] == 1]
            np.testing.assert_array_equal(rows[:, 1], np.sort(y[i, :, 1])[::-1][:nms_max])


# ---- case 7: merge at capacity -------------------------------------------------------------------------------------------
def capacity_input():
    b, n, n_classes = 3, 1100, 9
    y = blank(b, n, n_classes)
    i = np.arange(n)
    for img in range(b):
        put_boxes(y, img, disjoint(n, shift=3000 * img))
        for c in range(1, n_classes):
            y[img, :, c] = 0.5 + (((i * (7 + 2 * img) + c * 3) % 16) + 1) / 64.0   # 16 values: ties within and across classes
    return y


@pytest.fixture(scope="module")
def capacity():
    y = capacity_input()
    args = dict(LATTICE_ARGS, top_k=8300, nms_max_output_size=1024)
    return y, {kind: reference(kind, y, np.float32, **args) for kind in ("full", "fast")}


@pytest.mark.parametrize("top_k", [1, 200, 8300])
@pytest.mark.parametrize("kind", ["full", "fast"])
def test_merge_at_capacity(capacity, kind, top_k):
    """8 x 1024 = 8192 valid keys: no padding key is left in the sort.  Order = confidence, then class, then NMS order (box
    index here); rows past the kept ones are zeros, also past 8192."""
    y, refs = capacity
    ref = refs[kind]
    kept = 8192 if kind == "full" else 1024
    assert np.all((ref.index >= 0).sum(axis=1) == kept)
    _, out, _ = check_lattice(kind, y, ref=ref, **dict(LATTICE_ARGS, top_k=top_k, nms_max_output_size=1024))
    if top_k > kept:
        assert np.all(out[:, kept:] == 0.0)
        conf, cls, idx = ref.rows[0][:kept, 1], ref.rows[0][:kept, 0], ref.index[0][:kept]
        tie = conf[1:] == conf[:-1]
        assert tie.sum() > kept - 20
        if kind == "full":                                                    # lower class first, then lower box index
            assert np.all(cls[1:][tie] >= cls[:-1][tie])
            tie &= cls[1:] == cls[:-1]
        assert np.all(idx[1:][tie] > idx[:-1][tie])


def test_top_k_larger_than_kept():
    y = lattice_random(77, 3, 65, 3)
    ref, out, _ = check_lattice("full", y, **dict(LATTICE_ARGS, top_k=9000))
    kept = (ref.index >= 0).sum(axis=1)
    assert kept.max() < 64 and all(np.all(out[b, kept[b]:] == 0.0) for b in range(3))


# ---- case 8: refusals ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,n_classes,nms_max", [("full", 8, 4, 2731), ("full", 12289, 3, 4), ("fast", 8, 3, 8193),
                                                      ("fast", 12289, 3, 4)])
def test_refusals_write_nothing(kind, n, n_classes, nms_max):
    from jpeg_detection_resnet_ssd_amd._lib import DjError
    y = blank(3, n, n_classes)
    y[..., 1] = 0.75
    with pytest.raises(DjError):
        device(kind, y, **dict(LATTICE_ARGS, top_k=5, nms_max_output_size=nms_max))
    out, ws = device.last
    assert np.all(out == SENTINEL) and np.all(np.isnan(ws))


# ---- case 9: N at the cap, grid-stride branch of the box and prep kernels -----------------------------------------------
@pytest.mark.parametrize("kind", ["full", "fast"])
def test_box_cap_and_grid_stride(kind):
    b, n = 43, 12288                                                          # 528384 boxes > 2048 blocks * 256
    assert b * n > 2048 * 256
    y = blank(b, n, 2)
    corners = disjoint(n)
    y[:, :, 1] = 0.25                                                         # arg-max class 1, below the threshold
    want = []
    for img in range(b):
        put_boxes(y, img, np.roll(corners, 97 * img, axis=0))
        at = [(img * 277) % n, n - 1 - img, 8192 + 5 * img, 4096 + img, 256 * img + 255]
        order = np.roll(np.arange(5), img)
        y[img, at, 1] = 0.5 + (order + 1) / 16.0
        want.append([at[i] for i in np.argsort(-order, kind="stable")])
    assert 42 * n + sorted(want[42])[-2] >= 2048 * 256                        # boxes only the grid-stride pass decodes
    ref, out, _ = check_lattice(kind, y, **dict(LATTICE_ARGS, top_k=8, nms_max_output_size=6))
    np.testing.assert_array_equal(ref.index[:, :5], want)
    assert np.all(ref.index[:, 5:] == -1)


# ---- case 10: canvas -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["full", "fast"])
@pytest.mark.parametrize("norm,height,width", [(1, 256, 512), (1, 512, 256), (0, 256, 512)])
def test_canvas_axes(kind, norm, height, width):
    y = lattice_random(10, 3, 65, 3)
    ref, out, _ = check_lattice(kind, y, **dict(LATTICE_ARGS, normalize_coords=norm, img_height=height, img_width=width))
    # x scales by the width and y by the height; without normalize_coords the boxes stay fractions of the canvas
    i = ref.index[0, 0]
    sx, sy = (width, height) if norm else (1, 1)
    p = y[0, i, -8:-4].astype(np.float64)
    np.testing.assert_array_equal(out[0, 0, 2:], [(p[0] - p[2] / 2) * sx, (p[1] - p[3] / 2) * sy, (p[0] + p[2] / 2) * sx,
                                                  (p[1] + p[3] / 2) * sy])


# ---- case 11: the fast path's own rules ----------------------------------------------------------------------------------
def test_fast_argmax_background_and_cross_class_suppression():
    y = blank(3, 6, 3)
    boxes = [[0, 0, 48, 16], [15, 0, 63, 16], [0, 32, 16, 48], [32, 32, 48, 48], [64, 32, 80, 48], [96, 32, 112, 48]]
    for b in range(3):
        put_boxes(y, b, boxes)
    # image 0: box 0 p1 == p2 maximal -> class 1; box 1 (class 2) overlaps box 0 (IoU 33/63): suppressed across classes;
    # box 2 p0 == p1 maximal -> background; box 3 background; box 4 p0 == p2 -> background; box 5 class 2
    y[0, :, 0] = [0.25, 0.25, 0.75, 0.875, 0.5625, 0.5]
    y[0, :, 1] = [0.75, 0.0, 0.75, 0.25, 0.25, 0.25]
    y[0, :, 2] = [0.75, 0.625, 0.5, 0.25, 0.5625, 0.5625]
    # image 1: the class-2 box is the higher one and suppresses the class-1 box
    y[1, :2, 1] = [0.75, 0.0]
    y[1, :2, 2] = [0.0, 0.875]
    # image 2: the arg-max is thresholded, not a lower class that would pass on its own
    y[2, :3, 0] = [0.875, 0.0, 0.0]
    y[2, :3, 1] = [0.75, 0.5, 0.625]
    y[2, :3, 2] = [0.75, 0.5, 0.625]
    ref, out, _ = check_lattice("fast", y, **dict(LATTICE_ARGS, top_k=4))
    np.testing.assert_array_equal(ref.index, [[0, 5, -1, -1], [1, -1, -1, -1], [2, -1, -1, -1]])
    np.testing.assert_array_equal(out[:, 0, 0], [1, 2, 1])                    # class id in column 0
    np.testing.assert_array_equal(out[0, 1, :2], [2, 0.5625])


@pytest.mark.parametrize("n", [1, 65, 600])
def test_fast_two_classes(n):
    y = lattice_random(200 + n, 3, n, 2)
    check_lattice("fast", y, **LATTICE_ARGS)


# ---- random inputs: exact sequence, bounded coordinates ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["full", "fast"])
def test_random_exact_sequence(kind):
    y = R.ssd_like_predictions(R.RANDOM_SEED[kind])
    args = R.RANDOM_ARGS
    ref = reference(kind, y, np.float64, **args)
    assert min(ref.margins.values()) >= R.MIN_MARGIN, ref.margins           # from the statement alone, nothing excluded
    out, _ = device(kind, y, **args)
    want = ref.rows.astype(np.float32)
    side = np.array([args["img_width"], args["img_height"]] * 2, dtype=np.float64)
    bound = 1e-5 * np.maximum(np.abs(ref.rows[..., 2:]), side)
    err = np.abs(out[..., 2:].astype(np.float64) - ref.rows[..., 2:])
    live = ref.index >= 0
    print("%s: margins %r, worst coordinate error %.3e px = %.3f of the bound, rows per image %r"
          % (kind, ref.margins, err.max(), (err / bound).max(), live.sum(axis=1).tolist()))
    np.testing.assert_array_equal(out[..., 0], want[..., 0])
    np.testing.assert_array_equal(out[..., 1].view(np.uint32), want[..., 1].view(np.uint32))
    assert np.all(out[~live] == 0.0)
    assert np.all(err <= bound), (err / bound).max()


# ---- the layer: the only place the (height, width) order of the ABI is bound ---------------------------------------------
@pytest.mark.parametrize("fast", [False, True])
def test_layer_binds_height_and_width(fast):
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras.layers import Input
    from jpeg_detection_resnet_ssd_amd.keras.models import Model
    from jpeg_detection_resnet_ssd_amd.keras_layers.keras_layer_DecodeDetections import DecodeDetections
    kind = "fast" if fast else "full"
    y = lattice_random(31, 3, 65, 3)
    args = dict(LATTICE_ARGS, top_k=30)
    K.clear_session()
    inp = Input((y.shape[1], y.shape[2]))
    layer = DecodeDetections(confidence_thresh=args["confidence_thresh"], iou_threshold=args["iou_threshold"],
                             top_k=args["top_k"], nms_max_output_size=args["nms_max_output_size"], normalize_coords=True,
                             img_height=args["img_height"], img_width=args["img_width"], fast=fast)
    model = Model(inp, layer(inp))
    det = model.predict(y, batch_size=3)
    ref, out, _ = check_lattice(kind, y, **args)                            # the direct ABI call, against the statement
    assert (ref.index >= 0).sum() > 6
    assert_bits_equal(np.ascontiguousarray(det, dtype=np.float32), out)
