"""Plain restatement of the reference's two decoding layers, `DecodeDetections` and `DecodeDetectionsFast`
(localisation_part/keras_layers/keras_layer_DecodeDetections.py:109-265, ...Fast.py:111-260), written from what the TF
ops they are made of do.  It is the oracle of tests/test_decode_edges_gpu.py and imports nothing from the package.

Rules, as TF 1.x implements them:

* box decode: cx = cx_pred * var_cx * w_anchor + cx_anchor, w = exp(w_pred * var_w) * w_anchor (same for y / h), corners
  = centre -/+ half the size, then x * img_width and y * img_height when `normalize_coords`;
* threshold: `conf > confidence_thresh`, both float32 (the layer holds the threshold as a float32 constant).  A NaN
  confidence compares false and is never a candidate;
* `tf.image.non_max_suppression`: candidates in descending score, equal scores by ascending box index; a candidate is
  dropped when its IoU with an already selected box is `> iou_threshold` (float32); the IoU of a pair with a box of area
  <= 0 is 0 (TF) -- a 0/0 of a kernel compares false, the same decision -- so such a pair never suppresses; the loop
  stops at `nms_max_output_size` selected boxes;
* top-k: the per-class results, each padded to `nms_max_output_size` rows, are concatenated class-major; `tf.nn.top_k`
  sorts by confidence descending and returns the lower position first among equal values, i.e. lower class, then NMS
  order; rows past the selected ones are zeros;
* fast layer: `tf.argmax` (first maximum) over ALL classes and that confidence; boxes whose arg-max is class 0 are
  dropped; threshold; ONE NMS over what is left; column 0 carries the arg-max class.

`dtype` is the arithmetic of the box decode and of the IoU: float64 for the bounded comparison of random inputs, float32
for lattice inputs on which every float32 operation is exact, so that the result is THE float32 answer bit for bit.

Besides the rows the functions return, per row, the index of the box it came from (-1 for padding) and the decision
margins of the run: how far any comparison that decided something was from going the other way."""
import collections

import numpy as np

Decoded = collections.namedtuple("Decoded", "rows index margins")


def _new_margins():
    return {"conf": np.inf, "iou": np.inf, "score": np.inf}


def _note(margins, key, value):
    if value < margins[key]:
        margins[key] = float(value)


def _note_score_gaps(margins, scores):
    """Smallest gap between two DISTINCT values of a set of scores that are ordered against each other."""
    u = np.unique(np.asarray(scores, dtype=np.float64))
    if u.size > 1:
        _note(margins, "score", np.min(np.diff(u)))


def decode_boxes(y_pred, normalize_coords, img_height, img_width, dtype=np.float64):
    """(batch, N, n_classes + 12) -> (batch, N, 4) corners [xmin, ymin, xmax, ymax] in `dtype` arithmetic."""
    p = np.asarray(y_pred)[..., -12:].astype(dtype)
    half = dtype(0.5)
    cx = p[..., 0] * p[..., 8] * p[..., 6] + p[..., 4]
    cy = p[..., 1] * p[..., 9] * p[..., 7] + p[..., 5]
    w = np.exp(p[..., 2] * p[..., 10]) * p[..., 6]
    h = np.exp(p[..., 3] * p[..., 11]) * p[..., 7]
    sx = dtype(img_width) if normalize_coords else dtype(1)
    sy = dtype(img_height) if normalize_coords else dtype(1)
    out = np.stack([(cx - half * w) * sx, (cy - half * h) * sy, (cx + half * w) * sx, (cy + half * h) * sy], axis=-1)
    assert out.dtype == dtype
    return out


def _iou_one_to_many(box, others):
    """IoU of one box with each row of `others`, in the arrays' own dtype; (values, valid): `valid` is False where one of
    the two areas is <= 0 -- TF defines that IoU as 0, a plain division gives 0 or NaN: never above a threshold."""
    zero = box.dtype.type(0)
    iw = np.maximum(zero, np.minimum(box[2], others[:, 2]) - np.maximum(box[0], others[:, 0]))
    ih = np.maximum(zero, np.minimum(box[3], others[:, 3]) - np.maximum(box[1], others[:, 1]))
    inter = iw * ih
    area = (box[2] - box[0]) * (box[3] - box[1])
    areas = (others[:, 2] - others[:, 0]) * (others[:, 3] - others[:, 1])
    valid = (areas > zero) & (area > zero)
    union = area + areas - inter
    values = np.zeros(others.shape[0], dtype=box.dtype)
    np.divide(inter, union, out=values, where=valid)
    return values, valid


def greedy_nms(scores, boxes, candidates, iou_threshold, max_output_size, margins):
    """`tf.image.non_max_suppression` over the boxes `candidates` (ascending indices into scores / boxes).
    -> selected box indices in selection order."""
    thr = np.float32(iou_threshold)
    candidates = np.asarray(candidates, dtype=np.int64)
    _note_score_gaps(margins, scores[candidates])
    # descending score, equal scores by ascending index: a stable sort of ascending indices
    order = candidates[np.argsort(-scores[candidates].astype(np.float64), kind="stable")]
    selected = []
    sel_boxes = np.empty((min(max_output_size, order.size), 4), dtype=boxes.dtype)
    for i in order:
        if len(selected) >= max_output_size:
            break
        values, valid = _iou_one_to_many(boxes[i], sel_boxes[:len(selected)])
        if np.any(valid):
            _note(margins, "iou", np.min(np.abs(values[valid].astype(np.float64) - np.float64(thr))))
        if np.any(valid & (values > thr)):
            continue
        sel_boxes[len(selected)] = boxes[i]
        selected.append(int(i))
    return selected


def _top_k(rows, index, top_k, margins):
    """rows (R, 6) in concatenation order -> (top_k, 6), (top_k,): `tf.nn.top_k` on column 1 of the zero-padded rows."""
    out = np.zeros((top_k, 6), dtype=np.float64)
    out_index = np.full(top_k, -1, dtype=np.int64)
    if rows.shape[0]:
        _note_score_gaps(margins, rows[:, 1])
        order = np.argsort(-rows[:, 1], kind="stable")[:top_k]
        out[:order.size] = rows[order]
        out_index[:order.size] = index[order]
    return out, out_index


def _conf_margin(margins, conf, thresh):
    d = np.abs(conf.astype(np.float64) - np.float64(thresh))
    d = d[np.isfinite(d)]
    if d.size:
        _note(margins, "conf", d.min())


def decode_detections(y_pred, confidence_thresh, iou_threshold, top_k, nms_max_output_size, normalize_coords,
                      img_height, img_width, dtype=np.float64):
    """The `DecodeDetections` layer.  -> Decoded(rows (batch, top_k, 6) float64, index (batch, top_k), margins)."""
    y_pred = np.asarray(y_pred, dtype=np.float32)
    batch, _, width = y_pred.shape
    n_classes = width - 12
    thresh = np.float32(confidence_thresh)
    boxes = decode_boxes(y_pred, normalize_coords, img_height, img_width, dtype)
    margins = _new_margins()
    rows_out = np.zeros((batch, top_k, 6), dtype=np.float64)
    index_out = np.full((batch, top_k), -1, dtype=np.int64)
    for b in range(batch):
        rows, index = [], []
        for cls in range(1, n_classes):
            conf = y_pred[b, :, cls]
            _conf_margin(margins, conf, thresh)
            candidates = np.nonzero(conf > thresh)[0]          # NaN > thresh is False
            for i in greedy_nms(conf, boxes[b], candidates, iou_threshold, nms_max_output_size, margins):
                rows.append([float(cls), float(conf[i])] + [float(v) for v in boxes[b, i]])
                index.append(i)
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
        rows_out[b], index_out[b] = _top_k(rows, np.asarray(index, dtype=np.int64), top_k, margins)
    return Decoded(rows_out, index_out, margins)


def decode_detections_fast(y_pred, confidence_thresh, iou_threshold, top_k, nms_max_output_size, normalize_coords,
                           img_height, img_width, dtype=np.float64):
    """The `DecodeDetectionsFast` layer.  Same return value as `decode_detections`."""
    y_pred = np.asarray(y_pred, dtype=np.float32)
    batch, _, width = y_pred.shape
    n_classes = width - 12
    thresh = np.float32(confidence_thresh)
    boxes = decode_boxes(y_pred, normalize_coords, img_height, img_width, dtype)
    margins = _new_margins()
    rows_out = np.zeros((batch, top_k, 6), dtype=np.float64)
    index_out = np.full((batch, top_k), -1, dtype=np.int64)
    for b in range(batch):
        probs = y_pred[b, :, :n_classes]
        cls = np.zeros(probs.shape[0], dtype=np.int64)
        conf = probs[:, 0].copy()
        for c in range(1, n_classes):                           # tf.argmax: a later class wins only when strictly larger
            better = probs[:, c] > conf
            cls[better] = c
            conf[better] = probs[better, c]
        # arg-max decisions: the winner against every different value of its row
        gap = np.abs(probs.astype(np.float64) - conf[:, None].astype(np.float64))
        gap = gap[np.isfinite(gap) & (gap > 0)]
        if gap.size:
            _note(margins, "score", gap.min())
        _conf_margin(margins, conf[cls != 0], thresh)
        candidates = np.nonzero((cls != 0) & (conf > thresh))[0]
        sel = greedy_nms(conf, boxes[b], candidates, iou_threshold, nms_max_output_size, margins)
        rows = np.asarray([[float(cls[i]), float(conf[i])] + [float(v) for v in boxes[b, i]] for i in sel],
                          dtype=np.float64).reshape(-1, 6)
        rows_out[b], index_out[b] = _top_k(rows, np.asarray(sel, dtype=np.int64), top_k, margins)
    return Decoded(rows_out, index_out, margins)


# ---- seeded inputs shared by the CPU and the GPU tests -----------------------------------------------------------------
def ssd_like_predictions(seed, batch=3, n_boxes=2000, n_classes=6, n_objects=80):
    """Seeded SSD-like predictions (float32): softmax-like class rows (most boxes background, up to `n_objects` boxes per image
    confident in one foreground class), offsets ~ N(0, 1), anchors inside the unit square, variances 0.1 / 0.2."""
    rng = np.random.RandomState(seed)
    y = np.zeros((batch, n_boxes, n_classes + 12), dtype=np.float64)
    fg = rng.uniform(0.0, 1.0, size=(batch, n_boxes, n_classes - 1))
    bg = rng.uniform(0.90, 0.99, size=(batch, n_boxes))
    y[..., 0] = bg
    y[..., 1:n_classes] = fg / fg.sum(axis=-1, keepdims=True) * (1.0 - bg)[..., None]
    for b in range(batch):
        n_obj = n_objects * (b + 1) // batch                    # the first images keep fewer rows than top_k
        objs = rng.choice(n_boxes, size=n_obj, replace=False)
        cls = rng.randint(1, n_classes, size=n_obj)
        conf = rng.uniform(0.35, 0.95, size=n_obj)
        rest = rng.uniform(0.2, 1.0, size=(n_obj, n_classes))
        rest[np.arange(n_obj), cls] = 0.0
        rest[:, 0] *= 3.0
        rest = rest / rest.sum(axis=-1, keepdims=True) * (1.0 - conf)[:, None]
        rest[np.arange(n_obj), cls] = conf
        y[b, objs, :n_classes] = rest
    y[..., -12:-8] = rng.normal(0.0, 1.0, size=(batch, n_boxes, 4))
    # anchor centres gather around a few places, as the confident boxes around the objects of a picture do
    places = rng.uniform(0.15, 0.85, size=(batch, 12, 2))
    which = rng.randint(0, 12, size=(batch, n_boxes))
    y[..., -8:-6] = places[np.arange(batch)[:, None], which] + rng.uniform(-0.1, 0.1, size=(batch, n_boxes, 2))
    y[..., -6:-4] = rng.uniform(0.15, 0.45, size=(batch, n_boxes, 2))
    y[..., -4:] = [0.1, 0.1, 0.2, 0.2]
    return y.astype(np.float32)


# seeds of `ssd_like_predictions` whose decision margins are all >= 1e-4 at RANDOM_ARGS, found by running the
# restatement on the host (tests/test_decode_reference_cpu.py asserts it again)
RANDOM_ARGS = dict(confidence_thresh=0.3, iou_threshold=0.45, top_k=40, nms_max_output_size=50, normalize_coords=1,
                   img_height=300, img_width=500)
RANDOM_SEED = {"full": 65, "fast": 214}
MIN_MARGIN = 1e-4
