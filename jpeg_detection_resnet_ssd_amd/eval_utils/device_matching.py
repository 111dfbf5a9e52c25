"""Matching, precision / recall and sampled AP of the Pascal-VOC `Evaluator` on the device (csrc/dj_eval.hip).

`Evaluator.match_predictions` walks every prediction of a class in confidence order, but the greedy matching it performs
is sequential only inside one (class, image) pair: a prediction looks at the ground truth of its own image and class
alone, and the "already detected" marks it sets are read only by later predictions of the same pair.  So the work splits
into independent *segments*, one per (class, image) pair that has predictions, each holding its predictions in rank order.

  pack_evaluation     the Evaluator's python lists -> flat numpy arrays, rank order and segments (host)
  match_packed_host   the segment-wise matching in numpy: the machine-independent twin of dj_eval_match, and the proof
                      on the CPU that the segment-wise formulation equals the global loop
  DeviceEvaluation    upload once, dj_eval_match, dj_eval_precision_recall_ap, download: what
                      `Evaluator(device_matching=True)` runs
  collect_host        a decoded batch -> records (padding mask, inverse transform, decimal rounding) in numpy: the twin of
                      dj_eval_collect (csrc/dj_eval_collect.hip)
  rank_host           records -> the prediction and segment arrays of `pack_evaluation`: the twin of dj_eval_rank
  DeviceCollector     dj_eval_collect per batch, dj_eval_rank once, `DeviceEvaluation.from_device`: what
                      `Evaluator(device_predictions=True)` runs, the detections never leaving the device

Everything the host methods compute in float64 is computed in float64 in the same operation order, and every result is
equal bit for bit to theirs."""
from operator import itemgetter

import numpy as np

from ..bounding_box_utils.bounding_box_utils import _BORDER

MAX_GT_PER_IMAGE = 4096       # DJ_EVAL_MAX_GT of csrc/dj_eval.hip
MAX_RECALL_POINTS = 1024      # DJ_EVAL_MAX_POINTS


class PackedEvaluation(object):
    """Flat arrays of one evaluation (see `pack_evaluation`).

    Predictions of classes 1..n_classes, one class after another, each class in rank order:
      class_offsets [n_classes + 2] int32   class c occupies [class_offsets[c], class_offsets[c + 1])
      pred_class, pred_image [P] int32      class id; position of str(image_id) in data_generator.image_ids
      pred_conf [P] float32, pred_boxes [P][4] float32 (xmin, ymin, xmax, ymax)
    Segments, one per (class, image) pair with at least one prediction, ordered by (class, image):
      seg_class, seg_image [S] int32, seg_offsets [S + 1] int32, seg_ranks [P] int32 (ranks within the class, increasing)
    Ground truth after the `ignore_under_area` filter, image after image:
      gt_offsets [n_images + 1] int32, gt_boxes [G][4] float64, gt_class [G] int32 (-1: no integer class id),
      gt_neutral [G] uint8
    `use_neutral`: neutral boxes are in use (`ignore_neutral_boxes` and the generator has `eval_neutral`)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_pred(self):
        return int(self.class_offsets[-1])

    @property
    def max_gt_per_image(self):
        return int(np.diff(self.gt_offsets).max()) if len(self.gt_offsets) > 1 else 0


def pack_ground_truth(evaluator, ignore_neutral_boxes=True):
    """The ground-truth half of `pack_evaluation`, one short pass per image -> a dict: n_images, use_neutral, image_index
    (str(image_id) -> position in `image_ids`, a repeated id mapping to its last position), gt_offsets, gt_boxes, gt_class,
    gt_neutral as `PackedEvaluation` holds them."""
    gen = evaluator.data_generator
    g = evaluator.gt_format
    n_classes = evaluator.n_classes
    neutral_known = getattr(gen, "eval_neutral", None) is not None
    use_neutral = bool(ignore_neutral_boxes and neutral_known)
    # ---- ground truth, exactly as match_predictions builds its dictionary ----
    image_index = {}
    boxes, classes, neutrals, offsets = [], [], [], [0]
    for i, image_id in enumerate(gen.image_ids):
        labels, keep = evaluator._image_labels(i)
        neutral = np.asarray(gen.eval_neutral[i], dtype=bool) if use_neutral else np.zeros(len(labels), dtype=bool)
        neutral = neutral[:len(labels)][keep] if len(neutral) >= len(labels) else np.zeros(int(keep.sum()), dtype=bool)
        gt = labels[keep]
        image_index[str(image_id)] = i          # a repeated id: the last one wins, as in the host's dictionary
        boxes.append(gt[:, [g["xmin"], g["ymin"], g["xmax"], g["ymax"]]])
        cid = gt[:, g["class_id"]]
        with np.errstate(invalid="ignore"):
            whole = (cid == np.floor(cid)) & (cid >= 1) & (cid <= n_classes)    # `gt[:, class_id] == class_id` can hold
        classes.append(np.where(whole, cid, -1).astype(np.int32))
        neutrals.append(neutral.astype(np.uint8))
        offsets.append(offsets[-1] + len(gt))
    gt_boxes = np.ascontiguousarray(np.concatenate(boxes), dtype=np.float64) if boxes else np.zeros((0, 4))
    return dict(n_images=len(offsets) - 1, use_neutral=use_neutral, image_index=image_index,
                gt_offsets=np.asarray(offsets, dtype=np.int32), gt_boxes=gt_boxes.reshape(-1, 4),
                gt_class=np.concatenate(classes) if classes else np.zeros(0, dtype=np.int32),
                gt_neutral=np.concatenate(neutrals) if neutrals else np.zeros(0, dtype=np.uint8))


def pack_evaluation(evaluator, ignore_neutral_boxes=True):
    """`evaluator.prediction_results` and its generator's `labels` / `eval_neutral` / `image_ids` -> `PackedEvaluation`.

    Confidences and boxes are the float32 values `np.array(..., dtype=np.float32)` produces in `match_predictions`; ground
    truth goes through `Evaluator._image_labels` (the `ignore_under_area` filter) and the neutral flags follow the same
    indexing and the same "`eval_neutral` shorter than the labels -> all False" rule (`pack_ground_truth`).

    The rank order is fixed here: within a class it is `np.argsort(-conf, kind="stable")`, confidence descending and equal
    confidences in list order.  With distinct confidences that is what every `sorting_algorithm` of `match_predictions`
    gives; with ties it is what "mergesort" gives (numpy's "quicksort" leaves the order of ties unspecified).  A NaN
    confidence has no place in that order and raises ValueError."""
    n_classes = evaluator.n_classes
    truth = pack_ground_truth(evaluator, ignore_neutral_boxes)
    n_images, use_neutral, image_index = truth["n_images"], truth["use_neutral"], truth["image_index"]
    gt_offsets, gt_boxes, gt_class, gt_neutral = (truth[k] for k in ("gt_offsets", "gt_boxes", "gt_class", "gt_neutral"))
    # ---- predictions, each class in rank order ----
    class_offsets = np.zeros(n_classes + 2, dtype=np.int64)
    p_class, p_image, p_conf, p_boxes = [], [], [], []
    for class_id in range(1, n_classes + 1):
        preds = evaluator.prediction_results[class_id]
        class_offsets[class_id + 1] = class_offsets[class_id] + len(preds)
        if len(preds) == 0:
            continue
        # the tuples (a million of them on VOC 2007 test) in one pass; element by element the same conversions as
        # `np.array([p[1] for p in preds], dtype=np.float32)` and `np.array([p[2:6] for p in preds], dtype=np.float32)`
        ids = list(map(itemgetter(0), preds))
        flat = np.fromiter((v for p in preds for v in p[1:6]), dtype=np.float32, count=5 * len(preds)).reshape(-1, 5)
        conf, box = np.ascontiguousarray(flat[:, 0]), np.ascontiguousarray(flat[:, 1:])
        if np.isnan(conf).any():
            raise ValueError("class {}: a prediction has a NaN confidence, which has no rank".format(class_id))
        index_of = {raw: image_index[str(raw)] for raw in set(ids)}
        image = np.fromiter(map(index_of.__getitem__, ids), dtype=np.int32, count=len(ids))
        order = np.argsort(-conf, kind="stable")
        p_class.append(np.full(len(preds), class_id, dtype=np.int32))
        p_image.append(image[order])
        p_conf.append(conf[order])
        p_boxes.append(box[order])
    class_offsets[0] = 0
    if class_offsets[-1] >= 2 ** 31:
        raise ValueError("more than 2^31 predictions")
    if p_class:
        pred_class, pred_image = np.concatenate(p_class), np.concatenate(p_image)
        pred_conf, pred_boxes = np.concatenate(p_conf), np.ascontiguousarray(np.concatenate(p_boxes))
    else:
        pred_class, pred_image = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
        pred_conf, pred_boxes = np.zeros(0, dtype=np.float32), np.zeros((0, 4), dtype=np.float32)
    # ---- segments: a stable sort by (class, image) keeps the ranks of every pair increasing ----
    n_pred = len(pred_class)
    key = pred_class.astype(np.int64) * max(n_images, 1) + pred_image
    by_segment = np.argsort(key, kind="stable")
    sorted_key = key[by_segment]
    starts = np.flatnonzero(np.concatenate(([True], sorted_key[1:] != sorted_key[:-1]))) if n_pred else np.zeros(0, dtype=np.int64)
    seg_offsets = np.concatenate((starts, [n_pred])).astype(np.int32)
    seg_class = pred_class[by_segment[starts]] if n_pred else np.zeros(0, dtype=np.int32)
    seg_image = pred_image[by_segment[starts]] if n_pred else np.zeros(0, dtype=np.int32)
    seg_ranks = (by_segment - class_offsets[pred_class[by_segment]]).astype(np.int32) if n_pred else np.zeros(0, dtype=np.int32)
    return PackedEvaluation(n_classes=n_classes, n_images=n_images, use_neutral=use_neutral,
                            class_offsets=class_offsets.astype(np.int32), pred_class=pred_class, pred_image=pred_image,
                            pred_conf=pred_conf, pred_boxes=pred_boxes, seg_class=np.ascontiguousarray(seg_class),
                            seg_image=np.ascontiguousarray(seg_image), seg_offsets=seg_offsets, seg_ranks=seg_ranks,
                            gt_offsets=gt_offsets, gt_boxes=gt_boxes, gt_class=gt_class,
                            gt_neutral=gt_neutral)


def match_packed_host(packed, matching_iou_threshold=0.5, border_pixels="include"):
    """Segment by segment on the packed arrays -> (true_pos, false_pos): lists indexed by class id (entry 0 an empty list,
    as in the Evaluator) of int arrays holding the flags at rank positions.  The numpy statement of dj_eval_match: per
    prediction of a segment, in rank order, IoU in float64 against the image's rows of the class as `iou(...,
    coords='corners', mode='element-wise')` computes it, np.argmax, then the host's decisions line by line."""
    d = float(_BORDER[border_pixels])
    co = packed.class_offsets
    tp, fp = np.zeros(packed.n_pred, dtype=int), np.zeros(packed.n_pred, dtype=int)
    boxes = packed.pred_boxes.astype(float)
    for s in range(len(packed.seg_class)):
        cls, img = int(packed.seg_class[s]), int(packed.seg_image[s])
        g0, g1 = int(packed.gt_offsets[img]), int(packed.gt_offsets[img + 1])
        rows = g0 + np.flatnonzero(packed.gt_class[g0:g1] == cls)
        gt = packed.gt_boxes[rows]
        neutral = packed.gt_neutral[rows].astype(bool)
        taken = np.zeros(len(rows), dtype=bool)
        with np.errstate(divide="ignore", invalid="ignore"):
            a1 = (gt[:, 2] - gt[:, 0] + d) * (gt[:, 3] - gt[:, 1] + d)
            for rank in packed.seg_ranks[packed.seg_offsets[s]:packed.seg_offsets[s + 1]]:
                pos = int(co[cls]) + int(rank)
                if len(rows) == 0:
                    fp[pos] = 1
                    continue
                b = boxes[pos]
                w = np.maximum(0, np.minimum(gt[:, 2], b[2]) - np.maximum(gt[:, 0], b[0]) + 0.0)
                h = np.maximum(0, np.minimum(gt[:, 3], b[3]) - np.maximum(gt[:, 1], b[1]) + 0.0)
                inter = w * h
                a2 = (b[2] - b[0] + d) * (b[3] - b[1] + d)
                overlaps = inter / (a1 + a2 - inter)
                best = int(np.argmax(overlaps))
                if overlaps[best] < matching_iou_threshold:
                    fp[pos] = 1
                elif not (packed.use_neutral and neutral[best]):
                    if not taken[best]:
                        tp[pos] = 1
                        taken[best] = True
                    else:
                        fp[pos] = 1
    split = lambda a: [[]] + [a[co[c]:co[c + 1]] for c in range(1, packed.n_classes + 1)]
    return split(tp), split(fp)


class DeviceEvaluation(object):
    """One evaluation on the device: the packed arrays uploaded once, the flags of dj_eval_match kept there, and
    dj_eval_precision_recall_ap run on them for whichever ground-truth counts and recall thresholds are asked for."""

    def __init__(self, packed=None, device=None):
        import torch
        self.device = torch.device("cuda") if device is None else device
        self.packed = packed
        self.tp = self.fp = self.class_offsets = None
        self.n_classes = packed.n_classes if packed is not None else None
        self._split = None

    @classmethod
    def from_flags(cls, true_positives, false_positives, device=None):
        """Flags an earlier `match_predictions` left on the host (lists indexed by class id) -> a DeviceEvaluation that
        can run the precision / recall / AP kernel on them."""
        import torch
        self = cls(None, device)
        self.n_classes = len(true_positives) - 1
        sizes = [0, 0] + [len(true_positives[c]) for c in range(1, self.n_classes + 1)]
        offsets = np.cumsum(sizes).astype(np.int32)
        cat = lambda lst: np.concatenate([np.asarray(lst[c], dtype=np.int32).reshape(-1) for c in range(1, self.n_classes + 1)]
                                         + [np.zeros(0, dtype=np.int32)])
        self.tp = torch.from_numpy(cat(true_positives)).to(self.device)
        self.fp = torch.from_numpy(cat(false_positives)).to(self.device)
        self._set_offsets(offsets)
        return self

    def _set_offsets(self, offsets):
        import torch
        self._offsets_host = np.asarray(offsets, dtype=np.int32)
        self.class_offsets = torch.from_numpy(self._offsets_host.copy()).to(self.device)
        co = self._offsets_host
        self._split = lambda a: [[]] + [a[co[c]:co[c + 1]] for c in range(1, self.n_classes + 1)]

    def upload(self):
        """The packed arrays as CUDA tensors (`self.dev`), in one place so that it can be timed on its own."""
        import torch
        p = self.packed
        if p.max_gt_per_image > MAX_GT_PER_IMAGE:
            raise ValueError("an image has {} ground-truth boxes, the device path takes at most {}"
                             .format(p.max_gt_per_image, MAX_GT_PER_IMAGE))
        names = ("pred_boxes", "seg_ranks", "seg_offsets", "seg_class", "seg_image", "gt_boxes", "gt_class", "gt_neutral",
                 "gt_offsets")
        self.dev = {n: torch.from_numpy(np.ascontiguousarray(getattr(p, n))).to(self.device, non_blocking=True) for n in names}
        self._set_offsets(p.class_offsets)
        return self.dev

    def match(self, matching_iou_threshold, border_pixels):
        """dj_eval_match -> the int32 flag tensors (kept in `self.tp` / `self.fp`)."""
        import torch
        from .. import kernels
        d = self.dev
        n = self.packed.n_pred
        self.tp = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.fp = torch.zeros(n, dtype=torch.int32, device=self.device)
        if n:
            kernels.eval_match(d["pred_boxes"], d["seg_ranks"], d["seg_offsets"], d["seg_class"], d["seg_image"],
                               self.class_offsets, d["gt_boxes"], d["gt_class"], d["gt_neutral"], d["gt_offsets"],
                               self.packed.max_gt_per_image, self.packed.use_neutral, matching_iou_threshold,
                               _BORDER[border_pixels], self.tp, self.fp)
        return self.tp, self.fp

    def precision_recall_ap(self, num_gt_per_class=None, num_recall_points=11):
        """dj_eval_precision_recall_ap on the flags -> device tensors (cum_tp, cum_fp, precision, recall, ap).
        `num_gt_per_class`: the Evaluator's counts (None: zeros, for a caller that wants the cumulative counts only); the
        thresholds are the doubles `np.linspace(0, 1, num_recall_points, endpoint=True)` holds."""
        import torch
        from .. import kernels
        if not 1 <= num_recall_points <= MAX_RECALL_POINTS:
            raise ValueError("the device path samples 1 to {} recall points, not {}".format(MAX_RECALL_POINTS, num_recall_points))
        n = self.tp.numel()
        counts = np.zeros(self.n_classes + 1) if num_gt_per_class is None else np.asarray(num_gt_per_class, dtype=np.float64)
        num_gt = torch.from_numpy(np.ascontiguousarray(counts)).to(self.device)
        thresholds = torch.from_numpy(np.linspace(0, 1, num_recall_points, endpoint=True)).to(self.device)
        cum_tp = torch.empty(n, dtype=torch.int32, device=self.device)
        cum_fp = torch.empty(n, dtype=torch.int32, device=self.device)
        precision = torch.empty(n, dtype=torch.float64, device=self.device)
        recall = torch.empty(n, dtype=torch.float64, device=self.device)
        ap = torch.zeros(self.n_classes + 1, dtype=torch.float64, device=self.device)
        kernels.eval_precision_recall_ap(self.tp, self.fp, self.class_offsets, num_gt, thresholds, cum_tp, cum_fp, precision,
                                         recall, ap)
        return cum_tp, cum_fp, precision, recall, ap

    def per_class(self, tensor, dtype):
        """A per-prediction device tensor -> the Evaluator's list indexed by class id (entry 0 an empty list)."""
        return self._split(tensor.cpu().numpy().astype(dtype, copy=False))

    @classmethod
    def from_device(cls, ground_truth, ranked, class_offsets_host, device=None):
        """The arrays dj_eval_rank left on the device (`ranked`, already cut to the counts) together with the ground truth
        of `pack_ground_truth` -> a DeviceEvaluation whose `match` and `precision_recall_ap` run on tensors that were never
        on the host.  `max_gt_per_image` and `use_neutral` come from the ground-truth pack."""
        import torch
        n_classes = len(class_offsets_host) - 2
        packed = PackedEvaluation(n_classes=n_classes, n_images=ground_truth["n_images"], use_neutral=ground_truth["use_neutral"],
                                  class_offsets=np.asarray(class_offsets_host, dtype=np.int32),
                                  gt_offsets=ground_truth["gt_offsets"])
        self = cls(packed, device)
        if packed.max_gt_per_image > MAX_GT_PER_IMAGE:
            raise ValueError("an image has {} ground-truth boxes, the device path takes at most {}"
                             .format(packed.max_gt_per_image, MAX_GT_PER_IMAGE))
        self.dev = {n: ranked[n] for n in ("pred_boxes", "seg_ranks", "seg_offsets", "seg_class", "seg_image")}
        for n in ("gt_boxes", "gt_class", "gt_neutral", "gt_offsets"):
            self.dev[n] = torch.from_numpy(np.ascontiguousarray(ground_truth[n])).to(self.device, non_blocking=True)
        self._offsets_host = packed.class_offsets
        self.class_offsets = ranked["class_offsets"]
        co = self._offsets_host
        self._split = lambda a: [[]] + [a[co[c]:co[c + 1]] for c in range(1, self.n_classes + 1)]
        return self


# ---- collecting and ranking the detections (csrc/dj_eval_collect.hip) ----------------------------------------------------------
# What `Evaluator.predict_on_dataset` does to a decoded batch and what the prediction half of `pack_evaluation` does to the
# lists, stated on arrays: `collect_host` / `rank_host` are the machine-independent twins of dj_eval_collect / dj_eval_rank.
DESC_DTYPE = np.dtype([("image_index", np.int32), ("kind", np.int32), ("scale_y", np.float32), ("scale_x", np.float32)])
MAX_CONF_DIGITS = 8           # 10**d * float32 is exact in a double up to here: see `round_decimal`
RECORD_FIELDS = (("rec_class", np.int32), ("rec_image", np.int32), ("rec_ordinal", np.int32), ("rec_conf", np.float32),
                 ("rec_conf64", np.float64), ("rec_boxes", np.float32))
RANKED_FIELDS = ("class_offsets", "pred_class", "pred_image", "pred_conf", "pred_boxes", "seg_class", "seg_image",
                 "seg_offsets", "seg_ranks")


def round_decimal(values, digits):
    """CPython's `round(float(v), digits)` for float32 `values`, `digits` <= 8, as float64: `10**digits * v` is exact in a
    double (24 + 27 bits), `rint` rounds it half-even on the exact value as `round` does, and the one division is correctly
    rounded -- the double nearest to the decimal, which is what `round` returns.  The sign of zero survives."""
    scale = 10.0 ** int(digits)
    return np.rint(np.asarray(values, dtype=np.float32).astype(np.float64) * scale) / scale


def conf_digits_of(round_confidences):
    """`round_confidences` of `predict_on_dataset` -> digits (`True` is `round(x, True)`: 1 digit; 0: not rounded)."""
    digits = int(round_confidences) if round_confidences else 0
    if not 0 <= digits <= MAX_CONF_DIGITS:
        raise ValueError("device_predictions rounds confidences to 1..{} digits, not {}".format(MAX_CONF_DIGITS, digits))
    return digits


def batch_descriptors(image_index, inverse_transforms, n_valid=None):
    """Per-image chains of inverters -> the DESC_DTYPE records dj_eval_collect takes, or None when the chain of one of the
    first `n_valid` images cannot be stated as at most one resize (an inverter without `device_form`, or two resizes):
    that batch takes the fallback."""
    desc = np.zeros(len(image_index), dtype=DESC_DTYPE)
    desc["image_index"] = image_index
    for k in range(len(image_index) if n_valid is None else n_valid):
        chain = inverse_transforms[k] if inverse_transforms is not None else None
        for inverter in (chain or []):
            if inverter is None:
                continue
            form = getattr(inverter, "device_form", None)
            if form is None or form[0] not in ("identity", "resize"):
                return None
            if form[0] == "resize":
                if desc["kind"][k] == 1:
                    return None
                desc["kind"][k] = 1
                desc["scale_y"][k], desc["scale_x"][k] = np.float32(form[1]), np.float32(form[2])
    return desc


def collect_host(batches, n_classes, conf_digits=0):
    """The numpy statement of dj_eval_collect over a whole evaluation.  `batches`: tuples (decoded [B][rows][6] float32,
    n_valid, desc [B] DESC_DTYPE, boxes_final).  -> a dict of the RECORD_FIELDS arrays, `n` records long, and `errors`, the
    number of rows whose class id is no integer in 1..n_classes."""
    parts = {name: [] for name, _ in RECORD_FIELDS}
    errors, ordinal = 0, 0
    for decoded, n_valid, desc, boxes_final in batches:
        d = np.asarray(decoded, dtype=np.float32)[:n_valid]
        rows = d.shape[1]
        cls = d[:, :, 0]
        keep = cls != 0                                     # the host's padding mask: a NaN class id is not padding
        with np.errstate(invalid="ignore"):
            whole = (cls == np.floor(cls)) & (cls >= 1) & (cls <= n_classes)
        errors += int((keep & ~whole).sum())
        keep &= whole
        boxes = d[:, :, 2:6].copy()
        if not boxes_final:
            resize = (desc["kind"][:n_valid] == 1)[:, None, None]
            sy, sx = desc["scale_y"][:n_valid, None], desc["scale_x"][:n_valid, None]
            scaled = boxes.copy()
            with np.errstate(invalid="ignore", over="ignore"):
                scaled[:, :, 1], scaled[:, :, 3] = np.rint(boxes[:, :, 1] * sy), np.rint(boxes[:, :, 3] * sy)   # float32 products
                scaled[:, :, 0], scaled[:, :, 2] = np.rint(boxes[:, :, 0] * sx), np.rint(boxes[:, :, 2] * sx)
                boxes = round_decimal(np.where(resize, scaled, boxes), 1).astype(np.float32)
        conf = d[:, :, 1]
        with np.errstate(invalid="ignore", over="ignore"):
            conf64 = round_decimal(conf, conf_digits) if conf_digits else conf.astype(np.float64)
        parts["rec_class"].append(np.where(keep, cls, 0).astype(np.int32)[keep])
        parts["rec_image"].append(np.broadcast_to(desc["image_index"][:n_valid, None], keep.shape)[keep])
        parts["rec_ordinal"].append(np.broadcast_to(ordinal + np.arange(n_valid, dtype=np.int32)[:, None], keep.shape)[keep])
        parts["rec_conf"].append(conf64.astype(np.float32)[keep] if conf_digits else conf[keep])
        parts["rec_conf64"].append(conf64[keep])
        parts["rec_boxes"].append(boxes[keep])
        ordinal += n_valid
    out = {}
    for name, dtype in RECORD_FIELDS:
        empty = np.zeros((0, 4) if name == "rec_boxes" else 0, dtype=dtype)
        out[name] = np.ascontiguousarray(np.concatenate(parts[name] + [empty]), dtype=dtype)
    out["n"], out["errors"] = len(out["rec_class"]), errors
    return out


def conf_sort_key(conf):
    """float32 confidences -> uint32 keys that ascend as the confidence descends; -0.0 and 0.0 share a key."""
    conf = np.asarray(conf, dtype=np.float32)
    u = np.where(conf == 0, np.float32(0), conf).view(np.uint32)
    u = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return ~u


def rank_host(records, n_classes, n_images):
    """The numpy statement of dj_eval_rank: the records of `collect_host` -> a dict of the prediction and segment arrays of
    `PackedEvaluation` (RANKED_FIELDS), by the same three sorts of unique 64-bit keys.  A NaN confidence raises the
    ValueError of `pack_evaluation`."""
    n = records["n"]
    cls, img, conf = records["rec_class"][:n], records["rec_image"][:n], records["rec_conf"][:n]
    if np.isnan(conf).any():
        raise ValueError("a prediction has a NaN confidence, which has no rank")
    u64 = lambda a: np.asarray(a).astype(np.uint64)
    position = u64(np.arange(n))
    by_conf = np.argsort((u64(conf_sort_key(conf)) << np.uint64(32)) | position)          # record at global rank r
    by_class = np.argsort((u64(cls[by_conf]) << np.uint64(32)) | position)               # global rank at prediction p
    order = by_conf[by_class]
    pred_class, pred_image = cls[order], img[order]
    counts = np.bincount(pred_class, minlength=n_classes + 1)[:n_classes + 1]
    class_offsets = np.concatenate(([0, 0], np.cumsum(counts[1:]))).astype(np.int32)
    seg_key = (u64(pred_class.astype(np.int64) * n_images + pred_image) << np.uint64(32)) | position
    by_segment = np.argsort(seg_key)
    pair = (seg_key[by_segment] >> np.uint64(32)).astype(np.int64)
    starts = np.flatnonzero(np.concatenate(([True], pair[1:] != pair[:-1]))) if n else np.zeros(0, dtype=np.int64)
    return dict(class_offsets=class_offsets, pred_class=pred_class, pred_image=pred_image, pred_conf=conf[order],
                pred_boxes=np.ascontiguousarray(records["rec_boxes"][:n][order]).reshape(-1, 4),
                seg_class=(pair[starts] // max(n_images, 1)).astype(np.int32),
                seg_image=(pair[starts] % max(n_images, 1)).astype(np.int32),
                seg_offsets=np.concatenate((starts, [n])).astype(np.int32),
                seg_ranks=(by_segment - class_offsets[pred_class[by_segment]]).astype(np.int32))


def records_to_lists(records, n_classes, collected_ids, rounded):
    """Records on the host -> what the loop of `predict_on_dataset` builds: per class id the list of (image id as the
    generator gave it, confidence, xmin, ymin, xmax, ymax), the confidence an np.float32 or -- `rounded` -- the python float
    `round` returned, the coordinates python floats.  The coordinates are re-rounded from their float32 form: for |v| < 2^19
    float32(k / 10) lies within 0.05 of k / 10, above that `round(v, 1)` changes no float32 by more than its own spacing."""
    n = records["n"]
    cls = records["rec_class"][:n]
    results = [list() for _ in range(n_classes + 1)]
    for class_id in range(1, n_classes + 1):
        idx = np.flatnonzero(cls == class_id)
        if len(idx) == 0:
            continue
        ids = [collected_ids[o] for o in records["rec_ordinal"][idx].tolist()]
        conf = records["rec_conf64"][idx].tolist() if rounded else list(records["rec_conf"][idx])
        boxes = round_decimal(records["rec_boxes"][idx], 1)
        results[class_id] = list(zip(ids, conf, boxes[:, 0].tolist(), boxes[:, 1].tolist(), boxes[:, 2].tolist(),
                                     boxes[:, 3].tolist()))
    return results


def finish_batch_on_host(y, n_valid, inverse_transforms):
    """The fallback for a batch whose inverse transforms have no device form: the existing host code on the downloaded
    batch `y` ([B][rows][6]) -- padding mask, `apply_inverse_transforms`, `round(float(v), 1)` -- and the finished boxes put
    back into the rows they came from (class id and confidence untouched), for dj_eval_collect to append as final rows."""
    from .average_precision_evaluator import apply_inverse_transforms
    kept = [np.flatnonzero(y[i, :, 0] != 0) for i in range(len(y))]
    done = apply_inverse_transforms([y[i][kept[i]] for i in range(len(y))], inverse_transforms)
    out = np.zeros(y.shape, dtype=np.float32)
    for i in range(n_valid):
        rows = np.asarray(done[i]).reshape(-1, 6)
        out[i, kept[i], :2] = y[i][kept[i], :2]
        if len(rows):
            out[i, kept[i], 2:] = [[round(float(v), 1) for v in row[2:6]] for row in rows]
    return out


class DeviceCollector(object):
    """One evaluation's detections on the device: `add` appends a decoded batch (dj_eval_collect, no synchronisation),
    `rank` runs dj_eval_rank and makes the one small download of the evaluation -- the counters and the class offsets."""

    def __init__(self, n_classes, image_ids, conf_digits=0, device=None):
        import torch
        self.device = torch.device("cuda") if device is None else device
        self.n_classes, self.conf_digits = int(n_classes), int(conf_digits)
        self.n_images = len(image_ids)
        self.image_index = {str(image_id): i for i, image_id in enumerate(image_ids)}      # a repeated id: the last wins
        self.collected_ids = []
        self.records = self.counters = self.ranked = self.counts = None
        self.rows = None

    def _allocate(self, rows):
        import torch
        self.rows = int(rows)
        self.capacity = max(1, self.n_images * self.rows)
        self.records = {name: torch.empty((self.capacity, 4) if name == "rec_boxes" else self.capacity,
                                          dtype=getattr(torch, np.dtype(dtype).name), device=self.device)
                        for name, dtype in RECORD_FIELDS}
        self.counters = torch.zeros(4, dtype=torch.int32, device=self.device)

    def add(self, decoded, n_valid, image_ids, inverse_transforms=None):
        """`decoded`: the [B][rows][6] float32 CUDA tensor of the plan (consumed on the launch stream before the next
        forward pass overwrites it); the first `n_valid` images count.  A batch whose inverse transforms have no device
        form is downloaded, transformed and rounded by the host code and appended as final rows."""
        from .. import kernels
        if self.records is None:
            self._allocate(decoded.shape[1])
        if decoded.shape[1] != self.rows:
            raise ValueError("the decoded batches have {} and {} rows per image".format(self.rows, decoded.shape[1]))
        if len(self.collected_ids) + n_valid > self.n_images:
            raise ValueError("more images collected than the dataset has")
        index = np.zeros(decoded.shape[0], dtype=np.int32)
        index[:n_valid] = [self.image_index[str(i)] for i in image_ids[:n_valid]]
        desc = batch_descriptors(index, inverse_transforms, n_valid)
        final = desc is None
        if final:
            decoded, desc = self._finish_on_host(decoded, n_valid, inverse_transforms), batch_descriptors(index, None)
        kernels.eval_collect(decoded.contiguous(), n_valid, desc, len(self.collected_ids), self.n_classes, self.n_images,
                             self.conf_digits, final, self.records, self.counters)
        self.collected_ids.extend(image_ids[:n_valid])
        self.ranked = None

    def _finish_on_host(self, decoded, n_valid, inverse_transforms):
        import torch
        return torch.from_numpy(finish_batch_on_host(decoded.cpu().numpy(), n_valid, inverse_transforms)).to(self.device)

    def rank(self):
        """-> (ranked device tensors cut to the counts, class offsets on the host); ValueError for a bad class id or a
        NaN confidence."""
        import torch
        from .. import kernels
        if self.ranked is not None:
            return self.ranked
        if self.records is None:
            self._allocate(1)
        cap = self.capacity
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=self.device)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
        out = dict(class_offsets=i32(self.n_classes + 2), pred_class=i32(cap), pred_image=i32(cap), pred_conf=f32(cap),
                   pred_boxes=f32(cap, 4), seg_class=i32(cap), seg_image=i32(cap), seg_offsets=i32(cap + 1), seg_ranks=i32(cap))
        workspace = torch.empty(kernels.eval_rank_workspace_bytes(cap, self.n_classes), dtype=torch.uint8, device=self.device)
        self.counters[2] = 0
        kernels.eval_rank(self.records, self.n_classes, max(1, self.n_images), self.counters, out, workspace)
        small = torch.cat((self.counters, out["class_offsets"])).cpu().numpy()      # the evaluation's one download
        n_pred, errors, n_seg, dropped = (int(v) for v in small[:4])
        if errors or dropped:
            raise ValueError("{} predictions have a class id that is no integer in 1..{} or a NaN confidence, which has no "
                             "rank".format(errors + dropped, self.n_classes))
        self.counts = (n_pred, n_seg)
        cut = {"class_offsets": self.n_classes + 2, "seg_class": n_seg, "seg_image": n_seg, "seg_offsets": n_seg + 1}
        self.ranked = ({k: v[:cut.get(k, n_pred)] for k, v in out.items()}, small[4:].astype(np.int32))
        return self.ranked

    def download_records(self):
        """The records as the dict `collect_host` returns (one download of every array)."""
        if self.records is None:
            self._allocate(1)
        n = int(self.counters[0])
        out = {name: t[:n].cpu().numpy() for name, t in self.records.items()}
        out["n"], out["errors"] = n, int(self.counters[1])
        return out

    def prediction_results(self):
        rec = self.download_records()
        if rec["errors"]:
            raise ValueError("{} predictions have a class id that is no integer in 1..{}".format(rec["errors"], self.n_classes))
        return records_to_lists(rec, self.n_classes, self.collected_ids, self.conf_digits > 0)
