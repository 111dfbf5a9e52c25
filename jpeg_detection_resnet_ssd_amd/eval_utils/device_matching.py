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


def pack_evaluation(evaluator, ignore_neutral_boxes=True):
    """`evaluator.prediction_results` and its generator's `labels` / `eval_neutral` / `image_ids` -> `PackedEvaluation`.

    Confidences and boxes are the float32 values `np.array(..., dtype=np.float32)` produces in `match_predictions`; ground
    truth goes through `Evaluator._image_labels` (the `ignore_under_area` filter) and the neutral flags follow the same
    indexing and the same "`eval_neutral` shorter than the labels -> all False" rule.

    The rank order is fixed here: within a class it is `np.argsort(-conf, kind="stable")`, confidence descending and equal
    confidences in list order.  With distinct confidences that is what every `sorting_algorithm` of `match_predictions`
    gives; with ties it is what "mergesort" gives (numpy's "quicksort" leaves the order of ties unspecified).  A NaN
    confidence has no place in that order and raises ValueError."""
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
    n_images = len(offsets) - 1
    gt_boxes = np.ascontiguousarray(np.concatenate(boxes), dtype=np.float64) if boxes else np.zeros((0, 4))
    gt_boxes = gt_boxes.reshape(-1, 4)
    gt_class = np.concatenate(classes) if classes else np.zeros(0, dtype=np.int32)
    gt_neutral = np.concatenate(neutrals) if neutrals else np.zeros(0, dtype=np.uint8)
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
                            gt_offsets=np.asarray(offsets, dtype=np.int32), gt_boxes=gt_boxes, gt_class=gt_class,
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
