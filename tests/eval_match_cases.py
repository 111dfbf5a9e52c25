"""Evaluation cases shared by tests/test_eval_match_cpu.py and tests/test_eval_match_gpu.py: seeded random datasets that
reach every path of the matching (more than 64 ground-truth rows in an image, an image without ground truth, a class
without predictions, neutral boxes, a neutral list shorter than its labels, the area filter, all three border rules) and
hand-made ones for the decisions that ties and special values settle.  The host `Evaluator` is the reference; its results
are computed once per case and shared."""
import functools

import numpy as np

from jpeg_detection_resnet_ssd_amd.bounding_box_utils.bounding_box_utils import iou
from jpeg_detection_resnet_ssd_amd.eval_utils.average_precision_evaluator import Evaluator

OUTCOMES = ("tp", "low_iou_fp", "duplicate_fp", "no_gt_fp", "neutral_ignored")


class FakeData(object):
    def __init__(self, labels, image_ids, eval_neutral=None):
        self.labels = labels
        self.image_ids = image_ids
        self.eval_neutral = eval_neutral

    def get_dataset_size(self):
        return len(self.labels)


def _random_case(seed, border_pixels, ignore_under_area=0, ignore_neutral_boxes=True, short_neutral=False, fill=0):
    """3 classes, 6 images with 0 / 70 / 5 / 66 / 12 / 3 ground-truth rows; class 3 has no predictions; (class 1, image 1)
    has 260 predictions.  `short_neutral`: image 4's neutral list is shorter than its labels, which `match_predictions`
    reads as "no neutral box in this image" and `get_num_gt_per_class` cannot index: such a case counts without neutrals.
    `fill`: that many more random detections per (class, image) pair; with 400 a class has more than 2048 predictions, so
    the scan of dj_eval_precision_recall_ap (1024 ranks per chunk) carries its counts over two chunk boundaries."""
    rng = np.random.default_rng(seed)
    n_classes, counts = 3, [0, 70, 5, 66, 12, 3]
    image_ids = ["img%d" % i for i in range(len(counts))]
    labels, neutral = [], []
    for n in counts:
        x0, y0 = rng.integers(0, 250, n), rng.integers(0, 250, n)
        w, h = rng.integers(5, 60, n), rng.integers(5, 60, n)
        labels.append(np.stack([rng.integers(1, n_classes + 1, n), x0, y0, x0 + w, y0 + h], axis=1).astype(float).reshape(-1, 5))
        neutral.append(rng.random(n) < 0.2)
    if short_neutral:
        neutral[4] = neutral[4][:-2]
    preds = [[] for _ in range(n_classes + 1)]
    for class_id in (1, 2):
        for i, image_id in enumerate(image_ids):
            gt = labels[i][labels[i][:, 0] == class_id][:, 1:]
            target = 260 if (class_id, i) == (1, 1) else 12 + 3 * i + fill
            boxes = []
            for row in gt:                      # jittered copies of the ground truth: matches, near misses, duplicates
                for _ in range(int(rng.integers(0, 4))):
                    boxes.append(row + rng.normal(0, rng.choice([0.5, 3.0, 12.0]), 4))
            while len(boxes) < target:          # and boxes anywhere
                x0, y0 = rng.uniform(0, 280, 2)
                boxes.append(np.array([x0, y0, x0 + rng.uniform(4, 70), y0 + rng.uniform(4, 70)]))
            for b in boxes:
                preds[class_id].append((image_id, 0.0) + tuple(round(float(v), 1) for v in b))
    total = sum(len(p) for p in preds)
    conf = (rng.permutation(total) + 1.0) / (total + 1.0)      # distinct, also as float32
    k = 0
    for class_id in (1, 2):
        order = rng.permutation(len(preds[class_id]))          # list order is not rank order
        preds[class_id] = [preds[class_id][j] for j in order]
        for j, p in enumerate(preds[class_id]):
            preds[class_id][j] = (p[0], float(conf[k])) + p[2:]
            k += 1
    return dict(name="random-%d-%s-area%d-neutral%d-fill%d" % (seed, border_pixels, ignore_under_area, ignore_neutral_boxes, fill),
                n_classes=n_classes, labels=labels, image_ids=image_ids, eval_neutral=neutral, preds=preds,
                ignore_under_area=ignore_under_area, ignore_neutral_boxes=ignore_neutral_boxes,
                count_ignore_neutral=ignore_neutral_boxes and not short_neutral, threshold=0.5, border_pixels=border_pixels)


def _hand_ties():
    """'include' borders, threshold = the IoU of (0,0,9,9) and (0,0,9,4), 36/114 as iou() rounds it.
    Class 1, img0: two identical boxes A, A' and a box B.  Detections on A: the first takes A (np.argmax: first index), the
      second finds A again -> duplicate, never A'.  Detections on B: IoU == threshold -> match; one just below -> FP.
    Class 2, img1: two detections of equal confidence on one box: list order decides, the first is the TP."""
    thr = float(iou(np.array([0., 0, 9, 9]), np.array([0., 0, 9, 4]), coords="corners", mode="element-wise",
                    border_pixels="include")[0])
    labels = [np.array([[1., 100, 100, 150, 150], [1, 100, 100, 150, 150], [1, 0, 0, 9, 9]]),
              np.array([[2., 20, 20, 80, 80], [1, 200, 200, 240, 240]])]
    c1 = [("img0", 0.9, 100.0, 100.0, 150.0, 150.0), ("img0", 0.8, 100.0, 100.0, 150.0, 150.0),
          ("img0", 0.7, 0.0, 0.0, 9.0, 4.0), ("img0", 0.6, 0.0, 0.0, 9.0, 3.0), ("img1", 0.5, 201.0, 200.0, 240.0, 240.0)]
    c2 = [("img1", 0.75, 21.0, 20.0, 80.0, 80.0), ("img1", 0.75, 20.0, 20.0, 80.0, 80.0), ("img0", 0.75, 1.0, 1.0, 5.0, 5.0)]
    return dict(name="hand-ties", n_classes=2, labels=labels, image_ids=["img0", "img1"], eval_neutral=None,
                preds=[[], c1, c2], ignore_under_area=0, ignore_neutral_boxes=True, count_ignore_neutral=True, threshold=thr,
                border_pixels="include", expect_tp={1: [1, 0, 1, 0, 1], 2: [1, 0, 0]}, expect_fp={1: [0, 1, 0, 1, 0], 2: [0, 1, 1]})


def _hand_nan():
    """'half' borders.  Class 1: a zero-area box and a zero-area detection at the same point: 0/0 = NaN, which np.argmax
    prefers to the 0.0 of the ordinary box before it and which is not `<` the threshold -> TP; the same again -> duplicate.
    Class 2 has detections but no ground truth anywhere: recall 0/0.  Both boxes of class 1 are neutral and the counts
    leave them out, while the matching runs without neutral boxes and awards true positives on them: recall x/0."""
    labels = [np.array([[1., 0, 0, 10, 10], [1, 5, 5, 5, 5]]), np.zeros((0, 5))]
    c1 = [("img0", 0.9, 5.0, 5.0, 5.0, 5.0), ("img0", 0.8, 5.0, 5.0, 5.0, 5.0), ("img0", 0.7, 0.0, 0.0, 10.0, 10.0),
          ("img1", 0.6, 0.0, 0.0, 10.0, 10.0)]
    c2 = [("img0", 0.5, 0.0, 0.0, 10.0, 10.0), ("img1", 0.4, 0.0, 0.0, 10.0, 10.0)]
    return dict(name="hand-nan", n_classes=2, labels=labels, image_ids=["img0", "img1"],
                eval_neutral=[np.array([True, True]), np.zeros(0, dtype=bool)], preds=[[], c1, c2], ignore_under_area=0,
                ignore_neutral_boxes=False, count_ignore_neutral=True, threshold=0.5, border_pixels="half",
                expect_tp={1: [1, 0, 1, 0], 2: [0, 0]}, expect_fp={1: [0, 1, 0, 1], 2: [1, 1]})


@functools.lru_cache(maxsize=None)
def cases():
    return (_random_case(11, "include"), _random_case(12, "half", short_neutral=True), _random_case(13, "exclude"),
            _random_case(14, "include", ignore_under_area=600), _random_case(15, "half", ignore_neutral_boxes=False),
            _hand_ties(), _hand_nan(), _random_case(16, "include", fill=400))


def make_evaluator(case, device_matching=None):
    kw = {} if device_matching is None else {"device_matching": device_matching}
    ev = Evaluator(model=None, n_classes=case["n_classes"],
                   data_generator=FakeData(case["labels"], case["image_ids"], case["eval_neutral"]), model_mode="inference",
                   ignore_under_area=case["ignore_under_area"], **kw)
    ev.prediction_results = [list(p) for p in case["preds"]]
    return ev


def run(ev, case, mode="sample", num_recall_points=11):
    """The stages after `predict_on_dataset`, called one by one as `__call__` does."""
    with np.errstate(invalid="ignore", divide="ignore"):      # the host's iou() divides 0 by 0 in the NaN case
        return _run(ev, case, mode, num_recall_points)


def _run(ev, case, mode, num_recall_points):
    ev.get_num_gt_per_class(ignore_neutral_boxes=case["count_ignore_neutral"], verbose=False)
    ev.match_predictions(ignore_neutral_boxes=case["ignore_neutral_boxes"], matching_iou_threshold=case["threshold"],
                         border_pixels=case["border_pixels"], sorting_algorithm="mergesort", verbose=False)
    ev.compute_precision_recall(verbose=False)
    ev.compute_average_precisions(mode=mode, num_recall_points=num_recall_points, verbose=False)
    ev.compute_mean_average_precision()
    return ev


@functools.lru_cache(maxsize=None)
def host_result(index, mode="sample", num_recall_points=11):
    """The host Evaluator's results for case `index` (computed once; do not modify)."""
    return run(make_evaluator(cases()[index]), cases()[index], mode, num_recall_points)


@functools.lru_cache(maxsize=None)
def outcome_counts():
    """How often each outcome occurs over all cases, read off the host's flags: a prediction without either flag matched a
    neutral box; a false positive is 'no ground truth' when its image has no row of the class, 'low IoU' when its best
    overlap is below the threshold, a duplicate otherwise."""
    counts = dict.fromkeys(OUTCOMES, 0)
    for index, case in enumerate(cases()):
        ev = host_result(index)
        where = {str(i): k for k, i in enumerate(case["image_ids"])}
        for class_id in range(1, case["n_classes"] + 1):
            preds = case["preds"][class_id]
            if not preds:
                continue
            order = np.argsort(-np.array([p[1] for p in preds], dtype=np.float32), kind="stable")
            for rank, idx in enumerate(order):
                tp, fp = ev.true_positives[class_id][rank], ev.false_positives[class_id][rank]
                if tp:
                    counts["tp"] += 1
                elif not fp:
                    counts["neutral_ignored"] += 1
                else:
                    labels, keep = ev._image_labels(where[str(preds[idx][0])])
                    gt = labels[keep]
                    gt = gt[gt[:, 0] == class_id]
                    if len(gt) == 0:
                        counts["no_gt_fp"] += 1
                        continue
                    box = np.array(preds[idx][2:6], dtype=np.float32).astype(float)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        overlaps = iou(gt[:, 1:], box, coords="corners", mode="element-wise", border_pixels=case["border_pixels"])
                    low = overlaps[int(np.argmax(overlaps))] < case["threshold"]
                    counts["low_iou_fp" if low else "duplicate_fp"] += 1
    return counts


# the hand-derived cases of tests/test_evaluator_cpu.py, with their known answers
def textbook_case():
    labels = [np.array([[1, 10, 10, 50, 50], [1, 100, 100, 160, 160]]), np.array([[1, 20, 20, 80, 80], [2, 0, 0, 30, 30]])]
    c1 = [("img0", 0.95, 10, 10, 50, 50), ("img1", 0.90, 200, 200, 250, 250), ("img0", 0.80, 101, 101, 160, 160),
          ("img0", 0.70, 12, 12, 50, 50), ("img1", 0.60, 20, 22, 80, 80)]
    return dict(name="textbook", n_classes=2, labels=labels, image_ids=["img0", "img1"], eval_neutral=None, preds=[[], c1, []],
                ignore_under_area=0, ignore_neutral_boxes=True, count_ignore_neutral=True, threshold=0.5,
                border_pixels="include")


def neutral_edge_case():
    thr = float(iou(np.array([0., 0, 9, 9]), np.array([0., 0, 9, 4]), coords="corners", mode="element-wise",
                    border_pixels="include")[0])
    labels = [np.array([[1, 0, 0, 9, 9], [1, 50, 50, 99, 99]])]
    preds = [("img0", 0.9, 50, 50, 99, 99), ("img0", 0.8, 0, 0, 9, 4), ("img0", 0.7, 0, 0, 9, 3)]
    return dict(name="neutral-edge", n_classes=1, labels=labels, image_ids=["img0"], eval_neutral=[np.array([False, True])],
                preds=[[], preds], ignore_under_area=0, ignore_neutral_boxes=True, count_ignore_neutral=True, threshold=thr,
                border_pixels="include")
