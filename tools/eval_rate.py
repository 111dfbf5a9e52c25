"""Cost of the Pascal-VOC matching / precision-recall / AP stages of the `Evaluator` on a synthetic dataset of VOC-2007-test
proportions (4952 images, 20 classes, a few ground-truth boxes per image, about 200 detections per image), host path vs
device path:

  (a) host:   Evaluator.match_predictions (numpy, one Python iteration per prediction; `--host-reps` runs, it takes the
              better part of a minute), compute_precision_recall, compute_average_precisions, and their sum
  (b) device: Evaluator(device_matching=True), the same three calls, and split into
              packing (python lists -> flat arrays, rank order, segments; host), upload, dj_eval_match and
              dj_eval_precision_recall_ap (by device events), download of every result array
  (c) collection, from the decoded [B][detections][6] batches as the DecodeDetections layer leaves them on the GPU to the
      arrays dj_eval_match reads, on the same detections with a `Resize` inverter per image:
      host:   per batch download, padding mask, apply_inverse_transforms, the per-box loop; then pack_evaluation and upload
              (`--host-reps` runs)
      device: Evaluator(device_predictions=True)'s path: dj_eval_collect per batch, then dj_eval_rank with its one small
              download

    python tools/eval_rate.py [--images 4952] [--detections 200] [--reps 5] [--host-reps 1] [--batch-size 8]

Medians over the repetitions after warm-up; every timed window ends in a device synchronise.  The results of the two
paths are compared for equality.  Prints one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from jpeg_detection_resnet_ssd_amd.eval_utils.average_precision_evaluator import (Evaluator, append_batch_results,
                                                                                 apply_inverse_transforms)
from jpeg_detection_resnet_ssd_amd.eval_utils.device_matching import (RANKED_FIELDS, DeviceCollector, DeviceEvaluation,
                                                                      pack_evaluation)


def median_ms(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def event_ms(fn, reps):
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


class Dataset(object):
    def __init__(self, labels, neutral):
        self.labels, self.eval_neutral = labels, neutral
        self.image_ids = ["%06d" % i for i in range(len(labels))]

    def get_dataset_size(self):
        return len(self.labels)


def make_dataset(rng, n_images, n_classes, detections):
    """Per image 1 + Poisson(1.5) objects on a 500 x 375 canvas, an eighth of them 'difficult'; detections are jittered
    copies of the objects (some repeated) filled up to `detections` with boxes anywhere, classes drawn at random, the
    confidence of a good detection high and the others' skewed towards the 0.01 cut-off, as an SSD's top-200 are."""
    labels, neutral = [], []
    decoded = np.zeros((n_images, detections, 6), dtype=np.float32)    # the same detections as a decoded tensor
    results = [list() for _ in range(n_classes + 1)]
    for i in range(n_images):
        n = 1 + int(rng.poisson(1.5))
        w, h = rng.uniform(30, 300, n), rng.uniform(30, 250, n)
        x0, y0 = rng.uniform(0, 500 - w), rng.uniform(0, 375 - h)
        cls = rng.integers(1, n_classes + 1, n)
        labels.append(np.round(np.stack([cls, x0, y0, x0 + w, y0 + h], axis=1)))
        neutral.append(rng.random(n) < 0.125)
        image_id = "%06d" % i
        m = detections
        src = rng.integers(0, n, m)
        good = rng.random(m) < 0.03 * n
        boxes = labels[-1][src, 1:] + rng.normal(0, 6, (m, 4))
        rw, rh = rng.uniform(10, 300, m), rng.uniform(10, 250, m)
        rx, ry = rng.uniform(0, 500 - rw), rng.uniform(0, 375 - rh)
        boxes = np.where(good[:, None], boxes, np.stack([rx, ry, rx + rw, ry + rh], axis=1))
        pcls = np.where(good, cls[src], rng.integers(1, n_classes + 1, m))
        conf = np.where(good, rng.uniform(0.3, 1.0, m), 0.01 + 0.5 * rng.random(m) ** 4).astype(np.float32)
        decoded[i, :, 0], decoded[i, :, 1], decoded[i, :, 2:] = pcls, conf, boxes
        for k in range(m):
            results[int(pcls[k])].append((image_id, conf[k], round(float(boxes[k, 0]), 1), round(float(boxes[k, 1]), 1),
                                          round(float(boxes[k, 2]), 1), round(float(boxes[k, 3]), 1)))
    return Dataset(labels, neutral), results, decoded


def collection_stage(args, data, decoded, res):
    """(c): both paths start from the decoded batches resident on the GPU and end with the matching's inputs there."""
    from jpeg_detection_resnet_ssd_amd.data.ssd_augment import Resize
    inverter = Resize(300, 300)(np.zeros((375, 500, 3), dtype=np.uint8), return_inverter=True)[1]
    pred_format = {"class_id": 0, "conf": 1, "xmin": 2, "ymin": 3, "xmax": 4, "ymax": 5}
    n, ids = len(decoded), data.image_ids
    batches = [torch.from_numpy(decoded[i:i + args.batch_size]).cuda() for i in range(0, n, args.batch_size)]
    out = {}

    def host_path():
        results, seen = [list() for _ in range(args.classes + 1)], 0
        for t in batches:
            y = t.cpu().numpy()
            y_pred = [y[i][y[i, :, 0] != 0] for i in range(len(y))]
            y_pred = apply_inverse_transforms(y_pred, [[inverter]] * len(y))
            append_batch_results(results, y_pred, ids[seen:seen + len(y)], seen, n, False, pred_format)
            seen += len(y)
        out["lists_s"] = time.perf_counter()
        ev = Evaluator(model=None, n_classes=args.classes, data_generator=data)
        ev.prediction_results = results
        out["packed"] = pack_evaluation(ev, True)
        DeviceEvaluation(out["packed"]).upload()

    def collect():
        c, seen = DeviceCollector(args.classes, ids, 0), 0
        for t in batches:
            c.add(t, len(t), ids[seen:seen + len(t)], [[inverter]] * len(t))
            seen += len(t)
        out["collector"] = c

    def rank():
        out["collector"].ranked = None
        out["collector"].rank()

    def device_path():
        collect()
        rank()

    res["batches"] = len(batches)
    res["device_collect_rank_ms"] = median_ms(device_path, args.reps)
    res["device_collect_ms"] = median_ms(collect, args.reps)
    res["device_rank_ms"] = median_ms(rank, args.reps)
    t0 = time.perf_counter()
    res["host_collect_pack_upload_ms"] = median_ms(host_path, args.host_reps, warmup=0)
    res["host_lists_ms"] = (out["lists_s"] - t0) * 1e3 if args.host_reps == 1 else None
    res["host_over_device_collection"] = res["host_collect_pack_upload_ms"][0] / res["device_collect_rank_ms"][0]
    ranked = out["collector"].rank()[0]
    same = True
    for name in RANKED_FIELDS:
        a, b = ranked[name].cpu().numpy(), getattr(out["packed"], name)
        bits = lambda v: np.ascontiguousarray(v).view(np.uint32) if v.dtype == np.float32 else v
        same = same and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))
    res["device_collection_equals_host"] = bool(same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4952)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--detections", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--batch-size", type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "eval_rate.py measures on the GPU"
    rng = np.random.default_rng(0)
    data, results, decoded = make_dataset(rng, args.images, args.classes, args.detections)
    settings = dict(ignore_neutral_boxes=True, matching_iou_threshold=0.5, border_pixels="include",
                    sorting_algorithm="mergesort", verbose=False)

    def evaluator(device):
        ev = Evaluator(model=None, n_classes=args.classes, data_generator=data, device_matching=device)
        ev.prediction_results = results
        ev.get_num_gt_per_class(ignore_neutral_boxes=True, verbose=False)
        return ev

    def stages(ev):
        ev.match_predictions(**settings)
        ev.compute_precision_recall(verbose=False)
        ev.compute_average_precisions(mode="sample", num_recall_points=11, verbose=False)

    res = {"images": args.images, "classes": args.classes, "predictions": sum(len(r) for r in results),
           "ground_truth": int(sum(len(l) for l in data.labels)), "reps": args.reps, "host_reps": args.host_reps}
    # (b) device path first: its warm-up also loads the library
    dev_ev = evaluator(True)
    res["device_ms"] = median_ms(lambda: stages(dev_ev), args.reps)
    res["pack_ms"] = median_ms(lambda: pack_evaluation(dev_ev, True), args.reps)
    packed = pack_evaluation(dev_ev, True)
    res["segments"] = int(len(packed.seg_class))
    res["upload_MB"] = sum(getattr(packed, n).nbytes for n in ("pred_boxes", "seg_ranks", "seg_offsets", "seg_class",
                                                               "seg_image", "gt_boxes", "gt_class", "gt_neutral",
                                                               "gt_offsets", "class_offsets")) / 1e6
    de = DeviceEvaluation(packed)
    res["upload_ms"] = median_ms(de.upload, args.reps)
    reps = max(20, args.reps)
    res["eval_match_ms"] = event_ms(lambda: de.match(0.5, "include"), reps)
    res["eval_precision_recall_ap_ms"] = event_ms(lambda: de.precision_recall_ap(dev_ev.num_gt_per_class, 11), reps)
    outs = de.precision_recall_ap(dev_ev.num_gt_per_class, 11)

    def download():
        for t in (de.tp, de.fp) + tuple(outs[:2]):
            de.per_class(t, int)
        for t in outs[2:4]:
            de.per_class(t, float)
        outs[4].cpu()
    res["download_ms"] = median_ms(download, args.reps)
    res["download_MB"] = (4 * 4 + 2 * 8) * packed.n_pred / 1e6
    # (a) host path
    host_ev = evaluator(False)
    res["host_match_ms"] = median_ms(lambda: host_ev.match_predictions(**settings), args.host_reps, warmup=0)
    res["host_precision_recall_ms"] = median_ms(lambda: host_ev.compute_precision_recall(verbose=False), args.reps)
    res["host_average_precisions_ms"] = median_ms(lambda: host_ev.compute_average_precisions(verbose=False), args.reps)
    res["host_ms"] = sum(res[k][0] for k in ("host_match_ms", "host_precision_recall_ms", "host_average_precisions_ms"))
    res["host_over_device"] = res["host_ms"] / res["device_ms"][0]
    same = host_ev.average_precisions == dev_ev.average_precisions
    for name in ("true_positives", "false_positives", "cumulative_true_positives", "cumulative_false_positives",
                 "cumulative_precisions", "cumulative_recalls"):
        for c in range(1, args.classes + 1):
            same = same and np.array_equal(getattr(host_ev, name)[c], getattr(dev_ev, name)[c], equal_nan=True)
    res["device_equals_host"] = bool(same)
    res["mAP"] = float(np.average(dev_ev.average_precisions[1:]))
    collection_stage(args, data, decoded, res)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
