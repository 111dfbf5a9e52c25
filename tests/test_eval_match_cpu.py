"""eval_utils/device_matching.py on the CPU: the packing (rank order, segments, the NaN-confidence error) and
`match_packed_host`, the segment-wise numpy statement of csrc/dj_eval.hip, against `Evaluator.match_predictions`' global
loop over every case of tests/eval_match_cases.py."""
import numpy as np
import pytest

import eval_match_cases as C
from jpeg_detection_resnet_ssd_amd.eval_utils.device_matching import match_packed_host, pack_evaluation


def test_cases_reach_every_outcome():
    counts = C.outcome_counts()
    assert all(counts[k] > 0 for k in C.OUTCOMES), counts


@pytest.mark.parametrize("index", range(len(C.cases())), ids=[c["name"] for c in C.cases()])
def test_segmentwise_matching_equals_the_global_loop(index):
    assert all(C.outcome_counts()[k] > 0 for k in C.OUTCOMES), C.outcome_counts()
    case, host = C.cases()[index], C.host_result(index)
    packed = pack_evaluation(C.make_evaluator(case), case["ignore_neutral_boxes"])
    tp, fp = match_packed_host(packed, case["threshold"], case["border_pixels"])
    assert len(tp) == len(fp) == case["n_classes"] + 1 and len(tp[0]) == len(fp[0]) == 0
    for class_id in range(1, case["n_classes"] + 1):
        np.testing.assert_array_equal(tp[class_id], host.true_positives[class_id])
        np.testing.assert_array_equal(fp[class_id], host.false_positives[class_id])
        assert tp[class_id].dtype == host.true_positives[class_id].dtype
        if "expect_tp" in case:       # the hand-made cases also carry their derived answers
            np.testing.assert_array_equal(tp[class_id], case["expect_tp"][class_id])
            np.testing.assert_array_equal(fp[class_id], case["expect_fp"][class_id])


def test_rank_order_and_segments():
    case = C.cases()[0]
    ev = C.make_evaluator(case)
    p = pack_evaluation(ev, True)
    ids = {name: i for i, name in enumerate(case["image_ids"])}
    assert p.class_offsets.tolist() == [0, 0, len(case["preds"][1]), len(case["preds"][1]) + len(case["preds"][2]),
                                        len(case["preds"][1]) + len(case["preds"][2])]
    for class_id in (1, 2):
        preds = case["preds"][class_id]
        conf = np.array([q[1] for q in preds], dtype=np.float32)
        order = np.argsort(-conf, kind="mergesort")
        sl = slice(p.class_offsets[class_id], p.class_offsets[class_id + 1])
        np.testing.assert_array_equal(p.pred_conf[sl], conf[order])
        np.testing.assert_array_equal(p.pred_boxes[sl], np.array([q[2:6] for q in preds], dtype=np.float32)[order])
        np.testing.assert_array_equal(p.pred_image[sl], [ids[preds[j][0]] for j in order])
        assert (p.pred_class[sl] == class_id).all() and p.pred_conf.dtype == p.pred_boxes.dtype == np.float32
    # every prediction is in exactly one segment, a segment is one (class, image) pair, its ranks increase
    assert p.seg_offsets[0] == 0 and p.seg_offsets[-1] == p.n_pred and (np.diff(p.seg_offsets) > 0).all()
    pairs = list(zip(p.seg_class.tolist(), p.seg_image.tolist()))
    assert len(set(pairs)) == len(pairs) and 3 not in p.seg_class
    seen = np.zeros(p.n_pred, dtype=int)
    for s, (class_id, image) in enumerate(pairs):
        ranks = p.seg_ranks[p.seg_offsets[s]:p.seg_offsets[s + 1]]
        assert (np.diff(ranks) > 0).all()
        pos = p.class_offsets[class_id] + ranks
        assert (p.pred_class[pos] == class_id).all() and (p.pred_image[pos] == image).all()
        seen[pos] += 1
    assert (seen == 1).all() and np.diff(p.seg_offsets).max() >= 260
    # ground truth: float64 rows per image
    assert p.gt_boxes.dtype == np.float64 and p.gt_offsets.tolist() == np.cumsum([0, 0, 70, 5, 66, 12, 3]).tolist()
    assert p.max_gt_per_image == 70 and p.use_neutral
    np.testing.assert_array_equal(p.gt_boxes, np.concatenate(case["labels"])[:, 1:])
    np.testing.assert_array_equal(p.gt_class, np.concatenate(case["labels"])[:, 0])
    for i in range(6):
        np.testing.assert_array_equal(p.gt_neutral[p.gt_offsets[i]:p.gt_offsets[i + 1]], case["eval_neutral"][i])
    assert p.gt_neutral.any()
    # a neutral list shorter than the image's labels counts as all False (image 4 of the second case)
    short = C.cases()[1]
    assert len(short["eval_neutral"][4]) < len(short["labels"][4]) and short["eval_neutral"][4].any()
    q = pack_evaluation(C.make_evaluator(short), True)
    assert not q.gt_neutral[q.gt_offsets[4]:q.gt_offsets[5]].any() and q.gt_neutral[:q.gt_offsets[4]].any()


def test_equal_confidences_keep_list_order():
    case = C.cases()[5]
    p = pack_evaluation(C.make_evaluator(case), True)
    sl = slice(p.class_offsets[2], p.class_offsets[3])
    np.testing.assert_array_equal(p.pred_boxes[sl][:, 0], [21.0, 20.0, 1.0])


def test_area_filter_and_neutral_switch():
    case = C.cases()[3]
    p = pack_evaluation(C.make_evaluator(case), True)
    kept = [(l[:, 4] - l[:, 2]) * (l[:, 3] - l[:, 1]) >= 600 for l in case["labels"]]
    assert p.gt_offsets.tolist() == np.cumsum([0] + [int(k.sum()) for k in kept]).tolist() and 0 < p.gt_offsets[-1] < 156
    np.testing.assert_array_equal(p.gt_neutral[p.gt_offsets[1]:p.gt_offsets[2]], case["eval_neutral"][1][kept[1]])
    assert not pack_evaluation(C.make_evaluator(case), False).gt_neutral.any()


def test_a_class_spans_several_scan_chunks():
    p = pack_evaluation(C.make_evaluator(C.cases()[7]), True)
    assert min(np.diff(p.class_offsets)[1:3]) > 2048


def test_nan_confidence_is_an_error():
    case = dict(C.cases()[5])
    case["preds"] = [[], list(case["preds"][1]) + [("img0", float("nan"), 0.0, 0.0, 1.0, 1.0)], case["preds"][2]]
    with pytest.raises(ValueError, match="NaN"):
        pack_evaluation(C.make_evaluator(case), True)
