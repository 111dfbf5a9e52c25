"""GPU: `Evaluator(device_matching=True)` (csrc/dj_eval.hip: dj_eval_match, dj_eval_precision_recall_ap) against the host
`Evaluator` on every case of tests/eval_match_cases.py: every result attribute equal element for element, bit for bit."""
import numpy as np
import pytest

import eval_match_cases as C
from jpeg_detection_resnet_ssd_amd.eval_utils.average_precision_evaluator import Evaluator

pytestmark = pytest.mark.gpu

PER_CLASS = ("true_positives", "false_positives", "cumulative_true_positives", "cumulative_false_positives",
             "cumulative_precisions", "cumulative_recalls")


def assert_same_results(dev, host, n_classes):
    for name in PER_CLASS:
        a, b = getattr(dev, name), getattr(host, name)
        assert len(a) == len(b) == n_classes + 1 and len(a[0]) == 0
        for class_id in range(1, n_classes + 1):
            np.testing.assert_array_equal(a[class_id], b[class_id], err_msg="%s[%d]" % (name, class_id))
            assert a[class_id].dtype == b[class_id].dtype and a[class_id].shape == b[class_id].shape, (name, class_id)
    assert len(dev.average_precisions) == n_classes + 1
    for class_id in range(n_classes + 1):
        assert dev.average_precisions[class_id] == host.average_precisions[class_id], class_id
        assert type(dev.average_precisions[class_id]) is type(host.average_precisions[class_id])
    assert dev.mean_average_precision == host.mean_average_precision
    np.testing.assert_array_equal(dev.num_gt_per_class, host.num_gt_per_class)


@pytest.mark.parametrize("mode,points", [("sample", 11), ("sample", 101), ("integrate", 11)])
@pytest.mark.parametrize("index", range(len(C.cases())), ids=[c["name"] for c in C.cases()])
def test_device_evaluator_equals_host(cuda, index, mode, points):
    assert all(C.outcome_counts()[k] > 0 for k in C.OUTCOMES), C.outcome_counts()
    case = C.cases()[index]
    host = C.host_result(index, mode, points)
    dev = C.run(C.make_evaluator(case, device_matching=True), case, mode, points)
    assert_same_results(dev, host, case["n_classes"])
    if "expect_tp" in case:
        for class_id in range(1, case["n_classes"] + 1):
            np.testing.assert_array_equal(dev.true_positives[class_id], case["expect_tp"][class_id])
            np.testing.assert_array_equal(dev.false_positives[class_id], case["expect_fp"][class_id])


def test_stages_need_their_predecessors_and_accept_host_flags(cuda):
    case = C.cases()[0]
    ev = C.make_evaluator(case, device_matching=True)
    with pytest.raises(ValueError, match="match_predictions"):
        ev.compute_precision_recall(verbose=False)
    with pytest.raises(ValueError, match="compute_precision_recall"):
        ev.compute_average_precisions(verbose=False)
    ev.prediction_results = None
    with pytest.raises(ValueError, match="predict_on_dataset"):
        ev.match_predictions(verbose=False)
    # flags matched on the host, curves and AP on the device
    host = C.host_result(0)
    mixed = C.make_evaluator(case)
    mixed.get_num_gt_per_class(ignore_neutral_boxes=True, verbose=False)
    mixed.match_predictions(ignore_neutral_boxes=True, matching_iou_threshold=0.5, border_pixels="include",
                            sorting_algorithm="mergesort", verbose=False)
    mixed.device_matching = True
    mixed.compute_precision_recall(verbose=False)
    mixed.compute_average_precisions(verbose=False)
    mixed.compute_mean_average_precision()
    assert_same_results(mixed, host, case["n_classes"])


def test_textbook_curve_on_the_device(cuda):
    """tests/test_evaluator_cpu.py:test_textbook_precision_recall_curve through the device path."""
    case = C.textbook_case()
    ev = C.run(C.make_evaluator(case, device_matching=True), case)
    np.testing.assert_array_equal(ev.true_positives[1], [1, 0, 1, 0, 1])
    np.testing.assert_array_equal(ev.false_positives[1], [0, 1, 0, 1, 0])
    np.testing.assert_array_equal(ev.cumulative_true_positives[1], [1, 1, 2, 2, 3])
    np.testing.assert_array_equal(ev.cumulative_false_positives[1], [0, 1, 1, 2, 2])
    np.testing.assert_allclose(ev.cumulative_precisions[1], [1, 1 / 2, 2 / 3, 2 / 4, 3 / 5])
    np.testing.assert_allclose(ev.cumulative_recalls[1], [1 / 3, 1 / 3, 2 / 3, 2 / 3, 1])
    ap_sample = (4 * 1.0 + 3 * (2 / 3) + 4 * (3 / 5)) / 11
    np.testing.assert_allclose(ev.average_precisions[1], ap_sample)
    assert ev.average_precisions[2] == 0.0 and list(ev.num_gt_per_class) == [0, 3, 1]
    assert len(ev.true_positives[2]) == len(ev.cumulative_true_positives[2]) == len(ev.cumulative_recalls[2]) == 0
    np.testing.assert_allclose(ev.mean_average_precision, ap_sample / 2)
    C.run(ev, case, mode="integrate")
    np.testing.assert_allclose(ev.average_precisions[1], 1.0 * (1 / 3) + (2 / 3) * (1 / 3))


def test_neutral_boxes_and_threshold_edge_on_the_device(cuda):
    """tests/test_evaluator_cpu.py:test_neutral_boxes_and_threshold_edge through the device path."""
    case = C.neutral_edge_case()
    np.testing.assert_allclose(case["threshold"], 36.0 / 114.0)
    ev = C.run(C.make_evaluator(case, device_matching=True), case)
    assert list(ev.num_gt_per_class) == [0, 1]
    np.testing.assert_array_equal(ev.true_positives[1], [0, 1, 0])
    np.testing.assert_array_equal(ev.false_positives[1], [0, 0, 1])
    np.testing.assert_allclose(ev.average_precisions[1], 1.0)


def test_full_call_on_a_model_stub_on_the_device(cuda):
    """`__call__` end to end (tests/test_evaluator_cpu.py:test_full_call_on_a_model_stub) with device_matching=True."""
    from jpeg_detection_resnet_ssd_amd.data.generators import SyntheticDataGeneratorDCT
    data = SyntheticDataGeneratorDCT(n_images=10, seed=3)

    class Oracle(object):
        def __init__(self):
            self.seen = 0

        def predict(self, batch_X):
            b = batch_X[0].shape[0]
            out = np.zeros((b, 8, 6))
            for k in range(b):
                gt = data.labels[(self.seen + k) % 10]
                out[k, :len(gt), 0] = gt[:, 0]
                out[k, :len(gt), 1] = 0.9
                out[k, :len(gt), 2:] = gt[:, 1:]
            self.seen += b
            return out

    ev = Evaluator(model=Oracle(), n_classes=20, data_generator=data, model_mode="inference", device_matching=True)
    m, aps = ev(img_height=300, img_width=300, batch_size=4, verbose=False, return_average_precisions=True)
    present = sorted({int(c) for g in data.labels for c in g[:, 0]})
    for c in range(1, 21):
        assert aps[c] == (1.0 if c in present else 0.0)
    np.testing.assert_allclose(m, len(present) / 20.0)
    assert sum(len(r) for r in ev.prediction_results) == sum(len(g) for g in data.labels)
