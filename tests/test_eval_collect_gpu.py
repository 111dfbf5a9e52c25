"""GPU: dj_eval_collect / dj_eval_rank (csrc/dj_eval_collect.hip) against the host loop of `predict_on_dataset` +
`pack_evaluation` on the cases of tests/eval_collect_cases.py, and `Evaluator(device_predictions=True)` against the host
Evaluator on a stub model and on an SSD inference model.  Integers are compared as they are, floats by their bits."""
import numpy as np
import pytest
import torch

import eval_collect_cases as C
from jpeg_detection_resnet_ssd_amd.eval_utils import device_matching as dm
from jpeg_detection_resnet_ssd_amd.eval_utils.average_precision_evaluator import Evaluator

pytestmark = pytest.mark.gpu

CASES = C.small_cases() + C.large_cases()
PER_CLASS = ("true_positives", "false_positives", "cumulative_true_positives", "cumulative_false_positives",
             "cumulative_precisions", "cumulative_recalls")


def collect(case):
    collector = dm.DeviceCollector(case["n_classes"], case["image_ids"], dm.conf_digits_of(case["round_confidences"]))
    for y, n_valid, ids, chain in case["batches"]:
        collector.add(torch.from_numpy(y).cuda(), n_valid, ids, chain)
    return collector


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_collect_and_rank_equal_the_host_loop_and_pack_evaluation(cuda, case):
    lists, packed = C.reference(case)
    collector = collect(case)
    ranked, offsets = collector.rank()
    assert collector.counts == (packed.n_pred, len(packed.seg_class))
    assert np.array_equal(offsets, packed.class_offsets)
    C.assert_ranked_equals_packed({k: v.cpu().numpy() for k, v in ranked.items()}, packed)
    # the records themselves against the numpy statement, and the lists made of them against the host's
    want = dm.collect_host(C.statement_batches(case), case["n_classes"], dm.conf_digits_of(case["round_confidences"]))
    got = collector.download_records()
    assert got["n"] == want["n"] and got["errors"] == 0
    for name, _ in dm.RECORD_FIELDS:
        assert got[name].dtype == want[name].dtype and np.array_equal(C.bits(got[name]), C.bits(want[name])), name
    if case in C.small_cases():
        C.assert_same_lists(collector.prediction_results(), lists)


def test_fallback_batches_are_appended_as_final_rows(cuda, monkeypatch):
    case = {c["name"]: c for c in CASES}["fallback"]
    finals = []
    from jpeg_detection_resnet_ssd_amd import kernels
    real = kernels.eval_collect
    monkeypatch.setattr(kernels, "eval_collect", lambda *a: (finals.append(bool(a[7])), real(*a))[1])
    collect(case)
    assert finals == [True, True, False]             # image 1: no device form; image 3: two resizes; last batch: 1 valid image


@pytest.mark.parametrize("row,message", [((5, 0.5, 1, 2, 3, 4), "class id"), ((1.5, 0.5, 1, 2, 3, 4), "class id"),
                                         ((2, np.nan, 1, 2, 3, 4), "NaN confidence")])
def test_bad_class_ids_and_nan_confidences_raise(cuda, row, message):
    case = C.with_rows(C.small_cases()[0], "bad", {(1, 2): row})
    with pytest.raises(ValueError, match=message):
        collect(case).rank()


def test_capacity_is_checked_before_the_launch(cuda):
    case = C.small_cases()[0]
    collector = collect(case)
    y, _, ids, chain = case["batches"][0]
    with pytest.raises(ValueError, match="more images"):
        collector.add(torch.from_numpy(y).cuda(), 3, ids, chain)
    from jpeg_detection_resnet_ssd_amd import _lib, kernels
    desc = dm.batch_descriptors(np.zeros(3, np.int32), None)
    with pytest.raises(_lib.DjError, match="capacity"):
        kernels.eval_collect(torch.from_numpy(y).cuda(), 3, desc, len(case["image_ids"]) - 2, case["n_classes"],
                             len(case["image_ids"]), 0, False, collector.records, collector.counters)


# ---- Evaluator level ---------------------------------------------------------------------------------------------------------
class Stub(object):
    """A model whose decoded output is seeded by the number of the call: `predict` gives it as numpy, the device-output
    method as a CUDA tensor."""

    def __init__(self, n_classes=20, rows=8):
        self.calls, self.n_classes, self.rows = 0, n_classes, rows

    def _batch(self, b):
        rng = np.random.default_rng(1000 + self.calls)
        self.calls += 1
        y = np.zeros((b, self.rows, 6), dtype=np.float32)
        keep = rng.random((b, self.rows)) < 0.7
        y[:, :, 0] = np.where(keep, rng.integers(1, self.n_classes + 1, (b, self.rows)), 0)
        y[:, :, 1] = rng.choice([0.9, 0.5, 0.25, 0.0, -0.0, 0.123456789], (b, self.rows))
        y[:, :, 2:4] = rng.uniform(-5, 200, (b, self.rows, 2))
        y[:, :, 4:6] = y[:, :, 2:4] + rng.uniform(1, 120, (b, self.rows, 2))
        y[0, 0, 2:] = [0.25, 0.75, 1.25, 100.05]
        return y

    def predict(self, x):
        return self._batch(len(x[0]))

    def predict_on_batch(self, x, to_host=True):
        assert not to_host
        return torch.from_numpy(self._batch(len(x[0]))).cuda()


def run(ev, **kw):
    ev(img_height=300, img_width=300, batch_size=2, verbose=False, **kw)
    return ev


def assert_same_evaluation(dev, host, n_classes):
    C.assert_same_lists(dev.prediction_results, host.prediction_results)
    for name in PER_CLASS:
        a, b = getattr(dev, name), getattr(host, name)
        assert len(a) == len(b) == n_classes + 1 and len(a[0]) == 0
        for c in range(1, n_classes + 1):
            assert a[c].dtype == b[c].dtype and a[c].shape == b[c].shape, (name, c)
            assert np.array_equal(C.bits(a[c]), C.bits(b[c])), (name, c)
    assert len(dev.average_precisions) == n_classes + 1
    for c in range(n_classes + 1):
        assert type(dev.average_precisions[c]) is type(host.average_precisions[c])
        assert C.bits(np.array([dev.average_precisions[c]])) == C.bits(np.array([host.average_precisions[c]])), c
    assert C.bits(np.array([dev.mean_average_precision])) == C.bits(np.array([host.mean_average_precision]))


@pytest.mark.parametrize("round_confidences", [False, True, 3])
def test_evaluator_on_a_stub_model_equals_the_host_evaluator(cuda, round_confidences):
    from jpeg_detection_resnet_ssd_amd.data.generators import SyntheticDataGeneratorDCT
    data = SyntheticDataGeneratorDCT(n_images=5, seed=3)
    host = run(Evaluator(Stub(), 20, data, model_mode="inference"), round_confidences=round_confidences,
               sorting_algorithm="mergesort")
    dev = run(Evaluator(Stub(), 20, data, model_mode="inference", device_predictions=True), round_confidences=round_confidences)
    assert sum(len(r) for r in host.prediction_results) > 20
    assert_same_evaluation(dev, host, 20)


def test_no_per_batch_download_and_no_pack_evaluation(cuda, monkeypatch):
    from jpeg_detection_resnet_ssd_amd.data.generators import SyntheticDataGeneratorDCT
    calls = {"pack": 0, "download": 0}
    monkeypatch.setattr(dm, "pack_evaluation", lambda *a, **k: calls.__setitem__("pack", calls["pack"] + 1))
    for name in ("cpu", "numpy", "tolist", "item"):
        def counted(self, *a, _real=getattr(torch.Tensor, name), **k):
            calls["download"] += bool(self.is_cuda)
            return _real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    counts = []
    for n_images in (5, 9):
        data = SyntheticDataGeneratorDCT(n_images=n_images, seed=3)
        ev = Evaluator(Stub(), 20, data, model_mode="inference", device_predictions=True)
        calls["download"] = 0
        ev.predict_on_dataset(300, 300, batch_size=2, verbose=False)
        assert calls["download"] == 0                # 3 and 5 batches, none of them downloaded
        ev.get_num_gt_per_class(verbose=False)
        ev.match_predictions(verbose=False)
        counts.append(calls["download"])
    # the counters with the class offsets, then the four result arrays: the same whatever the number of batches
    assert counts == [5, 5] and calls["pack"] == 0


def test_evaluator_on_an_ssd_inference_model_equals_the_host_evaluator(cuda):
    from jpeg_detection_resnet_ssd_amd import workloads
    from jpeg_detection_resnet_ssd_amd.data.generators import SyntheticDataGeneratorDCT
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.models.keras_ssd300_dct_j2d_resnet import ssd_resnet_EF_layers_custom
    K.clear_session()
    infer = ssd_resnet_EF_layers_custom(archi="ssd_custom", **dict(workloads.SSD_ARGS, mode="inference",
                                                                  confidence_thresh=0.01, top_k=20))
    weights = infer.get_weights_dict()
    for k in weights:                                # random init: keep exp() of the box offsets finite
        if "mbox_loc" in k or "mbox_conf" in k:
            weights[k] = weights[k] * 1e-5
    infer.set_weights_dict(weights)
    data = SyntheticDataGeneratorDCT(n_images=5, seed=11)
    host = run(Evaluator(infer, 20, data, model_mode="inference"), sorting_algorithm="mergesort")
    dev = run(Evaluator(infer, 20, data, model_mode="inference", device_predictions=True))
    per_image = {}
    for results in host.prediction_results:
        for p in results:
            per_image[p[0]] = per_image.get(p[0], 0) + 1
    assert sorted(per_image) == sorted(data.image_ids) and min(per_image.values()) >= 1      # no empty evaluation
    assert_same_evaluation(dev, host, 20)
    with pytest.raises(ValueError, match="training"):
        Evaluator(infer, 20, data, model_mode="training", device_predictions=True)
