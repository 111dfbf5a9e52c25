"""CPU: `collect_host` + `rank_host` (eval_utils/device_matching.py), the numpy statement of csrc/dj_eval_collect.hip,
against the host loop of `Evaluator.predict_on_dataset` + `pack_evaluation`; the decimal rounding identity the kernel
relies on against CPython's `round`; the lazily materialised `prediction_results`; the device forms of the inverters.
Every comparison is on integers or on the raw bits of floats."""
import numpy as np
import pytest

import eval_collect_cases as C
from jpeg_detection_resnet_ssd_amd.eval_utils import device_matching as dm
from jpeg_detection_resnet_ssd_amd.eval_utils.average_precision_evaluator import Evaluator

CASES = C.small_cases() + C.large_cases()


def statement(case):
    records = dm.collect_host(C.statement_batches(case), case["n_classes"], dm.conf_digits_of(case["round_confidences"]))
    assert records["errors"] == 0
    return records, dm.rank_host(records, case["n_classes"], len(case["image_ids"]))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_statement_equals_the_host_loop_and_pack_evaluation(case):
    lists, packed = C.reference(case)
    records, ranked = statement(case)
    assert records["n"] == sum(len(r) for r in lists) == packed.n_pred
    C.assert_ranked_equals_packed(ranked, packed)


def test_the_cases_hold_what_they_are_for():
    by_name = {c["name"]: c for c in CASES}
    lists, packed = C.reference(by_name["ties-and-zeros"])
    assert packed.class_offsets[-1] == packed.class_offsets[-2] > 0                # the last class has no predictions
    y = np.concatenate([b[0] for b in by_name["ties-and-zeros"]["batches"]])
    cls = y[:, :, 0]
    assert np.any((cls[:, :-1] == 0) & (cls[:, 1:] != 0))                          # padding between valid rows
    both_zeros, within, across = False, False, False
    for c in range(1, 4):
        conf = np.array([p[1] for p in lists[c]], dtype=np.float32)
        zeros = conf[conf == 0]
        both_zeros |= bool(np.signbit(zeros).any() and not np.signbit(zeros).all())    # +0.0 and -0.0 in one class
        ids = [p[0] for p in lists[c]]
        same = [(ids[i], ids[j]) for i in range(len(ids)) for j in range(i + 1, len(ids)) if conf[i] == conf[j]]
        within |= any(a == b for a, b in same)                                         # ties within an image
        across |= any(a != b for a, b in same)                                         # ... and across images and batches
    assert both_zeros and within and across
    assert C.reference(by_name["no-predictions"])[1].n_pred == 0
    wrapped = by_name["wrapped-last-batch"]["batches"]
    assert [b[1] for b in wrapped] == [2, 2, 1] and wrapped[-1][2] == ["img4", "img0"]
    packed = C.reference(by_name["repeated-ids"])[1]
    assert set(packed.pred_image.tolist()) == {2, 3, 4}                            # a repeated id maps to its last position
    descs = [dm.batch_descriptors(np.zeros(len(b[2]), np.int32), b[3], b[1]) for b in by_name["fallback"]["batches"]]
    assert [d is None for d in descs] == [True, True, False]                       # no device form; two resizes
    resize = dm.batch_descriptors(np.zeros(3, np.int32), by_name["resize"]["batches"][0][3])
    assert resize["kind"].tolist() == [1, 1, 1] and resize["scale_y"].tolist() == [1.25, np.float32(333 / 300), 1.25]
    assert float(np.float32(333 / 300)) != 333 / 300 and float(np.float32(375 / 300)) == 375 / 300
    # products that land on .5: 2.0 * 1.25 = 2.5 -> 2; 2.8f * 1.25 rounds to 3.5 as a float32 product (-> 4), not as a double
    inv = C.resize_inverter(375, 500)
    out = inv(np.array([[1, 0.5, 0, 2.0, 0, 2.8]], dtype=np.float32))
    assert out[0, 3] == 2.0 and out[0, 5] == 4.0 and float(np.float32(2.8)) * 1.25 < 3.5
    assert len(C.reference(by_name["8000-one-class"])[0][1]) == 8000
    assert len(C.reference(by_name["one-long-segment"])[1].seg_class) == 1


def test_bad_class_ids_and_nan_confidences_raise():
    base = C.small_cases()[0]
    n_classes, n_images = base["n_classes"], len(base["image_ids"])
    for cls in (n_classes + 1, -1, 1.5, np.nan):
        case = C.with_rows(base, "bad-class", {(1, 2): (cls, 0.5, 1, 2, 3, 4)})
        assert dm.collect_host(C.statement_batches(case), n_classes)["errors"] == 1
    case = C.with_rows(base, "nan-conf", {(1, 2): (2, np.nan, 1, 2, 3, 4)})
    records = dm.collect_host(C.statement_batches(case), n_classes)
    assert records["errors"] == 0
    with pytest.raises(ValueError, match="NaN confidence"):
        dm.rank_host(records, n_classes, n_images)
    ev = C.make_evaluator(case)
    ev.prediction_results = C.host_lists(case)
    with pytest.raises(ValueError, match="NaN confidence"):
        dm.pack_evaluation(ev)
    with pytest.raises(ValueError, match="1..8 digits"):
        dm.conf_digits_of(9)


def test_rounding_identity_against_pythons_round():
    """round(float(v), d) == rint(10**d * v) / 10**d as doubles for float32 v, sign of zero included."""
    rng = np.random.default_rng(0)
    quarters = (np.arange(-400, 4001) * 0.25).astype(np.float32)                   # every multiple of 0.25 in -100..1000
    coords = np.concatenate([quarters, rng.uniform(-1e5, 8e5, 150000).astype(np.float32),
                             rng.uniform(-400, 400, 150000).astype(np.float32), np.float32([0.0, -0.0, -0.04, 0.05, -0.05])])
    want = np.array([round(float(v), 1) for v in coords])
    assert np.array_equal(dm.round_decimal(coords, 1).view(np.uint64), want.view(np.uint64))
    assert dm.round_decimal(np.float32([0.25, 0.75, 1.25, -0.25]), 1).tolist() == [0.2, 0.8, 1.2, -0.2]
    # the float32 form re-rounds to the same double (what the lazily built lists rely on)
    again = dm.round_decimal(want.astype(np.float32), 1)
    assert np.array_equal(again.view(np.uint64), want.view(np.uint64))
    conf = np.concatenate([rng.random(20000).astype(np.float32), (np.arange(0, 41) * 0.025).astype(np.float32)])
    for d in range(1, 9):
        want = np.array([round(float(v), d) for v in conf])
        assert np.array_equal(dm.round_decimal(conf, d).view(np.uint64), want.view(np.uint64)), d


@pytest.mark.parametrize("case", C.small_cases(), ids=[c["name"] for c in C.small_cases()])
def test_lazy_prediction_results_equal_the_hosts_lists(case):
    records, _ = statement(case)
    ids = [i for _, n_valid, batch_ids, _ in case["batches"] for i in batch_ids[:n_valid]]
    got = dm.records_to_lists(records, case["n_classes"], ids, bool(case["round_confidences"]))
    C.assert_same_lists(got, C.reference(case)[0])


def test_device_forms_describe_the_inverters():
    from jpeg_detection_resnet_ssd_amd.data.ssd_augment import Resize, _identity_inverter
    rng = np.random.default_rng(5)
    boxes = np.concatenate([rng.uniform(-50, 400, (500, 6)), rng.choice(C.EDGE_COORDS, (100, 6))]).astype(np.float32)
    assert _identity_inverter.device_form == ("identity",) and _identity_inverter(boxes) is boxes
    for h, w in ((375, 500), (333, 500), (300, 300), (1, 7), (480, 301)):
        inv = C.resize_inverter(h, w)
        kind, sy, sx = inv.device_form
        assert kind == "resize" and sy == h / 300 and sx == w / 300
        want = inv(boxes)
        got = boxes.copy()
        got[:, [3, 5]] = np.rint(boxes[:, [3, 5]] * np.float32(sy))
        got[:, [2, 4]] = np.rint(boxes[:, [2, 4]] * np.float32(sx))
        assert want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    other = Resize(300, 300, labels_format={"class_id": 0, "ymin": 1, "xmin": 2, "ymax": 3, "xmax": 4})
    inv = other(np.zeros((10, 10, 3), dtype=np.uint8), return_inverter=True)[1]
    assert not hasattr(inv, "device_form")                                         # other columns: the batch falls back


def test_evaluator_surface_of_device_predictions():
    case = C.small_cases()[0]
    ev = C.make_evaluator(case, device_predictions=True)
    assert ev.device_predictions and ev.device_matching and ev.prediction_results is None
    with pytest.raises(ValueError, match="predict_on_dataset"):
        ev.match_predictions(verbose=False)
    lists = C.host_lists(case)
    ev.prediction_results = lists                    # assigning puts the evaluator on the lists
    assert ev.prediction_results is lists
    with pytest.raises(ValueError, match="training"):
        Evaluator(None, 3, None, model_mode="training", device_predictions=True)
    with pytest.raises(ValueError, match="pred_format"):
        Evaluator(None, 3, None, pred_format={"class_id": 0, "conf": 1, "ymin": 2, "xmin": 3, "ymax": 4, "xmax": 5},
                  device_predictions=True)
    assert not Evaluator(None, 3, None).device_predictions


def test_pack_ground_truth_is_the_ground_truth_half_of_pack_evaluation():
    case = C.small_cases()[0]
    packed = C.reference(case)[1]
    truth = dm.pack_ground_truth(C.make_evaluator(case))
    for name in ("gt_offsets", "gt_boxes", "gt_class", "gt_neutral"):
        assert np.array_equal(truth[name], getattr(packed, name)) and truth[name].dtype == getattr(packed, name).dtype
    assert truth["n_images"] == packed.n_images and truth["use_neutral"] == packed.use_neutral


def test_entry_points_check_their_arguments_before_any_launch():
    """No GPU needed: every call below must fail in the host-side checks (the pointers are never dereferenced)."""
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    fake = 0x1000
    desc = np.zeros(3, dtype=dm.DESC_DTYPE)
    assert dm.DESC_DTYPE.itemsize == 16

    def collect(n_valid=3, first=0, digits=0, capacity=24, rows=8):
        return lib.dj_eval_collect(fake, 3, rows, n_valid, desc.ctypes.data, first, 4, 7, digits, 0, fake, fake, fake, fake, fake,
                                   fake, capacity, fake, None)
    assert collect(digits=9) < 0 and b"conf_digits" in lib.dj_last_error()
    assert collect(first=1) < 0 and b"capacity" in lib.dj_last_error()             # (1 + 3) * 8 records > 24
    assert collect(n_valid=4) < 0 and b"sizes" in lib.dj_last_error()
    desc["image_index"][1] = 7
    assert collect() < 0 and b"outside the dataset" in lib.dj_last_error()
    desc["image_index"][1], desc["kind"][2] = 0, 2
    assert collect() < 0 and b"unknown transform" in lib.dj_last_error()
    need = lib.dj_eval_rank_workspace_bytes(1000, 20)
    assert need >= 4 * 8 * 1000 + 4 * 22 + 4 * 4 and lib.dj_eval_rank_workspace_bytes(0, 20) == 0
    rank = lambda cap, n_images, ws: lib.dj_eval_rank(fake, fake, fake, fake, cap, 20, n_images, fake, fake, fake, fake, fake, fake,
                                                      fake, fake, fake, fake, fake, ws, None)
    assert rank(1000, 5, need - 1) < 0 and b"workspace" in lib.dj_last_error()
    assert rank(1000, 2 ** 27, need) < 0 and b"2^31" in lib.dj_last_error()
    assert rank(0, 5, need) < 0 and b"capacity" in lib.dj_last_error()
