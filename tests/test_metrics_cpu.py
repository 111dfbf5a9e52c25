"""CPU: the host statement of the validation metrics (keras/metrics.py:classification_counts_host, what dj_eval_accumulate
counts), which compile-time metrics the device sweep takes, Model.metrics_names, the classifier Evaluator and the
configuration's evaluation surface."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def _one_hot(t, c):
    y = np.zeros((len(t), c), np.float32)
    y[np.arange(len(t)), t] = 1.0
    return y


def _hits(y_true, probs, ks):
    from jpeg_detection_resnet_ssd_amd.keras.metrics import classification_counts_host
    out = classification_counts_host(np.asarray(y_true, np.float32), np.asarray(probs, np.float32), ks)
    assert out.dtype == np.int64 and out[0] == len(probs)
    return [int(v) for v in out[1:]]


def test_counts_ties_count_as_in_the_top_k():
    # target (class 3) tied with classes 1 and 2 below one larger class: one class strictly above it, so it is in the top
    # k for every k >= 2 although the tie straddles k = 2, and not in the top 1
    probs = [[0.4, 0.2, 0.2, 0.2]]
    assert _hits(_one_hot([3], 4), probs, [1, 2, 3, 4]) == [0, 1, 1, 1]
    # a three-way tie for the first place: a hit for every k >= 1, whichever of the three the target is
    probs = [[0.3, 0.3, 0.3, 0.1]]
    for t in (0, 1, 2):
        assert _hits(_one_hot([t], 4), probs, [1, 2, 3]) == [1, 1, 1]
    assert _hits(_one_hot([3], 4), probs, [1, 2, 3, 4]) == [0, 0, 0, 1]
    # categorical accuracy takes the FIRST maximum
    assert _hits(_one_hot([0], 4), probs, [0]) == [1]
    assert _hits(_one_hot([1], 4), probs, [0]) == [0]


def test_counts_nan_and_inf():
    # a target whose probability is NaN (or infinite) is never a hit for k >= 1
    assert _hits(_one_hot([1], 3), [[0.5, NAN, 0.2]], [1, 2, 3]) == [0, 0, 0]
    assert _hits(_one_hot([1], 3), [[0.5, INF, 0.2]], [1, 2, 3]) == [0, 0, 0]
    # a NaN in another class compares false: it is not counted as lying above the target ...
    assert _hits(_one_hot([2], 3), [[NAN, 0.1, 0.2]], [1, 2]) == [1, 1]
    # ... while +Inf in another class is
    assert _hits(_one_hot([2], 3), [[INF, 0.1, 0.2]], [1, 2]) == [0, 1]
    # np.argmax: a NaN counts as the maximum, for the prediction (k = 0) and for the target alike
    assert _hits(_one_hot([0], 3), [[NAN, 0.9, 0.2]], [0]) == [1]
    assert _hits(_one_hot([1], 3), [[NAN, 0.9, 0.2]], [0]) == [0]
    assert _hits([[0.0, 1.0, NAN]], [[0.1, 0.2, 0.7]], [0, 1]) == [1, 1]      # t = 2


def test_counts_all_equal_rows_and_empty_targets():
    c = 5
    probs = np.full((c, c), 0.2, np.float32)
    # all-equal rows: nothing lies strictly above the target, a hit for every k >= 1; for k = 0 only when t == 0
    assert _hits(_one_hot(np.arange(c), c), probs, [1, 2, 5, 0]) == [c, c, c, 1]
    # an all-zero y_true row gives t == 0
    y = np.zeros((2, 3), np.float32)
    assert _hits(y, [[0.5, 0.3, 0.2], [0.1, 0.3, 0.6]], [1, 0]) == [1, 1]
    # several rows add up; no rows at all
    y = _one_hot([0, 1, 2, 2], 3)
    p = [[0.5, 0.3, 0.2], [0.5, 0.3, 0.2], [0.5, 0.3, 0.2], [0.2, 0.3, 0.5]]
    assert _hits(y, p, [0, 1, 2, 3]) == [2, 2, 3, 4]
    from jpeg_detection_resnet_ssd_amd.keras.metrics import classification_counts_host
    assert list(classification_counts_host(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), [1, 0])) == [0, 0, 0]


def _config_module():
    spec = importlib.util.spec_from_file_location("cfg_resnet_metrics", os.path.join(ROOT, "config", "resnet", "config_file.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tiny_model(metrics):
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras import layers as L
    from jpeg_detection_resnet_ssd_amd.keras.models import Model
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import SGD
    K.clear_session()
    x = L.Input(shape=(4, 4, 3))
    y = L.Dense(6, activation="softmax")(L.GlobalAveragePooling2D()(L.Conv2D(8, (3, 3), padding="same")(x)))
    model = Model(x, y)
    model.compile(optimizer=SGD(lr=0.01), loss="categorical_crossentropy", metrics=metrics)
    return model


def test_metric_recognition_and_names():
    from jpeg_detection_resnet_ssd_amd.keras import metrics as M
    mod = _config_module()
    top1, top5 = mod._top_k_accuracy(1), mod._top_k_accuracy(5)
    assert top1.__name__ == top5.__name__ == "_func"                  # the log keys do not change
    assert top1._dj_metric == ("top_k", 1) and top5._dj_metric == ("top_k", 5)
    assert M.device_metric_k(top1) == 1 and M.device_metric_k(top5) == 5
    assert M.device_metric_k("accuracy") == 0 and M.device_metric_k("acc") == 0
    assert M.device_metric_k(M.top_k_categorical_accuracy) == 5 and M.device_metric_k(M.categorical_accuracy) == 0

    def unknown(y_true, y_pred):
        return 0.5
    assert M.device_metric_k(unknown) is None and M.device_metric_k(lambda t, p: 1.0) is None
    assert M.device_metric_k("mae") is None

    def mistagged(y_true, y_pred):
        return 0.5
    mistagged._dj_metric = ("top_k", "5")
    assert M.device_metric_k(mistagged) is None

    assert [n for n, _ in M.metric_entries([top1, top5, "accuracy", unknown, "mae", top1])] == \
        ["_func", "_func_1", "acc", "unknown", "_func_2"]
    assert _tiny_model([top1, top5, "accuracy"]).metrics_names == ["loss", "_func", "_func_1", "acc"]
    assert _tiny_model(None).metrics_names == ["loss"]
    assert _tiny_model([unknown, "acc"]).metrics_names == ["loss", "unknown", "acc"]


class _StubModel(object):
    def __init__(self, scores):
        self.scores, self.calls = list(scores), []

    def evaluate_generator(self, generator, **kwargs):
        self.calls.append((generator, kwargs))
        return self.scores[(len(self.calls) - 1) % len(self.scores)]


def test_classifier_evaluator():
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.evaluation import Evaluator
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.evaluation.evaluators import Evaluator as Same
    assert Evaluator is Same
    ev = Evaluator()
    assert ev.score is None and ev.test_generator is None and ev.runs is False
    with pytest.raises(RuntimeError, match="generator should be specified"):
        ev(_StubModel([[1.0]]))
    with pytest.raises(RuntimeError, match="generator should be specified"):
        ev.make_runs(_StubModel([[1.0]]))

    gen = object()
    model = _StubModel([[2.0, 0.25, 0.75]])
    ev(model, gen)
    assert ev.score == [2.0, 0.25, 0.75] and ev.test_generator is gen
    assert model.calls == [(gen, {"verbose": 1})]
    assert str(ev) == "The evaluated score is [2.0, 0.25, 0.75]."

    # make_runs: the element-wise mean of the runs; the generator of the constructor serves when none is given
    ev2 = Evaluator(gen)
    model = _StubModel([[1.0, 0.0, 0.5], [3.0, 0.5, 1.0]])
    ev2.make_runs(model, number_of_runs=4)
    assert len(model.calls) == 4 and all(g is gen for g, _ in model.calls)
    np.testing.assert_array_equal(ev2.score, np.array([2.0, 0.25, 0.75]))
    assert ev2.runs and ev2.number_of_runs == 4
    assert str(ev2) == "Number of runs: 4\nAverage score: {}".format(np.array([2.0, 0.25, 0.75]))
    other = object()
    ev2(_StubModel([0.5]), other)                      # a plain call afterwards reports a single score again
    assert ev2.test_generator is other and str(ev2) == "The evaluated score is 0.5."


def test_evaluator_display_results(capsys):
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.evaluation import Evaluator
    ev = Evaluator(object())
    ev(_StubModel([[1.5, 0.5]]))
    ev.display_results()
    assert capsys.readouterr().out == "The evaluated score is [1.5, 0.5].\n"


@pytest.mark.parametrize("archi,deconv,shapes", [
    ("deconv", True, [(4, 28, 28, 64), (4, 14, 14, 64), (4, 14, 14, 64)]),
    ("late_concat_rfa_thinner", False, [(4, 28, 28, 64), (4, 14, 14, 128)])])
def test_config_evaluation_surface(monkeypatch, archi, deconv, shapes):
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.evaluation import Evaluator
    for var in ("DJ_TEST_DIR", "DJ_VAL_DIR", "DJ_TRAIN_DIR", "DJ_INDEX_FILE", "DJ_DEVICE_PREP"):
        monkeypatch.delenv(var, raising=False)
    mod = _config_module()
    K.clear_session()
    cfg = mod.TrainingConfiguration(deconv=deconv, archi=archi, load_pretrained_weights=False)
    assert cfg.evaluator is None and cfg.test_generator is None
    cfg._batch_size = 4
    cfg.prepare_for_inference()
    cfg.prepare_testing_generator()
    cfg.prepare_evaluator()
    assert isinstance(cfg.evaluator, Evaluator)
    gen = cfg.test_generator
    assert isinstance(gen, mod.SyntheticDCTClassificationGenerator) and len(gen) == 8
    x, y = gen[0]
    assert [a.shape for a in x] == shapes and y.shape == (4, 1000) and np.all(y.sum(-1) == 1.0)
    x2, y2 = gen[0]                                    # a pass can be repeated: the batches do not change
    assert all(np.array_equal(a, b) for a, b in zip(x, x2)) and np.array_equal(y, y2)
    assert [m._dj_metric for m in cfg.metrics] == [("top_k", 1), ("top_k", 5)]


def test_rgb_config_inherits_the_evaluation_surface(monkeypatch):
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.evaluation import Evaluator
    for var in ("DJ_TEST_DIR", "DJ_VAL_DIR", "DJ_INDEX_FILE"):
        monkeypatch.delenv(var, raising=False)
    spec = importlib.util.spec_from_file_location("cfg_rgb_metrics", os.path.join(ROOT, "config", "resnetRGB", "config_file.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    K.clear_session()
    cfg = mod.TrainingConfiguration(load_pretrained_weights=False)
    cfg._batch_size = 2
    cfg.prepare_testing_generator()
    cfg.prepare_evaluator()
    assert isinstance(cfg.evaluator, Evaluator)
    x, y = cfg.test_generator[0]
    assert x[0].shape == (2, 224, 224, 3) and y.shape == (2, 1000)


def check_accumulate_refusals():
    """dj_eval_accumulate checks its arguments on the host before any launch (fake pointers, never dereferenced)."""
    import ctypes
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    fake = 0x1000
    ks = (ctypes.c_int * 9)(0, 1, 5, 7, 2, 3, 4, 6, 1)
    call = lib.dj_eval_accumulate
    assert call(fake, fake, 4, 10, ks, 9, fake, 1.0, fake, fake, None) < 0 and b"n_k" in lib.dj_last_error()
    assert call(fake, fake, 4, 6, ks, 4, fake, 1.0, fake, fake, None) < 0 and b"k = 7" in lib.dj_last_error()
    neg = (ctypes.c_int * 1)(-1)
    assert call(fake, fake, 4, 6, neg, 1, fake, 1.0, fake, fake, None) < 0 and b"k = -1" in lib.dj_last_error()
    assert call(fake, fake, -1, 6, ks, 2, fake, 1.0, fake, fake, None) < 0 and b"rows" in lib.dj_last_error()
    assert call(fake, fake, 4, 0, ks, 1, fake, 1.0, fake, fake, None) < 0 and b"C = 0" in lib.dj_last_error()
    assert call(fake, fake, 4, 10, ks, 3, fake, 1.0, None, fake, None) < 0 and b"null" in lib.dj_last_error()
    assert call(fake, fake, 4, 10, ks, 3, fake, 1.0, fake, None, None) < 0 and b"null" in lib.dj_last_error()


def test_accumulate_refusals_without_a_gpu():
    check_accumulate_refusals()
