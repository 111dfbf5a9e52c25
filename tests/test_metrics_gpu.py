"""GPU: dj_eval_accumulate against its host statement (counts exactly equal, the float64 loss sums exactly equal), and the
Keras surface above it: Model.evaluate_generator, the val_ metrics of fit_generator, and the evaluate.py entry script."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def _planted_batch(rows, c, ks, call):
    """Random probabilities and one-hot targets with, row after row, a tie at a top-k boundary that is a hit, one that is a
    miss, a NaN / +Inf in another class and at the target, an all-equal row under an all-zero y_true, and targets at
    index 0 and C - 1."""
    rng = np.random.default_rng(1000 * rows + 10 * c + call)
    p = rng.random((rows, c), dtype=np.float32) + np.float32(1e-3)
    p /= p.sum(-1, keepdims=True)
    t = rng.integers(0, c, rows)
    t[0] = 0 if call % 2 == 0 else c - 1
    if rows > 1:
        t[1] = c - 1 if call % 2 == 0 else 0
    y = np.zeros((rows, c), np.float32)
    y[np.arange(rows), t] = 1.0
    k = max([kk for kk in ks if 0 < kk < c] or [1])
    for i in range(rows):
        kind, ti, other = (i + 3 * call) % 8, t[i], (t[i] + 1 + i) % c
        order = np.sort(p[i])[::-1]
        if kind == 1:            # k - 1 classes above, the k-th place shared with another class: a hit for k
            p[i, ti] = order[min(k, c) - 1]
            p[i, other] = p[i, ti]
        elif kind == 2 and c > k:   # the k-th place is a tie above the target: k classes above, a miss for k
            p[i, ti] = order[k]
            p[i, np.argsort(p[i])[::-1][:k]] = order[k - 1]
        elif kind == 3:
            p[i, other] = np.nan
        elif kind == 4:
            p[i, ti] = np.nan
        elif kind == 5:
            p[i, other] = np.inf
        elif kind == 6:
            p[i, ti] = np.inf
        elif kind == 7:
            p[i, :] = np.float32(1.0 / c)
            y[i, :] = 0.0
    return y, p


@pytest.mark.parametrize("c", [1, 3, 63, 64, 65, 1000, 1001])
@pytest.mark.parametrize("rows", [1, 5, 257])
def test_accumulate_matches_the_host_statement(rows, c, cuda):
    from jpeg_detection_resnet_ssd_amd import kernels
    from jpeg_detection_resnet_ssd_amd.keras.metrics import classification_counts_host
    ks = [min(k, c) for k in (0, 1, 5, c)]
    ks_arr = np.asarray(ks, np.int32)
    acc = torch.zeros(2, dtype=torch.float64, device=cuda)
    counts = torch.zeros(1 + len(ks), dtype=torch.int64, device=cuda)
    want_counts = np.zeros(1 + len(ks), np.int64)
    want_loss, want_weight = 0.0, 0.0
    rng = np.random.default_rng(7 * rows + c)
    for call, weight in enumerate([float(rows), 1.0, 2.5]):
        y, p = _planted_batch(rows, c, ks, call)
        loss = rng.random(8, dtype=np.float32) * np.float32(7.0)
        kernels.eval_accumulate(torch.from_numpy(y).to(cuda), torch.from_numpy(p).to(cuda), ks_arr,
                                torch.from_numpy(loss).to(cuda), weight, acc, counts)
        want_counts += classification_counts_host(y, p, ks)
        want_loss = want_loss + weight * float(loss[0])       # float64, product rounded before the sum, in call order
        want_weight = want_weight + weight
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == want_counts.tolist()
    assert acc.cpu().tolist() == [want_loss, want_weight]
    # a call without rows changes only `acc`
    loss = torch.full((8,), 0.3, device=cuda)
    kernels.eval_accumulate(None, None, ks_arr, loss, 3.0, acc, counts)
    y, p = _planted_batch(rows, c, ks, 0)
    dev_y, dev_p = torch.from_numpy(y).to(cuda), torch.from_numpy(p).to(cuda)
    kernels.eval_accumulate(dev_y[:0], dev_p[:0], ks_arr, loss, 0.25, acc, counts)
    want_loss = (want_loss + 3.0 * float(np.float32(0.3))) + 0.25 * float(np.float32(0.3))
    want_weight = (want_weight + 3.0) + 0.25
    # ... and one without a loss only the counts
    kernels.eval_accumulate(dev_y, dev_p, ks_arr, None, 5.0, acc, counts)
    want_counts += classification_counts_host(y, p, ks)
    assert counts.cpu().tolist() == want_counts.tolist()
    assert acc.cpu().tolist() == [want_loss, want_weight]


def test_accumulate_refuses_bad_arguments_before_any_launch(cuda):
    from test_metrics_cpu import check_accumulate_refusals
    check_accumulate_refusals()
    torch.cuda.synchronize()          # nothing was launched on the fake pointers: the device is still healthy


# ---- Model.evaluate_generator / fit_generator ---------------------------------------------------------------------------------
N_CLASSES = 10


def _top_k_accuracy(k):
    from jpeg_detection_resnet_ssd_amd.keras.metrics import top_k_categorical_accuracy

    def _func(y_true, y_pred):
        return top_k_categorical_accuracy(y_true, y_pred, k)
    _func._dj_metric = ("top_k", k)
    return _func


def _classifier(metrics, seed=5):
    """Input, Conv2D (l2-regularised), GlobalAveragePooling2D, Dense softmax: 1,226 weights."""
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras import layers as L
    from jpeg_detection_resnet_ssd_amd.keras.models import Model
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import SGD
    from jpeg_detection_resnet_ssd_amd.keras.regularizers import l2
    K.clear_session()
    K.set_random_seed(seed)
    x = L.Input(shape=(8, 8, 3))
    h = L.Conv2D(32, (3, 3), padding="same", activation="relu", kernel_regularizer=l2(1e-2), name="conv")(x)
    y = L.Dense(N_CLASSES, activation="softmax", name="probs")(L.GlobalAveragePooling2D(name="pool")(h))
    model = Model(x, y)
    model.compile(optimizer=SGD(lr=0.05, momentum=0.9), loss="categorical_crossentropy", metrics=metrics)
    return model


class _Batches(object):
    """keras.utils.Sequence surface over fixed batches of unequal sizes."""

    def __init__(self, sizes, seed):
        rng = np.random.default_rng(seed)
        self.items = []
        for b in sizes:
            x = rng.standard_normal((b, 8, 8, 3)).astype(np.float32)
            y = np.zeros((b, N_CLASSES), np.float32)
            y[np.arange(b), rng.integers(0, N_CLASSES, b)] = 1.0
            self.items.append((x, y))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]

    def __iter__(self):
        while True:
            for item in self.items:
                yield item


def _expected(model, batches, ks):
    """(size-weighted mean, plain mean) of test_on_batch, and hits / rows of the host statement on predict_on_batch."""
    from jpeg_detection_resnet_ssd_amd.keras.metrics import classification_counts_host
    losses = [model.test_on_batch(x, y) for x, y in batches.items]
    sizes = [x.shape[0] for x, _ in batches.items]
    counts = sum(classification_counts_host(y, model.predict_on_batch(x), ks) for x, y in batches.items)
    weighted = sum(b * v for b, v in zip(sizes, losses)) / sum(sizes)
    return weighted, sum(losses) / len(losses), [int(h) / int(counts[0]) for h in counts[1:]]


def test_evaluate_generator(cuda, monkeypatch):
    from jpeg_detection_resnet_ssd_amd.keras import models
    model = _classifier([_top_k_accuracy(1), _top_k_accuracy(5), "accuracy"])
    assert model.metrics_names == ["loss", "_func", "_func_1", "acc"]
    batches = _Batches([8, 8, 8, 3], seed=21)
    want_loss, _, want_metrics = _expected(model, batches, [1, 5, 0])
    assert model._reg_penalty() > 0.0

    downloads = []
    original = models._EvalSweep._download

    def counting(self):
        downloads.append(1)
        return original(self)
    monkeypatch.setattr(models._EvalSweep, "_download", counting)

    got = model.evaluate_generator(batches)
    assert isinstance(got, list) and len(got) == 4 and len(downloads) == 1
    print("evaluate_generator:", got, "expected:", [want_loss] + want_metrics)
    assert got[1:] == want_metrics
    assert 0.0 <= got[1] <= got[2] <= 1.0
    assert abs(got[0] - want_loss) <= 1e-12 * abs(want_loss)
    # repeated calls, with and without the background thread: identical values, one download each
    assert model.evaluate_generator(batches) == got
    assert model.evaluate_generator(batches, workers=0) == got
    assert model.evaluate_generator(iter(batches), steps=4, max_queue_size=2) == got
    assert len(downloads) == 4
    part = model.evaluate_generator(batches, steps=2)
    assert len(downloads) == 5 and part != got
    with pytest.raises(ValueError, match="steps=None"):
        model.evaluate_generator(iter(batches))
    assert isinstance(model.test_on_batch(*batches[0]), float)


def test_evaluate_generator_with_a_metric_the_kernel_does_not_take(cuda):
    """Any other callable is evaluated per batch on the device tensors and averaged weighted by batch size."""
    def first_class_mass(y_true, y_pred):
        assert y_true.is_cuda and y_pred.is_cuda
        return float(y_pred[:, 0].double().mean())
    model = _classifier([_top_k_accuracy(5), first_class_mass])
    assert model.metrics_names == ["loss", "_func", "first_class_mass"]
    batches = _Batches([8, 3], seed=22)
    want_loss, _, want_metrics = _expected(model, batches, [5])
    want_mass = sum(x.shape[0] * float(model.predict_on_batch(x)[:, 0].astype(np.float64).mean())
                    for x, _ in batches.items) / 11
    got = model.evaluate_generator(batches)
    assert got[1] == want_metrics[0]
    assert abs(got[2] - want_mass) <= 1e-12 and abs(got[0] - want_loss) <= 1e-12 * abs(want_loss)
    # without metrics: a scalar
    plain = _classifier(None)
    value = plain.evaluate_generator(batches)
    assert isinstance(value, float)
    assert abs(value - _expected(plain, batches, [])[0]) <= 1e-12 * abs(value)


def test_fit_generator_reports_validation_metrics(cuda, tmp_path):
    from jpeg_detection_resnet_ssd_amd.keras.callbacks import CSVLogger
    model = _classifier([_top_k_accuracy(1), _top_k_accuracy(5), "accuracy"])
    train, val = _Batches([8, 8, 8], seed=31), _Batches([8, 8, 8, 3], seed=32)
    log = str(tmp_path / "results.csv")
    hist = model.fit_generator(train, steps_per_epoch=3, epochs=2, validation_data=val, verbose=0,
                               callbacks=[CSVLogger(filename=log, separator=",", append=True)])
    h = hist.history
    for key in ("loss", "_func", "_func_1", "acc", "val_loss", "val__func", "val__func_1", "val_acc"):
        assert key in h and len(h[key]) == 2, key
    # the weights have not changed since the last epoch's validation sweep
    _, want_val_loss, want_metrics = _expected(model, val, [1, 5, 0])
    after = model.evaluate_generator(val)
    print("fit_generator:", {k: v[-1] for k, v in h.items()}, "evaluate_generator:", after, "mean test_on_batch:", want_val_loss)
    assert [h["val__func"][-1], h["val__func_1"][-1], h["val_acc"][-1]] == after[1:] == want_metrics
    assert abs(h["val_loss"][-1] - want_val_loss) <= 1e-12 * abs(want_val_loss)
    rows = list(csv.reader(open(log)))
    assert {"val_loss", "val__func", "val__func_1", "val_acc", "_func", "_func_1", "acc"} <= set(rows[0])
    assert [r[0] for r in rows[1:]] == ["0", "1"]
    for key in ("val__func", "val__func_1", "val_acc", "val_loss"):
        col = rows[0].index(key)
        assert [float(r[col]) for r in rows[1:]] == pytest.approx(h[key], rel=1e-9)
    # validation data given as one (x, y) batch
    x, y = val[3]
    hist = model.fit_generator(train, steps_per_epoch=1, epochs=1, validation_data=(x, y), verbose=0)
    assert hist.history["val_loss"][0] == pytest.approx(model.test_on_batch(x, y), rel=1e-12)
    assert {"val__func", "val__func_1", "val_acc"} <= set(hist.history)


def test_evaluate_generator_of_an_ssd_model_returns_the_weighted_loss(cuda):
    from test_ssd_gpu import build, make_batch
    archi = "cb5_only"
    model, sizes = build(archi)
    assert model.metrics_names == ["loss"]

    class Seq(object):
        def __init__(self):
            self.items = [make_batch(archi, sizes, 2, seed=70), make_batch(archi, sizes, 1, seed=71)]

        def __len__(self):
            return len(self.items)

        def __getitem__(self, i):
            return self.items[i]

        def __iter__(self):
            while True:
                for item in self.items:
                    yield item

    seq = Seq()
    want = (2 * model.test_on_batch(*seq[0]) + 1 * model.test_on_batch(*seq[1])) / 3
    got = model.evaluate_generator(seq)
    print("ssd evaluate_generator:", got, "expected:", want)
    assert isinstance(got, float) and np.isfinite(got)
    assert abs(got - want) <= 1e-12 * abs(want)
    assert model.evaluate_generator(seq) == got


# ---- evaluate.py --------------------------------------------------------------------------------------------------------------
SAVED_CONFIG = '''"""A saved configuration as training.py copies it, shrunk to two synthetic batches of two images."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location("_resnet_config", os.path.join({root!r}, "config", "resnet", "config_file.py"))
_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mod)


class TrainingConfiguration(_mod.TrainingConfiguration):
    def __init__(self, *args, **kwargs):
        super(TrainingConfiguration, self).__init__(*args, **kwargs)
        self._batch_size = 2

    def prepare_testing_generator(self):
        self._test_generator = _mod.SyntheticDCTClassificationGenerator(self._batch_size, self.deconv, self.num_classes,
                                                                        n_batches=2, seed=3)
'''


def test_evaluate_entry_script(cuda, tmp_path):
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.networks.resnet_dct import ResNet50Custom
    experiment = tmp_path / "thomasC_deconv_key"
    (experiment / "config").mkdir(parents=True)
    (experiment / "checkpoints").mkdir()
    (experiment / "config" / "saved_config.py").write_text(SAVED_CONFIG.format(root=ROOT))
    K.clear_session()
    K.set_random_seed(3)
    weights = str(experiment / "checkpoints" / "epoch-01_loss-6.9000_val_loss-6.9000.h5")
    ResNet50Custom(weights=None, archi="deconv").save_weights(weights)
    env = dict(os.environ, DJ_AUTOTUNE="table")
    for var in ("WORLD_SIZE", "DJ_TEST_DIR", "DJ_VAL_DIR", "DJ_INDEX_FILE"):
        env.pop(var, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), str(experiment), weights, "--archi", "deconv"],
                       capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("The evaluated score is [")]
    assert len(lines) == 2 and lines[0] == lines[1], r.stdout[-1500:]       # print(evaluator), then display_results()
    score = [float(v) for v in lines[0][len("The evaluated score is ["):-2].split(",")]
    assert len(score) == 3 and np.isfinite(score[0]) and 0.0 <= score[1] <= score[2] <= 1.0
