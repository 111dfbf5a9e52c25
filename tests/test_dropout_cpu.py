"""Dropout and the VGG-DCT classifiers without a GPU: the Philox4x32-10 host statement (keras/dropout.py) against
Random123's known answers, the mask's properties, the layer's surface, the structure of the lowered plans, the two
builders and the two configurations."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = dict(classes=10, filters=(32, 64, 64), fc_units=128, input_size=12)


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


@pytest.mark.parametrize("counter,key,expected", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, expected):
    from jpeg_detection_resnet_ssd_amd.keras.dropout import philox4x32_10
    assert _hex(philox4x32_10(counter, key)) == expected
    # vectorised: the same block among others
    ctr = [np.array([1, c, 2], dtype=np.uint32) for c in counter]
    out = philox4x32_10(ctr, key)
    assert all(o.dtype == np.uint32 and o.shape == (3,) for o in out)
    assert _hex([o[1] for o in out]) == expected


def test_keep_mask_is_a_pure_function_with_the_prefix_property():
    from jpeg_detection_resnet_ssd_amd.keras.dropout import dropout_keep_host
    full = dropout_keep_host(8192, 0.5, seed=17, rank=0, step=3)
    assert full.dtype == np.bool_ and full.shape == (8192,)
    assert np.array_equal(full, dropout_keep_host(8192, 0.5, seed=17, rank=0, step=3))
    assert np.array_equal(dropout_keep_host(5, 0.5, seed=17, rank=0, step=3), full[:5])
    assert np.array_equal(dropout_keep_host(1021, 0.5, seed=17, rank=0, step=3), full[:1021])
    for other in (dict(seed=17, rank=0, step=4), dict(seed=17, rank=1, step=3), dict(seed=18, rank=0, step=3),
                  dict(seed=17, rank=0, step=3 + 2 ** 32)):
        assert not np.array_equal(full, dropout_keep_host(8192, 0.5, **other)), other


@pytest.mark.parametrize("rate", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("seed", [1, 2024, 0xDEADBEEF])
def test_kept_share_is_one_minus_rate(rate, seed):
    """n Bernoulli(p = 1 - rate) draws: the kept share lies within five standard deviations, 5 sqrt(p (1 - p) / n)."""
    from jpeg_detection_resnet_ssd_amd.keras.dropout import dropout_keep_host
    n, p = 8192, 1.0 - rate
    share = float(dropout_keep_host(n, rate, seed=seed, rank=0, step=0).mean())
    assert abs(share - p) <= 5.0 * math.sqrt(p * (1.0 - p) / n), (share, p)


def test_threshold_rule_and_host_dropout():
    from jpeg_detection_resnet_ssd_amd.keras import dropout as D
    assert D.dropout_threshold(0.5) == 2 ** 31
    assert D.dropout_threshold(0) == 0 and D.dropout_keep_host(100, 0.0, 1, 0, 0).all()
    assert D.dropout_threshold(1.0 - 2.0 ** -40) == 2 ** 32 - 1
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            D.dropout_threshold(bad)
    # the kept elements are exactly those whose Philox word reaches the threshold
    words = np.stack(D.philox4x32_10((np.arange(2, dtype=np.uint32), 0, 3, 0), (17, 0)), axis=1).reshape(-1)
    assert np.array_equal(D.dropout_keep_host(8, 0.5, 17, 0, 3), words >= 2 ** 31)
    x = np.linspace(-2, 2, 8, dtype=np.float32)
    keep = D.dropout_keep_host(8, 0.5, 17, 0, 3)
    y = D.dropout_host(x, 0.5, 17, 0, 3)
    assert y.dtype == np.float32 and np.array_equal(y, np.where(keep, x * np.float32(2.0), x * np.float32(0.0)))
    # a product, not a select: Inf / NaN at a dropped position gives NaN
    dropped = int(np.flatnonzero(~keep)[0])
    x[dropped] = np.inf
    assert np.isnan(D.dropout_host(x, 0.5, 17, 0, 3)[dropped])


def test_layer_surface():
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras.layers import Dropout, Input
    for bad in (-0.01, 1.0, 2):
        with pytest.raises(ValueError):
            Dropout(bad)
    with pytest.raises(NotImplementedError):
        Dropout(0.5, noise_shape=(None, 1))
    K.clear_session()
    lyr = Dropout(0.25, seed=7)
    out = lyr(Input((4096,)))
    assert out.shape == (None, 4096) and lyr.output_shape == (None, 4096)
    assert lyr.weights == [] and lyr.count_params() == 0 and lyr.name == "dropout_1"
    assert lyr.get_config()["rate"] == 0.25 and lyr.seed == 7
    K.set_random_seed(5)
    a, b = Dropout(0.5).seed, Dropout(0.5).seed
    K.set_random_seed(5)
    assert (Dropout(0.5).seed, Dropout(0.5).seed) == (a, b) and a != b and 0 <= a < 2 ** 32
    K.set_random_seed(6)
    assert Dropout(0.5).seed != a


def _dropout_launches(launches):
    return [f.dj_entry for f in launches if hasattr(f, "dj_entry")]


@pytest.mark.parametrize("rate", [0.5, 0.0])
def test_plans_hold_one_forward_and_one_backward_launch_per_layer(monkeypatch, rate):
    """Lowered on the host: nothing runs."""
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras import layers as L
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import SGD
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.networks import vgg_dct
    monkeypatch.setenv("DJ_AUTOTUNE", "table")
    K.clear_session()
    K.set_random_seed(3)
    model = vgg_dct(dropout_rate=rate, **SMALL)
    model.compile(optimizer=SGD(lr=0.01, momentum=0.9, nesterov=True), loss="categorical_crossentropy")
    model._ensure_params(device=torch.device("cpu"))
    names = [l.name for l in model.layers if isinstance(l, L.Dropout)]
    assert len(names) == 2
    train = model._plan(4, True, True)
    expect = [] if rate == 0.0 else names
    assert _dropout_launches(train.fwd) == [("dj_dropout_fwd", n) for n in expect]
    assert _dropout_launches(train.bwd) == [("dj_dropout_bwd", n) for n in reversed(expect)]
    for plan in (model._plan(4, False, False), model._plan(4, False, True)):
        assert _dropout_launches(plan.fwd) == [] and plan.bwd == []
        for lyr in model.layers:
            if isinstance(lyr, L.Dropout):      # an alias of its input
                assert plan.values[id(lyr.outbound[0])] is plan.values[id(lyr.inbound[0])]
    if rate:
        for lyr in model.layers:
            if isinstance(lyr, L.Dropout):
                v = train.values[id(lyr.outbound[0])]
                assert v.buf.dtype == torch.float32 and v.buf.shape == (4, 128)
                assert v.buf.data_ptr() != train.values[id(lyr.inbound[0])].buf.data_ptr()


def test_a_16_bit_input_is_refused():
    from jpeg_detection_resnet_ssd_amd.engine import Plan, Value
    from jpeg_detection_resnet_ssd_amd.keras.layers import Dropout, Input
    lyr = Dropout(0.5, seed=1)
    lyr(Input((8,)))
    plan = Plan(torch.device("cpu"), 2, True)
    with pytest.raises(NotImplementedError, match="fp32"):
        lyr.lower(plan, None, [Value(torch.zeros(2, 8, dtype=torch.float16), needs_grad=True)])


VGG_NAMES = ["b_norm_64", "b_norm_128", "conv1_1_dct_256", "conv4_1", "conv4_2", "conv4_3", "pool4", "conv5_1", "conv5_2",
             "conv5_3", "pool5", "flatten", "fc1", "fc2", "predictions"]


@pytest.mark.parametrize("builder,params,third", [("vgga_dct", 132640744, False), ("vggd_dct", 137360360, True)])
def test_builders(builder, params, third):
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras import layers as L
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras import networks
    K.clear_session()
    model = getattr(networks, builder)()
    assert model.count_params() == params
    assert sum(w.size for w in model.weight_specs if not w.trainable) == 384
    assert [t.shape for t in model.inputs] == [(None, 28, 28, 64), (None, 14, 14, 128)]
    assert [t.shape for t in model.outputs] == [(None, 1000)]
    names = [l.name for l in model.layers]
    expect = [n for n in VGG_NAMES if third or not n.endswith("_3")]
    assert [n for n in names if n in VGG_NAMES] == expect
    assert model.get_layer("pool5").output_shape == (None, 7, 7, 512)
    assert model.get_layer("conv5_1").input_shape == (None, 14, 14, 640)
    drops = [l for l in model.layers if isinstance(l, L.Dropout)]
    assert [d.rate for d in drops] == [0.5, 0.5] and drops[0].seed != drops[1].seed
    assert names.index("fc1") < names.index(drops[0].name) < names.index("fc2") < names.index(drops[1].name)
    assert not any(w.l2 for w in model.weight_specs)


def _load_config(folder):
    spec = importlib.util.spec_from_file_location("cfg_" + folder, os.path.join(ROOT, "config", folder, "config_file.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("folder,project,params", [("vggA_dct", "vgg-dct", 132640744),
                                                   ("vggD_dct", "vggD-dct_retrain_for_weights", 137360360)])
def test_configurations_and_horovod_scaling_rules(folder, project, params):
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras import callbacks as cb
    K.clear_session()
    cfg = _load_config(folder).TrainingConfiguration()
    assert (cfg.batch_size, cfg.batch_size_divider, cfg.steps_per_epoch, cfg.epochs, cfg.validation_steps) == \
        (256, 4, 5000, 120, 50000 // 256)
    assert cfg.optimizer.get_config() == {"lr": 0.01, "momentum": 0.9, "decay": 0.0, "nesterov": True}
    assert cfg.project_name == project and cfg.network.count_params() == params
    assert getattr(cfg.loss, "_dj_loss", cfg.loss) == "categorical_crossentropy"
    assert [m._dj_metric for m in cfg.metrics] == [("top_k", 1), ("top_k", 5)]
    assert [type(c) for c in cfg.callbacks] == [cb.TerminateOnNaN, cb.EarlyStopping]
    assert cfg.early_stopping.monitor == "val_loss" and cfg.early_stopping.patience == 10
    assert cfg.weights is None and cfg.horovod is None

    class FakeHvd:
        class callbacks:
            BroadcastGlobalVariablesCallback = staticmethod(lambda r: ("bcast", r))
            MetricAverageCallback = staticmethod(lambda: "avg")
            LearningRateWarmupCallback = staticmethod(lambda warmup_epochs, verbose: ("warmup", warmup_epochs))

        @staticmethod
        def size():
            return 16

        @staticmethod
        def rank():
            return 0

        @staticmethod
        def DistributedOptimizer(o):
            return o
    cfg.prepare_horovod(FakeHvd)
    assert abs(cfg.optimizer.lr - 0.01 * 16 / 4) < 1e-12
    assert cfg.batch_size == 64 and cfg.steps_per_epoch == 5000 // 4 and cfg.validation_steps == 3 * 195 // 16
    assert cfg.callbacks[0] == ("bcast", 0) and cfg.callbacks[1] == "avg" and cfg.callbacks[2] == ("warmup", 5)
    assert isinstance(cfg.callbacks[3], cb.ReduceLROnPlateau) and cfg.callbacks[3].patience == 5
    cfg.prepare_training_generators()
    x, y = cfg.train_generator[0]
    assert [a.shape for a in x] == [(64, 28, 28, 64), (64, 14, 14, 128)] and y.shape == (64, 1000)
    xv, yv = cfg.validation_generator[0]
    assert [a.shape for a in xv] == [(64, 28, 28, 64), (64, 14, 14, 128)] and yv.shape == (64, 1000)
    cfg.prepare_testing_generator()
    cfg.prepare_evaluator()
    assert len(cfg.test_generator) == 8 and cfg.evaluator is not None
