"""SSDInputEncoder on the GPU (dj_ssd_encode_targets) against the reference-generated golden encodings and against
the host numpy encoder: random and adversarial ground truth on the SSD300 anchor sets, and every named case of
tests/encode_cases.py (greedy-matching quirk, redo loop, index edges, ties, exact thresholds, caps, batch shapes, class ids)
plus a seeded sweep under every option set of the small 68-anchor family."""
import os

import numpy as np
import pytest
import torch

import encode_cases as ec
from encode_cases import SIZES, encoder

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
OPTS = list(ec.OPTION_SETS)


def assert_rows(dev, want, n_cls, msg=""):
    # class vectors, anchors, variances: exact (index work); offsets: <= 1 float32 ulp (device log vs libm log)
    np.testing.assert_array_equal(dev[..., :n_cls], want[..., :n_cls], err_msg=msg)
    np.testing.assert_array_equal(dev[..., -8:], want[..., -8:], err_msg=msg)
    np.testing.assert_allclose(dev[..., n_cls:n_cls + 4], want[..., n_cls:n_cls + 4], rtol=2.4e-7, atol=1e-12, err_msg=msg)


def compare(enc, gt):
    host = enc(gt)
    dev = enc.encode_on_device(gt).cpu().numpy()
    want = host.astype(np.float32)
    assert np.isfinite(want).all()
    assert_rows(dev, want, enc.n_classes)
    return host, dev


@pytest.mark.parametrize("which", ["custom", "identical"])
def test_encoder_against_reference_fixture(which):
    g = np.load(os.path.join(GOLD, "encoder_%s.npz" % which), allow_pickle=False)
    counts, flat = g["gt_count"], g["gt"]
    gt, k = [], 0
    for c in counts:                       # ragged ground truth stored flat + counts
        gt.append(flat[k:k + int(c)])
        k += int(c)
    enc = encoder(SIZES[which])
    dev = enc.encode_on_device(gt).cpu().numpy()
    want = g["y_true"].astype(np.float32)
    np.testing.assert_array_equal(dev[..., :21], want[..., :21])
    np.testing.assert_array_equal(dev[..., -8:], want[..., -8:])
    np.testing.assert_allclose(dev[..., 21:25], want[..., 21:25], rtol=2.4e-7, atol=1e-12)


def test_encoder_random_batches():
    from jpeg_detection_resnet_ssd_amd.data import synthetic_dct as sd
    enc = encoder(SIZES["custom"])
    for seed in (1, 2, 3):
        host, dev = compare(enc, sd.random_ground_truth(8, seed=seed))
    assert (host[..., 1:21].sum(-1) > 0).sum() > 0


def test_encoder_adversarial_ground_truth():
    rng = np.random.default_rng(0)
    # identical boxes (ties between ground truths), boxes on anchor centres, 60 boxes in one image, an empty image
    same = np.array([[3, 50, 60, 150, 200], [7, 50, 60, 150, 200], [9, 50, 60, 150, 200]], dtype=float)
    grid = np.array([[1 + (i % 20), 8 * i + 0.0, 8 * i + 0.0, 8 * i + 30.0, 8 * i + 30.0] for i in range(30)])
    many = []
    for _ in range(60):
        x0, y0 = rng.uniform(0, 250, 2)
        w, h = rng.uniform(20, 50, 2)
        many.append([rng.integers(1, 21), x0, y0, min(x0 + w, 300), min(y0 + h, 300)])
    gt = [same, grid, np.array(many), np.zeros((0, 5)), np.array([[5, 0, 0, 300, 300]], dtype=float)]
    compare(encoder(SIZES["custom"]), gt)
    compare(encoder(SIZES["identical"], neg_iou_limit=0.3), gt)                 # neutral boxes exist
    compare(encoder(SIZES["custom"], matching_type="bipartite", neg_iou_limit=0.4), gt)


def test_encoder_errors_and_out_buffer():
    from jpeg_detection_resnet_ssd_amd.ssd_encoder_decoder.ssd_input_encoder import DegenerateBoxError
    enc = encoder(SIZES["custom"])
    with pytest.raises(DegenerateBoxError):
        enc.encode_on_device([np.array([[1, 10, 10, 10, 50]], dtype=float)])
    out = torch.full((2, 8732, 33), -5.0, device="cuda")
    gt = [np.array([[2, 10, 20, 110, 220]], dtype=float), np.zeros((0, 5))]
    r = enc.encode_on_device(gt, out=out)
    assert r.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(out.cpu().numpy()[..., :21], enc(gt).astype(np.float32)[..., :21])


def test_training_step_with_device_encoded_targets():
    """train_on_batch fed with PendingTargets (DeviceLabelEncoder) == fed with the host-encoded numpy y_true."""
    from jpeg_detection_resnet_ssd_amd import workloads
    from jpeg_detection_resnet_ssd_amd.data import synthetic_dct as sd
    from jpeg_detection_resnet_ssd_amd.ssd_encoder_decoder.ssd_input_encoder import DeviceLabelEncoder
    losses = []
    for device_side in (False, True):
        model, sizes = workloads.build_ssd("ssd_custom")
        enc = workloads.make_encoder(sizes)
        x = sd.dct_batch(2, seed=5, split_chroma=False)
        gt = sd.random_ground_truth(2, seed=5)
        y = DeviceLabelEncoder(enc)(gt) if device_side else enc(gt).astype(np.float32)
        losses.append(model.train_on_batch(x, y))
    assert abs(losses[0] - losses[1]) <= 1e-5 * abs(losses[0])


# ---- every option set x every named case, one launch per option set -------------------------------------------------
_BATCHES = {}


def encoded_batch(opt):
    """(encoder, host float32, device, spans) of all the named cases under one option set: one host pass, one launch (a
    workgroup per image), `out=` pre-filled with NaN."""
    if opt not in _BATCHES:
        enc = ec.small_encoder(**ec.OPTION_SETS[opt])
        images, spans = ec.batch(enc)
        want = enc(images).astype(np.float32)
        out = torch.full(want.shape, float("nan"), device="cuda")
        r = enc.encode_on_device(images, out=out)
        assert r.data_ptr() == out.data_ptr()
        _BATCHES[opt] = (enc, want, out.cpu().numpy(), spans)
    return _BATCHES[opt]


@pytest.mark.parametrize("case", list(ec.CASES))
@pytest.mark.parametrize("opt", OPTS)
def test_named_case_under_option_set(opt, case):
    enc, want, dev, spans = encoded_batch(opt)
    (a, b), = [(a, b) for name, a, b in spans if name == case]
    assert b > a and np.isfinite(want[a:b]).all()
    assert not np.isnan(dev[a:b]).any()                      # every element of the NaN-filled `out=` was overwritten
    assert_rows(dev[a:b], want[a:b], enc.n_classes, "%s / %s" % (opt, case))     # anchor 0 of the quirk cases included


@pytest.mark.parametrize("opt", OPTS)
def test_threshold_and_twin_cases(opt):
    o = ec.OPTION_SETS[opt]
    for which in ("pos", "neg"):
        enc, images, a, _ = ec.threshold_case(which, **o)
        host, dev = compare(enc, images)
        cls = dev[0, a, :enc.n_classes]
        assert cls.sum() == (1 if which == "pos" else 0) and cls[enc.background_id] == 0     # IoU == threshold counts
    enc, images, a = ec.twin_case(**o)
    host, dev = compare(enc, images)
    assert dev[0, a, enc.background_id] == 0 and (dev[0, a, -8:] == dev[0, a + 1, -8:]).all()


@pytest.mark.parametrize("opt", OPTS)
def test_seeded_sweep(opt):
    enc = ec.small_encoder(**ec.OPTION_SETS[opt])
    images = ec.sweep(enc, seed=100 + OPTS.index(opt))
    assert len(images) == ec.SWEEP_IMAGES >= 300
    host, dev = compare(enc, images)
    n = enc.n_classes
    fg = np.delete(host[..., :n], enc.background_id, axis=-1).sum(-1) > 0
    assert fg.sum() > ec.SWEEP_IMAGES and (host[..., :n].sum(-1) == 0).any() == \
        (enc.matching_type == "bipartite" or enc.neg_iou_limit < enc.pos_iou_threshold)


def test_ssd300_index_edges_cap_and_quirk():
    """Best anchors at 0, 8731 and the workgroup stride (1023 / 1024); exactly 128 distinct boxes in one image; the reported
    divergence (a matched box 0, then a box outside every anchor), under both matching types."""
    for over in (dict(), dict(matching_type="bipartite", neg_iou_limit=0.4)):
        enc = encoder(SIZES["custom"], **over)
        images, spans = ec.batch(enc, ec.SSD300_CASES)
        assert max(len(g) for g in images) == 128
        want = enc(images).astype(np.float32)
        out = torch.full(want.shape, float("nan"), device="cuda")
        dev = enc.encode_on_device(images, out=out).cpu().numpy()
        for name, a, b in spans:
            assert_rows(dev[a:b], want[a:b], enc.n_classes, "%s / %s" % (sorted(over.items()), name))


def test_caps_refuse_before_any_launch():
    from jpeg_detection_resnet_ssd_amd._lib import DjError
    enc = ec.small_encoder()
    (full,) = ec.CASES["cap_128"](enc)
    over = np.concatenate([full, full[:1]])
    out = torch.full((1, ec.SMALL_ANCHORS, enc.n_classes + 12), float("nan"), device="cuda")
    with pytest.raises(DjError, match="at most 128 ground-truth boxes"):
        enc.encode_on_device([over], out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                            # nothing was launched
    compare(enc, [full])                                     # exactly the cap is served
    big = ec.small_encoder(predictor_sizes=[(56, 56), (2, 2), (1, 1)])
    n = big.generate_encoding_template(1).shape[1]
    assert n > 12288
    out = torch.full((1, n, big.n_classes + 12), float("nan"), device="cuda")
    with pytest.raises(DjError, match="more than 12288 anchor boxes"):
        big.encode_on_device([full[:3]], out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_batch_shapes():
    enc = ec.small_encoder(neg_iou_limit=0.3)
    empty = np.zeros((0, 5))
    host, dev = compare(enc, [empty, empty, empty])                       # an all-empty batch
    assert (dev[..., enc.background_id] == 1).all() and (dev[..., enc.n_classes:enc.n_classes + 4] == 0).all()
    (full,) = ec.CASES["cap_128"](enc)
    one = ec.rows([1, 5, 5, 40, 30])
    gt = [empty, full, one, empty, full[:7], one]                         # 0, 128, 1, 0, 7, 1 boxes: padding rows are ignored
    host, dev = compare(enc, gt)
    np.testing.assert_array_equal(dev[2], dev[5])
    np.testing.assert_array_equal(dev[0], dev[3])
    host1, dev1 = compare(enc, [one])                                     # the same image alone: max_gt = 1
    np.testing.assert_array_equal(dev1[0], dev[2])


def test_out_buffer_is_overwritten_in_every_column():
    enc = encoder(SIZES["custom"])
    out = torch.full((2, 8732, 33), float("nan"), device="cuda")
    gt = [np.array([[2, 10, 20, 110, 220]], dtype=float), np.zeros((0, 5))]
    r = enc.encode_on_device(gt, out=out)
    assert r.data_ptr() == out.data_ptr()
    dev = out.cpu().numpy()
    assert not np.isnan(dev).any()
    assert_rows(dev, enc(gt).astype(np.float32), 21)


@pytest.mark.parametrize("coords", ["corners", "minmax"])
def test_other_coordinate_modes_stay_unimplemented(coords):
    enc = ec.small_encoder(coords=coords, normalize_coords=False)
    with pytest.raises(NotImplementedError):
        enc.encode_on_device([ec.rows([1, 5, 5, 40, 30])])
