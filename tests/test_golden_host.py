"""CPU: the host-side box / matching / encoder / anchor code and the oracle's anchor restatement against
golden vectors produced by the reference's own numpy modules (tests/golden/make_fixtures.py)."""
import os

import numpy as np
import pytest

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRAIN = dict(img_height=300, img_width=300, n_classes=20, scales=[0.1, 0.2, 0.37, 0.54, 0.71, 0.88, 1.05],
             aspect_ratios_per_layer=[[1.0, 2.0, 0.5], [1.0, 2.0, 0.5, 3.0, 1.0 / 3.0], [1.0, 2.0, 0.5, 3.0, 1.0 / 3.0],
                                      [1.0, 2.0, 0.5, 3.0, 1.0 / 3.0], [1.0, 2.0, 0.5], [1.0, 2.0, 0.5]],
             two_boxes_for_ar1=True, steps=[8, 16, 32, 64, 100, 300], offsets=[0.5] * 6, clip_boxes=False,
             variances=[0.1, 0.1, 0.2, 0.2], matching_type="multi", pos_iou_threshold=0.5, neg_iou_limit=0.5,
             normalize_coords=True)
SIZES = {"custom": [(38, 38), (19, 19), (10, 10), (5, 5), (3, 3), (1, 1)],
         "identical": [(38, 38), (10, 10), (5, 5), (5, 5), (3, 3), (1, 1)]}


def load(name):
    with np.load(os.path.join(G, name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def split_gt(f):
    out, o = [], 0
    for n in f["gt_count"]:
        out.append(f["gt"][o:o + n] if n else np.zeros((0, 5)))
        o += n
    return out


def test_box_utils_match_reference():
    from jpeg_detection_resnet_ssd_amd.bounding_box_utils.bounding_box_utils import (convert_coordinates,
                                                                                    intersection_area, iou)
    f = load("box_utils.npz")
    a, b = f["a"], f["b"]
    for key, ref in f.items():
        if "__" in key:
            name, bp = key.split("__")
            np.testing.assert_allclose(convert_coordinates(a, 0, name, border_pixels=bp), ref, rtol=0, atol=1e-12)
    np.testing.assert_allclose(iou(a, b, coords="corners"), f["iou_corners_outer"], atol=1e-12)
    np.testing.assert_allclose(iou(a, a[::-1].copy(), coords="corners", mode="element-wise"), f["iou_corners_elem"],
                               atol=1e-12)
    np.testing.assert_allclose(iou(convert_coordinates(a, 0, "corners2centroids"),
                                   convert_coordinates(b, 0, "corners2centroids"), coords="centroids"),
                               f["iou_centroids_outer"], atol=1e-12)
    np.testing.assert_allclose(iou(convert_coordinates(a, 0, "corners2minmax"), convert_coordinates(b, 0, "corners2minmax"),
                                   coords="minmax", border_pixels="include"), f["iou_minmax_include"], atol=1e-12)
    np.testing.assert_allclose(intersection_area(a, b, coords="corners"), f["inter_corners"], atol=1e-9)
    with pytest.raises(ValueError):
        convert_coordinates(a, 0, "corners2nothing")
    with pytest.raises(ValueError):
        iou(a[None], b)


def test_matching_matches_reference():
    from jpeg_detection_resnet_ssd_amd.ssd_encoder_decoder.matching_utils import match_bipartite_greedy, match_multi
    f = load("matching.npz")
    np.testing.assert_array_equal(match_bipartite_greedy(f["weights"]), f["bipartite"])
    gi, ai = match_multi(f["weights"], 0.8)
    np.testing.assert_array_equal(gi, f["multi_gt"])
    np.testing.assert_array_equal(ai, f["multi_anchor"])


@pytest.mark.parametrize("key", ["custom", "identical"])
def test_encoder_and_anchors_match_reference(key):
    from jpeg_detection_resnet_ssd_amd.bounding_box_utils.anchor_boxes import anchor_boxes_for_map
    from jpeg_detection_resnet_ssd_amd.ssd_encoder_decoder.ssd_input_encoder import SSDInputEncoder
    from oracle import ssd_resnet_dct as oracle
    f = load("encoder_%s.npz" % key)
    enc = SSDInputEncoder(predictor_sizes=SIZES[key], **TRAIN)
    tmpl = enc.generate_encoding_template(1)[0]
    assert tmpl.shape == f["template"].shape == ({"custom": 8732, "identical": 6716}[key], 33)
    np.testing.assert_allclose(tmpl, f["template"], rtol=0, atol=1e-12)
    y = enc(split_gt(f))
    np.testing.assert_allclose(y, f["y_true"], rtol=0, atol=1e-10)
    cfg = oracle.TRAIN_SSD_ARGS
    for i, (h, w) in enumerate(SIZES[key]):
        ref = f["layer%d" % i]
        mine = anchor_boxes_for_map(300, 300, h, w, TRAIN["scales"][i], TRAIN["scales"][i + 1],
                                    TRAIN["aspect_ratios_per_layer"][i], True, TRAIN["steps"][i], TRAIN["offsets"][i],
                                    False, TRAIN["variances"], "centroids", True)
        np.testing.assert_allclose(mine[..., :4], ref, rtol=0, atol=1e-12)
        np.testing.assert_allclose(mine[..., 4:], np.broadcast_to(TRAIN["variances"], mine[..., 4:].shape))
        orc = oracle.anchor_boxes(h, w, cfg["scales"][i], cfg["scales"][i + 1], cfg["aspect_ratios"][i], cfg["steps"][i],
                                  cfg["offsets"][i])
        np.testing.assert_allclose(orc[..., :4], ref, rtol=0, atol=1e-12)


def test_encoder_other_coordinate_modes():
    from jpeg_detection_resnet_ssd_amd.ssd_encoder_decoder.ssd_input_encoder import DegenerateBoxError, SSDInputEncoder
    f = load("encoder_small_corners.npz")
    enc = SSDInputEncoder(img_height=300, img_width=300, n_classes=3, predictor_sizes=[(4, 4), (2, 2)], min_scale=0.2,
                          max_scale=0.8, aspect_ratios_global=[0.5, 1.0, 2.0], two_boxes_for_ar1=True, clip_boxes=True,
                          matching_type="bipartite", coords="corners", normalize_coords=False, neg_iou_limit=0.3)
    np.testing.assert_allclose(enc([f["gt"]]), f["y_true"], atol=1e-10)
    f = load("encoder_small_minmax.npz")
    enc = SSDInputEncoder(img_height=200, img_width=300, n_classes=3, predictor_sizes=[(4, 6), (2, 3)], min_scale=0.2,
                          max_scale=0.8, aspect_ratios_global=[0.5, 1.0, 2.0], two_boxes_for_ar1=False, coords="minmax",
                          normalize_coords=True)
    np.testing.assert_allclose(enc([f["gt"]]), f["y_true"], atol=1e-10)
    with pytest.raises(DegenerateBoxError):
        enc([np.array([[1, 50., 50., 40., 80.]])])
    with pytest.raises(ValueError):
        SSDInputEncoder(300, 300, 3, [(4, 4)], scales=[0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        SSDInputEncoder(300, 300, 3, [(4, 4)], variances=[0.1, 0.1, 0.2])


def test_encoder_small_family_options_match_reference():
    """Every option axis of the encoder (border pixels, pixel / normalised coordinates, clipping, background id, matching
    type, thresholds hit exactly, variances, steps / offsets) on the greedy-matching quirk, tie and border cases of
    tests/encode_cases.py: the host encoder reproduces what the reference's own encoder wrote, exactly."""
    import json
    from jpeg_detection_resnet_ssd_amd.ssd_encoder_decoder.ssd_input_encoder import SSDInputEncoder
    import encode_cases as ec
    f = load("encoder_small_options.npz")
    keys = sorted(k[:-len(".y_true")] for k in f if k.endswith(".y_true"))
    assert keys == sorted("%s.%s" % (o, e) for o in ec.OPTION_SETS
                          for e in ("cases", "threshold_pos", "threshold_neg", "twin"))
    seen = set()
    for key in keys:
        kwargs = json.loads(str(f[key + ".options"]))
        gt = split_gt({"gt": f[key + ".gt"], "gt_count": f[key + ".gt_count"]})
        y = SSDInputEncoder(**kwargs)(gt)
        assert y.shape == f[key + ".y_true"].shape and np.isfinite(y).all()
        np.testing.assert_array_equal(y, f[key + ".y_true"], err_msg=key)
        seen.add((kwargs["border_pixels"], kwargs["matching_type"]))
        opt, entry = key.rsplit(".", 1)
        if entry == "cases":            # the stored ground truth is what the cases build today
            now, _ = ec.batch(ec.small_encoder(**ec.OPTION_SETS[opt]), names=ec.GOLDEN_CASES)
            assert len(now) == len(gt) and all(np.array_equal(a, b) for a, b in zip(now, gt))
    assert {b for b, _ in seen} == {"half", "include", "exclude"} and {m for _, m in seen} == {"multi", "bipartite"}


def test_anchor_layer_agrees_with_encoder_template():
    """AnchorBoxes (model side) and SSDInputEncoder (target side) must produce the same anchors in the same order
    -- the contract between y_pred and y_true rows (keras_ssd300_dct_j2d_resnet.py:775-879 vs ssd_input_encoder.py:574-591)."""
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd import workloads
    K.clear_session()
    for archi, key in (("ssd_custom", "custom"), ("deconv", "identical")):
        model, sizes = workloads.build_ssd(archi, compile_model=False)
        assert [tuple(s) for s in sizes] == SIZES[key]
        rows = []
        for name in ["conv4_3_norm", "fc7", "conv6_2", "conv7_2", "conv8_2", "conv9_2"]:
            rows.append(model.get_layer(name + "_mbox_priorbox").anchors().reshape(-1, 8))
        anchors = np.concatenate(rows, axis=0)
        f = load("encoder_%s.npz" % key)
        np.testing.assert_allclose(anchors[:, :4], f["template"][:, -12:-8], atol=1e-12)
        np.testing.assert_allclose(anchors[:, 4:], f["template"][:, -4:], atol=1e-12)
