"""`ssd_300DCT_no_reg`, drop-in for localisation_part/models/keras_ssd300_dct_j2d_no_regularizer.py: the graph of
`ssd_300DCT` (keras_ssd300_dct_j2d.py) in which no layer carries a kernel regulariser and every convolution keeps Keras'
default initialiser.  `l2_regularization` is accepted and unused, as in the reference."""
from .keras_ssd300_dct_j2d import _PER_LAYER_RATIOS, _ssd_300dct


def ssd_300DCT_no_reg(image_size, n_classes, mode="training", l2_regularization=0.0005, min_scale=None, max_scale=None,
                      scales=None, aspect_ratios_global=None, aspect_ratios_per_layer=_PER_LAYER_RATIOS,
                      two_boxes_for_ar1=True, steps=[8, 16, 32, 64, 100, 300], offsets=None, clip_boxes=False,
                      variances=[0.1, 0.1, 0.2, 0.2], coords="centroids", normalize_coords=True,
                      subtract_mean=[123, 117, 104], divide_by_stddev=None, swap_channels=[2, 1, 0],
                      confidence_thresh=0.01, iou_threshold=0.45, top_k=200, nms_max_output_size=400,
                      return_predictor_sizes=False):
    return _ssd_300dct(False, image_size, n_classes, mode, l2_regularization, min_scale, max_scale, scales,
                       aspect_ratios_global, aspect_ratios_per_layer, two_boxes_for_ar1, steps, offsets, clip_boxes,
                       variances, coords, normalize_coords, confidence_thresh, iou_threshold, top_k, nms_max_output_size,
                       return_predictor_sizes)
