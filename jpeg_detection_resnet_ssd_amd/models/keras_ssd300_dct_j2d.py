"""SSD300 over the VGG-DCT backbone: `ssd_300DCT`, drop-in for the builder of
localisation_part/models/keras_ssd300_dct_j2d.py:31-470 (the detector of "Fast object detection in compressed JPEG
images") -- same keyword arguments, validation errors, layer names and predictor order.  The backbone is the one of the
`vggd_dct` classifier (vgg_jpeg_keras/networks/vgg_dct.py) up to conv5_3, so a classifier checkpoint loads into it by
name; `pool5_ssd`, the dilated `fc6`, `fc7` and the stock SSD extra layers follow.

Inputs are the de-quantised JPEG DCT coefficients jpeg2dct emits for a 300x300 image, Y (38, 38, 64) and
CbCr (19, 19, 128), whatever `image_size` says: that argument only feeds the anchors and the decoder.
Output: (batch, 8732, n_classes + 1 + 4 + 8) = [softmax class scores | 4 box offsets | 4 anchor coordinates | 4 variances].

`ssd_300DCT_no_reg` (keras_ssd300_dct_j2d_no_regularizer.py) is the same graph built by `_ssd_300dct(regularized=False)`."""
from ..keras.layers import BatchNormalization, Concatenate, Conv2D, Input, MaxPooling2D, ZeroPadding2D
from ..keras_layers.keras_layer_L2Normalization import L2Normalization
from .keras_ssd300_dct_j2d_resnet import _check_ssd_arguments, _head_conv, _multibox

_PER_LAYER_RATIOS = [[1.0, 2.0, 0.5], [1.0, 2.0, 0.5, 3.0, 1.0 / 3.0], [1.0, 2.0, 0.5, 3.0, 1.0 / 3.0],
                     [1.0, 2.0, 0.5, 3.0, 1.0 / 3.0], [1.0, 2.0, 0.5], [1.0, 2.0, 0.5]]


def _backbone_conv(x, filters, name):
    """VGG convolution as the reference writes it: 3x3, 'same', fused ReLU, Keras' default initialiser, no regulariser
    (in either builder) and no BatchNormalization."""
    return Conv2D(filters, (3, 3), activation="relu", padding="same", name=name)(x)


def _ssd_300dct(regularized, image_size, n_classes, mode, l2_regularization, min_scale, max_scale, scales,
                aspect_ratios_global, aspect_ratios_per_layer, two_boxes_for_ar1, steps, offsets, clip_boxes, variances,
                coords, normalize_coords, confidence_thresh, iou_threshold, top_k, nms_max_output_size,
                return_predictor_sizes):
    n_predictor_layers = 6
    n_classes += 1
    l2_reg = l2_regularization

    def extra(x, filters, kernel, name, **kw):
        """fc6 .. conv9_2: he_normal and l2(l2_reg), or, without `regularized`, Keras' defaults as the no_reg builder has them."""
        return _head_conv(x, filters, kernel, name, l2_reg, regularized=regularized, **kw)

    img_height, img_width = image_size[0], image_size[1]
    scales, aspect_ratios, n_boxes, steps, offsets, variances = _check_ssd_arguments(
        n_predictor_layers, min_scale, max_scale, scales, aspect_ratios_global, aspect_ratios_per_layer,
        two_boxes_for_ar1, steps, offsets, variances)

    input_y = Input((38, 38, 64))
    input_cbcr = Input((19, 19, 128))
    norm_cbcr = BatchNormalization(name="b_norm_128")(input_cbcr)
    x = BatchNormalization(name="b_norm_64")(input_y)
    x = _backbone_conv(x, 256, "conv1_1_dct_256")
    x = _backbone_conv(x, 512, "conv4_1")
    x = _backbone_conv(x, 512, "conv4_2")
    conv4_3 = _backbone_conv(x, 512, "conv4_3")
    x = MaxPooling2D((2, 2), strides=(2, 2), name="pool4")(conv4_3)
    x = Concatenate(axis=-1)([x, norm_cbcr])
    x = _backbone_conv(x, 512, "conv5_1")
    x = _backbone_conv(x, 512, "conv5_2")
    x = _backbone_conv(x, 512, "conv5_3")
    pool5 = MaxPooling2D((3, 3), strides=(1, 1), padding="same", name="pool5_ssd")(x)

    fc6 = extra(pool5, 1024, (3, 3), "fc6", dilation=(6, 6))
    fc7 = extra(fc6, 1024, (1, 1), "fc7")
    conv6_1 = extra(fc7, 256, (1, 1), "conv6_1")
    conv6_1 = ZeroPadding2D(padding=((1, 1), (1, 1)), name="conv6_padding")(conv6_1)
    conv6_2 = extra(conv6_1, 512, (3, 3), "conv6_2", strides=(2, 2), padding="valid")
    conv7_1 = extra(conv6_2, 128, (1, 1), "conv7_1")
    conv7_1 = ZeroPadding2D(padding=((1, 1), (1, 1)), name="conv7_padding")(conv7_1)
    conv7_2 = extra(conv7_1, 256, (3, 3), "conv7_2", strides=(2, 2), padding="valid")   # 10x10 -> 5x5
    conv8_1 = extra(conv7_2, 128, (1, 1), "conv8_1")
    conv8_2 = extra(conv8_1, 256, (3, 3), "conv8_2", padding="valid")
    conv9_1 = extra(conv8_2, 128, (1, 1), "conv9_1")
    conv9_2 = extra(conv9_1, 256, (3, 3), "conv9_2", padding="valid")
    conv4_3_norm = L2Normalization(gamma_init=20, name="conv4_3_norm")(conv4_3)
    sources = [conv4_3_norm, fc7, conv6_2, conv7_2, conv8_2, conv9_2]
    decode_args = dict(confidence_thresh=confidence_thresh, iou_threshold=iou_threshold, top_k=top_k,
                       nms_max_output_size=nms_max_output_size, coords=coords, normalize_coords=normalize_coords,
                       img_height=img_height, img_width=img_width)
    return _multibox(sources, [input_y, input_cbcr], n_classes, n_boxes, l2_reg, img_height, img_width, scales,
                     aspect_ratios, two_boxes_for_ar1, steps, offsets, clip_boxes, variances, coords, normalize_coords,
                     mode, return_predictor_sizes, decode_args, regularized=regularized)


def ssd_300DCT(image_size, n_classes, mode="training", l2_regularization=0.0005, min_scale=None, max_scale=None,
               scales=None, aspect_ratios_global=None, aspect_ratios_per_layer=_PER_LAYER_RATIOS, two_boxes_for_ar1=True,
               steps=[8, 16, 32, 64, 100, 300], offsets=None, clip_boxes=False, variances=[0.1, 0.1, 0.2, 0.2],
               coords="centroids", normalize_coords=True, subtract_mean=[123, 117, 104], divide_by_stddev=None,
               swap_channels=[2, 1, 0], confidence_thresh=0.01, iou_threshold=0.45, top_k=200, nms_max_output_size=400,
               return_predictor_sizes=False):
    """VGG-DCT SSD300: predictors on conv4_3 (38x38x512, L2-normalised), fc7 (19x19), conv6_2 (10x10), conv7_2 (5x5),
    conv8_2 (3x3) and conv9_2 (1x1): 8732 boxes.  fc6 .. conv9_2 and the twelve predictor convolutions carry
    l2(l2_regularization) and he_normal, the backbone neither.  `subtract_mean`, `divide_by_stddev` and `swap_channels`
    are accepted and unused: the reference defines their Lambda functions and never applies them to the DCT inputs."""
    return _ssd_300dct(True, image_size, n_classes, mode, l2_regularization, min_scale, max_scale, scales,
                       aspect_ratios_global, aspect_ratios_per_layer, two_boxes_for_ar1, steps, offsets, clip_boxes,
                       variances, coords, normalize_coords, confidence_thresh, iou_threshold, top_k, nms_max_output_size,
                       return_predictor_sizes)
