"""keras.applications.imagenet_utils.preprocess_input, 'caffe' mode only (the mode of keras.applications.vgg16 and
resnet50): RGB -> BGR, then the ImageNet channel means subtracted, in float32.  Parity unpinned against
keras_applications; this module is the contract.  Unlike Keras it never writes into the caller's array."""
import numpy as np

from ...data.rgb_warp import CAFFE_MEAN, caffe_preprocess


def preprocess_input(x, data_format=None, mode="caffe", **kwargs):
    """A (..., 3) channels-last array (any dtype; integers become float32) -> float32: channels reversed, then
    [103.939, 116.779, 123.68] subtracted.  The mean is rounded to float32 first and the difference is rounded once."""
    if mode != "caffe":
        raise NotImplementedError("preprocess_input: mode=%r is not implemented (only 'caffe')" % (mode,))
    if data_format not in (None, "channels_last"):
        raise NotImplementedError("preprocess_input: data_format=%r is not implemented (only 'channels_last')" % (data_format,))
    x = np.asarray(x)
    if x.ndim < 1 or x.shape[-1] != 3:
        raise ValueError("preprocess_input: expected a channels-last array with 3 channels, got shape %s" % (x.shape,))
    return caffe_preprocess(x)


preprocess_input._dj_device_prep = 1      # data/rgb_warp.py:PREP_CAFFE -- what dj_rgb_warp runs in its place
__all__ = ["preprocess_input", "CAFFE_MEAN"]
