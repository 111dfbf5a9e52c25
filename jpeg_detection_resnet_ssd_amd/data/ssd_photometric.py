"""The photometric part of the SSD300 training augmentation: `SSDPhotometricDistortions` and what it is made of, restated
from the reference's localisation_part/data_generator (data_augmentation_chain_original_ssd.py:146-206,
object_detection_2d_photometric_ops.py) with its constructor arguments, its defaults and its order of `np.random` draws.

`ssd_photometric_host(image, params)` is the pixel contract: one (H, W, 3) uint8 image and the drawn parameters of one
call -> the distorted image, in numpy.  csrc/dj_ssd_photometric.hip reproduces it byte for byte, in place on the staged
rectangles of a ragged batch (`kernels.ssd_photometric`, called from data/patch_resize.py before dj_patch_resize).  Every
operation is pointwise (the contrast is about the constant 127.5, not the image's mean), so distorting the staged part of an
image equals distorting the image and cutting the part out.

What decides bits:

  float32      between uint8 images the reference computes in float32 (`image.astype(np.float32)`), and a Python-float
               parameter combines with a float32 array as float32.  Every drawn parameter is stored as `np.float32` once;
               that value is used on the host and on the GPU.  Each operation rounds on its own (no fused multiply-add).
  to uint8     `np.round(x).astype(np.uint8)`: round half to even.
  hue          `np.remainder(H + delta, 180.0)` in float32: the sum of H = 0 and a tiny negative delta is lifted by 180 and
               rounds to exactly 180.0, so the byte 180 is a legal hue for HSV -> RGB and is kept.
  round trip   RGB -> HSV -> RGB runs even when no operation was drawn, as in the reference, and changes pixels: over all
               2^24 colours by up to 5 levels, 1.046 on average.

The colour conversions are OpenCV's 8-bit ones (`cv2.cvtColor` with COLOR_RGB2HSV / COLOR_HSV2RGB, H in 0..180), RESTATED
here from their formulas: there is no OpenCV on the machines this package is developed on, so -- as with the resize, which
is Pillow's -- this module is the contract, not a particular cv2 build.  tests/test_ssd_photometric_cpu.py compares with
cv2 where it is installed.

  RGB -> HSV   integers with 12 fractional bits.  sdiv[i] = rint((255 << 12) / i), hdiv[i] = rint((180 << 12) / (6 i)) for
               i = 1..255, entry 0 = 0.  v = max(r, g, b), d = v - min(r, g, b), S = (d * sdiv[v] + 2048) >> 12; the hue
               term is g - b when v == r, else b - r + 2 d when v == g, else r - g + 4 d (ties are decided in that order);
               H = (term * hdiv[d] + 2048) >> 12 with an arithmetic shift, + 180 when negative.
  HSV -> RGB   float32.  s = S * (1.f / 255.f), v = V * (1.f / 255.f); s == 0: r = g = b = v.  Otherwise h = fmodf(H * (6.f /
               180.f), 6.f), sector = floor(h), f = h - sector (a sector outside 0..5: sector 0, f = 0), tab = {v, v (1 - s),
               v (1 - s f), v (1 - s (1 - f))}, (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}][sector];
               each channel clip(rint(x * 255.f), 0, 255).

`Gamma` and `HistogramEqualization` are not restated: the reference's chains do not use them."""
from collections import namedtuple

import numpy as np

_F = np.float32
HSV_SHIFT = 12
_I = np.arange(1, 256, dtype=np.float64)
SDIV = np.concatenate([[0], np.rint((255 << HSV_SHIFT) / _I)]).astype(np.int32)
HDIV = np.concatenate([[0], np.rint((180 << HSV_SHIFT) / (6.0 * _I))]).astype(np.int32)
_SECTORS = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]], dtype=np.intp)      # (b, g, r)
_ORDERS = {(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)}

BRIGHTNESS, CONTRAST, SATURATION, HUE = 1, 2, 4, 8      # DJ_SSD_PHOTO_* of include/dj_hip.h: bits of `flags`
# dj_ssd_photo_params (include/dj_hip.h), C layout
PARAMS_DTYPE = np.dtype([("sequence", np.int32), ("flags", np.int32), ("brightness", np.float32), ("contrast", np.float32),
                         ("saturation", np.float32), ("hue", np.float32), ("order", np.int32, (3,)), ("reserved", np.int32)],
                        align=True)

PhotoParams = namedtuple("PhotoParams", "sequence brightness contrast saturation hue order")
PhotoParams.__doc__ = """The draws of one `SSDPhotometricDistortions` call: `sequence` 1 or 2, `brightness` (delta), `contrast`
(factor), `saturation` (factor) and `hue` (delta) each an `np.float32` or None when the operation was not drawn, `order` the
channel order after the swap, a permutation of (0, 1, 2)."""


def _check_image(image):
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("expected an (H, W, 3) uint8 image, got %s %s" % (image.dtype, image.shape))
    return image


def check_params(params):
    """-> a `PhotoParams` with plain ints, `np.float32` parameters (None: off) and a tuple for the order; ValueError for a
    sequence other than 1 or 2, a parameter that is not finite or an order that is no permutation of (0, 1, 2)."""
    p = PhotoParams(*params)
    if p.sequence not in (1, 2):
        raise ValueError("sequence must be 1 or 2, got %r" % (p.sequence,))
    values = []
    for name in ("brightness", "contrast", "saturation", "hue"):
        v = getattr(p, name)
        if v is not None:
            v = _F(v)
            if not np.isfinite(v):
                raise ValueError("%s: the parameter %r is not finite" % (name, getattr(p, name)))
        values.append(v)
    order = tuple(int(c) for c in p.order)
    if order not in _ORDERS:
        raise ValueError("order must be a permutation of (0, 1, 2), got %r" % (p.order,))
    return PhotoParams(int(p.sequence), *values, order)


# ---- the colour conversions -------------------------------------------------------------------------------------------------
def rgb_to_hsv_host(rgb):
    """OpenCV's 8-bit COLOR_RGB2HSV, restated: (..., 3) uint8 RGB -> uint8 (H in 0..179, S, V)."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.shape[-1] == 3, "expected an (..., 3) uint8 array"
    r, g, b = (rgb[..., c].astype(np.int32) for c in range(3))
    v = np.maximum(np.maximum(r, g), b)
    d = v - np.minimum(np.minimum(r, g), b)
    s = (d * SDIV[v] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    term = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (term * HDIV[d] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    h = h + np.where(h < 0, 180, 0)
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


def hsv_to_rgb_host(hsv):
    """OpenCV's 8-bit COLOR_HSV2RGB, restated: (..., 3) uint8 (H, S, V) -> uint8 RGB.  Any byte is accepted for H: the
    hue wraps (180 is 0)."""
    hsv = np.asarray(hsv)
    assert hsv.dtype == np.uint8 and hsv.shape[-1] == 3, "expected an (..., 3) uint8 array"
    scale = _F(1.0) / _F(255.0)
    h = np.fmod(hsv[..., 0].astype(_F) * (_F(6.0) / _F(180.0)), _F(6.0))
    s = hsv[..., 1].astype(_F) * scale
    v = hsv[..., 2].astype(_F) * scale
    sector = np.floor(h)
    f = h - sector
    sector = sector.astype(np.int32)
    outside = (sector < 0) | (sector > 5)
    sector = np.where(outside, 0, sector)
    f = np.where(outside, _F(0.0), f)
    one = _F(1.0)
    tab = np.stack([v, v * (one - s), v * (one - s * f), v * (one - s * (one - f))], axis=-1)
    bgr = np.take_along_axis(tab, _SECTORS[sector], axis=-1)
    bgr = np.where((s == 0)[..., None], v[..., None], bgr)
    out = np.clip(np.rint(bgr * _F(255.0)), 0, 255).astype(np.uint8)
    return out[..., ::-1]


# ---- the pixel contract -----------------------------------------------------------------------------------------------------
def _to_uint8(x):
    return np.round(x, decimals=0).astype(np.uint8)


def _brightness(x, delta):
    return np.clip(x + delta, 0, 255)


def _contrast(x, factor):
    return np.clip(_F(127.5) + factor * (x - _F(127.5)), 0, 255)


def _saturation(x, factor):
    x[..., 1] = np.clip(x[..., 1] * factor, 0, 255)
    return x


def _hue(x, delta):
    x[..., 0] = np.remainder(x[..., 0] + delta, _F(180.0))
    return x


def ssd_photometric_host(image, params):
    """`SSDPhotometricDistortions` with its draws made: the (H, W, 3) uint8 image after
       sequence 1: brightness, contrast, ->u8, RGB->HSV, saturation, hue, ->u8, HSV->RGB, channel order
       sequence 2: brightness, ->u8, RGB->HSV, saturation, hue, ->u8, HSV->RGB, contrast, ->u8, channel order
    with every operation that `params` leaves at None skipped and everything between uint8 images in float32."""
    image = _check_image(image)
    p = check_params(params)
    x = image.astype(_F)
    if p.brightness is not None:
        x = _brightness(x, p.brightness)
    if p.sequence == 1 and p.contrast is not None:
        x = _contrast(x, p.contrast)
    x = rgb_to_hsv_host(_to_uint8(x)).astype(_F)
    if p.saturation is not None:
        x = _saturation(x, p.saturation)
    if p.hue is not None:
        x = _hue(x, p.hue)
    x = hsv_to_rgb_host(_to_uint8(x))
    if p.sequence == 2:
        x = x.astype(_F)
        if p.contrast is not None:
            x = _contrast(x, p.contrast)
        x = _to_uint8(x)
    return np.ascontiguousarray(x[:, :, list(p.order)])


def pack_params(params):
    """A list of per-image `PhotoParams` -> the PARAMS_DTYPE array dj_ssd_photometric reads (parameters of operations that
    are off are zero)."""
    params = [check_params(p) for p in params]
    arr = np.zeros(len(params), dtype=PARAMS_DTYPE)
    for i, p in enumerate(params):
        arr["sequence"][i] = p.sequence
        for name, bit in (("brightness", BRIGHTNESS), ("contrast", CONTRAST), ("saturation", SATURATION), ("hue", HUE)):
            v = getattr(p, name)
            if v is not None:
                arr["flags"][i] |= bit
                arr[name][i] = v
        arr["order"][i] = p.order
    return arr


# ---- object_detection_2d_photometric_ops.py ---------------------------------------------------------------------------------
def _returns(image, labels):
    return image if labels is None else (image, labels)


class ConvertColor(object):
    """Converts uint8 images between RGB and HSV (`rgb_to_hsv_host` / `hsv_to_rgb_host`); the reference's grayscale
    targets are not restated."""

    def __init__(self, current='RGB', to='HSV', keep_3ch=True):
        if not ((current in {'RGB', 'HSV'}) and (to in {'RGB', 'HSV', 'GRAY'})):
            raise NotImplementedError
        if to == 'GRAY':
            raise NotImplementedError("ConvertColor: the conversions to GRAY are not restated")
        self.current = current
        self.to = to
        self.keep_3ch = keep_3ch

    def __call__(self, image, labels=None):
        if self.current == 'RGB' and self.to == 'HSV':
            image = rgb_to_hsv_host(image)
        elif self.current == 'HSV' and self.to == 'RGB':
            image = hsv_to_rgb_host(image)
        return _returns(image, labels)


class ConvertDataType(object):
    """Converts images between uint8 (rounding half to even) and float32."""

    def __init__(self, to='uint8'):
        if not (to == 'uint8' or to == 'float32'):
            raise ValueError("`to` can be either of 'uint8' or 'float32'.")
        self.to = to

    def __call__(self, image, labels=None):
        if self.to == 'uint8':
            image = np.round(image, decimals=0).astype(np.uint8)
        else:
            image = image.astype(np.float32)
        return _returns(image, labels)


class ConvertTo3Channels(object):
    """1-channel and 4-channel images become 3-channel images (the fourth channel is dropped); others pass."""

    def __init__(self):
        pass

    def __call__(self, image, labels=None):
        if image.ndim == 2:
            image = np.stack([image] * 3, axis=-1)
        elif image.ndim == 3:
            if image.shape[2] == 1:
                image = np.concatenate([image] * 3, axis=-1)
            elif image.shape[2] == 4:
                image = image[:, :, :3]
        return _returns(image, labels)


class Hue(object):
    """Adds `delta` to the hue of a float HSV image, modulo 180."""

    def __init__(self, delta):
        if not (-180 <= delta <= 180):
            raise ValueError("`delta` must be in the closed interval `[-180, 180]`.")
        self.delta = delta

    def __call__(self, image, labels=None):
        image[:, :, 0] = (image[:, :, 0] + self.delta) % 180.0
        return _returns(image, labels)


class _RandomOp(object):
    """The coin every random operation of the reference tosses: `uniform(0, 1)`, and when p >= 1 - prob the parameter's
    draw (`_draw`).  `draw()` makes both without touching a pixel -> the parameter, or None."""

    def draw(self):
        p = np.random.uniform(0, 1)
        if p >= (1.0 - self.prob):
            return self._draw()
        return None

    def __call__(self, image, labels=None):
        value = self.draw()
        if value is None:
            return _returns(image, labels)
        setattr(self._op, self._name, value)
        return self._op(image, labels)


class RandomHue(_RandomOp):
    _name = 'delta'

    def __init__(self, max_delta=18, prob=0.5):
        if not (0 <= max_delta <= 180):
            raise ValueError("`max_delta` must be in the closed interval `[0, 180]`.")
        self.max_delta = max_delta
        self.prob = prob
        self.change_hue = self._op = Hue(delta=0)

    def _draw(self):
        return np.float32(np.random.uniform(-self.max_delta, self.max_delta))


class Saturation(object):
    """Multiplies the saturation of a float HSV image by `factor`, clipped to 0..255."""

    def __init__(self, factor):
        if factor <= 0.0:
            raise ValueError("It must be `factor > 0`.")
        self.factor = factor

    def __call__(self, image, labels=None):
        image[:, :, 1] = np.clip(image[:, :, 1] * self.factor, 0, 255)
        return _returns(image, labels)


class RandomSaturation(_RandomOp):
    _name = 'factor'

    def __init__(self, lower=0.3, upper=2.0, prob=0.5):
        if lower >= upper:
            raise ValueError("`upper` must be greater than `lower`.")
        self.lower = lower
        self.upper = upper
        self.prob = prob
        self.change_saturation = self._op = Saturation(factor=1.0)

    def _draw(self):
        return np.float32(np.random.uniform(self.lower, self.upper))


class Brightness(object):
    """Adds `delta` to every channel of a float RGB image, clipped to 0..255."""

    def __init__(self, delta):
        self.delta = delta

    def __call__(self, image, labels=None):
        image = np.clip(image + self.delta, 0, 255)
        return _returns(image, labels)


class RandomBrightness(_RandomOp):
    _name = 'delta'

    def __init__(self, lower=-84, upper=84, prob=0.5):
        if lower >= upper:
            raise ValueError("`upper` must be greater than `lower`.")
        self.lower = float(lower)
        self.upper = float(upper)
        self.prob = prob
        self.change_brightness = self._op = Brightness(delta=0)

    def _draw(self):
        return np.float32(np.random.uniform(self.lower, self.upper))


class Contrast(object):
    """Scales a float RGB image about 127.5 by `factor`, clipped to 0..255."""

    def __init__(self, factor):
        if factor <= 0.0:
            raise ValueError("It must be `factor > 0`.")
        self.factor = factor

    def __call__(self, image, labels=None):
        image = np.clip(127.5 + self.factor * (image - 127.5), 0, 255)
        return _returns(image, labels)


class RandomContrast(_RandomOp):
    _name = 'factor'

    def __init__(self, lower=0.5, upper=1.5, prob=0.5):
        if lower >= upper:
            raise ValueError("`upper` must be greater than `lower`.")
        self.lower = lower
        self.upper = upper
        self.prob = prob
        self.change_contrast = self._op = Contrast(factor=1.0)

    def _draw(self):
        return np.float32(np.random.uniform(self.lower, self.upper))


class ChannelSwap(object):
    """Reorders the channels: output channel k is input channel `order[k]`."""

    def __init__(self, order):
        self.order = order

    def __call__(self, image, labels=None):
        image = image[:, :, self.order]
        return _returns(image, labels)


class RandomChannelSwap(_RandomOp):
    _name = 'order'

    def __init__(self, prob=0.5):
        self.prob = prob
        # every permutation of the three channels except the original order
        self.permutations = ((0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
        self.swap_channels = self._op = ChannelSwap(order=(0, 1, 2))

    def _draw(self):
        return self.permutations[np.random.randint(5)]


# ---- data_augmentation_chain_original_ssd.py --------------------------------------------------------------------------------
class SSDPhotometricDistortions(object):
    """The photometric distortions of the original Caffe SSD's `train_transform_param`: brightness +-32, contrast,
    saturation 0.5 .. 1.5 and hue +-18, each with probability 0.5, in one of two orders chosen by `np.random.choice(2)`
    (1: sequence 1), and a channel swap of probability 0 that still tosses its coin.

    `__call__(image, labels)` runs the sequence on pixels as the reference does.  `draw()` makes the same `np.random`
    calls in the same order and returns them as a `PhotoParams`; `apply(image, params)` is `ssd_photometric_host`, so
    `apply(image, draw())` under one seed gives what the call gives."""

    def __init__(self):
        self.convert_RGB_to_HSV = ConvertColor(current='RGB', to='HSV')
        self.convert_HSV_to_RGB = ConvertColor(current='HSV', to='RGB')
        self.convert_to_float32 = ConvertDataType(to='float32')
        self.convert_to_uint8 = ConvertDataType(to='uint8')
        self.convert_to_3_channels = ConvertTo3Channels()
        self.random_brightness = RandomBrightness(lower=-32, upper=32, prob=0.5)
        self.random_contrast = RandomContrast(lower=0.5, upper=1.5, prob=0.5)
        self.random_saturation = RandomSaturation(lower=0.5, upper=1.5, prob=0.5)
        self.random_hue = RandomHue(max_delta=18, prob=0.5)
        self.random_channel_swap = RandomChannelSwap(prob=0.0)

        self.sequence1 = [self.convert_to_3_channels,
                          self.convert_to_float32,
                          self.random_brightness,
                          self.random_contrast,
                          self.convert_to_uint8,
                          self.convert_RGB_to_HSV,
                          self.convert_to_float32,
                          self.random_saturation,
                          self.random_hue,
                          self.convert_to_uint8,
                          self.convert_HSV_to_RGB,
                          self.random_channel_swap]

        self.sequence2 = [self.convert_to_3_channels,
                          self.convert_to_float32,
                          self.random_brightness,
                          self.convert_to_uint8,
                          self.convert_RGB_to_HSV,
                          self.convert_to_float32,
                          self.random_saturation,
                          self.random_hue,
                          self.convert_to_uint8,
                          self.convert_HSV_to_RGB,
                          self.convert_to_float32,
                          self.random_contrast,
                          self.convert_to_uint8,
                          self.random_channel_swap]

    def __call__(self, image, labels=None):
        sequence = self.sequence1 if np.random.choice(2) else self.sequence2
        for transform in sequence:
            image = transform(image)
        return _returns(np.ascontiguousarray(image), labels)

    def draw(self):
        """The draws of one call, no pixel touched -> `PhotoParams`."""
        drawn = {}
        if np.random.choice(2):
            sequence, ops = 1, ("brightness", "contrast", "saturation", "hue")
        else:
            sequence, ops = 2, ("brightness", "saturation", "hue", "contrast")
        for name in ops:
            drawn[name] = getattr(self, "random_" + name).draw()
        order = self.random_channel_swap.draw()
        return PhotoParams(sequence, drawn["brightness"], drawn["contrast"], drawn["saturation"], drawn["hue"],
                           (0, 1, 2) if order is None else tuple(order))

    @staticmethod
    def apply(image, params):
        return ssd_photometric_host(image, params)
