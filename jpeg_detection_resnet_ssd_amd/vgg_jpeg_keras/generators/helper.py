"""The photometric augmentations the reference's classifier generators take as `transformations`
(classification_part/vgg_jpeg_keras/generators/helper.py:12-45; its default training configuration passes
`[lighting, contrast, brightness, saturation]`): numpy callables on an (H, W, 3) uint8 image that draw from `np.random`
and return uint8, clipped to [0, 255] and truncated.  Names, arguments, defaults and draws are the reference's.

The generators' device path recognises these four callables by identity and runs them on the GPU
(csrc/dj_photometric.hip) from the same draws: `draw_parameters` makes a callable's draw without applying it, through
the same `_alpha` the callables use, so the two cannot drift apart.

One departure from the reference for equal draws: `lighting` fixes the sign of each eigenvector after `eigh` (the
component of largest magnitude is made positive, the lowest index winning ties).  LAPACK does not specify the signs, so
the reference's result depends on the library build; the normal draws are symmetric, so the distribution is unchanged.
An image of a single pixel (the reference's covariance is undefined there) is returned unchanged."""
import numpy as np

from ...data import photometric as _ph

_WEIGHTS = np.array(_ph.GREY_WEIGHTS)


def _alpha(var, offset_var):
    """One uniform draw scaled to [1 - offset_var, 1 - offset_var + 2 * var)."""
    return 2 * np.random.random() * var + 1 - offset_var


def _to_u8(x):
    return np.clip(x, 0, 255).astype(np.uint8)          # clip, then truncate


def grayscale(rgb):
    """(H, W, 3) -> (H, W) float64 luma."""
    return np.dot(rgb, _WEIGHTS)


def saturation(rgb, saturation_var=0.5):
    """Blend each pixel with its own grey value."""
    grey = grayscale(rgb)
    a = _alpha(saturation_var, saturation_var)
    return _to_u8(a * rgb + (1 - a) * grey[..., None])


def brightness(rgb, brightness_var=0.5, saturation_var=0.5):
    """Scale the pixels.  The offset of alpha is 1 - saturation_var, not 1 - brightness_var: the reference's quirk, kept."""
    return _to_u8(_alpha(brightness_var, saturation_var) * rgb)


def contrast(rgb, contrast_var=0.5):
    """Blend each pixel with the image's mean grey value."""
    m = grayscale(rgb).mean()
    a = _alpha(contrast_var, contrast_var)
    return _to_u8(a * rgb + (1 - a) * m)


def lighting(img, lighting_std=0.5):
    """Shift the three channels along the principal axes of the image's colour covariance (pixels / 255), each axis by
    eigenvalue * normal draw * lighting_std; eigenvector signs fixed as the module docstring says."""
    n = np.random.randn(3) * lighting_std
    samples = img.reshape(-1, 3) / 255.0
    if samples.shape[0] < 2:
        return _to_u8(img)
    lam, vec = np.linalg.eigh(np.cov(samples, rowvar=False))
    return _to_u8(img + 255 * (_ph.fix_signs(vec) @ (lam * n)))


PHOTOMETRIC_CODES = {saturation: _ph.SATURATION, brightness: _ph.BRIGHTNESS, contrast: _ph.CONTRAST, lighting: _ph.LIGHTING}


def photometric_code(transformation):
    """The device operation code of one of the four callables above (by identity), None for anything else."""
    for fn, code in PHOTOMETRIC_CODES.items():
        if transformation is fn:
            return code
    return None


def draw_parameters(transformation):
    """The draw `transformation` (one of the four callables, with its default arguments) would make from `np.random`,
    as the device operation `(code, parameters)`."""
    code = photometric_code(transformation)
    if code is None:
        raise ValueError("%r is not one of saturation, brightness, contrast, lighting" % (transformation,))
    if code == _ph.LIGHTING:
        return code, tuple(float(v) for v in np.random.randn(3) * 0.5)          # lighting_std's default
    return code, (float(_alpha(0.5, 0.5)),)
