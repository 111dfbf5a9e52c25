"""The SSD300 training augmentation: `SSDDataAugmentation` and the geometric transforms it is made of, restated from the
reference's localisation_part/data_generator (data_augmentation_chain_original_ssd.py, ..._no_crop.py,
object_detection_2d_patch_sampling_ops.py, object_detection_2d_image_boxes_validation_utils.py,
object_detection_2d_geometric_ops.py) with its constructor arguments, its defaults and its order of `np.random` draws, so
that under one seed the boxes come out as the reference's (tests/golden/ssd_augment.npz).

Every transform runs in two modes.  Called with an image it returns pixels, as the reference does.  Called with a
`Geometry` in place of the image -- which is what `plan(height, width, labels)` does -- it makes the same draws and the
same label arithmetic and touches no pixel: expand, crop and flip compose into one window of the source image on a
constant background, which `data/patch_resize.py` then resamples on the host (`patch_resize_host`) or on the GPU
(`DevicePatchResize`).

The photometric stage, `SSDPhotometricDistortions`, lives in data/ssd_photometric.py and is re-exported here.  Given to a
chain's `photometric_distortions` slot it runs first, as in the reference: on pixels in the chain's call, and as a drawn
`PhotoParams` record in `plan(..., return_photometric=True)`, which `ssd_photometric_host` or the GPU (dj_ssd_photometric,
before the window is cut) then applies.  The chains' default leaves the slot empty.

Two departures from the reference, both on the pixel side only:
  * the resize is Pillow's, not OpenCV's (no OpenCV here to pin it to): the five interpolation codes the chain draws from
    map to NEAREST, BILINEAR, BICUBIC, BOX and LANCZOS (`CV2_TO_PILLOW`).  Pillow antialiases when it shrinks, OpenCV's
    linear and cubic modes do not;
  * the colour conversions of the photometric stage are the in-tree restatement of OpenCV's 8-bit formulas
    (data/ssd_photometric.py), not calls into a cv2 build.
The slot also takes any other host callable `(image, labels) -> (image, labels)`; such a callable cannot be planned."""
import inspect

import numpy as np

from ..bounding_box_utils.bounding_box_utils import iou
from . import patch_resize as _pr
from .patch_resize import patch_resize_host, resize_host, window_host      # noqa: F401  (the pixel contract, re-exported)
from .ssd_photometric import SSDPhotometricDistortions, ssd_photometric_host      # noqa: F401  (the photometric stage)

# OpenCV's interpolation codes, which the reference's constructors take, and the Pillow filter each one runs as here
INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA, INTER_LANCZOS4 = 0, 1, 2, 3, 4
CV2_TO_PILLOW = {INTER_NEAREST: _pr.NEAREST, INTER_LINEAR: _pr.BILINEAR, INTER_CUBIC: _pr.BICUBIC, INTER_AREA: _pr.BOX,
                 INTER_LANCZOS4: _pr.LANCZOS}
_LABELS_FORMAT = {'class_id': 0, 'xmin': 1, 'ymin': 2, 'xmax': 3, 'ymax': 4}


def pillow_filter(interpolation_mode):
    try:
        return CV2_TO_PILLOW[int(interpolation_mode)]
    except (KeyError, TypeError, ValueError):
        raise ValueError("interpolation mode %r is not one of INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA, "
                         "INTER_LANCZOS4 (0..4)" % (interpolation_mode,))


# ---- planning mode: the image that is not there -----------------------------------------------------------------------------
class Geometry(object):
    """Stands in for the image while a chain is planned: the current picture is the window (y0, x0, h, w) of a source image
    of (src_h, src_w) on `background`, mirrored left-right when `flip` is set and resized with `filter` to `out_size`
    once a resize has been planned.  `shape` is what `image.shape` would be."""

    def __init__(self, src_h, src_w, window=None, flip=False, filter=None, background=None, out_size=None):
        self.src_h, self.src_w = int(src_h), int(src_w)
        self.y0, self.x0, self.h, self.w = (0, 0, self.src_h, self.src_w) if window is None else (int(v) for v in window)
        self.flip, self.filter, self.background, self.out_size = bool(flip), filter, background, out_size

    @property
    def shape(self):
        return (self.out_size if self.out_size is not None else (self.h, self.w)) + (3,)

    ndim = 3

    def astuple(self):
        """(win_y0, win_x0, win_h, win_w, flip, filter, background) of data/patch_resize.py; filter None: no resize yet."""
        return (self.y0, self.x0, self.h, self.w, self.flip, self.filter,
                tuple(int(c) for c in self.background) if self.background is not None else (0, 0, 0))

    @classmethod
    def fromtuple(cls, src_h, src_w, geometry):
        y0, x0, h, w, flip, filt, background = geometry
        return cls(src_h, src_w, (y0, x0, h, w), flip, filt, tuple(background))

    def _open(self, what):
        if self.filter is not None:
            raise ValueError("%s after a resize cannot be planned as one window of the source image" % what)

    def crop_pad(self, ymin, xmin, height, width, background):
        self._open("a crop or a padding")
        inside = ymin >= 0 and xmin >= 0 and ymin + height <= self.h and xmin + width <= self.w
        bg = self.background
        if not inside:
            # what the new window shows outside the current one is background, so the current one must show the whole
            # source image, and whatever padding it already shows must be of the same colour
            covers = self.y0 <= 0 and self.x0 <= 0 and self.y0 + self.h >= self.src_h and self.x0 + self.w >= self.src_w
            padded = (self.h, self.w) != (self.src_h, self.src_w)
            new = tuple(int(c) for c in background)
            if not covers or (padded and bg is not None and tuple(bg) != new):
                raise ValueError("a padding after a crop, or in another colour than an earlier padding, cannot be planned "
                                 "as one window of the source image")
            bg = new
        x = self.w - (xmin + width) if self.flip else xmin
        return Geometry(self.src_h, self.src_w, (self.y0 + ymin, self.x0 + x, height, width), self.flip, None, bg)

    def mirror(self):
        self._open("a flip")
        return Geometry(self.src_h, self.src_w, (self.y0, self.x0, self.h, self.w), not self.flip, None, self.background)

    def resize(self, out_height, out_width, filter):
        self._open("a second resize")
        return Geometry(self.src_h, self.src_w, (self.y0, self.x0, self.h, self.w), self.flip, filter, self.background,
                        (int(out_height), int(out_width)))


def _planned(image):
    return isinstance(image, Geometry)


class _Plannable(object):
    def plan(self, height, width, labels=None, geometry=None, return_inverter=False):
        """The draws and the label arithmetic of `self(image, labels)` for an image of (height, width), no pixel touched
        -> what the call returns with the geometry (win_y0, win_x0, win_h, win_w, flip, filter, background) in place of
        the image: (geometry, labels[, inverter]), or without labels `geometry` / (geometry, inverter); None when the
        transform gives up (`can_fail`).  `geometry`: what earlier transforms planned for the same source image, to
        compose with.  `return_inverter` is for the transforms whose call takes it."""
        start = Geometry(height, width) if geometry is None else Geometry.fromtuple(height, width, geometry)
        args = (start,) if labels is None else (start, labels)
        out = self(*args, return_inverter=True) if return_inverter else self(*args)
        out = out if isinstance(out, tuple) else (out,)
        if out[0] is None:
            return None
        out = (out[0].astuple(),) + tuple(out[1:])
        return out if len(out) > 1 else out[0]


# ---- object_detection_2d_image_boxes_validation_utils.py --------------------------------------------------------------------
class BoundGenerator(object):
    """Draws (lower, upper) bound pairs from a sample space; None stands for 0.0 / 1.0."""

    def __init__(self, sample_space=((0.1, None), (0.3, None), (0.5, None), (0.7, None), (0.9, None), (None, None)),
                 weights=None):
        if (not (weights is None)) and len(weights) != len(sample_space):
            raise ValueError("`weights` must either be `None` for uniform distribution or have the same length as `sample_space`.")
        self.sample_space = []
        for bound_pair in sample_space:
            if len(bound_pair) != 2:
                raise ValueError("All elements of the sample space must be 2-tuples.")
            bound_pair = list(bound_pair)
            if bound_pair[0] is None:
                bound_pair[0] = 0.0
            if bound_pair[1] is None:
                bound_pair[1] = 1.0
            if bound_pair[0] > bound_pair[1]:
                raise ValueError("For all sample space elements, the lower bound cannot be greater than the upper bound.")
            self.sample_space.append(bound_pair)
        self.sample_space_size = len(self.sample_space)
        self.weights = [1.0 / self.sample_space_size] * self.sample_space_size if weights is None else weights

    def __call__(self):
        i = np.random.choice(self.sample_space_size, p=self.weights)
        return self.sample_space[i]


class BoxFilter(object):
    """Returns the boxes that meet the overlap / minimum-area / non-degeneracy criteria with respect to an image size."""

    def __init__(self, check_overlap=True, check_min_area=True, check_degenerate=True, overlap_criterion='center_point',
                 overlap_bounds=(0.3, 1.0), min_area=16, labels_format=_LABELS_FORMAT, border_pixels='half'):
        if not isinstance(overlap_bounds, (list, tuple, BoundGenerator)):
            raise ValueError("`overlap_bounds` must be either a 2-tuple of scalars or a `BoundGenerator` object.")
        if isinstance(overlap_bounds, (list, tuple)) and (overlap_bounds[0] > overlap_bounds[1]):
            raise ValueError("The lower bound must not be greater than the upper bound.")
        if not (overlap_criterion in {'iou', 'area', 'center_point'}):
            raise ValueError("`overlap_criterion` must be one of 'iou', 'area', or 'center_point'.")
        self.overlap_criterion = overlap_criterion
        self.overlap_bounds = overlap_bounds
        self.min_area = min_area
        self.check_overlap = check_overlap
        self.check_min_area = check_min_area
        self.check_degenerate = check_degenerate
        self.labels_format = labels_format
        self.border_pixels = border_pixels

    def __call__(self, labels, image_height=None, image_width=None):
        labels = np.copy(labels)
        xmin, ymin = self.labels_format['xmin'], self.labels_format['ymin']
        xmax, ymax = self.labels_format['xmax'], self.labels_format['ymax']
        requirements_met = np.ones(shape=labels.shape[0], dtype=bool)
        if self.check_degenerate:
            requirements_met *= (labels[:, xmax] > labels[:, xmin]) * (labels[:, ymax] > labels[:, ymin])
        if self.check_min_area:
            requirements_met *= (labels[:, xmax] - labels[:, xmin]) * (labels[:, ymax] - labels[:, ymin]) >= self.min_area
        if self.check_overlap:
            if isinstance(self.overlap_bounds, BoundGenerator):
                lower, upper = self.overlap_bounds()
            else:
                lower, upper = self.overlap_bounds
            if self.overlap_criterion == 'iou':
                image_coords = np.array([0, 0, image_width, image_height])
                image_boxes_iou = iou(image_coords, labels[:, [xmin, ymin, xmax, ymax]], coords='corners',
                                      mode='element-wise', border_pixels=self.border_pixels)
                requirements_met *= (image_boxes_iou > lower) * (image_boxes_iou <= upper)
            elif self.overlap_criterion == 'area':
                d = {'half': 0, 'include': 1, 'exclude': -1}[self.border_pixels]
                box_areas = (labels[:, xmax] - labels[:, xmin] + d) * (labels[:, ymax] - labels[:, ymin] + d)
                clipped_boxes = np.copy(labels)
                clipped_boxes[:, [ymin, ymax]] = np.clip(labels[:, [ymin, ymax]], a_min=0, a_max=image_height - 1)
                clipped_boxes[:, [xmin, xmax]] = np.clip(labels[:, [xmin, xmax]], a_min=0, a_max=image_width - 1)
                intersection_areas = ((clipped_boxes[:, xmax] - clipped_boxes[:, xmin] + d)
                                      * (clipped_boxes[:, ymax] - clipped_boxes[:, ymin] + d))
                if lower == 0.0:
                    mask_lower = intersection_areas > lower * box_areas
                else:
                    mask_lower = intersection_areas >= lower * box_areas
                mask_upper = intersection_areas <= upper * box_areas
                requirements_met *= mask_lower * mask_upper
            elif self.overlap_criterion == 'center_point':
                cy = (labels[:, ymin] + labels[:, ymax]) / 2
                cx = (labels[:, xmin] + labels[:, xmax]) / 2
                requirements_met *= (cy >= 0.0) * (cy <= image_height - 1) * (cx >= 0.0) * (cx <= image_width - 1)
        return labels[requirements_met]


class ImageValidator(object):
    """True when at least `n_boxes_min` boxes (or 'all') meet the overlap requirement with an image of the given size."""

    def __init__(self, overlap_criterion='center_point', bounds=(0.3, 1.0), n_boxes_min=1, labels_format=_LABELS_FORMAT,
                 border_pixels='half'):
        if not ((isinstance(n_boxes_min, int) and n_boxes_min > 0) or n_boxes_min == 'all'):
            raise ValueError("`n_boxes_min` must be a positive integer or 'all'.")
        self.overlap_criterion = overlap_criterion
        self.bounds = bounds
        self.n_boxes_min = n_boxes_min
        self.labels_format = labels_format
        self.border_pixels = border_pixels
        self.box_filter = BoxFilter(check_overlap=True, check_min_area=False, check_degenerate=False,
                                    overlap_criterion=self.overlap_criterion, overlap_bounds=self.bounds,
                                    labels_format=self.labels_format, border_pixels=self.border_pixels)

    def __call__(self, labels, image_height, image_width):
        self.box_filter.overlap_bounds = self.bounds
        self.box_filter.labels_format = self.labels_format
        valid_labels = self.box_filter(labels=labels, image_height=image_height, image_width=image_width)
        if isinstance(self.n_boxes_min, int):
            return len(valid_labels) >= self.n_boxes_min
        return len(valid_labels) == len(labels)


# ---- object_detection_2d_patch_sampling_ops.py ------------------------------------------------------------------------------
class PatchCoordinateGenerator(object):
    """Draws (ymin, xmin, height, width) of a patch: two of height, width and aspect ratio are drawn or fixed
    (`must_match`), the third follows, then the position, so that patch and image overlap as much as possible."""

    def __init__(self, img_height=None, img_width=None, must_match='h_w', min_scale=0.3, max_scale=1.0,
                 scale_uniformly=False, min_aspect_ratio=0.5, max_aspect_ratio=2.0, patch_ymin=None, patch_xmin=None,
                 patch_height=None, patch_width=None, patch_aspect_ratio=None):
        if not (must_match in {'h_w', 'h_ar', 'w_ar'}):
            raise ValueError("`must_match` must be either of 'h_w', 'h_ar' and 'w_ar'.")
        if min_scale >= max_scale:
            raise ValueError("It must be `min_scale < max_scale`.")
        if min_aspect_ratio >= max_aspect_ratio:
            raise ValueError("It must be `min_aspect_ratio < max_aspect_ratio`.")
        if scale_uniformly and not ((patch_height is None) and (patch_width is None)):
            raise ValueError("If `scale_uniformly == True`, `patch_height` and `patch_width` must both be `None`.")
        self.img_height = img_height
        self.img_width = img_width
        self.must_match = must_match
        self.min_scale = min_scale
        self.max_scale = max_scale
        self.scale_uniformly = scale_uniformly
        self.min_aspect_ratio = min_aspect_ratio
        self.max_aspect_ratio = max_aspect_ratio
        self.patch_ymin = patch_ymin
        self.patch_xmin = patch_xmin
        self.patch_height = patch_height
        self.patch_width = patch_width
        self.patch_aspect_ratio = patch_aspect_ratio

    def __call__(self):
        if self.must_match == 'h_w':
            if not self.scale_uniformly:
                if self.patch_height is None:
                    patch_height = int(np.random.uniform(self.min_scale, self.max_scale) * self.img_height)
                else:
                    patch_height = self.patch_height
                if self.patch_width is None:
                    patch_width = int(np.random.uniform(self.min_scale, self.max_scale) * self.img_width)
                else:
                    patch_width = self.patch_width
            else:
                scaling_factor = np.random.uniform(self.min_scale, self.max_scale)
                patch_height = int(scaling_factor * self.img_height)
                patch_width = int(scaling_factor * self.img_width)
        elif self.must_match == 'h_ar':
            if self.patch_height is None:
                patch_height = int(np.random.uniform(self.min_scale, self.max_scale) * self.img_height)
            else:
                patch_height = self.patch_height
            if self.patch_aspect_ratio is None:
                patch_aspect_ratio = np.random.uniform(self.min_aspect_ratio, self.max_aspect_ratio)
            else:
                patch_aspect_ratio = self.patch_aspect_ratio
            patch_width = int(patch_height * patch_aspect_ratio)
        elif self.must_match == 'w_ar':
            if self.patch_width is None:
                patch_width = int(np.random.uniform(self.min_scale, self.max_scale) * self.img_width)
            else:
                patch_width = self.patch_width
            if self.patch_aspect_ratio is None:
                patch_aspect_ratio = np.random.uniform(self.min_aspect_ratio, self.max_aspect_ratio)
            else:
                patch_aspect_ratio = self.patch_aspect_ratio
            patch_height = int(patch_width / patch_aspect_ratio)

        if self.patch_ymin is None:
            # a negative range: the patch is taller than the image and is placed so that it contains it
            y_range = self.img_height - patch_height
            patch_ymin = np.random.randint(0, y_range + 1) if y_range >= 0 else np.random.randint(y_range, 1)
        else:
            patch_ymin = self.patch_ymin
        if self.patch_xmin is None:
            x_range = self.img_width - patch_width
            patch_xmin = np.random.randint(0, x_range + 1) if x_range >= 0 else np.random.randint(x_range, 1)
        else:
            patch_xmin = self.patch_xmin
        return (patch_ymin, patch_xmin, patch_height, patch_width)


def _returns(image, labels, inverter, return_inverter):
    out = (image,) if labels is None else (image, labels)
    if return_inverter:
        out = out + (inverter,)
    return out if len(out) > 1 else out[0]


def _identity_inverter(labels):
    return labels


# `device_form`: what an inverter computes, for eval_utils/device_matching.py to run it on the GPU (dj_eval_collect)
_identity_inverter.device_form = ("identity",)


class CropPad(_Plannable):
    """Takes the patch (patch_ymin, patch_xmin, patch_height, patch_width), given in the image's coordinates, out of the
    image: cropped where the patch lies inside, padded with `background` where it does not."""

    def __init__(self, patch_ymin, patch_xmin, patch_height, patch_width, clip_boxes=True, box_filter=None,
                 background=(0, 0, 0), labels_format=_LABELS_FORMAT):
        if not (isinstance(box_filter, BoxFilter) or box_filter is None):
            raise ValueError("`box_filter` must be either `None` or a `BoxFilter` object.")
        self.patch_height = patch_height
        self.patch_width = patch_width
        self.patch_ymin = patch_ymin
        self.patch_xmin = patch_xmin
        self.clip_boxes = clip_boxes
        self.box_filter = box_filter
        self.background = background
        self.labels_format = labels_format

    def __call__(self, image, labels=None, return_inverter=False):
        img_height, img_width = image.shape[:2]
        if (self.patch_ymin > img_height) or (self.patch_xmin > img_width):
            raise ValueError("The given patch doesn't overlap with the input image.")
        if labels is not None:
            labels = np.copy(labels)
        xmin, ymin = self.labels_format['xmin'], self.labels_format['ymin']
        xmax, ymax = self.labels_format['xmax'], self.labels_format['ymax']
        patch_ymin, patch_xmin = self.patch_ymin, self.patch_xmin

        if _planned(image):
            image = image.crop_pad(patch_ymin, patch_xmin, self.patch_height, self.patch_width, self.background)
        else:
            if image.ndim != 3:
                raise ValueError("expected an (H, W, 3) image")
            # a canvas of the patch's size filled with the background, the part of the image under it pasted in
            image = window_host(image, (patch_ymin, patch_xmin, self.patch_height, self.patch_width, False, None,
                                        self.background))

        def inverter(labels):
            labels = np.copy(labels)
            labels[:, [ymin + 1, ymax + 1]] += patch_ymin
            labels[:, [xmin + 1, xmax + 1]] += patch_xmin
            return labels

        if labels is not None:
            labels[:, [ymin, ymax]] -= patch_ymin
            labels[:, [xmin, xmax]] -= patch_xmin
            if not (self.box_filter is None):
                self.box_filter.labels_format = self.labels_format
                labels = self.box_filter(labels=labels, image_height=self.patch_height, image_width=self.patch_width)
            if self.clip_boxes:
                labels[:, [ymin, ymax]] = np.clip(labels[:, [ymin, ymax]], a_min=0, a_max=self.patch_height - 1)
                labels[:, [xmin, xmax]] = np.clip(labels[:, [xmin, xmax]], a_min=0, a_max=self.patch_width - 1)
        return _returns(image, labels, inverter, return_inverter)


class _PatchSampler(_Plannable):
    def _try(self, image, labels, return_inverter):
        """One candidate patch: drawn, checked against the validator, taken -> the transform's return value, or None."""
        xmin, ymin = self.labels_format['xmin'], self.labels_format['ymin']
        xmax, ymax = self.labels_format['xmax'], self.labels_format['ymax']
        patch_ymin, patch_xmin, patch_height, patch_width = self.patch_coord_generator()
        self.sample_patch.patch_ymin = patch_ymin
        self.sample_patch.patch_xmin = patch_xmin
        self.sample_patch.patch_height = patch_height
        self.sample_patch.patch_width = patch_width
        if self.check_aspect_ratio:
            aspect_ratio = patch_width / patch_height
            if not (self.patch_coord_generator.min_aspect_ratio <= aspect_ratio <= self.patch_coord_generator.max_aspect_ratio):
                return None
        if (labels is None) or (self.image_validator is None):
            return self.sample_patch(image, labels, return_inverter)
        new_labels = np.copy(labels)
        new_labels[:, [ymin, ymax]] -= patch_ymin
        new_labels[:, [xmin, xmax]] -= patch_xmin
        if self.image_validator(labels=new_labels, image_height=patch_height, image_width=patch_width):
            return self.sample_patch(image, labels, return_inverter)
        return None

    def _prepare(self, image):
        img_height, img_width = image.shape[:2]
        self.patch_coord_generator.img_height = img_height
        self.patch_coord_generator.img_width = img_width
        if not self.image_validator is None:
            self.image_validator.labels_format = self.labels_format
        self.sample_patch.labels_format = self.labels_format


class RandomPatch(_PatchSampler):
    """With probability `prob`, up to `n_trials_max` candidate patches; the first valid one is taken.  Without a valid
    one: the unaltered image, or Nones with `can_fail`."""
    check_aspect_ratio = False

    def __init__(self, patch_coord_generator, box_filter=None, image_validator=None, n_trials_max=3, clip_boxes=True,
                 prob=1.0, background=(0, 0, 0), can_fail=False, labels_format=_LABELS_FORMAT):
        if not isinstance(patch_coord_generator, PatchCoordinateGenerator):
            raise ValueError("`patch_coord_generator` must be an instance of `PatchCoordinateGenerator`.")
        if not (isinstance(image_validator, ImageValidator) or image_validator is None):
            raise ValueError("`image_validator` must be either `None` or an `ImageValidator` object.")
        self.patch_coord_generator = patch_coord_generator
        self.box_filter = box_filter
        self.image_validator = image_validator
        self.n_trials_max = n_trials_max
        self.clip_boxes = clip_boxes
        self.prob = prob
        self.background = background
        self.can_fail = can_fail
        self.labels_format = labels_format
        self.sample_patch = CropPad(patch_ymin=None, patch_xmin=None, patch_height=None, patch_width=None,
                                    clip_boxes=self.clip_boxes, box_filter=self.box_filter, background=self.background,
                                    labels_format=self.labels_format)

    def __call__(self, image, labels=None, return_inverter=False):
        p = np.random.uniform(0, 1)
        if p >= (1.0 - self.prob):
            self._prepare(image)
            for _ in range(max(1, self.n_trials_max)):
                out = self._try(image, labels, return_inverter)
                if out is not None:
                    return out
            if self.can_fail:
                n_outputs = 1 + (labels is not None) + bool(return_inverter)      # one None in place of each output
                return (None,) * n_outputs if n_outputs > 1 else None
            return _returns(image, labels, None, return_inverter)
        return _returns(image, labels, _identity_inverter, return_inverter)


class RandomPatchInf(_PatchSampler):
    """As `RandomPatch`, but it goes on until a valid patch is found or the coin returns the image unaltered, and draws
    new validator bounds from `bound_generator` every `n_trials_max` candidates."""
    check_aspect_ratio = True

    def __init__(self, patch_coord_generator, box_filter=None, image_validator=None, bound_generator=None, n_trials_max=50,
                 clip_boxes=True, prob=0.857, background=(0, 0, 0), labels_format=_LABELS_FORMAT):
        if not isinstance(patch_coord_generator, PatchCoordinateGenerator):
            raise ValueError("`patch_coord_generator` must be an instance of `PatchCoordinateGenerator`.")
        if not (isinstance(image_validator, ImageValidator) or image_validator is None):
            raise ValueError("`image_validator` must be either `None` or an `ImageValidator` object.")
        if not (isinstance(bound_generator, BoundGenerator) or bound_generator is None):
            raise ValueError("`bound_generator` must be either `None` or a `BoundGenerator` object.")
        self.patch_coord_generator = patch_coord_generator
        self.box_filter = box_filter
        self.image_validator = image_validator
        self.bound_generator = bound_generator
        self.n_trials_max = n_trials_max
        self.clip_boxes = clip_boxes
        self.prob = prob
        self.background = background
        self.labels_format = labels_format
        self.sample_patch = CropPad(patch_ymin=None, patch_xmin=None, patch_height=None, patch_width=None,
                                    clip_boxes=self.clip_boxes, box_filter=self.box_filter, background=self.background,
                                    labels_format=self.labels_format)

    def __call__(self, image, labels=None, return_inverter=False):
        self._prepare(image)
        while True:
            p = np.random.uniform(0, 1)
            if p >= (1.0 - self.prob):
                if not ((self.image_validator is None) or (self.bound_generator is None)):
                    self.image_validator.bounds = self.bound_generator()
                for _ in range(max(1, self.n_trials_max)):
                    out = self._try(image, labels, return_inverter)
                    if out is not None:
                        return out
            else:
                return _returns(image, labels, _identity_inverter, return_inverter)


# ---- object_detection_2d_geometric_ops.py -----------------------------------------------------------------------------------
class Resize(_Plannable):
    """Resizes to (height, width); `interpolation_mode` is an OpenCV code, run as the Pillow filter of `CV2_TO_PILLOW`."""

    def __init__(self, height, width, interpolation_mode=INTER_LINEAR, box_filter=None, labels_format=_LABELS_FORMAT):
        if not (isinstance(box_filter, BoxFilter) or box_filter is None):
            raise ValueError("`box_filter` must be either `None` or a `BoxFilter` object.")
        self.out_height = height
        self.out_width = width
        self.interpolation_mode = interpolation_mode
        self.box_filter = box_filter
        self.labels_format = labels_format

    def __call__(self, image, labels=None, return_inverter=False):
        img_height, img_width = image.shape[:2]
        xmin, ymin = self.labels_format['xmin'], self.labels_format['ymin']
        xmax, ymax = self.labels_format['xmax'], self.labels_format['ymax']
        filt = pillow_filter(self.interpolation_mode)
        if _planned(image):
            image = image.resize(self.out_height, self.out_width, filt)
        else:
            image = resize_host(np.ascontiguousarray(image), (self.out_width, self.out_height), filt)

        def inverter(labels):
            labels = np.copy(labels)
            labels[:, [ymin + 1, ymax + 1]] = np.round(labels[:, [ymin + 1, ymax + 1]] * (img_height / self.out_height), decimals=0)
            labels[:, [xmin + 1, xmax + 1]] = np.round(labels[:, [xmin + 1, xmax + 1]] * (img_width / self.out_width), decimals=0)
            return labels

        if (xmin, ymin, xmax, ymax) == (1, 2, 3, 4):     # the columns the device form is stated for
            inverter.device_form = ("resize", img_height / self.out_height, img_width / self.out_width)

        if labels is not None:
            labels = np.copy(labels)
            labels[:, [ymin, ymax]] = np.round(labels[:, [ymin, ymax]] * (self.out_height / img_height), decimals=0)
            labels[:, [xmin, xmax]] = np.round(labels[:, [xmin, xmax]] * (self.out_width / img_width), decimals=0)
            if not (self.box_filter is None):
                self.box_filter.labels_format = self.labels_format
                labels = self.box_filter(labels=labels, image_height=self.out_height, image_width=self.out_width)
        return _returns(image, labels, inverter, return_inverter)


class ResizeRandomInterp(_Plannable):
    """`Resize` with the interpolation mode drawn from `interpolation_modes` per call."""

    def __init__(self, height, width,
                 interpolation_modes=[INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA, INTER_LANCZOS4],
                 box_filter=None, labels_format=_LABELS_FORMAT):
        if not (isinstance(interpolation_modes, (list, tuple))):
            raise ValueError("`interpolation_mode` must be a list or tuple.")
        self.height = height
        self.width = width
        self.interpolation_modes = interpolation_modes
        self.box_filter = box_filter
        self.labels_format = labels_format
        self.resize = Resize(height=self.height, width=self.width, box_filter=self.box_filter,
                             labels_format=self.labels_format)

    def __call__(self, image, labels=None, return_inverter=False):
        self.resize.interpolation_mode = np.random.choice(self.interpolation_modes)
        self.resize.labels_format = self.labels_format
        return self.resize(image, labels, return_inverter)


class Flip(_Plannable):
    """Mirrors left-right ('horizontal') or top-bottom ('vertical'); only the first can be planned."""

    def __init__(self, dim='horizontal', labels_format=_LABELS_FORMAT):
        if not (dim in {'horizontal', 'vertical'}):
            raise ValueError("`dim` can be one of 'horizontal' and 'vertical'.")
        self.dim = dim
        self.labels_format = labels_format

    def __call__(self, image, labels=None, return_inverter=False):
        img_height, img_width = image.shape[:2]
        xmin, ymin = self.labels_format['xmin'], self.labels_format['ymin']
        xmax, ymax = self.labels_format['xmax'], self.labels_format['ymax']
        if self.dim == 'horizontal':
            image = image.mirror() if _planned(image) else image[:, ::-1]
            if labels is None:
                return image
            labels = np.copy(labels)
            labels[:, [xmin, xmax]] = img_width - labels[:, [xmax, xmin]]
            return image, labels
        if _planned(image):
            raise ValueError("a vertical flip cannot be planned: the window of data/patch_resize.py mirrors left-right only")
        image = image[::-1]
        if labels is None:
            return image
        labels = np.copy(labels)
        labels[:, [ymin, ymax]] = img_height - labels[:, [ymax, ymin]]
        return image, labels


class RandomFlip(_Plannable):
    """`Flip` with probability `prob`."""

    def __init__(self, dim='horizontal', prob=0.5, labels_format=_LABELS_FORMAT):
        self.dim = dim
        self.prob = prob
        self.labels_format = labels_format
        self.flip = Flip(dim=self.dim, labels_format=self.labels_format)

    def __call__(self, image, labels=None):
        p = np.random.uniform(0, 1)
        if p >= (1.0 - self.prob):
            self.flip.labels_format = self.labels_format
            return self.flip(image, labels)
        elif labels is None:
            return image
        else:
            return image, labels


# ---- data_augmentation_chain_original_ssd.py --------------------------------------------------------------------------------
class SSDRandomCrop(_Plannable):
    """The random crops of the original Caffe SSD's `batch_sampler`: patches of 0.3 to 1.0 of each side with an aspect
    ratio in 0.5 .. 2, valid when one box reaches the drawn minimum IoU with the patch; boxes whose centre falls outside
    the patch are dropped, the rest clipped to it."""

    def __init__(self, labels_format=_LABELS_FORMAT):
        self.labels_format = labels_format
        self.bound_generator = BoundGenerator(sample_space=((None, None), (0.1, None), (0.3, None), (0.5, None),
                                                            (0.7, None), (0.9, None)), weights=None)
        self.patch_coord_generator = PatchCoordinateGenerator(must_match='h_w', min_scale=0.3, max_scale=1.0,
                                                              scale_uniformly=False, min_aspect_ratio=0.5,
                                                              max_aspect_ratio=2.0)
        self.box_filter = BoxFilter(check_overlap=True, check_min_area=False, check_degenerate=False,
                                    overlap_criterion='center_point', labels_format=self.labels_format)
        self.image_validator = ImageValidator(overlap_criterion='iou', n_boxes_min=1, labels_format=self.labels_format,
                                              border_pixels='half')
        self.random_crop = RandomPatchInf(patch_coord_generator=self.patch_coord_generator, box_filter=self.box_filter,
                                          image_validator=self.image_validator, bound_generator=self.bound_generator,
                                          n_trials_max=50, clip_boxes=True, prob=0.857, labels_format=self.labels_format)

    def __call__(self, image, labels=None, return_inverter=False):
        self.random_crop.labels_format = self.labels_format
        return self.random_crop(image, labels, return_inverter)


class SSDExpand(_Plannable):
    """The random expansion of the original Caffe SSD: with probability 0.5 the image is placed at a random position on a
    canvas of the mean colour 1 to 4 times its size."""

    def __init__(self, background=(123, 117, 104), labels_format=_LABELS_FORMAT):
        self.labels_format = labels_format
        self.patch_coord_generator = PatchCoordinateGenerator(must_match='h_w', min_scale=1.0, max_scale=4.0,
                                                              scale_uniformly=True)
        self.expand = RandomPatch(patch_coord_generator=self.patch_coord_generator, box_filter=None, image_validator=None,
                                  n_trials_max=1, clip_boxes=False, prob=0.5, background=background,
                                  labels_format=self.labels_format)

    def __call__(self, image, labels=None, return_inverter=False):
        self.expand.labels_format = self.labels_format
        return self.expand(image, labels, return_inverter)


class _SSDChain(object):
    def _build(self, img_height, img_width, background, labels_format, photometric_distortions):
        if photometric_distortions is not None and not callable(photometric_distortions):
            raise ValueError("`photometric_distortions` must be None, an `SSDPhotometricDistortions` or a callable "
                             "(image, labels) -> (image, labels)")
        self.labels_format = labels_format
        self.photometric_distortions = photometric_distortions
        self.expand = SSDExpand(background=background, labels_format=self.labels_format)
        self.random_crop = SSDRandomCrop(labels_format=self.labels_format)
        self.random_flip = RandomFlip(dim='horizontal', prob=0.5, labels_format=self.labels_format)
        # resizing can shrink an already small box to zero height or width
        self.box_filter = BoxFilter(check_overlap=False, check_min_area=False, check_degenerate=True,
                                    labels_format=self.labels_format)
        self.resize = ResizeRandomInterp(height=img_height, width=img_width,
                                         interpolation_modes=[INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA,
                                                              INTER_LANCZOS4],
                                         box_filter=self.box_filter, labels_format=self.labels_format)

    def _run(self, image, labels, return_inverter, sequence):
        self.expand.labels_format = self.labels_format
        self.random_crop.labels_format = self.labels_format
        self.random_flip.labels_format = self.labels_format
        self.resize.labels_format = self.labels_format
        inverters = []
        for transform in sequence:
            if return_inverter and ('return_inverter' in inspect.signature(transform).parameters):
                image, labels, inverter = transform(image, labels, return_inverter=True)
                inverters.append(inverter)
            else:
                image, labels = transform(image, labels)
            if image is None:
                return (None, None, None) if return_inverter else (None, None)
        if return_inverter:
            return image, labels, inverters[::-1]
        return image, labels

    def __call__(self, image, labels, return_inverter=False):
        head = [self.photometric_distortions] if self.photometric_distortions is not None else []
        return self._run(image, labels, return_inverter, head + self.sequence)

    @property
    def plans_photometric(self):
        """Whether the photometric slot holds a stage whose draws `plan(..., return_photometric=True)` can make."""
        return hasattr(self.photometric_distortions, 'draw')

    def plan(self, height, width, labels, return_inverter=False, return_photometric=False):
        """The draws and the label arithmetic of the geometric stages for an image of (height, width), no pixel touched
        -> (geometry, labels[, inverters]) with geometry = (win_y0, win_x0, win_h, win_w, flip, filter, background) of
        data/patch_resize.py, or None when the chain gives up.  With `return_photometric` the draws of the photometric
        stage are made first, as the chain's call makes them, and their `PhotoParams` record comes back as an extra last
        element (None for an empty slot; a plain callable in the slot cannot be planned and raises): apply it to the
        decoded image (`ssd_photometric_host`, dj_ssd_photometric) before the window is cut.  Without the argument the
        photometric slot is not part of the plan and no draw is made for it."""
        record = None
        if return_photometric and self.photometric_distortions is not None:
            if not self.plans_photometric:
                raise ValueError("plan: the photometric callable %r has no `draw` and cannot be planned"
                                 % (self.photometric_distortions,))
            record = self.photometric_distortions.draw()
        out = self._run(Geometry(height, width), labels, return_inverter, self.sequence)
        if out[0] is None:
            return None
        out = (out[0].astuple(),) + tuple(out[1:])
        return out + (record,) if return_photometric else out


class SSDDataAugmentation(_SSDChain):
    """The augmentation of the original SSD training: [photometric stage,] expand, random crop, random flip, resize
    with a randomly drawn interpolation."""

    def __init__(self, img_height=300, img_width=300, background=(123, 117, 104), labels_format=_LABELS_FORMAT,
                 photometric_distortions=None):
        self._build(img_height, img_width, background, labels_format, photometric_distortions)
        self.sequence = [self.expand, self.random_crop, self.random_flip, self.resize]


class SSDDataAugmentationNoCrop(_SSDChain):
    """The reference's `..._no_crop` variant: [photometric stage,] random flip and resize only (expand and crop are built,
    as there, and not run)."""

    def __init__(self, img_height=300, img_width=300, background=(123, 117, 104), labels_format=_LABELS_FORMAT,
                 photometric_distortions=None):
        self._build(img_height, img_width, background, labels_format, photometric_distortions)
        self.sequence = [self.random_flip, self.resize]
