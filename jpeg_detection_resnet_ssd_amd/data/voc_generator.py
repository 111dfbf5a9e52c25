"""`DataGeneratorDCT` for Pascal VOC: the `parse_xml` / `generate` / `get_dataset_size` surface of the reference's
localisation_part/data_generator/object_detection_2d_data_generator_dct_j2d.py with its per-batch rules, on what is
installed here (xml.etree for the annotations, PIL for decoding, the in-tree reader or the GPU for the coefficients).

`generate` has two paths.  On the host path the transformations run on pixels (data/ssd_augment.py) and
`emit_dct_inputs` makes the model inputs.  With `device_prep=DevicePatchResize(...)` every transformation is PLANNED
(`transform.plan`: same draws, same boxes, no pixel touched), the plans of one image compose into one geometry, the
images are only decoded, and the first item of the batch is a `PendingPatchInputs`: window, mirror, resize and the JPEG
transform run on the GPU when the model uploads the batch.  A chain with a drawable photometric stage
(`SSDDataAugmentation(..., photometric_distortions=SSDPhotometricDistortions())`) is asked for that stage's draws too
(`plan(..., return_photometric=True)`), and the records go to `device_prep(images, geometries, photometric=records)`: the
stage then runs on the GPU on the staged pixels, before the window is cut.  Both paths leave bit-identical inputs.
With `device_decode=True` as well, a file is not decoded here either: it is read as bytes, and when the in-tree reader
calls it decodable (data/jpeg_pixels.py) it travels as a `CoefficientImage` whose height and width come from the header;
worker threads entropy-decode it into the pinned staging buffer (as many as `device_prep` was built with:
`DevicePatchResize(..., n_threads=)`) and dj_jpeg_pixels reconstructs the staged
rectangle on the GPU, byte for byte what Pillow would have decoded.  Any other file (progressive, CMYK, ...) is decoded
with Pillow as before, so a batch may mix the two.  Draws, boxes and dropped items do not depend on the switch.

Differences from the reference: images are decoded with `convert("RGB")` (its `ConvertTo3Channels` lives in the
photometric stage, which sees three channels here); the dataset is reshuffled with `np.random.permutation`
when a pass ends (sklearn is not used); HDF5 datasets and `parse_csv` / `parse_json` are not restated."""
import inspect
import os
import warnings
import xml.etree.ElementTree as ET
from copy import deepcopy

import numpy as np

from .jpeg_dct import emit_dct_inputs
from .ssd_augment import BoxFilter

VOC_CLASSES = ['background', 'aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow',
               'diningtable', 'dog', 'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor']


class DegenerateBatchError(Exception):
    """Every item of a batch was removed."""


def _text(node, tag, default=None):
    child = node.find(tag)
    if child is None or child.text is None:
        if default is None:
            raise ValueError("annotation lacks <%s>" % tag)
        return default
    return child.text.strip()


def _resize_target(transform):
    """(height, width) a transformation resizes to (its own, or that of the `resize` stage of a chain); None without one."""
    for obj in (transform, getattr(transform, 'resize', None)):
        for names in (('height', 'width'), ('out_height', 'out_width')):
            if all(hasattr(obj, n) for n in names):
                return tuple(int(getattr(obj, n)) for n in names)
    return None


class DataGeneratorDCT(object):
    def __init__(self, load_images_into_memory=False, labels_output_format=('class_id', 'xmin', 'ymin', 'xmax', 'ymax'),
                 **unused):
        self.labels_output_format = labels_output_format
        self.labels_format = {name: labels_output_format.index(name) for name in ('class_id', 'xmin', 'ymin', 'xmax', 'ymax')}
        self.load_images_into_memory = bool(load_images_into_memory)
        self.images = None
        self.filenames, self.image_ids, self.labels, self.eval_neutral = [], [], [], []
        self.dataset_size = 0
        self.dataset_indices = np.arange(0, dtype=np.int32)

    @staticmethod
    def _decode(filename):
        from PIL import Image
        with Image.open(filename) as image:
            return np.array(image.convert("RGB"), dtype=np.uint8)

    @classmethod
    def _read(cls, filename):
        """The file as a `CoefficientImage` when the GPU can reconstruct its pixels, else decoded as `_decode` does."""
        from .jpeg_pixels import CoefficientImage
        with open(filename, "rb") as f:
            data = f.read()
        try:
            return CoefficientImage(data)
        except ValueError:              # not `decodable`, or no JPEG the reader can parse
            return cls._decode(filename)

    def parse_xml(self, images_dirs, image_set_filenames, annotations_dirs=(), classes=VOC_CLASSES, include_classes='all',
                  exclude_truncated=False, exclude_difficult=False, ret=False, verbose=False):
        """Pascal VOC: one image-set file of ids and one directory of `<id>.xml` per images directory.  Fills
        `filenames`, `image_ids`, `labels` (per image a list of boxes in `labels_output_format`) and `eval_neutral` (per
        box: annotated 'difficult'); without annotation directories the last two are None."""
        self.images_dirs, self.annotations_dirs, self.image_set_filenames = images_dirs, annotations_dirs, image_set_filenames
        self.classes, self.include_classes = list(classes), include_classes
        self.filenames, self.image_ids, self.labels, self.eval_neutral = [], [], [], []
        if not annotations_dirs:
            self.labels = self.eval_neutral = None
            annotations_dirs = [None] * len(images_dirs)
        for images_dir, image_set_filename, annotations_dir in zip(images_dirs, image_set_filenames, annotations_dirs):
            with open(image_set_filename) as f:
                image_ids = [line.strip() for line in f if line.strip()]
            self.image_ids += image_ids
            for image_id in image_ids:
                filename = image_id + '.jpg'
                self.filenames.append(os.path.join(images_dir, filename))
                if annotations_dir is None:
                    continue
                root = ET.parse(os.path.join(annotations_dir, image_id + '.xml')).getroot()
                folder = _text(root, 'folder', '')
                boxes, eval_neutr = [], []
                for obj in root.iter('object'):
                    class_name = _text(obj, 'name')
                    class_id = self.classes.index(class_name)
                    if (not self.include_classes == 'all') and (class_id not in self.include_classes):
                        continue
                    truncated = int(_text(obj, 'truncated', '0'))
                    if exclude_truncated and truncated == 1:
                        continue
                    difficult = int(_text(obj, 'difficult', '0'))
                    if exclude_difficult and difficult == 1:
                        continue
                    bndbox = obj.find('bndbox')
                    item = {'folder': folder, 'image_name': filename, 'image_id': image_id, 'class_name': class_name,
                            'class_id': class_id, 'pose': _text(obj, 'pose', 'Unspecified'), 'truncated': truncated,
                            'difficult': difficult}
                    for key in ('xmin', 'ymin', 'xmax', 'ymax'):
                        item[key] = int(_text(bndbox, key))
                    boxes.append([item[name] for name in self.labels_output_format])
                    eval_neutr.append(bool(difficult))
                self.labels.append(boxes)
                self.eval_neutral.append(eval_neutr)
        self.dataset_size = len(self.filenames)
        self.dataset_indices = np.arange(self.dataset_size, dtype=np.int32)
        self.images = [self._decode(f) for f in self.filenames] if self.load_images_into_memory else None
        if ret:
            return self.images, self.filenames, self.labels, self.image_ids, self.eval_neutral

    def get_dataset_size(self):
        return self.dataset_size

    def _shuffle(self):
        order = np.random.permutation(self.dataset_size)
        self.dataset_indices = self.dataset_indices[order]
        for name in ("filenames", "labels", "image_ids", "eval_neutral", "images"):
            items = getattr(self, name)
            if items is not None:
                setattr(self, name, [items[k] for k in order])

    def generate(self, batch_size=32, shuffle=True, transformations=(), label_encoder=None,
                 returns=('processed_images', 'encoded_labels'), keep_images_without_gt=False,
                 degenerate_box_handling='remove', deconv=False, device_prep=None, n_threads=None,
                 device_decode=False):
        """Yields batches for ever; a pass that ends reshuffles (when `shuffle`) and starts over.  Per batch, as in the
        reference: an item without boxes, before or after its transformations, is dropped unless
        `keep_images_without_gt`; an item whose transformation gives up (returns None) is dropped; degenerate boxes are
        removed ('remove') or warned about ('warn').  Output order: processed_images, encoded_labels, processed_labels,
        filenames, image_ids, evaluation-neutral, inverse_transform, original_images, original_labels -- those named in
        `returns`.  `device_prep`: see the module's docstring; a transformation without `plan` raises there.
        `device_decode`: with `device_prep` only (ValueError otherwise): files the GPU can reconstruct are not decoded on
        the host (images already in memory stay the arrays they are)."""
        if self.dataset_size == 0:
            raise ValueError("the dataset is empty: call parse_xml first")
        if degenerate_box_handling not in ('remove', 'warn'):
            raise ValueError("`degenerate_box_handling` must be 'remove' or 'warn'")
        transformations = list(transformations)
        if device_decode and device_prep is None:
            raise ValueError("device_decode needs device_prep: the coefficients are turned into pixels where the batch "
                             "is staged for the GPU")
        if device_prep is not None:
            for transform in transformations:
                if not hasattr(transform, 'plan'):
                    raise ValueError("device_prep: transformation %r has no `plan` and cannot run as one window and "
                                     "resize on the GPU" % (transform,))
        if self.labels is not None:
            for transform in transformations:
                transform.labels_format = self.labels_format
        box_filter = BoxFilter(check_overlap=False, check_min_area=False, check_degenerate=True,
                               labels_format=self.labels_format)
        xmin, ymin, xmax, ymax = (self.labels_format[k] for k in ('xmin', 'ymin', 'xmax', 'ymax'))
        want_inverse = 'inverse_transform' in returns
        current = 0
        while True:
            if current >= self.dataset_size:
                current = 0
                if shuffle:
                    self._shuffle()
            window = slice(current, current + batch_size)
            batch_filenames = list(self.filenames[window])
            if self.images is not None:
                batch_X = list(self.images[window])
            elif device_decode:
                batch_X = [self._read(f) for f in batch_filenames]
            else:
                batch_X = [self._decode(f) for f in batch_filenames]
            batch_y = deepcopy(self.labels[window]) if self.labels is not None else None
            batch_eval_neutral = list(self.eval_neutral[window]) if self.eval_neutral is not None else None
            batch_image_ids = list(self.image_ids[window])
            batch_original_images = None
            if 'original_images' in returns:
                batch_original_images = [x.pixels() if hasattr(x, 'pixels') else deepcopy(x) for x in batch_X]
            batch_original_labels = deepcopy(batch_y) if 'original_labels' in returns else None
            current += batch_size

            remove, batch_inverse_transforms = [], []
            batch_geometry = [None] * len(batch_X)
            batch_photometric = [None] * len(batch_X)
            for i in range(len(batch_X)):
                if batch_y is not None:
                    batch_y[i] = np.array(batch_y[i])
                    if batch_y[i].size == 0 and not keep_images_without_gt:
                        remove.append(i)
                        batch_inverse_transforms.append([])
                        continue
                    if batch_y[i].size == 0:
                        batch_y[i] = batch_y[i].reshape(0, len(self.labels_output_format))
                inverse_transforms, failed = [], False
                height, width = batch_X[i].shape[:2]
                for transform in transformations:
                    labels = batch_y[i] if batch_y is not None else None
                    inverter = want_inverse and 'return_inverter' in inspect.signature(transform).parameters
                    if device_prep is not None:
                        planner = transform.plan
                        kwargs = {'geometry': batch_geometry[i]} if 'geometry' in inspect.signature(planner).parameters else {}
                        if kwargs == {} and batch_geometry[i] is not None:
                            raise ValueError("device_prep: %r plans a whole chain and has to come first" % (transform,))
                        if inverter and 'return_inverter' in inspect.signature(planner).parameters:
                            kwargs['return_inverter'] = True
                        else:
                            inverter = False
                        photometric = bool(getattr(transform, 'plans_photometric', False))
                        if photometric:
                            kwargs['return_photometric'] = True
                        out = planner(height, width, labels, **kwargs)
                        if photometric and out is not None:
                            batch_photometric[i], out = out[-1], out[:-1]
                        out = (None,) if out is None else (out if labels is not None or inverter else (out,))
                    else:
                        args = (batch_X[i],) + ((labels,) if labels is not None else ())
                        out = transform(*args, return_inverter=True) if inverter else transform(*args)
                        out = out if isinstance(out, tuple) else (out,)
                    if out[0] is None:
                        failed = True
                        break
                    if device_prep is not None:
                        batch_geometry[i] = out[0]
                    else:
                        batch_X[i] = out[0]
                    if labels is not None:
                        batch_y[i] = out[1]
                    if inverter:
                        last = out[-1]
                        inverse_transforms.extend(last if isinstance(last, list) else [last])
                if failed:
                    remove.append(i)
                    batch_inverse_transforms.append([])
                    continue
                batch_inverse_transforms.append(inverse_transforms[::-1])
                if batch_y is not None:
                    y = batch_y[i]
                    if np.any(y[:, xmax] - y[:, xmin] <= 0) or np.any(y[:, ymax] - y[:, ymin] <= 0):
                        if degenerate_box_handling == 'warn':
                            warnings.warn("Detected degenerate ground truth bounding boxes for batch item %d with bounding "
                                          "boxes %s, i.e. bounding boxes where xmax <= xmin and/or ymax <= ymin." % (i, y))
                        else:
                            batch_y[i] = box_filter(y)
                            if batch_y[i].size == 0 and not keep_images_without_gt:
                                remove.append(i)
            for j in sorted(remove, reverse=True):
                for items in (batch_X, batch_geometry, batch_photometric, batch_filenames, batch_inverse_transforms, batch_y,
                              batch_image_ids, batch_eval_neutral, batch_original_images, batch_original_labels):
                    if items is not None:
                        items.pop(j)
            if not batch_X:
                raise DegenerateBatchError("You produced an empty batch: every item was removed.")

            if device_prep is not None:
                size = (device_prep.out_height, device_prep.out_width)
                geometries = []
                for image, geometry in zip(batch_X, batch_geometry):
                    if geometry is None:       # no transformation: the whole image
                        geometry = (0, 0, image.shape[0], image.shape[1], False, None, (0, 0, 0))
                    geometries.append(geometry)
                for transform in transformations:      # the planned boxes are in the transformation's output size
                    if _resize_target(transform) not in (None, size):
                        raise ValueError("device_prep resizes to %s but %r was built for %s"
                                         % (size, transform, _resize_target(transform)))
                if any(rec is not None for rec in batch_photometric):
                    processed = device_prep(batch_X, geometries, photometric=batch_photometric)
                else:
                    processed = device_prep(batch_X, geometries)
            else:
                shapes = {im.shape for im in batch_X}
                if len(shapes) != 1:
                    raise DegenerateBatchError("After the transformations all images of a batch must have one size, got %s"
                                               % sorted(shapes))
                processed = emit_dct_inputs(np.stack(batch_X), deconv=deconv, n_threads=n_threads)

            batch_y_encoded = None
            if label_encoder is not None and batch_y is not None:
                batch_y_encoded = label_encoder(batch_y)
            ret = []
            if 'processed_images' in returns:
                ret.append(processed)
            if 'encoded_labels' in returns:
                ret.append(batch_y_encoded)
            if 'processed_labels' in returns:
                ret.append(batch_y)
            if 'filenames' in returns:
                ret.append(batch_filenames)
            if 'image_ids' in returns:
                ret.append(batch_image_ids)
            if 'evaluation-neutral' in returns:
                ret.append(batch_eval_neutral)
            if 'inverse_transform' in returns:
                ret.append(batch_inverse_transforms)
            if 'original_images' in returns:
                ret.append(batch_original_images)
            if 'original_labels' in returns:
                ret.append(batch_original_labels)
            yield ret
