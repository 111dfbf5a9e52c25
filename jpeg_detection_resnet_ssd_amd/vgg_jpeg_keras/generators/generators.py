"""The classifier's image generators with the surface of the reference's
(classification_part/vgg_jpeg_keras/generators/generators.py:15-353): a directory of class directories, an ImageNet-style
index file `{"<class id>": ["<directory name>", ...]}`, and per batch `[X_y, X_cbcr]` (DCTGeneratorJPEG2DCT) or
`[X_y, X_cb, X_cr]` (DCTGeneratorJPEG2DCTDeconv) with one-hot labels.  Per image, in the reference's order: decode and
`convert("RGB")`, resize, `random.randint` for the crop offset (scale=True only), crop, `random.uniform` for the flip
(flip=True only), the photometric `transformations`, JPEG emission.

`device_prep=False` does all of that on the host: PIL for the pixels, then `emit_dct_inputs`.  `device_prep=True` only
decodes and draws: the batch is a `PendingImageInputs` and resize, crop, flip, the photometric operations and the JPEG
transform run on the GPU when the model uploads it (data/image_prep.py, csrc/dj_imgprep.hip, csrc/dj_photometric.hip),
bit-exact with the host path.  On the device path `transformations` may hold only `saturation`, `brightness`, `contrast`
and `lighting` of helper.py (recognised by identity): their draws from `np.random` are made here, in the host path's
order, and travel with the batch.  `device_decode=True` on top of `device_prep=True` (ValueError without it) does not decode
either: a file is read as bytes, and a baseline file the GPU can reconstruct (data/jpeg_pixels.py:`decodable`) travels as a
`CoefficientImage` -- its size, which the draws need, is the header's; its coefficients are entropy-decoded into the staging
blob on `decode_threads` host threads when the model uploads the batch, and dj_jpeg_pixels makes the pixels.  Any other file
(progressive, CMYK, ...) is decoded by Pillow as before and goes into the same batch.  Draws, labels and the state of
`random` / `np.random` after a batch are those of `device_prep=True`.

Differences from the reference, all outside the numbers: class directories and files are listed in sorted order (the
reference takes `os.listdir` order), inputs are float32 and labels float32 (the reference fills int32 arrays with the same
values), and the resize filter is named explicitly (`resample`, default BICUBIC: what `im.resize(size)` has meant since
Pillow 7)."""
import json
import os
import random

import numpy as np

from ...data import image_prep
from ...data.jpeg_dct import emit_dct_inputs
from ...data.jpeg_pixels import read_image
from ...keras.utils import Sequence
from . import helper


def prepare_imagenet(index_file, data_directory):
    """-> ({directory name: class id}, class directory names, image paths)."""
    with open(index_file) as f:
        association = {value[0]: class_id for class_id, value in json.load(f).items()}
    classes, images_path = [], []
    for name in sorted(os.listdir(data_directory)):
        class_directory = os.path.join(data_directory, name)
        if os.path.isdir(class_directory):
            classes.append(name)
            images_path.extend(os.path.join(class_directory, image) for image in sorted(os.listdir(class_directory)))
    return association, classes, images_path


def device_switches(environ=os.environ):
    """The device arguments of the real-data generators (these and `flow_from_directory`) as the configurations read
    them from the environment: `DJ_DEVICE_PREP=1`, `DJ_DEVICE_DECODE=1` on top of it (ValueError without it) and
    `DJ_DECODE_THREADS`, default 16 and never derived from the CPU count."""
    device_prep = environ.get("DJ_DEVICE_PREP", "0") == "1"
    device_decode = environ.get("DJ_DEVICE_DECODE", "0") == "1"
    if device_decode and not device_prep:
        raise ValueError("DJ_DEVICE_DECODE=1 needs DJ_DEVICE_PREP=1")
    return {"device_prep": device_prep, "device_decode": device_decode,
            "decode_threads": int(environ.get("DJ_DECODE_THREADS", "16"))}


def coefficient_switch(environ=os.environ):
    """Whether the configurations feed the DCT architectures the files' own coefficients
    (coefficient_generators.py): `DJ_COEFFICIENT_INPUTS=1`.  That path has no pixels to prepare or distort, so combining it
    with `DJ_DEVICE_PREP`, `DJ_DEVICE_DECODE` or `DJ_PHOTOMETRIC` is a ValueError.  `DJ_DEVICE_ENTROPY=1`
    (`device_entropy_switch`) belongs to this path alone: without `DJ_COEFFICIENT_INPUTS=1` it is a ValueError."""
    if environ.get("DJ_COEFFICIENT_INPUTS", "0") != "1":
        if environ.get("DJ_DEVICE_ENTROPY", "0") == "1":
            raise ValueError("DJ_DEVICE_ENTROPY=1 needs DJ_COEFFICIENT_INPUTS=1: only the coefficient path entropy-decodes "
                             "on the GPU")
        return False
    clash = [k for k in ("DJ_DEVICE_PREP", "DJ_DEVICE_DECODE", "DJ_PHOTOMETRIC") if environ.get(k, "0") == "1"]
    if clash:
        raise ValueError("DJ_COEFFICIENT_INPUTS=1 cannot be combined with %s: the files' own coefficients are fed to the "
                         "model, there are no pixels to prepare or distort" % ", ".join(clash))
    return True


def device_entropy_switch(environ=os.environ):
    """Whether the coefficient generators entropy-decode restart-interval files on the GPU: `DJ_DEVICE_ENTROPY=1`, which
    needs `DJ_COEFFICIENT_INPUTS=1` (ValueError without it)."""
    return coefficient_switch(environ) and environ.get("DJ_DEVICE_ENTROPY", "0") == "1"


def unmarked_switch(environ=os.environ):
    """Whether the coefficient generators entropy-decode files WITHOUT restart intervals on the GPU as well, by chunks:
    `DJ_DEVICE_ENTROPY_UNMARKED=1`, which needs `DJ_DEVICE_ENTROPY=1` (ValueError without it)."""
    on = environ.get("DJ_DEVICE_ENTROPY_UNMARKED", "0") == "1"
    if on and not device_entropy_switch(environ):
        raise ValueError("DJ_DEVICE_ENTROPY_UNMARKED=1 needs DJ_DEVICE_ENTROPY=1: it widens what that switch decodes on the GPU")
    return on


class DCTGeneratorJPEG2DCT(Sequence):
    """Batches of `[X_y, X_cbcr]` ((B, T/8, T/8, 64), (B, T/16, T/16, 128)) and one-hot labels."""
    deconv = False

    def __init__(self, data_directory, index_file, batch_size=32, shuffle=True, scale=True, target_length=224, flip=True,
                 transformations=None, device_prep=False, resample=None, device_decode=False, decode_threads=None):
        if device_decode and not device_prep:
            raise ValueError("device_decode needs device_prep: the coefficients are turned into pixels where the batch "
                             "is staged for the GPU")
        if device_prep and transformations is not None and \
                not all(helper.photometric_code(t) is not None for t in transformations):
            raise NotImplementedError(
                "device_prep=True can be combined with `transformations` made of saturation, brightness, contrast and "
                "lighting of vgg_jpeg_keras.generators only: any other callable works on host pixels, and with "
                "device_prep the resized pixels exist on the GPU only; use device_prep=False")
        if device_prep and transformations is not None and len(transformations) > 4:
            raise NotImplementedError("device_prep=True runs at most 4 `transformations` per image, got %d"
                                      % len(transformations))
        self.association, self.classes, self.images_path = prepare_imagenet(index_file, data_directory)
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.number_of_data_samples = len(self.images_path)
        self.scale = scale
        self.target_length = target_length
        self.flip = flip
        self.transformations = transformations
        self.device_prep = bool(device_prep)
        self.device_decode = bool(device_decode)
        self.resample = image_prep.resolve_resample(resample)
        self.number_of_classes = len(self.classes)
        self.batches_per_epoch = len(self.images_path) // self.batch_size
        self.indexes = np.arange(len(self.images_path))
        self._prep = image_prep.DeviceImagePrep(target_length, self.resample, deconv=self.deconv,
                                                n_threads=decode_threads) if device_prep else None
        self.on_epoch_end()

    def __len__(self):
        return self.batches_per_epoch

    def __getitem__(self, index):
        index = index % self.batches_per_epoch      # more steps per epoch than batches wrap around
        return self._data_generation(self.indexes[index * self.batch_size:(index + 1) * self.batch_size])

    def on_epoch_end(self):
        if self.shuffle:
            np.random.shuffle(self.indexes)

    def _label(self, path):
        return int(self.association[os.path.basename(os.path.dirname(path))])

    def _host_pixels(self, im):
        """Steps 2 to 5 in PIL, drawing from `random` in the reference's order."""
        from PIL import Image
        t = self.target_length
        if self.scale:
            ratio = t / min(im.size)
            width, height = im.size
            im = im.resize((int(round(width * ratio)), int(round(height * ratio))), self.resample)
            offset = random.randint(0, max(im.size) - t)
            if im.size[0] > im.size[1]:
                im = im.crop((offset, 0, t + offset, t))
            else:
                im = im.crop((0, offset, t, t + offset))
        else:
            im = im.resize((int(t), int(t)), self.resample)
        if self.flip and random.uniform(0, 1) > 0.5:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        if self.transformations is not None:
            pixels = np.array(im)
            random.shuffle(self.transformations)
            for transformation in self.transformations:
                if random.uniform(0, 1) > 0.5:
                    pixels = transformation(pixels)
            im = Image.fromarray(pixels).convert("RGB")
        return np.asarray(im)

    def _draws(self, height, width):
        """The same draws for the device path, in the same order: -> ((scale, offset, flip), photometric operations or
        None).  A transformation that is taken makes its own draw from `np.random`, as the callable would."""
        offset = 0
        if self.scale:
            offset = random.randint(0, image_prep.max_offset(height, width, self.target_length))
        flip = bool(self.flip and random.uniform(0, 1) > 0.5)
        ops = None
        if self.transformations is not None:
            random.shuffle(self.transformations)
            ops = [helper.draw_parameters(t) for t in self.transformations if random.uniform(0, 1) > 0.5]
        return (bool(self.scale), offset, flip), ops

    def _data_generation(self, indexes):
        from PIL import Image
        y = np.zeros((len(indexes), self.number_of_classes), dtype=np.float32)
        images, params, ops = [], [], []
        for i, k in enumerate(indexes):
            path = self.images_path[k]
            if self.device_prep:
                # a `CoefficientImage`'s shape is its header's: the draws need no pixels
                if self.device_decode:
                    pixels = read_image(path)
                else:
                    with Image.open(path) as im:
                        pixels = np.asarray(im.convert("RGB"))
                images.append(pixels)
                draws, image_ops = self._draws(pixels.shape[0], pixels.shape[1])
                params.append(draws)
                ops.append(image_ops)
            else:
                with Image.open(path) as im:
                    images.append(self._host_pixels(im.convert("RGB")))
            y[i, self._label(path)] = 1
        if self.device_prep:
            return self._prep(images, params, ops if self.transformations is not None else None), y
        return emit_dct_inputs(np.stack(images), deconv=self.deconv), y


class DCTGeneratorJPEG2DCTDeconv(DCTGeneratorJPEG2DCT):
    """Batches of `[X_y, X_cb, X_cr]` ((B, T/8, T/8, 64) and twice (B, T/16, T/16, 64)) and one-hot labels."""
    deconv = True
