"""keras.preprocessing.image: `load_img`, `img_to_array`, `ImageDataGenerator(...).flow_from_directory(...)` -- the input
pipeline of the reference's RGB ResNet50 (classification_part/config/resnetRGB/config_file.py:157-172), restated from the
behaviour of Keras 2.2.4 with Keras-Preprocessing 1.1.0.

PARITY UNPINNED AGAINST keras_preprocessing; THE MODULE IS THE CONTRACT.  Keras-Preprocessing is not a dependency and no
test compares with it.  What is pinned: the warp equals `scipy.ndimage.affine_transform(order=1, mode='nearest')` bit for
bit (data/rgb_warp.py:affine_warp_host, tests/test_image_generator_cpu.py), the order of the `np.random` draws, the matrix
composition and the standardisation are the rules written below, and the GPU path (csrc/dj_rgbwarp.hip, through
`flow_from_directory(..., device_prep=True)`) equals the host path bit for bit, and so does `device_decode=True` on top of it,
which leaves JPEG decoding (csrc/dj_jpegpix.hip) and `load_img`'s resize (csrc/dj_patchresize.hip) to the GPU as well.

Implemented arguments of `ImageDataGenerator`: rotation_range, width_shift_range / height_shift_range (float form),
shear_range, zoom_range, horizontal_flip, vertical_flip, fill_mode='nearest', interpolation_order=1, rescale,
preprocessing_function, validation_split=0 and featurewise_center=True without `fit` (Keras warns and does nothing; so
does this).  Every other non-default argument raises NotImplementedError naming it.  Not built: `flow`,
`flow_from_dataframe`, `fit`, `save_to_dir`, class modes other than 'categorical' and None."""
import os
import threading
import warnings

import numpy as np

from ...data.rgb_warp import (PREP_CAFFE, PREP_NONE, PendingRGBFileInputs, PendingRGBInputs, RGBWarpStager,  # noqa: F401
                              affine_warp_host, make_record, pack_records)
from ..utils import Sequence

_PIL_INTERPOLATION_METHODS = {"nearest": 0, "lanczos": 1, "bilinear": 2, "bicubic": 3, "box": 4, "hamming": 5}
WHITE_LIST_FORMATS = ("png", "jpg", "jpeg", "bmp", "ppm", "tif", "tiff")


def load_img(path, grayscale=False, color_mode="rgb", target_size=None, interpolation="nearest"):
    """The file as a PIL image: converted to RGB if its mode differs, resized to `target_size` = (height, width) with the
    named PIL filter if its size differs."""
    from PIL import Image
    if grayscale or color_mode != "rgb":
        raise NotImplementedError("load_img: color_mode=%r is not implemented (only 'rgb')"
                                  % ("grayscale" if grayscale else color_mode,))
    if interpolation not in _PIL_INTERPOLATION_METHODS:
        raise ValueError("Invalid interpolation method %s specified. Supported methods are %s"
                         % (interpolation, ", ".join(_PIL_INTERPOLATION_METHODS)))
    img = Image.open(path)
    if img.mode != "RGB":
        img = img.convert("RGB")
    if target_size is not None:
        width_height = (int(target_size[1]), int(target_size[0]))
        if img.size != width_height:
            img = img.resize(width_height, _PIL_INTERPOLATION_METHODS[interpolation])
    return img


def img_to_array(img, data_format="channels_last", dtype="float32"):
    """A PIL image -> (H, W, C) array of `dtype`."""
    if data_format != "channels_last":
        raise NotImplementedError("img_to_array: data_format=%r is not implemented (only 'channels_last')" % (data_format,))
    x = np.asarray(img, dtype=dtype)
    if x.ndim == 2:
        x = x.reshape(x.shape + (1,))
    elif x.ndim != 3:
        raise ValueError("Unsupported image shape: %s" % (x.shape,))
    return x


def transform_matrix_offset_center(matrix, x, y):
    o_x, o_y = float(x) / 2 + 0.5, float(y) / 2 + 0.5
    offset = np.array([[1, 0, o_x], [0, 1, o_y], [0, 0, 1]])
    reset = np.array([[1, 0, -o_x], [0, 1, -o_y], [0, 0, 1]])
    return np.dot(np.dot(offset, matrix), reset)


def affine_matrix(shape, theta=0, tx=0, ty=0, shear=0, zx=1, zy=1):
    """The recentred 3 x 3 float64 matrix of an (H, W, ...) image: rotation . shift . shear . zoom, each factor present only
    when it is not trivial, as offset . M . reset with o = float(dim) / 2 + 0.5 per axis; None when no factor is present.
    Angles in degrees."""
    matrix = None
    if theta != 0:
        t = np.deg2rad(theta)
        matrix = np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])
    if tx != 0 or ty != 0:
        shift = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]])
        matrix = shift if matrix is None else np.dot(matrix, shift)
    if shear != 0:
        s = np.deg2rad(shear)
        shear_matrix = np.array([[1, -np.sin(s), 0], [0, np.cos(s), 0], [0, 0, 1]])
        matrix = shear_matrix if matrix is None else np.dot(matrix, shear_matrix)
    if zx != 1 or zy != 1:
        zoom = np.array([[zx, 0, 0], [0, zy, 0], [0, 0, 1]])
        matrix = zoom if matrix is None else np.dot(matrix, zoom)
    if matrix is None:
        return None
    return transform_matrix_offset_center(np.asarray(matrix, dtype=np.float64), shape[0], shape[1])


def apply_affine_transform(x, theta=0, tx=0, ty=0, shear=0, zx=1, zy=1, row_axis=0, col_axis=1, channel_axis=2,
                           fill_mode="nearest", cval=0., order=1):
    """The (H, W, C) image warped by `affine_matrix`: float32; `x` itself when no factor is present."""
    if (row_axis, col_axis, channel_axis) != (0, 1, 2):
        raise NotImplementedError("apply_affine_transform: only channels-last images (row_axis=0, col_axis=1, channel_axis=2)")
    if fill_mode != "nearest":
        raise NotImplementedError("apply_affine_transform: fill_mode=%r is not implemented (only 'nearest')" % (fill_mode,))
    if order != 1:
        raise NotImplementedError("apply_affine_transform: order=%r is not implemented (only 1)" % (order,))
    matrix = affine_matrix(np.shape(x), theta, tx, ty, shear, zx, zy)
    if matrix is None:
        return x
    return affine_warp_host(x, matrix)


def flip_axis(x, axis):
    x = np.asarray(x).swapaxes(axis, 0)
    x = x[::-1, ...]
    return x.swapaxes(0, axis)


class ImageDataGenerator(object):
    """Keras' argument list and defaults; see the module docstring for what is implemented."""

    def __init__(self, featurewise_center=False, samplewise_center=False, featurewise_std_normalization=False,
                 samplewise_std_normalization=False, zca_whitening=False, zca_epsilon=1e-6, rotation_range=0,
                 width_shift_range=0., height_shift_range=0., brightness_range=None, shear_range=0., zoom_range=0.,
                 channel_shift_range=0., fill_mode="nearest", cval=0., horizontal_flip=False, vertical_flip=False,
                 rescale=None, preprocessing_function=None, data_format="channels_last", validation_split=0.0,
                 interpolation_order=1, dtype="float32"):
        refused = [("samplewise_center", samplewise_center, False),
                   ("featurewise_std_normalization", featurewise_std_normalization, False),
                   ("samplewise_std_normalization", samplewise_std_normalization, False),
                   ("zca_whitening", zca_whitening, False), ("zca_epsilon", zca_epsilon, 1e-6),
                   ("brightness_range", brightness_range, None), ("channel_shift_range", channel_shift_range, 0.),
                   ("fill_mode", fill_mode, "nearest"), ("cval", cval, 0.),
                   ("data_format", data_format if data_format is not None else "channels_last", "channels_last"),
                   ("validation_split", validation_split, 0.0), ("interpolation_order", interpolation_order, 1),
                   ("dtype", dtype if dtype is not None else "float32", "float32")]
        for name, value, default in refused:
            if isinstance(value, np.ndarray) or value != default:
                raise NotImplementedError("ImageDataGenerator: %s=%r is not implemented (only %r)" % (name, value, default))
        for name, value in (("width_shift_range", width_shift_range), ("height_shift_range", height_shift_range)):
            if not isinstance(value, (float, np.floating)) and not (isinstance(value, (int, np.integer)) and value == 0):
                raise NotImplementedError("ImageDataGenerator: %s=%r is not implemented (only the float form)" % (name, value))
        self.featurewise_center = bool(featurewise_center)
        self.rotation_range = rotation_range
        self.width_shift_range, self.height_shift_range = width_shift_range, height_shift_range
        self.shear_range = shear_range
        if np.isscalar(zoom_range):
            self.zoom_range = [1 - zoom_range, 1 + zoom_range]
        elif len(zoom_range) == 2:
            self.zoom_range = [zoom_range[0], zoom_range[1]]
        else:
            raise ValueError("`zoom_range` should be a float or a tuple or list of two floats. Received: %s" % (zoom_range,))
        self.fill_mode, self.cval, self.interpolation_order = fill_mode, cval, interpolation_order
        self.horizontal_flip, self.vertical_flip = horizontal_flip, vertical_flip
        self.rescale = rescale
        self.preprocessing_function = preprocessing_function
        self.data_format, self.dtype = "channels_last", "float32"
        self.channel_axis, self.row_axis, self.col_axis = 3, 1, 2
        self.validation_split = 0.0
        self.mean = None

    def flow_from_directory(self, directory, target_size=(256, 256), color_mode="rgb", classes=None,
                            class_mode="categorical", batch_size=32, shuffle=True, seed=None, save_to_dir=None,
                            save_prefix="", save_format="png", follow_links=False, subset=None, interpolation="nearest",
                            device_prep=False, device_decode=False, decode_threads=None):
        return DirectoryIterator(directory, self, target_size=target_size, color_mode=color_mode, classes=classes,
                                 class_mode=class_mode, batch_size=batch_size, shuffle=shuffle, seed=seed,
                                 save_to_dir=save_to_dir, save_prefix=save_prefix, save_format=save_format,
                                 follow_links=follow_links, subset=subset, interpolation=interpolation,
                                 device_prep=device_prep, device_decode=device_decode, decode_threads=decode_threads)

    def flow(self, *args, **kwargs):
        raise NotImplementedError("ImageDataGenerator.flow is not implemented (only flow_from_directory)")

    def flow_from_dataframe(self, *args, **kwargs):
        raise NotImplementedError("ImageDataGenerator.flow_from_dataframe is not implemented (only flow_from_directory)")

    def fit(self, *args, **kwargs):
        raise NotImplementedError("ImageDataGenerator.fit is not implemented: featurewise statistics are never applied")

    def standardize(self, x):
        """`preprocessing_function(x)` first, then `x *= rescale` in float32; `featurewise_center` without `fit` warns."""
        if self.preprocessing_function:
            x = self.preprocessing_function(x)
        if self.rescale:
            x = x * np.float32(self.rescale)
        self._warn_unfit()
        return x

    def _warn_unfit(self):
        if self.featurewise_center:
            warnings.warn("This ImageDataGenerator specifies `featurewise_center`, but it hasn't been fit on any training "
                          "data. Fit it first by calling `.fit(numpy_data)`.")

    def get_random_transform(self, img_shape, seed=None):
        """Keras' dict of one image's transform.  The `np.random` draws, in this order, each only where stated: theta if
        rotation_range; tx if height_shift_range; ty if width_shift_range; shear if shear_range; (zx, zy) unless the
        range is [1, 1]; flip_horizontal and flip_vertical always."""
        if seed is not None:
            np.random.seed(seed)
        theta = np.random.uniform(-self.rotation_range, self.rotation_range) if self.rotation_range else 0
        if self.height_shift_range:
            tx = np.random.uniform(-self.height_shift_range, self.height_shift_range)
            if self.height_shift_range < 1:
                tx *= img_shape[0]
        else:
            tx = 0
        if self.width_shift_range:
            ty = np.random.uniform(-self.width_shift_range, self.width_shift_range)
            if self.width_shift_range < 1:
                ty *= img_shape[1]
        else:
            ty = 0
        shear = np.random.uniform(-self.shear_range, self.shear_range) if self.shear_range else 0
        if self.zoom_range[0] == 1 and self.zoom_range[1] == 1:
            zx, zy = 1, 1
        else:
            zx, zy = np.random.uniform(self.zoom_range[0], self.zoom_range[1], 2)
        flip_horizontal = (np.random.random() < 0.5) * self.horizontal_flip
        flip_vertical = (np.random.random() < 0.5) * self.vertical_flip
        return {"theta": theta, "tx": tx, "ty": ty, "shear": shear, "zx": zx, "zy": zy, "flip_horizontal": flip_horizontal,
                "flip_vertical": flip_vertical, "channel_shift_intensity": None, "brightness": None}

    def apply_transform(self, x, transform_parameters):
        """The warp, then the column flip, then the row flip of one (H, W, C) image."""
        p = transform_parameters
        x = apply_affine_transform(x, p.get("theta", 0), p.get("tx", 0), p.get("ty", 0), p.get("shear", 0), p.get("zx", 1),
                                   p.get("zy", 1), fill_mode=self.fill_mode, cval=self.cval, order=self.interpolation_order)
        if p.get("flip_horizontal", False):
            x = flip_axis(x, 1)
        if p.get("flip_vertical", False):
            x = flip_axis(x, 0)
        return x

    def random_transform(self, x, seed=None):
        return self.apply_transform(x, self.get_random_transform(np.shape(x), seed))

    def transform_record(self, img_shape, transform_parameters):
        """The same transform as the record dj_rgb_warp reads (data/rgb_warp.py:RECORD_DTYPE)."""
        p = transform_parameters
        matrix = affine_matrix(img_shape, p.get("theta", 0), p.get("tx", 0), p.get("ty", 0), p.get("shear", 0),
                               p.get("zx", 1), p.get("zy", 1))
        return make_record(matrix, p.get("flip_horizontal", False), p.get("flip_vertical", False))


def _valid_files(directory, follow_links):
    """(root, file name) of every white-listed file below `directory`: directories in sorted walk order, names sorted."""
    for root, _, files in sorted(os.walk(directory, followlinks=follow_links), key=lambda x: x[0]):
        for fname in sorted(files):
            if fname.lower().endswith(WHITE_LIST_FORMATS):
                yield root, fname


class DirectoryIterator(Sequence):
    """Keras' DirectoryIterator: a `Sequence` (`len`, `[index]`, `on_epoch_end`) and an iterator (`next()`), yielding
    (float32 (b, H, W, 3), one-hot float32 labels) -- or, with `device_prep`, (PendingRGBInputs, labels): the same draws in
    the same order, decode and resize on the host, warp, flips and standardisation on the GPU when the model uploads.
    With `device_decode` on top (ValueError without `device_prep`) the host neither decodes nor resizes: a file is read as
    bytes, a baseline JPEG the GPU can reconstruct travels as a `CoefficientImage` and any other file as Pillow's full-size
    RGB array, in a `PendingRGBFileInputs`; its coefficients are read on `decode_threads` host threads at upload time, and
    dj_jpeg_pixels, `interpolation`'s resize (dj_patch_resize) and the warp run on the GPU.  `interpolation` must then be
    a filter data/device_staging.py restates (every one but 'hamming': NotImplementedError)."""

    def __init__(self, directory, image_data_generator, target_size=(256, 256), color_mode="rgb", classes=None,
                 class_mode="categorical", batch_size=32, shuffle=True, seed=None, data_format="channels_last",
                 save_to_dir=None, save_prefix="", save_format="png", follow_links=False, subset=None,
                 interpolation="nearest", dtype="float32", device_prep=False, device_decode=False, decode_threads=None):
        if color_mode != "rgb":
            raise NotImplementedError("flow_from_directory: color_mode=%r is not implemented (only 'rgb')" % (color_mode,))
        if class_mode not in ("categorical", None):
            raise NotImplementedError("flow_from_directory: class_mode=%r is not implemented (only 'categorical' and None)"
                                      % (class_mode,))
        if save_to_dir is not None:
            raise NotImplementedError("flow_from_directory: save_to_dir is not implemented")
        if subset is not None:
            raise NotImplementedError("flow_from_directory: subset=%r is not implemented (validation_split is 0)" % (subset,))
        if data_format != "channels_last" or dtype != "float32":
            raise NotImplementedError("flow_from_directory: only data_format='channels_last' and dtype='float32'")
        if interpolation not in _PIL_INTERPOLATION_METHODS:
            raise ValueError("Invalid interpolation method %s specified. Supported methods are %s"
                             % (interpolation, ", ".join(_PIL_INTERPOLATION_METHODS)))
        self.directory, self.image_data_generator = directory, image_data_generator
        self.target_size = tuple(int(v) for v in target_size)
        self.image_shape = self.target_size + (3,)
        self.color_mode, self.class_mode, self.interpolation = color_mode, class_mode, interpolation
        self.device_prep, self.device_decode = bool(device_prep), bool(device_decode)
        if self.device_decode and not self.device_prep:
            raise ValueError("device_decode needs device_prep: the coefficients are turned into pixels where the batch "
                             "is staged for the GPU")
        if self.device_decode:
            from ...data import device_staging
            self._resample = _PIL_INTERPOLATION_METHODS[interpolation]
            if self._resample not in device_staging.RESTATED:
                raise NotImplementedError("flow_from_directory(device_decode=True): interpolation=%r is not restated for "
                                          "the device (only %s); use device_decode=False" % (interpolation, ", ".join(
                                              k for k, v in _PIL_INTERPOLATION_METHODS.items() if v in device_staging.RESTATED)))
        if self.device_prep:
            fn = image_data_generator.preprocessing_function
            if fn is not None and getattr(fn, "_dj_device_prep", None) != PREP_CAFFE:
                raise NotImplementedError("flow_from_directory(device_prep=True): preprocessing_function=%r cannot run on the "
                                          "device (only keras.applications.vgg16.preprocess_input or None)" % (fn,))
            self._prep_code = PREP_NONE if fn is None else PREP_CAFFE
            self._stager = device_staging.StagingBuffers(decode_threads) if self.device_decode else RGBWarpStager()
        if not classes:
            classes = sorted(d for d in os.listdir(directory) if os.path.isdir(os.path.join(directory, d)))
        self.num_classes = len(classes)
        self.class_indices = dict(zip(classes, range(len(classes))))
        self.filenames, labels = [], []
        for name in classes:
            sub = os.path.join(directory, name)
            for root, fname in _valid_files(sub, follow_links):
                self.filenames.append(os.path.join(name, os.path.relpath(os.path.join(root, fname), sub)))
                labels.append(self.class_indices[name])
        self.classes = np.asarray(labels, dtype="int32")
        self.samples = len(self.filenames)
        print("Found %d images belonging to %d classes." % (self.samples, self.num_classes))
        self.n, self.batch_size, self.seed, self.shuffle = self.samples, int(batch_size), seed, shuffle
        self.batch_index, self.total_batches_seen = 0, 0
        self.lock = threading.Lock()
        self.index_array = None
        self.index_generator = self._flow_index()

    # ---- Keras' Iterator ------------------------------------------------------------------------------------------------
    def _set_index_array(self):
        self.index_array = np.arange(self.n)
        if self.shuffle:
            self.index_array = np.random.permutation(self.n)

    def __len__(self):
        return (self.n + self.batch_size - 1) // self.batch_size

    def __getitem__(self, idx):
        if idx >= len(self):
            raise ValueError("Asked to retrieve element {idx}, but the Sequence has length {length}".format(idx=idx,
                                                                                                         length=len(self)))
        if self.seed is not None:
            np.random.seed(self.seed + self.total_batches_seen)
        self.total_batches_seen += 1
        if self.index_array is None:
            self._set_index_array()
        return self._get_batches_of_transformed_samples(self.index_array[self.batch_size * idx:self.batch_size * (idx + 1)])

    def on_epoch_end(self):
        self._set_index_array()

    def reset(self):
        self.batch_index = 0

    def _flow_index(self):
        self.reset()
        while True:
            if self.seed is not None:
                np.random.seed(self.seed + self.total_batches_seen)
            if self.batch_index == 0:
                self._set_index_array()
            current = (self.batch_index * self.batch_size) % self.n if self.n else 0
            if self.n > current + self.batch_size:
                self.batch_index += 1
            else:
                self.batch_index = 0
            self.total_batches_seen += 1
            yield self.index_array[current:current + self.batch_size]

    def __iter__(self):
        return self

    def __next__(self):
        return self.next()

    def next(self):
        with self.lock:
            index_array = next(self.index_generator)
        return self._get_batches_of_transformed_samples(index_array)

    # ---- one batch -------------------------------------------------------------------------------------------------------
    def _labels(self, index_array):
        y = np.zeros((len(index_array), self.num_classes), dtype=np.float32)
        y[np.arange(len(index_array)), self.classes[index_array]] = 1.
        return y

    def _file_batch(self, index_array):
        """The `device_decode` batch: the draws of the `device_prep` batch in the same order, no pixel touched."""
        from ...data.jpeg_pixels import read_image
        gen = self.image_data_generator
        images, records = [], []
        for j in index_array:
            images.append(read_image(os.path.join(self.directory, self.filenames[j])))
            records.append(gen.transform_record(self.image_shape, gen.get_random_transform(self.image_shape)))
        gen._warn_unfit()      # the warning of the host path's `standardize`
        return PendingRGBFileInputs(images, pack_records(records), self.target_size, self._resample, self._prep_code,
                                    gen.rescale if gen.rescale else None, self._stager)

    def _get_batches_of_transformed_samples(self, index_array):
        gen = self.image_data_generator
        if self.device_decode:
            batch_x = self._file_batch(index_array)
            return batch_x if self.class_mode is None else (batch_x, self._labels(index_array))
        if self.device_prep:
            pixels = np.empty((len(index_array),) + self.image_shape, dtype=np.uint8)
            records = []
        else:
            batch_x = np.zeros((len(index_array),) + self.image_shape, dtype=np.float32)
        for i, j in enumerate(index_array):
            img = load_img(os.path.join(self.directory, self.filenames[j]), color_mode=self.color_mode,
                           target_size=self.target_size, interpolation=self.interpolation)
            if self.device_prep:
                pixels[i] = np.asarray(img, dtype=np.uint8)
                records.append(gen.transform_record(self.image_shape, gen.get_random_transform(self.image_shape)))
            else:
                x = img_to_array(img)
                x = gen.apply_transform(x, gen.get_random_transform(x.shape))
                batch_x[i] = gen.standardize(x)
            if hasattr(img, "close"):
                img.close()
        if self.device_prep:
            gen._warn_unfit()      # the warning of the host path's `standardize`
            batch_x = PendingRGBInputs(pixels, pack_records(records), self._prep_code,
                                       gen.rescale if gen.rescale else None, self._stager)
        if self.class_mode is None:
            return batch_x
        return batch_x, self._labels(index_array)
