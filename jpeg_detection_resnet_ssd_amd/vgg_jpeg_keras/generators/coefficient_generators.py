"""Classifier generators that feed pre-sized JPEG files to the models as their OWN DCT coefficients
(data/coefficient_inputs.py): no decoding to pixels, no resize, no re-encoding.  The surface is that of generators.py -- a
directory of class directories, an ImageNet-style index file, `[X_y, X_cbcr]` (DCTGeneratorCoefficients) or
`[X_y, X_cb, X_cr]` (DCTGeneratorCoefficientsDeconv) with one-hot labels -- and, as in the reference's DCTGeneratorImageNet,
a file's coefficients are read as they are.

Per image, in this order: the bytes and the header are read; `random.randint(0, height // 16 - T // 16)` draws the row
origin and `random.randint(0, width // 16 - T // 16)` the column origin of a T x T window, in whole MCUs of the real image
(`random_crop=False`: no draw, the centred window `(n - T // 16) // 2`); `random.uniform(0, 1) > 0.5` draws the mirror
(`flip=True` only).  A file smaller than the target, or one that is not eligible (not baseline, not 4:2:0 or gray), is a
ValueError naming its path: files are expected to be pre-sized (tools/presize_dataset.py).

`device=True` returns `(PendingCoefficientInputs, y)`: the entropy decoding runs on `decode_threads` host threads and the
window, mirror and de-quantisation on the GPU when the model uploads the batch.  `device_entropy=True` on top of it: a
batch whose files all carry restart intervals (tools/presize_dataset.py --restart-rows / --restart-mcus) is entropy-decoded
on the GPU too, from the files' bytes, with no host thread; any other batch takes the host threads (`host_batches` counts
them).  `unmarked=True` on top of that: batches with ordinary files, which carry no restart intervals, are entropy-decoded on
the GPU as well, by chunks (`chunk_bytes`); only a batch with a file that even the wider pre-pass refuses takes the host
threads.  `device=False` returns the host statement's
arrays.  Both make the same draws and leave `random` in the same state."""
import os
import random

import numpy as np

from ...data.coefficient_inputs import MCU, DeviceCoefficientInputs, check_file, coefficient_inputs_host
from ...keras.utils import Sequence
from .generators import prepare_imagenet


class DCTGeneratorCoefficients(Sequence):
    """Batches of `[X_y, X_cbcr]` ((B, T/8, T/8, 64), (B, T/16, T/16, 128)) and one-hot labels."""
    deconv = False

    def __init__(self, data_directory, index_file, batch_size=32, shuffle=True, target_length=224, random_crop=True,
                 flip=True, device=True, decode_threads=None, device_entropy=False, unmarked=False, chunk_bytes=None):
        if int(target_length) < MCU or int(target_length) % MCU:
            raise ValueError("target_length must be a positive multiple of %d, got %r" % (MCU, target_length))
        if device_entropy and not device:
            raise ValueError("device_entropy needs device=True: the files are entropy-decoded where the batch is uploaded")
        if unmarked and not device_entropy:
            raise ValueError("unmarked needs device_entropy=True: it widens what is entropy-decoded on the GPU")
        self.association, self.classes, self.images_path = prepare_imagenet(index_file, data_directory)
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.number_of_data_samples = len(self.images_path)
        self.target_length = int(target_length)
        self.random_crop = bool(random_crop)
        self.flip = bool(flip)
        self.device = bool(device)
        self.number_of_classes = len(self.classes)
        self.batches_per_epoch = len(self.images_path) // self.batch_size
        self.indexes = np.arange(len(self.images_path))
        self._emit = DeviceCoefficientInputs(deconv=self.deconv, n_threads=decode_threads,
                                             device_entropy=device_entropy, unmarked=unmarked,
                                             chunk_bytes=chunk_bytes) if device else None
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

    def _read(self, path):
        with open(path, "rb") as f:
            data = f.read()
        try:
            image = check_file(data)
        except ValueError as e:
            raise ValueError("%s: %s" % (path, e))
        image.name = path      # for the message of a failure that is only found on the GPU
        return image

    def check_inputs(self):
        """Wait for the batches handed to a model and raise the ValueError of one whose entropy decoding failed on the GPU
        (`device_entropy=True`: such a failure is found behind the batch).  `evaluate_generator` and `fit_generator` call
        it when a sweep or an epoch ends."""
        if self._emit is not None:
            self._emit.check()

    @property
    def host_batches(self):
        """Batches that `device_entropy=True` could not take because a file had no restart intervals (with
        `unmarked=True`: because a file failed the wider pre-pass too)."""
        return self._emit.host_batches if self._emit is not None else 0

    def _draws(self, path, height, width):
        """-> ((y0, x0, T, T), mirror) of one image, drawn from `random` in the module's order."""
        t = self.target_length // MCU
        free = (height // MCU - t, width // MCU - t)
        if min(free) < 0:
            raise ValueError("%s: %d x %d holds no %d x %d window of whole MCUs: pre-size the files"
                             % (path, height, width, self.target_length, self.target_length))
        if self.random_crop:
            origin = [random.randint(0, free[0]), random.randint(0, free[1])]
        else:
            origin = [free[0] // 2, free[1] // 2]
        mirror = bool(self.flip and random.uniform(0, 1) > 0.5)
        return (MCU * origin[0], MCU * origin[1], self.target_length, self.target_length), mirror

    def _data_generation(self, indexes):
        y = np.zeros((len(indexes), self.number_of_classes), dtype=np.float32)
        images, windows, flips = [], [], []
        for i, k in enumerate(indexes):
            path = self.images_path[k]
            image = self._read(path)
            window, mirror = self._draws(path, image.shape[0], image.shape[1])
            images.append(image)
            windows.append(window)
            flips.append(mirror)
            y[i, self._label(path)] = 1
        if self.device:
            return self._emit(images, windows, flips), y
        return coefficient_inputs_host(images, windows, flips, deconv=self.deconv), y


class DCTGeneratorCoefficientsDeconv(DCTGeneratorCoefficients):
    """Batches of `[X_y, X_cb, X_cr]` ((B, T/8, T/8, 64) and twice (B, T/16, T/16, 64)) and one-hot labels."""
    deconv = True
