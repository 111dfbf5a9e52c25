"""What config/vggA_dct/config_file.py and config/vggD_dct/config_file.py share: the TrainingConfiguration surface of
config/resnet/config_file.py (same properties, same DJ_* environment rules, same synthetic fallback) with the settings of
classification_part/config/vggA_dct/config_file.py and config/vggD_dct/config_file.py.  The two files differ in the
builder and the project name only, so each is a subclass that names them; a saved copy of either (training.py writes
`saved_config.py` into the experiment folder) stays loadable because this module lives in the package.

Data: with `DJ_TRAIN_DIR`, `DJ_VAL_DIR` and `DJ_INDEX_FILE` all set, DCTGeneratorJPEG2DCT reads real images -- the training
one with `scale=True` and the four photometric transformations when `DJ_PHOTOMETRIC=1`, the validation one with
`scale=False`; `DJ_DEVICE_PREP=1` moves resize, crop, flip and the JPEG transform to the GPU, and `DJ_DEVICE_DECODE=1` on
top of it (an error without it) the decoding of baseline JPEG files, read on `DJ_DECODE_THREADS` host threads (default 16).
`DJ_COEFFICIENT_INPUTS=1` (with none of those switches, else an error) feeds pre-sized baseline 4:2:0 files as their own
coefficients instead (generators/coefficient_generators.py): random window and mirror for training, the centred window for
validation and test.  Otherwise synthetic
[Y 28x28x64, CbCr 14x14x128] batches with one-hot labels.  `prepare_testing_generator` reads `DJ_TEST_DIR`, or `DJ_VAL_DIR`
without it, with `DJ_INDEX_FILE`."""
from os import environ
from os.path import join

import numpy as np

from ..data import synthetic_dct as sd
from ..keras.callbacks import CSVLogger, EarlyStopping, ModelCheckpoint, ReduceLROnPlateau, TerminateOnNaN
from ..keras.losses import categorical_crossentropy
from ..keras.metrics import top_k_categorical_accuracy
from ..keras.optimizers import SGD
from ..keras.utils import Sequence
from .evaluation import Evaluator


def _top_k_accuracy(k):
    def _func(y_true, y_pred):
        return top_k_categorical_accuracy(y_true, y_pred, k)
    _func._dj_metric = ("top_k", k)      # a validation / evaluation sweep counts it on the device, without calling it
    return _func


class SyntheticVGGDCTGenerator(Sequence):
    """Batches ([Y, CbCr], one-hot labels) shaped like DCTGeneratorJPEG2DCT output at 224x224."""

    def __init__(self, batch_size, num_classes=1000, n_batches=64, seed=0):
        self.batch_size, self.num_classes, self.n_batches, self.seed = batch_size, num_classes, n_batches, seed

    def __len__(self):
        return self.n_batches

    def __getitem__(self, index):
        x = sd.fast_dct_batch(self.batch_size, seed=self.seed + index, grid=28, split_chroma=False)
        rng = np.random.default_rng(self.seed + 7 * index + 1)
        y = np.zeros((self.batch_size, self.num_classes), dtype=np.float32)
        y[np.arange(self.batch_size), rng.integers(0, self.num_classes, self.batch_size)] = 1.0
        return x, y


class VGGDCTTrainingConfiguration(object):
    def __init__(self, builder, project_name):
        self.description = ""
        self._workers = 4
        self._multiprocessing = True
        self._gpus = 1
        self._project_name = project_name
        self._workspace = "thomasC"
        self.num_classes = 1000
        self.img_size = (224, 224)
        self._weights = None
        self._network = builder(self.num_classes)
        self._epochs = 120
        self._batch_size = 256
        self.batch_size_divider = 4
        self._steps_per_epoch = 5000
        self._validation_steps = 50000 // self._batch_size
        self.optimizer_parameters = {"lr": 0.01, "momentum": 0.9, "decay": 0, "nesterov": True}
        self._optimizer = SGD(**self.optimizer_parameters)
        self._loss = categorical_crossentropy
        self._metrics = [_top_k_accuracy(1), _top_k_accuracy(5)]
        self.train_directory = join(environ.get("DATASET_PATH_TRAIN", ""), "imagenet/train")
        self.validation_directory = join(environ.get("DATASET_PATH_VAL", ""), "imagenet/validation")
        self.index_file = join(environ.get("PROJECT_PATH", ""), "data/imagenet_class_index.json")
        self.model_checkpoint = None
        self.csv_logger = None
        self.terminate_on_nan = TerminateOnNaN()
        self.early_stopping = EarlyStopping(monitor="val_loss", min_delta=0, patience=10)
        self._callbacks = [self.terminate_on_nan, self.early_stopping]
        self._horovod = None
        self._train_generator = None
        self._validation_generator = None
        self._test_generator = None
        self._evaluator = None

    # -- callbacks -------------------------------------------------------------------------------
    def add_csv_logger(self, output_path, filename="results.csv", separator=",", append=True):
        if self.horovod is not None and self.horovod.rank() != 0:
            return
        self.csv_logger = CSVLogger(filename=join(output_path, filename), separator=separator, append=append)
        self._callbacks.append(self.csv_logger)

    def add_model_checkpoint(self, output_path, verbose=1, save_best_only=True):
        if self.horovod is not None and self.horovod.rank() != 0:
            return
        self.model_checkpoint = ModelCheckpoint(
            filepath=join(output_path, "epoch-{epoch:02d}_loss-{loss:.4f}_val_loss-{val_loss:.4f}.h5"),
            verbose=verbose, save_best_only=save_best_only)
        self._callbacks.append(self.model_checkpoint)

    def prepare_horovod(self, hvd):
        """The Horovod rules of config/resnet: lr *= size / 4, per-rank batch = 256 // 4, steps //= size // 4, validation
        steps = 3 * steps // size; broadcast from rank 0, metric averaging, the 5-epoch learning-rate warm-up and
        ReduceLROnPlateau(patience=5)."""
        self._horovod = hvd
        self._callbacks = [hvd.callbacks.BroadcastGlobalVariablesCallback(0), hvd.callbacks.MetricAverageCallback(),
                           hvd.callbacks.LearningRateWarmupCallback(warmup_epochs=5, verbose=1),
                           ReduceLROnPlateau(patience=5, verbose=1), self.terminate_on_nan, self.early_stopping]
        self.optimizer_parameters["lr"] = self.optimizer_parameters["lr"] * hvd.size() / self.batch_size_divider
        self._optimizer = hvd.DistributedOptimizer(SGD(**self.optimizer_parameters))
        self._batch_size = self._batch_size // self.batch_size_divider
        self._steps_per_epoch = self._steps_per_epoch // max(1, hvd.size() // self.batch_size_divider)
        self._validation_steps = 3 * self._validation_steps // hvd.size()

    def prepare_for_inference(self):
        pass

    def prepare_evaluator(self):
        self._evaluator = Evaluator()

    def prepare_testing_generator(self):
        directory = environ.get("DJ_TEST_DIR") or environ.get("DJ_VAL_DIR")
        index_file = environ.get("DJ_INDEX_FILE")
        if directory and index_file:
            from .generators import DCTGeneratorJPEG2DCT, coefficient_switch, device_switches
            self.validation_directory, self.index_file = directory, index_file
            if coefficient_switch():
                self._test_generator = self._coefficient_generator(directory, index_file, training=False)
            else:
                self._test_generator = DCTGeneratorJPEG2DCT(directory, index_file, self._batch_size, scale=False,
                                                            **device_switches())
        else:
            self._test_generator = SyntheticVGGDCTGenerator(self._batch_size, self.num_classes, n_batches=8, seed=999983)

    def _coefficient_generator(self, directory, index_file, training):
        """`DJ_COEFFICIENT_INPUTS=1`: pre-sized files fed as their own coefficients -- a random window and mirror for
        training, the centred window and no mirror for validation and test."""
        from .generators import DCTGeneratorCoefficients, device_entropy_switch, unmarked_switch
        return DCTGeneratorCoefficients(directory, index_file, self._batch_size, target_length=self.img_size[0],
                                        random_crop=training, flip=training,
                                        decode_threads=int(environ.get("DJ_DECODE_THREADS", "16")),
                                        device_entropy=device_entropy_switch(), unmarked=unmarked_switch())

    def prepare_training_generators(self):
        rank = self.horovod.rank() if self.horovod is not None else 0
        real = [environ.get(k) for k in ("DJ_TRAIN_DIR", "DJ_VAL_DIR", "DJ_INDEX_FILE")]
        if all(real):
            from .generators import DCTGeneratorJPEG2DCT, coefficient_switch, device_switches
            self.train_directory, self.validation_directory, self.index_file = real
            if coefficient_switch():
                self._train_generator = self._coefficient_generator(real[0], real[2], training=True)
                self._validation_generator = self._coefficient_generator(real[1], real[2], training=False)
                return
            switches = device_switches()
            transformations = None
            if environ.get("DJ_PHOTOMETRIC", "0") == "1":
                from .generators import brightness, contrast, lighting, saturation
                transformations = [lighting, contrast, brightness, saturation]
            self._train_generator = DCTGeneratorJPEG2DCT(real[0], real[2], self._batch_size, scale=True,
                                                         transformations=transformations, **switches)
            self._validation_generator = DCTGeneratorJPEG2DCT(real[1], real[2], self._batch_size, scale=False, **switches)
        else:
            self._train_generator = SyntheticVGGDCTGenerator(self._batch_size, self.num_classes, seed=1000 * rank)
            self._validation_generator = SyntheticVGGDCTGenerator(self._batch_size, self.num_classes, n_batches=8,
                                                                  seed=999983)

    workers = property(lambda self: self._workers)
    multiprocessing = property(lambda self: self._multiprocessing)
    gpus = property(lambda self: self._gpus)
    project_name = property(lambda self: self._project_name)
    workspace = property(lambda self: self._workspace)
    network = property(lambda self: self._network)
    epochs = property(lambda self: self._epochs)
    batch_size = property(lambda self: self._batch_size)
    steps_per_epoch = property(lambda self: self._steps_per_epoch)
    validation_steps = property(lambda self: self._validation_steps)
    optimizer = property(lambda self: self._optimizer)
    loss = property(lambda self: self._loss)
    metrics = property(lambda self: self._metrics)
    callbacks = property(lambda self: self._callbacks)
    horovod = property(lambda self: self._horovod)
    train_generator = property(lambda self: self._train_generator)
    validation_generator = property(lambda self: self._validation_generator)
    test_generator = property(lambda self: self._test_generator)
    evaluator = property(lambda self: self._evaluator)

    @property
    def weights(self):
        return self._weights

    @weights.setter
    def weights(self, value):
        self._weights = value
