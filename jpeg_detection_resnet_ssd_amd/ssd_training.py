"""What the two Pascal-VOC SSD trainers share (training_dct_pascal_j2d_resnet.py and training_dct_pascal_j2d.py at the
repository root, drop-ins for the scripts of the same names in localisation_part/): the flag groups both parsers have, the
working-directory set-up, the reference's builder arguments, and everything from `model.compile` to `fit_generator`.
Each script keeps what is its own: its loading-check flags, its model builder and how it treats `--weights`."""
import importlib
import os
from math import ceil

IMG_HEIGHT, IMG_WIDTH, IMG_CHANNELS = 300, 300, 3
N_CLASSES = 20
SCALES = [0.1, 0.2, 0.37, 0.54, 0.71, 0.88, 1.05]
ASPECT_RATIOS = [[1.0, 2.0, 0.5], [1.0, 2.0, 0.5, 3.0, 1.0 / 3.0], [1.0, 2.0, 0.5, 3.0, 1.0 / 3.0],
                 [1.0, 2.0, 0.5, 3.0, 1.0 / 3.0], [1.0, 2.0, 0.5], [1.0, 2.0, 0.5]]
TWO_BOXES_FOR_AR1 = True
STEPS = [8, 16, 32, 64, 100, 300]
OFFSETS = [0.5, 0.5, 0.5, 0.5, 0.5, 0.5]
CLIP_BOXES = False
VARIANCES = [0.1, 0.1, 0.2, 0.2]
NORMALIZE_COORDS = True

# Layers of a VGG-DCT classifier checkpoint that the detector has no use for (training_dct_pascal_j2d.py:126)
VGG_IGNORED_LAYERS = ("pool5", "flatten", "dropout_1", "dropout_2", "fc1", "fc2", "predictions")


def ssd_args():
    """The builder arguments both reference trainers pass (training_dct_pascal_j2d.py:92-103)."""
    return {"image_size": (IMG_HEIGHT, IMG_WIDTH, IMG_CHANNELS), "n_classes": N_CLASSES, "mode": "training",
            "l2_regularization": 0.0005, "scales": SCALES, "aspect_ratios_per_layer": ASPECT_RATIOS,
            "two_boxes_for_ar1": TWO_BOXES_FOR_AR1, "steps": STEPS, "offsets": OFFSETS, "clip_boxes": CLIP_BOXES,
            "variances": VARIANCES, "normalize_coords": NORMALIZE_COORDS}


def add_common_arguments(parser):
    """The three required flag pairs both reference parsers end with, then this repository's optional additions."""
    ssd_augmentation = parser.add_mutually_exclusive_group(required=True)
    ssd_augmentation.add_argument("--crop", action="store_true")
    ssd_augmentation.add_argument("--no_crop", action="store_true")
    training_set = parser.add_mutually_exclusive_group(required=True)
    training_set.add_argument("--p07", action="store_true")
    training_set.add_argument("--p07p12", action="store_true")
    regularizer = parser.add_mutually_exclusive_group(required=True)
    regularizer.add_argument("--reg", action="store_true")
    regularizer.add_argument("--no_reg", action="store_true")
    # additions (all optional)
    parser.add_argument("--generator", default=None, help="module:factory returning (train_gen_obj, val_gen_obj) with the "
                        "DataGeneratorDCT.generate()/get_dataset_size() surface; default: synthetic JPEG-DCT data")
    parser.add_argument("--epochs", type=int, default=480)
    parser.add_argument("--steps_per_epoch", type=int, default=1000)
    parser.add_argument("--batch_size", type=int, default=32)
    parser.add_argument("--synthetic_images", type=int, default=2048)


def prepare_environment(args):
    """Device selection and the LOCAL_WORK_DIR / EXPERIMENTS_OUTPUT_DIRECTORY directories; runs before torch is imported."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1 and args.visible_device not in ("-1", ""):
        os.environ["HIP_VISIBLE_DEVICES"] = args.visible_device       # CUDA_VISIBLE_DEVICES of the reference
    os.environ["CUDA_VISIBLE_DEVICES_REQUESTED"] = args.visible_device
    if "LOCAL_WORK_DIR" not in os.environ:
        os.environ["LOCAL_WORK_DIR"] = "./" + args.visible_device
    else:
        os.environ["LOCAL_WORK_DIR"] = os.path.join(os.environ["LOCAL_WORK_DIR"], args.visible_device)
    os.makedirs(os.environ["LOCAL_WORK_DIR"], exist_ok=True)
    os.environ.setdefault("EXPERIMENTS_OUTPUT_DIRECTORY", os.environ["LOCAL_WORK_DIR"])
    os.makedirs(os.environ["EXPERIMENTS_OUTPUT_DIRECTORY"], exist_ok=True)


def init_distributed():
    """-> (rank, world, local rank); selects the local GPU."""
    import torch
    from . import dist as djdist
    rank, world, local = djdist.init_from_env()
    if torch.cuda.is_available():
        torch.cuda.set_device(local)
    return rank, world, local


def check_checkpoint_layers(checkpoint_layers, model_layers, vgg=False, ssd=False):
    """The reference trainer's check before `load_weights(by_name=True)` (training_dct_pascal_j2d.py:118-132), stated on
    names: `checkpoint_layers` are the layers the checkpoint holds, `model_layers` those of the model being loaded.  With
    `vgg` (a VGG-DCT classifier checkpoint) the classifier's own tail may be left behind; with `ssd` nothing may.
    -> the names that are ignored, in checkpoint order."""
    if not (vgg or ssd):
        raise Exception("Error, the type of check should have been specified.")
    model_layers = set(model_layers)
    ignored = []
    for name in checkpoint_layers:
        if name in model_layers:
            continue
        if not vgg or name not in VGG_IGNORED_LAYERS:
            raise NameError("The model you are trying to load contains weights that will not be loaded: {}".format(name))
        ignored.append(name)
    return ignored


def checkpoint_layer_names(path):
    """Layer names of an .npz checkpoint, in file order: its keys are '<layer>/<weight>' (Model.save_weights)."""
    import numpy as np
    names = []
    with np.load(path, allow_pickle=False) as z:
        for key in z.files:
            layer = key.rsplit("/", 1)[0]
            if layer not in names:
                names.append(layer)
    return names


def train(model, args, rank, world, deconv=False, initial_epoch=0):
    """Compile `model` as the reference does, build the generators `args` and the environment select, and run
    fit_generator with the reference's callbacks.  -> the History."""
    from . import dist as djdist
    from .keras.callbacks import (CSVLogger, EarlyStopping, ModelCheckpoint, ReduceLROnPlateau, TensorBoard,
                                  TerminateOnNaN)
    from .keras.optimizers import SGD
    from .keras_loss_function.keras_ssd_loss import SSDLoss
    from .ssd_encoder_decoder.ssd_input_encoder import SSDInputEncoder

    img_height, img_width, n_classes = IMG_HEIGHT, IMG_WIDTH, N_CLASSES
    sgd = SGD(lr=0.001, momentum=0.9, decay=0.0, nesterov=False)
    ssd_loss = SSDLoss(neg_pos_ratio=3, alpha=1.0)
    model.compile(optimizer=sgd, loss=ssd_loss.compute_loss)
    if world > 1:
        dp = djdist.DataParallel(model)
        dp.broadcast_weights(0)

    if args.generator:
        mod, fn = args.generator.split(":")
        train_dataset, val_dataset = getattr(importlib.import_module(mod), fn)(args)
    elif os.environ.get("DATASET_PATH"):
        from .data.voc_generator import DataGeneratorDCT
        years = ["VOC2007", "VOC2012"] if args.p07p12 else ["VOC2007"]
        dirs = [os.path.join(os.environ["DATASET_PATH"], y) for y in years]
        train_dataset, val_dataset = DataGeneratorDCT(), DataGeneratorDCT()
        for dataset, image_set, exclude_difficult in ((train_dataset, "train.txt", False), (val_dataset, "val.txt", True)):
            dataset.parse_xml(images_dirs=[os.path.join(d, "JPEGImages") for d in dirs],
                              image_set_filenames=[os.path.join(d, "ImageSets", "Main", image_set) for d in dirs],
                              annotations_dirs=[os.path.join(d, "Annotations") for d in dirs], include_classes="all",
                              exclude_truncated=False, exclude_difficult=exclude_difficult, ret=False)
    else:
        from .data.generators import SyntheticDataGeneratorDCT
        train_dataset = SyntheticDataGeneratorDCT(n_images=args.synthetic_images, seed=1234 + 100000 * rank)
        val_dataset = SyntheticDataGeneratorDCT(n_images=max(args.batch_size, args.synthetic_images // 8), seed=987654)

    batch_size = args.batch_size
    predictor_sizes = [model.get_layer("%s_mbox_conf_%d" % (n, n_classes + 1)).output_shape[1:3]
                       for n in ("conv4_3_norm", "fc7", "conv6_2", "conv7_2", "conv8_2", "conv9_2")]
    ssd_input_encoder = SSDInputEncoder(img_height=img_height, img_width=img_width, n_classes=n_classes,
                                        predictor_sizes=predictor_sizes, scales=SCALES,
                                        aspect_ratios_per_layer=ASPECT_RATIOS, two_boxes_for_ar1=TWO_BOXES_FOR_AR1,
                                        steps=STEPS, offsets=OFFSETS, clip_boxes=CLIP_BOXES, variances=VARIANCES,
                                        matching_type="multi", pos_iou_threshold=0.5, neg_iou_limit=0.5,
                                        normalize_coords=NORMALIZE_COORDS)
    label_encoder = ssd_input_encoder
    if os.environ.get("DJ_DEVICE_ENCODER", "1") != "0":
        # same encodings (tests/test_encode_gpu.py), computed on the GPU at upload time instead of ~7 ms/image of host numpy
        from .ssd_encoder_decoder.ssd_input_encoder import DeviceLabelEncoder
        label_encoder = DeviceLabelEncoder(ssd_input_encoder)
    emit_kwargs = {}
    if os.environ.get("DJ_DEVICE_DCT", "0") == "1":
        # opt-in: the generators hand over uint8 pixels and the JPEG transform (what PIL save + jpeg2dct.loads compute,
        # tests/test_rgb_dct_gpu.py) runs on the GPU at upload time
        from .data.jpeg_dct import DeviceDCTEmitter
        emit_kwargs["dct_emitter"] = DeviceDCTEmitter(quality=75, deconv=deconv)
    train_transformations, val_transformations = [], []
    if os.environ.get("DATASET_PATH") and not args.generator:
        # the reference's chains, its plain Resize for validation.  Their photometric stage (brightness, contrast, saturation
        # and hue jitter, data/ssd_photometric.py) is opt-in: DJ_PHOTOMETRIC=1, on the host path and, with DJ_DEVICE_PREP=1, on
        # the GPU (tests/test_ssd_photometric_gpu.py); validation is never distorted
        from .data.ssd_augment import Resize, SSDDataAugmentation, SSDDataAugmentationNoCrop, SSDPhotometricDistortions
        chain = SSDDataAugmentation if args.crop else SSDDataAugmentationNoCrop
        photometric = SSDPhotometricDistortions() if os.environ.get("DJ_PHOTOMETRIC", "0") == "1" else None
        train_transformations = [chain(img_height=img_height, img_width=img_width, photometric_distortions=photometric)]
        val_transformations = [Resize(height=img_height, width=img_width)]
        emit_kwargs.pop("dct_emitter", None)      # the VOC generator's device switch is DJ_DEVICE_PREP
        if os.environ.get("DJ_DEVICE_PREP", "0") == "1":
            # opt-in: the generator decodes and plans, window + mirror + resize + JPEG transform run on the GPU at upload time
            # (tests/test_ssd_augment_gpu.py)
            from .data.patch_resize import DevicePatchResize
            emit_kwargs["device_prep"] = DevicePatchResize(img_height, img_width, quality=75, deconv=deconv,
                                                           n_threads=int(os.environ.get("DJ_DECODE_THREADS", "16")))
            if os.environ.get("DJ_DEVICE_DECODE", "0") == "1":
                # opt-in on top: files travel as entropy-decoded coefficients (read on DJ_DECODE_THREADS host threads, default
                # 16) and dj_jpeg_pixels makes the staged pixels
                # (tests/test_jpeg_pixels_gpu.py); files it does not cover are decoded with Pillow as before
                emit_kwargs["device_decode"] = True
        elif os.environ.get("DJ_DEVICE_DECODE", "0") == "1":
            raise SystemExit("DJ_DEVICE_DECODE=1 needs DJ_DEVICE_PREP=1")
    train_generator = train_dataset.generate(batch_size=batch_size, shuffle=True, transformations=train_transformations,
                                             label_encoder=label_encoder,
                                             returns={"processed_images", "encoded_labels"},
                                             keep_images_without_gt=False, deconv=deconv, **emit_kwargs)
    val_generator = val_dataset.generate(batch_size=batch_size, shuffle=False, transformations=val_transformations,
                                         label_encoder=label_encoder, returns={"processed_images", "encoded_labels"},
                                         keep_images_without_gt=False, deconv=deconv, **emit_kwargs)
    train_dataset_size = train_dataset.get_dataset_size()
    val_dataset_size = val_dataset.get_dataset_size()
    if rank == 0:
        print("Number of images in the training dataset:\t{:>6}".format(train_dataset_size))
        print("Number of images in the validation dataset:\t{:>6}".format(val_dataset_size))

    callbacks = [ReduceLROnPlateau(monitor="val_loss", factor=0.1, patience=7), TerminateOnNaN(),
                 TensorBoard(log_dir=os.path.join(os.environ["LOCAL_WORK_DIR"], "./logs")),
                 EarlyStopping(monitor="val_loss", min_delta=0, patience=10)]
    if rank == 0:
        out_dir = os.environ["EXPERIMENTS_OUTPUT_DIRECTORY"]
        callbacks = [ModelCheckpoint(filepath=os.path.join(
            out_dir, "ssd300_pascal_07+12_epoch-{epoch:02d}_loss-{loss:.4f}_val_loss-{val_loss:.4f}.h5"),
            monitor="val_loss", verbose=1, save_best_only=True, save_weights_only=False, mode="auto", period=1),
            CSVLogger(filename=os.path.join(out_dir, "ssd300_pascal_07+12_training_log.csv"), separator=",",
                      append=True)] + callbacks

    return model.fit_generator(generator=train_generator, steps_per_epoch=args.steps_per_epoch, epochs=args.epochs,
                               callbacks=callbacks, validation_data=val_generator,
                               validation_steps=ceil(val_dataset_size / batch_size), initial_epoch=initial_epoch)
