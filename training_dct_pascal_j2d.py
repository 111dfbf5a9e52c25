#!/usr/bin/env python
"""Drop-in for localisation_part/training_dct_pascal_j2d.py, the trainer of the VGG-DCT SSD300 (`ssd_300DCT` with --reg,
`ssd_300DCT_no_reg` with --no_reg): same flags, same model / optimizer / loss / encoder / callback set-up, running on
MI355X.  There is no --archi and no --restart: the reference's script has neither.

    python3 training_dct_pascal_j2d.py -vd 0 --crop --p07p12 --reg --vgg --weights vggd_dct_checkpoint.npz

Data, environment variables (DATASET_PATH, DJ_DEVICE_PREP, DJ_DEVICE_DECODE, DJ_PHOTOMETRIC, DJ_DEVICE_ENCODER), the
optional arguments and multi-GPU launch are those of training_dct_pascal_j2d_resnet.py: both scripts run
jpeg_detection_resnet_ssd_amd/ssd_training.py.

`--weights`: the reference opens the checkpoint with `load_model` to list its layers, refuses one that holds a layer the
detector would not load, then calls `load_weights(by_name=True)`.  Checkpoints here are .npz name->array archives, so the
layer names are read from the archive's keys and the same check runs on them: with --vgg (a `vggd_dct` classifier
checkpoint) the classifier's tail pool5 / flatten / dropout_1 / dropout_2 / fc1 / fc2 / predictions is ignored and any other
unknown layer is a NameError; with --ssd every layer must exist in the detector.
"""
from argparse import ArgumentParser

from jpeg_detection_resnet_ssd_amd import ssd_training

parser = ArgumentParser(description="Script to train the SSD on the pascal voc dataset.")
parser.add_argument("--weights", default=None, help="The weights to load into the model")
parser.add_argument("-vd", "--visible_device", help="The device to use when training with the GPU", default="-1")
loading_check = parser.add_mutually_exclusive_group(required=True)
loading_check.add_argument("--ssd", action="store_true")
loading_check.add_argument("--vgg", action="store_true")
ssd_training.add_common_arguments(parser)
args = parser.parse_args()

ssd_training.prepare_environment(args)

from jpeg_detection_resnet_ssd_amd.models.keras_ssd300_dct_j2d import ssd_300DCT  # noqa: E402
from jpeg_detection_resnet_ssd_amd.models.keras_ssd300_dct_j2d_no_regularizer import ssd_300DCT_no_reg  # noqa: E402

rank, world, local = ssd_training.init_distributed()

if args.no_reg:
    model = ssd_300DCT_no_reg(**ssd_training.ssd_args())
elif args.reg:
    model = ssd_300DCT(**ssd_training.ssd_args())
else:
    raise Exception("Network selection error.")

if args.weights:
    ignored = ssd_training.check_checkpoint_layers(ssd_training.checkpoint_layer_names(args.weights),
                                                   [layer.name for layer in model.layers], vgg=args.vgg, ssd=args.ssd)
    for name in ignored:
        print("Ignoring layer: {}".format(name))
    model.load_weights(args.weights, by_name=True)

history = ssd_training.train(model, args, rank, world)
