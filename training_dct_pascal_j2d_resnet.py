#!/usr/bin/env python
"""Drop-in for localisation_part/training_dct_pascal_j2d_resnet.py: same flags (including the required-but-unused
ones), same environment variables, same model / optimizer / loss / encoder / callback set-up, running on MI355X.

    python3 training_dct_pascal_j2d_resnet.py -vd 0 --crop --p07p12 --reg --resnet --archi ssd_custom

Differences, all forced by what is absent offline: the Pascal-VOC DataGeneratorDCT (PIL / cv2 / jpeg2dct) is
replaced by a synthetic JPEG-DCT generator with the same emission contract unless `DATASET_PATH` points at a Pascal-VOC
tree in the reference's layout (VOC2007/ and, with --p07p12, VOC2012/, each with JPEGImages, Annotations and
ImageSets/Main: then data/voc_generator.py reads it, augmented by data/ssd_augment.py as --crop / --no_crop select, on
the host or, with `DJ_DEVICE_PREP=1`, planned on the host and run on the GPU; `DJ_DEVICE_DECODE=1` on top of that leaves
the pixel half of JPEG decoding to the GPU too) or `--generator module:factory` names a
user-supplied one; checkpoints are .npz name->array archives (h5py is not installed); `--weights` goes straight to
`load_weights(by_name=True)` (the reference's preceding `load_model` only prints a summary).
Multi-GPU (not in the reference: "no multi-GPU support for this part") = one process per GPU:
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 training_dct_pascal_j2d_resnet.py ...
"""
import os
from argparse import ArgumentParser

from jpeg_detection_resnet_ssd_amd import ssd_training

parser = ArgumentParser(description="Script to train the SSD Resnet on the pascal voc dataset.")
parser.add_argument("--weights", default=None, help="The weights to load into the model")
parser.add_argument("-vd", "--visible_device", help="The device to use when training with the GPU", default="-1")
parser.add_argument("--restart", default=None, help="Wether the simulation starts from a previous save")
parser.add_argument("--archi", help="""The network architecture to use, value can be :\n
* cb5_only : CbCr and Y only go through the conv block 5 of Resnet50\n
* deconv : deconvolution architecture of Uber article\n
* up_sampling : up sampling architecture of Uber article\n
* y_cb4_cbcr_cb5 :Y go through the conv block 4 of Resnet50 and CbCr go through conv block 5\n
* ssd_custom : the extra-feature layers of SSD are removed to match dimension with full Late-concat-RFA architecture of Uber
""")
loading_check = parser.add_mutually_exclusive_group(required=True)
loading_check.add_argument("--ssd", action="store_true")
loading_check.add_argument("--resnet", action="store_true")
ssd_training.add_common_arguments(parser)
args = parser.parse_args()

ssd_training.prepare_environment(args)
deconv = args.archi == "deconv"

from jpeg_detection_resnet_ssd_amd.models.keras_ssd300_dct_j2d_resnet import (ssd_resnet_EF_layers_custom,  # noqa: E402
                                                                             ssd_resnet_EF_layers_identical)

rank, world, local = ssd_training.init_distributed()

ssd_args = dict(ssd_training.ssd_args(), archi=args.archi)
if args.archi == "ssd_custom":
    model = ssd_resnet_EF_layers_custom(**ssd_args)
else:
    model = ssd_resnet_EF_layers_identical(**ssd_args)

if args.restart:
    model.load_weights(args.restart, by_name=True)
elif args.weights:
    model.load_weights(args.weights, by_name=True)

if args.restart:
    # "..._epoch-{epoch:02d}_loss-..." (the ModelCheckpoint pattern of ssd_training.train).  The reference parses the whole
    # path (`args.restart.split('-')[1]`), which breaks on a directory name containing '-'; the file name alone is parsed here
    initial_epoch = int(os.path.basename(args.restart).split("-")[1].split("_")[0])
else:
    initial_epoch = 0
history = ssd_training.train(model, args, rank, world, deconv=deconv, initial_epoch=initial_epoch)
