#!/usr/bin/env python
"""Drop-in for classification_part/evaluate.py: the positional `experiment` (an experiment directory as training.py lays
it out) and `weights` (a checkpoint of that experiment), the same sequence of calls on the experiment's saved
configuration, and the evaluator's report at the end, running on MI355X.

    python3 evaluate.py experiments/<experiment> experiments/<experiment>/checkpoints/<weights> --archi deconv

The configuration is `config/saved_config.py` of the experiment directory, which is what training.py writes; the name the
reference imports, `config/temp_config.py`, is read when that file is absent.  `--archi` is needed for the same reason as
in training.py: the configuration builds its network from it.  The data comes from `prepare_testing_generator`
(`DJ_TEST_DIR` or `DJ_VAL_DIR` with `DJ_INDEX_FILE`, else synthetic batches)."""
import argparse
import importlib
import sys
from os.path import isfile, join

parser = argparse.ArgumentParser()
parser.add_argument("experiment", help="Experiment directory written by training.py.")
parser.add_argument("weights", help="Weights file to evaluate, usually one of the experiment's checkpoints.")
parser.add_argument("--archi", default="late_concat_rfa_thinner", help="Network architecture, as given to training.py "
                    "(the ResNet50-DCT names, resnet_rgb, vggA_dct or vggD_dct).")
args = parser.parse_args()

DCT_ARCHIS = ["cb5_only", "deconv", "up_sampling", "up_sampling_rfa", "y_cb4_cbcr_cb5", "late_concat_rfa_thinner",
              "late_concat_more_channels"]

config_dir = join(args.experiment, "config")
sys.path.append(config_dir)
module = "saved_config" if isfile(join(config_dir, "saved_config.py")) or not isfile(join(config_dir, "temp_config.py")) \
    else "temp_config"
TrainingConfiguration = importlib.import_module(module).TrainingConfiguration
# evaluation never starts from the Keras ImageNet weights: the checkpoint is loaded below
if args.archi in DCT_ARCHIS:
    config = TrainingConfiguration(deconv=args.archi == "deconv", archi=args.archi, load_pretrained_weights=False)
elif args.archi == "resnet_rgb":
    config = TrainingConfiguration(load_pretrained_weights=False)
else:
    config = TrainingConfiguration()

config.prepare_for_inference()
config.prepare_testing_generator()
config.prepare_evaluator()

model = config.network
model.load_weights(args.weights)
model.compile(loss=config.loss, optimizer=config.optimizer, metrics=config.metrics)

evaluator = config.evaluator
evaluator(model, config.test_generator)
print(evaluator)
evaluator.display_results()
