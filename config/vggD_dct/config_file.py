"""Training configuration for `vggd_dct`, the VGG-D classifier on JPEG-DCT inputs: the settings of
classification_part/config/vggD_dct/config_file.py (batch 256, 5000 steps x 120 epochs, Nesterov SGD at lr 0.01,
top-1 / top-5) on the TrainingConfiguration surface of config/resnet/config_file.py.  Everything but the builder and the
project name is shared with config/vggA_dct, in jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.vgg_dct_configuration, whose
docstring states the `DJ_*` data rules.

    python3 training.py -c config/vggD_dct --archi vggD_dct --horovod False --use_pretrained_weights False"""
from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.networks import vggd_dct
from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.vgg_dct_configuration import VGGDCTTrainingConfiguration


class TrainingConfiguration(VGGDCTTrainingConfiguration):
    def __init__(self):
        super(TrainingConfiguration, self).__init__(vggd_dct, "vggD-dct_retrain_for_weights")
