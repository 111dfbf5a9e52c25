"""keras.applications.vgg16: only `preprocess_input`, which the reference's RGB configuration hands to its
ImageDataGenerator (classification_part/config/resnetRGB/config_file.py:12,164,169)."""
from .imagenet_utils import preprocess_input  # noqa: F401
