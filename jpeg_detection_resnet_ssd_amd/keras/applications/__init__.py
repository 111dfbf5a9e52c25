"""keras.applications bits the reference imports."""
from . import imagenet_utils, vgg16  # noqa: F401
