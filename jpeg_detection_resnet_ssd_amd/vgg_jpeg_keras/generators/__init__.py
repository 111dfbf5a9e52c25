from .generators import DCTGeneratorJPEG2DCT, DCTGeneratorJPEG2DCTDeconv, device_switches, prepare_imagenet  # noqa: F401
from .helper import brightness, contrast, grayscale, lighting, saturation  # noqa: F401
