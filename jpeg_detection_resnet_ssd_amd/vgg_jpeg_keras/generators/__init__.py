from .coefficient_generators import DCTGeneratorCoefficients, DCTGeneratorCoefficientsDeconv  # noqa: F401
from .generators import (DCTGeneratorJPEG2DCT, DCTGeneratorJPEG2DCTDeconv, coefficient_switch, device_entropy_switch,  # noqa: F401
                         device_switches, prepare_imagenet, unmarked_switch)
from .helper import brightness, contrast, grayscale, lighting, saturation  # noqa: F401
