from .generators import DCTGeneratorJPEG2DCT, DCTGeneratorJPEG2DCTDeconv, prepare_imagenet  # noqa: F401
