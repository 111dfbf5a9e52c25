"""keras.preprocessing bits the reference imports."""
from . import image  # noqa: F401
