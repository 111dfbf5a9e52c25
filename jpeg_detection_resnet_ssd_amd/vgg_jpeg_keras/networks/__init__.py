from .vgg_dct import vgg_dct, vgga_dct, vggd_dct  # noqa: F401
