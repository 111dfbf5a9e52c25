"""RGB pixels of a baseline / extended-sequential JPEG from its entropy-decoded coefficients: the half of a decoder that
is small-integer arithmetic without data-dependent control flow, stated here in numpy (`jpeg_pixels_host`) and run on the
GPU by csrc/dj_jpegpix.hip (`kernels.jpeg_pixels`).  The other half, entropy decoding, is the in-tree reader's
(csrc/dj_jpeg.cpp).  The statement equals Pillow's `Image.open(f).convert("RGB")` byte for byte, i.e. libjpeg's default
decompression (jidctint.c, jdsample.c, jdcolor.c):

  * de-quantisation: coefficient * table entry in int32;
  * the integer "slow" inverse DCT with CONST_BITS = 13 and PASS1_BITS = 2: a column pass descaled by 11 bits, a row pass
    descaled by 18, then + 128 and a clamp to 0..255;
  * chroma upsampling by the triangle ("fancy") filter.  h2v1: output column 2k is (3 c[k] + c[k - 1] + 1) >> 2 and column
    2k + 1 is (3 c[k] + c[k + 1] + 2) >> 2.  h2v2: with s[k] = 3 c[r][k] + c[r'][k], where r' is the row above r for an even
    output row and the row below for an odd one, column 2k is (3 s[k] + s[k - 1] + 8) >> 4 and column 2k + 1 is
    (3 s[k] + s[k + 1] + 7) >> 4.  A neighbour past the component's real down-sampled extent (ceil(width / 2) columns,
    ceil(height / 2) rows -- not the block grid's) is the edge sample itself, which is libjpeg's first / last-column case
    and its replicated context rows.  A component whose down-sampled width is 2 or less is upsampled by plain replication
    in both directions instead: libjpeg selects the triangle filter only for wider ones;
  * YCbCr -> RGB in 16-bit fixed point: R = Y + ((91881 (Cr - 128) + 32768) >> 16), B = Y + ((116130 (Cb - 128) + 32768)
    >> 16), G = Y + ((-22554 (Cb - 128) - 46802 (Cr - 128) + 32768) >> 16) -- one rounding constant for the whole green
    term -- each clamped to 0..255;
  * a one-component file is gray, replicated to three channels; 4:4:4 needs no upsampling.

libjpeg looks inverse-DCT results up in a range table that WRAPS (`& 1023`) for samples far outside anything a forward DCT
of 8-bit pixels produces; the statement (and the kernel) clamp instead, so the two differ only on such files.

`CoefficientImage` is what a generator hands the planners and the staging layer in place of a decoded array: the file's
bytes, its header's geometry, and `.pixels()` = the statement."""
import numpy as np

from ..jpeg2dct import numpy as reader

CONST_BITS, PASS1_BITS = 13, 2
# FIX(x) = round(x * 2^13) of jidctint.c
F_0_298631336, F_0_390180644, F_0_541196100, F_0_765366865 = 2446, 3196, 4433, 6270
F_0_899976223, F_1_175875602, F_1_501321110, F_1_847759065 = 7373, 9633, 12299, 15137
F_1_961570560, F_2_053119869, F_2_562915447, F_3_072711026 = 16069, 16819, 20995, 25172
# FIX(x) = round(x * 2^16) of jdcolor.c
CR_R, CB_B, CR_G, CB_G = 91881, 116130, 46802, 22554


def decodable(buf):
    """Whether `jpeg_pixels_host` / dj_jpeg_pixels reconstruct this file: the reader's verdict (include/dj_jpeg_decode.h), False
    for what it cannot parse."""
    try:
        return bool(reader.decode_info(buf).device_decodable)
    except ValueError:
        return False


def _idct_1d(d, shift):
    """jidctint.c's 1-D pass over the last axis of (..., 8) int32, descaled by `shift` bits."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., k] for k in range(8))
    z1 = (d2 + d6) * F_0_541196100
    tmp2 = z1 - d6 * F_1_847759065
    tmp3 = z1 + d2 * F_0_765366865
    tmp0 = (d0 + d4) << CONST_BITS
    tmp1 = (d0 - d4) << CONST_BITS
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = d7, d5, d3, d1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175875602
    t0, t1, t2, t3 = t0 * F_0_298631336, t1 * F_2_053119869, t2 * F_3_072711026, t3 * F_1_501321110
    z1, z2 = z1 * -F_0_899976223, z2 * -F_2_562915447
    z3, z4 = z3 * -F_1_961570560 + z5, z4 * -F_0_390180644 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3], axis=-1)
    return (out + (1 << (shift - 1))) >> shift


def idct_blocks(coef, table):
    """(bh, bw, 64) raw int16 coefficients and the component's (64,) table, natural order -> (8 bh, 8 bw) uint8 samples."""
    bh, bw = coef.shape[:2]
    d = (coef.astype(np.int32) * np.asarray(table, dtype=np.int32)).reshape(bh, bw, 8, 8)
    ws = _idct_1d(d.transpose(0, 1, 3, 2), CONST_BITS - PASS1_BITS).transpose(0, 1, 3, 2)      # columns
    px = _idct_1d(ws, CONST_BITS + PASS1_BITS + 3)                                             # rows
    px = np.clip(px + 128, 0, 255).astype(np.uint8)
    return px.transpose(0, 2, 1, 3).reshape(8 * bh, 8 * bw)


def upsample(c, h, v, height, width):
    """A chroma plane of real extent c.shape, sampled h x v times coarser than luma (h in 1, 2; v in 1, 2; v == 2 only
    with h == 2) -> (height, width) int32, as libjpeg's default upsamplers do it (the module's docstring)."""
    c = c.astype(np.int32)
    ch, cw = c.shape
    y, x = np.arange(height), np.arange(width)
    if h == 1 and v == 1:
        return c[:height, :width]
    if cw <= 2:                                   # libjpeg: no triangle filter for so narrow a component
        return c[(y // v)[:, None], (x // h)[None, :]]
    k = x >> 1
    kn = np.where(x & 1, np.minimum(k + 1, cw - 1), np.maximum(k - 1, 0))
    if v == 1:
        rows = c[:height]
        return (3 * rows[:, k] + rows[:, kn] + np.where(x & 1, 2, 1)[None, :]) >> 2
    r = y >> 1
    rn = np.where(y & 1, np.minimum(r + 1, ch - 1), np.maximum(r - 1, 0))
    s = 3 * c[r] + c[rn]
    return (3 * s[:, k] + s[:, kn] + np.where(x & 1, 7, 8)[None, :]) >> 4


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((CR_R * cr + 32768) >> 16)
    g = y + ((-CB_G * cb - CR_G * cr + 32768) >> 16)
    b = y + ((CB_B * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def _require(info):
    if not info.device_decodable:
        raise ValueError("this JPEG is not reconstructed here (SOF%d, %d components, precision %d): decode it with Pillow"
                         % (info.base.sof, info.base.n_components, info.precision))


def check_rect(rect, height, width):
    """None (the whole image) or (ya, yb, xa, xb) -> plain ints with 0 <= ya <= yb <= height and the same across."""
    if rect is None:
        return 0, height, 0, width
    ya, yb, xa, xb = (int(v) for v in rect)
    if not (0 <= ya <= yb <= height and 0 <= xa <= xb <= width):
        raise ValueError("rect %r leaves the image of %d x %d" % (rect, height, width))
    return ya, yb, xa, xb


def jpeg_pixels_host(buf, rect=None):
    """`np.array(Image.open(io.BytesIO(buf)).convert("RGB"))` for a file that is `decodable`, from the reader's raw
    coefficients and tables -> (height, width, 3) uint8; `rect` = (ya, yb, xa, xb): rows ya..yb-1 and columns xa..xb-1
    of it.  ValueError for any other file.  libjpeg's range table wraps (`& 1023`) for inverse-DCT results far outside
    what a forward DCT of 8-bit pixels produces; this statement clamps them."""
    buf = bytes(buf)
    info = reader.decode_info(buf)
    _require(info)
    b = info.base
    height, width, n = b.height, b.width, b.n_components
    ya, yb, xa, xb = check_rect(rect, height, width)
    planes = reader.loads(buf, normalized=False, channels=3 if n == 3 else 1)
    tables = np.array(b.quant, dtype=np.int32)
    luma = idct_blocks(planes[0], tables[0])[:height, :width]
    if n == 1:
        rgb = np.repeat(luma[:, :, None], 3, axis=2)
    else:
        h, v = b.h_samp[0], b.v_samp[0]
        ch, cw = -(-height // v), -(-width // h)
        chroma = [upsample(idct_blocks(planes[c], tables[c])[:ch, :cw], h, v, height, width) for c in (1, 2)]
        rgb = ycc_to_rgb(luma, chroma[0], chroma[1])
    return np.ascontiguousarray(rgb[ya:yb, xa:xb])


class CoefficientImage(object):
    """A decodable JPEG file standing where a decoded (height, width, 3) uint8 array would: `data` its bytes, `info` the
    reader's `JpegDecodeInfo`, `shape` = (height, width, 3) from the header so that the planners work unchanged, and
    `pixels()` the host statement.  ValueError for a file that is not `decodable`."""
    dtype = np.dtype(np.uint8)
    ndim = 3

    def __init__(self, data):
        self.data = bytes(data)
        self.info = reader.decode_info(self.data)
        _require(self.info)
        self.shape = (int(self.info.base.height), int(self.info.base.width), 3)

    def pixels(self, rect=None):
        return jpeg_pixels_host(self.data, rect)

    def __deepcopy__(self, memo):
        return self                    # immutable

    @property
    def n_components(self):
        return int(self.info.base.n_components)

    @property
    def sampling(self):
        """(h, v) of luma over chroma: (1, 1) for gray and 4:4:4."""
        b = self.info.base
        return (int(b.h_samp[0]), int(b.v_samp[0])) if b.n_components == 3 else (1, 1)

    def grids(self):
        """[(blocks_h, blocks_w)] per component."""
        b = self.info.base
        return [(int(b.blocks_h[c]), int(b.blocks_w[c])) for c in range(b.n_components)]

    def tables(self):
        """(3, 64) int32: the table of each component, natural order (gray: its one table three times)."""
        q = np.array(self.info.base.quant, dtype=np.int32)
        return q[:3].copy() if self.n_components == 3 else np.repeat(q[:1], 3, axis=0)


def read_image(path):
    """What a `device_decode` classifier generator hands over for the file at `path`: a `CoefficientImage` when the file
    is `decodable`, else the (height, width, 3) uint8 array of Pillow's `convert("RGB")` (progressive or CMYK JPEG, PNG,
    ...), decoded from the bytes already read."""
    import io
    with open(path, "rb") as f:
        data = f.read()
    if decodable(data):
        return CoefficientImage(data)
    from PIL import Image
    with Image.open(io.BytesIO(data)) as image:
        return np.array(image.convert("RGB"), dtype=np.uint8)
