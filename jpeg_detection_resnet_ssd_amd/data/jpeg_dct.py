"""RGB batch -> JPEG -> de-quantised DCT coefficient tensors: the emission step at the end of the reference's
generators (localisation_part/data_generator/object_detection_2d_data_generator_dct_j2d.py:1167-1195;
classification_part/vgg_jpeg_keras/generators/generators.py:120-130,179-187,337-346), with the in-tree coefficient
reader in place of jpeg2dct and the whole batch decoded by host threads into float32 tensors ready for upload.

The same numbers are a pure integer function of the pixels, so the step also exists without a JPEG file in between:
`rgb_to_dct_host` states that function in numpy and `DeviceDCTEmitter` / `emit_dct_inputs_device` run it on the GPU
(csrc/dj_rgb2dct.hip), bit-exact with the PIL + reader path (tests/test_rgb_dct_cpu.py, tests/test_rgb_dct_gpu.py).
`PendingInputs` is the protocol by which a batch reaches a model's resident input buffers through that kernel; the batches
of data/image_prep.py and data/patch_resize.py, which first make their pixels on the GPU, derive from it too."""
import io

import numpy as np

from ..jpeg2dct import numpy as j2d


def rgb_to_jpeg_bytes(image, **save_kwargs):
    """`Image.fromarray(image).save(fake_file, format="jpeg")` (PIL defaults: quality 75, 4:2:0)."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.asarray(image, dtype=np.uint8)).save(buf, format="jpeg", **save_kwargs)
    return buf.getvalue()


def blocks_for(height, width):
    """Block grids of a 4:2:0 JPEG: Y ceil(h/8) x ceil(w/8), chroma ceil(ceil(h/2)/8) x ceil(ceil(w/2)/8)."""
    return ((-(-height // 8), -(-width // 8)), (-(-(-(-height // 2)) // 8), -(-(-(-width // 2)) // 8)))


def emit_dct_inputs(batch_X, deconv=False, n_threads=None, jpeg_bytes=None, **save_kwargs):
    """batch_X: (B, H, W, 3) uint8 (or a list of equally sized images).  Returns `[X_y, X_cbcr]`, or
    `[X_y, X_cb, X_cr]` when deconv=True -- float32, 300x300 -> (B,38,38,64) / (B,19,19,128 | 64).
    `jpeg_bytes` may pass already-encoded JPEGs instead of pixels."""
    if jpeg_bytes is None:
        jpeg_bytes = [rgb_to_jpeg_bytes(img, **save_kwargs) for img in batch_X]
    inf = j2d.info(jpeg_bytes[0])
    y_blocks, c_blocks = (inf.blocks_h[0], inf.blocks_w[0]), (inf.blocks_h[1], inf.blocks_w[1])
    y, cb, cr = j2d.decode_batch(jpeg_bytes, y_blocks, c_blocks, normalized=True, n_threads=n_threads)
    if deconv:
        return [y, cb, cr]
    return [y, np.concatenate([cb, cr], axis=-1)]


# ---- the same coefficients straight from the pixels ------------------------------------------------------------------------
def quant_tables(quality=75):
    """libjpeg's `jpeg_set_quality` tables (Annex K scaled, clipped to 1..255 as baseline files require) ->
    (luma, chroma), each (64,) int32 in natural order."""
    from . import synthetic_dct as sd
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError("quality must be in 1..100, got %r" % (quality,))
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base.reshape(64).astype(np.int64) * scale + 50) // 100, 1, 255).astype(np.int32)
                 for base in (sd._LUMA_BASE, sd._CHROMA_BASE))


def resolve_tables(quality, tables):
    if tables is None:
        return quant_tables(quality)
    luma, chroma = (np.asarray(t).reshape(-1) for t in tables)
    for name, t in (("luma", luma), ("chroma", chroma)):
        if t.size != 64 or (t != np.floor(t)).any() or t.min() < 1 or t.max() > 255:
            raise ValueError("%s quantisation table: expected 64 integer entries in 1..255 (natural order)" % name)
    return luma.astype(np.int32), chroma.astype(np.int32)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """libjpeg's integer "slow" forward DCT along the last axis: 13-bit constants; the row pass (`first`) leaves its
    outputs scaled up by 4, the column pass removes that and the constants' scale."""
    n = 11 if first else 15
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    o[7] = _descale(t4 + z1 + z3, n)
    o[5] = _descale(t5 + z2 + z4, n)
    o[3] = _descale(t6 + z2 + z3, n)
    o[1] = _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def _plane_blocks(plane, table, normalized):
    """(8*bh, 8*bw) samples 0..255 -> (bh, bw, 64) quantised levels (times the table when `normalized`)."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).astype(np.int32) - 128
    b = _fdct_pass(b, True)
    b = _fdct_pass(b.swapaxes(-1, -2), False).swapaxes(-1, -2)
    q = table.reshape(8, 8).astype(np.int32)
    q8 = q * 8
    level = np.sign(b) * ((np.abs(b) + (q8 >> 1)) // q8)      # half away from zero; the division truncates
    return (level * q if normalized else level).reshape(bh, bw, 64)


def _pad_edge(plane, height, width):
    return np.pad(plane, ((0, height - plane.shape[0]), (0, width - plane.shape[1])), mode="edge")


def rgb_to_dct_host(image, quality=75, tables=None, normalized=True):
    """(H, W, 3) uint8 RGB -> (dct_y, dct_cb, dct_cr) int16 exactly as `jpeg2dct.numpy.loads` returns them for the
    baseline 4:2:0 JPEG that PIL / libjpeg writes of `image` at `quality` (or with the two natural-order `tables`):
    the numpy twin of csrc/dj_rgb2dct.hip and the statement of its contract.  All arithmetic is int32."""
    image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError("expected an (H, W, 3) uint8 image, got %s %s" % (image.dtype, image.shape))
    luma, chroma = resolve_tables(quality, tables)
    h, w = image.shape[:2]
    r, g, b = (image[..., i].astype(np.int32) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16
    h16, w16 = -(-h // 16) * 16, -(-w // 16) * 16

    def subsample(p):
        # columns are replicated to the MCU edge BEFORE averaging, an odd last row pairs with itself, and rows below are
        # copies of the last AVERAGED row
        p = _pad_edge(p, h + (h & 1), w16)
        s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
        bias = 1 + (np.arange(s.shape[1], dtype=np.int32) & 1)
        return _pad_edge((s + bias[None, :]) >> 2, h16 // 2, w16 // 2)

    (ybh, ybw), (cbh, cbw) = blocks_for(h, w)
    planes = (_plane_blocks(_pad_edge(y, h16, w16), luma, normalized)[:ybh, :ybw],
              _plane_blocks(subsample(cb), chroma, normalized)[:cbh, :cbw],
              _plane_blocks(subsample(cr), chroma, normalized)[:cbh, :cbw])
    return tuple(np.ascontiguousarray(p).astype(np.int16) for p in planes)


def input_shapes(batch, height, width, deconv=False):
    """Shapes of the model inputs `emit_dct_inputs` produces for a (batch, height, width, 3) RGB batch."""
    (yh, yw), (ch, cw) = blocks_for(height, width)
    if deconv:
        return [(batch, yh, yw, 64), (batch, ch, cw, 64), (batch, ch, cw, 64)]
    return [(batch, yh, yw, 64), (batch, ch, cw, 128)]


def emit_resident(pixels, tables, deconv, buffers):
    """dj_rgb_to_dct of a resident (B, H, W, 3) uint8 CUDA batch into `buffers` ([Y, CbCr], or [Y, Cb, Cr] when `deconv`),
    on the current stream."""
    from .. import kernels
    outs = tuple(buffers) if deconv else (buffers[0], buffers[1][..., :64], buffers[1][..., 64:])
    kernels.rgb_to_dct(pixels, tables, outs, normalized=True)
    return buffers


class PendingInputs(object):
    """One batch on its way into a model's resident input buffers, transformed at upload time (`Model.train_on_batch /
    predict_on_batch / predict / fit_generator` accept it where they accept the list of input arrays).  `emitter` carries
    `tables` and `deconv`; `shape` is that of the pixel batch the model sees (`shape[0]` is the batch size, as for the
    first array of an input list).  A subclass provides `sliced(index)`, `host_pixels()` (the uint8 batch computed on the
    host) and `resident_pixels(device)` (the same batch as a uint8 CUDA tensor, made on the current stream)."""

    def __init__(self, emitter, shape):
        self.emitter, self.shape = emitter, tuple(shape)

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, index):
        if not isinstance(index, slice):
            raise TypeError("%s can only be sliced along the batch" % type(self).__name__)
        return self.sliced(index)

    @property
    def shapes(self):
        b, h, w, _ = self.shape
        return input_shapes(b, h, w, self.emitter.deconv)

    def emit_into(self, buffers):
        """Make the uint8 batch resident and launch the transform on the current stream, writing into `buffers`: float32
        CUDA tensors of `self.shapes` ([Y, CbCr] or [Y, Cb, Cr])."""
        buffers = list(buffers)
        if [tuple(t.shape) for t in buffers] != [tuple(s) for s in self.shapes]:
            raise ValueError("emit_into: expected buffers of shapes %s, got %s"
                             % (self.shapes, [tuple(t.shape) for t in buffers]))
        return emit_resident(self.resident_pixels(buffers[0].device), self.emitter.tables, self.emitter.deconv, buffers)

    def numpy(self):
        """The same inputs computed on the host (`host_pixels`, then `rgb_to_dct_host` per image), float32."""
        planes = [rgb_to_dct_host(img, tables=self.emitter.tables) for img in self.host_pixels()]
        y, cb, cr = (np.stack([p[i] for p in planes]).astype(np.float32) for i in range(3))
        return [y, cb, cr] if self.emitter.deconv else [y, np.concatenate([cb, cr], axis=-1)]


def check_batch(batch_X):
    x = np.ascontiguousarray(np.asarray(batch_X))
    if x.ndim != 4 or x.shape[3] != 3 or x.dtype != np.uint8:
        raise ValueError("expected a (B, H, W, 3) uint8 batch, got %s %s" % (x.dtype, x.shape))
    return x


class PendingDCTInputs(PendingInputs):
    """The pixels of one batch, to be transformed straight into a model's resident input buffers at upload time: one
    upload of the uint8 pixels, then dj_rgb_to_dct."""

    def __init__(self, emitter, batch_X):
        self.pixels = check_batch(batch_X)
        PendingInputs.__init__(self, emitter, self.pixels.shape)

    def sliced(self, index):
        return PendingDCTInputs(self.emitter, self.pixels[index])

    def host_pixels(self):
        return self.pixels

    def resident_pixels(self, device):
        import torch
        return torch.from_numpy(self.pixels).to(device, non_blocking=True)


class DeviceDCTEmitter(object):
    """Stands where the reference's generators save each augmented image as a JPEG and read it back with jpeg2dct
    (localisation_part/data_generator/object_detection_2d_data_generator_dct_j2d.py:1167-1195): the generator thread only
    carries the uint8 pixels, the transform runs on the GPU when the model uploads the batch (like DeviceLabelEncoder for
    the targets).  `quality` as in `Image.save(..., quality=)` (PIL's default 75), or two natural-order `tables`."""

    def __init__(self, quality=75, tables=None, deconv=False):
        self.tables = resolve_tables(quality, tables)
        self.quality = None if tables is not None else int(quality)
        self.deconv = bool(deconv)

    def __call__(self, batch_X):
        return PendingDCTInputs(self, batch_X)


def emit_dct_inputs_device(batch_X, deconv=False, quality=75, tables=None, device=None):
    """`emit_dct_inputs` on the GPU: (B, H, W, 3) uint8 (numpy, or a CUDA tensor already resident) -> `[X_y, X_cbcr]`
    or `[X_y, X_cb, X_cr]` as float32 CUDA tensors, for callers outside `Model`."""
    import torch
    tabs = resolve_tables(quality, tables)
    if isinstance(batch_X, torch.Tensor):
        dev = batch_X
    else:
        dev = torch.from_numpy(check_batch(batch_X)).to(device if device is not None else "cuda", non_blocking=True)
    b, h, w, _ = dev.shape
    bufs = [torch.empty(s, dtype=torch.float32, device=dev.device) for s in input_shapes(b, h, w, deconv)]
    return emit_resident(dev, tabs, deconv, bufs)
