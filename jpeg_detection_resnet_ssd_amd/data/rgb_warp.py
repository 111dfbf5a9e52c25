"""The per-image work of Keras' `ImageDataGenerator` on a loaded RGB image -- affine warp, flips, standardisation -- as a
statement that does not depend on scipy: `affine_warp_host` is the warp (`scipy.ndimage.affine_transform(channel,
M[:2, :2], M[:2, 2], order=1, mode='nearest', cval=0.)` per colour channel, bit for bit; tests/test_image_generator_cpu.py
holds the comparison), `rgb_warp_host` the whole call of csrc/dj_rgbwarp.hip and the oracle of its tests.  The draws and
the matrix composition live in keras/preprocessing/image.py; here an image's transform is a record with its draws made.

What decides bits of the warp, all float64, each product and sum rounded once (numpy's elementwise loops fuse nothing):

    r = (A00*i + A01*j) + o0 ;  c = (A10*i + A11*j) + o1
    r = clip(r, 0, H-1) ;  c = clip(c, 0, W-1)
    r0 = floor(r), tr = r - r0, r1 = min(r0+1, H-1)            (same for c)
    out = (((x[r0,c0]*(1-tr))*(1-tc) + (x[r0,c1]*(1-tr))*tc) + (x[r1,c0]*tr)*(1-tc)) + (x[r1,c1]*tr)*tc
    result = float32(out)

`PendingRGBInputs` is one batch on its way into a model's resident input buffer through that kernel: the protocol of
data/jpeg_dct.py:PendingInputs (`shape`, `shapes`, `sliced`, `emit_into`).  `PendingRGBFileInputs` is the same batch one
step earlier: files not yet decoded nor resized, which dj_jpeg_pixels and dj_patch_resize turn into that kernel's input."""
import numpy as np

PREP_NONE, PREP_CAFFE = 0, 1                          # DJ_RGB_PREP_* of include/dj_hip.h
CAFFE_MEAN = (103.939, 116.779, 123.68)               # BGR; subtracted in float32

# dj_rgb_warp_record (include/dj_hip.h), C layout
RECORD_DTYPE = np.dtype([("m", np.float64, (6,)), ("identity", np.int32), ("flip_cols", np.int32),
                         ("flip_rows", np.int32), ("reserved", np.int32)], align=True)


def affine_warp_host(x, M):
    """The (H, W, C) uint8 or float32 image `x` warped by the 3 x 3 (or 2 x 3) matrix `M` that maps output (row, column, 1)
    to input coordinates: bilinear, nearest fill -> float32 (H, W, C)."""
    x = np.asarray(x)
    if x.ndim != 3 or x.dtype not in (np.uint8, np.float32):
        raise ValueError("expected an (H, W, C) uint8 or float32 image, got %s %s" % (x.dtype, x.shape))
    M = np.asarray(M, dtype=np.float64)
    h, w = x.shape[:2]
    i = np.arange(h, dtype=np.float64)[:, None]
    j = np.arange(w, dtype=np.float64)[None, :]
    r = (M[0, 0] * i + M[0, 1] * j) + M[0, 2]
    c = (M[1, 0] * i + M[1, 1] * j) + M[1, 2]
    r = np.clip(r, 0.0, float(h - 1))
    c = np.clip(c, 0.0, float(w - 1))
    fr, fc = np.floor(r), np.floor(c)
    tr, tc = (r - fr)[:, :, None], (c - fc)[:, :, None]
    ur, uc = 1.0 - tr, 1.0 - tc
    r0, c0 = fr.astype(np.int64), fc.astype(np.int64)
    r1, c1 = np.minimum(r0 + 1, h - 1), np.minimum(c0 + 1, w - 1)
    xd = x.astype(np.float64)
    out = (((xd[r0, c0] * ur) * uc + (xd[r0, c1] * ur) * tc) + (xd[r1, c0] * tr) * uc) + (xd[r1, c1] * tr) * tc
    return out.astype(np.float32)


def caffe_preprocess(x):
    """`preprocess_input(x, mode='caffe')` of a float32 (..., 3) array: channels reversed, the float32 mean subtracted."""
    x = np.asarray(x, dtype=np.float32)[..., ::-1]
    return x - np.asarray(CAFFE_MEAN, dtype=np.float32)


def make_record(matrix=None, flip_cols=False, flip_rows=False):
    """One image's transform -> a RECORD_DTYPE scalar array: `matrix` the recentred 3 x 3 (None: no warp)."""
    rec = np.zeros((), dtype=RECORD_DTYPE)
    if matrix is None:
        rec["identity"] = 1
        rec["m"] = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    else:
        m = np.asarray(matrix, dtype=np.float64)
        if m.shape not in ((3, 3), (2, 3)) or not np.isfinite(m[:2]).all():
            raise ValueError("expected a finite 3 x 3 matrix, got %r" % (matrix,))
        rec["m"] = m[:2].reshape(6)
    rec["flip_cols"], rec["flip_rows"] = int(bool(flip_cols)), int(bool(flip_rows))
    return rec


def pack_records(records):
    """A list of `make_record` results -> the contiguous RECORD_DTYPE array dj_rgb_warp reads."""
    arr = np.zeros(len(records), dtype=RECORD_DTYPE)
    for k, rec in enumerate(records):
        arr[k] = rec
    return arr


def check_pixels(pixels):
    x = np.ascontiguousarray(np.asarray(pixels))
    if x.ndim != 4 or x.shape[3] != 3 or x.dtype != np.uint8 or 0 in x.shape:
        raise ValueError("expected a non-empty (B, H, W, 3) uint8 batch, got %s %s" % (x.dtype, x.shape))
    return x


def check_call(pixels, records, preprocess, rescale):
    pixels = check_pixels(pixels)
    records = np.asarray(records)
    if records.dtype != RECORD_DTYPE or records.shape != (pixels.shape[0],):
        raise ValueError("expected one RECORD_DTYPE record per image")
    if preprocess not in (PREP_NONE, PREP_CAFFE):
        raise ValueError("unknown preprocessing code %r" % (preprocess,))
    return pixels, np.ascontiguousarray(records), int(preprocess), None if rescale is None else np.float32(rescale)


def rgb_warp_host(pixels, records, preprocess=PREP_NONE, rescale=None):
    """What dj_rgb_warp writes for the (B, H, W, 3) uint8 batch `pixels`: per image the warp (unless the record says
    identity), the column flip, the row flip, the preprocessing and the float32 rescale -> (B, H, W, 3) float32."""
    pixels, records, preprocess, rescale = check_call(pixels, records, preprocess, rescale)
    out = np.empty(pixels.shape, dtype=np.float32)
    for k, (img, rec) in enumerate(zip(pixels, records)):
        x = img.astype(np.float32) if rec["identity"] else affine_warp_host(img, rec["m"].reshape(2, 3))
        if rec["flip_cols"]:
            x = x[:, ::-1]
        if rec["flip_rows"]:
            x = x[::-1]
        if preprocess == PREP_CAFFE:
            x = caffe_preprocess(x)
        if rescale is not None:
            x = x * rescale
        out[k] = x
    return out


def rgb_warp_device(pixels, records, preprocess=PREP_NONE, rescale=None, out=None, device=None, stream=None):
    """`rgb_warp_host` on the GPU for callers outside `Model`: uploads pixels and records, launches dj_rgb_warp into `out`
    (a float32 CUDA tensor of the batch's shape whose rows may be strided; None: a fresh one) and waits for it."""
    import torch

    from .. import kernels
    pixels, records, preprocess, rescale = check_call(pixels, records, preprocess, rescale)
    device = torch.device(device if device is not None else (out.device if out is not None else "cuda"))
    pix_dev = torch.from_numpy(pixels).to(device)
    rec_dev = torch.from_numpy(records.view(np.uint8).reshape(-1)).to(device)
    if out is None:
        out = torch.empty(pixels.shape, dtype=torch.float32, device=device)
    kernels.rgb_warp(pix_dev, rec_dev, records, out, preprocess, None if rescale is None else float(rescale), stream=stream)
    (torch.cuda.current_stream(device) if stream is None else torch.cuda.ExternalStream(stream)).synchronize()
    return out


# ---- one batch on its way into a model's input buffer -------------------------------------------------------------------------
ALIGN = 64


class RGBWarpStager(object):
    """The buffers a device iterator keeps, per device and grown on demand: two pinned staging blobs used in turn (records,
    then pixels from a multiple of 64 bytes), each refilled only after the upload that last read it has finished, and the
    blob's device copy.  The manner of data/device_staging.py:ResidentBuffers, without descriptors of its own."""

    def __init__(self):
        self._state = {}

    def upload(self, pixels, records, device):
        """-> (pixels, record bytes) as CUDA tensors, valid until the next call on this device; the copy is queued on the
        current stream."""
        import torch

        from .device_staging import ResidentBuffers
        device = torch.device(device)
        st = self._state.setdefault(str(device), {"slots": [[None, None], [None, None]], "turn": 0, "blob": None})
        slot = st["slots"][st["turn"]]
        st["turn"] ^= 1
        if slot[1] is not None:
            slot[1].synchronize()
        pix_off = -(-records.nbytes // ALIGN) * ALIGN
        nbytes = pix_off + pixels.size
        slot[0] = ResidentBuffers._grown(slot[0], nbytes)
        st["blob"] = ResidentBuffers._grown(st["blob"], nbytes, device)
        host = slot[0].numpy()
        host[:records.nbytes] = records.view(np.uint8).reshape(-1)
        host[pix_off:nbytes] = pixels.reshape(-1)
        st["blob"][:nbytes].copy_(slot[0][:nbytes], non_blocking=True)
        if slot[1] is None:
            slot[1] = torch.cuda.Event()
        slot[1].record()
        return st["blob"][pix_off:nbytes].view(pixels.shape), st["blob"][:records.nbytes]


class PendingRGBInputs(object):
    """The decoded, resized pixels of one batch with each image's drawn transform, to be warped straight into a model's
    resident input buffer at upload time: one upload of pixels and records, then dj_rgb_warp.  `Model.train_on_batch /
    predict_on_batch / predict / fit_generator` accept it where they accept the list of input arrays."""

    def __init__(self, pixels, records, preprocess=PREP_NONE, rescale=None, stager=None):
        self.pixels, self.records, self.preprocess, self.rescale = check_call(pixels, records, preprocess, rescale)
        self.stager = stager if stager is not None else RGBWarpStager()
        self.shape = tuple(self.pixels.shape)

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, index):
        if not isinstance(index, slice):
            raise TypeError("PendingRGBInputs can only be sliced along the batch")
        return self.sliced(index)

    def sliced(self, index):
        return PendingRGBInputs(self.pixels[index], self.records[index], self.preprocess, self.rescale, self.stager)

    @property
    def shapes(self):
        return [self.shape]

    def emit_into(self, buffers):
        """Upload pixels and records in one copy and launch the warp on the current stream, writing into `buffers[0]`: the
        float32 CUDA tensor of `self.shape`."""
        buffers = list(buffers)
        if [tuple(t.shape) for t in buffers] != self.shapes:
            raise ValueError("emit_into: expected buffers of shapes %s, got %s"
                             % (self.shapes, [tuple(t.shape) for t in buffers]))
        from .. import kernels
        pix_dev, rec_dev = self.stager.upload(self.pixels, self.records, buffers[0].device)
        kernels.rgb_warp(pix_dev, rec_dev, self.records, buffers[0], self.preprocess,
                         None if self.rescale is None else float(self.rescale))
        return buffers

    def numpy(self):
        """The same input computed on the host (`rgb_warp_host`), as the list of arrays the model takes."""
        return [rgb_warp_host(self.pixels, self.records, self.preprocess, self.rescale)]


# ---- the same from files that are neither decoded nor resized on the host ----------------------------------------------------
def load_geometry(height, width, resample):
    """The `patch_resize` geometry of `load_img`'s resize: the whole image, no mirror, the iterator's filter.  Where a
    side already has the target's length the plan takes the identity taps, so a file of the target size comes through
    unchanged, as `load_img` leaves it."""
    return (0, 0, int(height), int(width), False, resample, (0, 0, 0))


class PendingRGBFileInputs(object):
    """One batch of the RGB iterator whose files were neither decoded nor resized on the host: `images` holds a
    `CoefficientImage` per file the GPU can reconstruct and the full-size (H_i, W_i, 3) uint8 array of every other,
    `records` each image's drawn transform, `target_size` = (height, width) and `resample` the Pillow code of the
    iterator's `interpolation`.  At upload time one pinned blob `[resize descriptors | taps | pixels of the decoded files |
    warp records | decode descriptors | tables | coefficient planes]` goes up in one copy; dj_jpeg_pixels makes the
    remaining pixels, dj_patch_resize (a whole-image window without mirror) the dense (B, H, W, 3) uint8 batch, and
    dj_rgb_warp writes the model's input.  The protocol of `PendingRGBInputs`; `stager`: the `StagingBuffers` an iterator
    keeps across batches."""

    def __init__(self, images, records, target_size, resample, preprocess=PREP_NONE, rescale=None, stager=None):
        from . import device_staging as ds
        from .patch_resize import PatchPlan
        self.images = ds.check_images(images)
        height, width = (int(v) for v in target_size)
        self.shape = (len(self.images), height, width, 3)
        self.resample = ds.resolve_filter(resample)
        records = np.ascontiguousarray(np.asarray(records))
        if records.dtype != RECORD_DTYPE or records.shape != (len(self.images),):
            raise ValueError("expected one RECORD_DTYPE record per image")
        if preprocess not in (PREP_NONE, PREP_CAFFE):
            raise ValueError("unknown preprocessing code %r" % (preprocess,))
        self.records, self.preprocess = records, int(preprocess)
        self.rescale = None if rescale is None else np.float32(rescale)
        self.stager = stager if stager is not None else ds.StagingBuffers()
        # descriptors and taps are made where the batch is made (the iterator's thread), not at upload time
        self.plan = PatchPlan(ds.plan_items(self.images),
                              [load_geometry(im.shape[0], im.shape[1], self.resample) for im in self.images],
                              height, width, extra=[("records", self.records)])

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, index):
        if not isinstance(index, slice):
            raise TypeError("PendingRGBFileInputs can only be sliced along the batch")
        return self.sliced(index)

    def sliced(self, index):
        return PendingRGBFileInputs(self.images[index], self.records[index], self.shape[1:3], self.resample,
                                    self.preprocess, self.rescale, self.stager)

    @property
    def shapes(self):
        return [self.shape]

    def emit_into(self, buffers):
        """Stage and upload the blob and launch dj_jpeg_pixels, dj_patch_resize and dj_rgb_warp on the current stream,
        writing into `buffers[0]`: the float32 CUDA tensor of `self.shape`."""
        buffers = list(buffers)
        if [tuple(t.shape) for t in buffers] != self.shapes:
            raise ValueError("emit_into: expected buffers of shapes %s, got %s"
                             % (self.shapes, [tuple(t.shape) for t in buffers]))
        from .. import kernels
        device = buffers[0].device
        pixels = self.stager.run(self.plan, self.images, device)
        rec_dev = self.plan.part(self.stager.blob(device), self.plan.records_offset, self.records)
        kernels.rgb_warp(pixels, rec_dev, self.records, buffers[0], self.preprocess,
                         None if self.rescale is None else float(self.rescale))
        return buffers

    def pixels(self):
        """The dense (B, H, W, 3) uint8 batch computed on the host: `CoefficientImage.pixels()` where a file travels as
        coefficients, then `resize_host`."""
        from . import device_staging as ds
        size = (self.shape[2], self.shape[1])
        return np.stack([ds.resize_host(im, size, self.resample) for im in ds.decoded(self.images)])

    def numpy(self):
        """The same input computed on the host (`pixels`, then `rgb_warp_host`), as the list of arrays the model takes."""
        return [rgb_warp_host(self.pixels(), self.records, self.preprocess, self.rescale)]
