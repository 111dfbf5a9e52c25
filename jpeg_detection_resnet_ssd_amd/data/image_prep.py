"""Decoded image -> the network-sized RGB pixels the JPEG emission step starts from: steps 2 to 4 of the reference's
classifier generators (classification_part/vgg_jpeg_keras/generators/generators.py:141-167 and :299-325), which run
between `Image.open(...).convert("RGB")` and `im.save(fake_file, format="jpeg")`:

  2. `im.resize((int(round(width * r)), int(round(height * r))))` with r = target_length / min(im.size) (scale=True), or
     `im.resize((target_length, target_length))` (scale=False);
  3. `im.crop(...)` of target_length along the longer side at `offset` (along x when the resized width is larger than the
     resized height, along y otherwise -- with equal sides the only offset is 0 and the two agree);
  4. `im.transpose(FLIP_LEFT_RIGHT)` when the flip was drawn.

All three are an integer function of the pixels.  data/device_staging.py restates Pillow's `Image.resize` (the taps of its
two-pass resampler and the passes themselves); `resample_coeffs` and `resize_host` here are that statement for the three
filters the classifier generators may ask for, and `prep_host` is steps 2 to 4 for one image; tests/test_image_prep_cpu.py
pins them to the installed Pillow and to tests/golden/image_prep.npz.  csrc/dj_imgprep.hip runs the same arithmetic on the
GPU (`DeviceImagePrep`, `prep_device`): the host computes the taps, the device does everything that touches pixels.  The
staging blob, the resident buffers and the upload are device_staging's; what is here is the geometry of one image, the copy
of its pixels and the order of the kernels."""
import numpy as np

from . import device_staging as ds
from .device_staging import (BICUBIC, BILINEAR, BOX, HAMMING, LANCZOS, NEAREST, PRECISION_BITS, check_image, check_images,  # noqa: F401
                             identity_coeffs, round_up)
from .jpeg_dct import PendingInputs
from .jpeg_pixels import CoefficientImage

SUPPORTED = (BILINEAR, BICUBIC, BOX)      # NEAREST and LANCZOS stay refused here: the classifier generators never draw them


def resolve_resample(resample):
    """None (Pillow's default for `Image.resize`: BICUBIC), a Pillow resampling code or its name -> the code; ValueError
    for a filter this module does not restate."""
    return ds.resolve_filter(resample, SUPPORTED)


def resample_coeffs(in_size, out_size, resample=None):
    """What Pillow's resampler computes for one axis -> (bounds, coeffs): bounds (out_size, 2) int32 = first source
    index and tap count of each output sample, coeffs (out_size, ksize) int32 = its taps at 22 fractional bits (zero past
    the count).  The arrays are cached and read-only."""
    in_size, out_size = ds.check_sizes(in_size, out_size)
    return ds.windowed_coeffs(in_size, out_size, resolve_resample(resample))


def axis_coeffs(in_size, out_size, resample=None):
    """`resample_coeffs`, or the identity taps when the pass is skipped."""
    return ds.filter_coeffs(in_size, out_size, resample, SUPPORTED)


def resize_host(image, size, resample=None):
    """`Image.fromarray(image).resize(size, resample)` for an (H, W, 3) uint8 image and size = (width, height)."""
    return ds.resize_host(image, size, resample, SUPPORTED)


def prep_geometry(height, width, target_length, scale, offset):
    """(height, width) of the decoded image -> (resized width, resized height, crop x, crop y) as the reference's
    generators compute them; ValueError for an offset outside 0 .. max(resized size) - target_length."""
    t, offset = int(target_length), int(offset)
    if t < 1 or height < 1 or width < 1:
        raise ValueError("sizes must be >= 1")
    if not scale:
        if offset != 0:
            raise ValueError("scale=False takes no crop: offset must be 0, got %d" % offset)
        return t, t, 0, 0
    ratio = t / min(width, height)
    rw, rh = int(round(width * ratio)), int(round(height * ratio))
    if not 0 <= offset <= max(rw, rh) - t:
        raise ValueError("offset %d outside 0..%d" % (offset, max(rw, rh) - t))
    crop_x, crop_y = (offset, 0) if rw > rh else (0, offset)
    if crop_x + t > rw or crop_y + t > rh:
        raise ValueError("the %dx%d window at (%d, %d) leaves the resized %dx%d image" % (t, t, crop_x, crop_y, rw, rh))
    return rw, rh, crop_x, crop_y


def max_offset(height, width, target_length, scale=True):
    """Upper end of the reference's `random.randint(0, max(im.size) - target_length)` for a decoded (height, width)."""
    if not scale:
        return 0
    ratio = int(target_length) / min(width, height)
    return max(int(round(width * ratio)), int(round(height * ratio))) - int(target_length)


def prep_host(image, target_length=224, scale=True, offset=0, flip=False, resample=None):
    """Steps 2 to 4 for one (H, W, 3) uint8 image -> (target_length, target_length, 3) uint8: what
    `im.resize(...).crop(...)[.transpose(FLIP_LEFT_RIGHT)]` leaves in the reference's generators."""
    image = check_image(image)
    t = int(target_length)
    rw, rh, cx, cy = prep_geometry(image.shape[0], image.shape[1], t, scale, offset)
    out = resize_host(image, (rw, rh), resample)[cy:cy + t, cx:cx + t]
    if flip:
        out = out[:, ::-1]
    return np.ascontiguousarray(out)


# ---- the same on the GPU: csrc/dj_imgprep.hip ------------------------------------------------------------------------------
# dj_image_prep_desc (include/dj_hip.h), C layout
DESC_DTYPE = np.dtype([(n, np.int64) for n in ("src_offset", "src_stride", "scratch_offset")]
                      + [(n, np.int32) for n in ("src_h", "src_w", "res_h", "res_w", "crop_y", "crop_x", "flip", "h_bounds",
                                                 "h_taps", "h_ksize", "v_bounds", "v_taps", "v_ksize", "row0", "n_rows")],
                      align=True)


class BatchPlan(ds.StagedPlan):
    """Everything `dj_image_prep` needs for one ragged batch except the pixels' bytes: per-image descriptors, the shared
    int32 pool of bounds and taps (one copy per distinct (source size, resized size) pair of the batch) and the layout of
    one staging buffer `[descriptors | pool | photometric lists | pixels]`, each part at a multiple of 64 bytes.  `ops`
    (optional): per image, the photometric operations [(code, parameters), ...] of data/photometric.py that
    dj_photometric runs on the prepared pixels; without it the third part is empty.  An item of `shapes` may be a
    `CoefficientImage` instead of (height, width): its whole image is then reconstructed on the GPU from the file's
    coefficients into the place its pixels would have been copied to (`StagedPlan`), and the decode parts lie behind the
    four above."""
    DESC_DTYPE = DESC_DTYPE

    def __init__(self, shapes, params, target_length=224, resample=None, ops=None):
        code = resolve_resample(resample)
        t = int(target_length)
        items = list(shapes)
        shapes = ds.item_shapes(items)
        params = [(bool(s), int(o), bool(f)) for s, o, f in params]
        if len(shapes) != len(params) or not shapes:
            raise ValueError("expected one (scale, offset, flip) per image and at least one image")
        self.batch, self.target, self.resample = len(shapes), t, code
        self.out_shape = (self.batch, t, t, 3)
        self.desc = np.zeros(self.batch, dtype=DESC_DTYPE)
        taps = ds.TapsPool(SUPPORTED)
        src_off = scratch_off = 0
        for i, ((h, w), (scale, offset, flip)) in enumerate(zip(shapes, params)):
            rw, rh, cx, cy = prep_geometry(h, w, t, scale, offset)
            hb, hk, hn, _ = taps.get((w, rw), w, rw, code)
            vb, vk, vn, vbounds = taps.get((h, rh), h, rh, code)
            row0 = int(vbounds[cy, 0])
            n_rows = int(vbounds[cy + t - 1, 0] + vbounds[cy + t - 1, 1]) - row0
            d = self.desc[i]
            d["src_offset"], d["src_stride"], d["scratch_offset"] = src_off, 3 * w, scratch_off
            d["src_h"], d["src_w"], d["res_h"], d["res_w"] = h, w, rh, rw
            d["crop_y"], d["crop_x"], d["flip"] = cy, cx, int(flip)
            d["h_bounds"], d["h_taps"], d["h_ksize"] = hb, hk, hn
            d["v_bounds"], d["v_taps"], d["v_ksize"] = vb, vk, vn
            d["row0"], d["n_rows"] = row0, n_rows
            src_off += round_up(3 * w * h)
            scratch_off += round_up(3 * t * n_rows)
        self.pool = taps.array()
        self.shapes = shapes
        self.src_bytes, self.scratch_bytes = src_off, scratch_off
        self.ops = None
        if ops is not None:
            from .photometric import pack_ops
            self.ops = pack_ops(ops, self.batch)
        # dj_image_prep reads any row of the source (its vertical taps reach where the resize puts them): the whole image is staged
        decode = self._plan_decode(items, [(0, h, 0, w) for h, w in shapes],
                                   [(int(d["src_offset"]), int(d["src_stride"])) for d in self.desc])
        self._lay_out([("desc", self.desc), ("pool", self.pool), ("ops", self.ops), ("src", self.src_bytes)] + decode)

    def _fill_pixels(self, src, images):
        for d, (h, w), img in zip(self.desc, self.shapes, images):
            if not isinstance(img, CoefficientImage):
                o = int(d["src_offset"])
                src[o:o + 3 * w * h].reshape(h, w, 3)[...] = img

    def launch_photometric(self, blob_dev, pixels, stream=None):
        """dj_photometric on the prepared batch, in place, its lists read from the device copy of the staging buffer."""
        from .. import kernels
        return kernels.photometric(pixels, self.part(blob_dev, self.ops_offset, self.ops), self.ops, stream=stream)

    def launch(self, blob_host, blob_dev, out, scratch, stream=None):
        """dj_jpeg_pixels for the items that travel as coefficients, dj_image_prep into `out`, then dj_photometric on it
        when the plan carries operation lists."""
        from .. import kernels
        self.launch_decode(blob_host, blob_dev, scratch, stream)
        src_h, desc_h, pool_h = self.views(blob_host)
        src_d, desc_d, pool_d = self.views(blob_dev)
        kernels.image_prep(src_d, desc_d, desc_h, pool_d, pool_h, self.target, out, scratch, stream=stream)
        if self.ops is not None:
            self.launch_photometric(blob_dev, out, stream=stream)
        return out


def prep_device(images, params, target_length=224, resample=None, device=None, out=None, stream=None, ops=None,
                n_threads=None):
    """`prep_host` for a list of (H_i, W_i, 3) uint8 images and per-image (scale, offset, flip) on the GPU -> the
    (B, target_length, target_length, 3) uint8 CUDA batch, for callers outside `Model` (fresh buffers every call;
    `DeviceImagePrep` keeps its own).  `ops`: per-image photometric operation lists, run on the prepared pixels.  An
    image may be a `CoefficientImage`: its pixels are then made on the GPU, its coefficients read by `n_threads` host
    threads (`StagedPlan.fill`)."""
    images = check_images(images)
    plan = BatchPlan(ds.plan_items(images), params, target_length, resample, ops=ops)
    return ds.run_once(plan, images, device, out, stream, n_threads)


class PendingImageInputs(PendingInputs):
    """The decoded images of one batch and their draws, to be resized, cropped, flipped, optionally augmented
    photometrically and JPEG-transformed straight into a model's resident input buffers at upload time: one upload of
    `[descriptors | taps | photometric lists | pixels]` from pinned memory, then dj_image_prep into the emitter's resident
    uint8 batch, dj_photometric on it in place when the batch carries operation lists, and dj_rgb_to_dct.  `ops`: None, or
    per image the photometric operations [(code, parameters), ...] of data/photometric.py with their draws made."""

    def __init__(self, prep, images, params, ops=None):
        self.prep = prep
        self.images = check_images(images)
        self.params = [(bool(s), int(o), bool(f)) for s, o, f in params]
        if ops is not None:
            from .photometric import check_ops
            ops = check_ops(ops, len(self.images))
        self.ops = ops
        # descriptors and taps are made where the batch is made (a generator's prefetch thread), not at upload time
        self.plan = BatchPlan(ds.plan_items(self.images), self.params, prep.target_length, prep.resample, ops=ops)
        PendingInputs.__init__(self, prep, self.plan.out_shape)

    def sliced(self, index):
        return PendingImageInputs(self.prep, self.images[index], self.params[index],
                                  None if self.ops is None else self.ops[index])

    def resident_pixels(self, device):
        return self.prep.run(self.plan, self.images, device)

    def pixels(self):
        """The (B, T, T, 3) uint8 batch computed on the host (`prep_host` per image, then `photometric_host`; an item that
        travels as coefficients is `jpeg_pixels_host` of its file first)."""
        p = self.prep
        out = np.stack([prep_host(im, p.target_length, s, o, f, p.resample)
                        for im, (s, o, f) in zip(ds.decoded(self.images), self.params)])
        if self.ops is not None:
            from .photometric import photometric_host
            out = photometric_host(out, self.ops)
        return out

    host_pixels = pixels


class DeviceImagePrep(ds.ResidentBuffers):
    """Stands where the reference's classifier generators resize, crop and flip each decoded image in PIL and then save
    it as a JPEG and read it back (vgg_jpeg_keras/generators/generators.py:141-187): the generator thread only decodes
    and draws, the pixels go up once and both steps run on the GPU when the model uploads the batch.  `resample`: a
    Pillow resampling code or name (None: Pillow's default, BICUBIC); `quality` / `tables` / `deconv`, `n_threads` and the
    buffers as `ResidentBuffers` keeps them.  Handed `CoefficientImage`s, the generator thread does not even decode: the
    files' coefficients go up and dj_jpeg_pixels makes the staged pixels."""

    def __init__(self, target_length=224, resample=None, quality=75, tables=None, deconv=False, n_threads=None):
        self.target_length = int(target_length)
        if self.target_length < 1:
            raise ValueError("target_length must be >= 1")
        self.resample = resolve_resample(resample)
        ds.ResidentBuffers.__init__(self, quality, tables, deconv, n_threads)

    def __call__(self, images, params, ops=None):
        return PendingImageInputs(self, images, params, ops)

    def photometric(self, plan, pixels):
        """dj_photometric alone, in place on `pixels`, on the current stream, with the operation lists of the `plan` that
        `run` staged last (`run` itself has already applied them to the batch it returned)."""
        return plan.launch_photometric(self._state[str(pixels.device)]["blob"], pixels)
