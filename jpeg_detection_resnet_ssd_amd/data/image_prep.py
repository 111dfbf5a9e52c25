"""Decoded image -> the network-sized RGB pixels the JPEG emission step starts from: steps 2 to 4 of the reference's
classifier generators (classification_part/vgg_jpeg_keras/generators/generators.py:141-167 and :299-325), which run
between `Image.open(...).convert("RGB")` and `im.save(fake_file, format="jpeg")`:

  2. `im.resize((int(round(width * r)), int(round(height * r))))` with r = target_length / min(im.size) (scale=True), or
     `im.resize((target_length, target_length))` (scale=False);
  3. `im.crop(...)` of target_length along the longer side at `offset` (along x when the resized width is larger than the
     resized height, along y otherwise -- with equal sides the only offset is 0 and the two agree);
  4. `im.transpose(FLIP_LEFT_RIGHT)` when the flip was drawn.

All three are an integer function of the pixels.  Pillow's `Image.resize` (src/libImaging/Resample.c) resamples in two
passes, horizontal then vertical, each skipped when its dimension is unchanged, with a uint8 image between them.  Per
output sample it takes the source samples whose centres lie within `support * max(scale, 1)` of the output sample's centre
(scale = in_size / out_size), evaluates the filter in double precision, normalises the weights by their sum (accumulated
in source order) and rounds each to 22 fractional bits, half away from zero.  A pass then computes, in 32-bit integers,
clip8((2^21 + sum(pixel * tap)) >> 22).  `resample_coeffs` restates the tap computation, `resize_host` the two passes and
`prep_host` steps 2 to 4 for one image; tests/test_image_prep_cpu.py pins them to the installed Pillow and to
tests/golden/image_prep.npz.  csrc/dj_imgprep.hip runs the same arithmetic on the GPU (`DeviceImagePrep`,
`prep_device`): the host computes the taps, the device does everything that touches pixels.

All pixel arithmetic here is int32 / int64."""
import functools
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2      # Pillow's fixed-point fraction for 8-bit images

# Pillow's `Image.Resampling` codes
NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 0, 1, 2, 3, 4, 5
_NAMES = {NEAREST: "NEAREST", LANCZOS: "LANCZOS", BILINEAR: "BILINEAR", BICUBIC: "BICUBIC", BOX: "BOX", HAMMING: "HAMMING"}


def _bicubic(x):
    a = -0.5      # Pillow's (Keys) parameter
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def _bilinear(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _box(x):
    return np.where((x > -0.5) & (x <= 0.5), 1.0, 0.0)


def _lanczos(x):
    # Pillow's truncated sinc, a = 3: sinc(x) * sinc(x / 3) on -3 <= x < 3, with sinc(x) = sin(pi x) / (pi x)
    def sinc(v):
        v = v * math.pi
        return np.where(v == 0.0, 1.0, np.sin(v) / np.where(v == 0.0, 1.0, v))
    return np.where((x >= -3.0) & (x < 3.0), sinc(x) * sinc(x / 3), 0.0)


_FILTERS = {BICUBIC: (_bicubic, 2.0), BILINEAR: (_bilinear, 1.0), BOX: (_box, 0.5)}     # code -> (filter, support)
SUPPORTED = tuple(sorted(_FILTERS))
# restated for data/patch_resize.py only: `resolve_resample`, and with it every entry point of this module, keeps refusing it
_MORE_FILTERS = {LANCZOS: (_lanczos, 3.0)}


def resolve_resample(resample):
    """None (Pillow's default for `Image.resize`: BICUBIC), a Pillow resampling code or its name -> the code; ValueError
    for a filter this module does not restate."""
    if resample is None:
        return BICUBIC
    if isinstance(resample, str):
        code = {v: k for k, v in _NAMES.items()}.get(resample.upper())
    else:
        code = int(resample)
    if code not in _FILTERS:
        raise ValueError("resample filter %r is not supported: supported filters are %s"
                         % (resample, ", ".join(_NAMES[c] for c in SUPPORTED)))
    return code


@functools.lru_cache(maxsize=4096)
def _coeffs(in_size, out_size, code):
    filt, support = _FILTERS[code] if code in _FILTERS else _MORE_FILTERS[code]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # the C cast truncates; operands are >= -support
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    live = x < xmax[:, None]
    w = np.where(live, filt(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss), 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for k in range(ksize):             # Pillow's order of accumulation
        ww = ww + w[:, k]
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    v = w * float(1 << PRECISION_BITS)
    taps = np.where(w < 0, np.trunc(-0.5 + v), np.trunc(0.5 + v)).astype(np.int32)
    taps[~live] = 0
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    bounds.setflags(write=False)
    taps.setflags(write=False)
    return bounds, taps


def resample_coeffs(in_size, out_size, resample=None):
    """What Pillow's resampler computes for one axis -> (bounds, coeffs): bounds (out_size, 2) int32 = first source
    index and tap count of each output sample, coeffs (out_size, ksize) int32 = its taps at 22 fractional bits (zero past
    the count).  The arrays are cached and read-only."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("sizes must be >= 1, got %d -> %d" % (in_size, out_size))
    return _coeffs(in_size, out_size, resolve_resample(resample))


def identity_coeffs(size):
    """Taps of a skipped pass (the dimension is unchanged and Pillow copies): one tap of 2^22 per sample, under which a
    pass returns its input."""
    return _identity(int(size))


@functools.lru_cache(maxsize=1024)
def _identity(size):
    bounds = np.stack([np.arange(size), np.ones(size, dtype=np.int64)], axis=1).astype(np.int32)
    taps = np.full((size, 1), 1 << PRECISION_BITS, dtype=np.int32)
    bounds.setflags(write=False)
    taps.setflags(write=False)
    return bounds, taps


def axis_coeffs(in_size, out_size, resample=None):
    """`resample_coeffs`, or the identity taps when the pass is skipped."""
    if int(in_size) == int(out_size):
        resolve_resample(resample)
        return identity_coeffs(in_size)
    return resample_coeffs(in_size, out_size, resample)


def _pass(img, bounds, taps):
    """One resampling pass along axis 1 of (rows, in_size, channels) uint8."""
    out = np.empty((img.shape[0], bounds.shape[0], img.shape[2]), dtype=np.uint8)
    for xx in range(bounds.shape[0]):
        x0, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        ss = (img[:, x0:x0 + n].astype(np.int32) * taps[xx, :n][None, :, None]).sum(axis=1, dtype=np.int32)
        out[:, xx] = np.clip((ss + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255)
    return out


def _check_image(image):
    image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError("expected an (H, W, 3) uint8 image, got %s %s" % (image.dtype, image.shape))
    return image


def resize_host(image, size, resample=None):
    """`Image.fromarray(image).resize(size, resample)` for an (H, W, 3) uint8 image and size = (width, height)."""
    image = _check_image(image)
    code = resolve_resample(resample)
    width, height = int(size[0]), int(size[1])
    if width < 1 or height < 1:
        raise ValueError("size must be positive, got %r" % (size,))
    h, w = image.shape[:2]
    if width != w:
        image = _pass(image, *resample_coeffs(w, width, code))
    if height != h:
        image = _pass(image.transpose(1, 0, 2), *resample_coeffs(h, height, code)).transpose(1, 0, 2)
    return np.ascontiguousarray(image)


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
    image = _check_image(image)
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
_ALIGN = 64


def _round_up(n, a=_ALIGN):
    return -(-n // a) * a


class BatchPlan(object):
    """Everything `dj_image_prep` needs for one ragged batch except the pixels' bytes: per-image descriptors, the shared
    int32 pool of bounds and taps (one copy per distinct (source size, resized size) pair of the batch) and the layout of
    one staging buffer `[descriptors | pool | photometric lists | pixels]`, each part at a multiple of 64 bytes.  `ops`
    (optional): per image, the photometric operations [(code, parameters), ...] of data/photometric.py that
    dj_photometric runs on the prepared pixels; without it the third part is empty."""

    def __init__(self, shapes, params, target_length=224, resample=None, ops=None):
        code = resolve_resample(resample)
        t = int(target_length)
        shapes = [(int(h), int(w)) for h, w in shapes]
        params = [(bool(s), int(o), bool(f)) for s, o, f in params]
        if len(shapes) != len(params) or not shapes:
            raise ValueError("expected one (scale, offset, flip) per image and at least one image")
        self.batch, self.target, self.resample = len(shapes), t, code
        self.desc = np.zeros(self.batch, dtype=DESC_DTYPE)
        chunks, where, n_ints = [], {}, 0

        def pooled(in_size, out_size):
            nonlocal n_ints
            key = (in_size, out_size)
            if key not in where:
                bounds, taps = axis_coeffs(in_size, out_size, code)
                where[key] = (n_ints, n_ints + bounds.size, taps.shape[1], bounds)
                chunks.extend((bounds.reshape(-1), taps.reshape(-1)))
                n_ints += bounds.size + taps.size
            return where[key]

        src_off = scratch_off = 0
        for i, ((h, w), (scale, offset, flip)) in enumerate(zip(shapes, params)):
            rw, rh, cx, cy = prep_geometry(h, w, t, scale, offset)
            hb, hk, hn, _ = pooled(w, rw)
            vb, vk, vn, vbounds = pooled(h, rh)
            row0 = int(vbounds[cy, 0])
            n_rows = int(vbounds[cy + t - 1, 0] + vbounds[cy + t - 1, 1]) - row0
            d = self.desc[i]
            d["src_offset"], d["src_stride"], d["scratch_offset"] = src_off, 3 * w, scratch_off
            d["src_h"], d["src_w"], d["res_h"], d["res_w"] = h, w, rh, rw
            d["crop_y"], d["crop_x"], d["flip"] = cy, cx, int(flip)
            d["h_bounds"], d["h_taps"], d["h_ksize"] = hb, hk, hn
            d["v_bounds"], d["v_taps"], d["v_ksize"] = vb, vk, vn
            d["row0"], d["n_rows"] = row0, n_rows
            src_off += _round_up(3 * w * h)
            scratch_off += _round_up(3 * t * n_rows)
        self.pool = np.concatenate(chunks).astype(np.int32, copy=False)
        self.shapes = shapes
        self.src_bytes, self.scratch_bytes = src_off, scratch_off
        self.desc_offset = 0
        self.pool_offset = _round_up(self.desc.nbytes)
        self.ops = None
        if ops is not None:
            from .photometric import pack_ops
            self.ops = pack_ops(ops, self.batch)
        self.ops_offset = self.pool_offset + _round_up(self.pool.nbytes)
        self.src_offset = self.ops_offset + (_round_up(self.ops.nbytes) if self.ops is not None else 0)
        self.nbytes = self.src_offset + self.src_bytes

    def fill(self, staging, images):
        """Write descriptors, pool and the images' pixels into `staging`, a uint8 numpy array of at least `nbytes`."""
        staging[:self.desc.nbytes] = self.desc.view(np.uint8)
        staging[self.pool_offset:self.pool_offset + self.pool.nbytes] = self.pool.view(np.uint8)
        if self.ops is not None:
            staging[self.ops_offset:self.ops_offset + self.ops.nbytes] = self.ops.view(np.uint8).reshape(-1)
        for d, (h, w), img in zip(self.desc, self.shapes, images):
            o = self.src_offset + int(d["src_offset"])
            staging[o:o + 3 * w * h].reshape(h, w, 3)[...] = img

    def views(self, blob):
        """(pixels, descriptors, pool) of a staging buffer or of its device copy: a uint8 numpy array (descriptors come
        back as a DESC_DTYPE array, the pool as int32) or a 1-D uint8 torch tensor (descriptors stay bytes)."""
        src = blob[self.src_offset:self.src_offset + self.src_bytes]
        desc = blob[:self.desc.nbytes]
        pool = blob[self.pool_offset:self.pool_offset + self.pool.nbytes]
        if isinstance(blob, np.ndarray):
            return src, desc.view(DESC_DTYPE), pool.view(np.int32)
        import torch
        return src, desc, pool.view(torch.int32)


def _run_photometric(plan, blob_dev, pixels, shift_out=None, stream=None):
    """dj_photometric on the prepared batch, its lists read from the device copy of the staging buffer."""
    from .. import kernels
    lists = blob_dev[plan.ops_offset:plan.ops_offset + plan.ops.nbytes]
    return kernels.photometric(pixels, lists, plan.ops, shift_out=shift_out, stream=stream)


def _check_images(images):
    images = [_check_image(im) for im in images]
    if not images:
        raise ValueError("expected at least one image")
    return images


def _run_plan(plan, blob_host, blob_dev, out, scratch, stream=None):
    from .. import kernels
    src_h, desc_h, pool_h = plan.views(blob_host)
    src_d, desc_d, pool_d = plan.views(blob_dev)
    return kernels.image_prep(src_d, desc_d, desc_h, pool_d, pool_h, plan.target, out, scratch, stream=stream)


def prep_device(images, params, target_length=224, resample=None, device=None, out=None, stream=None, ops=None):
    """`prep_host` for a list of (H_i, W_i, 3) uint8 images and per-image (scale, offset, flip) on the GPU -> the
    (B, target_length, target_length, 3) uint8 CUDA batch, for callers outside `Model` (fresh buffers every call;
    `DeviceImagePrep` keeps its own).  `ops`: per-image photometric operation lists, run on the prepared pixels."""
    import torch
    images = _check_images(images)
    plan = BatchPlan([im.shape[:2] for im in images], params, target_length, resample, ops=ops)
    device = torch.device(device if device is not None else "cuda")
    staging = torch.empty(plan.nbytes, dtype=torch.uint8).pin_memory()
    host = staging.numpy()
    plan.fill(host, images)
    blob = staging.to(device, non_blocking=True)
    t = plan.target
    if out is None:
        out = torch.empty((plan.batch, t, t, 3), dtype=torch.uint8, device=device)
    scratch = torch.empty(plan.scratch_bytes, dtype=torch.uint8, device=device)
    _run_plan(plan, host, blob, out, scratch, stream=stream)
    if plan.ops is not None:
        _run_photometric(plan, blob, out, stream=stream)
    # the pinned buffer and the scratch go away with this frame: wait for the copy and the two passes
    (torch.cuda.current_stream(device) if stream is None else torch.cuda.ExternalStream(stream)).synchronize()
    return out


class PendingImageInputs(object):
    """The decoded images of one batch and their draws, to be resized, cropped, flipped, optionally augmented
    photometrically and JPEG-transformed straight into a model's resident input buffers at upload time: the protocol of
    `PendingDCTInputs` (`Model.train_on_batch / predict_on_batch / predict / fit_generator` accept it where they accept
    the list of input arrays).  `ops`: None, or per image the photometric operations [(code, parameters), ...] of
    data/photometric.py with their draws made."""

    def __init__(self, prep, images, params, ops=None):
        self.prep = prep
        self.images = _check_images(images)
        self.params = [(bool(s), int(o), bool(f)) for s, o, f in params]
        if ops is not None:
            from .photometric import check_ops
            ops = check_ops(ops, len(self.images))
        self.ops = ops
        # descriptors and taps are made where the batch is made (a generator's prefetch thread), not at upload time
        self.plan = BatchPlan([im.shape[:2] for im in self.images], self.params, prep.target_length, prep.resample, ops=ops)

    def __len__(self):
        return len(self.images)

    @property
    def shape(self):
        """Of the pixel batch the model sees: `shape[0]` is the batch size, as for the first array of an input list."""
        t = self.prep.target_length
        return (len(self.images), t, t, 3)

    def __getitem__(self, index):
        if not isinstance(index, slice):
            raise TypeError("PendingImageInputs can only be sliced along the batch")
        return PendingImageInputs(self.prep, self.images[index], self.params[index],
                                  None if self.ops is None else self.ops[index])

    @property
    def shapes(self):
        from .jpeg_dct import input_shapes
        t = self.prep.target_length
        return input_shapes(len(self.images), t, t, self.prep.deconv)

    def emit_into(self, buffers):
        """One upload of `[descriptors | taps | photometric lists | pixels]` from pinned memory, then dj_image_prep into
        the emitter's resident uint8 batch, dj_photometric on it in place when the batch carries operation lists, and
        dj_rgb_to_dct into `buffers` (float32 CUDA tensors of `self.shapes`), all on the current stream."""
        from .. import kernels
        buffers = list(buffers)
        if [tuple(t.shape) for t in buffers] != [tuple(s) for s in self.shapes]:
            raise ValueError("emit_into: expected buffers of shapes %s, got %s"
                             % (self.shapes, [tuple(t.shape) for t in buffers]))
        pixels = self.prep.run(self.plan, self.images, buffers[0].device)
        if self.plan.ops is not None:
            self.prep.photometric(self.plan, pixels)
        outs = tuple(buffers) if self.prep.deconv else (buffers[0], buffers[1][..., :64], buffers[1][..., 64:])
        kernels.rgb_to_dct(pixels, self.prep.tables, outs, normalized=True)
        return buffers

    def pixels(self):
        """The (B, T, T, 3) uint8 batch computed on the host (`prep_host` per image, then `photometric_host`)."""
        p = self.prep
        out = np.stack([prep_host(im, p.target_length, s, o, f, p.resample) for im, (s, o, f) in zip(self.images, self.params)])
        if self.ops is not None:
            from .photometric import photometric_host
            out = photometric_host(out, self.ops)
        return out

    def numpy(self):
        """The model inputs computed on the host (`pixels`, then `rgb_to_dct_host` per image), float32."""
        from .jpeg_dct import rgb_to_dct_host
        planes = [rgb_to_dct_host(img, tables=self.prep.tables) for img in self.pixels()]
        y, cb, cr = (np.stack([p[i] for p in planes]).astype(np.float32) for i in range(3))
        return [y, cb, cr] if self.prep.deconv else [y, np.concatenate([cb, cr], axis=-1)]


class DeviceImagePrep(object):
    """Stands where the reference's classifier generators resize, crop and flip each decoded image in PIL and then save
    it as a JPEG and read it back (vgg_jpeg_keras/generators/generators.py:141-187): the generator thread only decodes
    and draws, the pixels go up once and both steps run on the GPU when the model uploads the batch.  `resample`: a
    Pillow resampling code or name (None: Pillow's default, BICUBIC); `quality` / `tables` / `deconv` as for
    `DeviceDCTEmitter`.

    Buffers are kept per emitter and device and grown on demand: two pinned staging buffers used in turn, each refilled
    only after the upload that last read it has finished (an event recorded behind the copy), the device copy of the
    staging buffer, the scratch of the horizontal pass and the uint8 batch."""

    def __init__(self, target_length=224, resample=None, quality=75, tables=None, deconv=False):
        from .jpeg_dct import _resolve_tables
        self.target_length = int(target_length)
        if self.target_length < 1:
            raise ValueError("target_length must be >= 1")
        self.resample = resolve_resample(resample)
        self.tables = _resolve_tables(quality, tables)
        self.quality = None if tables is not None else int(quality)
        self.deconv = bool(deconv)
        self._state = {}

    def __call__(self, images, params, ops=None):
        return PendingImageInputs(self, images, params, ops)

    @staticmethod
    def _grown(tensor, nbytes, make):
        if tensor is None or tensor.numel() < nbytes:
            return make(max(nbytes, 0 if tensor is None else tensor.numel() * 3 // 2))
        return tensor

    def run(self, plan, images, device):
        """Stage, upload and launch dj_image_prep for `plan` on the current stream -> the resident (B, T, T, 3) uint8
        batch (valid until the next call on this device)."""
        import torch
        device = torch.device(device)
        st = self._state.setdefault(str(device), {"slots": [[None, None], [None, None]], "turn": 0, "blob": None,
                                                  "scratch": None, "out": None})
        slot = st["slots"][st["turn"]]
        st["turn"] ^= 1
        if slot[1] is not None:
            slot[1].synchronize()          # the copy that last read this staging buffer
        slot[0] = self._grown(slot[0], plan.nbytes, lambda n: torch.empty(n, dtype=torch.uint8).pin_memory())
        st["blob"] = self._grown(st["blob"], plan.nbytes, lambda n: torch.empty(n, dtype=torch.uint8, device=device))
        st["scratch"] = self._grown(st["scratch"], plan.scratch_bytes,
                                    lambda n: torch.empty(n, dtype=torch.uint8, device=device))
        n_out = plan.batch * plan.target * plan.target * 3
        st["out"] = self._grown(st["out"], n_out, lambda n: torch.empty(n, dtype=torch.uint8, device=device))
        host = slot[0].numpy()
        plan.fill(host, images)
        st["blob"][:plan.nbytes].copy_(slot[0][:plan.nbytes], non_blocking=True)
        if slot[1] is None:
            slot[1] = torch.cuda.Event()
        slot[1].record()
        out = st["out"][:n_out].view(plan.batch, plan.target, plan.target, 3)
        _run_plan(plan, host, st["blob"], out, st["scratch"])
        return out

    def photometric(self, plan, pixels):
        """dj_photometric on the batch `run` has just prepared for `plan`, in place, on the current stream: the
        operation lists went up with the descriptors."""
        return _run_photometric(plan, self._state[str(pixels.device)]["blob"], pixels)
