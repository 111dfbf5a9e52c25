"""What the device image-prep pipelines (data/image_prep.py: resize, crop, flip; data/patch_resize.py: window, mirror,
resize) share, none of which knows what a descriptor means:

  * Pillow's resampling taps (`filter_coeffs`) and the two-pass resize on the host (`resize_host`), for a caller-given set
    of allowed filters;
  * `TapsPool`: the deduplicated int32 pool of bounds and taps of one batch;
  * `StagedPlan`: descriptors, pool and the layout of one staging blob whose parts each start at a multiple of 64 bytes,
    with `fill`, `views` and (in the subclass) `launch`; and, for the items of a batch that are `CoefficientImage`s
    (data/jpeg_pixels.py: a JPEG file's bytes in place of its decoded pixels), the decode descriptors, tables and raw
    coefficient planes that dj_jpeg_pixels turns into those items' staged pixels on the GPU;
  * `StagingBuffers`: the per-device buffers kept across batches and the staging, upload and launch of one plan (`run`);
    `ResidentBuffers`: the same with the JPEG settings of an emitter;
  * `run_once`: the same with fresh buffers, for callers outside `Model`.

Pillow's `Image.resize` (src/libImaging/Resample.c) resamples in two passes, horizontal then vertical, each skipped when its
dimension is unchanged, with a uint8 image between them.  Per output sample it takes the source samples whose centres lie
within `support * max(scale, 1)` of the output sample's centre (scale = in_size / out_size), evaluates the filter in double
precision, normalises the weights by their sum (accumulated in source order) and rounds each to 22 fractional bits, half
away from zero.  A pass then computes, in 32-bit integers, clip8((2^21 + sum(pixel * tap)) >> 22).  NEAREST is not that
resampler but the nearest-neighbour affine transform (src/libImaging/Geometry.c: ImagingScaleAffine): output sample k reads
source sample int(x_k) with x_0 = scale / 2 and x_{k+1} = x_k + scale ACCUMULATED in double precision.  It is expressed as
one tap of 2^22 per sample, under which a pass copies, so the same two passes serve every filter.

All pixel arithmetic here is int32 / int64."""
import functools
import math

import numpy as np

from .jpeg_pixels import CoefficientImage

PRECISION_BITS = 32 - 8 - 2      # Pillow's fixed-point fraction for 8-bit images

# Pillow's `Image.Resampling` codes
NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 0, 1, 2, 3, 4, 5
FILTER_NAMES = {NEAREST: "NEAREST", LANCZOS: "LANCZOS", BILINEAR: "BILINEAR", BICUBIC: "BICUBIC", BOX: "BOX", HAMMING: "HAMMING"}


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


_WINDOWED = {BICUBIC: (_bicubic, 2.0), BILINEAR: (_bilinear, 1.0), BOX: (_box, 0.5), LANCZOS: (_lanczos, 3.0)}   # code -> (filter, support)
RESTATED = (NEAREST,) + tuple(sorted(_WINDOWED))      # every filter this module can make taps for


def resolve_filter(resample, allowed=RESTATED):
    """None (Pillow's default for `Image.resize`: BICUBIC), a Pillow resampling code or its name -> the code; ValueError
    for a filter outside `allowed`."""
    if resample is None:
        return BICUBIC
    if isinstance(resample, str):
        code = {v: k for k, v in FILTER_NAMES.items()}.get(resample.upper())
    else:
        code = int(resample)
    if code not in allowed:
        raise ValueError("resample filter %r is not supported: supported filters are %s"
                         % (resample, ", ".join(FILTER_NAMES[c] for c in sorted(allowed))))
    return code


def _frozen(bounds, taps):
    bounds.setflags(write=False)
    taps.setflags(write=False)
    return bounds, taps


@functools.lru_cache(maxsize=4096)
def windowed_coeffs(in_size, out_size, code):
    """(bounds, taps) of Pillow's two-pass resampler for one axis and one of its windowed filters, whatever the sizes."""
    filt, support = _WINDOWED[code]
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
    return _frozen(np.stack([xmin, xmax], axis=1).astype(np.int32), taps)


@functools.lru_cache(maxsize=4096)
def _nearest(in_size, out_size):
    scale = float(in_size) / out_size
    first = np.empty(out_size, dtype=np.int64)
    x = scale * 0.5
    for k in range(out_size):          # Pillow adds the step up; k * scale would round differently
        first[k] = int(x)
        x += scale
    # Pillow leaves a sample whose source index falls past the image unwritten; (k + 0.5) * scale stays below in_size - scale / 2,
    # far from where the accumulated rounding could carry it, and the minimum only keeps the index provably inside
    first = np.minimum(first, in_size - 1)
    bounds = np.stack([first, np.ones(out_size, dtype=np.int64)], axis=1).astype(np.int32)
    return _frozen(bounds, np.full((out_size, 1), 1 << PRECISION_BITS, dtype=np.int32))


@functools.lru_cache(maxsize=1024)
def _identity(size):
    bounds = np.stack([np.arange(size), np.ones(size, dtype=np.int64)], axis=1).astype(np.int32)
    return _frozen(bounds, np.full((size, 1), 1 << PRECISION_BITS, dtype=np.int32))


def identity_coeffs(size):
    """Taps of a skipped pass (the dimension is unchanged and Pillow copies): one tap of 2^22 per sample, under which a
    pass returns its input."""
    return _identity(int(size))


def check_sizes(in_size, out_size):
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("sizes must be >= 1, got %d -> %d" % (in_size, out_size))
    return in_size, out_size


def filter_coeffs(in_size, out_size, resample=None, allowed=RESTATED):
    """What `Image.resize` computes for one axis -> (bounds, taps): bounds (out_size, 2) int32 = first source index and
    tap count of each output sample, taps (out_size, ksize) int32 = its taps at 22 fractional bits (zero past the count);
    the identity taps when the size is unchanged (Pillow skips the pass, and its nearest-neighbour path then reads sample
    k for k).  The arrays are cached and read-only."""
    in_size, out_size = check_sizes(in_size, out_size)
    code = resolve_filter(resample, allowed)
    if in_size == out_size:
        return identity_coeffs(in_size)
    if code == NEAREST:
        return _nearest(in_size, out_size)
    return windowed_coeffs(in_size, out_size, code)


def resample_pass(img, bounds, taps):
    """One resampling pass along axis 1 of (rows, in_size, channels) uint8."""
    out = np.empty((img.shape[0], bounds.shape[0], img.shape[2]), dtype=np.uint8)
    for xx in range(bounds.shape[0]):
        x0, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        ss = (img[:, x0:x0 + n].astype(np.int32) * taps[xx, :n][None, :, None]).sum(axis=1, dtype=np.int32)
        out[:, xx] = np.clip((ss + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255)
    return out


def check_image(image):
    if isinstance(image, CoefficientImage):      # stands for the (H, W, 3) uint8 image its file decodes to
        return image
    image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError("expected an (H, W, 3) uint8 image, got %s %s" % (image.dtype, image.shape))
    return image


def check_images(images):
    images = [check_image(im) for im in images]
    if not images:
        raise ValueError("expected at least one image")
    return images


def plan_items(images):
    """What a plan takes per image: the `CoefficientImage` itself, (height, width) of a decoded array."""
    return [im if isinstance(im, CoefficientImage) else im.shape[:2] for im in images]


def item_shapes(items):
    """(height, width) of every item of `plan_items`, as plain ints."""
    return [(int(s.shape[0]), int(s.shape[1])) if isinstance(s, CoefficientImage) else (int(s[0]), int(s[1])) for s in items]


def decoded(images):
    """The batch with every `CoefficientImage` replaced by the host statement of its pixels."""
    return [im.pixels() if isinstance(im, CoefficientImage) else im for im in images]


def resize_host(image, size, resample=None, allowed=RESTATED):
    """`Image.fromarray(image).resize(size, resample)` for an (H, W, 3) uint8 image, size = (width, height) and a filter
    of `allowed`."""
    image = check_image(image)
    code = resolve_filter(resample, allowed)
    width, height = int(size[0]), int(size[1])
    if width < 1 or height < 1:
        raise ValueError("size must be positive, got %r" % (size,))
    h, w = image.shape[:2]
    if width != w:
        image = resample_pass(image, *filter_coeffs(w, width, code, allowed))
    if height != h:
        image = resample_pass(image.transpose(1, 0, 2), *filter_coeffs(h, height, code, allowed)).transpose(1, 0, 2)
    return np.ascontiguousarray(image)


# ---- one staging blob per batch ---------------------------------------------------------------------------------------------
ALIGN = 64
MAX_FILL_THREADS = 16      # of `fill`'s batch reader when the caller names no count: past that a batch of 32 files gains nothing


def round_up(n, a=ALIGN):
    return -(-n // a) * a


class TapsPool(object):
    """The int32 pool of one batch: bounds then taps of every distinct axis resize, one copy each."""

    def __init__(self, allowed=RESTATED):
        self.allowed, self.chunks, self.where, self.n_ints = allowed, [], {}, 0

    def get(self, key, in_size, out_size, code):
        """-> (bounds offset, taps offset, tap row length, bounds) in ints from the pool's start, of
        `filter_coeffs(in_size, out_size, code)`; equal keys share one copy."""
        if key not in self.where:
            bounds, taps = filter_coeffs(in_size, out_size, code, self.allowed)
            self.where[key] = (self.n_ints, self.n_ints + bounds.size, taps.shape[1], bounds)
            self.chunks.extend((bounds.reshape(-1), taps.reshape(-1)))
            self.n_ints += bounds.size + taps.size
        return self.where[key]

    def array(self):
        return np.concatenate(self.chunks).astype(np.int32, copy=False)


# dj_jpeg_pixels_desc (include/dj_hip.h), C layout
DECODE_DTYPE = np.dtype([("coef_offset", np.int64, 3), ("sample_offset", np.int64, 3), ("dst_offset", np.int64),
                         ("dst_stride", np.int64)]
                        + [(n, np.int32) for n in ("table_offset", "n_components", "h_samp", "v_samp", "height", "width",
                                                   "ya", "yb", "xa", "xb")]
                        + [(n, np.int32, 3) for n in ("blocks_h", "blocks_w", "by0", "by1", "bx0", "bx1")], align=True)


def needed_samples(a, b, factor, extent):
    """[lo, hi] of the samples of a component sampled `factor` (1 or 2) times coarser than the image, of real extent
    `extent`, that image rows / columns a..b-1 read -- the triangle filter's neighbour included."""
    s = factor - 1
    return max((a >> s) - s, 0), min(((b - 1) >> s) + s, extent - 1)


class StagedPlan(object):
    """Everything the kernels of one ragged batch need except the pixels' bytes: `desc` (one DESC_DTYPE record per
    image), `pool`, `src_bytes` / `scratch_bytes`, `out_shape` and the layout of one staging blob.  A subclass fills
    `desc` in its geometry loop, then calls `_lay_out` with its parts in order: (name, array), (name, None) for a part
    this batch does not carry, and ("src", src_bytes) for the pixels, which its `_fill_pixels` writes.  Part `name`
    starts at `<name>_offset`, a multiple of 64; the blob ends with its last part (`nbytes`).  `launch` issues the
    plan's kernels in order.

    A batch in which some items are `CoefficientImage`s: the subclass calls `_plan_decode` with, per item, the rectangle
    it stages and where that rectangle's pixels lie in the "src" part, and puts the parts it returns BEHIND its own.  Such
    items' pixels are not copied by `_fill_pixels`: `fill` has the batch reader write their raw coefficient planes
    into the blob, and `launch_decode` (first in the subclass's `launch`) runs dj_jpeg_pixels, which writes the
    rectangles where `_fill_pixels` would have.  Whole planes are staged, about 3 bytes per image pixel, because the
    reader's workers emit whole planes, each copied from the worker's own planes to its place in the blob.  The sample planes of the inverse DCT take scratch behind `scratch_bytes` as the
    subclass left it.  A batch without such items has no such parts: its blob and its launches are what they were."""
    DESC_DTYPE = None
    decode = None          # DECODE_DTYPE records of the CoefficientImage items that stage something; None without any

    def _plan_decode(self, images, rects, dst):
        """images: the batch, any item possibly a `CoefficientImage`; rects[i] = (ya, yb, xa, xb) staged of item i (empty:
        nothing); dst[i] = (byte offset in the "src" part, row stride) of that rectangle.  Grows `scratch_bytes`; -> the
        parts to lay out behind the plan's own ([] when no item needs decoding)."""
        items = [i for i, (im, (ya, yb, xa, xb)) in enumerate(zip(images, rects))
                 if isinstance(im, CoefficientImage) and yb > ya and xb > xa]
        if not items:
            return []
        self.decode_items = items
        self.decode = np.zeros(len(items), dtype=DECODE_DTYPE)
        self.tables = np.zeros((len(items), 3, 64), dtype=np.int32)
        self.plane_offsets = np.zeros((len(items), 4), dtype=np.int64)      # relative to the "coef" part
        self.plane_capacity = np.zeros((len(items), 4), dtype=np.int64)
        coef_off, scratch_off = 0, round_up(self.scratch_bytes)
        for j, i in enumerate(items):
            im, (ya, yb, xa, xb), d = images[i], rects[i], self.decode[j]
            height, width = im.shape[:2]
            h, v = im.sampling
            d["dst_offset"], d["dst_stride"] = dst[i]
            d["table_offset"], d["n_components"], d["h_samp"], d["v_samp"] = 192 * j, im.n_components, h, v
            d["height"], d["width"], d["ya"], d["yb"], d["xa"], d["xb"] = height, width, ya, yb, xa, xb
            self.tables[j] = im.tables()
            for c, (bh, bw) in enumerate(im.grids()):
                fy, fx = (1, 1) if c == 0 else (v, h)
                r0, r1 = needed_samples(ya, yb, fy, -(-height // fy))
                k0, k1 = needed_samples(xa, xb, fx, -(-width // fx))
                d["blocks_h"][c], d["blocks_w"][c] = bh, bw
                d["by0"][c], d["by1"][c], d["bx0"][c], d["bx1"][c] = r0 // 8, r1 // 8 + 1, k0 // 8, k1 // 8 + 1
                d["coef_offset"][c], d["sample_offset"][c] = coef_off, scratch_off
                self.plane_offsets[j, c], self.plane_capacity[j, c] = coef_off, bh * bw * 64
                coef_off += round_up(bh * bw * 128)
                scratch_off += round_up((r1 // 8 + 1 - r0 // 8) * (k1 // 8 + 1 - k0 // 8) * 64)
        self.coef_bytes, self.scratch_bytes = coef_off, scratch_off
        return [("decode", self.decode), ("tables", self.tables), ("coef", self.coef_bytes)]

    def decode_views(self, blob):
        """(descriptors, tables, coefficient planes) of a staging buffer or of its device copy, as `views` returns its
        parts (numpy: a DECODE_DTYPE array, int32, bytes; torch: bytes all three)."""
        desc = self.part(blob, self.decode_offset, self.decode, DECODE_DTYPE)
        tables = self.part(blob, self.tables_offset, self.tables, np.int32)
        return desc, tables, blob[self.coef_offset:self.coef_offset + self.coef_bytes]

    def launch_decode(self, blob_host, blob_dev, scratch, stream=None):
        """dj_jpeg_pixels for the plan's `CoefficientImage` items: their staged rectangles appear in the "src" part of
        `blob_dev` as if the host had copied them there.  Nothing without such items."""
        if self.decode is None:
            return
        from .. import kernels
        desc_h, tables_h, _ = self.decode_views(blob_host)
        desc_d, tables_d, coef_d = self.decode_views(blob_dev)
        kernels.jpeg_pixels(coef_d, desc_d, desc_h, tables_d, tables_h,
                            blob_dev[self.src_offset:self.src_offset + self.src_bytes], scratch, stream=stream)

    def _lay_out(self, parts):
        self.parts, end = [], 0
        for name, content in parts:
            offset = round_up(end)
            setattr(self, name + "_offset", offset)
            if isinstance(content, np.ndarray):
                self.parts.append((offset, content.view(np.uint8).reshape(-1)))
                end = offset + content.nbytes
            else:
                end = offset + (content or 0)
        self.nbytes = end

    def fill(self, staging, images, n_threads=None):
        """Write descriptors, pool, the pixels and whatever else the plan carries into `staging`, a uint8 numpy array of
        at least `nbytes`.  The raw coefficient planes of `CoefficientImage` items are entropy-decoded into it by
        `n_threads` host threads (None: one per CPU this process may use, 16 at the most), each into planes of its own that
        it then copies to their place in `staging`; a file that fails there raises ValueError."""
        for offset, content in self.parts:
            staging[offset:offset + content.size] = content
        self._fill_pixels(staging[self.src_offset:self.src_offset + self.src_bytes], images)
        if self.decode is not None:
            self._read_planes(staging, images, self.decode_items, n_threads)

    def _read_planes(self, staging, images, items, n_threads=None):
        """Entropy-decode the raw coefficient planes of `images[i]` for i in `items` into the "coef" part of `staging`,
        where `plane_offsets` / `plane_capacity` say, on `n_threads` host threads (None: one per CPU this process may use,
        16 at the most); ValueError naming the items that failed."""
        from ..jpeg2dct import numpy as reader
        status = reader.read_raw_batch([images[i].data for i in items], staging[:self.nbytes],
                                       self.plane_offsets + self.coef_offset, self.plane_capacity,
                                       n_threads if n_threads is not None else min(reader.default_threads(), MAX_FILL_THREADS))
        if status.any():
            raise ValueError("items %s of the batch could not be read: %s"
                             % ([items[j] for j in np.flatnonzero(status)], reader.last_error()))

    def part(self, blob, offset, array, dtype=None):
        """The bytes of `array`'s part at `offset` of a staging buffer (a uint8 numpy array: viewed as `dtype`) or of its
        device copy (a 1-D uint8 torch tensor: bytes)."""
        part = blob[offset:offset + array.nbytes]
        return part.view(dtype) if dtype is not None and isinstance(blob, np.ndarray) else part

    def views(self, blob):
        """(pixels, descriptors, pool) of a staging buffer or of its device copy: a uint8 numpy array (descriptors come
        back as a DESC_DTYPE array, the pool as int32) or a 1-D uint8 torch tensor (descriptors stay bytes)."""
        src = blob[self.src_offset:self.src_offset + self.src_bytes]
        desc = self.part(blob, 0, self.desc, self.DESC_DTYPE)
        pool = self.part(blob, self.pool_offset, self.pool)
        if isinstance(blob, np.ndarray):
            return src, desc, pool.view(np.int32)
        import torch
        return src, desc, pool.view(torch.int32)

    def launch(self, blob_host, blob_dev, out, scratch, stream=None):
        raise NotImplementedError


def _uint8(n, device=None):
    import torch
    return torch.empty(n, dtype=torch.uint8).pin_memory() if device is None else torch.empty(n, dtype=torch.uint8, device=device)


def run_once(plan, images, device=None, out=None, stream=None, n_threads=None):
    """Pin, fill (`n_threads` as for `StagedPlan.fill`), upload and launch `plan` with fresh buffers -> its uint8 CUDA
    batch, complete on return."""
    import torch
    device = torch.device(device if device is not None else "cuda")
    staging = _uint8(plan.nbytes)
    host = staging.numpy()
    plan.fill(host, images, n_threads)
    blob = staging.to(device, non_blocking=True)
    if out is None:
        out = torch.empty(plan.out_shape, dtype=torch.uint8, device=device)
    plan.launch(host, blob, out, _uint8(plan.scratch_bytes, device), stream=stream)
    # the pinned buffer and the scratch go away with this frame: wait for the copy and the kernels
    (torch.cuda.current_stream(device) if stream is None else torch.cuda.ExternalStream(stream)).synchronize()
    return out


class StagingBuffers(object):
    """The buffers of whoever stages plans, kept per device and grown on demand: two pinned staging buffers used in turn,
    each refilled only after the upload that last read it has finished (an event recorded behind the copy), the device
    copy of the staging buffer, the scratch of the horizontal pass and the uint8 batch.  `n_threads`: host threads
    `StagedPlan.fill` reads coefficient planes with (None: its default).  A plan whose kernels report per-item statuses
    (`n_status`, `status_view`, `failures`) has them copied to a pinned array of the slot in front of the slot's event;
    they are read, and a failure raised as ValueError, when the slot is next used (`_check_slot`)."""

    def __init__(self, n_threads=None):
        self.n_threads = None if n_threads is None else int(n_threads)
        self._state = {}

    def blob(self, device):
        """The device copy of the staging buffer that `run` uploaded last on `device`."""
        import torch
        return self._state[str(torch.device(device))]["blob"]

    @staticmethod
    def _grown(tensor, nbytes, device=None):
        if tensor is None or tensor.numel() < nbytes:
            return _uint8(max(nbytes, 0 if tensor is None else tensor.numel() * 3 // 2), device)
        return tensor

    def run(self, plan, images, device, out=None):
        """Stage, upload and launch `plan` on the current stream -> the resident uint8 batch of `plan.out_shape` (valid
        until the next call on this device).  `out`: what the plan's `launch` writes instead of that batch (a plan whose
        kernels write a model's input buffers themselves); it is returned."""
        import torch
        device = torch.device(device)
        # a slot: [pinned staging buffer, event, pinned int32 statuses, (plan, images) whose statuses are on their way]
        st = self._state.setdefault(str(device), {"slots": [[None, None, None, None], [None, None, None, None]], "turn": 0,
                                                  "blob": None, "scratch": None, "out": None})
        slot = st["slots"][st["turn"]]
        st["turn"] ^= 1
        if slot[1] is not None:
            slot[1].synchronize()          # the copy that last read this staging buffer
            self._check_slot(slot)
        n_out = int(np.prod(plan.out_shape))
        slot[0] = self._grown(slot[0], plan.nbytes)
        for name, n in (("blob", plan.nbytes), ("scratch", plan.scratch_bytes), ("out", n_out)):
            st[name] = self._grown(st[name], n, device)
        host = slot[0].numpy()
        plan.fill(host, images, self.n_threads)
        st["blob"][:plan.nbytes].copy_(slot[0][:plan.nbytes], non_blocking=True)
        if slot[1] is None:
            slot[1] = torch.cuda.Event()
        n_status = getattr(plan, "n_status", 0)
        if not n_status:
            slot[1].record()
        if out is None:
            out = st["out"][:n_out].view(plan.out_shape)
        plan.launch(host, st["blob"], out, st["scratch"])
        if n_status:
            # the kernels' per-segment statuses follow the batch to the slot's pinned array, in front of the slot's event:
            # nothing waits here, and whoever next waits for the event (the slot's reuse, `check`) reads them
            if slot[2] is None or slot[2].numel() < n_status:
                slot[2] = torch.empty(max(n_status, 1024), dtype=torch.int32).pin_memory()
            slot[2][:n_status].copy_(plan.status_view(st["scratch"]), non_blocking=True)
            slot[3] = (plan, images)
            slot[1].record()
        return out

    @staticmethod
    def _check_slot(slot):
        """After the slot's event: raise ValueError for the batch last emitted through it if a kernel reported a failure."""
        if slot[3] is None:
            return
        (plan, images), slot[3] = slot[3], None
        text = plan.failures(slot[2].numpy(), images)
        if text is not None:
            raise ValueError(text)


class ResidentBuffers(StagingBuffers):
    """An emitter's JPEG settings (`quality` / `tables` / `deconv` as for `DeviceDCTEmitter`) and its `StagingBuffers`."""

    def __init__(self, quality=75, tables=None, deconv=False, n_threads=None):
        from .jpeg_dct import resolve_tables
        self.tables = resolve_tables(quality, tables)
        self.quality = None if tables is not None else int(quality)
        self.deconv = bool(deconv)
        StagingBuffers.__init__(self, n_threads)
