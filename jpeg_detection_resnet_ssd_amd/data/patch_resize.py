"""A window of a decoded image on a constant background, optionally mirrored, resized to the network's input size: the
pixel side of the SSD augmentation chain (data/ssd_augment.py), whose expand, crop, flip and resize stages compose into
exactly that.  The geometry of one image is

    (win_y0, win_x0, win_h, win_w, flip, filter, background)

with the window in source-image coordinates (it may start at negative coordinates and may extend past either far edge:
what lies outside the image is `background`), `flip` the left-right mirror of the window BEFORE the resize and `filter` a
Pillow resampling code.  `patch_resize_host` states the contract in numpy, csrc/dj_patchresize.hip runs it on the GPU
(`DevicePatchResize`, `PendingPatchInputs`: the protocol of `PendingImageInputs`).

The resize is Pillow's, as everywhere in this package (data/image_prep.py), here with all five filters the chain draws from:
BICUBIC, BILINEAR and BOX as restated there, LANCZOS through the same tap computation, and NEAREST, which in
`Image.resize` is not the two-pass resampler but the nearest-neighbour affine transform (src/libImaging/Geometry.c:
ImagingScaleAffine): output sample k reads source sample int(x_k) with x_0 = scale / 2 and x_{k+1} = x_k + scale
ACCUMULATED in double precision.  It is expressed as one tap of 2^22 per sample, under which a resampling pass copies, so
the same two passes serve all five."""
import functools

import numpy as np

from . import image_prep as ip
from .image_prep import BICUBIC, BILINEAR, BOX, LANCZOS, NEAREST, PRECISION_BITS

FILTERS = (NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX)
_NAMES = {c: ip._NAMES[c] for c in FILTERS}


def resolve_filter(resample):
    """A Pillow resampling code or its name (None: BICUBIC, Pillow's default) -> the code; ValueError for HAMMING and
    anything else that is not restated."""
    if resample is None:
        return BICUBIC
    if isinstance(resample, str):
        code = {v: k for k, v in _NAMES.items()}.get(resample.upper())
    else:
        code = int(resample)
    if code not in FILTERS:
        raise ValueError("resample filter %r is not supported: supported filters are %s"
                         % (resample, ", ".join(_NAMES[c] for c in sorted(FILTERS))))
    return code


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
    taps = np.full((out_size, 1), 1 << PRECISION_BITS, dtype=np.int32)
    bounds.setflags(write=False)
    taps.setflags(write=False)
    return bounds, taps


def filter_coeffs(in_size, out_size, resample=None):
    """(bounds, taps) of one axis as `image_prep.resample_coeffs` returns them, for any of the five filters; the identity
    taps when the size is unchanged (Pillow skips the pass, and its nearest-neighbour path then reads sample k for k)."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("sizes must be >= 1, got %d -> %d" % (in_size, out_size))
    code = resolve_filter(resample)
    if in_size == out_size:
        return ip.identity_coeffs(in_size)
    if code == NEAREST:
        return _nearest(in_size, out_size)
    return ip._coeffs(in_size, out_size, code)


def resize_host(image, size, resample=None):
    """`Image.fromarray(image).resize(size, resample)` for an (H, W, 3) uint8 image, size = (width, height) and any of
    NEAREST, BILINEAR, BICUBIC, BOX, LANCZOS."""
    image = ip._check_image(image)
    code = resolve_filter(resample)
    width, height = int(size[0]), int(size[1])
    if width < 1 or height < 1:
        raise ValueError("size must be positive, got %r" % (size,))
    h, w = image.shape[:2]
    if width != w:
        image = ip._pass(image, *filter_coeffs(w, width, code))
    if height != h:
        image = ip._pass(image.transpose(1, 0, 2), *filter_coeffs(h, height, code)).transpose(1, 0, 2)
    return np.ascontiguousarray(image)


def check_geometry(geometry):
    """-> (win_y0, win_x0, win_h, win_w, flip, filter code, (r, g, b)) with plain ints; ValueError for an empty window."""
    y0, x0, wh, ww, flip, filt, background = geometry
    y0, x0, wh, ww = int(y0), int(x0), int(wh), int(ww)
    if wh < 1 or ww < 1:
        raise ValueError("the window must hold at least one pixel, got %d x %d" % (wh, ww))
    bg = tuple(int(c) for c in background)
    if len(bg) != 3 or min(bg) < 0 or max(bg) > 255:
        raise ValueError("background: expected three values in 0..255, got %r" % (background,))
    return y0, x0, wh, ww, bool(flip), resolve_filter(filt), bg


def _overlap(origin, size, limit):
    """[lo, hi) of the image axis 0..limit that the window [origin, origin + size) covers (hi <= lo: none of it)."""
    return max(origin, 0), min(origin + size, limit)


def window_host(image, geometry):
    """The window of `geometry` before its resize, (win_h, win_w, 3) uint8: a canvas of the background with the part of
    the image under it pasted in, as the reference's `CropPad` builds it, mirrored when the flip is set."""
    image = ip._check_image(image)
    y0, x0, wh, ww, flip, _, bg = check_geometry(geometry)
    canvas = np.zeros((wh, ww, 3), dtype=np.uint8)
    canvas[:, :] = bg
    ya, yb = _overlap(y0, wh, image.shape[0])
    xa, xb = _overlap(x0, ww, image.shape[1])
    if yb > ya and xb > xa:
        canvas[ya - y0:yb - y0, xa - x0:xb - x0] = image[ya:yb, xa:xb]
    return np.ascontiguousarray(canvas[:, ::-1]) if flip else canvas


def patch_resize_host(image, geometry, out_height, out_width):
    """The pixel contract of one geometry -> (out_height, out_width, 3) uint8: the window, mirrored first when the flip is
    set (Pillow's normalised taps need not be mirror-symmetric, so the mirror belongs on the fetch), then
    `resize_host(window, (out_width, out_height), filter)`."""
    return resize_host(window_host(image, geometry), (int(out_width), int(out_height)), check_geometry(geometry)[5])


# ---- the same on the GPU: csrc/dj_patchresize.hip ---------------------------------------------------------------------------
# dj_patch_resize_desc (include/dj_hip.h), C layout
DESC_DTYPE = np.dtype([(n, np.int64) for n in ("src_offset", "src_stride", "scratch_offset")]
                      + [(n, np.int32) for n in ("src_h", "src_w", "win_y0", "win_x0", "win_h", "win_w", "flip", "background",
                                                 "h_bounds", "h_taps", "h_ksize", "v_bounds", "v_taps", "v_ksize")],
                      align=True)
_round_up = ip._round_up


class PatchPlan(object):
    """Everything `dj_patch_resize` needs for one ragged batch except the pixels' bytes: per-image descriptors, the shared
    int32 pool of bounds and taps (one copy per distinct (window size, output size, filter) triple of the batch) and the
    layout of one staging buffer `[descriptors | pool | pixels]`, each part at a multiple of 64 bytes.  Only the
    rectangle of each image that its window covers is staged: the descriptor's window is relative to that rectangle.
    `photometric` (optional): per image, the `PhotoParams` of data/ssd_photometric.py that dj_ssd_photometric applies to
    the staged rectangles before the resize; the records then travel as a fourth part behind the pixels.  Without them
    there is no such part and the layout is the three-part one."""

    def __init__(self, shapes, geometries, out_height, out_width, photometric=None):
        shapes = [(int(h), int(w)) for h, w in shapes]
        geometries = [check_geometry(g) for g in geometries]
        if len(shapes) != len(geometries) or not shapes:
            raise ValueError("expected one geometry per image and at least one image")
        oh, ow = int(out_height), int(out_width)
        if oh < 1 or ow < 1:
            raise ValueError("the output size must be positive, got %d x %d" % (oh, ow))
        self.batch, self.out_height, self.out_width = len(shapes), oh, ow
        self.desc = np.zeros(self.batch, dtype=DESC_DTYPE)
        self.rects = []
        chunks, where, n_ints = [], {}, 0

        def pooled(in_size, out_size, code):
            nonlocal n_ints
            key = (in_size, out_size, code if in_size != out_size else -1)
            if key not in where:
                bounds, taps = filter_coeffs(in_size, out_size, code)
                where[key] = (n_ints, n_ints + bounds.size, taps.shape[1])
                chunks.extend((bounds.reshape(-1), taps.reshape(-1)))
                n_ints += bounds.size + taps.size
            return where[key]

        src_off = scratch_off = 0
        for i, ((h, w), (y0, x0, wh, ww, flip, code, bg)) in enumerate(zip(shapes, geometries)):
            ya, yb = _overlap(y0, wh, h)
            xa, xb = _overlap(x0, ww, w)
            if yb <= ya or xb <= xa:
                ya = yb = xa = xb = 0          # the window misses the image: nothing is staged, every fetch is background
            self.rects.append((ya, yb, xa, xb))
            hb, hk, hn = pooled(ww, ow, code)
            vb, vk, vn = pooled(wh, oh, code)
            d = self.desc[i]
            d["src_offset"], d["src_stride"], d["scratch_offset"] = src_off, 3 * (xb - xa), scratch_off
            d["src_h"], d["src_w"] = yb - ya, xb - xa
            d["win_y0"], d["win_x0"], d["win_h"], d["win_w"] = y0 - ya, x0 - xa, wh, ww
            d["flip"], d["background"] = int(flip), bg[0] | (bg[1] << 8) | (bg[2] << 16)
            d["h_bounds"], d["h_taps"], d["h_ksize"] = hb, hk, hn
            d["v_bounds"], d["v_taps"], d["v_ksize"] = vb, vk, vn
            src_off += _round_up(3 * (xb - xa) * (yb - ya))
            scratch_off += _round_up(3 * ow * wh)
        self.pool = np.concatenate(chunks).astype(np.int32, copy=False)
        self.shapes = shapes
        self.src_bytes, self.scratch_bytes = max(src_off, 64), scratch_off
        self.pool_offset = _round_up(self.desc.nbytes)
        self.src_offset = self.pool_offset + _round_up(self.pool.nbytes)
        self.nbytes = self.src_offset + self.src_bytes
        self.photo = self.photo_offset = None
        if photometric is not None:
            from .ssd_photometric import pack_params
            self.photo = pack_params(photometric)
            if len(self.photo) != self.batch:
                raise ValueError("expected one photometric record per image: %d records for %d images"
                                 % (len(self.photo), self.batch))
            self.photo_offset = _round_up(self.nbytes)
            self.nbytes = self.photo_offset + self.photo.nbytes

    def fill(self, staging, images):
        """Write descriptors, pool, the staged rectangles' pixels and the photometric records, if any, into `staging`, a
        uint8 numpy array of at least `nbytes`."""
        staging[:self.desc.nbytes] = self.desc.view(np.uint8)
        if self.photo is not None:
            staging[self.photo_offset:self.photo_offset + self.photo.nbytes] = self.photo.view(np.uint8)
        staging[self.pool_offset:self.pool_offset + self.pool.nbytes] = self.pool.view(np.uint8)
        for d, (ya, yb, xa, xb), img in zip(self.desc, self.rects, images):
            if yb > ya:
                o = self.src_offset + int(d["src_offset"])
                staging[o:o + 3 * (xb - xa) * (yb - ya)].reshape(yb - ya, xb - xa, 3)[...] = img[ya:yb, xa:xb]

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

    def photo_view(self, blob):
        """The photometric records of a staging buffer or of its device copy (a PARAMS_DTYPE array, or bytes for a torch
        tensor); None for a plan without them."""
        if self.photo is None:
            return None
        part = blob[self.photo_offset:self.photo_offset + self.photo.nbytes]
        if isinstance(blob, np.ndarray):
            from .ssd_photometric import PARAMS_DTYPE
            return part.view(PARAMS_DTYPE)
        return part


def _run_plan(plan, blob_host, blob_dev, out, scratch, stream=None):
    from .. import kernels
    src_h, desc_h, pool_h = plan.views(blob_host)
    src_d, desc_d, pool_d = plan.views(blob_dev)
    if plan.photo is not None:         # in place on the staged rectangles, before the resize reads them
        kernels.ssd_photometric(src_d, desc_d, desc_h, plan.photo_view(blob_dev), plan.photo_view(blob_host), stream=stream)
    return kernels.patch_resize(src_d, desc_d, desc_h, pool_d, pool_h, out, scratch, stream=stream)


def patch_resize_device(images, geometries, out_height, out_width, device=None, out=None, stream=None, photometric=None):
    """`patch_resize_host` for a list of (H_i, W_i, 3) uint8 images and one geometry each on the GPU -> the
    (B, out_height, out_width, 3) uint8 CUDA batch, for callers outside `Model` (fresh buffers every call;
    `DevicePatchResize` keeps its own).  `photometric`: one `PhotoParams` per image, applied before the window is cut
    (`ssd_photometric_host`)."""
    import torch
    images = ip._check_images(images)
    plan = PatchPlan([im.shape[:2] for im in images], geometries, out_height, out_width, photometric)
    device = torch.device(device if device is not None else "cuda")
    staging = torch.empty(plan.nbytes, dtype=torch.uint8).pin_memory()
    host = staging.numpy()
    plan.fill(host, images)
    blob = staging.to(device, non_blocking=True)
    if out is None:
        out = torch.empty((plan.batch, plan.out_height, plan.out_width, 3), dtype=torch.uint8, device=device)
    scratch = torch.empty(plan.scratch_bytes, dtype=torch.uint8, device=device)
    _run_plan(plan, host, blob, out, scratch, stream=stream)
    # the pinned buffer and the scratch go away with this frame: wait for the copy and the two passes
    (torch.cuda.current_stream(device) if stream is None else torch.cuda.ExternalStream(stream)).synchronize()
    return out


class PendingPatchInputs(object):
    """The decoded images of one batch and their geometries, to be windowed, mirrored, resized and JPEG-transformed
    straight into a model's resident input buffers at upload time: the protocol of `PendingImageInputs`
    (`Model.train_on_batch / predict_on_batch / predict / fit_generator` accept it where they accept the list of input
    arrays).  `photometric`: one `PhotoParams` of data/ssd_photometric.py per image, or None; the stage runs on the
    decoded image, before its window is cut (dj_ssd_photometric on the GPU, `ssd_photometric_host` in the host twins)."""

    def __init__(self, prep, images, geometries, photometric=None):
        self.prep = prep
        self.images = ip._check_images(images)
        self.geometries = [check_geometry(g) for g in geometries]
        self.photometric = None
        if photometric is not None:
            from .ssd_photometric import check_params
            self.photometric = [check_params(p) for p in photometric]
        # descriptors and taps are made where the batch is made (a generator's prefetch thread), not at upload time
        self.plan = PatchPlan([im.shape[:2] for im in self.images], self.geometries, prep.out_height, prep.out_width,
                              self.photometric)

    def __len__(self):
        return len(self.images)

    @property
    def shape(self):
        """Of the pixel batch the model sees: `shape[0]` is the batch size, as for the first array of an input list."""
        return (len(self.images), self.prep.out_height, self.prep.out_width, 3)

    def __getitem__(self, index):
        if not isinstance(index, slice):
            raise TypeError("PendingPatchInputs can only be sliced along the batch")
        return PendingPatchInputs(self.prep, self.images[index], self.geometries[index],
                                  self.photometric[index] if self.photometric is not None else None)

    @property
    def shapes(self):
        from .jpeg_dct import input_shapes
        return input_shapes(len(self.images), self.prep.out_height, self.prep.out_width, self.prep.deconv)

    def emit_into(self, buffers):
        """One upload of `[descriptors | taps | pixels | photometric records]` from pinned memory, then
        dj_ssd_photometric on the staged pixels when there are records, dj_patch_resize into the emitter's resident uint8
        batch and dj_rgb_to_dct into `buffers` (float32 CUDA tensors of `self.shapes`), all on the current stream."""
        from .. import kernels
        buffers = list(buffers)
        if [tuple(t.shape) for t in buffers] != [tuple(s) for s in self.shapes]:
            raise ValueError("emit_into: expected buffers of shapes %s, got %s"
                             % (self.shapes, [tuple(t.shape) for t in buffers]))
        pixels = self.prep.run(self.plan, self.images, buffers[0].device)
        outs = tuple(buffers) if self.prep.deconv else (buffers[0], buffers[1][..., :64], buffers[1][..., 64:])
        kernels.rgb_to_dct(pixels, self.prep.tables, outs, normalized=True)
        return buffers

    def pixels(self):
        """The (B, out_height, out_width, 3) uint8 batch computed on the host (`ssd_photometric_host` where there are
        records, then `patch_resize_host`, per image)."""
        p = self.prep
        images = self.images
        if self.photometric is not None:
            from .ssd_photometric import ssd_photometric_host
            images = [ssd_photometric_host(im, rec) for im, rec in zip(images, self.photometric)]
        return np.stack([patch_resize_host(im, g, p.out_height, p.out_width) for im, g in zip(images, self.geometries)])

    def numpy(self):
        """The model inputs computed on the host (`pixels`, then `rgb_to_dct_host` per image), float32."""
        from .jpeg_dct import rgb_to_dct_host
        planes = [rgb_to_dct_host(img, tables=self.prep.tables) for img in self.pixels()]
        y, cb, cr = (np.stack([p[i] for p in planes]).astype(np.float32) for i in range(3))
        return [y, cb, cr] if self.prep.deconv else [y, np.concatenate([cb, cr], axis=-1)]


class DevicePatchResize(object):
    """Stands where the reference's SSD generator runs the geometric stages of its augmentation chain in numpy and cv2
    and then saves each image as a JPEG and reads it back: the generator thread only decodes and plans
    (`SSDDataAugmentation.plan`), the covered part of each image goes up once and both steps run on the GPU when the model
    uploads the batch -- after the chain's photometric stage, when the plan drew one (`photometric`).  `quality` / `tables`
    / `deconv` as for `DeviceDCTEmitter`.

    Buffers are kept per emitter and device and grown on demand, as in `DeviceImagePrep`: two pinned staging buffers used
    in turn, each refilled only after the upload that last read it has finished, the device copy of the staging buffer,
    the scratch of the horizontal pass and the uint8 batch."""

    def __init__(self, out_height=300, out_width=300, quality=75, tables=None, deconv=False):
        from .jpeg_dct import _resolve_tables
        self.out_height, self.out_width = int(out_height), int(out_width)
        if self.out_height < 1 or self.out_width < 1:
            raise ValueError("the output size must be positive")
        self.tables = _resolve_tables(quality, tables)
        self.quality = None if tables is not None else int(quality)
        self.deconv = bool(deconv)
        self._state = {}

    def __call__(self, images, geometries, photometric=None):
        return PendingPatchInputs(self, images, geometries, photometric)

    def run(self, plan, images, device):
        """Stage, upload and launch dj_ssd_photometric (for a plan with records) and dj_patch_resize for `plan` on the
        current stream -> the resident (B, out_height, out_width, 3) uint8 batch (valid until the next call on this
        device)."""
        import torch
        grown = ip.DeviceImagePrep._grown
        device = torch.device(device)
        st = self._state.setdefault(str(device), {"slots": [[None, None], [None, None]], "turn": 0, "blob": None,
                                                  "scratch": None, "out": None})
        slot = st["slots"][st["turn"]]
        st["turn"] ^= 1
        if slot[1] is not None:
            slot[1].synchronize()          # the copy that last read this staging buffer
        slot[0] = grown(slot[0], plan.nbytes, lambda n: torch.empty(n, dtype=torch.uint8).pin_memory())
        st["blob"] = grown(st["blob"], plan.nbytes, lambda n: torch.empty(n, dtype=torch.uint8, device=device))
        st["scratch"] = grown(st["scratch"], plan.scratch_bytes, lambda n: torch.empty(n, dtype=torch.uint8, device=device))
        n_out = plan.batch * plan.out_height * plan.out_width * 3
        st["out"] = grown(st["out"], n_out, lambda n: torch.empty(n, dtype=torch.uint8, device=device))
        host = slot[0].numpy()
        plan.fill(host, images)
        st["blob"][:plan.nbytes].copy_(slot[0][:plan.nbytes], non_blocking=True)
        if slot[1] is None:
            slot[1] = torch.cuda.Event()
        slot[1].record()
        out = st["out"][:n_out].view(plan.batch, plan.out_height, plan.out_width, 3)
        _run_plan(plan, host, st["blob"], out, st["scratch"])
        return out
