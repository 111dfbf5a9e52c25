"""A window of a decoded image on a constant background, optionally mirrored, resized to the network's input size: the
pixel side of the SSD augmentation chain (data/ssd_augment.py), whose expand, crop, flip and resize stages compose into
exactly that.  The geometry of one image is

    (win_y0, win_x0, win_h, win_w, flip, filter, background)

with the window in source-image coordinates (it may start at negative coordinates and may extend past either far edge:
what lies outside the image is `background`), `flip` the left-right mirror of the window BEFORE the resize and `filter` a
Pillow resampling code.  `patch_resize_host` states the contract in numpy, csrc/dj_patchresize.hip runs it on the GPU
(`DevicePatchResize`, `PendingPatchInputs`: the protocol of `PendingImageInputs`).

The resize is Pillow's, as everywhere in this package (data/device_staging.py restates it), here with all five filters the
chain draws from: BICUBIC, BILINEAR, BOX, LANCZOS and NEAREST.  The staging blob, the resident buffers and the upload are
device_staging's too; what is here is the geometry of one image, the copy of its staged rectangle and the order of the
kernels."""
import numpy as np

from . import device_staging as ds
from .device_staging import BICUBIC, BILINEAR, BOX, LANCZOS, NEAREST, PRECISION_BITS, check_image, check_images, round_up  # noqa: F401
from .jpeg_dct import PendingInputs
from .jpeg_pixels import CoefficientImage

FILTERS = (NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX)


def resolve_filter(resample):
    """A Pillow resampling code or its name (None: BICUBIC, Pillow's default) -> the code; ValueError for HAMMING and
    anything else that is not restated."""
    return ds.resolve_filter(resample, FILTERS)


def filter_coeffs(in_size, out_size, resample=None):
    """(bounds, taps) of one axis as `image_prep.resample_coeffs` returns them, for any of the five filters; the identity
    taps when the size is unchanged (Pillow skips the pass, and its nearest-neighbour path then reads sample k for k)."""
    return ds.filter_coeffs(in_size, out_size, resample, FILTERS)


def resize_host(image, size, resample=None):
    """`Image.fromarray(image).resize(size, resample)` for an (H, W, 3) uint8 image, size = (width, height) and any of
    NEAREST, BILINEAR, BICUBIC, BOX, LANCZOS."""
    return ds.resize_host(image, size, resample, FILTERS)


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
    image = check_image(image)
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


class PatchPlan(ds.StagedPlan):
    """Everything `dj_patch_resize` needs for one ragged batch except the pixels' bytes: per-image descriptors, the shared
    int32 pool of bounds and taps (one copy per distinct (window size, output size, filter) triple of the batch) and the
    layout of one staging buffer `[descriptors | pool | pixels]`, each part at a multiple of 64 bytes.  Only the
    rectangle of each image that its window covers is staged: the descriptor's window is relative to that rectangle.
    `photometric` (optional): per image, the `PhotoParams` of data/ssd_photometric.py that dj_ssd_photometric applies to
    the staged rectangles before the resize; the records then travel as a fourth part behind the pixels.  Without them
    there is no such part and the layout is the three-part one.  An item of `shapes` may be a `CoefficientImage` instead of
    (height, width): its staged rectangle is then reconstructed on the GPU from the file's coefficients (`StagedPlan`),
    whose parts lie behind all of these.  `extra`: further (name, array) parts a caller sends up in the same blob (the warp
    records of data/rgb_warp.py), laid out behind the plan's own and before the decode parts."""
    DESC_DTYPE = DESC_DTYPE
    photo_offset = None

    def __init__(self, shapes, geometries, out_height, out_width, photometric=None, extra=()):
        items = list(shapes)
        shapes = ds.item_shapes(items)
        geometries = [check_geometry(g) for g in geometries]
        if len(shapes) != len(geometries) or not shapes:
            raise ValueError("expected one geometry per image and at least one image")
        oh, ow = int(out_height), int(out_width)
        if oh < 1 or ow < 1:
            raise ValueError("the output size must be positive, got %d x %d" % (oh, ow))
        self.batch, self.out_height, self.out_width = len(shapes), oh, ow
        self.out_shape = (self.batch, oh, ow, 3)
        self.desc = np.zeros(self.batch, dtype=DESC_DTYPE)
        self.rects = []
        taps = ds.TapsPool(FILTERS)
        src_off = scratch_off = 0
        for i, ((h, w), (y0, x0, wh, ww, flip, code, bg)) in enumerate(zip(shapes, geometries)):
            ya, yb = _overlap(y0, wh, h)
            xa, xb = _overlap(x0, ww, w)
            if yb <= ya or xb <= xa:
                ya = yb = xa = xb = 0          # the window misses the image: nothing is staged, every fetch is background
            self.rects.append((ya, yb, xa, xb))
            hb, hk, hn, _ = taps.get((ww, ow, code if ww != ow else -1), ww, ow, code)
            vb, vk, vn, _ = taps.get((wh, oh, code if wh != oh else -1), wh, oh, code)
            d = self.desc[i]
            d["src_offset"], d["src_stride"], d["scratch_offset"] = src_off, 3 * (xb - xa), scratch_off
            d["src_h"], d["src_w"] = yb - ya, xb - xa
            d["win_y0"], d["win_x0"], d["win_h"], d["win_w"] = y0 - ya, x0 - xa, wh, ww
            d["flip"], d["background"] = int(flip), bg[0] | (bg[1] << 8) | (bg[2] << 16)
            d["h_bounds"], d["h_taps"], d["h_ksize"] = hb, hk, hn
            d["v_bounds"], d["v_taps"], d["v_ksize"] = vb, vk, vn
            src_off += round_up(3 * (xb - xa) * (yb - ya))
            scratch_off += round_up(3 * ow * wh)
        self.pool = taps.array()
        self.shapes = shapes
        self.src_bytes, self.scratch_bytes = max(src_off, 64), scratch_off
        parts = [("desc", self.desc), ("pool", self.pool), ("src", self.src_bytes)]
        self.photo = None
        if photometric is not None:
            from .ssd_photometric import pack_params
            self.photo = pack_params(photometric)
            if len(self.photo) != self.batch:
                raise ValueError("expected one photometric record per image: %d records for %d images"
                                 % (len(self.photo), self.batch))
            parts.append(("photo", self.photo))
        parts += list(extra)
        parts += self._plan_decode(items, self.rects, [(int(d["src_offset"]), int(d["src_stride"])) for d in self.desc])
        self._lay_out(parts)

    def _fill_pixels(self, src, images):
        for d, (ya, yb, xa, xb), img in zip(self.desc, self.rects, images):
            if yb > ya and not isinstance(img, CoefficientImage):
                o = int(d["src_offset"])
                src[o:o + 3 * (xb - xa) * (yb - ya)].reshape(yb - ya, xb - xa, 3)[...] = img[ya:yb, xa:xb]

    def photo_view(self, blob):
        """The photometric records of a staging buffer or of its device copy (a PARAMS_DTYPE array, or bytes for a torch
        tensor); None for a plan without them."""
        if self.photo is None:
            return None
        return self.part(blob, self.photo_offset, self.photo, self.photo.dtype)

    def launch(self, blob_host, blob_dev, out, scratch, stream=None):
        """dj_jpeg_pixels for the items that travel as coefficients, then dj_ssd_photometric in place on the staged
        rectangles when the plan carries records, before dj_patch_resize reads them into `out`."""
        from .. import kernels
        self.launch_decode(blob_host, blob_dev, scratch, stream)
        src_h, desc_h, pool_h = self.views(blob_host)
        src_d, desc_d, pool_d = self.views(blob_dev)
        if self.photo is not None:
            kernels.ssd_photometric(src_d, desc_d, desc_h, self.photo_view(blob_dev), self.photo_view(blob_host), stream=stream)
        return kernels.patch_resize(src_d, desc_d, desc_h, pool_d, pool_h, out, scratch, stream=stream)


def patch_resize_device(images, geometries, out_height, out_width, device=None, out=None, stream=None, photometric=None):
    """`patch_resize_host` for a list of (H_i, W_i, 3) uint8 images and one geometry each on the GPU -> the
    (B, out_height, out_width, 3) uint8 CUDA batch, for callers outside `Model` (fresh buffers every call;
    `DevicePatchResize` keeps its own).  `photometric`: one `PhotoParams` per image, applied before the window is cut
    (`ssd_photometric_host`)."""
    images = check_images(images)
    plan = PatchPlan(_plan_items(images), geometries, out_height, out_width, photometric)
    return ds.run_once(plan, images, device, out, stream)


_plan_items = ds.plan_items


class PendingPatchInputs(PendingInputs):
    """The decoded images of one batch and their geometries, to be windowed, mirrored, resized and JPEG-transformed
    straight into a model's resident input buffers at upload time: one upload of `[descriptors | taps | pixels |
    photometric records]` from pinned memory, then dj_ssd_photometric on the staged pixels when there are records,
    dj_patch_resize into the emitter's resident uint8 batch and dj_rgb_to_dct.  `photometric`: one `PhotoParams` of
    data/ssd_photometric.py per image, or None; the stage runs on the decoded image, before its window is cut
    (dj_ssd_photometric on the GPU, `ssd_photometric_host` in the host twins)."""

    def __init__(self, prep, images, geometries, photometric=None):
        self.prep = prep
        self.images = check_images(images)
        self.geometries = [check_geometry(g) for g in geometries]
        self.photometric = None
        if photometric is not None:
            from .ssd_photometric import check_params
            self.photometric = [check_params(p) for p in photometric]
        # descriptors and taps are made where the batch is made (a generator's prefetch thread), not at upload time
        self.plan = PatchPlan(_plan_items(self.images), self.geometries, prep.out_height, prep.out_width,
                              self.photometric)
        PendingInputs.__init__(self, prep, self.plan.out_shape)

    def sliced(self, index):
        return PendingPatchInputs(self.prep, self.images[index], self.geometries[index],
                                  self.photometric[index] if self.photometric is not None else None)

    def resident_pixels(self, device):
        return self.prep.run(self.plan, self.images, device)

    def pixels(self):
        """The (B, out_height, out_width, 3) uint8 batch computed on the host (`ssd_photometric_host` where there are
        records, then `patch_resize_host`, per image; an item that travels as coefficients is `jpeg_pixels_host` of its
        file first)."""
        p = self.prep
        images = ds.decoded(self.images)
        if self.photometric is not None:
            from .ssd_photometric import ssd_photometric_host
            images = [ssd_photometric_host(im, rec) for im, rec in zip(images, self.photometric)]
        return np.stack([patch_resize_host(im, g, p.out_height, p.out_width) for im, g in zip(images, self.geometries)])

    host_pixels = pixels


class DevicePatchResize(ds.ResidentBuffers):
    """Stands where the reference's SSD generator runs the geometric stages of its augmentation chain in numpy and cv2
    and then saves each image as a JPEG and reads it back: the generator thread decodes and plans
    (`SSDDataAugmentation.plan`) -- or, handed `CoefficientImage`s, does not even decode: the files' coefficients go up and
    dj_jpeg_pixels makes the staged pixels --, the covered part of each image goes up once and both steps run on the GPU
    when the model uploads the batch -- after the chain's photometric stage, when the plan drew one (`photometric`).  `quality` / `tables`
    / `deconv` and the buffers as `ResidentBuffers` keeps them."""

    def __init__(self, out_height=300, out_width=300, quality=75, tables=None, deconv=False, n_threads=None):
        self.out_height, self.out_width = int(out_height), int(out_width)
        if self.out_height < 1 or self.out_width < 1:
            raise ValueError("the output size must be positive")
        ds.ResidentBuffers.__init__(self, quality, tables, deconv, n_threads)

    def __call__(self, images, geometries, photometric=None):
        return PendingPatchInputs(self, images, geometries, photometric)
