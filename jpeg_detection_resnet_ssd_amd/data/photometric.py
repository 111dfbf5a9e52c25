"""The photometric augmentations of the reference's classifier generators (`saturation`, `brightness`, `contrast`,
`lighting` of classification_part/vgg_jpeg_keras/generators/helper.py:12-45, applied between the flip and the JPEG
emission) as a statement that does not depend on the machine's BLAS or LAPACK: `photometric_host` is the twin of
csrc/dj_photometric.hip and the oracle of its tests.  The callables themselves (numpy, drawing from `np.random`) live in
vgg_jpeg_keras/generators/helper.py; here an operation is `(code, parameters)` with its draw already made.

What decides bits, all float64:

  grey value    `rgb.dot([0.299, 0.587, 0.114])` evaluates to fma(b, w2, fma(g, w1, r * w0)) (measured on numpy 2.2.6 with
                scipy-openblas 0.3.29; tests/golden/photometric.npz holds a probe).  `grey_exact` restates that with
                exact rationals, rounding once where the fused form rounds.
  mean          `contrast` takes `grayscale(rgb).mean()`: numpy's sum over the flattened grey values, divided by n.  The
                sum is pairwise within chunks of 8192 elements and sequential over the chunks (`pairwise_sum`,
                `numpy_sum`).
  lighting      the first and second moments as exact integers, covariance of pixels / 255 with N - 1 in the denominator
                as one division per entry, eigenvalues ascending, each eigenvector's sign chosen so that its component
                of largest magnitude is positive (lowest index on ties; `fix_signs`).  LAPACK leaves the signs open and
                the normal draws are symmetric, so this rule is a choice, not a deviation in distribution.  An image of
                one pixel has no covariance; its shift is zero.
  every operation ends in `np.clip(x, 0, 255)` and truncation to uint8: a chain passes bytes from one to the next."""
from fractions import Fraction

import numpy as np

SATURATION, BRIGHTNESS, CONTRAST, LIGHTING = 1, 2, 3, 4      # DJ_PHOTO_* of include/dj_hip.h
MAX_OPS = 4
NAMES = {SATURATION: "saturation", BRIGHTNESS: "brightness", CONTRAST: "contrast", LIGHTING: "lighting"}
GREY_WEIGHTS = (0.299, 0.587, 0.114)
MAX_PIXELS = 1 << 18              # per image on the device: moments, covariance and leaf table stay exact / in LDS

# dj_photometric_ops (include/dj_hip.h), C layout
OPS_DTYPE = np.dtype([("n_ops", np.int32), ("code", np.int32, (MAX_OPS,)), ("reserved", np.int32),
                      ("param", np.float64, (MAX_OPS, 3))], align=True)

_W = tuple(Fraction(w) for w in GREY_WEIGHTS)       # the doubles' exact values
_grey_cache, _rg_cache = {}, {}


def grey_exact(rgb):
    """fma(b, w2, fma(g, w1, r * w0)) per pixel of an (..., 3) uint8 array -> float64, in exact arithmetic: three
    roundings, one per operation of the fused form.  Cached per distinct pixel (and per distinct (r, g) below it)."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.shape[-1] == 3
    flat = rgb.reshape(-1, 3).astype(np.int64)
    keys = (flat[:, 0] << 16) | (flat[:, 1] << 8) | flat[:, 2]
    uniq, inverse = np.unique(keys, return_inverse=True)
    vals = np.empty(uniq.size, dtype=np.float64)
    for i, k in enumerate(uniq.tolist()):
        v = _grey_cache.get(k)
        if v is None:
            t = _rg_cache.get(k >> 8)
            if t is None:
                t = _rg_cache[k >> 8] = Fraction(float(((k >> 8) & 255) * _W[1] + Fraction(float((k >> 16) * _W[0]))))
            v = _grey_cache[k] = float((k & 255) * _W[2] + t)
        vals[i] = v
    return vals[inverse.reshape(-1)].reshape(rgb.shape[:-1])


def pairwise_sum(a):
    """numpy's sum of a contiguous float64 vector, restated: fewer than 8 elements in order; up to 128 with eight
    accumulators over stride 8, combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the tail added in order; longer ranges
    split at n // 2 rounded down to a multiple of 8."""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    n = a.size
    if n < 8:
        res = np.float64(0.0)
        for v in a:
            res = res + v
        return float(res)
    if n <= 128:
        r = a[:8].copy()
        i = 8
        while i < n - n % 8:
            r = r + a[i:i + 8]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for v in a[i:]:
            res = res + v
        return float(res)
    n2 = n // 2
    n2 -= n2 % 8
    return float(np.float64(pairwise_sum(a[:n2])) + np.float64(pairwise_sum(a[n2:])))


def numpy_sum(a, chunk=8192):
    """`np.sum` of a contiguous float64 array, restated: the reduction hands the flattened values to the inner loop in
    chunks of its buffer size (8192 elements by default), each chunk is summed pairwise and the chunks' sums are added in
    order, starting from 0."""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    acc = np.float64(0.0)
    for i in range(0, a.size, chunk):
        acc = acc + np.float64(pairwise_sum(a[i:i + chunk]))
    return float(acc)


def grey_mean(pixels):
    """`grayscale(rgb).mean()` of one (H, W, 3) uint8 image."""
    gs = grey_exact(pixels)
    return float(np.float64(numpy_sum(gs)) / np.float64(gs.size))


def fix_signs(eigvec):
    """Columns of a (3, 3) eigenvector matrix, each negated if its component of largest magnitude (lowest index on ties)
    is negative."""
    v = np.array(eigvec, dtype=np.float64)
    for j in range(v.shape[1]):
        big = int(np.argmax(np.abs(v[:, j])))         # argmax returns the first of equal maxima
        if v[big, j] < 0:
            v[:, j] = -v[:, j]
    return v


def moment_covariance(pixels):
    """Covariance of the (N, 3) channel values / 255 with N - 1 in the denominator, from exact integer moments: entry
    (a, b) = (N * S_ab - S_a * S_b) / (N * (N - 1) * 255^2), numerator and denominator exact (in a double for N <= 2^18),
    one rounding."""
    flat = np.asarray(pixels).reshape(-1, 3).astype(np.int64)
    n = flat.shape[0]
    s1 = flat.sum(axis=0)
    s2 = flat.T @ flat
    den = n * (n - 1) * 65025
    cov = np.empty((3, 3), dtype=np.float64)
    for a in range(3):
        for b in range(3):
            num = n * int(s2[a, b]) - int(s1[a]) * int(s1[b])
            cov[a, b] = float(Fraction(num, den)) if den else 0.0
    return cov


def lighting_shift(pixels, normals):
    """The per-channel shift `lighting` adds to one (H, W, 3) uint8 image for `normals` = randn(3) * std -> (3,) float64:
    ((V[k,0] * t0 + V[k,1] * t1) + V[k,2] * t2) * 255 with t = eigenvalue * normal."""
    pixels = np.asarray(pixels)
    if pixels.shape[0] * pixels.shape[1] < 2:
        return np.zeros(3, dtype=np.float64)
    eigval, eigvec = np.linalg.eigh(moment_covariance(pixels))
    eigvec = fix_signs(eigvec)
    t = eigval * np.asarray(normals, dtype=np.float64)
    return ((eigvec[:, 0] * t[0] + eigvec[:, 1] * t[1]) + eigvec[:, 2] * t[2]) * 255.0


def _to_u8(x):
    return np.clip(x, 0, 255).astype(np.uint8)


def apply_host(pixels, code, params):
    """One operation on one (H, W, 3) uint8 image -> uint8."""
    x = np.asarray(pixels)
    assert x.dtype == np.uint8 and x.ndim == 3 and x.shape[2] == 3, "expected an (H, W, 3) uint8 image"
    xf = x.astype(np.float64)
    params = np.atleast_1d(np.asarray(params, dtype=np.float64))
    a = np.float64(params[0])
    if code == SATURATION:
        return _to_u8(xf * a + ((1 - a) * grey_exact(x))[:, :, None])
    if code == BRIGHTNESS:
        return _to_u8(xf * a)
    if code == CONTRAST:
        return _to_u8(xf * a + (1 - a) * np.float64(grey_mean(x)))
    if code == LIGHTING:
        return _to_u8(xf + lighting_shift(x, params[:3]))
    raise ValueError("unknown photometric operation code %r" % (code,))


def check_ops(ops, batch):
    """Per-image operation lists -> [[(code, parameters), ...], ...] with plain ints and tuples of floats (one for alpha,
    three for lighting); ValueError for a list longer than MAX_OPS, an unknown code, a wrong number of parameters or one
    that is not finite.  What it returns passes through it unchanged."""
    ops = [list(o) for o in ops]
    if len(ops) != batch:
        raise ValueError("expected one operation list per image: %d lists for %d images" % (len(ops), batch))
    out = []
    for i, lst in enumerate(ops):
        if len(lst) > MAX_OPS:
            raise ValueError("image %d: %d operations, at most %d are supported" % (i, len(lst), MAX_OPS))
        clean = []
        for code, params in lst:
            if code not in NAMES:
                raise ValueError("image %d: unknown photometric operation code %r" % (i, code))
            p = tuple(float(v) for v in np.atleast_1d(np.asarray(params, dtype=np.float64)))
            if len(p) != (3 if code == LIGHTING else 1) or not np.isfinite(p).all():
                raise ValueError("image %d: %s takes %d finite parameter(s), got %r"
                                 % (i, NAMES[code], 3 if code == LIGHTING else 1, params))
            clean.append((int(code), p))
        out.append(clean)
    return out


def pack_ops(ops, batch=None):
    """Per-image operation lists -> the OPS_DTYPE array dj_photometric reads (unused parameters are zero)."""
    ops = check_ops(ops, len(ops) if batch is None else batch)
    arr = np.zeros(len(ops), dtype=OPS_DTYPE)
    for i, lst in enumerate(ops):
        arr["n_ops"][i] = len(lst)
        for k, (code, p) in enumerate(lst):
            arr["code"][i, k] = code
            arr["param"][i, k, :len(p)] = p
    return arr


def photometric_host(pixels_uint8, ops):
    """The (B, H, W, 3) uint8 batch (or a list of images) after each image's operation list `ops[i]` =
    [(code, parameters), ...]: parameters = alpha for saturation / brightness / contrast, the three scaled normals for
    lighting.  A test oracle: exact rationals per distinct pixel, so it is slow on large noisy images."""
    ops = check_ops(ops, len(pixels_uint8))
    out = []
    for img, lst in zip(pixels_uint8, ops):
        img = np.asarray(img)
        for code, p in lst:
            img = apply_host(img, code, p)
        out.append(np.ascontiguousarray(img))
    return np.stack(out)


def photometric_device(pixels, ops, shift_out=False, stream=None):
    """`photometric_host` on the GPU for callers outside `Model`: `pixels` a (B, H, W, 3) uint8 CUDA tensor, modified in
    place and returned (with the (B, 3) float64 tensor of applied lighting shifts when `shift_out`).  Uploads the lists
    and waits for the kernel: the staging buffer goes away with this frame."""
    import torch

    from .. import kernels
    arr = pack_ops(ops, pixels.shape[0])
    ops_dev = torch.from_numpy(arr.view(np.uint8).reshape(-1)).to(pixels.device)
    shifts = torch.zeros((pixels.shape[0], 3), dtype=torch.float64, device=pixels.device) if shift_out else None
    kernels.photometric(pixels, ops_dev, arr, shift_out=shifts, stream=stream)
    (torch.cuda.current_stream(pixels.device) if stream is None else torch.cuda.ExternalStream(stream)).synchronize()
    return (pixels, shifts) if shift_out else pixels
