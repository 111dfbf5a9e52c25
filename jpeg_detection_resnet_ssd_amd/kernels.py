"""Tensor-level wrappers over the C ABI (include/dj_hip.h): they take torch CUDA tensors,
validate layout on the host, and launch on torch's current HIP stream.  No arithmetic
happens here and there is no fallback path."""
import math

import torch

from . import _lib
from ._lib import ConvDesc, check, ptr


import threading

_tls = threading.local()      # .recorder: set while `bound` captures a wrapper's C-ABI calls instead of launching them


def _stream():
    return _lib.current_stream()


class _Recorder(object):
    """Stands in for the library while a wrapper runs in capture mode: every entry point it would launch is noted with
    its converted arguments (the trailing stream argument dropped) and reports success."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def note(*args):
            self.calls.append((name, args[:-1]))
            return 0
        return note


def _L():
    rec = getattr(_tls, "recorder", None)
    return rec if rec is not None else _lib.load()


def bound(name, *args, ws=None, **kwargs):
    """-> a launcher for `kernels.<name>(*args, **kwargs[, workspace=ws.buf])` whose layout checks, descriptor copy and
    pointer conversions are done ONCE: the wrapper runs in capture mode the first time (and again if the workspace buffer
    was replaced), afterwards a launch is the recorded C-ABI call(s) with the current stream appended.  Plan buffers never
    move, so nothing else can go stale.  (Per conv launch the wrapper costs ~20 us of host time, ~4 ms per training step;
    the float16 step is 11 ms.)  A wrapper that a test or a profiler has replaced in this module is called through."""
    orig = globals()[name]
    state = [None, None]

    def run():
        f = globals()[name]
        wsb = ws.buf if ws is not None else None
        if f is not orig:
            return f(*args, **kwargs, **({"workspace": wsb} if ws is not None else {}))
        if state[0] is None or state[1] is not wsb:
            rec = _Recorder()
            _tls.recorder = rec
            try:
                orig(*args, **kwargs, **({"workspace": wsb} if ws is not None else {}))
            finally:
                _tls.recorder = None
            lib = _lib.load()
            state[0] = [(getattr(lib, n), a, n) for n, a in rec.calls]
            state[1] = wsb
        s = _lib.current_stream()
        for fn, a, n in state[0]:
            check(fn(*a, s), n)
    run.wrapper = name
    return run


# storage-type codes of include/dj_hip.h (DJ_F32 / DJ_F16 / DJ_BF16)
DT_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def dt_of(t):
    """Storage-type code of a tensor (None -> DJ_F32)."""
    return 0 if t is None else DT_CODE[t.dtype]


def any16(*tensors):
    """True when one of the tensors is held in 16 bits: an elementwise launch then goes through a `_t` entry point."""
    return any(t is not None and t.dtype != torch.float32 for t in tensors)


def _pixel_ld(t):
    """Pixel stride (elements) of an NHWC tensor that may be a channel slice of a wider buffer."""
    assert t.dim() == 4 and t.dtype in DT_CODE and t.is_cuda, "expected a float32 / float16 / bfloat16 CUDA NHWC tensor"
    b, h, w, c = t.shape
    ld = t.stride(2) if w > 1 else (t.stride(1) if h > 1 else (t.stride(0) if b > 1 else c))
    assert t.stride(3) == 1 or c == 1, "channels must be contiguous"
    assert ld >= c
    if w > 1:
        assert t.stride(2) == ld
    if h > 1:
        assert t.stride(1) == w * ld, "rows must be dense"
    if b > 1:
        assert t.stride(0) == h * w * ld, "images must be dense"
    return ld


def same_padding(in_size, kernel, stride, dilation=1):
    """TensorFlow 'SAME' rule -> (pad_before, pad_after, out_size)."""
    out = -(-in_size // stride)
    total = max((out - 1) * stride + (kernel - 1) * dilation + 1 - in_size, 0)
    return total // 2, total - total // 2, out


def conv_geometry(in_h, in_w, kernel, strides, padding, dilation):
    """Resolve Keras `padding` into explicit pads and the output size.
    `padding` is 'valid', 'same' or ((top, bottom), (left, right)) (ZeroPadding2D folded in)."""
    kh, kw = kernel
    sh, sw = strides
    dh, dw = dilation
    if padding == "same":
        pt, _, oh = same_padding(in_h, kh, sh, dh)
        pl, _, ow = same_padding(in_w, kw, sw, dw)
    else:
        if padding == "valid":
            (pt, pb), (pl, pr) = (0, 0), (0, 0)
        else:
            (pt, pb), (pl, pr) = padding
        oh = (in_h + pt + pb - (kh - 1) * dh - 1) // sh + 1
        ow = (in_w + pl + pr - (kw - 1) * dw - 1) // sw + 1
    return pt, pl, oh, ow


def make_conv_desc(batch, in_h, in_w, in_c, out_c, kernel, strides=(1, 1), padding="valid", dilation=(1, 1),
                   ld_x=None, ld_y=None):
    pt, pl, oh, ow = conv_geometry(in_h, in_w, kernel, strides, padding, dilation)
    return ConvDesc(batch, in_h, in_w, in_c, oh, ow, out_c, kernel[0], kernel[1], strides[0], strides[1],
                    dilation[0], dilation[1], pt, pl, ld_x or in_c, ld_y or out_c)


def _desc_for(desc, x, y):
    d = ConvDesc()
    for name, _ in ConvDesc._fields_:
        setattr(d, name, getattr(desc, name))
    if x is not None:
        d.ld_x = _pixel_ld(x)
        assert tuple(x.shape) == (d.batch, d.in_h, d.in_w, d.in_c), (tuple(x.shape), "vs desc")
    if y is not None:
        d.ld_y = _pixel_ld(y)
        assert tuple(y.shape) == (d.batch, d.out_h, d.out_w, d.out_c), (tuple(y.shape), "vs desc")
    return d


def conv2d_stats_rows(desc):
    return check(_lib.load().dj_conv2d_fwd_stats_rows(desc), "dj_conv2d_fwd_stats_rows")


def _weights_ok(w, d):
    return w.is_contiguous() and tuple(w.shape) == (d.kernel_h, d.kernel_w, d.in_c, d.out_c)


def _fwd(d, a, x, w, bias, y, pro_scale, pro_shift, stats, workspace):
    """Fill the fields every forward launch has and make the call."""
    assert _weights_ok(w, d)
    a.x, a.dt_x, a.w, a.dt_w, a.bias, a.y, a.dt_y = ptr(x), dt_of(x), ptr(w), dt_of(w), ptr(bias), ptr(y), dt_of(y)
    a.pro_scale, a.pro_shift, a.stats = ptr(pro_scale), ptr(pro_shift), ptr(stats)
    if workspace is not None:
        a.workspace, a.workspace_floats = ptr(workspace), workspace.numel()
    check(_L().dj_conv2d_nhwc_fwd(d, a, _stream()), "dj_conv2d_nhwc_fwd")
    return y


def _residual(a, x, res, res_scale, res_shift, sum_out):
    assert tuple(res.shape) == tuple(x.shape) and (sum_out is None or tuple(sum_out.shape) == tuple(x.shape))
    assert res.dtype == x.dtype, "the residual operand is read like x: same storage type"
    a.res, a.ld_res, a.res_scale, a.res_shift = ptr(res), _pixel_ld(res), ptr(res_scale), ptr(res_shift)
    if sum_out is not None:
        a.sum_out, a.ld_sum, a.dt_sum = ptr(sum_out), _pixel_ld(sum_out), dt_of(sum_out)


def conv2d_fwd(desc, x, w, bias, y, pro_scale=None, pro_shift=None, pro_relu=False, relu=False, stats=None,
               y_zeroed=False, workspace=None, stats_may_split=False):
    """`y_zeroed`: y is all zeros on entry (a split-K launch then skips its own memset).
    `workspace` (float tensor): split-K launches go through slabs + a fixed-order reduction (bit-reproducible) when it is
    large enough (conv2d_fwd_workspace_floats); `stats_may_split`: a launch with `stats` may then be split too."""
    a = _lib.ConvFwdArgs(pro_relu=int(pro_relu), flags=int(bool(relu)) | (2 if y_zeroed else 0) | (4 if stats_may_split else 0))
    return _fwd(_desc_for(desc, x, y), a, x, w, bias, y, pro_scale, pro_shift, stats, workspace)


def conv2d_fwd_workspace_floats(desc, stats_may_split=False):
    return check(_lib.load().dj_conv2d_fwd_workspace_floats(desc, int(stats_may_split)), "dj_conv2d_fwd_workspace_floats")


def conv2d_fwd_addrelu_supported(desc):
    return bool(_lib.load().dj_conv2d_fwd_addrelu_supported(desc))


def conv2d_fwd_addrelu(desc, x, w, bias, y, pro_scale, pro_shift, res, res_scale=None, res_shift=None, sum_out=None,
                       relu=False, stats=None, workspace=None):
    """1x1 stride-1 conv of relu(x*pro_scale+pro_shift + res*res_scale+res_shift); `sum_out` receives that input.
    `workspace`: as for conv2d_fwd."""
    a = _lib.ConvFwdArgs(pro_relu=1, flags=int(bool(relu)))
    _residual(a, x, res, res_scale, res_shift, sum_out)
    return _fwd(_desc_for(desc, x, y), a, x, w, bias, y, pro_scale, pro_shift, stats, workspace)


def _dgrad(desc, a, dy, w, bias, dx):
    d = _desc_for(desc, dx, dy)
    assert _weights_ok(w, d)
    a.dy, a.dt_dy, a.w, a.dt_w, a.bias, a.dx, a.dt_dx = ptr(dy), dt_of(dy), ptr(w), dt_of(w), ptr(bias), ptr(dx), dt_of(dx)
    check(_L().dj_conv2d_nhwc_dgrad(d, a, _stream()), "dj_conv2d_nhwc_dgrad")
    return dx


def _dgrad_relumask(desc, dy, w, dx, relu_mask, bias, beta):
    assert not any16(dy, dx, w, relu_mask), "conv2d_dgrad(relu_mask=...): every tensor must be torch.float32"
    assert tuple(relu_mask.shape) == tuple(dx.shape)
    a = _lib.ConvDgradArgs(flags=int(bool(beta)), mask_x=ptr(relu_mask), ld_mask=_pixel_ld(relu_mask))
    return _dgrad(desc, a, dy, w, bias, dx)


def conv2d_dgrad_relumask_supported(desc):
    return bool(_lib.load().dj_conv2d_dgrad_relumask_supported(desc))


def conv2d_dgrad(desc, dy, w, dx, bias=None, beta=False, no_split=False, relu_mask=None):
    """`no_split`: one K range per tile (no fp32 atomics): for the forward use as Conv2DTranspose.
    `relu_mask` (a tensor shaped like dx: the convolution's forward input x = relu(...)): the epilogue stores
    `relu_mask > 0 ? value : 0` -- the input gradient and the ReLU backward of x in one launch
    (dj_conv_dgrad_args.mask_x; fp32 tensors, one K range)."""
    if relu_mask is not None:
        return _dgrad_relumask(desc, dy, w, dx, relu_mask, bias, beta)
    return _dgrad(desc, _lib.ConvDgradArgs(flags=int(bool(beta)) | (2 if no_split else 0)), dy, w, bias, dx)


def conv2d_dgrad_relumask(desc, dy, w, dx, relu_mask, bias=None, beta=False):
    """conv2d_dgrad(..., relu_mask=relu_mask) under a name of its own, for the training plan (keras/layers.py): whoever
    replaces `conv2d_dgrad` in this module to time or to check the plan's launches (`bound` calls a replaced wrapper through)
    may rely on that name computing the plain input gradient, dx (+)= conv_transpose(dy, w) -- tests/test_replay_gpu.py
    compares every such launch with exactly that."""
    return _dgrad_relumask(desc, dy, w, dx, relu_mask, bias, beta)


def conv2d_dgrad_bnbwd(desc, dy, w, dx, z, mean, invstd, scale, shift, partial):
    """Input gradient + BatchNormalization backward statistics of dx in the same launch (dj_conv_dgrad_args.partial):
    `partial` [ceil(rows / 64)][2][in_c] receives what dj_bn_bwd_reduce would compute from (dx, z)."""
    assert tuple(z.shape) == tuple(dx.shape)
    rows = desc.batch * desc.in_h * desc.in_w
    assert partial.is_contiguous() and tuple(partial.shape) == ((rows + 63) // 64, 2, desc.in_c)
    a = _lib.ConvDgradArgs(flags=2, z=ptr(z), ld_z=_pixel_ld(z), dt_z=dt_of(z), mean=ptr(mean), invstd=ptr(invstd),
                           scale=ptr(scale), shift=ptr(shift), partial=ptr(partial))
    return _dgrad(desc, a, dy, w, None, dx)


def conv2d_wgrad(desc, x, dy, dw, pro_scale=None, pro_shift=None, pro_relu=False, dw_zeroed=False):
    d = _desc_for(desc, x, dy)
    assert _weights_ok(dw, d)
    a = _lib.ConvWgradArgs(ptr(x), dt_of(x), ptr(dy), dt_of(dy), ptr(dw), ptr(pro_scale), ptr(pro_shift), int(pro_relu),
                           int(dw_zeroed))
    check(_L().dj_conv2d_nhwc_wgrad(d, a, _stream()), "dj_conv2d_nhwc_wgrad")
    return dw


# ---- elementwise passes that exist in a float and a typed (`_t`) form ---------------------------------------------------
# -> (entry point, arguments...) for engine.call, chosen by the storage types of the tensors involved
def affine_act_call(x, ldx, scale, shift, res, ldres, res_scale, res_shift, y, ldy, rows, c, relu):
    """y = act(x*scale+shift [+ res*res_scale+res_shift])."""
    if any16(x, res, y):
        return ("dj_affine_act_t", x, dt_of(x), int(ldx), scale, shift, res, dt_of(res), int(ldres), res_scale, res_shift, y,
                dt_of(y), int(ldy), int(rows), int(c), int(relu))
    return ("dj_affine_act", x, int(ldx), scale, shift, res, int(ldres), res_scale, res_shift, y, int(ldy), int(rows), int(c),
            int(relu))


def relu_bwd_call(dy, ld_dy, y, ld_y, dx, ld_dx, rows, c, beta):
    if any16(dy, y, dx):
        return ("dj_relu_bwd_t", dy, dt_of(dy), int(ld_dy), y, dt_of(y), int(ld_y), dx, dt_of(dx), int(ld_dx), int(rows), int(c),
                int(beta))
    return ("dj_relu_bwd", dy, int(ld_dy), y, int(ld_y), dx, int(ld_dx), int(rows), int(c), int(beta))


def copy2d_call(src, ld_src, dst, ld_dst, rows, cols, beta):
    if any16(src, dst):
        return ("dj_copy2d_t", src, dt_of(src), int(ld_src), dst, dt_of(dst), int(ld_dst), int(rows), int(cols), int(beta))
    return ("dj_copy2d", src, int(ld_src), dst, int(ld_dst), int(rows), int(cols), int(beta))


def bn_bwd_reduce_call(dy, ld_dy, z, ld_z, mask_y, ld_y, mean, invstd, scale, shift, mode, rows, c, part):
    if any16(dy, z, mask_y):
        return ("dj_bn_bwd_reduce_t", dy, dt_of(dy), int(ld_dy), z, dt_of(z), int(ld_z), mask_y, dt_of(mask_y), int(ld_y), mean,
                invstd, scale, shift, int(mode), int(rows), int(c), part)
    return ("dj_bn_bwd_reduce", dy, int(ld_dy), z, int(ld_z), mask_y, int(ld_y), mean, invstd, scale, shift, int(mode), int(rows),
            int(c), part)


def bn_bwd_apply_call(dy, ld_dy, z, ld_z, mask_y, ld_y, scale, shift, mode, k0, k1, k2, dz, ld_dz, rows, c, dm, ld_dm, dm_beta):
    if any16(dy, z, mask_y, dz, dm):
        return ("dj_bn_bwd_apply_t", dy, dt_of(dy), int(ld_dy), z, dt_of(z), int(ld_z), mask_y, dt_of(mask_y), int(ld_y), scale,
                shift, int(mode), k0, k1, k2, dz, dt_of(dz), int(ld_dz), int(rows), int(c), dm, dt_of(dm), int(ld_dm),
                int(dm_beta))
    return ("dj_bn_bwd_apply", dy, int(ld_dy), z, int(ld_z), mask_y, int(ld_y), scale, shift, int(mode), k0, k1, k2, dz,
            int(ld_dz), int(rows), int(c), dm, int(ld_dm), int(dm_beta))


# ---- RGB batch -> JPEG DCT coefficient tensors ------------------------------------------------------------------------------
def _table_u16(table, what):
    import ctypes
    import numpy as np
    t = np.ascontiguousarray(np.asarray(table).reshape(-1))
    if t.size != 64 or (t != np.floor(t)).any() or t.min() < 0 or t.max() > 65535:
        raise ValueError("%s quantisation table: expected 64 integer entries in natural order" % what)
    return (ctypes.c_ushort * 64)(*[int(v) for v in t])


def rgb_to_dct(rgb_u8, tables, outs, normalized=True, stream=None):
    """(B, H, W, 3) uint8 CUDA tensor -> the de-quantised DCT coefficients of its baseline 4:2:0 JPEG, written into
    `outs` = (y, cb, cr): float32 NHWC block tensors (B, ceil(H/8), ceil(W/8), 64) and twice (B, ceil(ceil(H/2)/8),
    ceil(ceil(W/2)/8), 64), each of which may be a 64-channel slice of a wider buffer.  `tables` = (luma, chroma), 64
    entries each in natural order (data/jpeg_dct.py:quant_tables).  `stream`: a HIP stream handle (None: the current
    launch stream)."""
    assert rgb_u8.is_cuda and rgb_u8.dtype == torch.uint8 and rgb_u8.dim() == 4 and rgb_u8.shape[3] == 3, \
        "expected a (B, H, W, 3) uint8 CUDA tensor"
    b, h, w, _ = rgb_u8.shape
    assert rgb_u8.stride(3) == 1 and rgb_u8.stride(2) == 3, "pixels must be packed RGB"
    stride = rgb_u8.stride(1) if h > 1 else 3 * w
    assert b == 1 or rgb_u8.stride(0) == h * stride, "images must be dense"
    y, cb, cr = outs
    yg = (-(-h // 8), -(-w // 8))
    cg = (-(-(-(-h // 2)) // 8), -(-(-(-w // 2)) // 8))
    for t, g, name in ((y, yg, "y"), (cb, cg, "cb"), (cr, cg, "cr")):
        assert t.dtype == torch.float32 and tuple(t.shape) == (b,) + g + (64,), \
            "%s: expected float32 %s, got %s %s" % (name, (b,) + g + (64,), t.dtype, tuple(t.shape))
    luma, chroma = tables
    check(_L().dj_rgb_to_dct(ptr(rgb_u8), b, h, w, stride, _table_u16(luma, "luma"), _table_u16(chroma, "chroma"),
                             int(bool(normalized)), ptr(y), _pixel_ld(y), ptr(cb), _pixel_ld(cb), ptr(cr), _pixel_ld(cr),
                             stream if stream is not None else _stream()), "dj_rgb_to_dct")
    return outs


# ---- the staged blobs of data/device_staging.py ------------------------------------------------------------------------------
def _check_staged(desc_host, dtype, struct, desc_dev, bytes_1d, pool=None):
    """What dj_image_prep, dj_patch_resize and dj_ssd_photometric take of a staged blob: `desc_host` a numpy array of
    `dtype` (laid out as the ctypes `struct`), `desc_dev` its bytes on the device, `bytes_1d` the other 1-D uint8 CUDA
    tensors as (tensor, name) pairs and `pool` = (pool_dev, pool_host) where the entry point reads one -> the batch size."""
    import ctypes
    import numpy as np
    assert dtype.itemsize == ctypes.sizeof(struct), "descriptor layouts disagree"
    assert isinstance(desc_host, np.ndarray) and desc_host.dtype == dtype and desc_host.ndim == 1 \
        and desc_host.flags.c_contiguous, "desc_host: expected a contiguous 1-D array of DESC_DTYPE"
    if pool is not None:
        assert isinstance(pool[1], np.ndarray) and pool[1].dtype == np.int32 and pool[1].ndim == 1 \
            and pool[1].flags.c_contiguous, "pool_host: expected a contiguous 1-D int32 array"
    for t, name in bytes_1d:
        assert t.is_cuda and t.dtype == torch.uint8 and t.dim() == 1 and t.is_contiguous(), \
            "%s: expected a contiguous 1-D uint8 CUDA tensor" % name
    assert desc_dev.numel() >= desc_host.nbytes and desc_dev.data_ptr() % 8 == 0, "desc_dev: too small or misaligned"
    if pool is not None:
        assert pool[0].is_cuda and pool[0].dtype == torch.int32 and pool[0].dim() == 1 and pool[0].is_contiguous() \
            and pool[0].numel() >= pool[1].size, "pool_dev: expected a contiguous 1-D int32 CUDA tensor of the pool's size"
    return desc_host.shape[0]


def _packed_rgb_stride(t, what=""):
    """Row pitch in bytes of a (B, H, W, 3) uint8 tensor of packed RGB pixels whose rows may be strided (images dense)."""
    b, h, w, _ = t.shape
    assert t.stride(3) == 1 and (w == 1 or t.stride(2) == 3), what + "pixels must be packed RGB"
    stride = t.stride(1) if h > 1 else (t.stride(0) if b > 1 else 3 * w)      # one row per image: its pitch is the image pitch
    assert stride >= 3 * w and (b == 1 or t.stride(0) == h * stride), what + "images must be dense"
    return stride


# ---- ragged batch of decoded images -> resized, cropped, flipped uint8 batch -------------------------------------------------
def image_prep(src, desc_dev, desc_host, pool_dev, pool_host, target, out, scratch, stream=None):
    """dj_image_prep: `src` 1-D uint8 CUDA tensor holding the source images, `desc_dev` the descriptors' bytes on the
    device and `desc_host` the same descriptors as a numpy array of data/image_prep.py:DESC_DTYPE, `pool_dev` / `pool_host`
    the int32 bounds-and-taps pool as a CUDA tensor and as a numpy array, `out` a (B, target, target, 3) uint8 CUDA tensor
    whose rows may be strided (images dense), `scratch` a 1-D uint8 CUDA tensor of at least `image_prep_scratch_bytes`
    laid out as the descriptors say.  `stream`: a HIP stream handle (None: the current launch stream)."""
    from ._lib import ImagePrepDesc
    from .data.image_prep import DESC_DTYPE
    b = _check_staged(desc_host, DESC_DTYPE, ImagePrepDesc, desc_dev, ((src, "src"), (desc_dev, "desc_dev"), (scratch, "scratch")),
                      (pool_dev, pool_host))
    target = int(target)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (b, target, target, 3), \
        "out: expected uint8 %s, got %s %s" % ((b, target, target, 3), out.dtype, tuple(out.shape))
    stride = _packed_rgb_stride(out, "out: ")
    check(_L().dj_image_prep(ptr(src), src.numel(), ptr(desc_dev), desc_host.ctypes.data, b, ptr(pool_dev),
                             pool_host.ctypes.data, pool_host.size, target, ptr(out), stride, ptr(scratch), scratch.numel(),
                             stream if stream is not None else _stream()), "dj_image_prep")
    return out


def image_prep_scratch_bytes(desc_host, target):
    """Bytes of scratch dj_image_prep needs when every image's region is rounded up to 64 bytes."""
    return check(_L().dj_image_prep_scratch_bytes(desc_host.ctypes.data, desc_host.shape[0], int(target)),
                 "dj_image_prep_scratch_bytes")


# ---- photometric augmentation of a uint8 batch, in place ---------------------------------------------------------------------
def photometric(pixels, ops_dev, ops_host, shift_out=None, stream=None):
    """dj_photometric: `pixels` a (B, H, W, 3) uint8 CUDA tensor whose rows may be strided (images dense), modified in
    place; `ops_dev` the per-image operation lists' bytes on the device (1-D uint8) and `ops_host` the same lists as a
    numpy array of data/photometric.py:OPS_DTYPE; `shift_out` an optional contiguous (B, 3) float64 CUDA tensor that
    receives the lighting shifts applied.  `stream`: a HIP stream handle (None: the current launch stream)."""
    import ctypes
    import numpy as np
    from ._lib import PhotometricOps
    from .data.photometric import OPS_DTYPE
    assert OPS_DTYPE.itemsize == ctypes.sizeof(PhotometricOps), "operation-list layouts disagree"
    assert pixels.is_cuda and pixels.dtype == torch.uint8 and pixels.dim() == 4 and pixels.shape[3] == 3, \
        "expected a (B, H, W, 3) uint8 CUDA tensor"
    b, h, w, _ = pixels.shape
    assert isinstance(ops_host, np.ndarray) and ops_host.dtype == OPS_DTYPE and ops_host.shape == (b,) \
        and ops_host.flags.c_contiguous, "ops_host: expected a contiguous array of one OPS_DTYPE entry per image"
    assert ops_dev.is_cuda and ops_dev.dtype == torch.uint8 and ops_dev.dim() == 1 and ops_dev.is_contiguous() \
        and ops_dev.numel() >= ops_host.nbytes and ops_dev.data_ptr() % 8 == 0, \
        "ops_dev: expected a contiguous, 8-byte aligned 1-D uint8 CUDA tensor of the lists' size"
    stride = _packed_rgb_stride(pixels)
    if shift_out is not None:
        assert shift_out.is_cuda and shift_out.dtype == torch.float64 and tuple(shift_out.shape) == (b, 3) \
            and shift_out.is_contiguous(), "shift_out: expected a contiguous (B, 3) float64 CUDA tensor"
    check(_L().dj_photometric(ptr(pixels), b, h, w, stride, ptr(ops_dev), ops_host.ctypes.data, ptr(shift_out),
                              stream if stream is not None else _stream()), "dj_photometric")
    return pixels


# ---- Keras' ImageDataGenerator on a uint8 batch: affine warp, flips, standardisation -> float32 NHWC -------------------------
def rgb_warp(pixels, rec_dev, rec_host, out, preprocess=0, rescale=None, stream=None):
    """dj_rgb_warp: `pixels` a contiguous (B, H, W, 3) uint8 CUDA tensor; `rec_dev` the per-image records' bytes on the
    device (1-D uint8) and `rec_host` the same records as a numpy array of data/rgb_warp.py:RECORD_DTYPE; `out` a
    (B, H, W, 3) float32 CUDA tensor whose rows may be strided (images dense); `preprocess` 0 (none) or 1 (caffe: BGR and
    mean); `rescale` None or the float32 factor.  `stream`: a HIP stream handle (None: the current launch stream)."""
    import ctypes
    import numpy as np
    from ._lib import RgbWarpRecord
    from .data.rgb_warp import RECORD_DTYPE
    assert RECORD_DTYPE.itemsize == ctypes.sizeof(RgbWarpRecord), "record layouts disagree"
    assert pixels.is_cuda and pixels.dtype == torch.uint8 and pixels.dim() == 4 and pixels.shape[3] == 3 \
        and pixels.is_contiguous(), "pixels: expected a contiguous (B, H, W, 3) uint8 CUDA tensor"
    b, h, w, _ = pixels.shape
    assert isinstance(rec_host, np.ndarray) and rec_host.dtype == RECORD_DTYPE and rec_host.shape == (b,) \
        and rec_host.flags.c_contiguous, "rec_host: expected a contiguous array of one RECORD_DTYPE entry per image"
    assert rec_dev.is_cuda and rec_dev.dtype == torch.uint8 and rec_dev.dim() == 1 and rec_dev.is_contiguous() \
        and rec_dev.numel() >= rec_host.nbytes and rec_dev.data_ptr() % 8 == 0, \
        "rec_dev: expected a contiguous, 8-byte aligned 1-D uint8 CUDA tensor of the records' size"
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (b, h, w, 3), \
        "out: expected float32 %s, got %s %s" % ((b, h, w, 3), out.dtype, tuple(out.shape))
    stride = _packed_rgb_stride(out, "out: ")
    check(_L().dj_rgb_warp(ptr(pixels), b, h, w, ptr(rec_dev), rec_host.ctypes.data, int(preprocess),
                           int(rescale is not None), float(rescale) if rescale is not None else 1.0, ptr(out), stride,
                           stream if stream is not None else _stream()), "dj_rgb_warp")
    return out


# ---- ragged batch of decoded images -> a window of each on a background, mirrored, resized -----------------------------------
def patch_resize(src, desc_dev, desc_host, pool_dev, pool_host, out, scratch, stream=None):
    """dj_patch_resize: `src` 1-D uint8 CUDA tensor holding the staged rectangles, `desc_dev` the descriptors' bytes on the
    device and `desc_host` the same descriptors as a numpy array of data/patch_resize.py:DESC_DTYPE, `pool_dev` /
    `pool_host` the int32 bounds-and-taps pool as a CUDA tensor and as a numpy array, `out` a (B, out_h, out_w, 3) uint8
    CUDA tensor whose rows may be strided (images dense), `scratch` a 1-D uint8 CUDA tensor of at least
    `patch_resize_scratch_bytes` laid out as the descriptors say.  `stream`: a HIP stream handle (None: the current launch
    stream)."""
    from ._lib import PatchResizeDesc
    from .data.patch_resize import DESC_DTYPE
    b = _check_staged(desc_host, DESC_DTYPE, PatchResizeDesc, desc_dev, ((src, "src"), (desc_dev, "desc_dev"), (scratch, "scratch")),
                      (pool_dev, pool_host))
    assert out.is_cuda and out.dtype == torch.uint8 and out.dim() == 4 and out.shape[0] == b and out.shape[3] == 3, \
        "out: expected a (%d, out_h, out_w, 3) uint8 CUDA tensor, got %s %s" % (b, out.dtype, tuple(out.shape))
    out_h, out_w = int(out.shape[1]), int(out.shape[2])
    stride = _packed_rgb_stride(out, "out: ")
    check(_L().dj_patch_resize(ptr(src), src.numel(), ptr(desc_dev), desc_host.ctypes.data, b, ptr(pool_dev),
                               pool_host.ctypes.data, pool_host.size, out_h, out_w, ptr(out), stride, ptr(scratch),
                               scratch.numel(), stream if stream is not None else _stream()), "dj_patch_resize")
    return out


def patch_resize_scratch_bytes(desc_host, out_w):
    """Bytes of scratch dj_patch_resize needs when every image's region is rounded up to 64 bytes."""
    return check(_L().dj_patch_resize_scratch_bytes(desc_host.ctypes.data, desc_host.shape[0], int(out_w)),
                 "dj_patch_resize_scratch_bytes")


# ---- the photometric stage of the SSD augmentation chain, in place on the staged rectangles ----------------------------------
def ssd_photometric(src, desc_dev, desc_host, params_dev, params_host, stream=None):
    """dj_ssd_photometric: `src` the 1-D uint8 CUDA tensor holding the staged rectangles that dj_patch_resize will read,
    modified in place; `desc_dev` / `desc_host` the descriptors as for `patch_resize`; `params_dev` the per-image records'
    bytes on the device (1-D uint8) and `params_host` the same records as a numpy array of
    data/ssd_photometric.py:PARAMS_DTYPE.  `stream`: a HIP stream handle (None: the current launch stream)."""
    import ctypes
    import numpy as np
    from ._lib import PatchResizeDesc, SsdPhotoParams
    from .data.patch_resize import DESC_DTYPE
    from .data.ssd_photometric import PARAMS_DTYPE
    b = _check_staged(desc_host, DESC_DTYPE, PatchResizeDesc, desc_dev, ((src, "src"), (desc_dev, "desc_dev"), (params_dev, "params_dev")))
    assert PARAMS_DTYPE.itemsize == ctypes.sizeof(SsdPhotoParams), "parameter-record layouts disagree"
    assert isinstance(params_host, np.ndarray) and params_host.dtype == PARAMS_DTYPE and params_host.shape == (b,) \
        and params_host.flags.c_contiguous, "params_host: expected a contiguous array of one PARAMS_DTYPE record per image"
    assert params_dev.numel() >= params_host.nbytes and params_dev.data_ptr() % 4 == 0, "params_dev: too small or misaligned"
    check(_L().dj_ssd_photometric(ptr(src), src.numel(), ptr(desc_dev), desc_host.ctypes.data, ptr(params_dev),
                                  params_host.ctypes.data, b, stream if stream is not None else _stream()),
          "dj_ssd_photometric")
    return src


# ---- JPEG pixels from entropy-decoded coefficients, into the staged rectangles ------------------------------------------------
def jpeg_pixels(coef, desc_dev, desc_host, tables_dev, tables_host, dst, scratch, stream=None):
    """dj_jpeg_pixels: `coef` the 1-D uint8 CUDA tensor holding the raw int16 coefficient planes, `desc_dev` the decode
    descriptors' bytes on the device and `desc_host` the same as a numpy array of data/device_staging.py:DECODE_DTYPE,
    `tables_dev` the quantisation tables' bytes on the device (1-D uint8) and `tables_host` the same as an int32 numpy
    array (only its size is read), `dst` the 1-D uint8 CUDA tensor of staged pixels the rectangles are written into,
    `scratch` a 1-D uint8 CUDA tensor holding the sample planes where the descriptors say.  `stream`: a HIP stream handle
    (None: the current launch stream)."""
    import numpy as np
    from ._lib import JpegPixelsDesc
    from .data.device_staging import DECODE_DTYPE
    n = _check_staged(desc_host, DECODE_DTYPE, JpegPixelsDesc, desc_dev,
                      ((coef, "coef"), (desc_dev, "desc_dev"), (tables_dev, "tables_dev"), (dst, "dst"), (scratch, "scratch")))
    assert isinstance(tables_host, np.ndarray) and tables_host.dtype == np.int32, "tables_host: expected an int32 array"
    assert tables_dev.numel() >= tables_host.nbytes, "tables_dev: smaller than the tables"
    check(_L().dj_jpeg_pixels(ptr(coef), coef.numel(), ptr(desc_dev), desc_host.ctypes.data, n, ptr(tables_dev),
                              tables_host.size, ptr(dst), dst.numel(), ptr(scratch), scratch.numel(),
                              stream if stream is not None else _stream()), "dj_jpeg_pixels")
    return dst


# ---- the DCT input tensors from the files' own coefficients: window, mirror, de-quantise, scatter ----------------------------
def _block_stride(t, name, n, rows, cols):
    """(floats between the blocks of a (n, rows, cols, 64) float32 view, floats that may be written from its first
    element): blocks equally spaced in (image, row, column) order, 64 contiguous floats each."""
    assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (n, rows, cols, 64), \
        "%s: expected float32 %s, got %s %s" % (name, (n, rows, cols, 64), t.dtype, tuple(t.shape))
    ld = t.stride(2) if cols > 1 else (t.stride(1) if rows > 1 else (t.stride(0) if n > 1 else 64))
    assert t.stride(3) == 1 and ld >= 64 and (cols == 1 or t.stride(2) == ld) and (rows == 1 or t.stride(1) == cols * ld) \
        and (n == 1 or t.stride(0) == rows * cols * ld), "%s: blocks must be dense and equally spaced" % name
    return ld, t.untyped_storage().nbytes() // 4 - t.storage_offset()


def jpeg_dct_inputs(coef, desc_dev, desc_host, tables_dev, tables_host, outs, stream=None):
    """dj_jpeg_dct_inputs: `coef` the 1-D uint8 CUDA tensor holding the raw int16 coefficient planes, `desc_dev` the
    descriptors' bytes on the device and `desc_host` the same as a numpy array of data/coefficient_inputs.py:DESC_DTYPE,
    `tables_dev` the quantisation tables' bytes on the device (1-D uint8) and `tables_host` the same as an int32 numpy
    array (only its size is read), `outs` = (Y, Cb, Cr): float32 CUDA views of (n, yh, yw, 64) and twice (n, ch, cw, 64)
    whose blocks may be strided (Cb and Cr may be the halves of one 128-channel tensor).  Every element of the three is
    written.  `stream`: a HIP stream handle (None: the current launch stream)."""
    import numpy as np
    from ._lib import JpegDctDesc
    from .data.coefficient_inputs import DESC_DTYPE
    n = _check_staged(desc_host, DESC_DTYPE, JpegDctDesc, desc_dev,
                      ((coef, "coef"), (desc_dev, "desc_dev"), (tables_dev, "tables_dev")))
    assert isinstance(tables_host, np.ndarray) and tables_host.dtype == np.int32, "tables_host: expected an int32 array"
    assert tables_dev.numel() >= tables_host.nbytes, "tables_dev: smaller than the tables"
    y, cb, cr = outs
    assert y.dim() == 4 and cb.dim() == 4 and tuple(cb.shape) == tuple(cr.shape), "outs: expected (Y, Cb, Cr) block tensors"
    (yh, yw), (ch, cw) = y.shape[1:3], cb.shape[1:3]
    args = []
    for t, name, rows, cols in ((y, "Y", yh, yw), (cb, "Cb", ch, cw), (cr, "Cr", ch, cw)):
        ld, floats = _block_stride(t, name, n, rows, cols)
        args += [ptr(t), ld, floats]
    check(_L().dj_jpeg_dct_inputs(ptr(coef), coef.numel(), ptr(desc_dev), desc_host.ctypes.data, n, ptr(tables_dev),
                                  tables_host.size, yh, yw, ch, cw, *args, stream if stream is not None else _stream()),
          "dj_jpeg_dct_inputs")
    return outs


# ---- Huffman entropy decoding of restart-interval files: one lane per restart interval -----------------------------------------
def jpeg_entropy_decode(data, desc_dev, desc_host, seg_dev, seg_host, tables_dev, tables_host, out, status, stream=None):
    """dj_jpeg_entropy_decode: `data` the 1-D uint8 CUDA tensor holding the files' bytes, `desc_dev` / `seg_dev` the file
    descriptors' and segment records' bytes on the device and `desc_host` / `seg_host` the same as numpy arrays of
    data/coefficient_inputs.py:ENTROPY_DTYPE / SEGMENT_DTYPE, `tables_dev` the Huffman tables' bytes on the device (1-D
    uint8) and `tables_host` the same as an (n_tables, 896) uint8 numpy array (only its shape is read), `out` the 1-D
    uint8 CUDA tensor the raw int16 planes are written into where the descriptors say (every element of every plane),
    `status` an int32 CUDA tensor that receives one status per segment.  `stream`: a HIP stream handle (None: the current
    launch stream)."""
    import ctypes
    import numpy as np
    from ._lib import JpegEntropyDesc, JpegEntropySeg
    from .data.coefficient_inputs import ENTROPY_DTYPE, SEGMENT_DTYPE
    from .jpeg2dct.numpy import HUFF_BYTES
    n = _check_staged(desc_host, ENTROPY_DTYPE, JpegEntropyDesc, desc_dev,
                      ((data, "data"), (desc_dev, "desc_dev"), (seg_dev, "seg_dev"), (tables_dev, "tables_dev"), (out, "out")))
    assert SEGMENT_DTYPE.itemsize == ctypes.sizeof(JpegEntropySeg), "segment-record layouts disagree"
    assert isinstance(seg_host, np.ndarray) and seg_host.dtype == SEGMENT_DTYPE and seg_host.ndim == 1 \
        and seg_host.flags.c_contiguous, "seg_host: expected a contiguous 1-D array of SEGMENT_DTYPE"
    assert seg_dev.numel() >= seg_host.nbytes and seg_dev.data_ptr() % 8 == 0, "seg_dev: too small or misaligned"
    assert isinstance(tables_host, np.ndarray) and tables_host.dtype == np.uint8 and tables_host.ndim == 2 \
        and tables_host.shape[1] == HUFF_BYTES, "tables_host: expected an (n_tables, %d) uint8 array" % HUFF_BYTES
    assert tables_dev.numel() >= tables_host.size, "tables_dev: smaller than the tables"
    assert status.is_cuda and status.dtype == torch.int32 and status.dim() == 1 and status.is_contiguous() \
        and status.numel() >= seg_host.shape[0], "status: expected a contiguous int32 CUDA tensor of one entry per segment"
    check(_L().dj_jpeg_entropy_decode(ptr(data), data.numel(), ptr(desc_dev), desc_host.ctypes.data, n, ptr(seg_dev),
                                      seg_host.ctypes.data, seg_host.shape[0], ptr(tables_dev), tables_host.shape[0],
                                      ptr(out), out.numel(), ptr(status), stream if stream is not None else _stream()),
          "dj_jpeg_entropy_decode")
    return out, status


# ---- the same by chunks, for files without restart intervals: one lane per chunk ----------------------------------------------
def jpeg_entropy_decode_chunked(data, desc_dev, desc_host, seg_dev, seg_host, tables_dev, tables_host, out, status, chunk_bytes,
                                scratch, rounds=None, stream=None):
    """dj_jpeg_entropy_decode_chunked: the arguments of `jpeg_entropy_decode` (the records' `reserved` holding each
    segment's first chunk, as data/coefficient_inputs.py:`chunked_records` fills it), `chunk_bytes` (a multiple of 16 in
    16..4096), `scratch` a 1-D uint8 CUDA tensor, 16-byte aligned, of at least the bytes the entry point asks for (it
    refuses a shorter one), and optionally `rounds`, an int32 CUDA tensor that receives the synchronisation rounds of each
    segment."""
    import ctypes
    import numpy as np
    from ._lib import JpegEntropyDesc, JpegEntropySeg
    from .data.coefficient_inputs import ENTROPY_DTYPE, SEGMENT_DTYPE
    from .jpeg2dct.numpy import HUFF_BYTES
    n = _check_staged(desc_host, ENTROPY_DTYPE, JpegEntropyDesc, desc_dev,
                      ((data, "data"), (desc_dev, "desc_dev"), (seg_dev, "seg_dev"), (tables_dev, "tables_dev"), (out, "out"),
                       (scratch, "scratch")))
    assert SEGMENT_DTYPE.itemsize == ctypes.sizeof(JpegEntropySeg), "segment-record layouts disagree"
    assert isinstance(seg_host, np.ndarray) and seg_host.dtype == SEGMENT_DTYPE and seg_host.ndim == 1 \
        and seg_host.flags.c_contiguous, "seg_host: expected a contiguous 1-D array of SEGMENT_DTYPE"
    assert seg_dev.numel() >= seg_host.nbytes and seg_dev.data_ptr() % 8 == 0, "seg_dev: too small or misaligned"
    assert isinstance(tables_host, np.ndarray) and tables_host.dtype == np.uint8 and tables_host.ndim == 2 \
        and tables_host.shape[1] == HUFF_BYTES, "tables_host: expected an (n_tables, %d) uint8 array" % HUFF_BYTES
    assert tables_dev.numel() >= tables_host.size, "tables_dev: smaller than the tables"
    for t, name in ((status, "status"),) + (((rounds, "rounds"),) if rounds is not None else ()):
        assert t.is_cuda and t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous() \
            and t.numel() >= seg_host.shape[0], "%s: expected a contiguous int32 CUDA tensor of one entry per segment" % name
    check(_L().dj_jpeg_entropy_decode_chunked(ptr(data), data.numel(), ptr(desc_dev), desc_host.ctypes.data, n, ptr(seg_dev),
                                              seg_host.ctypes.data, seg_host.shape[0], ptr(tables_dev), tables_host.shape[0],
                                              ptr(out), out.numel(), ptr(status), int(chunk_bytes), ptr(scratch), scratch.numel(),
                                              ptr(rounds) if rounds is not None else None,
                                              stream if stream is not None else _stream()),
          "dj_jpeg_entropy_decode_chunked")
    return out, status


# ---- Pascal-VOC evaluation: greedy matching, then cumulative counts / precision / recall / sampled AP -------------------------
def _check_eval_tensor(t, name, dtype, numel):
    assert t.is_cuda and t.is_contiguous() and t.dtype == dtype and t.numel() == numel, \
        "%s: expected a contiguous %s CUDA tensor of %d elements" % (name, dtype, numel)


def eval_match(pred_boxes, seg_ranks, seg_offsets, seg_class, seg_image, class_offsets, gt_boxes, gt_class, gt_neutral,
               gt_offsets, max_gt_per_image, use_neutral, matching_iou_threshold, border_pixels, tp, fp):
    """dj_eval_match on the arrays of eval_utils/device_matching.py:pack_evaluation (CUDA tensors of the same dtypes):
    writes the true / false positive flags of every prediction at class offset + rank into the zeroed int32 tensors
    `tp` / `fp`.  `border_pixels`: 0 'half', 1 'include', -1 'exclude'."""
    n_pred, n_seg, n_gt = pred_boxes.shape[0], seg_class.numel(), gt_class.numel()
    n_classes, n_images = class_offsets.numel() - 2, gt_offsets.numel() - 1
    for t, name, dtype, numel in ((pred_boxes, "pred_boxes", torch.float32, n_pred * 4), (seg_ranks, "seg_ranks", torch.int32, n_pred),
                                  (seg_offsets, "seg_offsets", torch.int32, n_seg + 1), (seg_class, "seg_class", torch.int32, n_seg),
                                  (seg_image, "seg_image", torch.int32, n_seg),
                                  (class_offsets, "class_offsets", torch.int32, n_classes + 2),
                                  (gt_boxes, "gt_boxes", torch.float64, n_gt * 4), (gt_class, "gt_class", torch.int32, n_gt),
                                  (gt_neutral, "gt_neutral", torch.uint8, n_gt), (gt_offsets, "gt_offsets", torch.int32, n_images + 1),
                                  (tp, "tp", torch.int32, n_pred), (fp, "fp", torch.int32, n_pred)):
        _check_eval_tensor(t, name, dtype, numel)
    check(_L().dj_eval_match(ptr(pred_boxes), ptr(seg_ranks), ptr(seg_offsets), ptr(seg_class), ptr(seg_image), n_seg,
                             ptr(class_offsets), n_classes, n_pred, ptr(gt_boxes), ptr(gt_class), ptr(gt_neutral),
                             ptr(gt_offsets), n_images, n_gt, int(max_gt_per_image), int(bool(use_neutral)),
                             float(matching_iou_threshold), int(border_pixels), ptr(tp), ptr(fp), _stream()), "dj_eval_match")
    return tp, fp


def eval_precision_recall_ap(tp, fp, class_offsets, num_gt, thresholds, cum_tp, cum_fp, precision, recall, ap):
    """dj_eval_precision_recall_ap: from the int32 flags of `eval_match`, per class the running sums (`cum_tp` / `cum_fp`,
    int32), `precision` / `recall` (float64) per rank and `ap[class]` (float64, n_classes + 1 entries) sampled at the
    float64 `thresholds`; `num_gt` holds the n_classes + 1 ground-truth counts as float64."""
    n_pred, n_classes = tp.numel(), class_offsets.numel() - 2
    for t, name, dtype, numel in ((tp, "tp", torch.int32, n_pred), (fp, "fp", torch.int32, n_pred),
                                  (class_offsets, "class_offsets", torch.int32, n_classes + 2),
                                  (num_gt, "num_gt", torch.float64, n_classes + 1),
                                  (thresholds, "thresholds", torch.float64, thresholds.numel()),
                                  (cum_tp, "cum_tp", torch.int32, n_pred), (cum_fp, "cum_fp", torch.int32, n_pred),
                                  (precision, "precision", torch.float64, n_pred), (recall, "recall", torch.float64, n_pred),
                                  (ap, "ap", torch.float64, n_classes + 1)):
        _check_eval_tensor(t, name, dtype, numel)
    check(_L().dj_eval_precision_recall_ap(ptr(tp), ptr(fp), ptr(class_offsets), n_classes, n_pred, ptr(num_gt),
                                           ptr(thresholds), thresholds.numel(), ptr(cum_tp), ptr(cum_fp), ptr(precision),
                                           ptr(recall), ptr(ap), _stream()), "dj_eval_precision_recall_ap")
    return ap


def eval_collect(decoded, n_valid, desc_host, first_ordinal, n_classes, n_images, conf_digits, boxes_final, records, counters):
    """dj_eval_collect: append the rows of `decoded` ([B][rows][6] float32 CUDA tensor) whose class id is not 0, for the
    first `n_valid` images, to `records` (the dict of eval_utils/device_matching.py:DeviceCollector: rec_class, rec_image,
    rec_ordinal int32, rec_conf float32, rec_conf64 float64, rec_boxes float32 [capacity][4]) behind counters[0].
    `desc_host`: one device_matching.DESC_DTYPE record per image, on the host.  One launch, no synchronisation."""
    import ctypes
    import numpy as np
    from .eval_utils.device_matching import DESC_DTYPE
    assert decoded.dim() == 3 and decoded.shape[2] == 6, "decoded: expected [B][rows][6]"
    b, rows = int(decoded.shape[0]), int(decoded.shape[1])
    capacity = records["rec_class"].numel()
    _check_eval_tensor(decoded, "decoded", torch.float32, b * rows * 6)
    for name, dtype, numel in (("rec_class", torch.int32, capacity), ("rec_image", torch.int32, capacity),
                               ("rec_ordinal", torch.int32, capacity), ("rec_conf", torch.float32, capacity),
                               ("rec_conf64", torch.float64, capacity), ("rec_boxes", torch.float32, capacity * 4)):
        _check_eval_tensor(records[name], name, dtype, numel)
    _check_eval_tensor(counters, "counters", torch.int32, 4)
    assert DESC_DTYPE.itemsize == 16 and ctypes.sizeof(ctypes.c_int) == 4, "descriptor layouts disagree"
    assert isinstance(desc_host, np.ndarray) and desc_host.dtype == DESC_DTYPE and desc_host.shape == (b,) \
        and desc_host.flags.c_contiguous, "desc_host: expected a contiguous array of one DESC_DTYPE record per image"
    check(_L().dj_eval_collect(ptr(decoded), b, rows, int(n_valid), desc_host.ctypes.data, int(first_ordinal), int(n_classes),
                               int(n_images), int(conf_digits), int(bool(boxes_final)), ptr(records["rec_class"]),
                               ptr(records["rec_image"]), ptr(records["rec_ordinal"]), ptr(records["rec_conf"]),
                               ptr(records["rec_conf64"]), ptr(records["rec_boxes"]), capacity, ptr(counters), _stream()),
          "dj_eval_collect")
    return counters


def eval_rank_workspace_bytes(capacity, n_classes):
    return check(_L().dj_eval_rank_workspace_bytes(int(capacity), int(n_classes)), "dj_eval_rank_workspace_bytes")


def eval_rank(records, n_classes, n_images, counters, out, workspace):
    """dj_eval_rank: the counters[0] records of `records` -> `out`, a dict of CUDA tensors sized by the capacity:
    class_offsets [n_classes + 2], pred_class, pred_image, seg_class, seg_image, seg_ranks [capacity], seg_offsets
    [capacity + 1] int32, pred_conf [capacity], pred_boxes [capacity][4] float32; counters[2] receives the number of
    segments.  `workspace`: a uint8 CUDA tensor of `eval_rank_workspace_bytes` bytes.  No synchronisation."""
    capacity = records["rec_class"].numel()
    for name, dtype, numel in (("rec_class", torch.int32, capacity), ("rec_image", torch.int32, capacity),
                               ("rec_conf", torch.float32, capacity), ("rec_boxes", torch.float32, capacity * 4)):
        _check_eval_tensor(records[name], name, dtype, numel)
    for name, dtype, numel in (("class_offsets", torch.int32, n_classes + 2), ("pred_class", torch.int32, capacity),
                               ("pred_image", torch.int32, capacity), ("pred_conf", torch.float32, capacity),
                               ("pred_boxes", torch.float32, capacity * 4), ("seg_class", torch.int32, capacity),
                               ("seg_image", torch.int32, capacity), ("seg_offsets", torch.int32, capacity + 1),
                               ("seg_ranks", torch.int32, capacity)):
        _check_eval_tensor(out[name], name, dtype, numel)
    _check_eval_tensor(counters, "counters", torch.int32, 4)
    _check_eval_tensor(workspace, "workspace", torch.uint8, workspace.numel())
    check(_L().dj_eval_rank(ptr(records["rec_class"]), ptr(records["rec_image"]), ptr(records["rec_conf"]),
                            ptr(records["rec_boxes"]), capacity, int(n_classes), int(n_images), ptr(counters),
                            ptr(out["class_offsets"]), ptr(out["pred_class"]), ptr(out["pred_image"]), ptr(out["pred_conf"]),
                            ptr(out["pred_boxes"]), ptr(out["seg_class"]), ptr(out["seg_image"]), ptr(out["seg_offsets"]),
                            ptr(out["seg_ranks"]), ptr(workspace), workspace.numel(), _stream()), "dj_eval_rank")
    return out


# ---- validation metrics of a classifier, accumulated on the device over a pass of a generator ----------------------------------
def eval_accumulate(y_true, probs, ks, loss_mean, loss_weight, acc, counts):
    """dj_eval_accumulate: add one batch to the accumulators of a sweep.  `y_true` / `probs`: contiguous float32 CUDA
    tensors [rows][C], or both None (only the loss is accumulated); `ks`: a contiguous int32 numpy array of at most 8
    entries on the host (k >= 1: top-k accuracy as tf.nn.in_top_k counts it, 0: categorical accuracy); `loss_mean`: a
    float32 CUDA tensor whose first element is the batch's mean loss, or None; `acc`: float64 CUDA tensor [2] receiving
    (loss_weight * loss, loss_weight); `counts`: int64 CUDA tensor [1 + len(ks)] receiving (rows, hits per entry).  One launch, no
    synchronisation."""
    import numpy as np
    assert isinstance(ks, np.ndarray) and ks.dtype == np.int32 and ks.ndim == 1 and ks.flags.c_contiguous, \
        "ks: expected a contiguous int32 array on the host"
    rows, c = 0, 0
    if y_true is not None or probs is not None:
        assert y_true is not None and probs is not None and probs.dim() == 2 and y_true.shape == probs.shape, \
            "y_true / probs: expected two [rows][C] tensors of one shape"
        rows, c = int(probs.shape[0]), int(probs.shape[1])
        _check_eval_tensor(y_true, "y_true", torch.float32, rows * c)
        _check_eval_tensor(probs, "probs", torch.float32, rows * c)
    if loss_mean is not None:
        assert loss_mean.is_cuda and loss_mean.dtype == torch.float32 and loss_mean.numel() >= 1, \
            "loss_mean: expected a float32 CUDA tensor"
    _check_eval_tensor(acc, "acc", torch.float64, 2)
    _check_eval_tensor(counts, "counts", torch.int64, 1 + ks.size)
    check(_L().dj_eval_accumulate(ptr(y_true), ptr(probs), rows, c, ks.ctypes.data, int(ks.size), ptr(loss_mean),
                                  float(loss_weight), ptr(acc), ptr(counts), _stream()), "dj_eval_accumulate")
    return acc, counts
