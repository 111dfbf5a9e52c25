"""ctypes binding of csrc/libdj_hip.so (the C ABI declared in include/dj_hip.h).

There is no CPU fallback: if the library is missing the import of any compute entry point
raises, and every call checks the return code and raises `DjError` with dj_last_error()."""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_long, c_uint32, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DJ_LIB_PATH") or os.path.join(_HERE, "csrc", "libdj_hip.so")   # override: kernel experiments


class DjError(RuntimeError):
    pass


class CopyPart(Structure):   # dj_copy_part
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("ld_src", c_long), ("ld_dst", c_long), ("rows", c_long),
                ("cols", c_long), ("beta", c_int)]


class ColsumPart(Structure):   # dj_colsum_part
    _fields_ = [("x", c_void_p), ("out", c_void_p), ("rows", c_long), ("C", c_int), ("ld", c_int), ("beta", c_int)]


class ImagePrepDesc(Structure):   # dj_image_prep_desc
    _fields_ = ([(n, c_long) for n in ("src_offset", "src_stride", "scratch_offset")]
                + [(n, c_int) for n in ("src_h", "src_w", "res_h", "res_w", "crop_y", "crop_x", "flip", "h_bounds", "h_taps",
                                        "h_ksize", "v_bounds", "v_taps", "v_ksize", "row0", "n_rows")])


class PatchResizeDesc(Structure):   # dj_patch_resize_desc
    _fields_ = ([(n, c_long) for n in ("src_offset", "src_stride", "scratch_offset")]
                + [(n, c_int) for n in ("src_h", "src_w", "win_y0", "win_x0", "win_h", "win_w", "flip", "background", "h_bounds",
                                        "h_taps", "h_ksize", "v_bounds", "v_taps", "v_ksize")])


class JpegPixelsDesc(Structure):   # dj_jpeg_pixels_desc
    _fields_ = ([("coef_offset", c_long * 3), ("sample_offset", c_long * 3), ("dst_offset", c_long), ("dst_stride", c_long)]
                + [(n, c_int) for n in ("table_offset", "n_components", "h_samp", "v_samp", "height", "width", "ya", "yb",
                                        "xa", "xb")]
                + [(n, c_int * 3) for n in ("blocks_h", "blocks_w", "by0", "by1", "bx0", "bx1")])


class JpegDctDesc(Structure):   # dj_jpeg_dct_desc
    _fields_ = ([("coef_offset", c_long * 3)] + [(n, c_int * 3) for n in ("blocks_h", "blocks_w", "by0", "bx0")]
                + [(n, c_int) for n in ("table_offset", "n_components", "flip")])


class JpegEntropyDesc(Structure):   # dj_jpeg_entropy_desc
    _fields_ = ([("plane_offset", c_long * 3), ("plane_capacity", c_long * 3)]
                + [(n, c_int * 3) for n in ("blocks_h", "blocks_w", "h_blocks", "v_blocks", "dc_table", "ac_table")]
                + [(n, c_int) for n in ("table_first", "n_components", "mcus_x", "mcus_y", "seg_first", "n_segments")])


class JpegEntropySeg(Structure):   # dj_jpeg_entropy_seg
    _fields_ = [("begin", c_long), ("end", c_long), ("file", c_int), ("first_mcu", c_int), ("n_mcus", c_int), ("reserved", c_int)]


class PhotometricOps(Structure):   # dj_photometric_ops
    _fields_ = [("n_ops", c_int), ("code", c_int * 4), ("reserved", c_int), ("param", (c_double * 3) * 4)]


class RgbWarpRecord(Structure):   # dj_rgb_warp_record
    _fields_ = [("m", c_double * 6), ("identity", c_int), ("flip_cols", c_int), ("flip_rows", c_int), ("reserved", c_int)]


class SsdPhotoParams(Structure):   # dj_ssd_photo_params
    _fields_ = [("sequence", c_int), ("flags", c_int), ("brightness", c_float), ("contrast", c_float), ("saturation", c_float),
                ("hue", c_float), ("order", c_int * 3), ("reserved", c_int)]


class ConvDesc(Structure):
    """Mirror of `dj_conv2d_desc` (include/dj_hip.h)."""
    _fields_ = [(n, c_int) for n in (
        "batch", "in_h", "in_w", "in_c", "out_h", "out_w", "out_c",
        "kernel_h", "kernel_w", "stride_h", "stride_w", "dilation_h", "dilation_w",
        "pad_top", "pad_left", "ld_x", "ld_y")]


_P, _I = c_void_p, c_int


class ConvFwdArgs(Structure):   # dj_conv_fwd_args: all zeros = fp32 tensors, no option
    _fields_ = [("x", _P), ("dt_x", _I), ("w", _P), ("dt_w", _I), ("bias", _P), ("y", _P), ("dt_y", _I),
                ("pro_scale", _P), ("pro_shift", _P), ("pro_relu", _I), ("flags", _I), ("stats", _P),
                ("res", _P), ("ld_res", _I), ("res_scale", _P), ("res_shift", _P), ("sum_out", _P), ("ld_sum", _I),
                ("dt_sum", _I), ("workspace", _P), ("workspace_floats", c_long)]


class ConvDgradArgs(Structure):   # dj_conv_dgrad_args
    _fields_ = [("dy", _P), ("dt_dy", _I), ("w", _P), ("dt_w", _I), ("bias", _P), ("dx", _P), ("dt_dx", _I), ("flags", _I),
                ("z", _P), ("ld_z", _I), ("dt_z", _I), ("mean", _P), ("invstd", _P), ("scale", _P), ("shift", _P),
                ("partial", _P), ("mask_x", _P), ("ld_mask", _I)]


class ConvWgradArgs(Structure):   # dj_conv_wgrad_args
    _fields_ = [("x", _P), ("dt_x", _I), ("dy", _P), ("dt_dy", _I), ("dw", _P), ("pro_scale", _P), ("pro_shift", _P),
                ("pro_relu", _I), ("dw_zeroed", _I)]


_lib = None
ABI_VERSION = 5    # DJ_ABI_VERSION of include/dj_hip.h these bindings were written for


def load():
    """Load the shared library (idempotent).  Raises DjError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DjError(
            "HIP extension %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the compute path)" % LIB_PATH)
    # torch first: its wheel bundles the HIP runtime (libamdhip64) the process must share -- loading this library
    # before torch would bind it to /opt/rocm's copy instead, and kernels registered with one runtime cannot be
    # launched on the device the other one owns ("no ROCm-capable device is detected")
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    lib.dj_abi_version.restype = c_int
    have = lib.dj_abi_version()
    if have != ABI_VERSION:
        # a stale build product (the .so is git-ignored and travels with the working tree): calling it through these
        # signatures would pass arguments it reads differently
        raise DjError("%s reports ABI version %d, these bindings are written for %d: rebuild it "
                      "(`python -c 'import __graft_entry__ as g; g.build()'`)" % (LIB_PATH, have, ABI_VERSION))
    _declare(lib)
    _lib = lib
    return lib


# name -> (restype, [argtypes]); kept in one table so the "exports every symbol" test can walk it
FP = c_void_p  # device float* passed as integer address
SIGNATURES = {
    "dj_last_error": (c_char_p, []),
    "dj_abi_version": (c_int, []),
    "dj_conv2d_fwd_stats_rows": (c_int, [POINTER(ConvDesc)]),
    "dj_conv2d_nhwc_fwd": (c_int, [POINTER(ConvDesc), POINTER(ConvFwdArgs), c_void_p]),
    "dj_conv2d_fwd_workspace_floats": (c_long, [POINTER(ConvDesc), c_int]),
    "dj_conv2d_nhwc_dgrad": (c_int, [POINTER(ConvDesc), POINTER(ConvDgradArgs), c_void_p]),
    "dj_conv2d_dgrad_relumask_supported": (c_int, [POINTER(ConvDesc)]),
    "dj_conv2d_nhwc_wgrad": (c_int, [POINTER(ConvDesc), POINTER(ConvWgradArgs), c_void_p]),
    "dj_shadow_weights": (c_int, [FP, FP, FP, c_long, c_void_p]),
    "dj_affine_act_t": (c_int, [FP, c_int, c_int, FP, FP, FP, c_int, c_int, FP, FP, FP, c_int, c_int, c_long, c_int, c_int,
                                c_void_p]),
    "dj_bn_bwd_reduce_t": (c_int, [FP, c_int, c_int, FP, c_int, c_int, FP, c_int, c_int, FP, FP, FP, FP, c_int, c_long, c_int, FP,
                                   c_void_p]),
    "dj_bn_bwd_apply_t": (c_int, [FP, c_int, c_int, FP, c_int, c_int, FP, c_int, c_int, FP, FP, c_int, FP, FP, FP, FP, c_int,
                                  c_int, c_long, c_int, FP, c_int, c_int, c_int, c_void_p]),
    "dj_relu_bwd_t": (c_int, [FP, c_int, c_int, FP, c_int, c_int, FP, c_int, c_int, c_long, c_int, c_int, c_void_p]),
    "dj_copy2d_t": (c_int, [FP, c_int, c_long, FP, c_int, c_long, c_long, c_long, c_int, c_void_p]),
    "dj_conv2d_fwd_addrelu_supported": (c_int, [POINTER(ConvDesc)]),
    "dj_colsum_direct": (c_int, [FP, c_long, c_int, c_int, FP, c_int, c_void_p]),
    "dj_colsum_multi": (c_int, [POINTER(ColsumPart), c_int, c_void_p]),
    "dj_copy2d_multi": (c_int, [POINTER(CopyPart), c_int, c_void_p]),
    "dj_set_fast_path": (None, [c_int]),
    "dj_set_gather_variants": (None, [c_int]),
    "dj_set_compute_mode": (c_int, [c_int]),
    "dj_set_thread_compute_mode": (c_int, [c_int]),
    "dj_get_compute_mode": (c_int, []),
    "dj_conv2d_tune_configs": (c_int, []),
    "dj_conv2d_tune_set": (c_int, [c_int, POINTER(ConvDesc), c_int, c_int]),
    "dj_conv2d_default_config": (c_int, [c_int, POINTER(ConvDesc), POINTER(c_int), POINTER(c_int)]),
    "dj_reduce_rows": (c_int, [c_long]),
    "dj_colstats_partial": (c_int, [FP, c_long, c_int, c_int, FP, c_void_p]),
    "dj_colsum_partial": (c_int, [FP, c_long, c_int, c_int, FP, c_void_p]),
    "dj_colreduce_finalize": (c_int, [FP, c_int, c_int, c_int, FP, c_int, c_void_p]),
    "dj_bn_train_finalize": (c_int, [FP, c_int, c_long, FP, FP, FP, c_float, c_float, FP, FP, FP, FP, FP, FP, c_int,
                                     c_void_p]),
    "dj_bn_infer_coeffs": (c_int, [FP, FP, FP, FP, c_float, FP, FP, c_int, c_void_p]),
    "dj_affine_act": (c_int, [FP, c_int, FP, FP, FP, c_int, FP, FP, FP, c_int, c_long, c_int, c_int, c_void_p]),
    "dj_bn_bwd_reduce": (c_int, [FP, c_int, FP, c_int, FP, c_int, FP, FP, FP, FP, c_int, c_long, c_int, FP, c_void_p]),
    "dj_bn_bwd_finalize": (c_int, [FP, c_int, c_long, FP, FP, FP, FP, FP, FP, FP, FP, c_int, c_void_p]),
    "dj_bn_bwd_apply": (c_int, [FP, c_int, FP, c_int, FP, c_int, FP, FP, c_int, FP, FP, FP, FP, c_int, c_long, c_int,
                                FP, c_int, c_int, c_void_p]),
    "dj_relu_bwd": (c_int, [FP, c_int, FP, c_int, FP, c_int, c_long, c_int, c_int, c_void_p]),
    "dj_copy2d": (c_int, [FP, c_long, FP, c_long, c_long, c_long, c_int, c_void_p]),
    "dj_upsample2x": (c_int, [FP, c_int, FP, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "dj_l2norm_fwd": (c_int, [FP, c_int, FP, FP, c_int, FP, c_long, c_int, c_void_p]),
    "dj_l2norm_bwd": (c_int, [FP, c_int, FP, c_int, FP, FP, FP, c_int, FP, c_long, c_int, c_int, c_void_p]),
    "dj_maxpool2d_fwd": (c_int, [FP, FP] + [c_int] * 13 + [c_void_p, c_void_p]),
    "dj_maxpool2d_bwd": (c_int, [FP, FP, FP] + [c_int] * 14 + [c_void_p, c_void_p]),
    "dj_softmax_fwd": (c_int, [FP, FP, c_long, c_int, c_void_p]),
    "dj_softmax_bwd": (c_int, [FP, FP, c_long, FP, c_long, c_int, c_int, c_void_p]),
    "dj_ssd_loss_workspace_floats": (c_long, [c_long]),
    "dj_ssd_loss_fwd": (c_int, [FP, FP, c_long, c_int, c_int, c_int, c_float, FP, FP, c_void_p]),
    "dj_ssd_loss_bwd": (c_int, [FP, FP, c_long, c_int, c_float, c_float, FP, FP, FP, c_void_p]),
    "dj_categorical_crossentropy": (c_int, [FP, FP, c_long, c_int, c_float, FP, FP, FP, c_void_p]),
    "dj_sgd_momentum_update": (c_int, [FP, FP, FP, c_long, c_float, c_float, c_int, c_float, c_float, FP, c_void_p]),
    "dj_optim_groups_per_pass": (c_long, []),
    "dj_adam_update": (c_int, [FP, FP, FP, FP, FP, c_long, c_float, c_float, c_float, c_float, c_float, c_float, FP,
                               c_void_p]),
    "dj_adadelta_update": (c_int, [FP, FP, FP, FP, c_long, c_float, c_float, c_float, c_float, c_float, c_float, FP,
                                   c_void_p]),
    "dj_rmsprop_update": (c_int, [FP, FP, FP, c_long] + [c_float] * 5 + [FP, c_void_p]),
    "dj_adagrad_update": (c_int, [FP, FP, FP, c_long] + [c_float] * 4 + [FP, c_void_p]),
    "dj_adamax_update": (c_int, [FP, FP, FP, FP, c_long] + [c_float] * 6 + [FP, c_void_p]),
    "dj_nadam_update": (c_int, [FP, FP, FP, FP, c_long] + [c_float] * 11 + [FP, c_void_p]),
    "dj_decode_detections_workspace_floats": (c_long, [c_int, c_int, c_int, c_int]),
    "dj_decode_detections": (c_int, [FP, c_int, c_int, c_int, c_float, c_float, c_int, c_int, c_int, c_int, c_int, FP, FP,
                                     c_void_p]),
    "dj_decode_detections_fast_workspace_floats": (c_long, [c_int, c_int, c_int]),
    "dj_decode_detections_fast": (c_int, [FP, c_int, c_int, c_int, c_float, c_float, c_int, c_int, c_int, c_int, c_int, FP, FP,
                                          c_void_p]),
    "dj_ssd_encode_targets": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                      c_int, c_double, c_double, c_int, FP, c_void_p]),
    "dj_global_avg_pool_fwd": (c_int, [FP, FP, c_int, c_int, c_int, c_void_p]),
    "dj_global_avg_pool_bwd": (c_int, [FP, FP, c_int, c_int, c_int, c_int, c_void_p]),
    "dj_rgb_to_dct": (c_int, [c_void_p, c_int, c_int, c_int, c_long, c_void_p, c_void_p, c_int, FP, c_long, FP, c_long, FP,
                              c_long, c_void_p]),
    "dj_image_prep_scratch_bytes": (c_long, [c_void_p, c_int, c_int]),
    "dj_image_prep": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_long, c_int, c_void_p, c_long,
                              c_void_p, c_long, c_void_p]),
    "dj_photometric": (c_int, [c_void_p, c_int, c_int, c_int, c_long, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dj_rgb_warp": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_long,
                            c_void_p]),
    "dj_patch_resize_scratch_bytes": (c_long, [c_void_p, c_int, c_int]),
    "dj_patch_resize": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_long, c_int, c_int, c_void_p,
                                c_long, c_void_p, c_long, c_void_p]),
    "dj_ssd_photometric": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "dj_jpeg_pixels": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_int, c_void_p, c_long, c_void_p, c_long, c_void_p,
                               c_long, c_void_p]),
    "dj_jpeg_dct_inputs": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_int, c_void_p, c_long, c_int, c_int, c_int, c_int,
                                   FP, c_long, c_long, FP, c_long, c_long, FP, c_long, c_long, c_void_p]),
    "dj_jpeg_entropy_decode": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                       c_void_p, c_long, c_void_p, c_void_p]),
    "dj_jpeg_entropy_chunked_scratch_bytes": (c_long, [c_long, c_long, c_long, c_long]),
    "dj_jpeg_entropy_decode_chunked": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                               c_int, c_void_p, c_long, c_void_p, c_int, c_void_p, c_long, c_void_p, c_void_p]),
    "dj_eval_match": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p,
                              c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_double, c_int, c_void_p, c_void_p,
                              c_void_p]),
    "dj_eval_precision_recall_ap": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dj_eval_collect": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p]),
    "dj_eval_rank_workspace_bytes": (c_long, [c_long, c_int]),
    "dj_eval_rank": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p]),
    "dj_eval_accumulate": (c_int, [FP, FP, c_long, c_int, c_void_p, c_int, FP, c_double, c_void_p, c_void_p, c_void_p]),
    "dj_dropout_groups_per_pass": (c_long, []),
    "dj_dropout_fwd": (c_int, [FP, FP, c_long, c_uint32, c_float, c_uint32, c_uint32, c_uint32, c_uint32, c_void_p]),
    "dj_dropout_bwd": (c_int, [FP, FP, c_long, c_uint32, c_float, c_uint32, c_uint32, c_uint32, c_uint32, c_int, c_void_p]),
}


def _declare(lib):
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args


def check(rc, what=""):
    if rc < 0:
        msg = load().dj_last_error()
        raise DjError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else "?"))
    return rc


def ptr(t):
    """Device address of a torch tensor (None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()


# The HIP stream the next launch goes to.  engine.Plan sets it while it runs its launch lists (the main stream, and the side
# stream around the launches it issues there): a plain attribute instead of torch's stream context manager, whose enter /
# exit cost ~25 us of host time per side-stream launch -- in the stretches of the step that consist of 5-10 us kernels (the
# extra-feature layers and predictor heads) the host was what the GPU waited for.  None: torch's current stream.
import threading

_stream_tls = threading.local()      # per thread: two threads may run plans of their own side by side


def set_launch_stream(handle):
    """Set (None: clear) the calling thread's launch stream; -> the previous setting."""
    prev = getattr(_stream_tls, "handle", None)
    _stream_tls.handle = handle
    return prev


def current_stream():
    h = getattr(_stream_tls, "handle", None)
    if h is not None:
        return h
    import torch
    return torch.cuda.current_stream().cuda_stream
