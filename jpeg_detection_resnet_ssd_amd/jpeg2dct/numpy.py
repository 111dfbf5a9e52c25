"""`jpeg2dct.numpy` look-alike: load / loads -> (dct_y, dct_cb, dct_cr), each (blocks_h, blocks_w, 64) int16 in natural
coefficient order, de-quantised when normalized=True (jpeg2dct's default) -- what
localisation_part/data_generator/object_detection_2d_data_generator_dct_j2d.py:1180 and
classification_part/vgg_jpeg_keras/generators/generators.py:120-130 consume.  `decode_batch` is the batched,
multi-threaded form that fills the float32 batch tensors directly."""
from __future__ import absolute_import

import ctypes
import os

import numpy as _np

_LIB = None


class JpegInfo(ctypes.Structure):   # dj_jpeg_info
    _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("n_components", ctypes.c_int),
                ("h_samp", ctypes.c_int * 4), ("v_samp", ctypes.c_int * 4), ("blocks_w", ctypes.c_int * 4),
                ("blocks_h", ctypes.c_int * 4), ("quant", (ctypes.c_int * 64) * 4), ("sof", ctypes.c_int)]


class JpegDecodeInfo(ctypes.Structure):   # dj_jpeg_decode_info
    _fields_ = [("base", JpegInfo), ("component_id", ctypes.c_int * 4), ("saw_jfif", ctypes.c_int),
                ("saw_adobe", ctypes.c_int), ("adobe_transform", ctypes.c_int), ("precision", ctypes.c_int),
                ("device_decodable", ctypes.c_int)]


HUFF_BYTES = 896      # DJ_JPEG_HUFF_BYTES


class JpegSegmentInfo(ctypes.Structure):   # dj_jpeg_segment_info
    _fields_ = [("decode", JpegDecodeInfo), ("entropy_decodable", ctypes.c_int), ("reason", ctypes.c_char * 100),
                ("restart_interval", ctypes.c_int), ("mcus_x", ctypes.c_int), ("mcus_y", ctypes.c_int),
                ("h_blocks", ctypes.c_int * 4), ("v_blocks", ctypes.c_int * 4), ("dc_table", ctypes.c_int * 4),
                ("ac_table", ctypes.c_int * 4), ("n_tables", ctypes.c_int), ("n_segments", ctypes.c_int),
                ("tables", (ctypes.c_ubyte * HUFF_BYTES) * 4)]


class SegmentScan(object):
    """What `scan_segments` found: `entropy_decodable` and, when it is False, `reason`; for an eligible file
    `restart_interval`, `mcus` = (down, across), per component `grids` [(blocks_h, blocks_w)], `mcu_blocks` [(down,
    across)] and `dc_table` / `ac_table` (indexes into `tables`), `tables` (n_tables, HUFF_BYTES) uint8 in the device
    form of include/dj_jpeg_segments.h, and `ranges` (n_segments, 2) int64: [begin, end) of each segment's bytes in the file."""

    def __init__(self, inf, ranges):
        self.entropy_decodable = bool(inf.entropy_decodable)
        self.reason = inf.reason.decode(errors="replace")
        b = inf.decode.base
        n = self.n_components = int(b.n_components)
        self.restart_interval = int(inf.restart_interval)
        self.mcus = (int(inf.mcus_y), int(inf.mcus_x))
        self.grids = [(int(b.blocks_h[c]), int(b.blocks_w[c])) for c in range(n)]
        self.mcu_blocks = [(int(inf.v_blocks[c]), int(inf.h_blocks[c])) for c in range(n)]
        self.dc_table = [int(inf.dc_table[c]) for c in range(n)]
        self.ac_table = [int(inf.ac_table[c]) for c in range(n)]
        self.tables4 = _np.frombuffer(inf.tables, dtype=_np.uint8).reshape(4, HUFF_BYTES).copy()      # unused ones zero
        self.tables = self.tables4[:int(inf.n_tables)]
        self.ranges = ranges

    @property
    def n_segments(self):
        return len(self.ranges)


def _lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "libdj_jpeg.so")
        if not os.path.exists(path):
            raise ImportError("libdj_jpeg.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = ctypes.CDLL(path)
        lib.dj_jpeg_last_error.restype = ctypes.c_char_p
        lib.dj_jpeg_read_info.restype = ctypes.c_int
        lib.dj_jpeg_read_info.argtypes = [ctypes.c_char_p, ctypes.c_long, ctypes.POINTER(JpegInfo)]
        lib.dj_jpeg_read_coefficients.restype = ctypes.c_int
        lib.dj_jpeg_read_coefficients.argtypes = [ctypes.c_char_p, ctypes.c_long, ctypes.c_int,
                                                  ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_long),
                                                  ctypes.POINTER(JpegInfo)]
        lib.dj_jpeg_decode_batch_f32.restype = ctypes.c_int
        lib.dj_jpeg_decode_batch_f32.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_long),
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_void_p] + [ctypes.c_int] * 5
        lib.dj_jpeg_read_decode_info.restype = ctypes.c_int
        lib.dj_jpeg_read_decode_info.argtypes = [ctypes.c_char_p, ctypes.c_long, ctypes.POINTER(JpegDecodeInfo)]
        lib.dj_jpeg_read_raw_batch.restype = ctypes.c_int
        lib.dj_jpeg_read_raw_batch.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_long), ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_int]
        lib.dj_jpeg_scan_segments.restype = ctypes.c_int
        lib.dj_jpeg_scan_segments.argtypes = [ctypes.c_char_p, ctypes.c_long, ctypes.POINTER(JpegSegmentInfo), ctypes.c_void_p,
                                              ctypes.c_long]
        lib.dj_jpeg_scan_segments_unmarked.restype = ctypes.c_int
        lib.dj_jpeg_scan_segments_unmarked.argtypes = lib.dj_jpeg_scan_segments.argtypes
        _LIB = lib
    return _LIB


def _check(rc):
    if rc != 0:
        raise ValueError("JPEG coefficient reader: " + _lib().dj_jpeg_last_error().decode())


def info(buf):
    """Frame geometry, sampling factors and quantisation tables (natural order) without decoding."""
    buf = bytes(buf)
    inf = JpegInfo()
    _check(_lib().dj_jpeg_read_info(buf, len(buf), ctypes.byref(inf)))
    return inf


def decode_info(buf):
    """`info` plus what decides the colour space (component ids, JFIF / Adobe markers, precision) and the reader's verdict
    `device_decodable` (include/dj_jpeg_decode.h) -> JpegDecodeInfo; ValueError for what the reader cannot parse."""
    buf = bytes(buf)
    inf = JpegDecodeInfo()
    _check(_lib().dj_jpeg_read_decode_info(buf, len(buf), ctypes.byref(inf)))
    return inf


def scan_segments(buf, max_segments=None, unmarked=False):
    """The pre-pass of entropy decoding on the GPU (include/dj_jpeg_segments.h: dj_jpeg_scan_segments): headers and one
    search for 0xFF bytes, no Huffman decoding -> `SegmentScan`.  A file that is not eligible -- one the reader cannot
    parse included -- comes back with `entropy_decodable` False and a `reason`, never as an exception.  `max_segments`: an
    upper bound the caller knows (the file's MCU count), which saves the first of two calls.  `unmarked=True`
    (dj_jpeg_scan_segments_unmarked): a file without restart intervals is eligible too, as one segment that holds all its
    MCUs (`restart_interval` = their number); every other file gives what it gives without."""
    buf = bytes(buf)
    scan = _lib().dj_jpeg_scan_segments_unmarked if unmarked else _lib().dj_jpeg_scan_segments
    inf = JpegSegmentInfo()
    if len(buf) == 0:
        inf.reason = b"empty file"
        return SegmentScan(inf, _np.zeros((0, 2), dtype=_np.int64))
    ranges = _np.zeros((int(max_segments or 0), 2), dtype=_np.int64)
    _check(scan(buf, len(buf), ctypes.byref(inf), ranges.ctypes.data, len(ranges)))
    if inf.n_segments > len(ranges):
        ranges = _np.zeros((inf.n_segments, 2), dtype=_np.int64)
        _check(scan(buf, len(buf), ctypes.byref(inf), ranges.ctypes.data, len(ranges)))
    return SegmentScan(inf, ranges[:inf.n_segments].copy())


def default_threads():
    try:
        return len(os.sched_getaffinity(0))
    except AttributeError:
        return os.cpu_count() or 1


def read_raw_batch(buffers, out, plane_offsets, plane_capacity, n_threads=None):
    """n JPEG byte strings -> their RAW (not de-quantised) int16 coefficient planes written into `out`, one caller-owned
    C-contiguous uint8 array (e.g. the numpy view of a pinned staging buffer), by `n_threads` host threads with the GIL
    released.  plane_offsets / plane_capacity: (n, 4) -- component c of file i goes to byte offset plane_offsets[i, c] and
    may take plane_capacity[i, c] values (both checked against the file and against `out`).  -> (n,) int32 status, 0 or
    negative per file: a file that fails leaves the others alone (`last_error()` has the first one's text)."""
    bufs = [bytes(b) for b in buffers]
    n = len(bufs)
    if n == 0:
        raise ValueError("expected at least one file")
    if not (isinstance(out, _np.ndarray) and out.dtype == _np.uint8 and out.ndim == 1 and out.flags["C_CONTIGUOUS"]
            and out.flags["WRITEABLE"]):
        raise ValueError("out: expected a writable C-contiguous 1-D uint8 array")
    offs = _np.ascontiguousarray(plane_offsets, dtype=_np.int64)
    caps = _np.ascontiguousarray(plane_capacity, dtype=_np.int64)
    if offs.shape != (n, 4) or caps.shape != (n, 4):
        raise ValueError("plane_offsets / plane_capacity: expected shape (%d, 4)" % n)
    arr = (ctypes.c_char_p * n)(*bufs)
    sizes = (ctypes.c_long * n)(*[len(b) for b in bufs])
    status = _np.zeros(n, dtype=_np.int32)
    rc = _lib().dj_jpeg_read_raw_batch(arr, sizes, n, out.ctypes.data, out.size, offs.ctypes.data, caps.ctypes.data,
                                       status.ctypes.data, int(n_threads if n_threads is not None else default_threads()))
    if rc < 0:
        _check(rc)
    return status


def last_error():
    return _lib().dj_jpeg_last_error().decode()


def loads(buf, normalized=True, channels=3):
    buf = bytes(buf)
    inf = info(buf)
    if inf.sof not in (0, 1):
        raise ValueError("JPEG coefficient reader: unsupported JPEG process SOF%d (only baseline / extended "
                         "sequential Huffman)" % inf.sof)
    n = inf.n_components
    planes = [_np.empty((inf.blocks_h[c], inf.blocks_w[c], 64), dtype=_np.int16) for c in range(n)]
    ptrs = (ctypes.c_void_p * 4)(*[p.ctypes.data for p in planes] + [None] * (4 - n))
    caps = (ctypes.c_long * 4)(*[p.size for p in planes] + [0] * (4 - n))
    _check(_lib().dj_jpeg_read_coefficients(buf, len(buf), int(bool(normalized)), ptrs, caps, None))
    if channels == 1 or n == 1:
        empty = _np.zeros((0, 0, 64), dtype=_np.int16)
        return (planes[0], empty, empty) if channels == 3 else (planes[0],)
    return tuple(planes[:3])


def load(filename, normalized=True, channels=3):
    with open(filename, "rb") as f:
        return loads(f.read(), normalized=normalized, channels=channels)


def decode_batch(buffers, y_blocks, c_blocks, normalized=True, n_threads=None, out=None):
    """n JPEG byte strings -> float32 (n, yh, yw, 64), (n, ch, cw, 64), (n, ch, cw, 64), decoded by `n_threads` host
    threads (the GIL is released for the whole call).  `out` may hold three preallocated (e.g. pinned) arrays."""
    bufs = [bytes(b) for b in buffers]
    n = len(bufs)
    (yh, yw), (ch, cw) = y_blocks, c_blocks
    if out is None:
        out = (_np.empty((n, yh, yw, 64), _np.float32), _np.empty((n, ch, cw, 64), _np.float32),
               _np.empty((n, ch, cw, 64), _np.float32))
    y, cb, cr = out
    for a, shp in ((y, (n, yh, yw, 64)), (cb, (n, ch, cw, 64)), (cr, (n, ch, cw, 64))):
        assert a.dtype == _np.float32 and a.flags["C_CONTIGUOUS"] and tuple(a.shape) == shp
    arr = (ctypes.c_char_p * n)(*bufs)
    sizes = (ctypes.c_long * n)(*[len(b) for b in bufs])
    if n_threads is None:
        n_threads = default_threads()
    _check(_lib().dj_jpeg_decode_batch_f32(arr, sizes, n, int(bool(normalized)), y.ctypes.data, cb.ctypes.data,
                                           cr.ctypes.data, yh, yw, ch, cw, int(n_threads)))
    return y, cb, cr
