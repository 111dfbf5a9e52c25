"""The networks' DCT inputs from a JPEG file's OWN coefficients: for a file that already has the network's geometry (a
dataset resized once, an evaluation set) decoding to pixels and re-encoding only rebuilds, with a generation loss, numbers
the entropy decoder already had.  This module states in numpy what reaches the model instead (`coefficient_inputs_host`),
and carries a batch to a model's resident input buffers, where csrc/dj_jpegdct.hip (`kernels.jpeg_dct_inputs`) writes the
same numbers bit for bit (`PendingCoefficientInputs`, `DeviceCoefficientInputs`).

Eligible files: what data/jpeg_pixels.py:`decodable` accepts (baseline / extended-sequential Huffman, 8 bits) AND either one
component (gray) or three with luma sampled 2x2 over chroma (4:2:0), the layout of the networks' inputs.  Anything else is
a ValueError that names the reason; there is no Pillow fallback, because this path has no pixels.

Window: (y0, x0, h, w) in pixels.  y0 and x0 are multiples of 16 (one MCU); along each axis the extent is a multiple of 16
or the window ends at the image's edge.  It yields the block grids `blocks_for(h, w)` of data/jpeg_dct.py -- luma
ceil(h/8) x ceil(w/8) from block (y0/8, x0/8), chroma ceil(ceil(h/2)/8) x ceil(ceil(w/2)/8) from block (y0/16, x0/16) --
which must lie inside the file's grids.  The default is the whole file: a 300x300 file gives (38, 38, 64) and
(19, 19, 128 | 64), the SSD300's inputs.

Value: float32(int16(coefficient * table entry)) -- the product in int32, truncated to int16 by two's-complement
wrap-around, then converted -- which is what the host reader emits (csrc/dj_jpeg.cpp: Decoder::emit, "jpeg2dct stores
shorts"); for a whole-file window the statement equals `emit_dct_inputs(None, jpeg_bytes=[...])` bit for bit.  A gray file
gives its Y plane and all-zero chroma.

Mirror: jpegtran's lossless horizontal flip, for windows with w % 16 == 0 only (then both grids mirror about the same
axis).  Output block column j of a component takes window block column n_cols - 1 - j, and in natural order k = 8u + v every
coefficient of odd v (k & 1) is negated: cos((2(7 - x) + 1) v pi / 16) = (-1)^v cos((2x + 1) v pi / 16).  The negation is
applied to the int16 value, with int16's wrap-around (-(-32768) = -32768), before the conversion to float.

Entropy decoding on the GPU (opt-in, `DeviceCoefficientInputs(device_entropy=True)`): a batch whose files all carry restart
intervals (jpeg2dct/numpy.py:`scan_segments` decides) uploads the files' bytes instead of their planes, and
csrc/dj_jpeg_entropy.hip (`kernels.jpeg_entropy_decode`) makes the same raw planes in device scratch, one restart interval
per lane, as data/entropy_decode.py states; any other batch takes the host reader whole.  The numbers that reach the model
are the same bit for bit.  `unmarked=True` on top of it widens that to ordinary files, which carry no restart intervals: a
batch that the one-lane-per-interval kernel cannot take, but whose files all pass the wider pre-pass
(`scan_segments(unmarked=True)`), is decoded by chunks (`ChunkedEntropyCoefficientPlan`, csrc/dj_jpeg_entropy_chunked.hip,
data/entropy_decode.py:`chunked_decode_host`), marked files riding along as several short segments.

All arithmetic here is int32 / int16."""
import numpy as np

from ..jpeg2dct import numpy as reader
from . import device_staging as ds
from .jpeg_dct import PendingInputs, blocks_for
from .jpeg_pixels import CoefficientImage

MCU = 16

# dj_jpeg_dct_desc (include/dj_hip.h), C layout
DESC_DTYPE = np.dtype([("coef_offset", np.int64, 3)] + [(n, np.int32, 3) for n in ("blocks_h", "blocks_w", "by0", "bx0")]
                      + [(n, np.int32) for n in ("table_offset", "n_components", "flip")], align=True)


def check_file(item):
    """bytes or a `CoefficientImage` -> the `CoefficientImage` of an eligible file; ValueError naming the reason for any
    other (progressive, CMYK, 12-bit: the reader's verdict; 4:4:4, 4:2:2: the sampling)."""
    image = item if isinstance(item, CoefficientImage) else CoefficientImage(item)
    if image.n_components == 3 and image.sampling != (2, 2):
        raise ValueError("this JPEG's luma is sampled %d x %d over chroma: only 4:2:0 (2 x 2) and gray files carry the "
                         "networks' block grids" % image.sampling)
    return image


def check_files(files):
    images = [check_file(f) for f in files]
    if not images:
        raise ValueError("expected at least one file")
    return images


def check_window(image, window=None):
    """None (the whole file) or (y0, x0, h, w) -> plain ints, checked against the module's rules and the file's grids."""
    height, width = image.shape[:2]
    if window is None:
        window = (0, 0, height, width)
    y0, x0, h, w = (int(v) for v in window)
    if y0 < 0 or x0 < 0 or y0 % MCU or x0 % MCU:
        raise ValueError("window origin (%d, %d) must be non-negative multiples of %d" % (y0, x0, MCU))
    if h < 1 or w < 1:
        raise ValueError("window extent %d x %d must be positive" % (h, w))
    for name, o, e, size in (("rows", y0, h, height), ("columns", x0, w, width)):
        if e % MCU and o + e != size:
            raise ValueError("window %s: an extent of %d from %d is neither a multiple of %d nor ends at the image's edge (%d)"
                             % (name, e, o, MCU, size))
    # luma, then chroma (Cr's grid is Cb's; a gray file has none to leave)
    for c, ((bh, bw), (gh, gw), (by0, bx0)) in enumerate(zip(image.grids(), blocks_for(h, w), origins((y0, x0)))):
        if by0 + gh > bh or bx0 + gw > bw:
            raise ValueError("window (%d, %d, %d, %d): component %d: %d x %d blocks from (%d, %d) leave the file's grid of "
                             "%d x %d" % (y0, x0, h, w, c, gh, gw, by0, bx0, bh, bw))
    return y0, x0, h, w


def check_batch(images, windows=None, flips=None):
    """-> (windows, flips, (h, w)) of a batch: one window shape for all, origins and flips per image."""
    n = len(images)
    windows = [None] * n if windows is None else list(windows)
    flips = [False] * n if flips is None else [bool(f) for f in flips]
    if len(windows) != n or len(flips) != n:
        raise ValueError("expected one window and one flip per file (%d), got %d and %d" % (n, len(windows), len(flips)))
    windows = [check_window(im, win) for im, win in zip(images, windows)]
    shapes = sorted({win[2:] for win in windows})
    if len(shapes) != 1:
        raise ValueError("mixed window shapes in one batch: %s" % shapes)
    h, w = shapes[0]
    if any(flips) and w % MCU:
        raise ValueError("the mirror needs a window width that is a multiple of %d, got %d" % (MCU, w))
    return windows, flips, (h, w)


def origins(window):
    """Block origins ((by0, bx0) of luma, of chroma) of a window."""
    y0, x0 = window[:2]
    return (y0 // 8, x0 // 8), (y0 // 16, x0 // 16)


def raw_planes(image):
    """The file's raw (not de-quantised) int16 planes [(blocks_h, blocks_w, 64)] per component, read as the staging
    layer reads them (the batch reader refuses a truncated file, as Pillow does); ValueError for a file that fails."""
    grids = image.grids()
    sizes = [bh * bw * 64 for bh, bw in grids]
    offsets, caps = np.zeros((1, 4), dtype=np.int64), np.zeros((1, 4), dtype=np.int64)
    offsets[0, :len(sizes)] = 2 * np.concatenate([[0], np.cumsum(sizes)[:-1]])
    caps[0, :len(sizes)] = sizes
    out = np.zeros(2 * sum(sizes), dtype=np.uint8)
    if reader.read_raw_batch([image.data], out, offsets, caps, n_threads=1).any():
        raise ValueError("the file could not be read: %s" % reader.last_error())
    values = out.view(np.int16)
    return [values[o // 2:o // 2 + s].reshape(bh, bw, 64) for o, s, (bh, bw) in zip(offsets[0], sizes, grids)]


def dequantised(plane, table):
    """(..., 64) raw int16 coefficients and a (64,) table -> int16: the int32 product wrapped to int16."""
    return (np.asarray(plane).astype(np.int32) * np.asarray(table).astype(np.int32)).astype(np.int16)


def mirrored(blocks):
    """(..., cols, 64) int16 -> the lossless horizontal mirror: block columns reversed, odd-v coefficients negated in int16."""
    out = np.array(np.asarray(blocks, dtype=np.int16)[..., ::-1, :])
    out[..., 1::2] = (-out[..., 1::2].astype(np.int32)).astype(np.int16)
    return out


def window_blocks(plane, table, by0, bx0, rows, cols, flip=False):
    """The statement for one component: blocks [by0, by0 + rows) x [bx0, bx0 + cols) of a raw plane -> (rows, cols, 64)
    float32."""
    plane = np.asarray(plane)
    if by0 < 0 or bx0 < 0 or by0 + rows > plane.shape[0] or bx0 + cols > plane.shape[1]:
        raise ValueError("%d x %d blocks from (%d, %d) leave the plane of %d x %d" % ((rows, cols, by0, bx0) + plane.shape[:2]))
    v = dequantised(plane[by0:by0 + rows, bx0:bx0 + cols], table)
    return (mirrored(v) if flip else v).astype(np.float32)


def coefficient_inputs_host(files, windows=None, flips=None, deconv=False):
    """files: JPEG bytes or `CoefficientImage`s; windows: per file None or (y0, x0, h, w), one shape for the batch; flips:
    per file -> `[X_y, X_cbcr]`, or `[X_y, X_cb, X_cr]` when deconv=True, float32."""
    images = check_files(files)
    windows, flips, (h, w) = check_batch(images, windows, flips)
    (yh, yw), (ch, cw) = blocks_for(h, w)
    n = len(images)
    y, cb, cr = (np.zeros((n, yh, yw, 64), np.float32), np.zeros((n, ch, cw, 64), np.float32),
                 np.zeros((n, ch, cw, 64), np.float32))
    for i, (im, win, flip) in enumerate(zip(images, windows, flips)):
        planes, tables = raw_planes(im), im.tables()
        (ly, lx), (cy, cx) = origins(win)
        y[i] = window_blocks(planes[0], tables[0], ly, lx, yh, yw, flip)
        if im.n_components == 3:
            cb[i] = window_blocks(planes[1], tables[1], cy, cx, ch, cw, flip)
            cr[i] = window_blocks(planes[2], tables[2], cy, cx, ch, cw, flip)
    return [y, cb, cr] if deconv else [y, np.concatenate([cb, cr], axis=-1)]


# ---- the same numbers on the GPU ---------------------------------------------------------------------------------------------
class CoefficientPlan(ds.StagedPlan):
    """Descriptors, tables and the layout of one staging blob `[descriptors | tables | coefficient planes]`, every part
    and every plane at a multiple of 64 bytes.  Whole planes are staged, because the batch reader emits whole planes;
    the kernel reads only the window.  There are no pixels: nothing is staged but what the reader writes."""
    DESC_DTYPE = DESC_DTYPE
    scratch_bytes = 0
    out_shape = (0,)

    def __init__(self, images, windows, flips, grids):
        n = len(images)
        self.batch, self.grids = n, grids
        self.desc = np.zeros(n, dtype=DESC_DTYPE)
        self.tables = np.zeros((n, 3, 64), dtype=np.int32)
        self.plane_offsets = np.zeros((n, 4), dtype=np.int64)      # relative to the "coef" part
        self.plane_capacity = np.zeros((n, 4), dtype=np.int64)
        coef_off = 0
        for i, (im, win, flip) in enumerate(zip(images, windows, flips)):
            d = self.desc[i]
            d["table_offset"], d["n_components"], d["flip"] = 192 * i, im.n_components, int(flip)
            self.tables[i] = im.tables()
            luma, chroma = origins(win)
            for c, (bh, bw) in enumerate(im.grids()):
                d["blocks_h"][c], d["blocks_w"][c] = bh, bw
                d["by0"][c], d["bx0"][c] = luma if c == 0 else chroma
                d["coef_offset"][c] = coef_off
                self.plane_offsets[i, c], self.plane_capacity[i, c] = coef_off, bh * bw * 64
                coef_off += ds.round_up(bh * bw * 128)
        self.coef_bytes = coef_off
        self._lay_out([("desc", self.desc), ("tables", self.tables), ("coef", self.coef_bytes)])

    def fill(self, staging, images, n_threads=None):
        """Write descriptors and tables into `staging`, a uint8 numpy array of at least `nbytes`, and have `n_threads`
        host threads (None: one per CPU this process may use, 16 at the most) entropy-decode the files' raw planes into
        it; a file that fails there raises ValueError naming its index."""
        for offset, content in self.parts:
            staging[offset:offset + content.size] = content
        self._read_planes(staging, images, list(range(self.batch)), n_threads)

    def views(self, blob):
        """(descriptors, tables, coefficient planes) of a staging buffer (numpy: a DESC_DTYPE array, int32, bytes) or of
        its device copy (torch: bytes all three)."""
        desc = self.part(blob, self.desc_offset, self.desc, DESC_DTYPE)
        tables = self.part(blob, self.tables_offset, self.tables, np.int32)
        return desc, tables, blob[self.coef_offset:self.coef_offset + self.coef_bytes]

    def launch(self, blob_host, blob_dev, out, scratch=None, stream=None):
        """dj_jpeg_dct_inputs into `out` = [Y, CbCr] or [Y, Cb, Cr]: float32 CUDA tensors of the batch's shapes."""
        from .. import kernels
        desc_h, tables_h, _ = self.views(blob_host)
        desc_d, tables_d, coef_d = self.views(blob_dev)
        outs = tuple(out) if len(out) == 3 else (out[0], out[1][..., :64], out[1][..., 64:])
        kernels.jpeg_dct_inputs(coef_d, desc_d, desc_h, tables_d, tables_h, outs, stream=stream)
        return out


# dj_jpeg_entropy_desc and dj_jpeg_entropy_seg (include/dj_hip.h), C layout
ENTROPY_DTYPE = np.dtype([("plane_offset", np.int64, 3), ("plane_capacity", np.int64, 3)]
                         + [(n, np.int32, 3) for n in ("blocks_h", "blocks_w", "h_blocks", "v_blocks", "dc_table", "ac_table")]
                         + [(n, np.int32) for n in ("table_first", "n_components", "mcus_x", "mcus_y", "seg_first",
                                                    "n_segments")], align=True)
SEGMENT_DTYPE = np.dtype([("begin", np.int64), ("end", np.int64), ("file", np.int32), ("first_mcu", np.int32),
                          ("n_mcus", np.int32), ("reserved", np.int32)], align=True)


def segment_scan(image, unmarked=False):
    """The pre-pass's verdict and findings for a `CoefficientImage` (jpeg2dct/numpy.py:`scan_segments`), made once per
    file where its header is parsed and kept on the image.  `unmarked`: the wider pre-pass, which a file without restart
    intervals passes as one segment; it is run only for a file that fails the other one, whose findings it repeats
    otherwise."""
    scan = getattr(image, "_segment_scan", None)
    if scan is None:
        bh, bw = image.grids()[0]
        scan = image._segment_scan = reader.scan_segments(image.data, max_segments=bh * bw)
    if unmarked and not scan.entropy_decodable:
        scan = getattr(image, "_segment_scan_unmarked", None)
        if scan is None:
            scan = image._segment_scan_unmarked = reader.scan_segments(image.data, max_segments=1, unmarked=True)
    return scan


def entropy_records(scans, plane_offsets, file_offsets):
    """-> (ENTROPY_DTYPE descriptors, SEGMENT_DTYPE records, (n_tables, HUFF_BYTES) uint8 tables) of a batch of eligible
    files: plane_offsets[i][c] the byte offset of file i's plane c in the output buffer, file_offsets[i] that of its
    first byte in the bytes buffer.  File i's tables are the four from 4 i on (unused ones zero)."""
    n = len(scans)
    desc = np.zeros(n, dtype=ENTROPY_DTYPE)
    counts = np.array([s.n_segments for s in scans], dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    mcus = np.array([s.mcus for s in scans], dtype=np.int64)
    interval = np.array([s.restart_interval for s in scans], dtype=np.int64)
    desc["table_first"], desc["n_components"] = 4 * np.arange(n), [s.n_components for s in scans]
    desc["mcus_y"], desc["mcus_x"], desc["seg_first"], desc["n_segments"] = mcus[:, 0], mcus[:, 1], first, counts

    def per_component(values, absent=0):      # [[per component] per file] -> (n, 3), absent components 0
        return [tuple(v) + (absent,) * (3 - len(v)) for v in values]
    grids = np.array(per_component([s.grids for s in scans], (0, 0)), dtype=np.int64)            # (n, 3, 2)
    blocks = np.array(per_component([s.mcu_blocks for s in scans], (0, 0)), dtype=np.int64)
    desc["blocks_h"], desc["blocks_w"], desc["v_blocks"], desc["h_blocks"] = grids[..., 0], grids[..., 1], blocks[..., 0], blocks[..., 1]
    desc["dc_table"], desc["ac_table"] = per_component([s.dc_table for s in scans]), per_component([s.ac_table for s in scans])
    desc["plane_offset"] = np.asarray([tuple(o)[:3] for o in plane_offsets], dtype=np.int64) * (grids[..., 0] > 0)
    desc["plane_capacity"] = grids[..., 0] * grids[..., 1] * 64
    tables = np.concatenate([s.tables4 for s in scans])
    segs = np.zeros(int(counts.sum()), dtype=SEGMENT_DTYPE)
    ranges = np.concatenate([s.ranges for s in scans]) + np.repeat(np.asarray(file_offsets[:n], dtype=np.int64), counts)[:, None]
    segs["begin"], segs["end"], segs["file"] = ranges[:, 0], ranges[:, 1], np.repeat(np.arange(n), counts)
    segs["first_mcu"] = (np.arange(len(segs)) - np.repeat(first, counts)) * np.repeat(interval, counts)
    segs["n_mcus"] = np.minimum(np.repeat(interval, counts), np.repeat(mcus[:, 0] * mcus[:, 1], counts) - segs["first_mcu"])
    return desc, segs, tables


class EntropyCoefficientPlan(CoefficientPlan):
    """The plan of a batch whose files are all entropy-decodable on the GPU (restart intervals; `segment_scan`): one staging
    blob `[dj_jpeg_dct descriptors | quantisation tables | entropy descriptors | segment records | Huffman tables | file
    bytes]`, every part at a multiple of 64 bytes.  The raw coefficient planes are not uploaded: they live in the
    per-device scratch (`scratch_bytes`: every plane at a multiple of 64 bytes, then one int32 status per segment), where
    dj_jpeg_entropy_decode writes them from the files' bytes and dj_jpeg_dct_inputs reads them.  `fill` copies bytes and
    starts no thread."""

    def __init__(self, images, windows, flips, grids, scans):
        CoefficientPlan.__init__(self, images, windows, flips, grids)      # descriptors, tables, plane offsets
        self.file_offsets = np.concatenate([[0], np.cumsum([len(im.data) for im in images])]).astype(np.int64)
        self.entropy, self.segments, self.huffman = entropy_records(scans, self.plane_offsets, self.file_offsets)
        self.n_status = len(self.segments)
        self.status_offset = self.coef_bytes                               # in the scratch, behind the planes
        self.scratch_bytes = self.coef_bytes + 4 * self.n_status
        self._lay_out([("desc", self.desc), ("tables", self.tables), ("entropy", self.entropy), ("segments", self.segments),
                       ("huffman", self.huffman), ("bytes", int(self.file_offsets[-1]))])

    def fill(self, staging, images, n_threads=None):
        """Write descriptors, records, tables and the files' bytes into `staging`, a uint8 numpy array of at least
        `nbytes`.  Nothing is decoded here."""
        for offset, content in self.parts:
            staging[offset:offset + content.size] = content
        for im, at in zip(images, self.file_offsets + self.bytes_offset):
            staging[at:at + len(im.data)] = np.frombuffer(im.data, dtype=np.uint8)

    def entropy_views(self, blob):
        """(entropy descriptors, segment records, Huffman tables, file bytes) of a staging buffer or of its device copy."""
        desc = self.part(blob, self.entropy_offset, self.entropy, ENTROPY_DTYPE)
        segs = self.part(blob, self.segments_offset, self.segments, SEGMENT_DTYPE)
        huff = self.part(blob, self.huffman_offset, self.huffman)
        if isinstance(blob, np.ndarray):
            huff = huff.reshape(self.huffman.shape)
        return desc, segs, huff, blob[self.bytes_offset:self.bytes_offset + int(self.file_offsets[-1])]

    def views(self, blob):
        """(descriptors, tables) of dj_jpeg_dct_inputs in a staging buffer or its device copy; the planes are in the scratch."""
        return (self.part(blob, self.desc_offset, self.desc, DESC_DTYPE), self.part(blob, self.tables_offset, self.tables, np.int32),
                None)

    def status_view(self, scratch):
        """The int32 statuses, one per segment, where `launch` had them written in `scratch`."""
        import torch
        return scratch[self.status_offset:self.status_offset + 4 * self.n_status].view(torch.int32)

    def launch(self, blob_host, blob_dev, out, scratch=None, stream=None):
        """dj_jpeg_entropy_decode into `scratch` (a 1-D uint8 CUDA tensor of at least `scratch_bytes`, 16-byte aligned),
        then dj_jpeg_dct_inputs from it into `out`."""
        from .. import kernels
        if scratch is None or scratch.numel() < self.scratch_bytes:
            raise ValueError("this plan needs %d bytes of device scratch" % self.scratch_bytes)
        desc_h, tables_h, _ = self.views(blob_host)
        desc_d, tables_d, _ = self.views(blob_dev)
        edesc_h, segs_h, huff_h, _ = self.entropy_views(blob_host)
        edesc_d, segs_d, huff_d, bytes_d = self.entropy_views(blob_dev)
        planes = scratch[:self.coef_bytes]
        kernels.jpeg_entropy_decode(bytes_d, edesc_d, edesc_h, segs_d, segs_h, huff_d, huff_h, planes, self.status_view(scratch),
                                    stream=stream)
        outs = tuple(out) if len(out) == 3 else (out[0], out[1][..., :64], out[1][..., 64:])
        kernels.jpeg_dct_inputs(planes, desc_d, desc_h, tables_d, tables_h, outs, stream=stream)
        return out

    def failures(self, status, images):
        """The text naming the files whose segments failed, from the plan's downloaded statuses; None when all are 0."""
        from .entropy_decode import STATUS_TEXT
        status = np.asarray(status)[:self.n_status]
        if not status.any():
            return None
        bad = []
        for i, d in enumerate(self.entropy):
            mine = status[d["seg_first"]:d["seg_first"] + d["n_segments"]]
            if mine.any():
                k = int(np.flatnonzero(mine)[0])
                bad.append("file %d%s: segment %d: %s" % (i, " (%s)" % images[i].name if getattr(images[i], "name", None) else "",
                                                          k, STATUS_TEXT.get(int(mine[k]), "status %d" % mine[k])))
        return "entropy decoding on the GPU failed for " + "; ".join(bad)


DEFAULT_CHUNK_BYTES = 512      # the lowest kernel time of 64 / 128 / 256 / 512 on the measured batch


def chunk_counts(segments, chunk_bytes):
    """The chunks of every record of a SEGMENT_DTYPE array: max(1, ceil((end - begin) / chunk_bytes))."""
    return np.maximum(1, -(-(segments["end"] - segments["begin"]) // int(chunk_bytes))).astype(np.int64)


def fill_chunks(desc, segs, chunk_bytes):
    """Write every record's first chunk -- the number of chunks of the records in front of it -- into its `reserved`, as
    dj_jpeg_entropy_decode_chunked reads it -> (chunks in all, blocks in all: the files' MCUs times their blocks per MCU,
    MCU padding included)."""
    counts = chunk_counts(segs, chunk_bytes)
    segs["reserved"] = np.concatenate([[0], np.cumsum(counts)[:-1]])
    per_mcu = (desc["h_blocks"] * desc["v_blocks"] * (np.arange(3)[None, :] < desc["n_components"][:, None])).sum(axis=1)
    return int(counts.sum()), int((desc["mcus_x"].astype(np.int64) * desc["mcus_y"] * per_mcu).sum())


def chunked_records(scans, plane_offsets, file_offsets, chunk_bytes):
    """`entropy_records` with `fill_chunks` applied -> (descriptors, records, tables, chunks in all, blocks in all)."""
    desc, segs, tables = entropy_records(scans, plane_offsets, file_offsets)
    return (desc, segs, tables) + fill_chunks(desc, segs, chunk_bytes)


def chunked_scratch_bytes(n_chunks, n_files, n_segments, n_blocks):
    """dj_jpeg_entropy_chunked_scratch_bytes (include/dj_hip.h): chunk records of 32 bytes, a first block per file, a
    failing block per segment and a DC difference per block, each part rounded up to 16 bytes."""
    return sum(ds.round_up(n, 16) for n in (32 * n_chunks, 8 * n_files, 4 * n_segments, 2 * n_blocks))


class ChunkedEntropyCoefficientPlan(EntropyCoefficientPlan):
    """The plan of a batch with files that carry no restart intervals, all eligible by `segment_scan(unmarked=True)`: the
    staging blob of `EntropyCoefficientPlan` (the records' `reserved` holding each segment's first chunk), and a scratch of
    `[planes | one int32 status per segment | chunk states, first blocks, failing blocks and DC differences]`, the last
    part at a multiple of 64 bytes, where dj_jpeg_entropy_decode_chunked works (data/entropy_decode.py states the scheme)."""

    def __init__(self, images, windows, flips, grids, scans, chunk_bytes=DEFAULT_CHUNK_BYTES):
        from .entropy_decode import check_chunk_bytes
        self.chunk_bytes = check_chunk_bytes(chunk_bytes)
        EntropyCoefficientPlan.__init__(self, images, windows, flips, grids, scans)
        # the records are laid out by reference: filling `reserved` here reaches the blob
        self.n_chunks, self.n_blocks = fill_chunks(self.entropy, self.segments, self.chunk_bytes)
        self.work_offset = ds.round_up(self.status_offset + 4 * self.n_status)
        self.work_bytes = chunked_scratch_bytes(self.n_chunks, self.batch, self.n_status, self.n_blocks)
        self.scratch_bytes = self.work_offset + self.work_bytes

    def launch(self, blob_host, blob_dev, out, scratch=None, stream=None):
        """dj_jpeg_entropy_decode_chunked into `scratch` (a 1-D uint8 CUDA tensor of at least `scratch_bytes`, 16-byte
        aligned), then dj_jpeg_dct_inputs from it into `out`."""
        from .. import kernels
        if scratch is None or scratch.numel() < self.scratch_bytes:
            raise ValueError("this plan needs %d bytes of device scratch" % self.scratch_bytes)
        desc_h, tables_h, _ = self.views(blob_host)
        desc_d, tables_d, _ = self.views(blob_dev)
        edesc_h, segs_h, huff_h, _ = self.entropy_views(blob_host)
        edesc_d, segs_d, huff_d, bytes_d = self.entropy_views(blob_dev)
        planes = scratch[:self.coef_bytes]
        kernels.jpeg_entropy_decode_chunked(bytes_d, edesc_d, edesc_h, segs_d, segs_h, huff_d, huff_h, planes,
                                            self.status_view(scratch), self.chunk_bytes,
                                            scratch[self.work_offset:self.work_offset + self.work_bytes], stream=stream)
        outs = tuple(out) if len(out) == 3 else (out[0], out[1][..., :64], out[1][..., 64:])
        kernels.jpeg_dct_inputs(planes, desc_d, desc_h, tables_d, tables_h, outs, stream=stream)
        return out


def chunkable(scans, chunk_bytes):
    """Whether every segment of these eligible scans stays within the chunk cap (entropy_decode.MAX_CHUNKS)."""
    from .entropy_decode import MAX_CHUNKS
    return all(int((s.ranges[:, 1] - s.ranges[:, 0]).max()) <= MAX_CHUNKS * int(chunk_bytes) for s in scans)


class PendingCoefficientInputs(PendingInputs):
    """The files of one batch with their windows and mirrors, on their way into a model's resident input buffers
    (`Model.train_on_batch / predict / fit_generator` accept it where they accept the list of input arrays): at upload time
    the files' raw planes are entropy-decoded into pinned memory, one copy takes `[descriptors | tables | planes]` up
    and one launch of dj_jpeg_dct_inputs writes the inputs.  `shape` is that of the pixel batch the windows stand for.
    With an emitter whose `device_entropy` is set and a batch whose files are ALL entropy-decodable on the GPU, the files'
    bytes go up instead and dj_jpeg_entropy_decode makes the planes there (`EntropyCoefficientPlan`); a batch with any
    other file takes the host path whole, and the emitter's `host_batches` counts it.  With `unmarked` set as well, a batch
    with files that carry no restart intervals, all eligible by the wider pre-pass and within the chunk cap, takes
    `ChunkedEntropyCoefficientPlan` in front of the host path."""

    def __init__(self, emitter, files, windows=None, flips=None, _count=True):
        self.images = check_files(files)
        self.windows, self.flips, (h, w) = check_batch(self.images, windows, flips)
        # descriptors and layout are made where the batch is made (a generator's prefetch thread), not at upload time
        scans = [segment_scan(im) for im in self.images] if getattr(emitter, "device_entropy", False) else None
        wider = None
        if scans is not None and getattr(emitter, "unmarked", False) and not all(s.entropy_decodable for s in scans):
            wider = [segment_scan(im, unmarked=True) for im in self.images]
            if not (all(s.entropy_decodable for s in wider) and chunkable(wider, emitter.chunk_bytes)):
                wider = None
        if scans is not None and all(s.entropy_decodable for s in scans):
            self.plan = EntropyCoefficientPlan(self.images, self.windows, self.flips, blocks_for(h, w), scans)
        elif wider is not None:
            self.plan = ChunkedEntropyCoefficientPlan(self.images, self.windows, self.flips, blocks_for(h, w), wider,
                                                      emitter.chunk_bytes)
        else:
            self.plan = CoefficientPlan(self.images, self.windows, self.flips, blocks_for(h, w))
            if scans is not None and _count:
                emitter.host_batches += 1
        PendingInputs.__init__(self, emitter, (len(self.images), h, w, 3))

    def sliced(self, index):
        return PendingCoefficientInputs(self.emitter, self.images[index], self.windows[index], self.flips[index], _count=False)

    def emit_into(self, buffers):
        """One copy and one launch on the current stream, writing every element of `buffers`: float32 CUDA tensors of
        `self.shapes` ([Y, CbCr] or [Y, Cb, Cr])."""
        buffers = list(buffers)
        if [tuple(t.shape) for t in buffers] != [tuple(s) for s in self.shapes]:
            raise ValueError("emit_into: expected buffers of shapes %s, got %s"
                             % (self.shapes, [tuple(t.shape) for t in buffers]))
        return self.emitter.run(self.plan, self.images, buffers[0].device, out=buffers)

    def numpy(self):
        """The same inputs computed on the host: the statement."""
        return coefficient_inputs_host(self.images, self.windows, self.flips, self.emitter.deconv)


class DeviceCoefficientInputs(ds.StagingBuffers):
    """Stands where a generator would decode a pre-sized file, crop it and encode it again: the generator thread reads
    bytes and headers and draws, and the file's own coefficients reach the model's inputs through the `StagingBuffers` kept
    here (two pinned buffers used in turn, the event behind the copy, the device blob grown on demand).  `n_threads`: host
    threads that entropy-decode a batch (None: `StagedPlan.fill`'s default).  `device_entropy`: batches whose files all carry
    restart intervals are entropy-decoded on the GPU (no host thread, the files' bytes are what goes up); `host_batches`
    counts the batches that took the host path instead.  `unmarked` (needs `device_entropy`): batches with files that carry
    no restart intervals are entropy-decoded on the GPU too, by chunks of `chunk_bytes` raw bytes (None:
    DEFAULT_CHUNK_BYTES), when every file passes the wider pre-pass; only the rest counts as `host_batches`.  A segment that fails on the GPU cannot raise where the batch is
    emitted without a stall: its status reaches the host behind the batch, and the ValueError naming the file is raised
    when the staging slot is next used, or by `check`."""

    def __init__(self, deconv=False, n_threads=None, device_entropy=False, unmarked=False, chunk_bytes=None):
        from .entropy_decode import check_chunk_bytes
        if unmarked and not device_entropy:
            raise ValueError("unmarked=True needs device_entropy=True: it widens what is entropy-decoded on the GPU")
        self.deconv = bool(deconv)
        self.device_entropy = bool(device_entropy)
        self.unmarked = bool(unmarked)
        self.chunk_bytes = check_chunk_bytes(DEFAULT_CHUNK_BYTES if chunk_bytes is None else chunk_bytes)
        self.host_batches = 0
        ds.StagingBuffers.__init__(self, n_threads)

    def check(self, device=None):
        """Wait for what was emitted on `device` (None: every device used) and raise the ValueError of a batch whose
        entropy decoding failed there.  For the end of a sweep, a tool or a test."""
        import torch
        for name in ([str(torch.device(device))] if device is not None else list(self._state)):
            if name in self._state:
                torch.cuda.synchronize(torch.device(name))
                for slot in self._state[name]["slots"]:
                    self._check_slot(slot)

    def __call__(self, files, windows=None, flips=None):
        return PendingCoefficientInputs(self, files, windows, flips)
