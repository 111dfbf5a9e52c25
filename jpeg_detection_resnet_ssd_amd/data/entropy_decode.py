"""Huffman entropy decoding of a baseline JPEG file one restart interval ("segment") at a time: the statement that
csrc/dj_jpeg_entropy.hip (`kernels.jpeg_entropy_decode`) follows bit for bit.  Plain Python and numpy, slow, for tests.

A segment is the entropy-coded bytes between two restart markers (jpeg2dct/numpy.py:`scan_segments` finds them without
decoding anything): it is byte-aligned, starts with every DC predictor at 0 and can be decoded on its own.

Bit source: the bytes of the segment's range; `FF 00` yields `FF`; `FF` followed by anything else, or by the range's end,
ends the data (the pre-pass never hands over such a range, a corrupted one can contain it).  Bits past the end read as 0.
Short segment: CONSUMING a bit past the end -- skipping it after a code matched, or receiving it as a magnitude bit -- is
status 4; peeking is not an error.
DC: the canonical Huffman symbol s; no code of 16 bits or fewer, or s > 11, is status 1; diff = extend(receive(s), s); the
predictor is int32, 0 at the segment's start; int16(predictor) is stored.
AC: the symbol rs; no code is status 2; r = rs >> 4, s = rs & 15; s == 0 and r != 15 ends the block; s == 0 and r == 15 adds
16 to k; otherwise k += r, k > 63 is status 3, else block[natural[k]] = int16(extend(receive(s), s)) and k += 1.
Blocks are walked in MCU order with the scan's blocks per MCU; a block outside the component's logical grid (MCU padding)
is decoded and dropped; a block is written only when complete.  The first error of a segment is its status; the failing
block and every later block of that segment stay zero; other segments are unaffected; bytes left over are ignored.
Every loop is bounded: 63 AC symbols per block, 16 bits per symbol, restart_interval * blocks-per-MCU blocks per segment."""
import numpy as np

from ..jpeg2dct import numpy as reader

OK, BAD_DC, BAD_AC, AC_OVERRUN, SHORT = 0, 1, 2, 3, 4
STATUS_TEXT = {OK: "ok", BAD_DC: "corrupt DC code", BAD_AC: "corrupt AC code", AC_OVERRUN: "AC run past the block end",
               SHORT: "the segment's data ends before its last block"}

# zig-zag position -> natural (row-major) index, T.81 figure A.6
NATURAL = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
           28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
           54, 47, 55, 62, 63)

COUNTERS = ("stuffed", "long_codes", "zrl", "eob", "full_blocks", "max_dc_category", "padding_blocks")


class _Error(Exception):
    pass


def huffman_tables(data):
    """The DHT segments in front of the first scan and the scan's selectors, parsed here (not taken from the pre-pass):
    -> ({(class, id): {(length, code): symbol}}, [(dc id, ac id)] per scan component)."""
    data = bytes(data)
    tables, p = {}, 2
    while p + 4 <= len(data):
        if data[p] != 0xFF:
            p += 1
            continue
        m = data[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            p += 2
            continue
        length = (data[p + 2] << 8) | data[p + 3]
        body = data[p + 4:p + 2 + length]
        if m == 0xC4:
            q = 0
            while q + 17 <= len(body):
                counts = body[q + 1:q + 17]
                symbols = body[q + 17:q + 17 + sum(counts)]
                codes, code, k = {}, 0, 0
                for l in range(1, 17):
                    for _ in range(counts[l - 1]):
                        codes[(l, code)] = symbols[k]
                        code, k = code + 1, k + 1
                    code <<= 1
                tables[(body[q] >> 4, body[q] & 15)] = codes
                q += 17 + sum(counts)
        elif m == 0xDA:
            return tables, [(body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(body[0])]
        p += 2 + length
    raise ValueError("no scan header")


class _Bits(object):
    def __init__(self, data, begin, end, counters):
        out = bytearray()
        p = begin
        while p < end:
            b = data[p]
            if b == 0xFF:
                if p + 1 < end and data[p + 1] == 0x00:
                    counters["stuffed"] += 1
                    p += 2
                else:
                    break
            else:
                p += 1
            out.append(b)
        self.total = 8 * len(out)
        self.value = int.from_bytes(bytes(out) + b"\0\0\0\0", "big")      # 32 zero bits behind the data
        self.width = self.total + 32
        self.pos = 0

    def peek(self, n):
        """The next n <= 16 bits, zeros past the end; nothing is consumed."""
        pos = min(self.pos, self.total + 16)
        return (self.value >> (self.width - pos - n)) & ((1 << n) - 1)

    def consume(self, n):
        self.pos += n
        if self.pos > self.total:
            raise _Error(SHORT)

    def receive(self, n):
        if n == 0:
            return 0
        v = self.peek(n)
        self.consume(n)
        return v


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _symbol(bits, codes, status, counters):
    for l in range(1, 17):
        sym = codes.get((l, bits.peek(l)))
        if sym is not None:
            if l > 9:
                counters["long_codes"] += 1
            bits.consume(l)
            return sym
    raise _Error(status)


def _int16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def _block(bits, dc, ac, pred, counters):
    blk = [0] * 64
    s = _symbol(bits, dc, BAD_DC, counters)
    if s > 11:
        raise _Error(BAD_DC)
    counters["max_dc_category"] = max(counters["max_dc_category"], s)
    pred += _extend(bits.receive(s), s)
    pred = ((pred + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    blk[0] = _int16(pred)
    k = 1
    for _ in range(63):                      # at most 63 AC symbols: each adds at least 1 to k
        if k >= 64:
            break
        rs = _symbol(bits, ac, BAD_AC, counters)
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r != 15:
                counters["eob"] += 1
                break
            counters["zrl"] += 1
            k += 16
            continue
        k += r
        if k > 63:
            raise _Error(AC_OVERRUN)
        blk[NATURAL[k]] = _int16(_extend(bits.receive(s), s))
        if k == 63:
            counters["full_blocks"] += 1     # the block ends at its last coefficient, without an end-of-block symbol
        k += 1
    return blk, pred


def entropy_decode_host(data, segments=None, counters=None):
    """data: the file's bytes; segments: the `SegmentScan` whose geometry, ranges and table selectors to decode with (None:
    `scan_segments(data)`; a corrupted copy of a file is decoded with the scan of the original) -> (planes, status): the raw
    int16 planes [(blocks_h, blocks_w, 64)] per component in natural order -- what `read_raw_batch` writes -- and an int32
    status per segment.  `counters`: a dict that receives how often each path was taken (COUNTERS)."""
    data = bytes(data)
    scan = reader.scan_segments(data) if segments is None else segments
    if not scan.entropy_decodable:
        raise ValueError("not entropy-decodable by segments: %s" % scan.reason)
    counters = {} if counters is None else counters
    for name in COUNTERS:
        counters.setdefault(name, 0)
    tables, selectors = huffman_tables(data)
    planes = [np.zeros((bh, bw, 64), dtype=np.int16) for bh, bw in scan.grids]
    status = np.zeros(scan.n_segments, dtype=np.int32)
    n_mcus = scan.mcus[0] * scan.mcus[1]
    for seg, (begin, end) in enumerate(scan.ranges):
        bits = _Bits(data, int(begin), int(end), counters)
        pred = [0] * scan.n_components
        first = seg * scan.restart_interval
        try:
            for mcu in range(first, min(first + scan.restart_interval, n_mcus)):
                my, mx = divmod(mcu, scan.mcus[1])
                for c, ((v, h), (bh, bw), (td, ta)) in enumerate(zip(scan.mcu_blocks, scan.grids, selectors)):
                    for by in range(v):
                        for bx in range(h):
                            blk, pred[c] = _block(bits, tables[(0, td)], tables[(1, ta)], pred[c], counters)
                            row, col = my * v + by, mx * h + bx
                            if row < bh and col < bw:
                                planes[c][row, col] = blk
                            else:
                                counters["padding_blocks"] += 1
        except _Error as e:
            status[seg] = e.args[0]
    return planes, status
