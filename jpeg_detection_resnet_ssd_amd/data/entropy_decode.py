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
Every loop is bounded: 63 AC symbols per block, 16 bits per symbol, restart_interval * blocks-per-MCU blocks per segment.

`chunked_decode_host` (below) is the model of the parallel scheme that csrc/dj_jpeg_entropy_chunked.hip
(`kernels.jpeg_entropy_decode_chunked`) runs for files without restart intervals; it states no result of its own: its planes
and statuses are those of `entropy_decode_host` with the scan of `scan_segments(data, unmarked=True)`."""
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
        self.raw = []                      # the raw index of every data byte, for the chunked scheme's positions
        while p < end:
            b = data[p]
            self.raw.append(p)
            if b == 0xFF:
                if p + 1 < end and data[p + 1] == 0x00:
                    counters["stuffed"] += 1
                    p += 2
                else:
                    self.raw.pop()
                    break
            else:
                p += 1
            out.append(b)
        self.stop = p                      # where the data ends: the range's end or a marker
        self.total = 8 * len(out)
        self.bytes = bytes(out) + b"\0" * 8                                  # zero bits behind the data
        self.pos = 0

    def peek(self, n):
        """The next n <= 16 bits, zeros past the end; nothing is consumed."""
        pos = min(self.pos, self.total + 16)
        window = int.from_bytes(self.bytes[pos >> 3:(pos >> 3) + 4], "big")
        return (window >> (32 - (pos & 7) - n)) & ((1 << n) - 1)

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


# ---- the same result by chunks: the statement csrc/dj_jpeg_entropy_chunked.hip follows ---------------------------------------
# A segment without restart markers inside is cut every `chunk_bytes` raw bytes.  A position is 8 * raw byte index + bit and
# never points into a stuffed 00; a decoder state is (position, u, k, status): u the block's index within the MCU, k = 0
# before the DC symbol and 1..63 inside the AC symbols.  A symbol (code and magnitude bits) belongs to the chunk in which
# its first bit lies; a chunk decodes, from its entry state, every symbol that starts before its end (its bit source runs
# on to the segment's end), and records its exit state and the blocks it completed.  An entry at or past the chunk's end
# (the segment's end for the last chunk) gives exit = entry and no block; a status != 0 freezes the state at the failing symbol's start.  Chunk 0 enters at the
# segment's start, every other chunk first at its guess (bit 0 of its first byte, of the next one if that byte is a stuffed
# 00) and then at its predecessor's exit, decoding again only when that differs from the entry it last used, until a round
# changes nothing: chunk c is right after at most c rounds, and the fixed point is the sequential decode.  A prefix sum of
# the completed blocks gives every chunk its first block; a final pass decodes every chunk once more from its true entry,
# stops at the segment's last block (the last chunk has no end: it runs past the data as the sequential decoder does),
# writes AC coefficients to the planes and DC differences by segment-wide block index (padding blocks included); a third
# pass sums the differences per component in scan order (int32 wrap-around, stored as int16), writes position 0 of every
# stored block and clears the block the segment failed in.  The segment's status is the first error met before its last
# block completes; errors in bytes left over are never met.
CHUNK_BYTES_MIN, CHUNK_BYTES_MAX, MAX_CHUNKS, SYNC_LANES = 16, 4096, 65536, 256
CHUNK_COUNTERS = ("chunks", "empty_chunks", "stuffed_first_byte", "entry_past_end", "speculative_errors", "late_redecodes",
                  "blocks_over_three_chunks", "segments_wider_than_a_workgroup", "leftover_errors", "max_rounds")


def check_chunk_bytes(chunk_bytes):
    chunk_bytes = int(chunk_bytes)
    if chunk_bytes % 16 or not CHUNK_BYTES_MIN <= chunk_bytes <= CHUNK_BYTES_MAX:
        raise ValueError("chunk_bytes must be a multiple of 16 in %d..%d, got %d" % (CHUNK_BYTES_MIN, CHUNK_BYTES_MAX, chunk_bytes))
    return chunk_bytes


def chunk_count(begin, end, chunk_bytes):
    """Chunks of the byte range [begin, end): at least one."""
    return max(1, -(-(int(end) - int(begin)) // int(chunk_bytes)))


class _ChunkBits(_Bits):
    """The segment's bit source, addressed by positions."""

    def __init__(self, data, begin, end):
        _Bits.__init__(self, data, begin, end, {"stuffed": 0})
        self.index = {r: i for i, r in enumerate(self.raw)}

    def seek(self, position):
        """Continue at a position; one that is no data byte's (behind a marker of a corrupted range) is the data's end."""
        byte = self.index.get(position >> 3)
        self.pos = self.total if byte is None else 8 * byte + (position & 7)

    def position(self):
        return 8 * self.raw[self.pos >> 3] + (self.pos & 7) if self.pos < self.total else 8 * self.stop


def _symbol_step(bits, tables, u, k, on_dc=None, on_ac=None):
    """One symbol with its magnitude bits from state (u, k) -> (k', whether the block is complete); _Error as `_block`."""
    dc, ac = tables[u]
    quiet = {"long_codes": 0}
    if k == 0:
        s = _symbol(bits, dc, BAD_DC, quiet)
        if s > 11:
            raise _Error(BAD_DC)
        diff = _extend(bits.receive(s), s)
        if on_dc is not None:
            on_dc(diff)
        return 1, False
    rs = _symbol(bits, ac, BAD_AC, quiet)
    r, s = rs >> 4, rs & 15
    if s == 0:
        if r != 15:
            return 0, True
        k += 16
    else:
        k += r
        if k > 63:
            raise _Error(AC_OVERRUN)
        v = _int16(_extend(bits.receive(s), s))
        if on_ac is not None:
            on_ac(k, v)
        k += 1
    return (0, True) if k >= 64 else (k, False)


def _decode_chunk(bits, tables, entry, limit, first_block=0, last_block=None, on_dc=None, on_ac=None, on_block=None):
    """Every symbol from `entry` that starts before position `limit` (None: no end) -> (exit state, blocks completed, the
    index of the block an error was met in or None).  With `last_block` it stops when that many blocks are complete."""
    position, u, k, status = entry
    if status != 0 or (limit is not None and position >= limit):
        return entry, 0, None
    bits.seek(position)
    bpm, blocks = len(tables), 0
    while True:
        position = bits.position()
        if (limit is not None and position >= limit) or (last_block is not None and first_block + blocks >= last_block):
            return (position, u, k, 0), blocks, None
        index = first_block + blocks
        try:
            k, complete = _symbol_step(bits, tables, u, k, on_dc and (lambda d: on_dc(index, d)),
                                       on_ac and (lambda kk, v: on_ac(index, kk, v)))
        except _Error as e:
            return (position, u, k, e.args[0]), blocks, index
        if complete:
            if on_block is not None:
                on_block(index)
            u, blocks = (u + 1) % bpm, blocks + 1


def chunked_decode_host(data, scan, chunk_bytes, counters=None):
    """The planes and statuses of `entropy_decode_host(data, scan)` by the chunked scheme above: `scan` from
    `scan_segments(data, unmarked=True)` (a corrupted copy is decoded with the scan of the original) -> (planes, status,
    rounds): rounds[s] the synchronisation rounds segment s took, at most its chunk count.  `counters`: a dict that
    receives how often each path of the scheme was taken (CHUNK_COUNTERS)."""
    data = bytes(data)
    chunk_bytes = check_chunk_bytes(chunk_bytes)
    if not scan.entropy_decodable:
        raise ValueError("not entropy-decodable by segments: %s" % scan.reason)
    counters = {} if counters is None else counters
    for name in CHUNK_COUNTERS:
        counters.setdefault(name, 0)
    huff, selectors = huffman_tables(data)
    tables, where = [], []                           # per block of the MCU: its (DC, AC) tables; (component, down, across)
    for c, ((v, h), (td, ta)) in enumerate(zip(scan.mcu_blocks, selectors)):
        for by in range(v):
            for bx in range(h):
                tables.append((huff[(0, td)], huff[(1, ta)]))
                where.append((c, by, bx))
    bpm = len(tables)
    planes = [np.zeros((bh, bw, 64), dtype=np.int16) for bh, bw in scan.grids]
    status = np.zeros(scan.n_segments, dtype=np.int32)
    rounds = np.zeros(scan.n_segments, dtype=np.int32)
    n_mcus = scan.mcus[0] * scan.mcus[1]

    def stored(first_mcu, index):                    # segment-wide block index -> (component, row, col) or None (padding)
        my, mx = divmod(first_mcu + index // bpm, scan.mcus[1])
        c, by, bx = where[index % bpm]
        row, col = my * scan.mcu_blocks[c][0] + by, mx * scan.mcu_blocks[c][1] + bx
        return (c, row, col) if row < scan.grids[c][0] and col < scan.grids[c][1] else None

    for seg, (begin, end) in enumerate(scan.ranges):
        begin, end = int(begin), int(end)
        n = chunk_count(begin, end, chunk_bytes)
        if n > MAX_CHUNKS:
            raise ValueError("segment %d: %d chunks of %d bytes, more than %d" % (seg, n, chunk_bytes, MAX_CHUNKS))
        first_mcu = seg * scan.restart_interval
        total = (min(first_mcu + scan.restart_interval, n_mcus) - first_mcu) * bpm
        bits = _ChunkBits(data, begin, end)
        # the last chunk ends with the segment while the chunks synchronise, and has no end in the final pass
        limits = [8 * min(begin + (c + 1) * chunk_bytes, end) for c in range(n)]
        counters["chunks"] += n
        counters["segments_wider_than_a_workgroup"] += n > SYNC_LANES
        # ---- synchronisation: entry[c], exit[c], blocks[c]
        entry = [(8 * begin, 0, 0, 0)]
        for c in range(1, n):
            at = begin + c * chunk_bytes
            stuffed = data[at] == 0x00 and data[at - 1] == 0xFF
            counters["stuffed_first_byte"] += stuffed
            entry.append((8 * (at + stuffed), 0, 0, 0))
        exits, blocks = [None] * n, [0] * n

        def decode(c, speculative):
            exits[c], blocks[c], _ = _decode_chunk(bits, tables, entry[c], limits[c])
            counters["entry_past_end"] += entry[c][3] == 0 and entry[c][0] >= limits[c]
            counters["speculative_errors"] += speculative and exits[c][3] != 0 and entry[c][3] == 0
        for c in range(n):
            decode(c, c > 0)
        for r in range(1, n + 1):                    # bounded by the chunk count; the last round changes nothing
            dirty = [c for c in range(1, n) if exits[c - 1] != entry[c]]
            if not dirty:
                break
            assert r < n, "no fixed point within the chunk count"
            rounds[seg] = r
            for c in dirty:
                entry[c] = exits[c - 1]
            for c in dirty:
                decode(c, False)
            counters["late_redecodes"] += len(dirty) if r >= 2 else 0
        counters["max_rounds"] = max(counters["max_rounds"], int(rounds[seg]))
        counters["empty_chunks"] += sum(b == 0 for b in blocks)
        first = [0] * n                              # exclusive prefix sum
        for c in range(1, n):
            first[c] = first[c - 1] + blocks[c - 1]
        # ---- final pass: AC coefficients to the planes, DC differences by block index
        diffs, bad, started = {}, total, {}

        def on_ac(index, k, v):
            at = stored(first_mcu, index)
            if at is not None:
                planes[at[0]][at[1], at[2], NATURAL[k]] = v
        for c in range(n):
            def on_dc(index, d, c=c):
                diffs[index] = d
                started[index] = c

            def on_block(index, c=c):
                counters["blocks_over_three_chunks"] += c - started[index] >= 2
            state, _, failed = _decode_chunk(bits, tables, entry[c], limits[c] if c + 1 < n else None, first[c], total,
                                             on_dc, on_ac, on_block)
            if failed is not None and entry[c][3] == 0:
                status[seg], bad = state[3], failed
        counters["leftover_errors"] += status[seg] == 0 and any(e[3] != 0 for e in exits)
        # ---- DC pass: predictors per component in scan order; the failing block is cleared
        pred = [0] * scan.n_components
        for index in range(total):
            at = stored(first_mcu, index)
            if index >= bad:
                if index == bad and at is not None:
                    planes[at[0]][at[1], at[2]] = 0
                continue
            c = where[index % bpm][0]
            pred[c] = ((pred[c] + diffs[index] + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
            if at is not None:
                planes[at[0]][at[1], at[2], 0] = _int16(pred[c])
    return planes, status, rounds
