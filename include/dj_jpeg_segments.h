/* dj_jpeg_segments.h -- C ABI of the host pre-pass of entropy decoding on the GPU (host code, libdj_jpeg.so): where a file's
 * restart intervals lie and its Huffman tables in the form the kernel reads.  Included by dj_jpeg_decode.h, whose conventions
 * hold: 0 or a negative code, text via dj_jpeg_last_error() (thread-local), thread-safe. */
#ifndef DJ_JPEG_SEGMENTS_H
#define DJ_JPEG_SEGMENTS_H

#include "dj_jpeg_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- For entropy-decoding restart-interval files on the GPU (data/entropy_decode.py states it, csrc/dj_jpeg_entropy.hip
 * runs it).  dj_jpeg_scan_segments parses headers and looks for 0xFF bytes in the entropy-coded data; it never decodes a
 * Huffman code.  The verdict `entropy_decodable` holds when the file is `device_decodable`, exactly one sequential scan
 * names all its components in frame order (a gray file: its one-component scan, one block per MCU over the logical
 * grid), every Huffman table the scan selects was defined before it and there are at most four of them, DRI > 0, the
 * entropy-coded data holds exactly ceil(n_mcus / Ri) - 1 restart markers in the cyclic order RST0..RST7 and no other
 * FF xx but FF 00, and the scan is followed by EOI.  Anything else -- a file the reader cannot parse and every proper
 * prefix of a file included -- is "not eligible" with `reason` set, never an error: the return value is 0 unless an
 * argument is null.
 * For an eligible file: the restart interval, the MCU grid, the blocks per MCU of each component, the index (0..3) of
 * each component's DC and AC table among `tables`, and segment s's entropy-coded bytes [ranges[2 s], ranges[2 s + 1]) as
 * offsets into the file, markers excluded -- written only when range_capacity (in segments) >= n_segments, so a first call
 * with range_capacity 0 asks for the count (n_segments <= the number of MCUs).
 * A table in device form is DJ_JPEG_HUFF_BYTES bytes, built from the same DHT data as the reader's own:
 *   uint16 lut[256]    on the next 8 bits: (length << 8) | symbol of a code of 8 bits or fewer, 0 for a longer one;
 *   int32  limit[16]   limit[l - 1] = (first code of length l + number of codes of length l) << (16 - l): with the next 16
 *                      bits as a number `look`, the code's length is the first l with look < limit[l - 1];
 *   int32  offset[16]  offset[l - 1] = index of the first symbol of length l - first code of length l;
 *   uint8  symbols[256]  the symbol of code c of length l is symbols[c + offset[l - 1]]. ---- */
#define DJ_JPEG_HUFF_BYTES 896
typedef struct dj_jpeg_segment_info {
  dj_jpeg_decode_info decode;
  int entropy_decodable;
  char reason[100];          /* why not ("" for an eligible file) */
  int restart_interval;      /* MCUs */
  int mcus_x, mcus_y;
  int h_blocks[4], v_blocks[4]; /* blocks per MCU across and down, per component */
  int dc_table[4], ac_table[4]; /* per component: which of `tables` */
  int n_tables;
  int n_segments;
  unsigned char tables[4][DJ_JPEG_HUFF_BYTES];
} dj_jpeg_segment_info;
int dj_jpeg_scan_segments(const unsigned char* data, long size, dj_jpeg_segment_info* info, long* ranges,
                          long range_capacity);

/* ---- The same pre-pass for files without restart intervals as well (data/entropy_decode.py:chunked_decode_host states how
 * they are decoded in parallel, csrc/dj_jpeg_entropy_chunked.hip runs it).  Same arguments, same conditions and the same
 * output for every file dj_jpeg_scan_segments accepts; in addition a file with no DRI segment (or DRI 0) is eligible when
 * its entropy-coded data holds no FF xx but FF 00 before EOI: it reports restart_interval = mcus_x * mcus_y and ONE segment,
 * the scan's entropy-coded bytes.  It never decodes a Huffman code either, never fails for a file's content and refuses
 * every proper prefix of a file. ---- */
int dj_jpeg_scan_segments_unmarked(const unsigned char* data, long size, dj_jpeg_segment_info* info, long* ranges,
                                   long range_capacity);

#ifdef __cplusplus
}
#endif
#endif
