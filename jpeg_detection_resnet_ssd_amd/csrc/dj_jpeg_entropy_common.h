// What the two entropy-decoding kernels (dj_jpeg_entropy.hip: one lane per restart interval; dj_jpeg_entropy_chunked.hip: one
// lane per chunk of a segment) share: the table format's size, the LDS row type, the zig-zag order, the bit source with
// FF 00 unstuffing, the symbol decoder, and the checks of the host copies of descriptors and records.  The rules are in
// data/entropy_decode.py's docstring.
#ifndef DJ_JPEG_ENTROPY_COMMON_H
#define DJ_JPEG_ENTROPY_COMMON_H
#include "../../include/dj_hip.h"
#include "dj_common.h"

#define DJ_JE_LANES 64
#define DJ_JE_HUFF_BYTES 896

typedef unsigned int dj_je_u32x4 __attribute__((ext_vector_type(4)));
typedef dj_je_u32x4 __attribute__((may_alias)) dj_je_row;      // a 16-byte row of the LDS block, also written as shorts

// zig-zag position -> natural (row-major) index, T.81 figure A.6
__device__ const unsigned char dj_je_natural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                                    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                                    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct DjJeBits {
  const unsigned char* bytes;
  long p, end;
  unsigned acc;      // the next bits, left-justified
  int nbits;         // bits in acc, zeros fed past the end of the data included
  int real;          // bits in acc that came from the data; negative once a bit past the end was consumed
  unsigned stuffed;  // bit i: the (i + 1)-th last data byte taken was followed by a stuffed zero (dj_je_position)
};

// at least 25 bits in acc
__device__ __forceinline__ void dj_je_fill(DjJeBits& b) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (b.nbits <= 24) {
      unsigned v = 0;
      bool got = false;
      if (b.p < b.end) {
        v = b.bytes[b.p];
        if (v != 0xFF) {
          ++b.p;
          got = true;
          b.stuffed <<= 1;
        } else if (b.p + 1 < b.end && b.bytes[b.p + 1] == 0x00) {      // a stuffed zero
          b.p += 2;
          got = true;
          b.stuffed = (b.stuffed << 1) | 1u;
        } else {                                                        // a marker or the range's end: the data ends here
          b.end = b.p;
          v = 0;
        }
      }
      b.acc |= v << (24 - b.nbits);
      b.nbits += 8;
      if (got) b.real += 8;
    }
  }
}

__device__ __forceinline__ void dj_je_skip(DjJeBits& b, int n) {      // 1 <= n <= 16
  b.acc <<= n;
  b.nbits -= n;
  b.real -= n;
}

__device__ __forceinline__ int dj_je_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }      // s >= 1

// -> the length of the code at the head of the bits (0: none of 16 bits or fewer) and its symbol; consumes nothing
__device__ __forceinline__ int dj_je_symbol(DjJeBits& b, const unsigned char* table, int& sym) {
  dj_je_fill(b);
  const int look = (int)(b.acc >> 16);
  const unsigned e = reinterpret_cast<const unsigned short*>(table)[look >> 8];
  int l = min((int)(e >> 8), 16);
  sym = (int)(e & 255);
  if (e == 0) {
    const int* limit = reinterpret_cast<const int*>(table + 512);
#pragma unroll
    for (int i = 16; i >= 9; --i)
      if (look < limit[i - 1]) l = i;      // descending: the shortest length wins
    if (l) {
      const int* offset = reinterpret_cast<const int*>(table + 576);
      sym = table[640 + (((look >> (16 - l)) + offset[l - 1]) & 255)];
    }
  }
  return l;
}

__device__ __forceinline__ int dj_je_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// The position of the next bit to be consumed as 8 * index into `bytes` + bit (it never points into a stuffed zero); past
// the data's end it is the end.
__device__ __forceinline__ long dj_je_position(const DjJeBits& b) {
  const int real = max(b.real, 0);
  const int n = (real + 7) >> 3;      // data bytes in acc, the oldest perhaps partly consumed: at most 4
  return (b.p - n - __popc(b.stuffed & ((1u << n) - 1u))) * 8 + ((8 - (real & 7)) & 7);
}

// The host copies of the file descriptors and segment records against the sizes given -> DJ_OK with the largest n_mcus of
// a record, or the error of the first check that fails.
static inline int dj_je_check_records(const dj_jpeg_entropy_desc* desc_host, int n_files, const dj_jpeg_entropy_seg* seg_host,
                                      int n_segments, int n_tables, long n_bytes, long out_bytes, int* max_mcus_out) {
  int next_segment = 0, max_mcus = 0;
  for (int i = 0; i < n_files; ++i) {
    const dj_jpeg_entropy_desc* d = desc_host + i;
    DJ_CHECK_ARG(d->n_components == 1 || d->n_components == 3, "jpeg_entropy_decode: file %d: %d components, expected 1 or 3", i,
                 d->n_components);
    DJ_CHECK_ARG(d->mcus_x >= 1 && d->mcus_x <= 8192 && d->mcus_y >= 1 && d->mcus_y <= 8192,
                 "jpeg_entropy_decode: file %d: MCU grid %d x %d outside 1..8192", i, d->mcus_y, d->mcus_x);
    DJ_CHECK_ARG(d->table_first >= 0 && d->table_first < n_tables, "jpeg_entropy_decode: file %d: first table %d outside the %d given",
                 i, d->table_first, n_tables);
    for (int c = 0; c < d->n_components; ++c) {
      const int bh = d->blocks_h[c], bw = d->blocks_w[c], h = d->h_blocks[c], v = d->v_blocks[c];
      DJ_CHECK_ARG(bh >= 1 && bh <= 8192 && bw >= 1 && bw <= 8192, "jpeg_entropy_decode: file %d: component %d: block grid %d x %d "
                   "outside 1..8192", i, c, bh, bw);
      DJ_CHECK_ARG(h >= 1 && h <= 4 && v >= 1 && v <= 4, "jpeg_entropy_decode: file %d: component %d: %d x %d blocks per MCU outside "
                   "1..4", i, c, v, h);
      DJ_CHECK_ARG((long)d->mcus_x * h >= bw && (long)d->mcus_y * v >= bh,
                   "jpeg_entropy_decode: file %d: component %d: %d x %d MCUs of %d x %d blocks do not cover the grid of %d x %d", i, c,
                   d->mcus_y, d->mcus_x, v, h, bh, bw);
      DJ_CHECK_ARG(d->dc_table[c] >= 0 && d->dc_table[c] <= 3 && d->ac_table[c] >= 0 && d->ac_table[c] <= 3 &&
                       d->table_first + d->dc_table[c] < n_tables && d->table_first + d->ac_table[c] < n_tables,
                   "jpeg_entropy_decode: file %d: component %d: table index %d / %d outside 0..3 or past the %d tables given", i, c,
                   d->dc_table[c], d->ac_table[c], n_tables);
      const long need = (long)bh * bw * 64;
      DJ_CHECK_ARG(d->plane_capacity[c] >= need, "jpeg_entropy_decode: file %d: component %d: a plane of %ld values exceeds its "
                   "capacity of %ld", i, c, need, d->plane_capacity[c]);
      DJ_CHECK_ARG(d->plane_offset[c] >= 0 && d->plane_offset[c] % 16 == 0 && d->plane_offset[c] <= out_bytes &&
                       2 * need <= out_bytes - d->plane_offset[c],
                   "jpeg_entropy_decode: file %d: component %d: %ld plane bytes at offset %ld leave the buffer of %ld (or the offset "
                   "is no multiple of 16)", i, c, 2 * need, d->plane_offset[c], out_bytes);
    }
    DJ_CHECK_ARG(d->seg_first == next_segment && d->n_segments >= 1 && d->n_segments <= n_segments - next_segment,
                 "jpeg_entropy_decode: file %d: segments [%d, %d + %d) do not follow the previous file's among the %d given", i,
                 d->seg_first, d->seg_first, d->n_segments, n_segments);
    int next_mcu = 0;
    for (int k = d->seg_first; k < d->seg_first + d->n_segments; ++k) {
      const dj_jpeg_entropy_seg* sg = seg_host + k;
      DJ_CHECK_ARG(sg->file == i, "jpeg_entropy_decode: segment %d names file %d, file %d owns it", k, sg->file, i);
      DJ_CHECK_ARG(sg->begin >= 0 && sg->begin <= sg->end && sg->end <= n_bytes,
                   "jpeg_entropy_decode: segment %d: bytes [%ld, %ld) leave the %ld given", k, sg->begin, sg->end, n_bytes);
      DJ_CHECK_ARG(sg->first_mcu == next_mcu && sg->n_mcus >= 1 && sg->n_mcus <= d->mcus_x * d->mcus_y - next_mcu,
                   "jpeg_entropy_decode: segment %d: MCUs [%d, %d + %d) do not tile file %d's %d in order", k, sg->first_mcu,
                   sg->first_mcu, sg->n_mcus, i, d->mcus_x * d->mcus_y);
      next_mcu += sg->n_mcus;
      if (sg->n_mcus > max_mcus) max_mcus = sg->n_mcus;
    }
    DJ_CHECK_ARG(next_mcu == d->mcus_x * d->mcus_y, "jpeg_entropy_decode: file %d: its segments hold %d of its %d MCUs", i, next_mcu,
                 d->mcus_x * d->mcus_y);
    next_segment += d->n_segments;
  }
  DJ_CHECK_ARG(next_segment == n_segments, "jpeg_entropy_decode: the files own %d of the %d segments given", next_segment, n_segments);
  *max_mcus_out = max_mcus;
  return DJ_OK;
}

#endif
