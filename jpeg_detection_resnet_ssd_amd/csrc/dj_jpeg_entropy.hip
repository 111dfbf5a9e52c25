// Huffman entropy decoding of restart-interval JPEG files to their raw int16 coefficient planes -- bit for bit what
// data/entropy_decode.py:entropy_decode_host states, which in turn equals the host reader (csrc/dj_jpeg.cpp) on valid files.
// The rules (bit source, DC / AC decoding, statuses, what an error leaves behind) are in that module's docstring and are
// not repeated here.
//
// Shape: a restart interval ("segment") is byte-aligned and starts with zero predictors, so it is the unit that can be
// decoded on its own: ONE LANE PER SEGMENT, a workgroup of one wave.  Every lane runs the same bounded loops (MCUs of
// the segment, blocks of the MCU, at most 63 AC symbols of a block, at most 16 bits of a symbol); the exec mask handles
// lanes whose segments are shorter.  The block under construction is NOT a register array (its index, the zig-zag
// position's natural index, is only known at run time, and such an array would live in scratch): each lane owns 128 bytes
// of LDS, laid out as 8 rows of 16 bytes with the lanes of a row side by side (row r of lane i at (r * 64 + i) * 16), so
// that a coefficient store is one 2-byte LDS write and the finished block leaves as eight 16-byte LDS reads and eight
// 16-byte global stores (the 128 bytes of a block are one cache line).  The LDS block is cleared as it is read, so the
// next block starts from zeros, and a block that failed is stored as zeros.
//
// Symbol decoding: the next 16 bits index a 256-entry table on their upper 8 bits (codes of 8 bits or fewer, the
// common case, one load); a longer code's length is the first l with look < limit[l - 1] (include/dj_jpeg_segments.h), eight
// compares.  Tables are read from global memory: the lanes of a wave may belong to different files.
//
// Safety: the host checks the host copies of descriptors and records; the kernel clamps what it reads from the device
// copies again -- indexes into [0, n), byte ranges into [0, n_bytes], counts to the maxima the host saw, stores to the
// plane's capacity and to out_bytes -- so corrupt device data costs wrong values, never an access outside the buffers.
// Integer arithmetic throughout, plain C++.
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

struct DjJpegEntropyParams {
  const unsigned char* bytes;
  long n_bytes;
  const dj_jpeg_entropy_desc* desc;
  int n_files;
  const dj_jpeg_entropy_seg* seg;
  int n_segments;
  const unsigned char* tables;
  int n_tables;
  unsigned char* out;
  long out_bytes;
  int* status;
  int max_mcus;      // the largest n_mcus of the host's records
};

struct DjJeBits {
  const unsigned char* bytes;
  long p, end;
  unsigned acc;      // the next bits, left-justified
  int nbits;         // bits in acc, zeros fed past the end of the data included
  int real;          // bits in acc that came from the data; negative once a bit past the end was consumed
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
        } else if (b.p + 1 < b.end && b.bytes[b.p + 1] == 0x00) {      // a stuffed zero
          b.p += 2;
          got = true;
        } else {                                                        // a marker or the range's end: the data ends
          b.p = b.end;
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

// One block into the lane's LDS rows (blk = the lane's first short; row r starts 512 r shorts further) -> status
__device__ __forceinline__ int dj_je_block(DjJeBits& b, const unsigned char* dc, const unsigned char* ac, int& pred,
                                           unsigned short* blk, const unsigned char* natural) {
  int sym;
  int l = dj_je_symbol(b, dc, sym);
  if (l == 0) return 1;
  dj_je_skip(b, l);
  if (b.real < 0) return 4;
  if (sym > 11) return 1;
  if (sym) {
    dj_je_fill(b);
    const int v = (int)(b.acc >> (32 - sym));
    dj_je_skip(b, sym);
    if (b.real < 0) return 4;
    pred = (int)((unsigned)pred + (unsigned)dj_je_extend(v, sym));
  }
  blk[0] = (unsigned short)pred;
  int k = 1;
  for (int it = 0; it < 63 && k < 64; ++it) {      // every symbol adds at least 1 to k
    l = dj_je_symbol(b, ac, sym);
    if (l == 0) return 2;
    dj_je_skip(b, l);
    if (b.real < 0) return 4;
    const int r = sym >> 4, s = sym & 15;
    if (s == 0) {
      if (r != 15) break;      // end of block
      k += 16;
      continue;
    }
    k += r;
    if (k > 63) return 3;
    dj_je_fill(b);
    const int v = (int)(b.acc >> (32 - s));
    dj_je_skip(b, s);
    if (b.real < 0) return 4;
    const int n = natural[k];
    blk[(n >> 3) * (DJ_JE_LANES * 8) + (n & 7)] = (unsigned short)dj_je_extend(v, s);
    ++k;
  }
  return 0;
}

__device__ __forceinline__ int dj_je_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(DJ_JE_LANES) void dj_jpeg_entropy_kernel(DjJpegEntropyParams p) {
  __shared__ dj_je_row rows[8 * DJ_JE_LANES];
  __shared__ unsigned char natural[64];
  const int lane = threadIdx.x;
  const dj_je_row zero = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int r = 0; r < 8; ++r) rows[r * DJ_JE_LANES + lane] = zero;
  natural[lane] = dj_je_natural[lane];
  __syncthreads();
  const int s = blockIdx.x * DJ_JE_LANES + lane;
  if (s >= p.n_segments) return;
  const dj_jpeg_entropy_seg* sg = p.seg + s;
  const dj_jpeg_entropy_desc* d = p.desc + dj_je_clamp(sg->file, 0, p.n_files - 1);
  DjJeBits b;
  b.bytes = p.bytes;
  b.end = min(max(sg->end, 0L), p.n_bytes);
  b.p = min(max(sg->begin, 0L), b.end);
  b.acc = 0;
  b.nbits = 0;
  b.real = 0;
  const int n_mcus = dj_je_clamp(sg->n_mcus, 0, p.max_mcus);
  const int first = dj_je_clamp(sg->first_mcu, 0, 1 << 26);
  const int mcus_x = max(d->mcus_x, 1);
  const int ncomp = d->n_components == 1 ? 1 : 3;
  const int table_first = dj_je_clamp(d->table_first, 0, p.n_tables - 1);
  // the file's geometry, read once (every loop over c is unrolled, so these are registers, not indexed arrays)
  int hs[3], vs[3], bhs[3], bws[3];
  const unsigned char *dcs[3], *acs[3];
  long planes[3], capacities[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    hs[c] = dj_je_clamp(d->h_blocks[c], 1, 4);
    vs[c] = dj_je_clamp(d->v_blocks[c], 1, 4);
    bhs[c] = dj_je_clamp(d->blocks_h[c], 0, 8192);
    bws[c] = dj_je_clamp(d->blocks_w[c], 0, 8192);
    dcs[c] = p.tables + (long)dj_je_clamp(table_first + dj_je_clamp(d->dc_table[c], 0, 3), 0, p.n_tables - 1) * DJ_JE_HUFF_BYTES;
    acs[c] = p.tables + (long)dj_je_clamp(table_first + dj_je_clamp(d->ac_table[c], 0, 3), 0, p.n_tables - 1) * DJ_JE_HUFF_BYTES;
    planes[c] = d->plane_offset[c];
    capacities[c] = d->plane_capacity[c];
  }
  unsigned short* blk = reinterpret_cast<unsigned short*>(rows) + lane * 8;
  int pred[3] = {0, 0, 0};
  int status = 0;
  for (int m = 0; m < n_mcus; ++m) {
    const int mcu = first + m;
    const int my = mcu / mcus_x, mx = mcu - my * mcus_x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {      // unrolled: pred[c] stays in a register
      if (c < ncomp) {
        const int h = hs[c], v = vs[c], bh = bhs[c], bw = bws[c];
        const unsigned char *dc = dcs[c], *ac = acs[c];
        const long plane = planes[c], capacity = capacities[c];
        for (int by = 0; by < v; ++by)
          for (int bx = 0; bx < h; ++bx) {
            if (status == 0) status = dj_je_block(b, dc, ac, pred[c], blk, natural);
            const long row = (long)my * v + by, col = (long)mx * h + bx;
            const long index = row * bw + col, at = plane + index * 128;
            // MCU padding is decoded and dropped; the store is clipped to the plane and to the buffer
            const bool store = row < bh && col < bw && plane >= 0 && (at & 15) == 0 && (index + 1) * 64 <= capacity &&
                               at + 128 <= p.out_bytes;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
              const dj_je_row value = rows[r * DJ_JE_LANES + lane];
              rows[r * DJ_JE_LANES + lane] = zero;
              if (store) *reinterpret_cast<dj_je_row*>(p.out + at + 16 * r) = status == 0 ? value : zero;
            }
          }
      }
    }
  }
  p.status[s] = status;
}

extern "C" int dj_jpeg_entropy_decode(const unsigned char* bytes, long n_bytes, const dj_jpeg_entropy_desc* desc_dev,
                                      const dj_jpeg_entropy_desc* desc_host, int n_files, const dj_jpeg_entropy_seg* seg_dev,
                                      const dj_jpeg_entropy_seg* seg_host, int n_segments, const unsigned char* tables,
                                      int n_tables, unsigned char* out, long out_bytes, int* status, void* stream) {
  DJ_CHECK_ARG(bytes, "jpeg_entropy_decode: bytes is null");
  DJ_CHECK_ARG(desc_dev, "jpeg_entropy_decode: desc_dev is null");
  DJ_CHECK_ARG(desc_host, "jpeg_entropy_decode: desc_host is null");
  DJ_CHECK_ARG(seg_dev, "jpeg_entropy_decode: seg_dev is null");
  DJ_CHECK_ARG(seg_host, "jpeg_entropy_decode: seg_host is null");
  DJ_CHECK_ARG(tables, "jpeg_entropy_decode: tables is null");
  DJ_CHECK_ARG(out, "jpeg_entropy_decode: out is null");
  DJ_CHECK_ARG(status, "jpeg_entropy_decode: status is null");
  DJ_CHECK_ARG(n_files >= 1 && n_files <= 65535, "jpeg_entropy_decode: the number of files must be in 1..65535 (got %d)", n_files);
  DJ_CHECK_ARG(n_segments >= 1 && n_segments <= (1 << 24), "jpeg_entropy_decode: the number of segments must be in 1..2^24 (got %d)",
               n_segments);
  DJ_CHECK_ARG(n_tables >= 1 && n_tables <= 4 * 65535, "jpeg_entropy_decode: the number of tables must be in 1..262140 (got %d)",
               n_tables);
  DJ_CHECK_ARG(n_bytes >= 1 && out_bytes >= 1, "jpeg_entropy_decode: n_bytes / out_bytes must be >= 1");
  DJ_CHECK_ARG(((uintptr_t)out & 15) == 0 && ((uintptr_t)tables & 15) == 0 && ((uintptr_t)desc_dev & 7) == 0 &&
                   ((uintptr_t)seg_dev & 7) == 0 && ((uintptr_t)status & 3) == 0,
               "jpeg_entropy_decode: out and tables must be 16-byte, desc_dev and seg_dev 8-byte and status 4-byte aligned");
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
  DjJpegEntropyParams p;
  p.bytes = bytes;
  p.n_bytes = n_bytes;
  p.desc = desc_dev;
  p.n_files = n_files;
  p.seg = seg_dev;
  p.n_segments = n_segments;
  p.tables = tables;
  p.n_tables = n_tables;
  p.out = out;
  p.out_bytes = out_bytes;
  p.status = status;
  p.max_mcus = max_mcus;
  hipLaunchKernelGGL(dj_jpeg_entropy_kernel, dim3((unsigned)dj_cdiv(n_segments, DJ_JE_LANES)), dim3(DJ_JE_LANES), 0,
                     (hipStream_t)stream, p);
  DJ_CHECK_LAUNCH("dj_jpeg_entropy_decode");
  return DJ_OK;
}
