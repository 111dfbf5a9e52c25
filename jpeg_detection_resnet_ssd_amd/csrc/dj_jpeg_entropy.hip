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
#include "dj_jpeg_entropy_common.h"

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
  b.stuffed = 0;
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
  int max_mcus = 0;
  const int rc = dj_je_check_records(desc_host, n_files, seg_host, n_segments, n_tables, n_bytes, out_bytes, &max_mcus);
  if (rc != DJ_OK) return rc;
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
