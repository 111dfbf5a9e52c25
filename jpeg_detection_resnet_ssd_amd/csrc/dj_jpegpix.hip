// RGB pixels of baseline / extended-sequential JPEG files from their entropy-decoded RAW coefficients, written into the
// staged pixel region of a ragged batch exactly where the host would have copied decoded pixels: byte for byte what
// data/jpeg_pixels.py:jpeg_pixels_host states in numpy, which is libjpeg's default decompression (what Pillow's
// Image.open(f).convert("RGB") returns).  It is csrc/dj_rgb2dct.hip run backwards: the same 13-bit constants, the same LDS
// rows padded to 9 dwords.  What decides bits:
//   * coefficient * table entry in int32, then jidctint.c's inverse DCT: column pass descaled by 11 bits, row pass by 18,
//     + 128, clamp (libjpeg's range table wraps for samples no forward DCT of 8-bit pixels produces; this clamps, as the
//     statement does);
//   * the triangle upsampling filters of jdsample.c for a chroma component wider than 2 samples -- with the neighbour past
//     the component's REAL down-sampled extent (not the block grid's) replaced by the edge sample, which gives libjpeg's
//     first / last-column cases and its replicated context rows -- and plain replication for a narrower one;
//   * jdcolor.c's 16-bit fixed-point YCbCr -> RGB with one rounding constant for the whole green term.
//
// Two passes, both plain C++ and small next to the upload of their input.  (a) The inverse DCT of the blocks the
// rectangle needs (the descriptor's block ranges: the covering range, widened by one chroma sample for the filter): eight
// lanes own one block, eight blocks a wave; each lane runs one column, the block turns in LDS, each lane runs one row and
// stores its eight samples as one 8-byte word into the component's uint8 sample plane in the scratch buffer.  (b) One
// thread per pixel of the rectangle: luma, the two upsampled chroma samples, the colour conversion, three byte stores
// (as dj_ssd_photometric, which rewrites the same bytes next).  blockIdx.y is the image, blockIdx.x runs over the largest
// image's work and the blocks past a smaller one leave at once.
#include "dj_resample.h"

#define DJ_JPX_THREADS 256
#define DJ_JPX_BLOCKS (DJ_JPX_THREADS / 8)      // 8x8 blocks per workgroup
#define DJ_JPX_LDW 9                            // dwords per staged block row: row-per-lane and column-per-lane accesses
                                                // both spread over the banks (dj_rgb2dct.hip)
#define DJ_JPX_MAX_SIDE 65535                   // a JPEG frame header's limit

// real extent of component c: rows (axis 0) or columns (axis 1)
__host__ __device__ __forceinline__ int jpx_extent(const dj_jpeg_pixels_desc* d, int c, int axis) {
  const int size = axis ? d->width : d->height, f = c == 0 ? 1 : (axis ? d->h_samp : d->v_samp);
  return (size + f - 1) / f;
}

// jidctint.c's 1-D pass, in place, descaled by `shift` bits
__device__ __forceinline__ void jpx_idct8(int* d, int shift) {
  int z1 = (d[2] + d[6]) * 4433;
  const int tmp2 = z1 - d[6] * 15137, tmp3 = z1 + d[2] * 6270;
  const int tmp0 = (d[0] + d[4]) * 8192, tmp1 = (d[0] - d[4]) * 8192;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  int t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
  z1 = t0 + t3;
  int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int z5 = (z3 + z4) * 9633;
  t0 *= 2446;
  t1 *= 16819;
  t2 *= 25172;
  t3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  t0 += z1 + z3;
  t1 += z2 + z4;
  t2 += z2 + z3;
  t3 += z1 + z4;
  const int r = 1 << (shift - 1);
  d[0] = (tmp10 + t3 + r) >> shift;
  d[7] = (tmp10 - t3 + r) >> shift;
  d[1] = (tmp11 + t2 + r) >> shift;
  d[6] = (tmp11 - t2 + r) >> shift;
  d[2] = (tmp12 + t1 + r) >> shift;
  d[5] = (tmp12 - t1 + r) >> shift;
  d[3] = (tmp13 + t0 + r) >> shift;
  d[4] = (tmp13 - t0 + r) >> shift;
}

__global__ __launch_bounds__(DJ_JPX_THREADS) void dj_jpegpix_idct_kernel(const unsigned char* __restrict__ coef,
                                                                         const dj_jpeg_pixels_desc* __restrict__ desc,
                                                                         const int* __restrict__ tables,
                                                                         unsigned char* __restrict__ scratch) {
  __shared__ int ws[DJ_JPX_BLOCKS][8][DJ_JPX_LDW];
  const dj_jpeg_pixels_desc* d = desc + blockIdx.y;
  int total = 0;
  for (int c = 0; c < d->n_components; ++c) total += (d->by1[c] - d->by0[c]) * (d->bx1[c] - d->bx0[c]);
  if ((int)(blockIdx.x * DJ_JPX_BLOCKS) >= total) return;      // uniform over the workgroup
  const int lane = threadIdx.x & 7, blk = threadIdx.x >> 3;
  // which block of which component: a thread past the last block loads and stores nothing but keeps the barrier
  int b = blockIdx.x * DJ_JPX_BLOCKS + blk, c = 0;
  bool live = false;
  for (; c < d->n_components; ++c) {
    const int count = (d->by1[c] - d->by0[c]) * (d->bx1[c] - d->bx0[c]);
    if (b < count) {
      live = true;
      break;
    }
    b -= count;
  }
  int v[8], ry = 0, rx = 0, nbx = 1;
  if (live) {
    nbx = d->bx1[c] - d->bx0[c];
    ry = b / nbx;                                              // block row / column within the range
    rx = b - ry * nbx;
    const short* p = reinterpret_cast<const short*>(coef + d->coef_offset[c]) +
                     ((long)(d->by0[c] + ry) * d->blocks_w[c] + (d->bx0[c] + rx)) * 64;
    const int* q = tables + d->table_offset + c * 64;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (int)p[k * 8 + lane] * q[k * 8 + lane];      // column `lane`
    jpx_idct8(v, 11);
#pragma unroll
    for (int k = 0; k < 8; ++k) ws[blk][k][lane] = v[k];
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = ws[blk][lane][k];                            // row `lane`
    jpx_idct8(v, 18);
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lo |= (unsigned)min(max(v[k] + 128, 0), 255) << (8 * k);
      hi |= (unsigned)min(max(v[k + 4] + 128, 0), 255) << (8 * k);
    }
    // sample_offset is a multiple of 8 and a plane row is 8 * nbx bytes: the word is aligned
    unsigned char* o = scratch + d->sample_offset[c] + ((long)(ry * 8 + lane) * nbx + rx) * 8;
    *reinterpret_cast<uint2*>(o) = make_uint2(lo, hi);
  }
}

// sample (r, k) of component c's plane, r and k in component coordinates
__device__ __forceinline__ int jpx_sample(const unsigned char* scratch, const dj_jpeg_pixels_desc* d, int c, int r, int k) {
  const long pitch = 8L * (d->bx1[c] - d->bx0[c]);
  return scratch[d->sample_offset[c] + (long)(r - 8 * d->by0[c]) * pitch + (k - 8 * d->bx0[c])];
}

// chroma component c at pixel (y, x), upsampled as jdsample.c does by default
__device__ __forceinline__ int jpx_chroma(const unsigned char* scratch, const dj_jpeg_pixels_desc* d, int c, int y, int x) {
  const int h = d->h_samp, v = d->v_samp;
  if (h == 1) return jpx_sample(scratch, d, c, y, x);
  const int ch = jpx_extent(d, c, 0), cw = jpx_extent(d, c, 1);
  if (cw <= 2) return jpx_sample(scratch, d, c, v == 2 ? y >> 1 : y, x >> 1);      // too narrow for the triangle filter
  const int k = x >> 1, kn = (x & 1) ? min(k + 1, cw - 1) : max(k - 1, 0);
  if (v == 1) return (3 * jpx_sample(scratch, d, c, y, k) + jpx_sample(scratch, d, c, y, kn) + ((x & 1) ? 2 : 1)) >> 2;
  const int r = y >> 1, rn = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
  const int s = 3 * jpx_sample(scratch, d, c, r, k) + jpx_sample(scratch, d, c, rn, k);
  const int sn = 3 * jpx_sample(scratch, d, c, r, kn) + jpx_sample(scratch, d, c, rn, kn);
  return (3 * s + sn + ((x & 1) ? 7 : 8)) >> 4;
}

__device__ __forceinline__ unsigned char jpx_clamp8(int s) { return (unsigned char)min(max(s, 0), 255); }

__global__ __launch_bounds__(DJ_JPX_THREADS) void dj_jpegpix_colour_kernel(const unsigned char* __restrict__ scratch,
                                                                           const dj_jpeg_pixels_desc* __restrict__ desc,
                                                                           unsigned char* __restrict__ dst) {
  const dj_jpeg_pixels_desc* d = desc + blockIdx.y;
  const int rw = d->xb - d->xa, n = rw * (d->yb - d->ya);      // the host copy was checked: below 2^31
  const int idx = blockIdx.x * DJ_JPX_THREADS + threadIdx.x;
  if (idx >= n) return;
  const int ry = idx / rw, rx = idx - ry * rw;
  const int y = d->ya + ry, x = d->xa + rx;
  const int luma = jpx_sample(scratch, d, 0, y, x);
  int r = luma, g = luma, b = luma;
  if (d->n_components == 3) {
    const int cb = jpx_chroma(scratch, d, 1, y, x) - 128, cr = jpx_chroma(scratch, d, 2, y, x) - 128;
    r = luma + ((91881 * cr + 32768) >> 16);
    g = luma + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    b = luma + ((116130 * cb + 32768) >> 16);
  }
  unsigned char* o = dst + d->dst_offset + (long)ry * d->dst_stride + 3L * rx;
  o[0] = jpx_clamp8(r);
  o[1] = jpx_clamp8(g);
  o[2] = jpx_clamp8(b);
}

// [lo, hi] of the samples of component c that rows / columns a..b-1 of the image read, the filter's neighbour included
static inline void jpx_needed(const dj_jpeg_pixels_desc* d, int c, int axis, int a, int b, int* lo, int* hi) {
  const int s = c == 0 ? 0 : (axis ? d->h_samp : d->v_samp) - 1, extent = jpx_extent(d, c, axis);
  *lo = (a >> s) - s;
  if (*lo < 0) *lo = 0;
  *hi = ((b - 1) >> s) + s;
  if (*hi > extent - 1) *hi = extent - 1;
}

extern "C" int dj_jpeg_pixels(const unsigned char* coef, long coef_bytes, const dj_jpeg_pixels_desc* desc_dev,
                              const dj_jpeg_pixels_desc* desc_host, int n, const int* tables, long table_ints,
                              unsigned char* dst, long dst_bytes, unsigned char* scratch, long scratch_bytes, void* stream) {
  DJ_CHECK_ARG(coef, "jpeg_pixels: coef is null");
  DJ_CHECK_ARG(desc_dev, "jpeg_pixels: desc_dev is null");
  DJ_CHECK_ARG(desc_host, "jpeg_pixels: desc_host is null");
  DJ_CHECK_ARG(tables, "jpeg_pixels: tables is null");
  DJ_CHECK_ARG(dst, "jpeg_pixels: dst is null");
  DJ_CHECK_ARG(scratch, "jpeg_pixels: scratch is null");
  DJ_CHECK_ARG(n >= 1 && n <= 65535, "jpeg_pixels: the number of images must be in 1..65535 (got %d)", n);
  DJ_CHECK_ARG(coef_bytes >= 1 && table_ints >= 1 && dst_bytes >= 1 && scratch_bytes >= 1,
               "jpeg_pixels: coef_bytes / table_ints / dst_bytes / scratch_bytes must be >= 1");
  DJ_CHECK_ARG(((uintptr_t)coef & 1) == 0 && ((uintptr_t)scratch & 7) == 0 && ((uintptr_t)tables & 3) == 0,
               "jpeg_pixels: coef must be 2-byte, tables 4-byte and scratch 8-byte aligned");
  long scratch_end = 0, max_blocks = 0, max_pixels = 0;
  for (int i = 0; i < n; ++i) {
    const dj_jpeg_pixels_desc* d = desc_host + i;
    DJ_CHECK_ARG(d->n_components == 1 || d->n_components == 3, "jpeg_pixels: image %d: %d components, expected 1 or 3", i,
                 d->n_components);
    const bool sampling_ok = d->n_components == 1 ? (d->h_samp == 1 && d->v_samp == 1)
                                                  : ((d->h_samp == 1 || d->h_samp == 2) && (d->v_samp == 1 || d->v_samp == 2) &&
                                                     !(d->h_samp == 1 && d->v_samp == 2));
    DJ_CHECK_ARG(sampling_ok, "jpeg_pixels: image %d: luma sampling %d x %d of %d components is not 1x1, 2x1 or 2x2", i,
                 d->h_samp, d->v_samp, d->n_components);
    DJ_CHECK_ARG(d->height >= 1 && d->height <= DJ_JPX_MAX_SIDE && d->width >= 1 && d->width <= DJ_JPX_MAX_SIDE,
                 "jpeg_pixels: image %d: size %d x %d outside 1..%d", i, d->height, d->width, DJ_JPX_MAX_SIDE);
    DJ_CHECK_ARG(d->ya >= 0 && d->ya < d->yb && d->yb <= d->height && d->xa >= 0 && d->xa < d->xb && d->xb <= d->width,
                 "jpeg_pixels: image %d: rectangle rows [%d, %d) columns [%d, %d) is empty or leaves the image of %d x %d", i,
                 d->ya, d->yb, d->xa, d->xb, d->height, d->width);
    DJ_CHECK_ARG(d->table_offset >= 0 && d->table_offset + 64L * d->n_components <= table_ints,
                 "jpeg_pixels: image %d: tables at %d leave the %ld ints given", i, d->table_offset, table_ints);
    const long rh = d->yb - d->ya, rw = d->xb - d->xa;
    DJ_CHECK_ARG(rh * rw <= 0x7fffffffL, "jpeg_pixels: image %d: a rectangle of %ld x %ld pixels, at most 2^31 - 1 are supported",
                 i, rh, rw);
    DJ_CHECK_ARG(d->dst_stride >= 3 * rw, "jpeg_pixels: image %d: dst_stride %ld below 3 * width = %ld", i, d->dst_stride, 3 * rw);
    DJ_CHECK_ARG(d->dst_offset >= 0 && d->dst_stride <= dst_bytes && d->dst_offset <= dst_bytes &&
                     d->dst_offset + (rh - 1) * d->dst_stride + 3 * rw <= dst_bytes,
                 "jpeg_pixels: image %d: pixels at offset %ld leave the destination of %ld bytes", i, d->dst_offset, dst_bytes);
    long blocks = 0;
    for (int c = 0; c < d->n_components; ++c) {
      const int bh = (jpx_extent(d, c, 0) + 7) / 8, bw = (jpx_extent(d, c, 1) + 7) / 8;
      DJ_CHECK_ARG(d->blocks_h[c] == bh && d->blocks_w[c] == bw,
                   "jpeg_pixels: image %d: component %d: block grid %d x %d, the frame has %d x %d", i, c, d->blocks_h[c],
                   d->blocks_w[c], bh, bw);
      const long plane = (long)bh * bw * 128;
      DJ_CHECK_ARG(d->coef_offset[c] >= 0 && d->coef_offset[c] % 2 == 0 && d->coef_offset[c] <= coef_bytes &&
                       plane <= coef_bytes - d->coef_offset[c],
                   "jpeg_pixels: image %d: component %d: %ld coefficient bytes at offset %ld leave the buffer of %ld (or the "
                   "offset is odd)", i, c, plane, d->coef_offset[c], coef_bytes);
      int r0, r1, k0, k1;
      jpx_needed(d, c, 0, d->ya, d->yb, &r0, &r1);
      jpx_needed(d, c, 1, d->xa, d->xb, &k0, &k1);
      DJ_CHECK_ARG(d->by0[c] >= 0 && d->by0[c] <= r0 / 8 && d->by1[c] > r1 / 8 && d->by1[c] <= bh && d->bx0[c] >= 0 &&
                       d->bx0[c] <= k0 / 8 && d->bx1[c] > k1 / 8 && d->bx1[c] <= bw,
                   "jpeg_pixels: image %d: component %d: block rows [%d, %d) columns [%d, %d) do not cover samples [%d, %d] x "
                   "[%d, %d] or leave the grid of %d x %d", i, c, d->by0[c], d->by1[c], d->bx0[c], d->bx1[c], r0, r1, k0, k1, bh, bw);
      const long count = (long)(d->by1[c] - d->by0[c]) * (d->bx1[c] - d->bx0[c]);
      DJ_CHECK_ARG(d->sample_offset[c] % 8 == 0, "jpeg_pixels: image %d: component %d: sample_offset %ld is no multiple of 8", i,
                   c, d->sample_offset[c]);
      if (dj_check_scratch_region("jpeg_pixels", i, d->sample_offset[c], count * 64, &scratch_end, scratch_bytes) != DJ_OK)
        return DJ_ERR_ARG;
      blocks += count;
    }
    if (blocks > max_blocks) max_blocks = blocks;
    if (rh * rw > max_pixels) max_pixels = rh * rw;
  }
  const dim3 block(DJ_JPX_THREADS);
  const dim3 grid_a((unsigned)dj_cdiv(max_blocks, DJ_JPX_BLOCKS), (unsigned)n);
  const dim3 grid_b((unsigned)dj_cdiv(max_pixels, DJ_JPX_THREADS), (unsigned)n);
  hipLaunchKernelGGL(dj_jpegpix_idct_kernel, grid_a, block, 0, (hipStream_t)stream, coef, desc_dev, tables, scratch);
  DJ_CHECK_LAUNCH("dj_jpeg_pixels (inverse DCT)");
  hipLaunchKernelGGL(dj_jpegpix_colour_kernel, grid_b, block, 0, (hipStream_t)stream, scratch, desc_dev, dst);
  DJ_CHECK_LAUNCH("dj_jpeg_pixels (upsample and colour)");
  return DJ_OK;
}
