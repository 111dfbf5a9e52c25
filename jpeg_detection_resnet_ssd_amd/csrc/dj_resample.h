// What dj_imgprep.hip, dj_patchresize.hip and dj_ssd_photometric.hip share: Pillow's fixed-point resampling arithmetic on
// the device, and on the host the checks of what a staged blob's descriptors say about the pool, the staged pixels and the
// scratch buffer.  Each output sample of a pass is
//   clip8((2^21 + sum_k pixel[first + k] * tap[k]) >> 22)
// in 32-bit integers over host-made taps of 22 fractional bits (data/device_staging.py computes them).
//
// The host checks take the entry point's name and put it in front of their message, so every text reads as it did when each
// entry point carried its own copy.
#pragma once
#include "../../include/dj_hip.h"
#include "dj_common.h"

#define DJ_RESAMPLE_BITS 22               // Pillow's PRECISION_BITS for 8-bit images
#define DJ_RESAMPLE_MAX_SIDE 65536        // of a source image, a staged rectangle, a window and a tap row
#define DJ_RESAMPLE_SCRATCH_ALIGN 64

// ---- device ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned char dj_clip8(int s) {
  return (unsigned char)min(max(s >> DJ_RESAMPLE_BITS, 0), 255);
}

__device__ __forceinline__ void dj_store_clip8(unsigned char* o, int s0, int s1, int s2) {
  o[0] = dj_clip8(s0);
  o[1] = dj_clip8(s1);
  o[2] = dj_clip8(s2);
}

// `n` taps over the RGB pixels at p, p + stride, ...: stride 3 along a row, the row pitch down a column
template <typename Stride>
__device__ __forceinline__ void dj_accumulate_taps(const unsigned char* p, Stride stride, const int* taps, int n, int& s0,
                                                   int& s1, int& s2) {
  s0 = s1 = s2 = 1 << (DJ_RESAMPLE_BITS - 1);
  for (int t = 0; t < n; ++t) {
    const int c = taps[t];
    s0 += p[t * stride] * c;
    s1 += p[t * stride + 1] * c;
    s2 += p[t * stride + 2] * c;
  }
}

// One sample of a vertical pass: `bounds` / `taps` of its output row, `column` = this sample's column in row `row0` of the
// scratch image (rows `pitch` bytes apart; the bounds count rows from 0, the scratch image starts at row0), stored at `o`.
__device__ __forceinline__ void dj_vertical_sample(const int* bounds, const int* taps, const unsigned char* column, int row0,
                                                   long pitch, unsigned char* o) {
  const int first = bounds[0] - row0, n = bounds[1];
  int s0, s1, s2;
  dj_accumulate_taps(column + (long)first * pitch, pitch, taps, n, s0, s1, s2);
  dj_store_clip8(o, s0, s1, s2);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// bounds + taps of one axis: `count` pairs at `b_off`, `count` rows of `ksize` taps at `k_off`, all inside the pool; with
// `pool_host`, also every sample's taps inside the `size` window samples of that axis
static inline int dj_check_axis(const char* fn, const char* axis, int i, long b_off, long k_off, int ksize, int count,
                                long pool_ints, const int* pool_host = nullptr, int size = 0) {
  DJ_CHECK_ARG(ksize >= 1 && ksize <= DJ_RESAMPLE_MAX_SIDE, "%s: image %d: %s tap row length %d outside 1..%d", fn, i, axis,
               ksize, DJ_RESAMPLE_MAX_SIDE);
  DJ_CHECK_ARG(b_off >= 0 && b_off + 2L * count <= pool_ints, "%s: image %d: %s bounds [%ld, %ld) leave the pool of %ld", fn, i,
               axis, b_off, b_off + 2L * count, pool_ints);
  DJ_CHECK_ARG(k_off >= 0 && k_off + (long)ksize * count <= pool_ints, "%s: image %d: %s taps [%ld, %ld) leave the pool of %ld",
               fn, i, axis, k_off, k_off + (long)ksize * count, pool_ints);
  for (int j = 0; pool_host && j < count; ++j) {
    const int* b = pool_host + b_off + 2L * j;
    DJ_CHECK_ARG(b[0] >= 0 && b[1] >= 0 && b[1] <= ksize && (long)b[0] + b[1] <= size,
                 "%s: image %d: %s sample %d reads window samples [%d, %d + %d) of %d (tap row length %d)", fn, i, axis, j, b[0],
                 b[0], b[1], size, ksize);
  }
  return DJ_OK;
}

// the staged rectangle of a dj_patch_resize_desc: 0 x 0 (nothing staged) or inside the source buffer
static inline int dj_check_staged_rect(const char* fn, int i, const dj_patch_resize_desc* d, long src_bytes) {
  DJ_CHECK_ARG(d->src_h >= 0 && d->src_w >= 0 && d->src_h <= DJ_RESAMPLE_MAX_SIDE && d->src_w <= DJ_RESAMPLE_MAX_SIDE &&
                   (d->src_h == 0) == (d->src_w == 0),
               "%s: image %d: staged size %d x %d outside 1..%d (0 x 0: nothing staged)", fn, i, d->src_h, d->src_w,
               DJ_RESAMPLE_MAX_SIDE);
  if (d->src_h == 0) return DJ_OK;
  DJ_CHECK_ARG(d->src_stride >= 3L * d->src_w, "%s: image %d: src_stride %ld below 3 * width = %ld", fn, i, d->src_stride,
               3L * d->src_w);
  DJ_CHECK_ARG(d->src_offset >= 0 && d->src_stride <= src_bytes && d->src_offset <= src_bytes &&
                   d->src_offset + (d->src_h - 1) * d->src_stride + 3L * d->src_w <= src_bytes,
               "%s: image %d: pixels at offset %ld leave the source buffer of %ld bytes", fn, i, d->src_offset, src_bytes);
  return DJ_OK;
}

// bytes an image's scratch region takes when regions are laid end to end
static inline long dj_scratch_region_bytes(long need) {
  return (need + DJ_RESAMPLE_SCRATCH_ALIGN - 1) / DJ_RESAMPLE_SCRATCH_ALIGN * DJ_RESAMPLE_SCRATCH_ALIGN;
}

// image i's `need` scratch bytes at `offset`: behind the previous image's (`*end`, then moved past this one) and inside the
// buffer
static inline int dj_check_scratch_region(const char* fn, int i, long offset, long need, long* end, long scratch_bytes) {
  DJ_CHECK_ARG(offset >= *end && offset <= scratch_bytes && offset + need <= scratch_bytes,
               "%s: image %d: scratch [%ld, + %ld) overlaps image %d's or leaves the buffer of %ld bytes", fn, i, offset, need,
               i - 1, scratch_bytes);
  *end = offset + need;
  return DJ_OK;
}
