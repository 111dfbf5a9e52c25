// A window of each decoded RGB image on a constant background, optionally mirrored, resized -> one
// [batch][out_h][out_w][3] uint8 tensor: what the expand, crop, flip and resize stages of the SSD augmentation chain
// (data/ssd_augment.py) compose into, bit-exact with the numpy + Pillow statement data/patch_resize.py:patch_resize_host.
// The arithmetic is dj_imgprep.hip's: two passes with a uint8 image in between, each output sample
//   clip8((2^21 + sum_k pixel[first + k] * tap[k]) >> 22)
// in 32-bit integers over host-made taps of 22 fractional bits (NEAREST travels as one tap of 2^22 per sample).
//
// What differs is the fetch of the horizontal pass.  The taps index the WINDOW; window column x reads image column
// win_x0 + (flip ? win_w - 1 - x : x) and window row y reads image row win_y0 + y (the mirror is on the fetch because it
// comes before the resize and Pillow's normalised taps need not be mirror-symmetric), and a fetch outside the image
// yields the background.  Only the rectangle of the image under the window is staged, so "the image" here is that
// rectangle and the window origin is relative to it.  A window row wholly outside the image issues no load at all: an
// expanded canvas is mostly such rows.  The horizontal pass leaves win_h x out_w pixels in the scratch buffer, the
// vertical pass reads those and writes the output.  One launch per pass covers the ragged batch: blockIdx.y is the image,
// blockIdx.x runs over the tallest window's samples and the blocks past a smaller one leave at once.  One thread owns
// one pixel (three accumulators), as in dj_imgprep.hip, whose passes are bound by the number of byte loads, not by bytes.
#include "dj_resample.h"

#define DJ_PATCH_THREADS 256
#define DJ_PATCH_MAX_SIDE DJ_RESAMPLE_MAX_SIDE      // of the staged rectangle and of the window
#define DJ_PATCH_MAX_OUT 8192
#define DJ_PATCH_MAX_ORIGIN (1 << 24)     // |window origin|: keeps every int the kernels form far from overflow

__global__ __launch_bounds__(DJ_PATCH_THREADS) void dj_patch_h_kernel(const unsigned char* __restrict__ src,
                                                                      const dj_patch_resize_desc* __restrict__ desc,
                                                                      const int* __restrict__ pool,
                                                                      unsigned char* __restrict__ scratch, int out_w) {
  const dj_patch_resize_desc d = desc[blockIdx.y];
  const int idx = blockIdx.x * DJ_PATCH_THREADS + threadIdx.x;
  if (idx >= d.win_h * out_w) return;
  const int r = idx / out_w, j = idx - r * out_w;
  const int* bounds = pool + d.h_bounds + 2 * j;
  const int first = bounds[0], n = bounds[1];
  const int* taps = pool + d.h_taps + (long)j * d.h_ksize;
  const int bg0 = d.background & 255, bg1 = (d.background >> 8) & 255, bg2 = (d.background >> 16) & 255;
  const int row = d.win_y0 + r;
  int s0 = 1 << (DJ_RESAMPLE_BITS - 1), s1 = s0, s2 = s0;
  if (row >= 0 && row < d.src_h) {
    const unsigned char* line = src + d.src_offset + (long)row * d.src_stride;
    // image column of window column `first`, and the step from one tap to the next
    const int step = d.flip ? -1 : 1;
    int col = d.win_x0 + (d.flip ? d.win_w - 1 - first : first);
    for (int t = 0; t < n; ++t, col += step) {
      const int c = taps[t];
      int p0 = bg0, p1 = bg1, p2 = bg2;
      if (col >= 0 && col < d.src_w) {
        const unsigned char* p = line + 3L * col;
        p0 = p[0];
        p1 = p[1];
        p2 = p[2];
      }
      s0 += p0 * c;
      s1 += p1 * c;
      s2 += p2 * c;
    }
  } else {
    int sum = 0;
    for (int t = 0; t < n; ++t) sum += taps[t];
    s0 += bg0 * sum;
    s1 += bg1 * sum;
    s2 += bg2 * sum;
  }
  dj_store_clip8(scratch + d.scratch_offset + ((long)r * out_w + j) * 3, s0, s1, s2);
}

__global__ __launch_bounds__(DJ_PATCH_THREADS) void dj_patch_v_kernel(const unsigned char* __restrict__ scratch,
                                                                      const dj_patch_resize_desc* __restrict__ desc,
                                                                      const int* __restrict__ pool,
                                                                      unsigned char* __restrict__ out, long out_stride,
                                                                      int out_h, int out_w) {
  const dj_patch_resize_desc d = desc[blockIdx.y];
  const int idx = blockIdx.x * DJ_PATCH_THREADS + threadIdx.x;
  if (idx >= out_h * out_w) return;
  const int y = idx / out_w, j = idx - y * out_w;
  dj_vertical_sample(pool + d.v_bounds + 2 * y, pool + d.v_taps + (long)y * d.v_ksize, scratch + d.scratch_offset + 3L * j, 0,
                     3L * out_w, out + ((long)blockIdx.y * out_h + y) * out_stride + 3L * j);
}

extern "C" long dj_patch_resize_scratch_bytes(const dj_patch_resize_desc* desc_host, int batch, int out_w) {
  if (!desc_host || batch < 1 || out_w < 1 || out_w > DJ_PATCH_MAX_OUT) {
    dj_set_error("patch_resize_scratch_bytes: null descriptors, batch %d or out_w %d out of range", batch, out_w);
    return DJ_ERR_ARG;
  }
  long total = 0;
  for (int i = 0; i < batch; ++i) {
    if (desc_host[i].win_h < 1 || desc_host[i].win_h > DJ_PATCH_MAX_SIDE) {
      dj_set_error("patch_resize_scratch_bytes: image %d: win_h %d outside 1..%d", i, desc_host[i].win_h, DJ_PATCH_MAX_SIDE);
      return DJ_ERR_ARG;
    }
    total += dj_scratch_region_bytes(3L * out_w * desc_host[i].win_h);
  }
  return total;
}

extern "C" int dj_patch_resize(const unsigned char* src, long src_bytes, const dj_patch_resize_desc* desc_dev,
                               const dj_patch_resize_desc* desc_host, int batch, const int* pool_dev, const int* pool_host,
                               long pool_ints, int out_h, int out_w, unsigned char* out, long out_stride_bytes,
                               unsigned char* scratch, long scratch_bytes, void* stream) {
  DJ_CHECK_ARG(src, "patch_resize: src is null");
  DJ_CHECK_ARG(desc_dev, "patch_resize: desc_dev is null");
  DJ_CHECK_ARG(desc_host, "patch_resize: desc_host is null");
  DJ_CHECK_ARG(pool_dev, "patch_resize: pool_dev is null");
  DJ_CHECK_ARG(pool_host, "patch_resize: pool_host is null");
  DJ_CHECK_ARG(out, "patch_resize: out is null");
  DJ_CHECK_ARG(scratch, "patch_resize: scratch is null");
  DJ_CHECK_ARG(batch >= 1 && batch <= 65535, "patch_resize: batch must be in 1..65535 (got %d)", batch);
  DJ_CHECK_ARG(out_h >= 1 && out_h <= DJ_PATCH_MAX_OUT && out_w >= 1 && out_w <= DJ_PATCH_MAX_OUT,
               "patch_resize: output size %d x %d outside 1..%d", out_h, out_w, DJ_PATCH_MAX_OUT);
  DJ_CHECK_ARG(out_stride_bytes >= 3L * out_w, "patch_resize: out_stride_bytes %ld below 3 * out_w = %ld", out_stride_bytes,
               3L * out_w);
  DJ_CHECK_ARG(src_bytes >= 1 && pool_ints >= 1 && scratch_bytes >= 1,
               "patch_resize: src_bytes / pool_ints / scratch_bytes must be >= 1");
  long scratch_end = 0;
  int max_rows = 0;
  for (int i = 0; i < batch; ++i) {
    const dj_patch_resize_desc* d = desc_host + i;
    if (dj_check_staged_rect("patch_resize", i, d, src_bytes) != DJ_OK) return DJ_ERR_ARG;
    DJ_CHECK_ARG(d->win_h >= 1 && d->win_w >= 1 && d->win_h <= DJ_PATCH_MAX_SIDE && d->win_w <= DJ_PATCH_MAX_SIDE,
                 "patch_resize: image %d: window size %d x %d outside 1..%d", i, d->win_h, d->win_w, DJ_PATCH_MAX_SIDE);
    DJ_CHECK_ARG(d->win_y0 >= -DJ_PATCH_MAX_ORIGIN && d->win_y0 <= DJ_PATCH_MAX_ORIGIN && d->win_x0 >= -DJ_PATCH_MAX_ORIGIN &&
                     d->win_x0 <= DJ_PATCH_MAX_ORIGIN,
                 "patch_resize: image %d: window origin (y %d, x %d) outside +-%d", i, d->win_y0, d->win_x0, DJ_PATCH_MAX_ORIGIN);
    if (dj_check_axis("patch_resize", "horizontal", i, d->h_bounds, d->h_taps, d->h_ksize, out_w, pool_ints, pool_host, d->win_w) != DJ_OK ||
        dj_check_axis("patch_resize", "vertical", i, d->v_bounds, d->v_taps, d->v_ksize, out_h, pool_ints, pool_host, d->win_h) != DJ_OK ||
        dj_check_scratch_region("patch_resize", i, d->scratch_offset, 3L * out_w * d->win_h, &scratch_end, scratch_bytes) != DJ_OK)
      return DJ_ERR_ARG;
    if (d->win_h > max_rows) max_rows = d->win_h;
  }
  const dim3 block(DJ_PATCH_THREADS);
  const dim3 grid_h((unsigned)dj_cdiv((long)max_rows * out_w, DJ_PATCH_THREADS), (unsigned)batch);
  const dim3 grid_v((unsigned)dj_cdiv((long)out_h * out_w, DJ_PATCH_THREADS), (unsigned)batch);
  hipLaunchKernelGGL(dj_patch_h_kernel, grid_h, block, 0, (hipStream_t)stream, src, desc_dev, pool_dev, scratch, out_w);
  DJ_CHECK_LAUNCH("dj_patch_resize (horizontal pass)");
  hipLaunchKernelGGL(dj_patch_v_kernel, grid_v, block, 0, (hipStream_t)stream, scratch, desc_dev, pool_dev, out,
                     out_stride_bytes, out_h, out_w);
  DJ_CHECK_LAUNCH("dj_patch_resize (vertical pass)");
  return DJ_OK;
}
