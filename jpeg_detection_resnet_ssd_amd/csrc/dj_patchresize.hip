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
#include "../../include/dj_hip.h"
#include "dj_common.h"

#define DJ_PATCH_THREADS 256
#define DJ_PATCH_BITS 22                  // Pillow's PRECISION_BITS for 8-bit images
#define DJ_PATCH_MAX_SIDE 65536           // of the staged rectangle and of the window
#define DJ_PATCH_MAX_OUT 8192
#define DJ_PATCH_MAX_ORIGIN (1 << 24)     // |window origin|: keeps every int the kernels form far from overflow

__device__ __forceinline__ unsigned char patch_clip8(int s) {
  return (unsigned char)min(max(s >> DJ_PATCH_BITS, 0), 255);
}

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
  int s0 = 1 << (DJ_PATCH_BITS - 1), s1 = s0, s2 = s0;
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
  unsigned char* o = scratch + d.scratch_offset + ((long)r * out_w + j) * 3;
  o[0] = patch_clip8(s0);
  o[1] = patch_clip8(s1);
  o[2] = patch_clip8(s2);
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
  const int* bounds = pool + d.v_bounds + 2 * y;
  const int first = bounds[0], n = bounds[1];
  const int* taps = pool + d.v_taps + (long)y * d.v_ksize;
  const long pitch = 3L * out_w;
  const unsigned char* p = scratch + d.scratch_offset + (long)first * pitch + 3L * j;
  int s0 = 1 << (DJ_PATCH_BITS - 1), s1 = s0, s2 = s0;
  for (int t = 0; t < n; ++t) {
    const int c = taps[t];
    s0 += p[t * pitch] * c;
    s1 += p[t * pitch + 1] * c;
    s2 += p[t * pitch + 2] * c;
  }
  unsigned char* o = out + ((long)blockIdx.y * out_h + y) * out_stride + 3L * j;
  o[0] = patch_clip8(s0);
  o[1] = patch_clip8(s1);
  o[2] = patch_clip8(s2);
}

// bounds + taps of one axis: `count` pairs at `b_off`, `count` rows of `ksize` taps at `k_off`, all inside the pool, and
// every sample's taps inside the `size` window samples of that axis
static int patch_check_axis(const char* axis, int i, long b_off, long k_off, int ksize, int count, int size,
                            const int* pool_host, long pool_ints) {
  DJ_CHECK_ARG(ksize >= 1 && ksize <= DJ_PATCH_MAX_SIDE, "patch_resize: image %d: %s tap row length %d outside 1..%d", i, axis,
               ksize, DJ_PATCH_MAX_SIDE);
  DJ_CHECK_ARG(b_off >= 0 && b_off + 2L * count <= pool_ints, "patch_resize: image %d: %s bounds [%ld, %ld) leave the pool of %ld",
               i, axis, b_off, b_off + 2L * count, pool_ints);
  DJ_CHECK_ARG(k_off >= 0 && k_off + (long)ksize * count <= pool_ints,
               "patch_resize: image %d: %s taps [%ld, %ld) leave the pool of %ld", i, axis, k_off, k_off + (long)ksize * count,
               pool_ints);
  for (int j = 0; j < count; ++j) {
    const int* b = pool_host + b_off + 2L * j;
    DJ_CHECK_ARG(b[0] >= 0 && b[1] >= 0 && b[1] <= ksize && (long)b[0] + b[1] <= size,
                 "patch_resize: image %d: %s sample %d reads window samples [%d, %d + %d) of %d (tap row length %d)", i, axis, j,
                 b[0], b[0], b[1], size, ksize);
  }
  return DJ_OK;
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
    total += (3L * out_w * desc_host[i].win_h + 63) / 64 * 64;
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
    DJ_CHECK_ARG(d->src_h >= 0 && d->src_w >= 0 && d->src_h <= DJ_PATCH_MAX_SIDE && d->src_w <= DJ_PATCH_MAX_SIDE &&
                     (d->src_h == 0) == (d->src_w == 0),
                 "patch_resize: image %d: staged size %d x %d outside 1..%d (0 x 0: nothing staged)", i, d->src_h, d->src_w,
                 DJ_PATCH_MAX_SIDE);
    if (d->src_h > 0) {
      DJ_CHECK_ARG(d->src_stride >= 3L * d->src_w, "patch_resize: image %d: src_stride %ld below 3 * width = %ld", i,
                   d->src_stride, 3L * d->src_w);
      DJ_CHECK_ARG(d->src_offset >= 0 && d->src_stride <= src_bytes && d->src_offset <= src_bytes &&
                       d->src_offset + (d->src_h - 1) * d->src_stride + 3L * d->src_w <= src_bytes,
                   "patch_resize: image %d: pixels at offset %ld leave the source buffer of %ld bytes", i, d->src_offset,
                   src_bytes);
    }
    DJ_CHECK_ARG(d->win_h >= 1 && d->win_w >= 1 && d->win_h <= DJ_PATCH_MAX_SIDE && d->win_w <= DJ_PATCH_MAX_SIDE,
                 "patch_resize: image %d: window size %d x %d outside 1..%d", i, d->win_h, d->win_w, DJ_PATCH_MAX_SIDE);
    DJ_CHECK_ARG(d->win_y0 >= -DJ_PATCH_MAX_ORIGIN && d->win_y0 <= DJ_PATCH_MAX_ORIGIN && d->win_x0 >= -DJ_PATCH_MAX_ORIGIN &&
                     d->win_x0 <= DJ_PATCH_MAX_ORIGIN,
                 "patch_resize: image %d: window origin (y %d, x %d) outside +-%d", i, d->win_y0, d->win_x0, DJ_PATCH_MAX_ORIGIN);
    if (patch_check_axis("horizontal", i, d->h_bounds, d->h_taps, d->h_ksize, out_w, d->win_w, pool_host, pool_ints) != DJ_OK ||
        patch_check_axis("vertical", i, d->v_bounds, d->v_taps, d->v_ksize, out_h, d->win_h, pool_host, pool_ints) != DJ_OK)
      return DJ_ERR_ARG;
    const long need = 3L * out_w * d->win_h;
    DJ_CHECK_ARG(d->scratch_offset >= scratch_end && d->scratch_offset <= scratch_bytes && d->scratch_offset + need <= scratch_bytes,
                 "patch_resize: image %d: scratch [%ld, + %ld) overlaps image %d's or leaves the buffer of %ld bytes", i,
                 d->scratch_offset, need, i - 1, scratch_bytes);
    scratch_end = d->scratch_offset + need;
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
