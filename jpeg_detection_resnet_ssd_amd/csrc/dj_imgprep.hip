// Decoded RGB images of different sizes -> one [batch][T][T][3] uint8 tensor: the resize, crop and horizontal flip that the
// reference's classifier generators run in PIL before the JPEG emission step
// (classification_part/vgg_jpeg_keras/generators/generators.py:141-167, :299-325), bit-exact with Pillow's Image.resize.
// Pillow resamples in two passes with a uint8 image in between; each output sample is
//   clip8((2^21 + sum_k pixel[first + k] * tap[k]) >> 22)
// in 32-bit integers, the taps being double-precision filter weights rounded to 22 fractional bits.  The taps depend on the
// two sizes only, so the host computes them (data/image_prep.py:resample_coeffs, which also states the whole contract in
// numpy) and they travel with the pixels; everything that touches a pixel runs here.
//
// Only what the crop window needs is computed: the horizontal pass produces the window's T columns for the source rows
// that the window's vertical taps read (`row0`, `n_rows` of the descriptor) into the scratch buffer, the vertical pass
// reads those and writes the window, mirrored when the flip is set.  One launch per pass covers the ragged batch:
// blockIdx.y is the image, blockIdx.x runs over the largest image's samples and the blocks past a smaller image leave at
// once.  One thread owns one pixel (three accumulators); neighbouring lanes read neighbouring source bytes and the taps
// are shared by all rows (horizontal pass) or by the whole wave (vertical pass), so both passes live in L1 / L2.
#include "dj_resample.h"

#define DJ_IMGPREP_THREADS 256
#define DJ_IMGPREP_MAX_SIDE DJ_RESAMPLE_MAX_SIDE
#define DJ_IMGPREP_MAX_TARGET 8192

__global__ __launch_bounds__(DJ_IMGPREP_THREADS) void dj_imgprep_h_kernel(const unsigned char* __restrict__ src,
                                                                          const dj_image_prep_desc* __restrict__ desc,
                                                                          const int* __restrict__ pool,
                                                                          unsigned char* __restrict__ scratch, int T) {
  const dj_image_prep_desc d = desc[blockIdx.y];
  const int idx = blockIdx.x * DJ_IMGPREP_THREADS + threadIdx.x;
  if (idx >= d.n_rows * T) return;
  const int r = idx / T, j = idx - r * T;
  const int col = d.crop_x + j;
  const int* bounds = pool + d.h_bounds + 2 * col;
  const int first = bounds[0], n = bounds[1];
  const int* taps = pool + d.h_taps + (long)col * d.h_ksize;
  const unsigned char* p = src + d.src_offset + (long)(d.row0 + r) * d.src_stride + 3L * first;
  int s0, s1, s2;
  dj_accumulate_taps(p, 3, taps, n, s0, s1, s2);
  dj_store_clip8(scratch + d.scratch_offset + ((long)r * T + j) * 3, s0, s1, s2);
}

__global__ __launch_bounds__(DJ_IMGPREP_THREADS) void dj_imgprep_v_kernel(const unsigned char* __restrict__ scratch,
                                                                          const dj_image_prep_desc* __restrict__ desc,
                                                                          const int* __restrict__ pool,
                                                                          unsigned char* __restrict__ out, long out_stride,
                                                                          int T) {
  const dj_image_prep_desc d = desc[blockIdx.y];
  const int idx = blockIdx.x * DJ_IMGPREP_THREADS + threadIdx.x;
  if (idx >= T * T) return;
  const int y = idx / T, j = idx - y * T;
  const int row = d.crop_y + y;
  const int jj = d.flip ? T - 1 - j : j;      // FLIP_LEFT_RIGHT on the store
  dj_vertical_sample(pool + d.v_bounds + 2 * row, pool + d.v_taps + (long)row * d.v_ksize,
                     scratch + d.scratch_offset + 3L * j, d.row0, 3L * T,
                     out + ((long)blockIdx.y * T + y) * out_stride + 3L * jj);
}

extern "C" long dj_image_prep_scratch_bytes(const dj_image_prep_desc* desc_host, int batch, int target) {
  if (!desc_host || batch < 1 || target < 1 || target > DJ_IMGPREP_MAX_TARGET) {
    dj_set_error("image_prep_scratch_bytes: null descriptors, batch %d or target %d out of range", batch, target);
    return DJ_ERR_ARG;
  }
  long total = 0;
  for (int i = 0; i < batch; ++i) {
    if (desc_host[i].n_rows < 1 || desc_host[i].n_rows > DJ_IMGPREP_MAX_SIDE) {
      dj_set_error("image_prep_scratch_bytes: image %d: n_rows %d outside 1..%d", i, desc_host[i].n_rows, DJ_IMGPREP_MAX_SIDE);
      return DJ_ERR_ARG;
    }
    total += dj_scratch_region_bytes(3L * target * desc_host[i].n_rows);
  }
  return total;
}

extern "C" int dj_image_prep(const unsigned char* src, long src_bytes, const dj_image_prep_desc* desc_dev,
                             const dj_image_prep_desc* desc_host, int batch, const int* pool_dev, const int* pool_host,
                             long pool_ints, int target, unsigned char* out, long out_stride_bytes, unsigned char* scratch,
                             long scratch_bytes, void* stream) {
  DJ_CHECK_ARG(src, "image_prep: src is null");
  DJ_CHECK_ARG(desc_dev, "image_prep: desc_dev is null");
  DJ_CHECK_ARG(desc_host, "image_prep: desc_host is null");
  DJ_CHECK_ARG(pool_dev, "image_prep: pool_dev is null");
  DJ_CHECK_ARG(pool_host, "image_prep: pool_host is null");
  DJ_CHECK_ARG(out, "image_prep: out is null");
  DJ_CHECK_ARG(scratch, "image_prep: scratch is null");
  DJ_CHECK_ARG(batch >= 1 && batch <= 65535, "image_prep: batch must be in 1..65535 (got %d)", batch);
  DJ_CHECK_ARG(target >= 1 && target <= DJ_IMGPREP_MAX_TARGET, "image_prep: target must be in 1..%d (got %d)",
               DJ_IMGPREP_MAX_TARGET, target);
  DJ_CHECK_ARG(out_stride_bytes >= 3L * target, "image_prep: out_stride_bytes %ld below 3 * target = %ld", out_stride_bytes,
               3L * target);
  DJ_CHECK_ARG(src_bytes >= 1 && pool_ints >= 1 && scratch_bytes >= 1, "image_prep: src_bytes / pool_ints / scratch_bytes must be >= 1");
  const int T = target;
  long scratch_end = 0;
  int max_rows = 0;
  for (int i = 0; i < batch; ++i) {
    const dj_image_prep_desc* d = desc_host + i;
    DJ_CHECK_ARG(d->src_h >= 1 && d->src_w >= 1 && d->src_h <= DJ_IMGPREP_MAX_SIDE && d->src_w <= DJ_IMGPREP_MAX_SIDE,
                 "image_prep: image %d: source size %d x %d outside 1..%d", i, d->src_h, d->src_w, DJ_IMGPREP_MAX_SIDE);
    DJ_CHECK_ARG(d->res_h >= 1 && d->res_w >= 1 && d->res_h <= DJ_IMGPREP_MAX_SIDE && d->res_w <= DJ_IMGPREP_MAX_SIDE,
                 "image_prep: image %d: resized size %d x %d outside 1..%d", i, d->res_h, d->res_w, DJ_IMGPREP_MAX_SIDE);
    DJ_CHECK_ARG(d->src_stride >= 3L * d->src_w, "image_prep: image %d: src_stride %ld below 3 * width = %ld", i, d->src_stride,
                 3L * d->src_w);
    DJ_CHECK_ARG(d->src_offset >= 0 && d->src_offset + (d->src_h - 1) * d->src_stride + 3L * d->src_w <= src_bytes,
                 "image_prep: image %d: pixels at offset %ld leave the source buffer of %ld bytes", i, d->src_offset, src_bytes);
    DJ_CHECK_ARG(d->crop_x >= 0 && d->crop_y >= 0 && (long)d->crop_x + T <= d->res_w && (long)d->crop_y + T <= d->res_h,
                 "image_prep: image %d: the %d x %d window at (x %d, y %d) leaves the resized %d x %d image", i, T, T, d->crop_x,
                 d->crop_y, d->res_w, d->res_h);
    DJ_CHECK_ARG(d->row0 >= 0 && d->n_rows >= 1 && (long)d->row0 + d->n_rows <= d->src_h,
                 "image_prep: image %d: source rows [%d, %d + %d) leave the image of %d rows", i, d->row0, d->row0, d->n_rows,
                 d->src_h);
    if (dj_check_axis("image_prep", "horizontal", i, d->h_bounds, d->h_taps, d->h_ksize, d->res_w, pool_ints) != DJ_OK ||
        dj_check_axis("image_prep", "vertical", i, d->v_bounds, d->v_taps, d->v_ksize, d->res_h, pool_ints) != DJ_OK)
      return DJ_ERR_ARG;
    // every read of the two passes stays inside the source rows / the scratch rows
    for (int j = 0; j < T; ++j) {
      const int* bh = pool_host + d->h_bounds + 2L * (d->crop_x + j);
      DJ_CHECK_ARG(bh[0] >= 0 && bh[1] >= 0 && bh[1] <= d->h_ksize && (long)bh[0] + bh[1] <= d->src_w,
                   "image_prep: image %d: column %d reads source columns [%d, %d + %d) of %d (tap row length %d)", i,
                   d->crop_x + j, bh[0], bh[0], bh[1], d->src_w, d->h_ksize);
      const int* bv = pool_host + d->v_bounds + 2L * (d->crop_y + j);
      DJ_CHECK_ARG(bv[0] >= d->row0 && bv[1] >= 0 && bv[1] <= d->v_ksize && (long)bv[0] + bv[1] <= (long)d->row0 + d->n_rows,
                   "image_prep: image %d: row %d reads source rows [%d, %d + %d) outside [%d, %d + %d) (tap row length %d)", i,
                   d->crop_y + j, bv[0], bv[0], bv[1], d->row0, d->row0, d->n_rows, d->v_ksize);
    }
    if (dj_check_scratch_region("image_prep", i, d->scratch_offset, 3L * T * d->n_rows, &scratch_end, scratch_bytes) != DJ_OK)
      return DJ_ERR_ARG;
    if (d->n_rows > max_rows) max_rows = d->n_rows;
  }
  const dim3 block(DJ_IMGPREP_THREADS);
  const dim3 grid_h((unsigned)dj_cdiv((long)max_rows * T, DJ_IMGPREP_THREADS), (unsigned)batch);
  const dim3 grid_v((unsigned)dj_cdiv((long)T * T, DJ_IMGPREP_THREADS), (unsigned)batch);
  hipLaunchKernelGGL(dj_imgprep_h_kernel, grid_h, block, 0, (hipStream_t)stream, src, desc_dev, pool_dev, scratch, T);
  DJ_CHECK_LAUNCH("dj_image_prep (horizontal pass)");
  hipLaunchKernelGGL(dj_imgprep_v_kernel, grid_v, block, 0, (hipStream_t)stream, scratch, desc_dev, pool_dev, out,
                     out_stride_bytes, T);
  DJ_CHECK_LAUNCH("dj_image_prep (vertical pass)");
  return DJ_OK;
}
