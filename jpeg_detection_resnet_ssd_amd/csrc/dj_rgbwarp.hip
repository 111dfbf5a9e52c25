// Keras' ImageDataGenerator applied to a [batch][H][W][3] uint8 tensor, written as float32 NHWC straight into a model's
// input buffer: the affine warp, the flips and the standardisation of
//   ImageDataGenerator(rotation_range, shear_range, zoom_range, vertical_flip, preprocessing_function=preprocess_input)
// that the reference feeds its RGB ResNet50 with (classification_part/config/resnetRGB/config_file.py:157-172).  Per image
// Keras runs scipy.ndimage.affine_transform(order=1, mode='nearest') once per colour channel in float64;
// data/rgb_warp.py states that (`affine_warp_host`) and the whole call (`rgb_warp_host`), and this file equals both bit
// for bit.  What decides bits:
//
//   coordinates   r = (m0 * i + m1 * j) + m2, c = (m3 * i + m4 * j) + m5 in float64.  This file is compiled with contraction
//                 OFF: every product and sum rounds on its own, as scipy's C loop and numpy's elementwise loops do.
//   nearest fill  r and c are clipped to the image before the split into floor and fraction; the neighbour one past the
//                 last row / column is that row / column again.
//   value         (((x00 * (1-tr)) * (1-tc) + (x01 * (1-tr)) * tc) + (x10 * tr) * (1-tc)) + (x11 * tr) * tc in float64, left
//                 to right, rounded once to float32.
//   then          the flips as index mirroring (output pixel (i, j) is warped pixel (H-1-i, W-1-j) where flipped), the
//                 caffe preprocessing (channels reversed, float32 mean subtracted) and the float32 rescale.
//
// One thread makes four consecutive output pixels: the coordinate work of a pixel is shared by its three channels, and the
// twelve floats leave as three 16-byte stores.  The source image (150 KB at 224 x 224) is gathered from cache; no LDS.
#include "../../include/dj_hip.h"
#include "dj_common.h"

#pragma clang fp contract(off)

#define DJ_WARP_MAX_SIDE 32768
#define DJ_WARP_MAX_BLOCKS 65536

// The three float32 values of output pixel (i, j) of image `img`, record fields passed by value.
__device__ __forceinline__ void warp_pixel(const unsigned char* __restrict__ img, int H, int W, const double m[6],
                                           int identity, int flip_cols, int flip_rows, int i, int j, int prep,
                                           int has_rescale, float rescale, float* o) {
  const int si = flip_rows ? H - 1 - i : i, sj = flip_cols ? W - 1 - j : j;
  float v0, v1, v2;
  if (identity) {
    const unsigned char* p = img + 3L * ((long)si * W + sj);
    v0 = (float)p[0];
    v1 = (float)p[1];
    v2 = (float)p[2];
  } else {
    const double di = (double)si, dj = (double)sj;
    double r = (m[0] * di + m[1] * dj) + m[2];
    double c = (m[3] * di + m[4] * dj) + m[5];
    // fmax / fmin return the operand that is a number: whatever the device copy of the record holds, the indices below
    // stay inside the image
    r = fmin(fmax(r, 0.0), (double)(H - 1));
    c = fmin(fmax(c, 0.0), (double)(W - 1));
    const double fr = floor(r), fc = floor(c);
    const double tr = r - fr, tc = c - fc;
    const double ur = 1.0 - tr, uc = 1.0 - tc;
    const int r0 = (int)fr, c0 = (int)fc;
    const int r1 = min(r0 + 1, H - 1), c1 = min(c0 + 1, W - 1);
    const unsigned char* p00 = img + 3L * ((long)r0 * W + c0);
    const unsigned char* p01 = img + 3L * ((long)r0 * W + c1);
    const unsigned char* p10 = img + 3L * ((long)r1 * W + c0);
    const unsigned char* p11 = img + 3L * ((long)r1 * W + c1);
    float v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double x00 = (double)p00[k], x01 = (double)p01[k], x10 = (double)p10[k], x11 = (double)p11[k];
      const double acc = (((x00 * ur) * uc + (x01 * ur) * tc) + (x10 * tr) * uc) + (x11 * tr) * tc;
      v[k] = (float)acc;
    }
    v0 = v[0];
    v1 = v[1];
    v2 = v[2];
  }
  if (prep == DJ_RGB_PREP_CAFFE) {
    const float b = v2 - 103.939f, g = v1 - 116.779f, rd = v0 - 123.68f;
    v0 = b;
    v1 = g;
    v2 = rd;
  }
  if (has_rescale) {
    v0 = v0 * rescale;
    v1 = v1 * rescale;
    v2 = v2 * rescale;
  }
  o[0] = v0;
  o[1] = v1;
  o[2] = v2;
}

// The output is n_runs runs of run_len consecutive pixels, run s starting at out + s * run_stride floats: the whole batch
// as one run when its rows are dense, one run per pixel row otherwise.  Pixel p of run s is pixel s * run_len + p of the
// batch in [image][row][column] order.  One thread per group of four pixels of a run.  VEC4: every run starts 16-byte
// aligned, so whole groups leave as three 16-byte stores; the last, partial group of a run and every group of an
// unaligned output go element by element.
template <bool VEC4>
__global__ __launch_bounds__(256) void dj_rgb_warp_kernel(const unsigned char* __restrict__ pixels, int H, int W,
                                                          const dj_rgb_warp_record* __restrict__ rec, int prep,
                                                          int has_rescale, float rescale, float* __restrict__ out,
                                                          long n_runs, long run_len, long run_stride) {
  const long groups = (run_len + 3) >> 2;
  const long total = n_runs * groups;
  const long image_pixels = (long)H * W;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const long s = t / groups;
    const long p0 = (t - s * groups) << 2;
    const int n = (int)min(4L, run_len - p0);
    float* dst = out + s * run_stride + 3 * p0;
    float o[12];
    long b_have = -1;
    double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int identity = 1, flip_cols = 0, flip_rows = 0;
    const unsigned char* img = pixels;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < n) {
        const long g = s * run_len + p0 + e;
        const long b = g / image_pixels;
        const int rem = (int)(g - b * image_pixels);
        const int i = rem / W, j = rem - i * W;
        if (b != b_have) {               // a group may straddle two images of a dense batch
          const dj_rgb_warp_record* mine = rec + b;
#pragma unroll
          for (int k = 0; k < 6; ++k) m[k] = mine->m[k];
          identity = mine->identity;
          flip_cols = mine->flip_cols;
          flip_rows = mine->flip_rows;
          img = pixels + b * image_pixels * 3;
          b_have = b;
        }
        warp_pixel(img, H, W, m, identity, flip_cols, flip_rows, i, j, prep, has_rescale, rescale, o + 3 * e);
      }
    }
    if (VEC4 && n == 4) {
      f32x4 a, b4, c;
      a.x = o[0], a.y = o[1], a.z = o[2], a.w = o[3];
      b4.x = o[4], b4.y = o[5], b4.z = o[6], b4.w = o[7];
      c.x = o[8], c.y = o[9], c.z = o[10], c.w = o[11];
      reinterpret_cast<f32x4*>(dst)[0] = a;
      reinterpret_cast<f32x4*>(dst)[1] = b4;
      reinterpret_cast<f32x4*>(dst)[2] = c;
    } else {
#pragma unroll
      for (int e = 0; e < 12; ++e)
        if (e < 3 * n) dst[e] = o[e];
    }
  }
}

extern "C" int dj_rgb_warp(const unsigned char* pixels, int batch, int height, int width,
                           const dj_rgb_warp_record* rec_dev, const dj_rgb_warp_record* rec_host, int preprocess,
                           int has_rescale, float rescale, float* out, long out_row_stride, void* stream) {
  DJ_CHECK_ARG(pixels, "rgb_warp: pixels is null");
  DJ_CHECK_ARG(rec_dev, "rgb_warp: rec_dev is null");
  DJ_CHECK_ARG(rec_host, "rgb_warp: rec_host is null");
  DJ_CHECK_ARG(out, "rgb_warp: out is null");
  DJ_CHECK_ARG(batch >= 1, "rgb_warp: batch must be positive (got %d)", batch);
  DJ_CHECK_ARG(height >= 1 && width >= 1 && height <= DJ_WARP_MAX_SIDE && width <= DJ_WARP_MAX_SIDE,
               "rgb_warp: size (height x width) %d x %d outside 1..%d", height, width, DJ_WARP_MAX_SIDE);
  DJ_CHECK_ARG(out_row_stride >= 3L * width, "rgb_warp: out_row_stride %ld below 3 * width = %ld", out_row_stride,
               3L * width);
  DJ_CHECK_ARG(preprocess == DJ_RGB_PREP_NONE || preprocess == DJ_RGB_PREP_CAFFE,
               "rgb_warp: unknown preprocess code %d", preprocess);
  DJ_CHECK_ARG(!has_rescale || rescale - rescale == 0.0f, "rgb_warp: rescale is not finite");
  for (int i = 0; i < batch; ++i) {
    if (rec_host[i].identity) continue;
    for (int k = 0; k < 6; ++k)
      DJ_CHECK_ARG(rec_host[i].m[k] - rec_host[i].m[k] == 0.0, "rgb_warp: image %d: matrix entry %d is not finite", i, k);
  }
  const bool dense = out_row_stride == 3L * width;
  const long n_runs = dense ? 1 : (long)batch * height;
  const long run_len = dense ? (long)batch * height * width : (long)width;
  const long run_stride = dense ? 0 : out_row_stride;
  const bool v4 = ((uintptr_t)out & 15) == 0 && (dense || (out_row_stride & 3) == 0);
  const long threads = n_runs * ((run_len + 3) >> 2);
  long blocks = (threads + 255) / 256;
  if (blocks > DJ_WARP_MAX_BLOCKS) blocks = DJ_WARP_MAX_BLOCKS;
  if (v4)
    hipLaunchKernelGGL((dj_rgb_warp_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pixels, height,
                       width, rec_dev, preprocess, has_rescale, rescale, out, n_runs, run_len, run_stride);
  else
    hipLaunchKernelGGL((dj_rgb_warp_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pixels, height,
                       width, rec_dev, preprocess, has_rescale, rescale, out, n_runs, run_len, run_stride);
  DJ_CHECK_LAUNCH("dj_rgb_warp");
  return DJ_OK;
}
