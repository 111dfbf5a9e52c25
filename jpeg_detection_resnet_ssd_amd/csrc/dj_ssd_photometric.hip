// The photometric stage of the SSD augmentation chain (`SSDPhotometricDistortions`: brightness, contrast, saturation, hue
// around an RGB -> HSV -> RGB round trip in one of two orders, then a channel order), IN PLACE on the staged rectangles of a
// ragged batch, before dj_patch_resize reads them: byte for byte what data/ssd_photometric.py:ssd_photometric_host states
// in numpy.  Every operation is pointwise, so distorting the staged part of an image equals distorting the image.
//
// What decides bits (the module's docstring has the whole contract):
//   * between bytes the arithmetic is float32 and every operation rounds on its own: this file is compiled with
//     contraction OFF; bytes are made with rintf (round half to even), as np.round does;
//   * the hue is np.remainder(H + delta, 180): fmodf, lifted by 180 when negative -- which can round to exactly 180.0, a
//     byte the conversion back accepts;
//   * RGB -> HSV is OpenCV's 8-bit integer form with 12 fractional bits.  Its two reciprocal tables are rint((255 << 12) / i)
//     and rint((180 << 12) / (6 i)): rounded quotients, which a truncating integer division is not.  Each workgroup makes
//     them in LDS with one double-precision division per thread (correctly rounded, as the host's);
//   * HSV -> RGB is OpenCV's float32 form.  H <= 180 here, so H * (6.f / 180.f) <= 6.0000005 and fmodf(h, 6.f) is h - 6.f
//     exactly whenever h >= 6.f.
//
// One thread owns one pixel: three byte loads, the whole function in registers, three byte stores.  The record of the
// image selects the operations, so every branch on it is uniform over the workgroup.  blockIdx.y is the image, blockIdx.x
// runs over the largest rectangle's pixels and the blocks past a smaller one leave at once (an image with nothing staged
// costs only that), as in dj_patchresize.hip.
#include "dj_resample.h"

#pragma clang fp contract(off)

#define DJ_SSDP_THREADS 256
#define DJ_SSDP_SHIFT 12
#define DJ_SSDP_ALL (DJ_SSD_PHOTO_BRIGHTNESS | DJ_SSD_PHOTO_CONTRAST | DJ_SSD_PHOTO_SATURATION | DJ_SSD_PHOTO_HUE)

__device__ __forceinline__ float ssdp_clip(float x) { return fminf(fmaxf(x, 0.f), 255.f); }

__device__ __forceinline__ float ssdp_contrast(float x, float factor) {
  return ssdp_clip(127.5f + factor * (x - 127.5f));
}

__device__ __forceinline__ float ssdp_pick(int k, float c0, float c1, float c2) { return k == 0 ? c0 : (k == 1 ? c1 : c2); }

__global__ __launch_bounds__(DJ_SSDP_THREADS) void dj_ssd_photometric_kernel(unsigned char* __restrict__ src,
                                                                             const dj_patch_resize_desc* __restrict__ desc,
                                                                             const dj_ssd_photo_params* __restrict__ params) {
  __shared__ int sdiv[256], hdiv[256];
  const dj_patch_resize_desc d = desc[blockIdx.y];
  const int n = d.src_h * d.src_w;      // the host copy was checked: below 2^31
  if ((int)(blockIdx.x * DJ_SSDP_THREADS) >= n) return;
  {
    const int i = threadIdx.x;          // DJ_SSDP_THREADS == 256: one entry of each table per thread
    sdiv[i] = i ? (int)rint((double)(255 << DJ_SSDP_SHIFT) / (double)i) : 0;
    hdiv[i] = i ? (int)rint((double)(180 << DJ_SSDP_SHIFT) / (6.0 * (double)i)) : 0;
  }
  __syncthreads();
  const int idx = blockIdx.x * DJ_SSDP_THREADS + threadIdx.x;
  if (idx >= n) return;
  const dj_ssd_photo_params q = params[blockIdx.y];
  const int y = idx / d.src_w, x = idx - y * d.src_w;
  unsigned char* p = src + d.src_offset + (long)y * d.src_stride + 3L * x;

  float c0 = p[0], c1 = p[1], c2 = p[2];
  if (q.flags & DJ_SSD_PHOTO_BRIGHTNESS) {
    c0 = ssdp_clip(c0 + q.brightness);
    c1 = ssdp_clip(c1 + q.brightness);
    c2 = ssdp_clip(c2 + q.brightness);
  }
  if (q.sequence == 1 && (q.flags & DJ_SSD_PHOTO_CONTRAST)) {
    c0 = ssdp_contrast(c0, q.contrast);
    c1 = ssdp_contrast(c1, q.contrast);
    c2 = ssdp_contrast(c2, q.contrast);
  }
  // -> uint8, RGB -> HSV
  const int r = (int)rintf(c0), g = (int)rintf(c1), b = (int)rintf(c2);
  const int v = max(max(r, g), b), diff = v - min(min(r, g), b);
  const int si = (diff * sdiv[v] + (1 << (DJ_SSDP_SHIFT - 1))) >> DJ_SSDP_SHIFT;
  const int term = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
  int hi = (term * hdiv[diff] + (1 << (DJ_SSDP_SHIFT - 1))) >> DJ_SSDP_SHIFT;      // arithmetic shift: term may be negative
  hi += hi < 0 ? 180 : 0;
  // saturation and hue in float32, -> uint8
  float hf = (float)hi, sf = (float)si;
  if (q.flags & DJ_SSD_PHOTO_SATURATION) sf = ssdp_clip(sf * q.saturation);
  if (q.flags & DJ_SSD_PHOTO_HUE) {
    float m = fmodf(hf + q.hue, 180.f);
    if (m < 0.f) m += 180.f;            // np.remainder: the sign of the divisor
    hf = m;
  }
  const int H = (int)rintf(hf), S = (int)rintf(sf);
  // HSV -> RGB
  const float scale = 1.f / 255.f;
  const float s = (float)S * scale, vv = (float)v * scale;
  float fr = vv, fg = vv, fb = vv;
  if (S != 0) {                         // s == 0 exactly when S == 0
    float h = (float)H * (6.f / 180.f);
    if (h >= 6.f) h -= 6.f;
    const float fl = floorf(h);
    int sector = (int)fl;
    float f = h - fl;
    if ((unsigned)sector >= 6u) {
      sector = 0;
      f = 0.f;
    }
    const float t0 = vv, t1 = vv * (1.f - s), t2 = vv * (1.f - s * f), t3 = vv * (1.f - s * (1.f - f));
    // (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}][sector]
    fb = sector == 0 || sector == 1 ? t1 : (sector == 2 ? t3 : (sector == 5 ? t2 : t0));
    fg = sector == 0 ? t3 : (sector == 1 || sector == 2 ? t0 : (sector == 3 ? t2 : t1));
    fr = sector == 0 || sector == 5 ? t0 : (sector == 1 ? t2 : (sector == 4 ? t3 : t1));
  }
  c0 = ssdp_clip(rintf(fr * 255.f));
  c1 = ssdp_clip(rintf(fg * 255.f));
  c2 = ssdp_clip(rintf(fb * 255.f));
  if (q.sequence != 1 && (q.flags & DJ_SSD_PHOTO_CONTRAST)) {
    c0 = rintf(ssdp_contrast(c0, q.contrast));
    c1 = rintf(ssdp_contrast(c1, q.contrast));
    c2 = rintf(ssdp_contrast(c2, q.contrast));
  }
  // the host copy's order was checked; the device copy only selects among the three registers
  p[0] = (unsigned char)(int)ssdp_pick(q.order[0], c0, c1, c2);
  p[1] = (unsigned char)(int)ssdp_pick(q.order[1], c0, c1, c2);
  p[2] = (unsigned char)(int)ssdp_pick(q.order[2], c0, c1, c2);
}

extern "C" int dj_ssd_photometric(unsigned char* src, long src_bytes, const dj_patch_resize_desc* desc_dev,
                                  const dj_patch_resize_desc* desc_host, const dj_ssd_photo_params* params_dev,
                                  const dj_ssd_photo_params* params_host, int batch, void* stream) {
  DJ_CHECK_ARG(src, "ssd_photometric: src is null");
  DJ_CHECK_ARG(desc_dev, "ssd_photometric: desc_dev is null");
  DJ_CHECK_ARG(desc_host, "ssd_photometric: desc_host is null");
  DJ_CHECK_ARG(params_dev, "ssd_photometric: params_dev is null");
  DJ_CHECK_ARG(params_host, "ssd_photometric: params_host is null");
  DJ_CHECK_ARG(batch >= 1 && batch <= 65535, "ssd_photometric: batch must be in 1..65535 (got %d)", batch);
  DJ_CHECK_ARG(src_bytes >= 1, "ssd_photometric: src_bytes must be >= 1");
  long max_pixels = 0;
  for (int i = 0; i < batch; ++i) {
    const dj_patch_resize_desc* d = desc_host + i;
    const dj_ssd_photo_params* q = params_host + i;
    if (dj_check_staged_rect("ssd_photometric", i, d, src_bytes) != DJ_OK) return DJ_ERR_ARG;
    const long pixels = (long)d->src_h * d->src_w;
    DJ_CHECK_ARG(pixels <= 0x7fffffffL, "ssd_photometric: image %d: %d x %d staged pixels, at most 2^31 - 1 are supported", i,
                 d->src_h, d->src_w);
    DJ_CHECK_ARG(q->sequence == 1 || q->sequence == 2, "ssd_photometric: image %d: sequence %d is neither 1 nor 2", i,
                 q->sequence);
    DJ_CHECK_ARG((q->flags & ~DJ_SSDP_ALL) == 0, "ssd_photometric: image %d: flags 0x%x name an unknown operation", i, q->flags);
    const float par[4] = {q->brightness, q->contrast, q->saturation, q->hue};
    for (int k = 0; k < 4; ++k)         // of operations that are off, too: they travel as zero
      DJ_CHECK_ARG(par[k] - par[k] == 0.f, "ssd_photometric: image %d: parameter %d (brightness, contrast, saturation, hue) is not finite",
                   i, k);
    int seen = 0;
    for (int k = 0; k < 3; ++k)
      if (q->order[k] >= 0 && q->order[k] <= 2) seen |= 1 << q->order[k];
    DJ_CHECK_ARG(seen == 7, "ssd_photometric: image %d: order (%d, %d, %d) is no permutation of (0, 1, 2)", i, q->order[0],
                 q->order[1], q->order[2]);
    if (pixels > max_pixels) max_pixels = pixels;
  }
  if (max_pixels == 0) return DJ_OK;    // nothing is staged: every window misses its image
  const dim3 grid((unsigned)dj_cdiv(max_pixels, DJ_SSDP_THREADS), (unsigned)batch);
  hipLaunchKernelGGL(dj_ssd_photometric_kernel, grid, dim3(DJ_SSDP_THREADS), 0, (hipStream_t)stream, src, desc_dev,
                     params_dev);
  DJ_CHECK_LAUNCH("dj_ssd_photometric");
  return DJ_OK;
}
