// Dropout on the device: a stateless Philox4x32-10 mask, equal bit for bit to keras/dropout.py (the host statement).
// Element i takes lane (i & 3) of the Philox block whose counter is (lo32(i >> 2), hi32(i >> 2), ctr2, ctr3) under the
// key (key0, key1); it is kept iff that word >= threshold.  The caller packs (seed, rank, step) into key0, key1, ctr2,
// ctr3 as keras/dropout.py states.  y = (x * scale) * keep with keep 0.0f / 1.0f: a product, not a select, so an Inf or
// NaN at a dropped position gives NaN as TensorFlow's x * scale * mask does.
#include "../../include/dj_hip.h"
#include "dj_common.h"

#define DJ_DROPOUT_MAX_BLOCKS 4096

static inline int ew_blocks(long total) {
  long b = (total + 255) / 256;
  return (int)(b < 1 ? 1 : (b > DJ_DROPOUT_MAX_BLOCKS ? DJ_DROPOUT_MAX_BLOCKS : b));
}

struct dj_philox_out {
  uint32_t w[4];
};

__device__ __forceinline__ dj_philox_out dj_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                          uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0;
    c1 = lo1;
    c2 = n2;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  dj_philox_out o;
  o.w[0] = c0;
  o.w[1] = c1;
  o.w[2] = c2;
  o.w[3] = c3;
  return o;
}

// One thread per group of four consecutive elements.  VEC4: src / dst (and nothing else) are 16-byte aligned, so whole
// groups move as one 16-byte load and store; the last, partial group and every group of an unaligned tensor go element
// by element.  BWD: dst = beta ? dst + v : v.  src == dst is fine: a thread reads its own four elements before it writes.
template <bool VEC4, bool BWD>
__global__ __launch_bounds__(256) void dj_dropout_kernel(const float* src, float* dst, long n, uint32_t threshold,
                                                         float scale, uint32_t key0, uint32_t key1, uint32_t ctr2,
                                                         uint32_t ctr3, int beta) {
  const long groups = (n + 3) >> 2;
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
    dj_philox_out r = dj_philox4x32_10((uint32_t)g, (uint32_t)((unsigned long)g >> 32), ctr2, ctr3, key0, key1);
    const long i0 = g << 2;
    if (VEC4 && i0 + 4 <= n) {
      f32x4 v = *reinterpret_cast<const f32x4*>(src + i0);
      v.x = (v.x * scale) * (r.w[0] >= threshold ? 1.f : 0.f);
      v.y = (v.y * scale) * (r.w[1] >= threshold ? 1.f : 0.f);
      v.z = (v.z * scale) * (r.w[2] >= threshold ? 1.f : 0.f);
      v.w = (v.w * scale) * (r.w[3] >= threshold ? 1.f : 0.f);
      if (BWD && beta) v += *reinterpret_cast<const f32x4*>(dst + i0);
      *reinterpret_cast<f32x4*>(dst + i0) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long i = i0 + e;
        if (i < n) {
          float v = (src[i] * scale) * (r.w[e] >= threshold ? 1.f : 0.f);
          dst[i] = (BWD && beta) ? dst[i] + v : v;
        }
      }
    }
  }
}

template <bool BWD>
static int dropout_launch(const char* name, const float* src, float* dst, long n, unsigned threshold, float scale,
                          unsigned key0, unsigned key1, unsigned ctr2, unsigned ctr3, int beta, void* stream) {
  DJ_CHECK_ARG(src && dst && n > 0, "%s: bad arguments (src %p, dst %p, n %ld)", name, (const void*)src, (void*)dst, n);
  DJ_CHECK_ARG(beta == 0 || beta == 1, "%s: beta must be 0 or 1, got %d", name, beta);
  const bool v4 = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  const dim3 grid(ew_blocks((n + 3) >> 2));
  if (v4)
    hipLaunchKernelGGL((dj_dropout_kernel<true, BWD>), grid, dim3(256), 0, (hipStream_t)stream, src, dst, n,
                       (uint32_t)threshold, scale, (uint32_t)key0, (uint32_t)key1, (uint32_t)ctr2, (uint32_t)ctr3, beta);
  else
    hipLaunchKernelGGL((dj_dropout_kernel<false, BWD>), grid, dim3(256), 0, (hipStream_t)stream, src, dst, n,
                       (uint32_t)threshold, scale, (uint32_t)key0, (uint32_t)key1, (uint32_t)ctr2, (uint32_t)ctr3, beta);
  DJ_CHECK_LAUNCH(name);
  return DJ_OK;
}

extern "C" long dj_dropout_groups_per_pass(void) { return (long)DJ_DROPOUT_MAX_BLOCKS * 256; }

extern "C" int dj_dropout_fwd(const float* x, float* y, long n, unsigned threshold, float scale, unsigned key0,
                              unsigned key1, unsigned ctr2, unsigned ctr3, void* stream) {
  return dropout_launch<false>("dj_dropout_fwd", x, y, n, threshold, scale, key0, key1, ctr2, ctr3, 0, stream);
}

extern "C" int dj_dropout_bwd(const float* dy, float* dx, long n, unsigned threshold, float scale, unsigned key0,
                              unsigned key1, unsigned ctr2, unsigned ctr3, int beta, void* stream) {
  return dropout_launch<true>("dj_dropout_bwd", dy, dx, n, threshold, scale, key0, key1, ctr2, ctr3, beta, stream);
}
