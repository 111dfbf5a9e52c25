// keras.optimizers.Adam (with amsgrad) and Adadelta: one memory-bound pass over a segment of the flat parameter buffer,
// equal bit for bit to adam_host / adadelta_host of keras/optimizers.py (the host statement).  All arithmetic is fp32,
// every product, sum, quotient and square root rounded once in the order the statement writes them: nothing may be
// contracted into an fma, hence the pragma; the division and sqrtf are hipcc's correctly rounded expansions.
//
// One thread per group of four consecutive elements in a grid-stride loop over at most DJ_OPTIM_MAX_BLOCKS workgroups of
// 256 threads.  VEC4: every pointer is 16-byte aligned, so whole groups move as 16-byte loads and stores; the last,
// partial group and every group of an unaligned launch go element by element.  Every stream is read once and written
// once per step and a segment of a real model is far larger than the L2, so the gradient and the state buffers move with
// non-temporal loads and stores; the parameters, which the next forward pass reads, keep the default policy.
#pragma clang fp contract(off)
#include <atomic>

#include "../../include/dj_hip.h"
#include "dj_common.h"
#include "dj_sumsq.h"

#define DJ_OPTIM_MAX_BLOCKS 2048
#ifndef DJ_OPTIM_NT
#define DJ_OPTIM_NT 1   // 0: default cache policy on every stream (for measurements)
#endif

static inline int optim_blocks(long groups) {
  long b = (groups + 255) / 256;
  return (int)(b < 1 ? 1 : (b > DJ_OPTIM_MAX_BLOCKS ? DJ_OPTIM_MAX_BLOCKS : b));
}

__device__ DjSumsqSlot dj_optim_slots[DJ_SUMSQ_SLOTS];

__device__ __forceinline__ f32x4 ld_stream(const float* p) {
#if DJ_OPTIM_NT
  return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
#else
  return *reinterpret_cast<const f32x4*>(p);
#endif
}
__device__ __forceinline__ void st_stream(float* p, f32x4 v) {
#if DJ_OPTIM_NT
  __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p));
#else
  *reinterpret_cast<f32x4*>(p) = v;
#endif
}

struct DjAdamScalars {
  float lr_t, b1, b2, omb1, omb2, eps, l2x2, grad_scale;
};

// np.maximum: a NaN on either side gives NaN
__device__ __forceinline__ float max_nan(float a, float b) { return (b > a || b != b) ? b : a; }

template <bool AMSGRAD>
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float& vh, const DjAdamScalars& k,
                                             float& acc) {
  acc += p * p;
  const float ge = g * k.grad_scale + k.l2x2 * p;
  m = k.b1 * m + k.omb1 * ge;
  v = k.b2 * v + k.omb2 * (ge * ge);
  float d = v;
  if (AMSGRAD) {
    vh = max_nan(vh, v);
    d = vh;
  }
  p = p - (k.lr_t * m) / (sqrtf(d) + k.eps);
}

template <bool AMSGRAD, bool VEC4>
__global__ __launch_bounds__(256) void dj_adam_kernel(float* p, const float* g, float* m, float* v, float* vhat, long n,
                                                       DjAdamScalars k, float* sumsq, int slot) {
  float acc = 0.f;
  const long groups = (n + 3) >> 2;
  for (long gi = (long)blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += (long)gridDim.x * blockDim.x) {
    const long i0 = gi << 2;
    if (VEC4 && i0 + 4 <= n) {
      f32x4 pv = *reinterpret_cast<const f32x4*>(p + i0);
      const f32x4 gv = ld_stream(g + i0);
      f32x4 mv = ld_stream(m + i0), vv = ld_stream(v + i0), hv = {0.f, 0.f, 0.f, 0.f};
      if (AMSGRAD) hv = ld_stream(vhat + i0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pv[e], me = mv[e], ve = vv[e], he = hv[e];
        adam_element<AMSGRAD>(pe, gv[e], me, ve, he, k, acc);
        pv[e] = pe;
        mv[e] = me;
        vv[e] = ve;
        hv[e] = he;
      }
      *reinterpret_cast<f32x4*>(p + i0) = pv;
      st_stream(m + i0, mv);
      st_stream(v + i0, vv);
      if (AMSGRAD) st_stream(vhat + i0, hv);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long i = i0 + e;
        if (i < n) {
          float pi = p[i], mi = m[i], vi = v[i], hi = AMSGRAD ? vhat[i] : 0.f;
          adam_element<AMSGRAD>(pi, g[i], mi, vi, hi, k, acc);
          p[i] = pi;
          m[i] = mi;
          v[i] = vi;
          if (AMSGRAD) vhat[i] = hi;
        }
      }
    }
  }
  if (sumsq) dj_sumsq_finish(acc, &dj_optim_slots[slot], sumsq);
}

struct DjAdadeltaScalars {
  float lr, rho, omr, eps, l2x2, grad_scale;
};

__device__ __forceinline__ void adadelta_element(float& p, float g, float& a, float& d, const DjAdadeltaScalars& k,
                                                 float& acc) {
  acc += p * p;
  const float ge = g * k.grad_scale + k.l2x2 * p;
  a = k.rho * a + k.omr * (ge * ge);
  const float u = (ge * sqrtf(d + k.eps)) / sqrtf(a + k.eps);
  p = p - k.lr * u;
  d = k.rho * d + k.omr * (u * u);
}

template <bool VEC4>
__global__ __launch_bounds__(256) void dj_adadelta_kernel(float* p, const float* g, float* a, float* d, long n,
                                                           DjAdadeltaScalars k, float* sumsq, int slot) {
  float acc = 0.f;
  const long groups = (n + 3) >> 2;
  for (long gi = (long)blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += (long)gridDim.x * blockDim.x) {
    const long i0 = gi << 2;
    if (VEC4 && i0 + 4 <= n) {
      f32x4 pv = *reinterpret_cast<const f32x4*>(p + i0);
      const f32x4 gv = ld_stream(g + i0);
      f32x4 av = ld_stream(a + i0), dv = ld_stream(d + i0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pv[e], ae = av[e], de = dv[e];
        adadelta_element(pe, gv[e], ae, de, k, acc);
        pv[e] = pe;
        av[e] = ae;
        dv[e] = de;
      }
      *reinterpret_cast<f32x4*>(p + i0) = pv;
      st_stream(a + i0, av);
      st_stream(d + i0, dv);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long i = i0 + e;
        if (i < n) {
          float pi = p[i], ai = a[i], di = d[i];
          adadelta_element(pi, g[i], ai, di, k, acc);
          p[i] = pi;
          a[i] = ai;
          d[i] = di;
        }
      }
    }
  }
  if (sumsq) dj_sumsq_finish(acc, &dj_optim_slots[slot], sumsq);
}

static inline bool overlaps(const float* a, const float* b, long n) {
  return a && b && a < b + n && b < a + n;
}

static int next_slot(const float* sumsq) {
  static std::atomic<unsigned> next{0};
  return sumsq ? (int)(next.fetch_add(1u) % DJ_SUMSQ_SLOTS) : 0;
}

extern "C" long dj_optim_groups_per_pass(void) { return (long)DJ_OPTIM_MAX_BLOCKS * 256; }

extern "C" int dj_adam_update(float* param, const float* grad, float* m, float* v, float* vhat, long n, float lr_t,
                              float beta_1, float beta_2, float epsilon, float l2, float grad_scale, float* sumsq,
                              void* stream) {
  DJ_CHECK_ARG(param && grad && m && v && n > 0, "dj_adam_update: bad arguments (param %p, grad %p, m %p, v %p, n %ld)",
               (void*)param, (const void*)grad, (void*)m, (void*)v, n);
  DJ_CHECK_ARG(!overlaps(param, m, n) && !overlaps(param, v, n) && !overlaps(param, vhat, n) && !overlaps(m, v, n) &&
                   !overlaps(m, vhat, n) && !overlaps(v, vhat, n) && !overlaps(param, grad, n),
               "dj_adam_update: param, grad, m, v and vhat must not overlap");
  const DjAdamScalars k = {lr_t, beta_1, beta_2, 1.f - beta_1, 1.f - beta_2, epsilon, 2.f * l2, grad_scale};
  const long groups = (n + 3) >> 2;
  const bool v4 = (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v | (uintptr_t)vhat) & 15) == 0;
  const dim3 grid(optim_blocks(groups)), block(256);
  const int slot = next_slot(sumsq);
  hipStream_t s = (hipStream_t)stream;
  if (vhat) {
    if (v4)
      hipLaunchKernelGGL((dj_adam_kernel<true, true>), grid, block, 0, s, param, grad, m, v, vhat, n, k, sumsq, slot);
    else
      hipLaunchKernelGGL((dj_adam_kernel<true, false>), grid, block, 0, s, param, grad, m, v, vhat, n, k, sumsq, slot);
  } else {
    if (v4)
      hipLaunchKernelGGL((dj_adam_kernel<false, true>), grid, block, 0, s, param, grad, m, v, vhat, n, k, sumsq, slot);
    else
      hipLaunchKernelGGL((dj_adam_kernel<false, false>), grid, block, 0, s, param, grad, m, v, vhat, n, k, sumsq, slot);
  }
  DJ_CHECK_LAUNCH("dj_adam_update");
  return DJ_OK;
}

extern "C" int dj_adadelta_update(float* param, const float* grad, float* accum, float* delta_accum, long n, float lr,
                                  float rho, float one_minus_rho, float epsilon, float l2, float grad_scale,
                                  float* sumsq, void* stream) {
  DJ_CHECK_ARG(param && grad && accum && delta_accum && n > 0,
               "dj_adadelta_update: bad arguments (param %p, grad %p, accum %p, delta_accum %p, n %ld)", (void*)param,
               (const void*)grad, (void*)accum, (void*)delta_accum, n);
  DJ_CHECK_ARG(!overlaps(param, accum, n) && !overlaps(param, delta_accum, n) && !overlaps(accum, delta_accum, n) &&
                   !overlaps(param, grad, n),
               "dj_adadelta_update: param, grad, accum and delta_accum must not overlap");
  const DjAdadeltaScalars k = {lr, rho, one_minus_rho, epsilon, 2.f * l2, grad_scale};
  const long groups = (n + 3) >> 2;
  const bool v4 = (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)accum | (uintptr_t)delta_accum) & 15) == 0;
  const dim3 grid(optim_blocks(groups)), block(256);
  const int slot = next_slot(sumsq);
  hipStream_t s = (hipStream_t)stream;
  if (v4)
    hipLaunchKernelGGL((dj_adadelta_kernel<true>), grid, block, 0, s, param, grad, accum, delta_accum, n, k, sumsq, slot);
  else
    hipLaunchKernelGGL((dj_adadelta_kernel<false>), grid, block, 0, s, param, grad, accum, delta_accum, n, k, sumsq, slot);
  DJ_CHECK_LAUNCH("dj_adadelta_update");
  return DJ_OK;
}
