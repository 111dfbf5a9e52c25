// keras.optimizers.SGD, Adam (with amsgrad), Adadelta, RMSprop, Adagrad, Adamax and Nadam: one memory-bound pass over a
// segment of the flat parameter buffer, equal bit for bit to sgd_host / adam_host / adadelta_host / rmsprop_host /
// adagrad_host / adamax_host / nadam_host of keras/optimizers.py (the host statement).  All
// arithmetic is fp32, every product, sum, quotient and square root rounded once in the order the statement writes them:
// nothing is contracted into an fma, hence the pragma, and the fmas of the SGD statement are written out as
// __builtin_fmaf; the division and sqrtf are hipcc's correctly rounded expansions.
//
// A rule is a struct of its state pointers, its scalars and the update of one element.  Everything else exists once, in
// dj_optim_kernel and optim_launch.  One thread per group of four consecutive elements in a grid-stride loop over at most
// DJ_OPTIM_MAX_BLOCKS workgroups of 256 threads.  VEC4: every pointer is 16-byte aligned, so whole groups move as 16-byte
// loads and stores; the last, partial group and every group of an unaligned launch go element by element.  Every stream
// is read once and written once per step and a segment of a real model is far larger than the L2, so the gradient and the
// state buffers move with non-temporal loads and stores; the parameters, which the next forward pass reads, keep the
// default policy.  sumsq != NULL: sum(p^2) of the pre-update parameters goes through dj_sumsq_finish; the slots are
// shared by all rules.
//
// SGD used to be a kernel of its own in dj_loss.hip (one element per thread, 4096 workgroups, default cache policy, null
// checks only).  As a rule of this file it gained the four-per-thread geometry, so that dj_optim_groups_per_pass()
// describes it too, the non-temporal gradient and velocity streams, and the refusal of overlapping buffers.
#pragma clang fp contract(off)
#include <atomic>
#include <cstdio>

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

// ---- the rules: NS state buffers, their names for the error texts, and element(p, g, s[NS]) ------------------------------

// t = (2*l2)*p ; g' = fma(g, grad_scale, t) ; v = momentum*v - lr_t*g' ; p = nesterov ? fma(momentum, v, p) - lr_t*g' : p + v
// -- what hipcc made of the plain expressions while it was free to contract them; the select is wave-uniform
struct DjSgdRule {
  static constexpr int NS = 1;
  static constexpr const char* NAME = "dj_sgd_momentum_update";
  static constexpr const char* BUFFERS = "param, grad and velocity";
  static constexpr const char* STATE[NS] = {"velocity"};
  float* state[NS];
  float lr_t, momentum, l2x2, grad_scale;
  int nesterov;
  __device__ __forceinline__ void element(float& p, float g, float (&s)[NS]) const {
    const float ge = __builtin_fmaf(g, grad_scale, l2x2 * p);
    const float step = lr_t * ge;
    const float v = momentum * s[0] - step;
    s[0] = v;
    p = nesterov ? __builtin_fmaf(momentum, v, p) - step : p + v;
  }
};

struct DjAdamScalars {
  float lr_t, b1, b2, omb1, omb2, eps, l2x2, grad_scale;
};

// np.maximum: a NaN on either side gives NaN
__device__ __forceinline__ float max_nan(float a, float b) { return (b > a || b != b) ? b : a; }

template <bool AMSGRAD>
struct DjAdamRule {
  static constexpr int NS = AMSGRAD ? 3 : 2;
  static constexpr const char* NAME = "dj_adam_update";
  static constexpr const char* BUFFERS = "param, grad, m, v and vhat";
  static constexpr const char* STATE[3] = {"m", "v", "vhat"};
  float* state[NS];
  DjAdamScalars k;
  __device__ __forceinline__ void element(float& p, float g, float (&s)[NS]) const {
    const float ge = g * k.grad_scale + k.l2x2 * p;
    s[0] = k.b1 * s[0] + k.omb1 * ge;
    s[1] = k.b2 * s[1] + k.omb2 * (ge * ge);
    float d = s[1];
    if (AMSGRAD) {
      s[NS - 1] = max_nan(s[NS - 1], s[1]);
      d = s[NS - 1];
    }
    p = p - (k.lr_t * s[0]) / (sqrtf(d) + k.eps);
  }
};

struct DjAdadeltaRule {
  static constexpr int NS = 2;
  static constexpr const char* NAME = "dj_adadelta_update";
  static constexpr const char* BUFFERS = "param, grad, accum and delta_accum";
  static constexpr const char* STATE[NS] = {"accum", "delta_accum"};
  float* state[NS];
  float lr, rho, omr, eps, l2x2, grad_scale;
  __device__ __forceinline__ void element(float& p, float g, float (&s)[NS]) const {
    const float ge = g * grad_scale + l2x2 * p;
    s[0] = rho * s[0] + omr * (ge * ge);
    const float u = (ge * sqrtf(s[1] + eps)) / sqrtf(s[0] + eps);
    p = p - lr * u;
    s[1] = rho * s[1] + omr * (u * u);
  }
};

// a = rho*a + (1 - rho)*g'^2 ; p = p - (lr*g') / (sqrt(a) + eps)
struct DjRmspropRule {
  static constexpr int NS = 1;
  static constexpr const char* NAME = "dj_rmsprop_update";
  static constexpr const char* BUFFERS = "param, grad and accum";
  static constexpr const char* STATE[NS] = {"accum"};
  float* state[NS];
  float lr, rho, omr, eps, l2x2, grad_scale;
  __device__ __forceinline__ void element(float& p, float g, float (&s)[NS]) const {
    const float ge = g * grad_scale + l2x2 * p;
    s[0] = rho * s[0] + omr * (ge * ge);
    p = p - (lr * ge) / (sqrtf(s[0]) + eps);
  }
};

// a = a + g'^2 ; p as RMSprop's
struct DjAdagradRule {
  static constexpr int NS = 1;
  static constexpr const char* NAME = "dj_adagrad_update";
  static constexpr const char* BUFFERS = "param, grad and accum";
  static constexpr const char* STATE[NS] = {"accum"};
  float* state[NS];
  float lr, eps, l2x2, grad_scale;
  __device__ __forceinline__ void element(float& p, float g, float (&s)[NS]) const {
    const float ge = g * grad_scale + l2x2 * p;
    s[0] = s[0] + ge * ge;
    p = p - (lr * ge) / (sqrtf(s[0]) + eps);
  }
};

// Adam's first moment; u = max(b2*u, |g'|), the infinity norm, with np.maximum's NaN; no square root
struct DjAdamaxRule {
  static constexpr int NS = 2;
  static constexpr const char* NAME = "dj_adamax_update";
  static constexpr const char* BUFFERS = "param, grad, m and u";
  static constexpr const char* STATE[NS] = {"m", "u"};
  float* state[NS];
  float lr_t, b1, b2, omb1, eps, l2x2, grad_scale;
  __device__ __forceinline__ void element(float& p, float g, float (&s)[NS]) const {
    const float ge = g * grad_scale + l2x2 * p;
    s[0] = b1 * s[0] + omb1 * ge;
    s[1] = max_nan(b2 * s[1], __builtin_fabsf(ge));
    p = p - (lr_t * s[0]) / (s[1] + eps);
  }
};

struct DjNadamScalars {
  float lr, b1, b2, omb1, omb2, eps, c_g, c_m, c_v, omc_t, mc_t1, l2x2, grad_scale;
};

// Adam's two moments, each bias-corrected by a product with a reciprocal the caller made (c_g, c_m, c_v), and the
// Nesterov mix mbar = (1 - mc_t)*g'*c_g + mc_t1*m*c_m of the momentum schedule
struct DjNadamRule {
  static constexpr int NS = 2;
  static constexpr const char* NAME = "dj_nadam_update";
  static constexpr const char* BUFFERS = "param, grad, m and v";
  static constexpr const char* STATE[NS] = {"m", "v"};
  float* state[NS];
  DjNadamScalars k;
  __device__ __forceinline__ void element(float& p, float g, float (&s)[NS]) const {
    const float ge = g * k.grad_scale + k.l2x2 * p;
    s[0] = k.b1 * s[0] + k.omb1 * ge;
    s[1] = k.b2 * s[1] + k.omb2 * (ge * ge);
    const float mbar = k.omc_t * (ge * k.c_g) + k.mc_t1 * (s[0] * k.c_m);
    p = p - (k.lr * mbar) / (sqrtf(s[1] * k.c_v) + k.eps);
  }
};

// ---- the pass ----------------------------------------------------------------------------------------------------------
template <class Rule, bool VEC4>
__global__ __launch_bounds__(256) void dj_optim_kernel(float* p, const float* g, long n, Rule r, float* sumsq, int slot) {
  constexpr int NS = Rule::NS;
  float acc = 0.f;
  const long groups = (n + 3) >> 2;
  for (long gi = (long)blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += (long)gridDim.x * blockDim.x) {
    const long i0 = gi << 2;
    if (VEC4 && i0 + 4 <= n) {
      f32x4 pv = *reinterpret_cast<const f32x4*>(p + i0);
      const f32x4 gv = ld_stream(g + i0);
      f32x4 sv[NS];
#pragma unroll
      for (int k = 0; k < NS; ++k) sv[k] = ld_stream(r.state[k] + i0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pv[e], se[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) se[k] = sv[k][e];
        acc += pe * pe;
        r.element(pe, gv[e], se);
        pv[e] = pe;
#pragma unroll
        for (int k = 0; k < NS; ++k) sv[k][e] = se[k];
      }
      *reinterpret_cast<f32x4*>(p + i0) = pv;
#pragma unroll
      for (int k = 0; k < NS; ++k) st_stream(r.state[k] + i0, sv[k]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long i = i0 + e;
        if (i < n) {
          float pi = p[i], si[NS];
#pragma unroll
          for (int k = 0; k < NS; ++k) si[k] = r.state[k][i];
          acc += pi * pi;
          r.element(pi, g[i], si);
          p[i] = pi;
#pragma unroll
          for (int k = 0; k < NS; ++k) r.state[k][i] = si[k];
        }
      }
    }
  }
  if (sumsq) dj_sumsq_finish(acc, &dj_optim_slots[slot], sumsq);
}

static inline bool overlaps(const float* a, const float* b, long n) { return a < b + n && b < a + n; }

static int next_slot(const float* sumsq) {
  static std::atomic<unsigned> next{0};
  return sumsq ? (int)(next.fetch_add(1u) % DJ_SUMSQ_SLOTS) : 0;
}

// The checks and the launch of every rule: no null pointer and n > 0; no two of param, grad and the state buffers
// overlap; the 16-byte path only if every one of them is 16-byte aligned.
template <class Rule>
static int optim_launch(float* param, const float* grad, long n, const Rule& r, float* sumsq, void* stream) {
  const float* buf[2 + Rule::NS] = {param, grad};
  bool present = param && grad;
  char list[160];
  int len = snprintf(list, sizeof list, "param %p, grad %p", (void*)param, (const void*)grad);
  for (int k = 0; k < Rule::NS; ++k) {
    buf[2 + k] = r.state[k];
    present = present && r.state[k];
    len += snprintf(list + len, sizeof list - len, ", %s %p", Rule::STATE[k], (void*)r.state[k]);
  }
  DJ_CHECK_ARG(present && n > 0, "%s: bad arguments (%s, n %ld)", Rule::NAME, list, n);
  uintptr_t bits = 0;
  for (int a = 0; a < 2 + Rule::NS; ++a) {
    bits |= (uintptr_t)buf[a];
    for (int b = a + 1; b < 2 + Rule::NS; ++b)
      DJ_CHECK_ARG(!overlaps(buf[a], buf[b], n), "%s: %s must not overlap", Rule::NAME, Rule::BUFFERS);
  }
  const dim3 grid(optim_blocks((n + 3) >> 2)), block(256);
  const int slot = next_slot(sumsq);
  if ((bits & 15) == 0)
    hipLaunchKernelGGL((dj_optim_kernel<Rule, true>), grid, block, 0, (hipStream_t)stream, param, grad, n, r, sumsq, slot);
  else
    hipLaunchKernelGGL((dj_optim_kernel<Rule, false>), grid, block, 0, (hipStream_t)stream, param, grad, n, r, sumsq, slot);
  DJ_CHECK_LAUNCH(Rule::NAME);
  return DJ_OK;
}

extern "C" long dj_optim_groups_per_pass(void) { return (long)DJ_OPTIM_MAX_BLOCKS * 256; }

extern "C" int dj_sgd_momentum_update(float* param, const float* grad, float* velocity, long n, float lr_t,
                                      float momentum, int nesterov, float l2, float grad_scale, float* sumsq,
                                      void* stream) {
  return optim_launch(param, grad, n, DjSgdRule{{velocity}, lr_t, momentum, l2 + l2, grad_scale, nesterov}, sumsq, stream);
}

extern "C" int dj_adam_update(float* param, const float* grad, float* m, float* v, float* vhat, long n, float lr_t,
                              float beta_1, float beta_2, float epsilon, float l2, float grad_scale, float* sumsq,
                              void* stream) {
  const DjAdamScalars k = {lr_t, beta_1, beta_2, 1.f - beta_1, 1.f - beta_2, epsilon, 2.f * l2, grad_scale};
  if (vhat) return optim_launch(param, grad, n, DjAdamRule<true>{{m, v, vhat}, k}, sumsq, stream);
  return optim_launch(param, grad, n, DjAdamRule<false>{{m, v}, k}, sumsq, stream);
}

extern "C" int dj_adadelta_update(float* param, const float* grad, float* accum, float* delta_accum, long n, float lr,
                                  float rho, float one_minus_rho, float epsilon, float l2, float grad_scale,
                                  float* sumsq, void* stream) {
  return optim_launch(param, grad, n,
                      DjAdadeltaRule{{accum, delta_accum}, lr, rho, one_minus_rho, epsilon, 2.f * l2, grad_scale}, sumsq,
                      stream);
}

extern "C" int dj_rmsprop_update(float* param, const float* grad, float* accum, long n, float lr, float rho, float epsilon,
                                 float l2, float grad_scale, float* sumsq, void* stream) {
  return optim_launch(param, grad, n, DjRmspropRule{{accum}, lr, rho, 1.f - rho, epsilon, 2.f * l2, grad_scale}, sumsq,
                      stream);
}

extern "C" int dj_adagrad_update(float* param, const float* grad, float* accum, long n, float lr, float epsilon, float l2,
                                 float grad_scale, float* sumsq, void* stream) {
  return optim_launch(param, grad, n, DjAdagradRule{{accum}, lr, epsilon, 2.f * l2, grad_scale}, sumsq, stream);
}

extern "C" int dj_adamax_update(float* param, const float* grad, float* m, float* u, long n, float lr_t, float beta_1,
                                float beta_2, float epsilon, float l2, float grad_scale, float* sumsq, void* stream) {
  return optim_launch(param, grad, n, DjAdamaxRule{{m, u}, lr_t, beta_1, beta_2, 1.f - beta_1, epsilon, 2.f * l2, grad_scale},
                      sumsq, stream);
}

extern "C" int dj_nadam_update(float* param, const float* grad, float* m, float* v, long n, float lr, float beta_1,
                               float beta_2, float epsilon, float c_g, float c_m, float c_v, float one_minus_mc_t,
                               float mc_t1, float l2, float grad_scale, float* sumsq, void* stream) {
  const DjNadamScalars k = {lr, beta_1, beta_2, 1.f - beta_1, 1.f - beta_2, epsilon, c_g, c_m,
                            c_v, one_minus_mc_t, mc_t1, 2.f * l2, grad_scale};
  return optim_launch(param, grad, n, DjNadamRule{{m, v}, k}, sumsq, stream);
}
