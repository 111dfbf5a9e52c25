// Validation metrics accumulated on the device over a whole sweep: top-k / categorical accuracy hit counts and the
// weighted sum of the per-batch loss, without a host round trip per batch.
// Reference: classification_part/config/resnet/config_file.py:19-22 (top_k_categorical_accuracy, Keras 2.2.4 ->
// tf.nn.in_top_k), keras.metrics.categorical_accuracy, and Model.evaluate_generator's batch-size-weighted averages
// (classification_part/vgg_jpeg_keras/evaluation/evaluators.py:13-22).
#include "../../include/dj_hip.h"
#include "dj_common.h"

#define DJ_METRIC_MAX_K 8
#define DJ_METRIC_MAX_BLOCKS 1024

struct MetricKs {
  int k[DJ_METRIC_MAX_K];
};

// np.argmax order on (value, index) pairs: a NaN beats every number, otherwise the larger value wins, and equal
// candidates (two NaNs, or -0.0 and 0.0) resolve to the lower index.  Indices are compared explicitly, so neither the
// order in which a lane meets its classes nor the shape of the butterfly matters.
__device__ __forceinline__ bool metric_better(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn || bn) return vn && (!bn || i < bi);
  return v > bv || (v == bv && i < bi);
}

__device__ __forceinline__ void metric_wave_argmax(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    if (metric_better(ov, oi, v, i)) {
      v = ov;
      i = oi;
    }
  }
}

// One wave per row, rows strided over the waves of the grid; lanes stride over the classes (VEC: four consecutive
// classes per lane and load, C % 4 == 0 and both bases 16-byte aligned).  A wave keeps its hit counts in registers over
// all its rows; the block adds them up in LDS and makes at most n_k integer atomics.  The loss term and the row count have
// one writer, thread 0 of block 0: calls on one stream are serial, so the sums are taken in call order.
template <bool VEC>
__global__ __launch_bounds__(256) void dj_eval_accumulate_kernel(const float* __restrict__ y_true,
                                                                  const float* __restrict__ probs, long rows, int C,
                                                                  MetricKs ks, int n_k, const float* loss_mean,
                                                                  double loss_weight, double* acc,
                                                                  unsigned long long* counts) {
  __shared__ int hits_lds[4][DJ_METRIC_MAX_K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int hits[DJ_METRIC_MAX_K];
#pragma unroll
  for (int q = 0; q < DJ_METRIC_MAX_K; ++q) hits[q] = 0;

  for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += (long)gridDim.x * 4) {
    const float* tr = y_true + row * C;
    const float* pr = probs + row * C;
    // first maximum of y_true (the target) and of probs (categorical_accuracy), one pass over both rows
    float tv = 0.f, pv = 0.f;
    int ti = C, pi = C;     // C: "nothing seen yet", loses against every real candidate below
    if (VEC) {
      for (int c = lane * 4; c < C; c += 256) {
        const f32x4 t4 = *reinterpret_cast<const f32x4*>(tr + c);
        const f32x4 p4 = *reinterpret_cast<const f32x4*>(pr + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (ti == C || metric_better(t4[e], c + e, tv, ti)) {
            tv = t4[e];
            ti = c + e;
          }
          if (pi == C || metric_better(p4[e], c + e, pv, pi)) {
            pv = p4[e];
            pi = c + e;
          }
        }
      }
    } else {
      for (int c = lane; c < C; c += 64) {
        const float t = tr[c], p = pr[c];
        if (ti == C || metric_better(t, c, tv, ti)) {
          tv = t;
          ti = c;
        }
        if (pi == C || metric_better(p, c, pv, pi)) {
          pv = p;
          pi = c;
        }
      }
    }
    // lanes beyond C hold (-inf, C): below every number, and behind every real index among equals
    if (ti == C) tv = -INFINITY;
    if (pi == C) pv = -INFINITY;
    metric_wave_argmax(tv, ti);
    metric_wave_argmax(pv, pi);
    // tf.nn.in_top_k: classes strictly above the target's probability; a NaN compares false
    const float pt = pr[ti];
    int above = 0;
    if (VEC) {
      for (int c = lane * 4; c < C; c += 256) {
        const f32x4 p4 = *reinterpret_cast<const f32x4*>(pr + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) above += p4[e] > pt ? 1 : 0;
      }
    } else {
      for (int c = lane; c < C; c += 64) above += pr[c] > pt ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o);
    const bool finite = fabsf(pt) <= 3.402823466e+38f;     // false for NaN and +-Inf
#pragma unroll
    for (int q = 0; q < DJ_METRIC_MAX_K; ++q) {
      if (q < n_k) {
        const int k = ks.k[q];
        hits[q] += (k == 0 ? pi == ti : (finite && above < k)) ? 1 : 0;
      }
    }
  }

  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < DJ_METRIC_MAX_K; ++q) hits_lds[wave][q] = hits[q];
  }
  __syncthreads();
  if ((int)threadIdx.x < n_k) {
    const int q = threadIdx.x;
    const int h = hits_lds[0][q] + hits_lds[1][q] + hits_lds[2][q] + hits_lds[3][q];
    if (h) atomicAdd(&counts[1 + q], (unsigned long long)h);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    counts[0] += (unsigned long long)rows;
    if (loss_mean) {
#pragma clang fp contract(off)      // product and sum round separately, as the host's float64 statement does
      const double term = loss_weight * (double)loss_mean[0];
      acc[0] = acc[0] + term;
      acc[1] = acc[1] + loss_weight;
    }
  }
}

extern "C" int dj_eval_accumulate(const float* y_true, const float* probs, long rows, int C, const int* ks_host, int n_k,
                                  const float* loss_mean, double loss_weight, double* acc, long long* counts,
                                  void* stream) {
  DJ_CHECK_ARG(acc && counts, "eval_accumulate: acc / counts is null");
  DJ_CHECK_ARG(n_k >= 0 && n_k <= DJ_METRIC_MAX_K, "eval_accumulate: n_k = %d, at most %d metrics per call", n_k,
               DJ_METRIC_MAX_K);
  DJ_CHECK_ARG(n_k == 0 || ks_host, "eval_accumulate: ks is null");
  DJ_CHECK_ARG(rows >= 0, "eval_accumulate: rows = %ld", rows);
  DJ_CHECK_ARG(rows == 0 || C > 0, "eval_accumulate: C = %d with rows = %ld", C, rows);
  MetricKs ks;
  for (int q = 0; q < DJ_METRIC_MAX_K; ++q) ks.k[q] = 0;
  for (int q = 0; q < n_k; ++q) {
    // a loss-only call that states no class count (rows == 0, C <= 0) keeps the k entries of the pass it belongs to
    DJ_CHECK_ARG(ks_host[q] >= 0 && (ks_host[q] <= C || (rows == 0 && C <= 0)),
                 "eval_accumulate: k = %d is outside 0..C = %d", ks_host[q], C);
    ks.k[q] = ks_host[q];
  }
  if (!y_true || !probs) rows = 0;      // loss only (a detection model, a custom loss)
  if (rows == 0 && !loss_mean) return DJ_OK;
  long blocks = (rows + 3) / 4;
  blocks = blocks < 1 ? 1 : (blocks > DJ_METRIC_MAX_BLOCKS ? DJ_METRIC_MAX_BLOCKS : blocks);
  const bool vec = rows > 0 && C % 4 == 0 && (((uintptr_t)y_true | (uintptr_t)probs) & 15) == 0;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
  if (vec)
    hipLaunchKernelGGL(dj_eval_accumulate_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, y_true,
                       probs, rows, C, ks, n_k, loss_mean, loss_weight, acc, cnt);
  else
    hipLaunchKernelGGL(dj_eval_accumulate_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, y_true,
                       probs, rows, C, ks, n_k, loss_mean, loss_weight, acc, cnt);
  DJ_CHECK_LAUNCH("dj_eval_accumulate");
  return DJ_OK;
}
