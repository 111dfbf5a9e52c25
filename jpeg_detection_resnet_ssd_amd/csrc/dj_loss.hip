// Softmax, the SSD multibox loss with batch-wide hard-negative mining, categorical
// cross-entropy and global average pooling.
// Reference: localisation_part/keras_loss_function/keras_ssd_loss.py:53-211 (SSDLoss),
// localisation_part/models/keras_ssd300_dct_j2d_resnet.py:873 (softmax),
// classification_part/config/resnet/config_file.py:58-65 (categorical_crossentropy).
#include "../../include/dj_hip.h"
#include "dj_common.h"

static inline int ew_blocks(long total) {
  long b = (total + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// ---------------------------------------------------------------------------------
// softmax over the last axis: one row per group of G = 8 / 16 / 32 / 64 lanes (the 21-class rows of the SSD head: two rows per
// wave).  The xor butterfly of a group is the tail of the 64-lane butterfly, whose first steps would only add the
// identity held by the lanes beyond C -- same bits for any G >= C.
// ---------------------------------------------------------------------------------
static inline int softmax_group(int C) {
  int g = 8;
  while (g < 64 && g < C) g <<= 1;
  return g;
}

__global__ __launch_bounds__(256) void dj_softmax_fwd_kernel(const float* x, float* y, long rows, int C, int G) {
  const int per_wave = 64 / G;
  const int lane = threadIdx.x & 63, sub = lane / G, l = lane - sub * G;
  long row = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * per_wave + sub;
  const bool live = row < rows;
  const float* xr = x + (live ? row : 0) * C;
  float m = -INFINITY;
  if (live)
    for (int c = l; c < C; c += G) m = fmaxf(m, xr[c]);
  for (int o = G >> 1; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  float s = 0.f;
  if (live)
    for (int c = l; c < C; c += G) s += expf(xr[c] - m);
  for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (!live) return;
  float inv = 1.f / s;
  float* yr = y + row * C;
  for (int c = l; c < C; c += G) yr[c] = expf(xr[c] - m) * inv;
}

// dx (+)= p * (dp - sum(dp*p))
__global__ __launch_bounds__(256) void dj_softmax_bwd_kernel(const float* p, const float* dp, long ld_dp, float* dx,
                                                              long rows, int C, int beta, int G) {
  const int per_wave = 64 / G;
  const int lane = threadIdx.x & 63, sub = lane / G, l = lane - sub * G;
  long row = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * per_wave + sub;
  const bool live = row < rows;
  const float* pr = p + (live ? row : 0) * C;
  const float* gr = dp + (live ? row : 0) * ld_dp;
  float dot = 0.f;
  if (live)
    for (int c = l; c < C; c += G) dot += pr[c] * gr[c];
  for (int o = G >> 1; o > 0; o >>= 1) dot += __shfl_xor(dot, o);
  if (!live) return;
  float* dr = dx + row * C;
  for (int c = l; c < C; c += G) {
    float v = pr[c] * (gr[c] - dot);
    dr[c] = beta ? dr[c] + v : v;
  }
}

extern "C" int dj_softmax_fwd(const float* x, float* y, long rows, int C, void* stream) {
  DJ_CHECK_ARG(x && y && rows > 0 && C > 0, "softmax_fwd: bad arguments");
  const int G = softmax_group(C);
  hipLaunchKernelGGL(dj_softmax_fwd_kernel, dim3((unsigned)dj_cdiv(rows, 4 * (64 / G))), dim3(256), 0, (hipStream_t)stream,
                     x, y, rows, C, G);
  DJ_CHECK_LAUNCH("dj_softmax_fwd");
  return DJ_OK;
}

extern "C" int dj_softmax_bwd(const float* p, const float* dp, long ld_dp, float* dx, long rows, int C, int beta,
                              void* stream) {
  DJ_CHECK_ARG(p && dp && dx && rows > 0 && C > 0 && ld_dp >= C, "softmax_bwd: bad arguments");
  const int G = softmax_group(C);
  hipLaunchKernelGGL(dj_softmax_bwd_kernel, dim3((unsigned)dj_cdiv(rows, 4 * (64 / G))), dim3(256), 0, (hipStream_t)stream,
                     p, dp, ld_dp, dx, rows, C, beta, G);
  DJ_CHECK_LAUNCH("dj_softmax_bwd");
  return DJ_OK;
}

// ---------------------------------------------------------------------------------
// SSD multibox loss.  y_true / y_pred rows are [n_cls | 4 loc | 8 ignored].
//   per-box pass : cls[i] = -sum_c y_c log(max(p_c,1e-15)); loc[i] = smooth-L1; pos; negloss = cls*y_0
//   mining pass  : keep the k largest negloss over the WHOLE batch,
//                  k = min(max(ratio*n_pos, n_neg_min), #nonzero negloss); ties by lowest index
//   result       : out[0] = (sum pos*cls + sum keep*cls + alpha*sum pos*loc) / max(1, n_pos)
//                  out[1] = n_pos, out[2] = k, out[3] = class part, out[4] = loc part
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dj_ssd_loss_boxes_kernel(const float* y_true, const float* y_pred, long nbox,
                                                                 int n_cls, float* cls, float* loc, float* pos,
                                                                 float* negloss, float* partial) {
  __shared__ float red[4][256];
  const int W = n_cls + 12;
  float s_pos = 0.f, s_pc = 0.f, s_pl = 0.f, s_nz = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nbox; i += (long)gridDim.x * blockDim.x) {
    const float* t = y_true + i * W;
    const float* p = y_pred + i * W;
    float cl = 0.f, pmax = 0.f;
    for (int c = 0; c < n_cls; ++c) {
      float yc = t[c];
      if (yc != 0.f) cl -= yc * logf(fmaxf(p[c], 1e-15f));
      if (c >= 1) pmax = (c == 1) ? yc : fmaxf(pmax, yc);
    }
    float lo = 0.f;
    for (int j = 0; j < 4; ++j) {
      float d = t[n_cls + j] - p[n_cls + j];
      float a = fabsf(d);
      lo += (a < 1.f) ? 0.5f * d * d : a - 0.5f;
    }
    cls[i] = cl;
    loc[i] = lo;
    pos[i] = pmax;
    negloss[i] = cl * t[0];
    s_nz += (cl * t[0] != 0.f) ? 1.f : 0.f;
    s_pos += pmax;
    s_pc += cl * pmax;
    s_pl += lo * pmax;
  }
  red[0][threadIdx.x] = s_pos;
  red[1][threadIdx.x] = s_pc;
  red[2][threadIdx.x] = s_pl;
  red[3][threadIdx.x] = s_nz;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      red[0][threadIdx.x] += red[0][threadIdx.x + o];
      red[1][threadIdx.x] += red[1][threadIdx.x + o];
      red[2][threadIdx.x] += red[2][threadIdx.x + o];
      red[3][threadIdx.x] += red[3][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[blockIdx.x * 4 + 0] = red[0][0];
    partial[blockIdx.x * 4 + 1] = red[1][0];
    partial[blockIdx.x * 4 + 2] = red[2][0];
    partial[blockIdx.x * 4 + 3] = red[3][0];
  }
}

// ---- batch-wide hard-negative mining: exact k-th largest negative loss by a 3-level radix select (11+11+10
// bits of the fp32 pattern; losses are >= 0 so the patterns order like unsigned ints), spread over many workgroups.
// Every workgroup re-derives the selection state from the small global histograms, so no host round trip and no
// single-block pass over the batch is needed.  Ties at the threshold are resolved by arrival order (tf.nn.top_k
// leaves tie order unspecified as well).
#define DJ_HB 2048
struct MineState {
  long k;          // negatives to keep
  unsigned prefix; // selected high bits so far
  long need;       // how many still to take from the current prefix class
  double npos, spc, spl;
};

__device__ __forceinline__ void mine_reduce_partials(const float* partial, int npartial, double* out4) {
  __shared__ double red4[4][256];
  double a[4] = {0, 0, 0, 0};
  for (int b = threadIdx.x; b < npartial; b += blockDim.x)
    for (int q = 0; q < 4; ++q) a[q] += (double)partial[b * 4 + q];
  for (int q = 0; q < 4; ++q) red4[q][threadIdx.x] = a[q];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int q = 0; q < 4; ++q) red4[q][threadIdx.x] += red4[q][threadIdx.x + o];
    __syncthreads();
  }
  for (int q = 0; q < 4; ++q) out4[q] = red4[q][0];
  __syncthreads();
}

// scan one histogram level from the top: find the bin where the cumulative count reaches `need`
// (256 threads: LDS copy, per-thread run of nbins/256 bins, Hillis-Steele scan over the runs)
__device__ __forceinline__ void mine_scan_level(const unsigned* hist, int nbins, long need, int* bin_out, long* need_out) {
  __shared__ unsigned sh[DJ_HB];
  __shared__ long cum[256];
  __shared__ int s_bin;
  __shared__ long s_need;
  const int t = threadIdx.x;
  const int per = nbins / 256;
  for (int j = t; j < nbins; j += 256) sh[j] = hist[j];
  if (t == 0) {
    s_bin = 0;
    s_need = need;
  }
  __syncthreads();
  long local = 0;
  for (int e = 0; e < per; ++e) local += sh[nbins - 1 - (t * per + e)];
  cum[t] = local;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    long v = (t >= off) ? cum[t - off] : 0;
    __syncthreads();
    cum[t] += v;
    __syncthreads();
  }
  long before = (t > 0) ? cum[t - 1] : 0;
  if (cum[t] >= need && before < need) {
    long rem = need - before;
    for (int e = 0; e < per; ++e) {
      int idx = nbins - 1 - (t * per + e);
      long h = sh[idx];
      if (h >= rem) {
        s_bin = idx;
        s_need = rem;
        break;
      }
      rem -= h;
    }
  }
  __syncthreads();
  *bin_out = s_bin;
  *need_out = s_need;
  __syncthreads();
}

__device__ __forceinline__ MineState mine_state(const float* partial, int npartial, const unsigned* hist, int level,
                                                int ratio, int nmin) {
  double t[4];
  mine_reduce_partials(partial, npartial, t);
  MineState st;
  st.npos = t[0];
  st.spc = t[1];
  st.spl = t[2];
  long k = (long)ratio * (long)t[0];
  if (k < nmin) k = nmin;
  long nnz = (long)t[3];
  if (k > nnz) k = nnz;
  st.k = k;
  st.prefix = 0u;
  st.need = k;
  if (k > 0) {
    int b;
    if (level >= 1) {
      mine_scan_level(hist, DJ_HB, st.need, &b, &st.need);
      st.prefix = (unsigned)b << 21;
    }
    if (level >= 2) {
      mine_scan_level(hist + DJ_HB, DJ_HB, st.need, &b, &st.need);
      st.prefix |= (unsigned)b << 10;
    }
    if (level >= 3) {
      mine_scan_level(hist + 2 * DJ_HB, 1024, st.need, &b, &st.need);
      st.prefix |= (unsigned)b;
    }
  }
  return st;
}

// level 0/1/2 histogram of the elements whose higher bits match the prefix selected so far
__global__ __launch_bounds__(256) void dj_ssd_mine_hist_kernel(const float* negloss, long nbox, const float* partial,
                                                                int npartial, unsigned* hist, int level, int ratio,
                                                                int nmin) {
  __shared__ unsigned lh[DJ_HB];
  for (int j = threadIdx.x; j < DJ_HB; j += 256) lh[j] = 0u;
  MineState st = mine_state(partial, npartial, hist, level, ratio, nmin);
  if (st.k == 0) return;
  const unsigned himask = level == 0 ? 0u : (level == 1 ? 0xFFE00000u : 0xFFFFFC00u);
  const int shift = level == 0 ? 21 : (level == 1 ? 10 : 0);
  const unsigned dmask = level == 2 ? 1023u : 2047u;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nbox; i += (long)gridDim.x * 256) {
    unsigned u = __float_as_uint(negloss[i]);
    if ((u & himask) == st.prefix) atomicAdd(&lh[(u >> shift) & dmask], 1u);
  }
  __syncthreads();
  unsigned* gh = hist + level * DJ_HB;
  for (int j = threadIdx.x; j < DJ_HB; j += 256)
    if (lh[j]) atomicAdd(&gh[j], lh[j]);
}

// keep[i] = loss > T, or loss == T while tickets last; per-block sum of the kept classification losses
__global__ __launch_bounds__(256) void dj_ssd_mine_mark_kernel(const float* cls, const float* negloss, long nbox,
                                                                const float* partial, int npartial, unsigned* hist,
                                                                int ratio, int nmin, float* keep, float* keepsum) {
  __shared__ float red[256];
  MineState st = mine_state(partial, npartial, hist, 3, ratio, nmin);
  unsigned* ticket = hist + 3 * DJ_HB;
  float ks = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nbox; i += (long)gridDim.x * 256) {
    unsigned u = __float_as_uint(negloss[i]);
    bool kp = false;
    if (st.k > 0) {
      if (u > st.prefix)
        kp = true;
      else if (u == st.prefix)
        kp = (long)atomicAdd(ticket, 1u) < st.need;
    }
    keep[i] = kp ? 1.f : 0.f;
    if (kp) ks += cls[i];
  }
  red[threadIdx.x] = ks;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) keepsum[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void dj_ssd_loss_finalize_kernel(const float* partial, int npartial, const unsigned* hist,
                                                                    const float* keepsum, int nkeep, int ratio, int nmin,
                                                                    float alpha, float* out) {
  __shared__ double red[256];
  MineState st = mine_state(partial, npartial, hist, 0, ratio, nmin);
  double ks = 0.0;
  for (int b = threadIdx.x; b < nkeep; b += 256) ks += (double)keepsum[b];
  red[threadIdx.x] = ks;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double denom = st.npos > 1.0 ? st.npos : 1.0;
    double clsp = st.spc + red[0], locp = st.spl;
    out[0] = (float)((clsp + (double)alpha * locp) / denom);
    out[1] = (float)st.npos;
    out[2] = (float)st.k;
    out[3] = (float)(clsp / denom);
    out[4] = (float)(locp / denom);
  }
}

// d y_pred: classes -w*y_c/p_c [p_c > 1e-15], offsets -pos*alpha*f'(t-p), rest 0; all / max(1,n_pos) * upstream.
// One thread per ELEMENT of the (box, n_cls + 12) tensors: consecutive lanes touch consecutive floats (a thread per box
// strides by 132 B: 141 us against 30 us for the 6716-box, batch-32 head), and the rows of boxes that were neither
// matched nor mined -- 99 % of them -- are written as zeros without reading y_true / y_pred.
__global__ __launch_bounds__(256) void dj_ssd_loss_bwd_kernel(const float* y_true, const float* y_pred,
                                                               const float* pos, const float* keep, const float* out,
                                                               long nbox, int n_cls, float alpha, float upstream,
                                                               float* d_pred) {
  const int W = n_cls + 12;
  const float npos = out[1];
  const float inv = upstream / fmaxf(npos, 1.f);
  const long total = nbox * W;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long i = e / W;
    const int c = (int)(e - i * W);
    const float ps = pos[i];
    float v = 0.f;
    if (c < n_cls) {
      const float w = (ps + keep[i]) * inv;
      if (w != 0.f) {
        const float pc = y_pred[e];
        if (pc > 1e-15f) v = -w * y_true[e] / pc;
      }
    } else if (c < n_cls + 4) {
      const float wl = ps * alpha * inv;
      if (wl != 0.f) {
        const float df = y_true[e] - y_pred[e];
        const float g = (fabsf(df) < 1.f) ? df : ((df > 0.f) ? 1.f : (df < 0.f ? -1.f : 0.f));
        v = -wl * g;
      }
    }
    d_pred[e] = v;
  }
}

#define DJ_LOSS_BLOCKS 512
#define DJ_MINE_BLOCKS 256

// workspace layout (floats): cls[nbox] loc[nbox] pos[nbox] negloss[nbox] keep[nbox] partial[4*DJ_LOSS_BLOCKS]
//                            keepsum[DJ_MINE_BLOCKS] hist[3*DJ_HB + 8 (ticket)] (as 32-bit words)
extern "C" long dj_ssd_loss_workspace_floats(long nbox) {
  return 5 * nbox + 4 * DJ_LOSS_BLOCKS + DJ_MINE_BLOCKS + 3 * DJ_HB + 8 + 8;
}

extern "C" int dj_ssd_loss_fwd(const float* y_true, const float* y_pred, long nbox, int n_cls, int neg_pos_ratio,
                               int n_neg_min, float alpha, float* workspace, float* out5, void* stream) {
  DJ_CHECK_ARG(y_true && y_pred && workspace && out5 && nbox > 0 && n_cls > 1, "ssd_loss_fwd: bad arguments");
  DJ_CHECK_ARG(nbox < (1L << 31), "ssd_loss_fwd: too many boxes");
  hipStream_t s = (hipStream_t)stream;
  float* cls = workspace;
  float* loc = cls + nbox;
  float* pos = loc + nbox;
  float* negloss = pos + nbox;
  float* keep = negloss + nbox;
  float* partial = keep + nbox;
  float* keepsum = partial + 4 * DJ_LOSS_BLOCKS;
  unsigned* hist = reinterpret_cast<unsigned*>(keepsum + DJ_MINE_BLOCKS);
  int blocks = ew_blocks(nbox);
  if (blocks > DJ_LOSS_BLOCKS) blocks = DJ_LOSS_BLOCKS;
  int mblocks = ew_blocks(nbox);
  if (mblocks > DJ_MINE_BLOCKS) mblocks = DJ_MINE_BLOCKS;
  hipError_t e = hipMemsetAsync(hist, 0, (3 * DJ_HB + 8) * sizeof(unsigned), s);
  if (e != hipSuccess) {
    dj_set_error("ssd_loss_fwd: memset: %s", hipGetErrorString(e));
    return DJ_ERR_HIP;
  }
  hipLaunchKernelGGL(dj_ssd_loss_boxes_kernel, dim3(blocks), dim3(256), 0, s, y_true, y_pred, nbox, n_cls, cls, loc,
                     pos, negloss, partial);
  DJ_CHECK_LAUNCH("dj_ssd_loss_boxes");
  for (int level = 0; level < 3; ++level) {
    hipLaunchKernelGGL(dj_ssd_mine_hist_kernel, dim3(mblocks), dim3(256), 0, s, negloss, nbox, partial, blocks, hist,
                       level, neg_pos_ratio, n_neg_min);
    DJ_CHECK_LAUNCH("dj_ssd_mine_hist");
  }
  hipLaunchKernelGGL(dj_ssd_mine_mark_kernel, dim3(mblocks), dim3(256), 0, s, cls, negloss, nbox, partial, blocks, hist,
                     neg_pos_ratio, n_neg_min, keep, keepsum);
  DJ_CHECK_LAUNCH("dj_ssd_mine_mark");
  hipLaunchKernelGGL(dj_ssd_loss_finalize_kernel, dim3(1), dim3(256), 0, s, partial, blocks, hist, keepsum, mblocks,
                     neg_pos_ratio, n_neg_min, alpha, out5);
  DJ_CHECK_LAUNCH("dj_ssd_loss_finalize");
  return DJ_OK;
}

extern "C" int dj_ssd_loss_bwd(const float* y_true, const float* y_pred, long nbox, int n_cls, float alpha,
                               float upstream, const float* workspace, const float* out5, float* d_pred,
                               void* stream) {
  DJ_CHECK_ARG(y_true && y_pred && workspace && out5 && d_pred && nbox > 0 && n_cls > 1, "ssd_loss_bwd: bad arguments");
  const float* pos = workspace + 2 * nbox;
  const float* keep = workspace + 4 * nbox;
  hipLaunchKernelGGL(dj_ssd_loss_bwd_kernel, dim3(ew_blocks(nbox * (n_cls + 12))), dim3(256), 0, (hipStream_t)stream, y_true, y_pred,
                     pos, keep, out5, nbox, n_cls, alpha, upstream, d_pred);
  DJ_CHECK_LAUNCH("dj_ssd_loss_bwd");
  return DJ_OK;
}

// ---------------------------------------------------------------------------------
// categorical cross-entropy on probabilities (Keras 2.2.4, TF backend): one wave per sample
//   loss_i = -sum_c y_c log(clip(p_c / sum p, 1e-7, 1-1e-7)); out[0] = mean_i loss_i
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dj_cce_kernel(const float* y_true, const float* p, long rows, int C,
                                                      float upstream_over_rows, float* loss_rows, float* dp) {
  long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* pr = p + row * C;
  const float* tr = y_true + row * C;
  float S = 0.f;
  for (int c = lane; c < C; c += 64) S += pr[c];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) S += __shfl_xor(S, o);
  float l = 0.f, gp = 0.f;  // gp = sum_c g_c p_c with g = dL/dp'
  for (int c = lane; c < C; c += 64) {
    float q = pr[c] / S;
    float qc = fminf(fmaxf(q, 1e-7f), 1.f - 1e-7f);
    float yc = tr[c];
    if (yc != 0.f) {
      l -= yc * logf(qc);
      if (q > 1e-7f && q < 1.f - 1e-7f) gp += (-yc / qc) * pr[c];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    l += __shfl_xor(l, o);
    gp += __shfl_xor(gp, o);
  }
  if (lane == 0) loss_rows[row] = l;
  if (dp) {
    float* dr = dp + row * C;
    for (int c = lane; c < C; c += 64) {
      float q = pr[c] / S;
      float qc = fminf(fmaxf(q, 1e-7f), 1.f - 1e-7f);
      float g = (tr[c] != 0.f && q > 1e-7f && q < 1.f - 1e-7f) ? -tr[c] / qc : 0.f;
      dr[c] = (g / S - gp / (S * S)) * upstream_over_rows;
    }
  }
}

__global__ void dj_mean_kernel(const float* v, long n, float* out) {
  __shared__ double red[256];
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) s += (double)v[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(red[0] / (double)n);
}

extern "C" int dj_categorical_crossentropy(const float* y_true, const float* probs, long rows, int C, float upstream,
                                           float* loss_rows, float* d_probs, float* out_mean, void* stream) {
  DJ_CHECK_ARG(y_true && probs && loss_rows && out_mean && rows > 0 && C > 0, "cce: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(dj_cce_kernel, dim3((unsigned)dj_cdiv(rows, 4)), dim3(256), 0, s, y_true, probs, rows, C,
                     upstream / (float)rows, loss_rows, d_probs);
  DJ_CHECK_LAUNCH("dj_cce");
  hipLaunchKernelGGL(dj_mean_kernel, dim3(1), dim3(256), 0, s, loss_rows, rows, out_mean);
  DJ_CHECK_LAUNCH("dj_mean");
  return DJ_OK;
}

// mean over H*W of an NHWC tensor (GlobalAveragePooling2D) and its gradient
__global__ __launch_bounds__(256) void dj_gap_fwd_kernel(const float* x, float* y, int B, int HW, int C) {
  long total = (long)B * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    int c = (int)(i % C);
    long b = i / C;
    float s = 0.f;
    for (int q = 0; q < HW; ++q) s += x[(b * HW + q) * C + c];
    y[i] = s / (float)HW;
  }
}
__global__ __launch_bounds__(256) void dj_gap_bwd_kernel(const float* dy, float* dx, int B, int HW, int C, int beta) {
  long total = (long)B * HW * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    int c = (int)(i % C);
    long b = i / ((long)HW * C);
    float v = dy[b * C + c] / (float)HW;
    dx[i] = beta ? dx[i] + v : v;
  }
}
extern "C" int dj_global_avg_pool_fwd(const float* x, float* y, int B, int HW, int C, void* stream) {
  DJ_CHECK_ARG(x && y && B > 0 && HW > 0 && C > 0, "gap fwd: bad arguments");
  hipLaunchKernelGGL(dj_gap_fwd_kernel, dim3(ew_blocks((long)B * C)), dim3(256), 0, (hipStream_t)stream, x, y, B, HW, C);
  DJ_CHECK_LAUNCH("dj_global_avg_pool_fwd");
  return DJ_OK;
}
extern "C" int dj_global_avg_pool_bwd(const float* dy, float* dx, int B, int HW, int C, int beta, void* stream) {
  DJ_CHECK_ARG(dy && dx && B > 0 && HW > 0 && C > 0, "gap bwd: bad arguments");
  hipLaunchKernelGGL(dj_gap_bwd_kernel, dim3(ew_blocks((long)B * HW * C)), dim3(256), 0, (hipStream_t)stream, dy, dx, B,
                     HW, C, beta);
  DJ_CHECK_LAUNCH("dj_global_avg_pool_bwd");
  return DJ_OK;
}
