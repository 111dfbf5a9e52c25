// Host launchers of the implicit-GEMM convolution (see dj_igemm.h for the kernel).
#include "../../include/dj_hip.h"
#include "dj_conv_launch.h"
#include <string.h>
#include <map>
#include <mutex>
#include <atomic>
#include <array>
#include <algorithm>

static thread_local char g_err[512] = "";
void dj_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* dj_last_error(void) { return g_err; }
extern "C" int dj_abi_version(void) { return DJ_ABI_VERSION; }

// ---- the library's only mutable state: three settings, each safe to touch from any thread ----
// test switch: atomic, read once per launch
std::atomic<bool> g_dj_allow_fast{true};
extern "C" void dj_set_fast_path(int enable) { g_dj_allow_fast.store(enable != 0, std::memory_order_relaxed); }
std::atomic<bool> g_dj_gather_variants{true};
extern "C" void dj_set_gather_variants(int enable) { g_dj_gather_variants.store(enable != 0, std::memory_order_relaxed); }

// Arithmetic mode.  0: fp32 MFMA everywhere (default).  1: forward GEMMs round their operands to fp16, gradient GEMMs
// (dgrad, wgrad) to bf16 (gradients need the exponent range); 2: bf16 everywhere; 3 ("float32x3"): fp32 tensors, every
// product as three bf16 MFMAs on hi / lo split operands (~2^-17 relative per product); 4 ("float32x6"): six MFMAs on
// hi / mid / lo pieces (2^-24: fp32 results).  Mode 0 takes, per geometry, the fp32 MFMA kernel or the mode-4 kernel its
// tuning entry names (both fp32 results); 5: fp32 MFMA kernels only.  fp32 accumulation in all modes.
// A process-wide default (atomic) that a thread can override for its own launches: a plan lowered under one
// mode keeps running in it whatever other models or threads of the process select (engine.Plan sets the override before
// it launches).
static std::atomic<int> g_default_compute_mode{0};
static thread_local int tl_compute_mode = -1;
int dj_compute_mode() { return tl_compute_mode >= 0 ? tl_compute_mode : g_default_compute_mode.load(std::memory_order_relaxed); }
extern "C" int dj_set_compute_mode(int mode) {
  int prev = g_default_compute_mode.load(std::memory_order_relaxed);
  if (mode >= 0 && mode <= 5) g_default_compute_mode.store(mode, std::memory_order_relaxed);
  return prev;
}
extern "C" int dj_set_thread_compute_mode(int mode) {
  int prev = tl_compute_mode;
  if (mode >= -1 && mode <= 5) tl_compute_mode = mode;
  return prev;
}
extern "C" int dj_get_compute_mode(void) { return dj_compute_mode(); }

// instantiated in dj_conv_i00.hip (fwd), dj_conv_i01.hip (strided 1x1 dgrad as GEMM), dj_conv_i11.hip (dgrad),
// dj_conv_i20.hip (wgrad)
extern template int dj_launch_cfg<0, 0>(int, const DjIgemmParams&, int, hipStream_t);
extern template int dj_launch_cfg<0, 1>(int, const DjIgemmParams&, int, hipStream_t);
extern template int dj_launch_cfg<1, 1>(int, const DjIgemmParams&, int, hipStream_t);
extern template int dj_launch_cfg<2, 0>(int, const DjIgemmParams&, int, hipStream_t);

// Pick a tile shape: smallest padded-N waste first, then enough workgroups to fill
// 256 CUs (2 resident workgroups each for the large tiles).
static int choose_cfg(long M, long N, long K, bool allow_split, int* splits_out) {
  int bn;
  if (N > 96) {
    // 128 vs 64: both pad N to the same multiple of 64 or better with 64
    long pad128 = (long)dj_cdiv(N, 128) * 128, pad64 = (long)dj_cdiv(N, 64) * 64;
    bn = (pad64 < pad128) ? 64 : 128;
  } else if (N > 32 && (long)dj_cdiv(N, 64) * 64 <= (long)dj_cdiv(N, 32) * 32) {
    bn = 64;
  } else {
    bn = 32;
  }
  int cfg;
  auto tiles = [&](int bm, int b_n) { return (long)dj_cdiv(M, bm) * dj_cdiv(N, b_n); };
  if (bn == 128) {
    if (tiles(128, 128) >= 384)
      cfg = CFG_128x128;
    else if (tiles(128, 64) >= 256)
      cfg = CFG_128x64;
    else
      cfg = CFG_64x64;
  } else if (bn == 64) {
    cfg = (tiles(128, 64) >= 384) ? CFG_128x64 : CFG_64x64;
  } else {
    cfg = CFG_128x32;
  }
  int splits = 1;
  if (allow_split) {
    long t = tiles(kCfgs[cfg].bm, kCfgs[cfg].bn);
    if (t < 256) {
      long want = (512 + t - 1) / t;
      long maxs = K / 256;  // keep >= 8 K-steps per split
      if (maxs < 1) maxs = 1;
      splits = (int)(want < maxs ? want : maxs);
      if (splits < 1) splits = 1;
    }
  }
  *splits_out = splits;
  return cfg;
}


// ---------------------------------------------------------------------------------
// Per-geometry launch overrides (tile configuration, split-K factor) recorded by the plan-time
// autotuner (engine.Plan.autotune): key = direction (+4 when BN statistics are taken) + geometry.
// ---------------------------------------------------------------------------------
typedef std::array<int, 16> TuneKey;
static std::map<TuneKey, std::pair<int, int>> g_tune;
static std::mutex g_tune_mu;

// (the arithmetic mode of the calling thread is part of the key: the fp32 and the reduced-precision kernels have tables
// of their own, and two models of different modes in one process do not overwrite each other's choices)
static TuneKey tune_key(int dir, const dj_conv2d_desc* d) {
  return TuneKey{dir | (dj_compute_mode() << 4), d->batch, d->in_h, d->in_w, d->in_c, d->out_h, d->out_w, d->out_c, d->kernel_h, d->kernel_w,
                 d->stride_h, d->stride_w, d->dilation_h, d->dilation_w, d->pad_top, d->pad_left};
}

static bool tune_lookup(int dir, const dj_conv2d_desc* d, int* cfg, int* splits) {
  std::lock_guard<std::mutex> g(g_tune_mu);
  auto it = g_tune.find(tune_key(dir, d));
  if (it == g_tune.end()) return false;
  *cfg = it->second.first;
  *splits = it->second.second;
  return true;
}

// mode 0: [0, N_CFG) fp32 MFMA variants, [N_CFG, 2 N_CFG) the split-bf16 (float32x6) variants of the same indices
extern "C" int dj_conv2d_tune_configs(void) { return dj_compute_mode() == 0 ? 2 * N_CFG : N_CFG; }

// dir: 0 fwd, 1 dgrad, 2 wgrad, +4 when the forward takes BN statistics, 9 = input gradient that takes the
// BatchNormalization backward statistics (dj_conv_dgrad_args.partial).  cfg < 0 removes the override.
extern "C" int dj_conv2d_tune_set(int dir, const dj_conv2d_desc* d, int cfg, int splits) {
  DJ_CHECK_ARG(d != nullptr && cfg < (dj_compute_mode() == 0 ? 2 * N_CFG : N_CFG) && splits >= 1, "tune_set: bad arguments");
  std::lock_guard<std::mutex> g(g_tune_mu);
  if (cfg < 0)
    g_tune.erase(tune_key(dir, d));
  else
    g_tune[tune_key(dir, d)] = std::make_pair(cfg, splits);
  return DJ_OK;
}

// Default choice the launcher would make (for the tuner to seed its candidate list): writes cfg and splits.
extern "C" int dj_conv2d_default_config(int dir, const dj_conv2d_desc* d, int* cfg, int* splits);

static inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
// a thread's 4-element piece: 16 bytes of a fp32 tensor, 8 bytes of a 16-bit one
static inline bool aligned_dt(const void* p, int dt) { return (((uintptr_t)p) & (dt == 0 ? 15 : 7)) == 0; }

static int check_desc(const dj_conv2d_desc* d) {
  DJ_CHECK_ARG(d != nullptr, "conv desc is null");
  DJ_CHECK_ARG(d->batch > 0 && d->in_h > 0 && d->in_w > 0 && d->in_c > 0 && d->out_h > 0 && d->out_w > 0 &&
                   d->out_c > 0,
               "conv desc: non-positive dimension");
  DJ_CHECK_ARG(d->kernel_h > 0 && d->kernel_w > 0 && d->stride_h > 0 && d->stride_w > 0 && d->dilation_h > 0 &&
                   d->dilation_w > 0,
               "conv desc: non-positive kernel/stride/dilation");
  DJ_CHECK_ARG(d->pad_top >= 0 && d->pad_left >= 0, "conv desc: negative padding");
  DJ_CHECK_ARG(d->ld_x >= d->in_c && d->ld_y >= d->out_c, "conv desc: ld_x/ld_y smaller than channel count");
  // every output pixel must read inside [-pad, in + pad_after): guaranteed if the last tap start is valid
  long last_h = (long)(d->out_h - 1) * d->stride_h - d->pad_top;
  long last_w = (long)(d->out_w - 1) * d->stride_w - d->pad_left;
  DJ_CHECK_ARG(last_h < d->in_h && last_w < d->in_w, "conv desc: output grid larger than the input allows");
  DJ_CHECK_ARG((long)d->batch * d->in_h * d->in_w * (long)d->ld_x < (1L << 31) &&
                   (long)d->batch * d->out_h * d->out_w * (long)d->ld_y < (1L << 31),
               "conv desc: tensor exceeds 2^31 elements");
  return DJ_OK;
}

__global__ void dj_relu_rows_kernel(float* y, long rows, int cols, int ld) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = rows * cols;
  for (; i < total; i += (long)gridDim.x * blockDim.x) {
    long r = i / cols;
    int c = (int)(i - r * cols);
    float* p = y + r * ld + c;
    *p = fmaxf(*p, 0.f);
  }
}

static int extent_bytes(long pixels, long ld, long c, int es = 4) {
  long b = ((pixels - 1) * ld + c) * es;
  return (b > 0 && b < 0x7FFFFFF0L) ? (int)b : 0;
}

// storage types of the tensors of a launch (DJ_F32 / DJ_F16 / DJ_BF16)
static inline int dt_size(int dt) { return dt == DJ_F32 ? 4 : 2; }
static inline bool dt_ok(int dt) { return dt == DJ_F32 || dt == DJ_F16 || dt == DJ_BF16; }

// reciprocals of the row grid (p.rowH, p.rowW must be set): the kernels decompose a GEMM row into (image, h, w) with a
// float multiply and a one-step correction instead of integer divisions
static void set_row_recip(DjIgemmParams& p) {
  p.inv_rowHW = 1.0f / (float)(p.rowH * p.rowW);
  p.inv_rowW = 1.0f / (float)p.rowW;
}

static void fill_geom(DjIgemmParams& p, const dj_conv2d_desc* d) {
  p.KH = d->kernel_h;
  p.KW = d->kernel_w;
  p.sH = d->stride_h;
  p.sW = d->stride_w;
  p.dH = d->dilation_h;
  p.dW = d->dilation_w;
  p.pT = d->pad_top;
  p.pL = d->pad_left;
  set_row_recip(p);
}

extern "C" int dj_conv2d_fwd_stats_rows(const dj_conv2d_desc* d) {
  if (check_desc(d) != DJ_OK) return DJ_ERR_ARG;
  // one partial row per 64 output pixels, independent of the tile configuration the launcher picks
  return dj_cdiv((long)d->batch * d->out_h * d->out_w, 64);
}

// Second half of a split-K forward convolution without atomics: the K chunks left their partial tiles in `nsplit` slabs
// [rows][N]; this pass adds them IN A FIXED ORDER (bit-reproducible, unlike fp32 atomics in arrival order), takes the
// BatchNormalization column statistics of the sum (per 64 rows: [ceil(rows/64)][2][N], before the bias, as the GEMM
// epilogue does), then adds bias / applies ReLU and writes y.  One workgroup per 64 rows x (16 * VEC) columns.
template <int VEC>
__global__ __launch_bounds__(256) void dj_splitk_reduce_kernel(const float* slabs, int nsplit, long slab_stride, long rows,
                                                               int N, const float* bias, int relu, float* y, int ld_y,
                                                               float* stats) {
  // 16 column chunks (16 * VEC columns) x 16 row lanes; a thread owns rows ty, ty + 16, ty + 32, ty + 48 of the group
  __shared__ float red[16][16][2 * VEC];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int c = (blockIdx.y * 16 + tx) * VEC;
  const long r0 = (long)blockIdx.x * 64;
  float s[VEC], q[VEC], b[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    s[v] = 0.f;
    q[v] = 0.f;
    b[v] = (bias && c + v < N) ? bias[c + v] : 0.f;
  }
  if (c < N) {
    float a[4][VEC];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int v = 0; v < VEC; ++v) a[j][v] = 0.f;
    for (int k = 0; k < nsplit; ++k) {      // slabs in index order: the sum does not depend on who finished first
      const float* slab = slabs + (long)k * slab_stride + c;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long r = r0 + ty + 16 * j;
        if (r < rows) {
          if (VEC == 4) {
            f32x4 t = *reinterpret_cast<const f32x4*>(slab + r * N);
            a[j][0] += t.x;
            a[j][1 % VEC] += t.y;
            a[j][2 % VEC] += t.z;
            a[j][3 % VEC] += t.w;
          } else {
            a[j][0] += slab[r * N];
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long r = r0 + ty + 16 * j;
      if (r >= rows) continue;
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        s[v] += a[j][v];
        q[v] += a[j][v] * a[j][v];
        float o = a[j][v] + b[v];
        a[j][v] = relu ? fmaxf(o, 0.f) : o;
      }
      float* dst = y + r * ld_y + c;
      if (VEC == 4) *reinterpret_cast<f32x4*>(dst) = f32x4{a[j][0], a[j][1 % VEC], a[j][2 % VEC], a[j][3 % VEC]};
      else dst[0] = a[j][0];
    }
  }
  if (!stats) return;
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    red[ty][tx][v] = s[v];
    red[ty][tx][VEC + v] = q[v];
  }
  __syncthreads();
  if (ty == 0 && c < N) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      float ss = 0.f, qq = 0.f;
      for (int l = 0; l < 16; ++l) {     // fixed order over the row lanes
        ss += red[l][tx][v];
        qq += red[l][tx][VEC + v];
      }
      stats[((long)blockIdx.x * 2 + 0) * N + c + v] = ss;
      stats[((long)blockIdx.x * 2 + 1) * N + c + v] = qq;
    }
  }
}

static int launch_splitk_reduce(const float* slabs, int nsplit, long slab_stride, long rows, int N, const float* bias,
                                int relu, float* y, int ld_y, float* stats, hipStream_t s) {
  const bool v4 = (N % 4 == 0) && (ld_y % 4 == 0) && aligned16(slabs) && aligned16(y) && (slab_stride % 4 == 0);
  const int cols_per_block = v4 ? 64 : 16;
  dim3 grid((unsigned)((rows + 63) / 64), (unsigned)((N + cols_per_block - 1) / cols_per_block));
  if (v4)
    hipLaunchKernelGGL(dj_splitk_reduce_kernel<4>, grid, dim3(256), 0, s, slabs, nsplit, slab_stride, rows, N, bias, relu, y,
                       ld_y, stats);
  else
    hipLaunchKernelGGL(dj_splitk_reduce_kernel<1>, grid, dim3(256), 0, s, slabs, nsplit, slab_stride, rows, N, bias, relu, y,
                       ld_y, stats);
  DJ_CHECK_LAUNCH("dj_splitk_reduce_kernel");
  return DJ_OK;
}

// *kchunk = the K range of one split, a multiple of DJ_BK; -> the number of splits that are not empty
static int split_k(int K, int splits, int* kchunk) {
  *kchunk = dj_cdiv(dj_cdiv(K, splits), DJ_BK) * DJ_BK;
  return dj_cdiv(K, *kchunk);
}

// the memsets in front of a launch that accumulates with atomics (or scatters)
static int memset_status(hipError_t e, const char* what) {
  if (e == hipSuccess) return DJ_OK;
  dj_set_error("%s: memset: %s", what, hipGetErrorString(e));
  return DJ_ERR_HIP;
}
static int clear_rows(void* t, long rows, int cols, int ld, int es, hipStream_t s, const char* what) {
  return memset_status(hipMemset2DAsync(t, (size_t)ld * es, 0, (size_t)cols * es, (size_t)rows, s), what);
}

extern "C" int dj_conv2d_fwd_addrelu_supported(const dj_conv2d_desc* d) {
  if (check_desc(d)) return 0;
  return d->kernel_h == 1 && d->kernel_w == 1 && d->stride_h == 1 && d->stride_w == 1 && d->pad_top == 0 &&
         d->pad_left == 0 && d->in_h == d->out_h && d->in_w == d->out_w && d->in_c % 32 == 0 && d->ld_x % 4 == 0 &&
         d->out_c % 4 == 0;
}

extern "C" int dj_conv2d_nhwc_fwd(const dj_conv2d_desc* d, const dj_conv_fwd_args* args, void* stream) {
  DJ_CHECK_ARG(args != nullptr, "conv fwd: null argument struct");
  const dj_conv_fwd_args& a = *args;
  DJ_CHECK_ARG(dt_ok(a.dt_x) && dt_ok(a.dt_w) && dt_ok(a.dt_y) && dt_ok(a.dt_sum), "conv fwd: unknown storage type");
  DJ_CHECK_ARG(a.workspace_floats >= 0 && (a.workspace != nullptr || a.workspace_floats == 0), "conv fwd: bad workspace");
  DJ_CHECK_ARG(a.res || !a.sum_out, "conv fwd: sum_out without res");
  if (a.res) {
    DJ_CHECK_ARG(d && dj_conv2d_fwd_addrelu_supported(d), "conv fwd (residual add): needs a 1x1 stride-1 unpadded conv with "
                                                           "in_c %% 32 == 0");
    DJ_CHECK_ARG(a.pro_scale && a.pro_shift, "conv fwd (residual add): pro_scale and pro_shift are required");
    DJ_CHECK_ARG((a.res_scale == nullptr) == (a.res_shift == nullptr), "conv fwd (residual add): res_scale/res_shift come together");
    DJ_CHECK_ARG(a.ld_res >= d->in_c && a.ld_res % 4 == 0 && (!a.sum_out || (a.ld_sum >= d->in_c && a.ld_sum % 4 == 0)),
                 "conv fwd (residual add): bad ld_res / ld_sum");
    DJ_CHECK_ARG(aligned16(a.res) && aligned16(a.sum_out) && aligned16(a.res_scale) && aligned16(a.res_shift),
                 "conv fwd (residual add): tensors must be 16-byte aligned");
  }
  if (int rc = check_desc(d)) return rc;
  DJ_CHECK_ARG(a.x && a.w && a.y, "conv fwd: null tensor");
  const int dt_sum = a.sum_out ? a.dt_sum : DJ_F32;
  const bool io16 = a.dt_x != DJ_F32 || a.dt_y != DJ_F32 || dt_sum != DJ_F32 || a.dt_w != DJ_F32;
  DJ_CHECK_ARG((a.dt_x == DJ_F32 || a.dt_x == DJ_F16) && (a.dt_y == DJ_F32 || a.dt_y == DJ_F16) &&
                   (dt_sum == DJ_F32 || dt_sum == DJ_F16) && (a.dt_w == DJ_F32 || a.dt_w == DJ_F16),
               "conv fwd: activations and the weight shadow are held as fp32 or fp16");
  DJ_CHECK_ARG(!io16 || dj_compute_mode() == 1, "conv fwd: 16-bit tensors need arithmetic mode 1 (float16)");
  DJ_CHECK_ARG((a.pro_scale == nullptr) == (a.pro_shift == nullptr), "conv fwd: pro_scale/pro_shift must come together");
  hipStream_t s = (hipStream_t)stream;
  float* const y = (float*)a.y;
  float* const ws = a.workspace;
  DjIgemmParams p;
  memset(&p, 0, sizeof(p));
  p.A = (const float*)a.x;
  p.B = (const float*)a.w;
  p.C = y;
  p.bias = a.bias;
  p.pro_scale = a.pro_scale;
  p.pro_shift = a.pro_shift;
  p.pro_relu = a.res ? 1 : a.pro_relu;
  p.stats = a.stats;
  p.M = d->batch * d->out_h * d->out_w;
  p.N = d->out_c;
  p.K = d->kernel_h * d->kernel_w * d->in_c;
  p.rowH = d->out_h;
  p.rowW = d->out_w;
  p.srcH = d->in_h;
  p.srcW = d->in_w;
  p.srcC = d->in_c;
  p.ldsrc = d->ld_x;
  fill_geom(p, d);
  p.ldb = d->out_c;
  p.ldc = d->ld_y;
  p.cmap = 0;
  const bool y_zeroed = (a.flags & DJ_CONV_Y_ZEROED) != 0;
  const bool stats_may_split = (a.flags & DJ_CONV_STATS_MAY_SPLIT) != 0 && a.stats != nullptr && ws != nullptr;
  const int relu = a.flags & DJ_CONV_RELU;
  p.relu = relu;
  p.vecA = (d->in_c % 4 == 0) && (d->ld_x % 4 == 0) && aligned_dt(a.x, a.dt_x) &&
           (!a.pro_scale || (aligned16(a.pro_scale) && aligned16(a.pro_shift)));
  p.vecB = (d->out_c % 4 == 0) && aligned_dt(a.w, a.dt_w);
  p.a_bytes = extent_bytes((long)d->batch * d->in_h * d->in_w, d->ld_x, d->in_c, dt_size(a.dt_x));
  p.a_dt = a.dt_x;
  p.c_dt = a.dt_y;
  p.sum_dt = dt_sum;
  if (a.res) {
    p.A2 = (const float*)a.res;
    p.ldsrc2 = a.ld_res;
    p.pro_scale2 = a.res_scale;
    p.pro_shift2 = a.res_shift;
    p.sum_out = (float*)a.sum_out;
    p.ld_sum = a.ld_sum;
    p.a2_bytes = extent_bytes((long)d->batch * d->in_h * d->in_w, a.ld_res, d->in_c, dt_size(a.dt_x));
    p.sum_bytes = a.sum_out ? extent_bytes((long)d->batch * d->in_h * d->in_w, a.ld_sum, d->in_c, dt_size(dt_sum)) : 0;
  }
  p.b_bytes = extent_bytes((long)p.K, d->out_c, d->out_c, dt_size(a.dt_w));
  p.b_dt = a.dt_w;
  // (refusals come before the first write: a split launch clears y below)
  if (a.res) {
    DJ_CHECK_ARG(dj_fast_mode_fwd(p) == 3, "conv fwd (residual add): the branch-free kernel's preconditions do not hold "
                                           "(channels %% 32, 16-byte aligned tensors)");
  }
  DJ_CHECK_ARG(!io16 || dj_fast_mode_fwd(p) != 0, "conv fwd: 16-bit tensors need the branch-free kernel's preconditions "
                                                  "(in_c %% 32 == 0, out_c %% 4 == 0, 16-byte aligned tensors)");
  // statistics come out of the GEMM epilogue (one K range per tile) -- or, for a caller that allows it and supplies a
  // workspace, out of the slab reduction of a split launch (tuned like a launch without statistics)
  const bool wants_stats = a.stats != nullptr && !stats_may_split;
  int splits = 1;
  int cfg = choose_cfg(p.M, p.N, p.K, !wants_stats, &splits);
  tune_lookup(wants_stats ? 4 : 0, d, &cfg, &splits);
  if (wants_stats) splits = 1;
  if (a.dt_y != DJ_F32) splits = 1;   // a 16-bit result is written by one K range (no slabs, no atomics)
  splits = split_k(p.K, splits, &p.kchunk);
  // split-K through slabs in the caller's workspace + a fixed-order reduction (deterministic), when they fit
  bool slabs = splits > 1 && ws != nullptr && (long)splits * p.M * p.N <= a.workspace_floats && aligned16(ws);
  if (splits > 1 && !slabs && stats_may_split)   // statistics cannot come from atomics: one K range after all
    splits = split_k(p.K, 1, &p.kchunk);
  if (slabs) {
    p.C = ws;
    p.ldc = p.N;
    p.slab_stride = (long)p.M * p.N;
    p.bias = nullptr;
    p.relu = 0;
    p.stats = nullptr;
  } else if (splits > 1) {
    p.atomic = 1;
    p.relu = 0;
    if (!y_zeroed)
      if (int rc = clear_rows(y, p.M, d->out_c, d->ld_y, 4, s, "conv fwd")) return rc;
  }
  if (int rc = dj_launch_cfg<0, 0>(cfg, p, splits, s)) return rc;
  if (slabs) return launch_splitk_reduce(ws, splits, p.slab_stride, p.M, p.N, a.bias, relu, y, d->ld_y, a.stats, s);
  if (splits > 1 && relu) {
    long total = (long)p.M * p.N;
    int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(dj_relu_rows_kernel, dim3(blocks), dim3(256), 0, s, y, (long)p.M, p.N, d->ld_y);
    DJ_CHECK_LAUNCH("dj_relu_rows_kernel");
  }
  return DJ_OK;
}

// Floats of workspace with which dj_conv2d_nhwc_fwd runs this geometry without atomics under the CURRENT tuning
// choice (0: the launch is not split).  may_split_stats: as the flag of the same name.
extern "C" long dj_conv2d_fwd_workspace_floats(const dj_conv2d_desc* d, int may_split_stats) {
  if (check_desc(d)) return -1;
  const int M = d->batch * d->out_h * d->out_w, N = d->out_c, K = d->kernel_h * d->kernel_w * d->in_c;
  int splits = 1, kchunk;
  int cfg = choose_cfg(M, N, K, true, &splits);
  tune_lookup(0, d, &cfg, &splits);
  (void)may_split_stats;
  splits = split_k(K, splits, &kchunk);
  return splits > 1 ? (long)splits * M * N : 0;
}

static inline bool dgrad_is_strided_1x1(const dj_conv2d_desc* d) {
  return d->kernel_h == 1 && d->kernel_w == 1 && d->pad_top == 0 && d->pad_left == 0 && (d->stride_h > 1 || d->stride_w > 1) &&
         d->stride_h == d->stride_w;
}

extern "C" int dj_conv2d_nhwc_dgrad(const dj_conv2d_desc* d, const dj_conv_dgrad_args* args, void* stream) {
  DJ_CHECK_ARG(args != nullptr, "conv dgrad: null argument struct");
  const dj_conv_dgrad_args& a = *args;
  DJ_CHECK_ARG(dt_ok(a.dt_dy) && dt_ok(a.dt_w) && dt_ok(a.dt_dx) && dt_ok(a.dt_z), "conv dgrad: unknown storage type");
  // the BatchNormalization backward statistics are asked for by `partial`; z alone is no plain input gradient either
  const bool bnb = a.partial != nullptr || a.z != nullptr;
  if (bnb) {
    DJ_CHECK_ARG(a.z && a.mean && a.invstd && a.partial, "conv dgrad + BN backward statistics: null tensor");
    DJ_CHECK_ARG((a.scale == nullptr) == (a.shift == nullptr), "conv dgrad + BN backward statistics: scale/shift must come together");
    // one K range per tile, no accumulation: the accumulator of a tile IS the gradient the statistics are taken of
    DJ_CHECK_ARG(d && a.ld_z >= d->in_c && !a.bias && !(a.flags & 1), "conv dgrad + BN backward statistics: ld_z < in_c, or a bias / "
                                                                      "an accumulating launch");
  }
  if (a.mask_x) {
    DJ_CHECK_ARG(d && a.ld_mask >= d->in_c, "conv dgrad + ReLU mask: ld_mask < in_c");
    DJ_CHECK_ARG((long)d->batch * d->in_h * d->in_w * (long)a.ld_mask < (1L << 31), "conv dgrad + ReLU mask: mask exceeds 2^31 elements");
  }
  if (int rc = check_desc(d)) return rc;
  DJ_CHECK_ARG(a.dy && a.w && a.dx, "conv dgrad: null tensor");
  const int dt_z = bnb ? a.dt_z : DJ_F32;
  const bool io16 = a.dt_dy != DJ_F32 || a.dt_dx != DJ_F32 || a.dt_w != DJ_F32 || dt_z != DJ_F32;
  DJ_CHECK_ARG((a.dt_dy == DJ_F32 || a.dt_dy == DJ_BF16) && (a.dt_w == DJ_F32 || a.dt_w == DJ_BF16) &&
                   (dt_z == DJ_F32 || dt_z == DJ_F16),
               "conv dgrad: gradients and the weight shadow are held as fp32 or bf16, the BatchNormalization input as fp32 or fp16");
  DJ_CHECK_ARG(!io16 || dj_compute_mode() == 1, "conv dgrad: 16-bit tensors need arithmetic mode 1 (float16)");
  const bool one_k_range = bnb || (a.flags & DJ_DGRAD_NO_SPLIT) != 0;   // no split-K: no arrival-order arithmetic
  const int beta = a.flags & 1;
  hipStream_t s = (hipStream_t)stream;
  DjIgemmParams p;
  memset(&p, 0, sizeof(p));
  if (bnb) {
    p.bnb_z = (const float*)a.z;
    p.bnb_ldz = a.ld_z;
    p.bnb_zbytes = extent_bytes((long)d->batch * d->in_h * d->in_w, a.ld_z, d->in_c, dt_size(dt_z));
    p.bnb_zdt = dt_z;
    DJ_CHECK_ARG(p.bnb_zbytes > 0, "conv dgrad + BN backward statistics: z of 2 GiB or more");
    p.bnb_mean = a.mean;
    p.bnb_invstd = a.invstd;
    p.bnb_scale = a.scale;
    p.bnb_shift = a.shift;
    p.stats = a.partial;
  }
  p.A = (const float*)a.dy;
  p.B = (const float*)a.w;
  p.C = (float*)a.dx;
  p.bias = a.bias;
  p.N = d->in_c;
  p.srcC = d->out_c;
  p.ldsrc = d->ld_y;
  p.ldb = d->out_c;
  p.bTapStride = (long)d->in_c * d->out_c;
  p.ldc = d->ld_x;
  p.beta = beta;
  p.vecA = (d->out_c % 4 == 0) && (d->ld_y % 4 == 0) && aligned_dt(a.dy, a.dt_dy);
  p.vecB = (d->out_c % 4 == 0) && aligned_dt(a.w, a.dt_w);
  p.a_bytes = extent_bytes((long)d->batch * d->out_h * d->out_w, d->ld_y, d->out_c, dt_size(a.dt_dy));
  p.b_bytes = extent_bytes((long)d->kernel_h * d->kernel_w * d->in_c, d->out_c, d->out_c, dt_size(a.dt_w));
  p.b_dt = a.dt_w;
  p.a_dt = a.dt_dy;
  p.c_dt = a.dt_dx;
  const long in_pixels = (long)d->batch * d->in_h * d->in_w;
  bool strided_1x1 = dgrad_is_strided_1x1(d) && a.bias == nullptr;
  int splits = 1;
  DJ_CHECK_ARG(!(bnb && strided_1x1), "conv dgrad + BN backward statistics: not for strided 1x1 convolutions");
  if (a.mask_x) {
    DJ_CHECK_ARG(!bnb && !io16, "conv dgrad + ReLU mask: fp32 tensors, no BN backward statistics");
    DJ_CHECK_ARG(!dgrad_is_strided_1x1(d), "conv dgrad + ReLU mask: not for strided 1x1 convolutions (their dx is scattered)");
    const int mode = dj_compute_mode();
    DJ_CHECK_ARG(mode != 1 && mode != 2, "conv dgrad + ReLU mask: not in the 16-bit arithmetic modes");
    p.mask_x = a.mask_x;
    p.ld_mask = a.ld_mask;
  }
  if (strided_1x1) {
    // compact GEMM over the output grid, rows scattered to the strided input pixels
    p.M = d->batch * d->out_h * d->out_w;
    p.K = d->out_c;
    p.rowH = d->out_h;
    p.rowW = d->out_w;
    p.srcH = d->out_h;
    p.srcW = d->out_w;
    p.KH = p.KW = 1;
    p.sH = p.sW = p.dH = p.dW = 1;
    p.pT = p.pL = 0;
    set_row_recip(p);
    p.cmap = 1;
    p.cgH = d->out_h;
    p.cgW = d->out_w;
    p.cH = d->in_h;
    p.cW = d->in_w;
    p.cS = d->stride_h;
    // (refused before dx is cleared)
    DJ_CHECK_ARG(!io16 || (fast_mode<0, 1>(p)) != 0, "conv dgrad (strided 1x1): 16-bit tensors need the branch-free kernel's "
                                                   "preconditions (channels %% 32, 16-byte aligned tensors)");
    if (!beta)
      if (int rc = clear_rows(a.dx, in_pixels, d->in_c, d->ld_x, dt_size(a.dt_dx), s, "conv dgrad")) return rc;
    int cfg = choose_cfg(p.M, p.N, p.K, false, &splits);
    tune_lookup(1, d, &cfg, &splits);
    split_k(p.K, 1, &p.kchunk);
    return dj_launch_cfg<0, 1>(cfg, p, 1, s);
  }
  p.M = (int)in_pixels;
  p.K = d->kernel_h * d->kernel_w * d->out_c;
  p.rowH = d->in_h;
  p.rowW = d->in_w;
  p.srcH = d->out_h;
  p.srcW = d->out_w;
  fill_geom(p, d);
  p.cmap = 0;
  int cfg = choose_cfg(p.M, p.N, p.K, true, &splits);
  // the launch that also takes BatchNormalization backward statistics runs the EPI twin and is never split: a tuner
  // entry of its own (direction 9), falling back to the plain input gradient's tile variant
  bool tuned1 = false;
  if (!(bnb && tune_lookup(9, d, &cfg, &splits))) tuned1 = tune_lookup(1, d, &cfg, &splits);
  if (a.mask_x) {
    // the masked accumulate completes the value in registers: one K range.  A registered split factor is a measured
    // choice this launch cannot honour -- an error; the launcher's untuned guess is simply not split
    DJ_CHECK_ARG(!(tuned1 && splits > 1), "conv dgrad + ReLU mask: the tuning entry of this geometry splits the reduction");
    splits = 1;
  }
  if (one_k_range || a.dt_dx != DJ_F32) splits = 1;   // (a 16-bit result is written by one K range: no atomics)
  splits = split_k(p.K, splits, &p.kchunk);
  DJ_CHECK_ARG(!io16 || (fast_mode<1, 1>(p)) != 0, "conv dgrad: 16-bit tensors need the branch-free kernel's preconditions "
                                                 "(stride 1, channels %% 32, 16-byte aligned tensors)");
  if (splits > 1) {
    p.atomic = 1;
    if (!beta)
      if (int rc = clear_rows(a.dx, in_pixels, d->in_c, d->ld_x, 4, s, "conv dgrad")) return rc;
    p.beta = 0;
  }
  return dj_launch_cfg<1, 1>(cfg, p, splits, s);
}

extern "C" int dj_conv2d_dgrad_relumask_supported(const dj_conv2d_desc* d) {
  if (check_desc(d)) return 0;
  const int mode = dj_compute_mode();
  if (mode == 1 || mode == 2 || dgrad_is_strided_1x1(d)) return 0;
  int cfg = 0, splits = 1;
  if (tune_lookup(1, d, &cfg, &splits) && splits > 1) return 0;
  return 1;
}

// The weight gradient's untuned choice: tile by the (taps*Cin) x Cout extent only -- the pixel reduction is split over
// blockIdx.y to fill the chip
static int choose_cfg_wgrad(long M, long N, long K, int* splits_out) {
  int cfg;
  if (N > 96 && (long)dj_cdiv(N, 128) * 128 <= (long)dj_cdiv(N, 64) * 64)
    cfg = (M >= 128) ? CFG_128x128 : CFG_64x64;
  else if (N > 32)
    cfg = (M >= 128) ? CFG_128x64 : CFG_64x64;
  else
    cfg = CFG_128x32;
  long t = (long)dj_cdiv(M, kCfgs[cfg].bm) * dj_cdiv(N, kCfgs[cfg].bn);
  long want = (768 + t - 1) / t;
  long maxs = K / 128;
  if (maxs < 1) maxs = 1;
  *splits_out = (int)(want < maxs ? want : maxs);
  if (*splits_out < 1) *splits_out = 1;
  return cfg;
}

extern "C" int dj_conv2d_nhwc_wgrad(const dj_conv2d_desc* d, const dj_conv_wgrad_args* args, void* stream) {
  DJ_CHECK_ARG(args != nullptr, "conv wgrad: null argument struct");
  const dj_conv_wgrad_args& a = *args;
  DJ_CHECK_ARG(dt_ok(a.dt_x) && dt_ok(a.dt_dy), "conv wgrad: unknown storage type");
  if (int rc = check_desc(d)) return rc;
  DJ_CHECK_ARG(a.x && a.dy && a.dw, "conv wgrad: null tensor");
  const bool io16 = a.dt_x != DJ_F32 || a.dt_dy != DJ_F32;
  DJ_CHECK_ARG((a.dt_x == DJ_F32 || a.dt_x == DJ_F16) && (a.dt_dy == DJ_F32 || a.dt_dy == DJ_BF16),
               "conv wgrad: activations are held as fp32 or fp16, gradients as fp32 or bf16");
  DJ_CHECK_ARG(!io16 || dj_compute_mode() == 1, "conv wgrad: 16-bit tensors need arithmetic mode 1 (float16)");
  DJ_CHECK_ARG((a.pro_scale == nullptr) == (a.pro_shift == nullptr), "conv wgrad: pro_scale/pro_shift must come together");
  hipStream_t s = (hipStream_t)stream;
  DjIgemmParams p;
  memset(&p, 0, sizeof(p));
  p.A = (const float*)a.x;
  p.B = (const float*)a.dy;
  p.C = a.dw;
  p.pro_scale = a.pro_scale;
  p.pro_shift = a.pro_shift;
  p.pro_relu = a.pro_relu;
  p.M = d->kernel_h * d->kernel_w * d->in_c;
  p.N = d->out_c;
  p.K = d->batch * d->out_h * d->out_w;
  p.rowH = d->out_h;
  p.rowW = d->out_w;
  p.srcH = d->in_h;
  p.srcW = d->in_w;
  p.srcC = d->in_c;
  p.ldsrc = d->ld_x;
  fill_geom(p, d);
  p.ldb = d->ld_y;
  p.ldc = d->out_c;
  p.cmap = 0;
  p.vecA = (d->in_c % 4 == 0) && (d->ld_x % 4 == 0) && aligned_dt(a.x, a.dt_x) &&
           (!a.pro_scale || (aligned16(a.pro_scale) && aligned16(a.pro_shift)));
  p.vecB = (d->out_c % 4 == 0) && (d->ld_y % 4 == 0) && aligned_dt(a.dy, a.dt_dy);
  p.a_bytes = extent_bytes((long)d->batch * d->in_h * d->in_w, d->ld_x, d->in_c, dt_size(a.dt_x));
  p.b_bytes = extent_bytes((long)d->batch * d->out_h * d->out_w, d->ld_y, d->out_c, dt_size(a.dt_dy));
  p.a_dt = a.dt_x;
  p.b_dt = a.dt_dy;
  DJ_CHECK_ARG(!io16 || (fast_mode<2, 0>(p)) != 0, "conv wgrad: 16-bit tensors need the branch-free kernel's preconditions "
                                                 "(channels %% 4, 16-byte aligned tensors)");
  int splits = 1;
  int cfg = choose_cfg_wgrad(p.M, p.N, p.K, &splits);
  tune_lookup(2, d, &cfg, &splits);
  splits = split_k(p.K, splits, &p.kchunk);
  if (splits > 1) {
    p.atomic = 1;
    if (!a.dw_zeroed)
      if (int rc = memset_status(hipMemsetAsync(a.dw, 0, (size_t)p.M * p.N * 4, s), "conv wgrad")) return rc;
  }
  return dj_launch_cfg<2, 0>(cfg, p, splits, s);
}

extern "C" int dj_conv2d_default_config(int dir, const dj_conv2d_desc* d, int* cfg, int* splits) {
  if (int rc = check_desc(d)) return rc;
  DJ_CHECK_ARG(cfg && splits, "default_config: null output");
  int base = dir & 3;
  *splits = 1;
  if (base == 0)
    *cfg = choose_cfg((long)d->batch * d->out_h * d->out_w, d->out_c, (long)d->kernel_h * d->kernel_w * d->in_c,
                      (dir & 4) == 0, splits);
  else if (base == 1 && dgrad_is_strided_1x1(d))
    *cfg = choose_cfg((long)d->batch * d->out_h * d->out_w, d->in_c, d->out_c, false, splits);
  else if (base == 1)
    *cfg = choose_cfg((long)d->batch * d->in_h * d->in_w, d->in_c, (long)d->kernel_h * d->kernel_w * d->out_c, true, splits);
  else
    *cfg = choose_cfg_wgrad((long)d->kernel_h * d->kernel_w * d->in_c, d->out_c, (long)d->batch * d->out_h * d->out_w, splits);
  return DJ_OK;
}
