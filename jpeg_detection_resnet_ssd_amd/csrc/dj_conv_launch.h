// Tile variants of the implicit-GEMM convolution and their launchers.  dj_launch_cfg<AM, BMD> is instantiated once per
// GEMM role in its own translation unit (dj_conv_i*.hip) so that the ~100 kernel instantiations compile in parallel.
#pragma once
#include "../../include/dj_hip.h"
#include "dj_igemm.h"
#include "dj_igemm_fast.h"
#include <stdlib.h>
#include <atomic>

// ---------------------------------------------------------------------------------
// tile configurations
// ---------------------------------------------------------------------------------
struct TileCfg {
  int bm, bn;
};
static const TileCfg kCfgs[] = {{128, 128}, {128, 64}, {64, 64}, {128, 32}, {128, 128}, {128, 64}, {64, 64}, {64, 64}, {128, 64}, {128, 128}, {128, 64}, {64, 64}, {64, 64}, {128, 64}};
// *_S1: same tile with a single LDS stage; *_S1P: single stage with loads two K-steps ahead; *_P: two stages with
// the pinned-load / read-ahead schedule (fast kernel only; the generic kernel ignores the distinction)
enum {
  CFG_128x128 = 0,
  CFG_128x64,
  CFG_64x64,
  CFG_128x32,
  CFG_128x128_S1,
  CFG_128x64_S1,
  CFG_64x64_S1,
  CFG_64x64_S1P,
  CFG_128x64_S1P,
  CFG_128x128_P,
  CFG_128x64_P,
  CFG_64x64_P,
  CFG_64x64_PK2,
  CFG_128x64_PK2,
  N_CFG
};

template <typename KernT>
static int launch_kernel(KernT kern, int smem_bytes, int bm, int bn, const DjIgemmParams& p, int splits, hipStream_t s,
                         std::atomic<bool>* attr_done, int threads = 256) {
  // (first launch of an instantiation: two threads may both get here -- the call is idempotent, the flag is atomic so
  // that the header's "callable from any thread" holds by the letter as well)
  if (!attr_done->load(std::memory_order_relaxed)) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem_bytes);
    if (e != hipSuccess) {
      dj_set_error("hipFuncSetAttribute(%d B LDS): %s", smem_bytes, hipGetErrorString(e));
      return DJ_ERR_HIP;
    }
    attr_done->store(true, std::memory_order_relaxed);
  }
  int tiles_m = dj_cdiv(p.M, bm), tiles_n = dj_cdiv(p.N, bn);
  dim3 grid((unsigned)(tiles_m * tiles_n), (unsigned)splits);
  hipLaunchKernelGGL(kern, grid, dim3(threads), smem_bytes, s, p);
  DJ_CHECK_LAUNCH("dj_igemm_kernel");
  return DJ_OK;
}

// One launch site per kernel instantiation; an input-gradient launch that asks for BatchNormalization backward statistics
// (p.bnb_z) takes the EPI = 1 twin of the same variant, one that asks for the masked accumulate (p.mask_x) the EPI = 2 twin.
template <int BM, int BN, int WM, int WN, int AM, int BMD, int PRO, int NSTAGE, int KS, int NP>
static int launch_fast(int smem_bytes, const DjIgemmParams& p, int splits, hipStream_t s, int threads = 256) {
  if constexpr (AM == 1 && BMD == 1 && PRO == 0) {   // (the input-gradient GEMM has no prologue)
    if (p.bnb_z) {
      static std::atomic<bool> done1{false};
      return launch_kernel(dj_igemm_fast_kernel<BM, BN, WM, WN, AM, BMD, PRO, NSTAGE, KS, NP, 1>, smem_bytes, BM, BN, p,
                           splits, s, &done1, threads);
    }
    if (p.mask_x) {
      static std::atomic<bool> done2{false};
      return launch_kernel(dj_igemm_fast_kernel<BM, BN, WM, WN, AM, BMD, PRO, NSTAGE, KS, NP, 2>, smem_bytes, BM, BN, p,
                           splits, s, &done2, threads);
    }
  }
  if (p.mask_x) {
    dj_set_error("masked accumulate outside the input-gradient GEMM");
    return DJ_ERR_ARG;
  }
  static std::atomic<bool> done0{false};
  return launch_kernel(dj_igemm_fast_kernel<BM, BN, WM, WN, AM, BMD, PRO, NSTAGE, KS, NP, 0>, smem_bytes, BM, BN, p, splits,
                       s, &done0, threads);
}

extern std::atomic<bool> g_dj_allow_fast;   // dj_conv.hip
// dj_set_gather_variants (dj_conv.hip): false sends the launches of BOTH kernel families that would take the tap-cache /
// pixel-walk variants (NP 2 / 3) to their plain twins (NP 0); the bounds-free 1x1 variant (NP 1) is outside the switch
extern std::atomic<bool> g_dj_gather_variants;

// The gather variant (NP of dj_igemm_fast.h / dj_igemm_h16.h) of a branch-free launch: GEMM role `am`, tile rows `bm`,
// prologue `pro`.  np23: whether the caller has the NP 2 / 3 instantiations at all.
//   1: 1x1 kernel without padding -- for the weight gradient also stride 1, input pixel == output pixel
//   3: weight gradient with taps / padding / stride whose tiles lie under one filter tap each (incremental pixel walk)
//   2: forward / input gradient with taps / padding (row offsets of the current tap cached across its K-steps)
//   0: everything else, the residual-add prologue, and what the switches turn off: DJ_NO_NP=1 (all variants),
//      DJ_NO_WALK=1 (3), DJ_NO_TAPCACHE=1 (2), dj_set_gather_variants(0) (2 and 3)
inline int dj_gather_variant(int am, int bm, int pro, const DjIgemmParams& p, bool np23 = true) {
  static const bool np_off = getenv("DJ_NO_NP") != nullptr, walk_off = getenv("DJ_NO_WALK") != nullptr,
                    tap_off = getenv("DJ_NO_TAPCACHE") != nullptr;
  if (np_off || pro == 3) return 0;
  const bool same_grid = am != 2 || (p.sH == 1 && p.sW == 1 && p.rowH == p.srcH && p.rowW == p.srcW);
  if (p.KH == 1 && p.KW == 1 && p.pT == 0 && p.pL == 0 && same_grid) return 1;
  if (!np23 || !g_dj_gather_variants.load(std::memory_order_relaxed)) return 0;
  if (am == 2) return (!walk_off && p.srcC % bm == 0) ? 3 : 0;
  return tap_off ? 0 : 2;
}

// the branch-free kernel's instantiation for a variant (NP 2 exists for forward / input gradient, NP 3 for the weight gradient)
template <int BM, int BN, int WM, int WN, int AM, int BMD, int PRO, int NSTAGE>
static int launch_fast_np(int smem_bytes, const DjIgemmParams& p, int splits, hipStream_t s) {
  const int np = dj_gather_variant(AM, BM, PRO, p);
  if (np == 1) return launch_fast<BM, BN, WM, WN, AM, BMD, PRO, NSTAGE, 1, 1>(smem_bytes, p, splits, s);
  if constexpr (AM == 2) {
    if (np == 3) return launch_fast<BM, BN, WM, WN, AM, BMD, PRO, NSTAGE, 1, 3>(smem_bytes, p, splits, s);
  } else {
    if (np == 2) return launch_fast<BM, BN, WM, WN, AM, BMD, PRO, NSTAGE, 1, 2>(smem_bytes, p, splits, s);
  }
  return launch_fast<BM, BN, WM, WN, AM, BMD, PRO, NSTAGE, 1, 0>(smem_bytes, p, splits, s);
}

// fast = 0: generic kernel; 1: branch-free kernel; 2: branch-free kernel with the affine prologue; 3: with the
// residual-add prologue
template <int BM, int BN, int WM, int WN, int AM, int BMD, int NSTAGE>
static int launch_one(const DjIgemmParams& p, int splits, hipStream_t s, int fast) {
  using Cfg = DjIgemmCfg<BM, BN, WM, WN, AM, BMD>;
  static std::atomic<bool> done[1] = {{false}};
  const int smem_fast = Cfg::SMEM_BYTES / 2 * ((NSTAGE == 2 || NSTAGE == 4) ? 2 : 1);
  if (fast == 1) return launch_fast_np<BM, BN, WM, WN, AM, BMD, 0, NSTAGE>(smem_fast, p, splits, s);
  if (fast == 2) return launch_fast_np<BM, BN, WM, WN, AM, BMD, 1, NSTAGE>(smem_fast, p, splits, s);
  if (fast == 3) {   // forward GEMM only
    if constexpr (AM == 0 && BMD == 0) {
      return launch_fast<BM, BN, WM, WN, AM, BMD, 3, NSTAGE, 1, 0>(smem_fast, p, splits, s);
    } else {
      dj_set_error("residual-add prologue outside the forward GEMM");
      return DJ_ERR_ARG;
    }
  }
  if (p.mask_x) {   // masked accumulate on the generic kernel: its EPI = 2 twin (input-gradient GEMM only)
    if constexpr (AM == 1 && BMD == 1) {
      static std::atomic<bool> done2{false};
      return launch_kernel(dj_igemm_kernel<BM, BN, WM, WN, AM, BMD, 2>, Cfg::SMEM_BYTES, BM, BN, p, splits, s, &done2);
    } else {
      dj_set_error("masked accumulate outside the input-gradient GEMM");
      return DJ_ERR_ARG;
    }
  }
  return launch_kernel(dj_igemm_kernel<BM, BN, WM, WN, AM, BMD>, Cfg::SMEM_BYTES, BM, BN, p, splits, s, &done[0]);
}

// two K groups per workgroup: pipelined schedule, 512 threads, two LDS rings
template <int BM, int BN, int AM, int BMD>
static int launch_k2(const DjIgemmParams& p, int splits, hipStream_t s, int fast) {
  using Cfg = DjIgemmCfg<BM, BN, 2, 2, AM, BMD>;
  if (fast == 1)
    return launch_fast<BM, BN, 2, 2, AM, BMD, 0, 4, 2, 0>(2 * Cfg::SMEM_BYTES, p, splits, s, 512);
  if (fast == 3) {
    if constexpr (AM == 0 && BMD == 0) {
      return launch_fast<BM, BN, 2, 2, AM, BMD, 3, 4, 2, 0>(2 * Cfg::SMEM_BYTES, p, splits, s, 512);
    } else {
      dj_set_error("residual-add prologue outside the forward GEMM");
      return DJ_ERR_ARG;
    }
  }
  return launch_fast<BM, BN, 2, 2, AM, BMD, 1, 4, 2, 0>(2 * Cfg::SMEM_BYTES, p, splits, s, 512);
}

// 0: fp32 results (default; fp32 MFMA or split-bf16 kernel per tuning entry), 5: fp32 MFMA only.  1: forward GEMMs round
// their operands to fp16, gradient GEMMs (dgrad, wgrad) to bf16 (gradients need the exponent range); 2: bf16 everywhere;
// 3 / 4: fp32 products as three / six bf16 MFMAs on split operands.  fp32 accumulation in all modes.
int dj_compute_mode();   // dj_conv.hip: the calling thread's override, else the process default

// Preconditions of dj_igemm_fast_kernel (see its header comment).
template <int AM, int BMD>
static int fast_mode(const DjIgemmParams& p) {
  if (!g_dj_allow_fast.load(std::memory_order_relaxed) || !p.vecA || !p.vecB) return 0;
  if (p.a_bytes <= 0 || p.b_bytes <= 0) return 0;  // operand >= 2 GiB (extent overflowed int)
  if (AM != 2 && p.srcC % 32 != 0) return 0;
  if (AM != 2 && p.M >= (1 << 22)) return 0;   // dj_row_decompose: float-reciprocal row decomposition
  if (AM == 1 && (p.sH != 1 || p.sW != 1)) return 0;
  if (AM == 2 && (p.srcC % 4 != 0 || p.K >= (1 << 24))) return 0;
  if (BMD == 0 && (p.N % 4 != 0 || p.ldb % 4 != 0)) return 0;
  if (BMD == 1 && p.srcC % 32 != 0) return 0;
  if (p.A2) return (AM == 0 && BMD == 0 && p.pro_scale) ? 3 : 0;
  return p.pro_scale ? 2 : 1;
}

// reduced-precision MFMA variants exist for the two-stage 128x128 / 128x64 / 64x64 tiles of the fast kernel
static inline int dj_fast_mode_fwd(const DjIgemmParams& p) { return fast_mode<0, 0>(p); }

// Reduced-precision (16-bit-tile) variants: defined in dj_conv_launch_h16.h and instantiated in translation units of their
// own (dj_conv_h*.hip), so that they compile beside the fp32 kernels instead of behind them
template <int AM, int BMD>
int dj_launch_lowp(int cfg, const DjIgemmParams& p, int splits, hipStream_t s, int fast, int mode);

template <int AM, int BMD>
int dj_launch_cfg(int cfg, const DjIgemmParams& p, int splits, hipStream_t s) {
  const int fast = fast_mode<AM, BMD>(p);
  int mode = dj_compute_mode();
  if (mode == 5) mode = 0;                      // fp32 MFMA kernels only: its tables hold indices below N_CFG
  if (cfg >= N_CFG) {
    // mode 0, upper half of the index range: the split-bf16 kernel (fp32 tensors, fp32 results; dj_igemm_h16.h PREC 4)
    // of that index -- where the branch-free kernels' preconditions do not hold, the fp32 variant of the same index
    cfg -= N_CFG;
    if (fast && mode == 0 && cfg < N_CFG) return dj_launch_lowp<AM, BMD>(cfg, p, splits, s, fast, 4);
  }
  if (fast && mode != 0 && cfg >= 0 && cfg < N_CFG) {
    // A-mode 0 with B-mode 0 is the forward GEMM; everything else carries gradients
    return dj_launch_lowp<AM, BMD>(cfg, p, splits, s, fast, mode);
  }
  switch (cfg) {
    case CFG_128x128: return launch_one<128, 128, 2, 2, AM, BMD, 2>(p, splits, s, fast);
    case CFG_128x64: return launch_one<128, 64, 2, 2, AM, BMD, 2>(p, splits, s, fast);
    case CFG_64x64: return launch_one<64, 64, 2, 2, AM, BMD, 2>(p, splits, s, fast);
    case CFG_128x32: return launch_one<128, 32, 4, 1, AM, BMD, 2>(p, splits, s, fast);
    case CFG_128x128_S1:
      return fast ? launch_one<128, 128, 2, 2, AM, BMD, 1>(p, splits, s, fast)
                  : launch_one<128, 128, 2, 2, AM, BMD, 2>(p, splits, s, fast);
    case CFG_128x64_S1:
      return fast ? launch_one<128, 64, 2, 2, AM, BMD, 1>(p, splits, s, fast)
                  : launch_one<128, 64, 2, 2, AM, BMD, 2>(p, splits, s, fast);
    case CFG_64x64_S1:
      return fast ? launch_one<64, 64, 2, 2, AM, BMD, 1>(p, splits, s, fast)
                  : launch_one<64, 64, 2, 2, AM, BMD, 2>(p, splits, s, fast);
    case CFG_64x64_S1P:
      return fast ? launch_one<64, 64, 2, 2, AM, BMD, 3>(p, splits, s, fast)
                  : launch_one<64, 64, 2, 2, AM, BMD, 2>(p, splits, s, fast);
    case CFG_128x64_S1P:
      return fast ? launch_one<128, 64, 2, 2, AM, BMD, 3>(p, splits, s, fast)
                  : launch_one<128, 64, 2, 2, AM, BMD, 2>(p, splits, s, fast);
    case CFG_128x128_P:
      return fast ? launch_one<128, 128, 2, 2, AM, BMD, 4>(p, splits, s, fast)
                  : launch_one<128, 128, 2, 2, AM, BMD, 2>(p, splits, s, fast);
    case CFG_128x64_P:
      return fast ? launch_one<128, 64, 2, 2, AM, BMD, 4>(p, splits, s, fast)
                  : launch_one<128, 64, 2, 2, AM, BMD, 2>(p, splits, s, fast);
    case CFG_64x64_P:
      return fast ? launch_one<64, 64, 2, 2, AM, BMD, 4>(p, splits, s, fast)
                  : launch_one<64, 64, 2, 2, AM, BMD, 2>(p, splits, s, fast);
    case CFG_64x64_PK2:
      return fast ? launch_k2<64, 64, AM, BMD>(p, splits, s, fast) : launch_one<64, 64, 2, 2, AM, BMD, 2>(p, splits, s, fast);
    case CFG_128x64_PK2:
      return fast ? launch_k2<128, 64, AM, BMD>(p, splits, s, fast)
                  : launch_one<128, 64, 2, 2, AM, BMD, 2>(p, splits, s, fast);
  }
  dj_set_error("bad tile cfg %d", cfg);
  return DJ_ERR_ARG;
}

