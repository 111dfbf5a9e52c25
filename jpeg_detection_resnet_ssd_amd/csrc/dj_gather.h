// Gather arithmetic that the two branch-free convolution GEMMs (dj_igemm_fast.h, dj_igemm_h16.h) share word for word:
// the weight gradient's chunk set-up and the float-reciprocal pixel decomposition of its plain variant.  (Its
// incremental pixel walk, NP 3, is dj_walk.h.)  The helpers return values and write through no reference: a helper is
// optimised on its own before it is inlined, and there a store through a reference may alias every later load from `p`.
//
// What is NOT here, although both kernels hold a copy: the row set-up of the k-contiguous operand, the B offsets, the
// wave-uniform tap state with its advance, and recompute_tap.  Moved into functions, each of them changed the register
// allocation of kernels that use it (compared per kernel against the in-line code); they stay in the kernels until
// they can be shared without that.
#pragma once
#include "dj_igemm.h"

// weight gradient: a thread holds one pixel row of the K-step and 4-channel chunks of the tile's m' range (ONE pixel
// decomposition per K-step).  The chunk at m' = mm: its channel c and its tap's displacement (dh, dw)
struct DjGatherChunk {
  int c, dh, dw;
  bool ok;   // mm < M
};
__device__ __forceinline__ DjGatherChunk dj_gather_chunk(const DjIgemmParams& p, int mm) {
  DjGatherChunk g;
  g.ok = mm < p.M;
  int tap = mm / p.srcC;
  g.c = mm - tap * p.srcC;
  int kh = tap / p.KW;
  int kw = tap - kh * p.KW;
  g.dh = kh * p.dH - p.pT;
  g.dw = kw * p.dW - p.pL;
  return g;
}

// output pixel kp -> (image, oh, ow) for the plain weight gradient, every K-step: the float reciprocal is within one
// of the quotient (K < 2^24, checked by the launcher), a compare on the remainder corrects it
struct DjPixel {
  int img, oh, ow;
};
__device__ __forceinline__ DjPixel dj_pixel_decompose(const DjIgemmParams& p, int kp) {
  const int hw = p.rowH * p.rowW;
  int img = (int)((float)kp * p.inv_rowHW);
  int rem = kp - img * hw;
  int adj = (rem < 0) ? -1 : ((rem >= hw) ? 1 : 0);
  img += adj;
  rem -= adj * hw;
  int oh = (int)((float)rem * p.inv_rowW);
  int ow = rem - oh * p.rowW;
  int adj2 = (ow < 0) ? -1 : ((ow >= p.rowW) ? 1 : 0);
  oh += adj2;
  ow -= adj2 * p.rowW;
  return DjPixel{img, oh, ow};
}
