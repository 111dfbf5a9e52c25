// Incremental pixel walk of the weight gradient's gathered operand (NP 3 of dj_igemm_fast.h and of dj_igemm_h16.h).
//
// The weight-gradient GEMM reduces over output pixels: K-step t of a thread reads output pixel kp = kp0 + t * step
// (pixels are numbered image-major, then row, then column, over the rowH x rowW output map) and, under ONE filter tap
// (dh, dw), the input pixel (oh * sH + dh, ow * sW + dw) of the same image.  Decomposing kp every K-step costs two
// reciprocals and half a dozen integer multiplies per thread; but every thread moves by the SAME number of pixels per
// K-step, so (ow, oh) and the byte offset of the tapped input pixel advance by constants with two carries:
//
//   step = s_img * rowH * rowW + sh * rowW + sw   with sw < rowW, sh < rowH
//   ow += sw;            carry c1 when ow reaches rowW (at most once: ow < rowW, sw < rowW)
//   oh += sh + c1;       carry c2 when oh reaches rowH (at most once: oh + sh + 1 <= 2 rowH - 1)
//   off += c0 + (c1 ? add1 : 0) + (c2 ? add2 : 0)
//
// Plain C++: both kernel families include it, and so does the host program that checks the walk against the direct
// decomposition for every K-step of a grid of geometries (tests/pixel_walk_check.cpp) -- the check covers both.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DJ_WALK_HD __host__ __device__ __forceinline__
#else
#define DJ_WALK_HD inline
#endif

// the geometry the walk needs: output map, input map, strides, bytes between two input pixels
struct DjWalkGeom {
  int rowH, rowW, srcH, srcW, sH, sW, pix_bytes;
};

// what one K-step adds (the same for every thread of a launch)
struct DjWalkStep {
  int step;         // pixels per K-step
  int sw, sh;       // its column and row parts
  int c0, c1, c2;   // bytes per K-step, extra bytes of a row carry, extra bytes of an image carry
};

// a thread's position
struct DjWalkPos {
  int ow, oh;   // output pixel inside its image
  int kp;       // its index over all images
  int off;      // byte offset of the tapped input pixel (plus whatever the caller put into `base`)
};

DJ_WALK_HD DjWalkStep dj_walk_step(const DjWalkGeom& g, int step) {
  DjWalkStep s;
  const int hw = g.rowH * g.rowW;
  const int s_img = step / hw, r = step - s_img * hw;
  s.step = step;
  s.sh = r / g.rowW;
  s.sw = r - s.sh * g.rowW;
  s.c0 = ((s_img * g.srcH + s.sh * g.sH) * g.srcW + s.sw * g.sW) * g.pix_bytes;
  s.c1 = (g.sH * g.srcW - g.rowW * g.sW) * g.pix_bytes;
  s.c2 = (g.srcH - g.rowH * g.sH) * g.srcW * g.pix_bytes;
  return s;
}

// pixel kp under the tap (dh, dw); `base`: bytes added to every offset (channel position of the thread's first chunk)
DJ_WALK_HD DjWalkPos dj_walk_init(const DjWalkGeom& g, int kp, int dh, int dw, int base) {
  DjWalkPos w;
  const int hw = g.rowH * g.rowW;
  const int img = kp / hw, rem = kp - img * hw;
  w.kp = kp;
  w.oh = rem / g.rowW;
  w.ow = rem - w.oh * g.rowW;
  w.off = ((img * g.srcH + w.oh * g.sH + dh) * g.srcW + w.ow * g.sW + dw) * g.pix_bytes + base;
  return w;
}

// is the tapped input pixel (ih, iw) = (oh * sH + dh, ow * sW + dw) of the current position a pixel of the image, and
// the position before `kend` (the end of the K chunk)?  The caller computes ih / iw (on the GPU with 24-bit multiplies).
DJ_WALK_HD bool dj_walk_inside(const DjWalkGeom& g, const DjWalkPos& w, int ih, int iw, int kend) {
  return (w.kp < kend) & ((unsigned)ih < (unsigned)g.srcH) & ((unsigned)iw < (unsigned)g.srcW);
}

DJ_WALK_HD void dj_walk_advance(const DjWalkGeom& g, const DjWalkStep& s, DjWalkPos& w) {
  w.kp += s.step;
  w.ow += s.sw;
  const bool c1 = w.ow >= g.rowW;
  w.ow -= c1 ? g.rowW : 0;
  w.oh += s.sh + (c1 ? 1 : 0);
  const bool c2 = w.oh >= g.rowH;
  w.oh -= c2 ? g.rowH : 0;
  w.off += s.c0 + (c1 ? s.c1 : 0) + (c2 ? s.c2 : 0);
}
