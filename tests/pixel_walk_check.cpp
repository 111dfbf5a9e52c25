// Host check of the weight gradient's incremental pixel walk (csrc/dj_walk.h) against the direct decomposition of the
// pixel index that the plain kernels redo every K-step.  Both kernel families walk with this header: the split-bf16
// kernels in K-steps of 16 / 32, the fp32 MFMA kernels in K-steps of 32.  What is walked here: 4-byte elements, K-steps
// of 16 and 32, a thread's chunks 4 * 256 / step channels apart.  Built and run by tests/test_pixel_walk_cpu.py with
// -fsanitize=address,undefined; prints one summary line and exits non-zero on the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dj_walk.h"

namespace {

constexpr unsigned kOut = 0x80000000u;   // "no load": both sides are compared as (in-bounds flag, byte offset)

struct Geom {
  int batch, in_h, in_w, in_c, ld_x, kh, kw, sh, sw, dh, dw, same;
  int out_h, out_w, pad_t, pad_l;
};

// Keras padding rule: 'same' pads so that out = ceil(in / stride), the smaller half in front
void out_and_pad(int in, int k, int stride, int dil, int same, int& out, int& pad) {
  const int span = (k - 1) * dil + 1;
  if (same) {
    out = (in + stride - 1) / stride;
    int total = (out - 1) * stride + span - in;
    if (total < 0) total = 0;
    pad = total / 2;
  } else {
    out = (in - span) / stride + 1;
    if (in < span) out = 0;
    pad = 0;
  }
}

long long g_checked = 0;

// one launch: tiles of bm channels x taps, K chunks of kchunk pixels, K-steps of bk pixels, thread rows 0 .. bk - 1
bool check_launch(const Geom& g, int bm, int bk, int kchunk) {
  const int ea = 4;                       // fp32 tensors
  const int acg = 256 / bk;               // threads per pixel row; a thread's chunks are 4 * acg channels apart
  const int na = bk * bm / 1024;          // chunks per thread
  const int K = g.batch * g.out_h * g.out_w, hw = g.out_h * g.out_w;
  const int M = g.kh * g.kw * g.in_c;
  const DjWalkGeom wg{g.out_h, g.out_w, g.in_h, g.in_w, g.sh, g.sw, g.ld_x * ea};
  const DjWalkStep ws = dj_walk_step(wg, bk);
  if (ws.sw >= g.out_w || ws.sh >= g.out_h) {
    std::printf("step parts out of range\n");
    return false;
  }
  for (int m0 = 0; m0 < M; m0 += bm) {
    const int tap = m0 / g.in_c, cb = m0 - tap * g.in_c;
    const int kh = tap / g.kw, kw = tap - kh * g.kw;
    const int dh = kh * g.dh - g.pad_t, dw = kw * g.dw - g.pad_l;
    for (int kbeg = 0; kbeg < K; kbeg += kchunk) {
      const int kend = (kbeg + kchunk < K) ? kbeg + kchunk : K;
      const int nk = (kend - kbeg + bk - 1) / bk;
      for (int ar0 = 0; ar0 < bk; ++ar0) {
        for (int ac = 0; ac < acg; ac += acg - 1 > 0 ? acg - 1 : 1) {   // first and last thread of a pixel row
          DjWalkPos w = dj_walk_init(wg, kbeg + ar0, dh, dw, (cb + 4 * ac) * ea);
          // two steps past the chunk: the prefetch issues them (never consumed, but they must not load)
          for (int t = 0; t < nk + 2; ++t) {
            const int ih = w.oh * g.sh + dh, iw = w.ow * g.sw + dw;
            const bool ok = dj_walk_inside(wg, w, ih, iw, kend);
            // the direct decomposition
            const int kp = kbeg + t * bk + ar0;
            const int img = kp / hw, rem = kp - img * hw;
            const int oh = rem / g.out_w, ow = rem - oh * g.out_w;
            const int h = oh * g.sh + dh, x = ow * g.sw + dw;
            const bool ref_ok = kp < kend && h >= 0 && h < g.in_h && x >= 0 && x < g.in_w;
            for (int i = 0; i < na; ++i) {
              const int c = cb + 4 * (ac + acg * i);
              const unsigned ref = ref_ok ? (unsigned)(((img * g.in_h * g.in_w + h * g.in_w + x) * g.ld_x + c) * ea) : kOut;
              const unsigned got = ok ? (unsigned)w.off + (unsigned)(4 * acg * ea * i) : kOut;
              ++g_checked;
              if (ok != ref_ok || got != ref) {
                std::printf("mismatch: batch %d map %dx%d c %d ld %d k %dx%d stride %dx%d dil %dx%d same %d | bm %d bk %d kchunk %d "
                            "m0 %d kbeg %d row %d ac %d step %d chunk %d: walk (%d, %u) direct (%d, %u)\n",
                            g.batch, g.in_h, g.in_w, g.in_c, g.ld_x, g.kh, g.kw, g.sh, g.sw, g.dh, g.dw, g.same, bm, bk, kchunk,
                            m0, kbeg, ar0, ac, t, i, (int)ok, got, (int)ref_ok, ref);
                return false;
              }
            }
            if (w.kp != kp || (kp < K && (w.oh != oh || w.ow != ow))) {
              std::printf("position mismatch at step %d\n", t);
              return false;
            }
            dj_walk_advance(wg, ws, w);
          }
        }
      }
    }
  }
  return true;
}

// every launch shape of one geometry; false on the first mismatch
bool check_geom(Geom g, int& launches) {
  out_and_pad(g.in_h, g.kh, g.sh, g.dh, g.same, g.out_h, g.pad_t);
  out_and_pad(g.in_w, g.kw, g.sw, g.dw, g.same, g.out_w, g.pad_l);
  if (g.out_h < 1 || g.out_w < 1) return true;   // 'valid' on a map smaller than the dilated kernel
  const int K = g.batch * g.out_h * g.out_w;
  for (int bk : {16, 32})
    for (int bm : {64, 128}) {
      // chunk lengths as the launcher derives them from a number of splits (multiples of 32): they end
      // mid-row and mid-image on the odd maps; one chunk = the whole reduction
      std::vector<int> chunks;
      for (int splits = 1; splits <= 4; ++splits) {
        const int per = (K + splits - 1) / splits, kc = (per + 31) / 32 * 32;
        if (chunks.empty() || chunks.back() != kc) chunks.push_back(kc);
      }
      for (int kc : chunks) {
        if (!check_launch(g, bm, bk, kc)) return false;
        ++launches;
      }
    }
  return true;
}

Geom geom_of(int batch, int h, int w, int kh, int kw, int sh, int sw, int dh, int dw, int same) {
  return Geom{batch, h, w, (batch == 2) ? 256 : 128, (batch == 3) ? 136 : ((batch == 2) ? 256 : 128), kh, kw, sh, sw, dh, dw,
              same, 0, 0, 0, 0};
}

}   // namespace

int main() {
  const int maps[5][2] = {{1, 1}, {3, 3}, {5, 7}, {10, 10}, {19, 19}};
  int launches = 0;
  for (const auto& mp : maps)
    for (int k : {1, 3})
      for (int stride : {1, 2})
        for (int dil : {1, 6})
          for (int same : {1, 0})
            for (int batch = 1; batch <= 3; ++batch) {
              if (k == 1 && dil != 1) continue;
              if (!check_geom(geom_of(batch, mp[0], mp[1], k, k, stride, stride, dil, dil, same), launches)) return 1;
            }
  const int square = launches;
  // geometries that differ between the axes, on non-square maps of both orientations: kernels (1,3) / (3,1) / (2,3) / (3,3),
  // strides (1,1) / (2,1) / (1,2), dilations (1,1) / (1,3) / (2,1) -- an H/W swap in the step's parts or carries shows here
  const int amaps[4][2] = {{5, 7}, {7, 5}, {11, 8}, {9, 12}};
  const int kernels[4][2] = {{1, 3}, {3, 1}, {2, 3}, {3, 3}};
  const int strides[3][2] = {{1, 1}, {2, 1}, {1, 2}};
  const int dils[3][2] = {{1, 1}, {1, 3}, {2, 1}};
  for (const auto& mp : amaps)
    for (const auto& kk : kernels)
      for (const auto& ss : strides)
        for (const auto& dd : dils)
          for (int same : {1, 0})
            for (int batch = 1; batch <= 3; ++batch) {
              if (kk[0] == kk[1] && ss[0] == ss[1] && dd[0] == dd[1]) continue;   // (the grid above)
              if (!check_geom(geom_of(batch, mp[0], mp[1], kk[0], kk[1], ss[0], ss[1], dd[0], dd[1], same), launches)) return 1;
            }
  std::printf("pixel walk: %d launches, %lld offsets equal; %d launches on geometries that differ between the axes\n", launches,
              g_checked, launches - square);
  return launches > square && square > 0 ? 0 : 1;
}
