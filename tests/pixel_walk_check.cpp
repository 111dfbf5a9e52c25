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
  int batch, in_h, in_w, in_c, ld_x, k, stride, dil, same;
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
  const int M = g.k * g.k * g.in_c;
  const DjWalkGeom wg{g.out_h, g.out_w, g.in_h, g.in_w, g.stride, g.stride, g.ld_x * ea};
  const DjWalkStep ws = dj_walk_step(wg, bk);
  if (ws.sw >= g.out_w || ws.sh >= g.out_h) {
    std::printf("step parts out of range\n");
    return false;
  }
  for (int m0 = 0; m0 < M; m0 += bm) {
    const int tap = m0 / g.in_c, cb = m0 - tap * g.in_c;
    const int kh = tap / g.k, kw = tap - kh * g.k;
    const int dh = kh * g.dil - g.pad_t, dw = kw * g.dil - g.pad_l;
    for (int kbeg = 0; kbeg < K; kbeg += kchunk) {
      const int kend = (kbeg + kchunk < K) ? kbeg + kchunk : K;
      const int nk = (kend - kbeg + bk - 1) / bk;
      for (int ar0 = 0; ar0 < bk; ++ar0) {
        for (int ac = 0; ac < acg; ac += acg - 1 > 0 ? acg - 1 : 1) {   // first and last thread of a pixel row
          DjWalkPos w = dj_walk_init(wg, kbeg + ar0, dh, dw, (cb + 4 * ac) * ea);
          // two steps past the chunk: the prefetch issues them (never consumed, but they must not load)
          for (int t = 0; t < nk + 2; ++t) {
            const int ih = w.oh * g.stride + dh, iw = w.ow * g.stride + dw;
            const bool ok = dj_walk_inside(wg, w, ih, iw, kend);
            // the direct decomposition
            const int kp = kbeg + t * bk + ar0;
            const int img = kp / hw, rem = kp - img * hw;
            const int oh = rem / g.out_w, ow = rem - oh * g.out_w;
            const int h = oh * g.stride + dh, x = ow * g.stride + dw;
            const bool ref_ok = kp < kend && h >= 0 && h < g.in_h && x >= 0 && x < g.in_w;
            for (int i = 0; i < na; ++i) {
              const int c = cb + 4 * (ac + acg * i);
              const unsigned ref = ref_ok ? (unsigned)(((img * g.in_h * g.in_w + h * g.in_w + x) * g.ld_x + c) * ea) : kOut;
              const unsigned got = ok ? (unsigned)w.off + (unsigned)(4 * acg * ea * i) : kOut;
              ++g_checked;
              if (ok != ref_ok || got != ref) {
                std::printf("mismatch: batch %d map %dx%d c %d ld %d k %d stride %d dil %d same %d | bm %d bk %d kchunk %d m0 %d "
                            "kbeg %d row %d ac %d step %d chunk %d: walk (%d, %u) direct (%d, %u)\n",
                            g.batch, g.in_h, g.in_w, g.in_c, g.ld_x, g.k, g.stride, g.dil, g.same, bm, bk, kchunk, m0, kbeg,
                            ar0, ac, t, i, (int)ok, got, (int)ref_ok, ref);
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
              Geom g{batch, mp[0], mp[1], (batch == 2) ? 256 : 128, (batch == 3) ? 136 : ((batch == 2) ? 256 : 128), k, stride, dil,
                     same, 0, 0, 0, 0};
              out_and_pad(g.in_h, k, stride, dil, same, g.out_h, g.pad_t);
              out_and_pad(g.in_w, k, stride, dil, same, g.out_w, g.pad_l);
              if (g.out_h < 1 || g.out_w < 1) continue;   // 'valid' on a map smaller than the dilated kernel
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
                    if (!check_launch(g, bm, bk, kc)) return 1;
                    ++launches;
                  }
                }
            }
  std::printf("pixel walk: %d launches, %lld offsets equal\n", launches, g_checked);
  return launches > 0 ? 0 : 1;
}
