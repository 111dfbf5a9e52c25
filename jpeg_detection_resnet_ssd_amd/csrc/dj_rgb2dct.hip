// RGB batch -> de-quantised JPEG DCT coefficient tensors, bit-exact with what libjpeg writes into a baseline 4:2:0 file
// and a coefficient reader gets back out of it: the emission step at the end of the reference's generators
// (localisation_part/data_generator/object_detection_2d_data_generator_dct_j2d.py:1167-1195: PIL save + jpeg2dct.loads)
// without the file in between.  Everything between pixels and coefficients is integer arithmetic, restated here from
// libjpeg's documented algorithms: the 16-bit fixed-point RGB->YCbCr conversion, h2v2 box downsampling with its
// alternating 1,2 bias, the "slow" integer forward DCT (13-bit constants, 2 extra bits after the row pass) and
// quantisation by 8*table with round-half-away-from-zero.  The numpy twin is data/jpeg_dct.py:rgb_to_dct_host.
//
// One wave owns one 16x16 MCU (4 luma blocks + Cb + Cr); a 256-thread workgroup holds four of them.  The pass is
// bandwidth bound and small (32 images of 300x300: 8.6 MB in, 17.7 MB out), so it is plain C++: byte loads that run
// along pixel rows, six 8x8 blocks staged in LDS (rows padded to 9 dwords), one row / one column per lane for the two
// 1-D passes, and one contiguous 256 B store per block.
#include "../../include/dj_hip.h"
#include "dj_common.h"

#define DJ_R2D_WAVES 4       // MCUs per workgroup
#define DJ_R2D_LDW 9         // dwords per staged block row: odd, so row-per-lane and column-per-lane reads spread over banks

struct DjRgb2DctParams {
  const unsigned char* rgb;
  float* out_y;
  float* out_cb;
  float* out_cr;
  long ld_y, ld_cb, ld_cr;
  long stride;             // bytes between pixel rows
  long n_mcu;              // batch * mcu_h * mcu_w
  int H, W;
  int mcu_h, mcu_w;        // ceil(H/16), ceil(W/16) (also the chroma block grid)
  int ybh, ybw;            // luma block grid ceil(H/8), ceil(W/8)
  int normalized;
  unsigned short table[2][64];   // luma, chroma; natural order
};

__device__ __forceinline__ int r2d_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// libjpeg jfdctint.c's 1-D pass.  FIRST: the row pass (outputs scaled up by 4), else the column pass.
template <bool FIRST>
__device__ __forceinline__ void r2d_fdct8(int* d) {
  const int n = FIRST ? 11 : 15;
  int t0 = d[0] + d[7], t7 = d[0] - d[7];
  int t1 = d[1] + d[6], t6 = d[1] - d[6];
  int t2 = d[2] + d[5], t5 = d[2] - d[5];
  int t3 = d[3] + d[4], t4 = d[3] - d[4];
  int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (FIRST) {
    d[0] = (t10 + t11) * 4;
    d[4] = (t10 - t11) * 4;
  } else {
    d[0] = r2d_descale(t10 + t11, 2);
    d[4] = r2d_descale(t10 - t11, 2);
  }
  int z1 = (t12 + t13) * 4433;
  d[2] = r2d_descale(z1 + t13 * 6270, n);
  d[6] = r2d_descale(z1 - t12 * 15137, n);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  int z5 = (z3 + z4) * 9633;
  t4 *= 2446;
  t5 *= 16819;
  t6 *= 25172;
  t7 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7] = r2d_descale(t4 + z1 + z3, n);
  d[5] = r2d_descale(t5 + z2 + z4, n);
  d[3] = r2d_descale(t6 + z2 + z3, n);
  d[1] = r2d_descale(t7 + z1 + z4, n);
}

__global__ __launch_bounds__(DJ_R2D_WAVES * 64) void dj_rgb2dct_kernel(DjRgb2DctParams p) {
  __shared__ int blocks[DJ_R2D_WAVES][6][8][DJ_R2D_LDW];   // Y00 Y01 Y10 Y11 Cb Cr, samples - 128, then coefficients
  __shared__ unsigned char chroma[DJ_R2D_WAVES][2][16][16];  // full-resolution Cb, Cr of the MCU
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long mcu = (long)blockIdx.x * DJ_R2D_WAVES + wave;
  const bool live = mcu < p.n_mcu;      // a wave past the end loads and stores nothing but keeps the barriers
  const long per_img = (long)p.mcu_h * p.mcu_w;
  const long img = live ? mcu / per_img : 0;
  const int rem = live ? (int)(mcu - img * per_img) : 0;
  const int my = rem / p.mcu_w, mx = rem - my * p.mcu_w;
  int(*blk)[8][DJ_R2D_LDW] = blocks[wave];
  unsigned char(*chr)[16][16] = chroma[wave];

  // ---- pixels -> Y (into the four luma blocks) and full-resolution Cb, Cr; the image edge is replicated ----
  if (live) {
    const unsigned char* base = p.rgb + (size_t)img * p.H * p.stride;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pix = i * 64 + lane, ly = pix >> 4, lx = pix & 15;
      const int gy = min(my * 16 + ly, p.H - 1), gx = min(mx * 16 + lx, p.W - 1);
      const unsigned char* px = base + (size_t)gy * p.stride + (size_t)gx * 3;
      const int r = px[0], g = px[1], b = px[2];
      const int yv = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
      const int cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16;
      const int cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16;
      blk[(ly >> 3) * 2 + (lx >> 3)][ly & 7][lx & 7] = yv - 128;
      chr[0][ly][lx] = (unsigned char)cb;
      chr[1][ly][lx] = (unsigned char)cr;
    }
  }
  __syncthreads();

  // ---- 2x2 chroma averaging.  Columns: the full-resolution plane is replicated to the MCU edge BEFORE averaging (the
  // clamped loads above did that).  Rows: an odd last row pairs with itself, and below that the last AVERAGED row is
  // replicated -- so the pair is chosen from the clamped chroma row, not from clamped pixel rows. ----
  if (live) {
    const int cy = lane >> 3, cx = lane & 7;
    const int ch = (p.H + 1) >> 1;
    const int cyg = min(my * 8 + cy, ch - 1);
    const int r0 = 2 * cyg - my * 16;                      // >= 0: the MCU exists, so my * 8 <= ch - 1
    const int r1 = min(2 * cyg + 1, p.H - 1) - my * 16;
    const int bias = 1 + (cx & 1);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int s = chr[c][r0][2 * cx] + chr[c][r0][2 * cx + 1] + chr[c][r1][2 * cx] + chr[c][r1][2 * cx + 1];
      blk[4 + c][cy][cx] = ((s + bias) >> 2) - 128;
    }
  }
  __syncthreads();

  // ---- forward DCT: rows (one per lane, 48 lanes), then columns ----
  const int b6 = lane >> 3, k = lane & 7;
  if (lane < 48) {
    int d[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = blk[b6][k][j];
    r2d_fdct8<true>(d);
#pragma unroll
    for (int j = 0; j < 8; ++j) blk[b6][k][j] = d[j];
  }
  __syncthreads();
  if (lane < 48) {
    int d[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = blk[b6][j][k];
    r2d_fdct8<false>(d);
#pragma unroll
    for (int j = 0; j < 8; ++j) blk[b6][j][k] = d[j];
  }
  __syncthreads();

  // ---- quantise (exact integer division by 8 * table, half away from zero), de-quantise, store: lane = 8u + v ----
  if (live) {
    const int q_luma = p.table[0][lane], q_chroma = p.table[1][lane];
#pragma unroll
    for (int b = 0; b < 6; ++b) {
      const int q = b < 4 ? q_luma : q_chroma;
      const int c = blk[b][lane >> 3][lane & 7];
      const unsigned q8 = 8u * (unsigned)q;
      const unsigned a = (unsigned)(c < 0 ? -c : c);
      int level = (int)((a + (q8 >> 1)) / q8);
      if (c < 0) level = -level;
      const float v = (float)(p.normalized ? level * q : level);
      if (b < 4) {
        const int by = my * 2 + (b >> 1), bx = mx * 2 + (b & 1);
        if (by < p.ybh && bx < p.ybw)
          p.out_y[(((size_t)img * p.ybh + by) * p.ybw + bx) * p.ld_y + lane] = v;
      } else {
        float* out = b == 4 ? p.out_cb : p.out_cr;
        const long ld = b == 4 ? p.ld_cb : p.ld_cr;
        out[(((size_t)img * p.mcu_h + my) * p.mcu_w + mx) * ld + lane] = v;
      }
    }
  }
}

extern "C" int dj_rgb_to_dct(const unsigned char* rgb, int batch, int height, int width, long stride_bytes,
                             const unsigned short* luma_table, const unsigned short* chroma_table, int normalized,
                             float* out_y, long ld_y, float* out_cb, long ld_cb, float* out_cr, long ld_cr, void* stream) {
  DJ_CHECK_ARG(rgb, "rgb_to_dct: rgb is null");
  DJ_CHECK_ARG(luma_table, "rgb_to_dct: luma_table is null");
  DJ_CHECK_ARG(chroma_table, "rgb_to_dct: chroma_table is null");
  DJ_CHECK_ARG(out_y, "rgb_to_dct: out_y is null");
  DJ_CHECK_ARG(out_cb, "rgb_to_dct: out_cb is null");
  DJ_CHECK_ARG(out_cr, "rgb_to_dct: out_cr is null");
  DJ_CHECK_ARG(batch >= 1, "rgb_to_dct: batch must be >= 1 (got %d)", batch);
  DJ_CHECK_ARG(height >= 1, "rgb_to_dct: height must be >= 1 (got %d)", height);
  DJ_CHECK_ARG(width >= 1, "rgb_to_dct: width must be >= 1 (got %d)", width);
  DJ_CHECK_ARG(height <= 65536 && width <= 65536, "rgb_to_dct: height / width above 65536 (got %d x %d)", height, width);
  DJ_CHECK_ARG(stride_bytes >= 3L * width, "rgb_to_dct: stride_bytes %ld below 3 * width = %ld", stride_bytes, 3L * width);
  DJ_CHECK_ARG(ld_y >= 64, "rgb_to_dct: ld_y %ld below 64", ld_y);
  DJ_CHECK_ARG(ld_cb >= 64, "rgb_to_dct: ld_cb %ld below 64", ld_cb);
  DJ_CHECK_ARG(ld_cr >= 64, "rgb_to_dct: ld_cr %ld below 64", ld_cr);
  DjRgb2DctParams p;
  for (int i = 0; i < 64; ++i) {
    DJ_CHECK_ARG(luma_table[i] >= 1 && luma_table[i] <= 255, "rgb_to_dct: luma_table[%d] = %d outside 1..255", i,
                 (int)luma_table[i]);
    DJ_CHECK_ARG(chroma_table[i] >= 1 && chroma_table[i] <= 255, "rgb_to_dct: chroma_table[%d] = %d outside 1..255", i,
                 (int)chroma_table[i]);
    p.table[0][i] = luma_table[i];
    p.table[1][i] = chroma_table[i];
  }
  p.rgb = rgb;
  p.out_y = out_y;
  p.out_cb = out_cb;
  p.out_cr = out_cr;
  p.ld_y = ld_y;
  p.ld_cb = ld_cb;
  p.ld_cr = ld_cr;
  p.stride = stride_bytes;
  p.H = height;
  p.W = width;
  p.mcu_h = (height + 15) / 16;
  p.mcu_w = (width + 15) / 16;
  p.ybh = (height + 7) / 8;
  p.ybw = (width + 7) / 8;
  p.n_mcu = (long)batch * p.mcu_h * p.mcu_w;
  p.normalized = normalized != 0;
  const long grid = (p.n_mcu + DJ_R2D_WAVES - 1) / DJ_R2D_WAVES;
  DJ_CHECK_ARG(grid <= 0x7fffffffL, "rgb_to_dct: batch * height * width too large for one launch");
  hipLaunchKernelGGL(dj_rgb2dct_kernel, dim3((unsigned)grid), dim3(DJ_R2D_WAVES * 64), 0, (hipStream_t)stream, p);
  DJ_CHECK_LAUNCH("dj_rgb_to_dct");
  return DJ_OK;
}
