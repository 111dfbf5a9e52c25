// Photometric augmentation of a [batch][H][W][3] uint8 tensor in place: the `saturation`, `brightness`, `contrast` and
// `lighting` callables of the reference's classifier generators (classification_part/vgg_jpeg_keras/generators/helper.py:12-45,
// applied at generators.py:169-176 between the flip and the JPEG emission), bit for bit what numpy computes in float64 on
// the host.  data/photometric.py states the whole contract (`photometric_host`); the parts that decide bits are:
//
//   grey value     fma(b, 0.114, fma(g, 0.587, r * 0.299)): what `rgb.dot([0.299, 0.587, 0.114])` evaluates to.  This file
//                  is compiled with contraction OFF, so that this is the only fused operation in it: every other product
//                  and sum rounds on its own, as numpy's elementwise loops do.
//   mean (contrast) numpy's sum over the H*W grey values, divided by H*W: the reduction hands the values over in chunks of
//                  8192 (its default buffer size) and adds the chunks' sums in order; within a chunk the sum is pairwise:
//                  blocks of <= 128 elements summed with eight accumulators over stride 8, combined
//                  ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), tail added in order; longer ranges split at n/2 rounded down to a
//                  multiple of 8.  The leaves of those trees are summed by one thread each, then one thread walks the
//                  trees over the leaf sums.
//   lighting       the nine first and second moments as exact integers, the covariance of pixels / 255 as ONE correctly
//                  rounded division per entry ((N * Sab - Sa * Sb) / (N * (N - 1) * 255^2), both sides exact in a double
//                  for N <= 2^18), cyclic Jacobi for the 3 x 3 eigenproblem, eigenvalues ascending, each eigenvector's
//                  sign chosen so that its component of largest magnitude is positive (lowest index on ties).
//   every operation ends in clip to [0, 255], truncation to uint8 and a store: a chain passes bytes between operations.
//
// One workgroup per image runs the image's list of up to four operations with a barrier between them (a 224 x 224 image
// is 150 KB and stays in L2); one launch covers the batch.
#include "../../include/dj_hip.h"
#include "dj_common.h"

#pragma clang fp contract(off)

#define DJ_PHOTO_THREADS 1024
#define DJ_PHOTO_WAVES (DJ_PHOTO_THREADS / 64)
#define DJ_PHOTO_MAX_PIXELS (1 << 18)                         // moments and the covariance stay exact; leaves fit in LDS
#define DJ_PHOTO_MAX_LEAVES (DJ_PHOTO_MAX_PIXELS / 64)        // a leaf of a split range holds at least 64 elements
#define DJ_PHOTO_MAX_SIDE 8192
#define DJ_PHOTO_STACK 24                                     // depth of the pairwise tree: <= 8 for 8192 elements
#define DJ_PHOTO_CHUNK 8192                                   // numpy's reduction buffer: sums of chunks are added in order
#define DJ_PHOTO_LEAF 128                                     // numpy's PW_BLOCKSIZE

__device__ __forceinline__ double photo_grey(const unsigned char* p) {
  return fma((double)p[2], 0.114, fma((double)p[1], 0.587, (double)p[0] * 0.299));
}

__device__ __forceinline__ unsigned char photo_u8(double v) {
  return (unsigned char)(int)fmin(fmax(v, 0.0), 255.0);       // np.clip, then the truncating cast
}

// numpy's pairwise_sum for n <= 128 over the grey values of pixels first .. first + n - 1 (row-major over the image)
__device__ double photo_leaf_sum(const unsigned char* img, long stride, int W, int first, int n) {
  int y = first / W, x = first - y * W;
  const unsigned char* p = img + (long)y * stride + 3L * x;
#define PHOTO_NEXT(dst)            \
  do {                             \
    dst = photo_grey(p);           \
    p += 3;                        \
    if (++x == W) {                \
      x = 0;                       \
      p += stride - 3L * W;        \
    }                              \
  } while (0)
  double v;
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) {
      PHOTO_NEXT(v);
      res += v;
    }
    return res;
  }
  double r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) PHOTO_NEXT(r[k]);
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      PHOTO_NEXT(v);
      r[k] += v;
    }
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) {
    PHOTO_NEXT(v);
    res += v;
  }
#undef PHOTO_NEXT
  return res;
}

// Cyclic Jacobi on the symmetric 3 x 3 matrix a (upper triangle read): eigenvalues ascending in w, eigenvectors in the
// columns of v, signs by the rule above.
__device__ void photo_eigh3(double a[3][3], double w[3], double v[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  a[1][0] = a[0][1];
  a[2][0] = a[0][2];
  a[2][1] = a[1][2];
  for (int sweep = 0; sweep < 30; ++sweep) {
    const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
    if (off == 0.0) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const double g = 100.0 * fabs(apq);          // far below one ulp of both diagonal entries: nothing left to rotate
        if (fabs(a[p][p]) + g == fabs(a[p][p]) && fabs(a[q][q]) + g == fabs(a[q][q])) {
          a[p][q] = a[q][p] = 0.0;
          continue;
        }
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        // the smaller root of t^2 + 2 t theta - 1 = 0; for |theta| past 2^500 theta^2 overflows and t = 1 / (2 theta)
        const double t = fabs(theta) > 1e150 ? 0.5 / theta
                                             : (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        a[p][p] = a[p][p] - t * apq;
        a[q][q] = a[q][q] + t * apq;
        a[p][q] = a[q][p] = 0.0;
        const int r = 3 - p - q;
        const double arp = a[r][p], arq = a[r][q];
        a[r][p] = a[p][r] = c * arp - s * arq;
        a[r][q] = a[q][r] = s * arp + c * arq;
        for (int k = 0; k < 3; ++k) {
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - s * vkq;
          v[k][q] = s * vkp + c * vkq;
        }
      }
  }
  w[0] = a[0][0];
  w[1] = a[1][1];
  w[2] = a[2][2];
  for (int i = 0; i < 2; ++i)          // ascending, columns along
    for (int j = 0; j < 2 - i; ++j)
      if (w[j] > w[j + 1]) {
        const double tw = w[j];
        w[j] = w[j + 1];
        w[j + 1] = tw;
        for (int k = 0; k < 3; ++k) {
          const double tv = v[k][j];
          v[k][j] = v[k][j + 1];
          v[k][j + 1] = tv;
        }
      }
  for (int j = 0; j < 3; ++j) {
    int big = 0;
    for (int k = 1; k < 3; ++k)
      if (fabs(v[k][j]) > fabs(v[big][j])) big = k;
    if (v[big][j] < 0.0)
      for (int k = 0; k < 3; ++k) v[k][j] = -v[k][j];
  }
}

__global__ __launch_bounds__(DJ_PHOTO_THREADS) void dj_photometric_kernel(unsigned char* pixels, int H, int W,
                                                                          long stride,
                                                                          const dj_photometric_ops* __restrict__ ops,
                                                                          double* __restrict__ shift_out) {
  __shared__ double leaf_sum[DJ_PHOTO_MAX_LEAVES];
  __shared__ int leaf_first[DJ_PHOTO_MAX_LEAVES];
  __shared__ int n_leaves;
  __shared__ int st_n[DJ_PHOTO_STACK], st_first[DJ_PHOTO_STACK], st_state[DJ_PHOTO_STACK];
  __shared__ double st_val[DJ_PHOTO_STACK];
  __shared__ long long wave_part[DJ_PHOTO_WAVES][9];
  __shared__ double bcast[3];

  const int tid = threadIdx.x;
  const int N = H * W;
  unsigned char* img = pixels + (long)blockIdx.x * H * stride;
  const dj_photometric_ops* mine = ops + blockIdx.x;
  const int n_ops = min(max(mine->n_ops, 0), DJ_PHOTO_MAX_OPS);      // the host copy was checked; the device copy is only trusted this far
  bool have_leaves = false;
  double last_shift[3] = {0.0, 0.0, 0.0};

  for (int o = 0; o < n_ops; ++o) {
    const int code = mine->code[o];
    const double p0 = mine->param[o][0], p1 = mine->param[o][1], p2 = mine->param[o][2];
    __syncthreads();                   // the bytes the previous operation stored are what this one reads
    if (code == DJ_PHOTO_SATURATION || code == DJ_PHOTO_BRIGHTNESS) {
      const double a = p0, ia = 1.0 - a;
      for (int i = tid; i < N; i += DJ_PHOTO_THREADS) {
        const int y = i / W, x = i - y * W;
        unsigned char* p = img + (long)y * stride + 3L * x;
        const double r = p[0], g = p[1], b = p[2];
        if (code == DJ_PHOTO_SATURATION) {
          const double gs = ia * photo_grey(p);
          p[0] = photo_u8(r * a + gs);
          p[1] = photo_u8(g * a + gs);
          p[2] = photo_u8(b * a + gs);
        } else {
          p[0] = photo_u8(r * a);
          p[1] = photo_u8(g * a);
          p[2] = photo_u8(b * a);
        }
      }
    } else if (code == DJ_PHOTO_CONTRAST) {
      if (!have_leaves) {              // the leaves of numpy's summation tree over N elements, in order
        if (tid == 0) {
          int leaves = 0;
          for (int c0 = 0; c0 < N; c0 += DJ_PHOTO_CHUNK) {
            int sp = 0;
            st_n[0] = min(DJ_PHOTO_CHUNK, N - c0);
            st_first[0] = c0;
            while (sp >= 0) {
              const int n = st_n[sp], first = st_first[sp];
              --sp;
              if (n <= DJ_PHOTO_LEAF) {
                leaf_first[leaves++] = first;
              } else {
                int n2 = n / 2;
                n2 -= n2 % 8;
                st_n[sp + 1] = n - n2;   // the right half waits below the left one
                st_first[sp + 1] = first + n2;
                st_n[sp + 2] = n2;
                st_first[sp + 2] = first;
                sp += 2;
              }
            }
          }
          n_leaves = leaves;
        }
        have_leaves = true;
        __syncthreads();
      }
      const int leaves = n_leaves;
      for (int l = tid; l < leaves; l += DJ_PHOTO_THREADS) {
        const int first = leaf_first[l];
        const int n = (l + 1 < leaves ? leaf_first[l + 1] : N) - first;
        leaf_sum[l] = photo_leaf_sum(img, stride, W, first, n);
      }
      __syncthreads();
      if (tid == 0) {                  // the tree again, now adding: left sum + right sum at every split
        int leaf = 0;
        double total = 0.0;
        for (int c0 = 0; c0 < N; c0 += DJ_PHOTO_CHUNK) {
          int sp = 0;
          double ret = 0.0;
          st_n[0] = min(DJ_PHOTO_CHUNK, N - c0);
          st_state[0] = 0;
          while (sp >= 0) {
            const int n = st_n[sp];
            int n2 = n / 2;
            n2 -= n2 % 8;
            if (st_state[sp] == 0) {
              if (n <= DJ_PHOTO_LEAF) {
                ret = leaf_sum[leaf++];
                --sp;
              } else {
                st_state[sp] = 1;
                st_n[sp + 1] = n2;
                st_state[sp + 1] = 0;
                ++sp;
              }
            } else if (st_state[sp] == 1) {
              st_val[sp] = ret;
              st_state[sp] = 2;
              st_n[sp + 1] = n - n2;
              st_state[sp + 1] = 0;
              ++sp;
            } else {
              ret = st_val[sp] + ret;
              --sp;
            }
          }
          total = total + ret;
        }
        bcast[0] = total / (double)N;
      }
      __syncthreads();
      const double a = p0, m = (1.0 - a) * bcast[0];
      for (int i = tid; i < N; i += DJ_PHOTO_THREADS) {
        const int y = i / W, x = i - y * W;
        unsigned char* p = img + (long)y * stride + 3L * x;
        const double r = p[0], g = p[1], b = p[2];
        p[0] = photo_u8(r * a + m);
        p[1] = photo_u8(g * a + m);
        p[2] = photo_u8(b * a + m);
      }
    } else {                           // DJ_PHOTO_LIGHTING
      unsigned int s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};       // a thread sees <= 256 pixels: 256 * 255^2 < 2^32
      for (int i = tid; i < N; i += DJ_PHOTO_THREADS) {
        const int y = i / W, x = i - y * W;
        const unsigned char* p = img + (long)y * stride + 3L * x;
        const unsigned int r = p[0], g = p[1], b = p[2];
        s[0] += r;
        s[1] += g;
        s[2] += b;
        s[3] += r * r;
        s[4] += r * g;
        s[5] += r * b;
        s[6] += g * g;
        s[7] += g * b;
        s[8] += b * b;
      }
      long long t[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        t[k] = s[k];
        for (int d = 32; d > 0; d >>= 1) t[k] += __shfl_down(t[k], d, 64);
      }
      if ((tid & 63) == 0)
        for (int k = 0; k < 9; ++k) wave_part[tid >> 6][k] = t[k];
      __syncthreads();
      if (tid == 0) {
        long long S[9];
        for (int k = 0; k < 9; ++k) {
          S[k] = 0;
          for (int wv = 0; wv < DJ_PHOTO_WAVES; ++wv) S[k] += wave_part[wv][k];
        }
        double sh[3] = {0.0, 0.0, 0.0};
        if (N > 1) {
          const long long n = N;
          const double den = (double)(n * (n - 1) * 65025LL);
          double cov[3][3], w[3], v[3][3];
          cov[0][0] = (double)(n * S[3] - S[0] * S[0]) / den;
          cov[0][1] = (double)(n * S[4] - S[0] * S[1]) / den;
          cov[0][2] = (double)(n * S[5] - S[0] * S[2]) / den;
          cov[1][1] = (double)(n * S[6] - S[1] * S[1]) / den;
          cov[1][2] = (double)(n * S[7] - S[1] * S[2]) / den;
          cov[2][2] = (double)(n * S[8] - S[2] * S[2]) / den;
          photo_eigh3(cov, w, v);
          const double t0 = w[0] * p0, t1 = w[1] * p1, t2 = w[2] * p2;
          for (int k = 0; k < 3; ++k) sh[k] = ((v[k][0] * t0 + v[k][1] * t1) + v[k][2] * t2) * 255.0;
        }
        bcast[0] = sh[0];
        bcast[1] = sh[1];
        bcast[2] = sh[2];
      }
      __syncthreads();
      const double s0 = bcast[0], s1 = bcast[1], s2 = bcast[2];
      last_shift[0] = s0;
      last_shift[1] = s1;
      last_shift[2] = s2;
      for (int i = tid; i < N; i += DJ_PHOTO_THREADS) {
        const int y = i / W, x = i - y * W;
        unsigned char* p = img + (long)y * stride + 3L * x;
        const double r = p[0], g = p[1], b = p[2];
        p[0] = photo_u8(r + s0);
        p[1] = photo_u8(g + s1);
        p[2] = photo_u8(b + s2);
      }
    }
  }
  if (shift_out && tid == 0) {
    shift_out[3L * blockIdx.x + 0] = last_shift[0];
    shift_out[3L * blockIdx.x + 1] = last_shift[1];
    shift_out[3L * blockIdx.x + 2] = last_shift[2];
  }
}

extern "C" int dj_photometric(unsigned char* pixels, int batch, int height, int width, long stride_bytes,
                              const dj_photometric_ops* ops_dev, const dj_photometric_ops* ops_host, double* shift_out,
                              void* stream) {
  DJ_CHECK_ARG(pixels, "photometric: pixels is null");
  DJ_CHECK_ARG(ops_dev, "photometric: ops_dev is null");
  DJ_CHECK_ARG(ops_host, "photometric: ops_host is null");
  DJ_CHECK_ARG(batch >= 1 && batch <= 65535, "photometric: batch must be in 1..65535 (got %d)", batch);
  DJ_CHECK_ARG(height >= 1 && width >= 1 && height <= DJ_PHOTO_MAX_SIDE && width <= DJ_PHOTO_MAX_SIDE,
               "photometric: size %d x %d outside 1..%d", height, width, DJ_PHOTO_MAX_SIDE);
  DJ_CHECK_ARG((long)height * width <= DJ_PHOTO_MAX_PIXELS, "photometric: %d x %d pixels per image, at most %d are supported",
               height, width, DJ_PHOTO_MAX_PIXELS);
  DJ_CHECK_ARG(stride_bytes >= 3L * width, "photometric: stride_bytes %ld below 3 * width = %ld", stride_bytes, 3L * width);
  for (int i = 0; i < batch; ++i) {
    const dj_photometric_ops* o = ops_host + i;
    DJ_CHECK_ARG(o->n_ops >= 0 && o->n_ops <= DJ_PHOTO_MAX_OPS, "photometric: image %d: %d operations, at most %d are supported", i,
                 o->n_ops, DJ_PHOTO_MAX_OPS);
    for (int k = 0; k < o->n_ops; ++k) {
      DJ_CHECK_ARG(o->code[k] >= DJ_PHOTO_SATURATION && o->code[k] <= DJ_PHOTO_LIGHTING,
                   "photometric: image %d: operation %d has the unknown code %d", i, k, o->code[k]);
      const int n_par = o->code[k] == DJ_PHOTO_LIGHTING ? 3 : 1;
      for (int j = 0; j < n_par; ++j)
        DJ_CHECK_ARG(o->param[k][j] - o->param[k][j] == 0.0, "photometric: image %d: operation %d: parameter %d is not finite", i, k,
                     j);
    }
  }
  hipLaunchKernelGGL(dj_photometric_kernel, dim3((unsigned)batch), dim3(DJ_PHOTO_THREADS), 0, (hipStream_t)stream, pixels,
                     height, width, stride_bytes, ops_dev, shift_out);
  DJ_CHECK_LAUNCH("dj_photometric");
  return DJ_OK;
}
