// The networks' DCT input tensors from JPEG files' own coefficients: a window of each file's raw int16 planes, de-quantised,
// optionally mirrored, scattered into the float32 inputs -- bit for bit what data/coefficient_inputs.py states in numpy.
// What decides bits:
//   * coefficient * table entry in int32, WRAPPED to int16, then converted: the host reader's emission
//     (csrc/dj_jpeg.cpp: Decoder::emit, "jpeg2dct stores shorts");
//   * the mirror is jpegtran's lossless horizontal flip: output block column j reads window column n_cols - 1 - j and the
//     coefficients of odd horizontal frequency change sign, in int16, before the conversion.
//
// A memory-bound scatter, 2 bytes read and 4 written per coefficient, and small (64 windows of 224x224: 29 MB), so it is
// plain C++.  One thread owns one ROW of a block: one 16-byte load of eight coefficients, two 16-byte loads of the table
// row, eight multiply / wrap / convert, two 16-byte stores; the eight threads of a block read its 128 contiguous bytes and
// write its 256.  With that mapping the mirror's sign pattern (columns 1, 3, 5, 7 of the row) is the same for every
// thread and only the source block column changes.  blockIdx.y is the image, blockIdx.x runs over the rows of its
// yh * yw + 2 * ch * cw output blocks; a one-component image writes zeros where its chroma would go, so that every
// element of the (reused) outputs is written.  An output whose pointer or stride rules 16-byte stores out is written
// element by element.
#include "../../include/dj_hip.h"
#include "dj_common.h"

#define DJ_JDI_THREADS 256

struct DjJpegDctParams {
  const unsigned char* coef;
  const dj_jpeg_dct_desc* desc;
  const int* tables;
  float* out[3];
  long ld[3];
  int rows[3], cols[3];      // output block grid per component
  int vec[3];                // 16-byte stores allowed
  int units;                 // block rows per image: 8 * (yh * yw + 2 * ch * cw)
};

__global__ __launch_bounds__(DJ_JDI_THREADS) void dj_jpegdct_kernel(DjJpegDctParams p) {
  const int unit = blockIdx.x * DJ_JDI_THREADS + threadIdx.x;
  if (unit >= p.units) return;
  const dj_jpeg_dct_desc* d = p.desc + blockIdx.y;
  const int row = unit & 7;
  int b = unit >> 3, c = 0;
  const int n_luma = p.rows[0] * p.cols[0], n_chroma = p.rows[1] * p.cols[1];
  if (b >= n_luma) {
    b -= n_luma;
    c = 1;
    if (b >= n_chroma) {
      b -= n_chroma;
      c = 2;
    }
  }
  const int cols = p.cols[c];
  const int r = b / cols, j = b - r * cols;
  float v[8];
  if (c < d->n_components) {
    const int sj = d->flip ? cols - 1 - j : j;
    const unsigned char* src = p.coef + d->coef_offset[c] +
                               (((long)(d->by0[c] + r) * d->blocks_w[c] + (d->bx0[c] + sj)) * 64 + row * 8) * 2;
    const uint4 raw = *reinterpret_cast<const uint4*>(src);                // 16-byte aligned: checked on the host
    const int4* q = reinterpret_cast<const int4*>(p.tables + d->table_offset + c * 64 + row * 8);
    const int4 q0 = q[0], q1 = q[1];
    const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
    const int t[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int s = (short)(w[k >> 1] >> (16 * (k & 1)));
      int x = (short)((unsigned)s * (unsigned)t[k]);                       // the product wraps to int16
      if ((k & 1) && d->flip) x = (short)(-x);                             // -(-32768) stays -32768, as in int16
      v[k] = (float)x;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = 0.0f;
  }
  float* o = p.out[c] + (((long)blockIdx.y * p.rows[c] + r) * cols + j) * p.ld[c] + row * 8;
  if (p.vec[c]) {
    reinterpret_cast<float4*>(o)[0] = make_float4(v[0], v[1], v[2], v[3]);
    reinterpret_cast<float4*>(o)[1] = make_float4(v[4], v[5], v[6], v[7]);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = v[k];
  }
}

extern "C" int dj_jpeg_dct_inputs(const unsigned char* coef, long coef_bytes, const dj_jpeg_dct_desc* desc_dev,
                                  const dj_jpeg_dct_desc* desc_host, int n, const int* tables, long table_ints, int yh, int yw,
                                  int ch, int cw, float* out_y, long ld_y, long y_floats, float* out_cb, long ld_cb,
                                  long cb_floats, float* out_cr, long ld_cr, long cr_floats, void* stream) {
  DJ_CHECK_ARG(coef, "jpeg_dct_inputs: coef is null");
  DJ_CHECK_ARG(desc_dev, "jpeg_dct_inputs: desc_dev is null");
  DJ_CHECK_ARG(desc_host, "jpeg_dct_inputs: desc_host is null");
  DJ_CHECK_ARG(tables, "jpeg_dct_inputs: tables is null");
  DJ_CHECK_ARG(out_y, "jpeg_dct_inputs: out_y is null");
  DJ_CHECK_ARG(out_cb, "jpeg_dct_inputs: out_cb is null");
  DJ_CHECK_ARG(out_cr, "jpeg_dct_inputs: out_cr is null");
  DJ_CHECK_ARG(n >= 1 && n <= 65535, "jpeg_dct_inputs: the number of images must be in 1..65535 (got %d)", n);
  DJ_CHECK_ARG(coef_bytes >= 1 && table_ints >= 1, "jpeg_dct_inputs: coef_bytes / table_ints must be >= 1");
  DJ_CHECK_ARG(((uintptr_t)coef & 15) == 0 && ((uintptr_t)tables & 15) == 0 && ((uintptr_t)desc_dev & 7) == 0,
               "jpeg_dct_inputs: coef and tables must be 16-byte and desc_dev 8-byte aligned");
  DJ_CHECK_ARG(yh >= 1 && yh <= 8192 && yw >= 1 && yw <= 8192 && ch >= 1 && ch <= 8192 && cw >= 1 && cw <= 8192,
               "jpeg_dct_inputs: block grids %d x %d / %d x %d outside 1..8192", yh, yw, ch, cw);
  DjJpegDctParams p;
  p.coef = coef;
  p.desc = desc_dev;
  p.tables = tables;
  float* const outs[3] = {out_y, out_cb, out_cr};
  const long lds[3] = {ld_y, ld_cb, ld_cr}, avail[3] = {y_floats, cb_floats, cr_floats};
  const int rows[3] = {yh, ch, ch}, cols[3] = {yw, cw, cw};
  static const char* const names[3] = {"y", "cb", "cr"};
  for (int c = 0; c < 3; ++c) {
    DJ_CHECK_ARG(((uintptr_t)outs[c] & 3) == 0, "jpeg_dct_inputs: out_%s is not 4-byte aligned", names[c]);
    DJ_CHECK_ARG(lds[c] >= 64 && lds[c] <= (1L << 24), "jpeg_dct_inputs: ld_%s %ld outside 64..2^24", names[c], lds[c]);
    const long blocks = (long)n * rows[c] * cols[c];      // <= 65535 * 2^26
    DJ_CHECK_ARG(avail[c] >= 64 && (blocks - 1) <= (avail[c] - 64) / lds[c],
                 "jpeg_dct_inputs: %ld blocks %ld floats apart leave the %ld floats of out_%s", blocks, lds[c], avail[c],
                 names[c]);
    p.out[c] = outs[c];
    p.ld[c] = lds[c];
    p.rows[c] = rows[c];
    p.cols[c] = cols[c];
    p.vec[c] = ((uintptr_t)outs[c] & 15) == 0 && lds[c] % 4 == 0;
  }
  const long units = 8L * ((long)yh * yw + 2L * ch * cw);
  DJ_CHECK_ARG(units <= 0x7fffffffL - DJ_JDI_THREADS, "jpeg_dct_inputs: block grids too large for one launch");
  p.units = (int)units;
  for (int i = 0; i < n; ++i) {
    const dj_jpeg_dct_desc* d = desc_host + i;
    DJ_CHECK_ARG(d->n_components == 1 || d->n_components == 3, "jpeg_dct_inputs: image %d: %d components, expected 1 or 3", i,
                 d->n_components);
    DJ_CHECK_ARG(d->flip == 0 || d->flip == 1, "jpeg_dct_inputs: image %d: flip %d is neither 0 nor 1", i, d->flip);
    DJ_CHECK_ARG(d->table_offset >= 0 && d->table_offset % 4 == 0 && d->table_offset + 64L * d->n_components <= table_ints,
                 "jpeg_dct_inputs: image %d: tables at %d leave the %ld ints given (or the offset is no multiple of 4)", i,
                 d->table_offset, table_ints);
    for (int c = 0; c < d->n_components; ++c) {
      const int bh = d->blocks_h[c], bw = d->blocks_w[c];
      DJ_CHECK_ARG(bh >= 1 && bh <= 8192 && bw >= 1 && bw <= 8192, "jpeg_dct_inputs: image %d: component %d: block grid %d x %d "
                   "outside 1..8192", i, c, bh, bw);
      const long plane = (long)bh * bw * 128;
      DJ_CHECK_ARG(d->coef_offset[c] >= 0 && d->coef_offset[c] % 16 == 0 && d->coef_offset[c] <= coef_bytes &&
                       plane <= coef_bytes - d->coef_offset[c],
                   "jpeg_dct_inputs: image %d: component %d: %ld coefficient bytes at offset %ld leave the buffer of %ld (or "
                   "the offset is no multiple of 16)", i, c, plane, d->coef_offset[c], coef_bytes);
      DJ_CHECK_ARG(d->by0[c] >= 0 && d->by0[c] <= bh - rows[c] && d->bx0[c] >= 0 && d->bx0[c] <= bw - cols[c],
                   "jpeg_dct_inputs: image %d: component %d: a window of %d x %d blocks from (%d, %d) leaves the grid of %d x %d",
                   i, c, rows[c], cols[c], d->by0[c], d->bx0[c], bh, bw);
    }
  }
  const dim3 grid((unsigned)dj_cdiv(units, DJ_JDI_THREADS), (unsigned)n);
  hipLaunchKernelGGL(dj_jpegdct_kernel, grid, dim3(DJ_JDI_THREADS), 0, (hipStream_t)stream, p);
  DJ_CHECK_LAUNCH("dj_jpeg_dct_inputs");
  return DJ_OK;
}
