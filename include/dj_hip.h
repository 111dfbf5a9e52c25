/* dj_hip.h -- C ABI of the MI355X (gfx950) compute library behind the
 * ResNet50-DCT + SSD300 hot path.
 *
 * The reference (Shulk97/JPEG_detection_Resnet_SSD) has no native boundary of its own:
 * its "operator API" is Keras 2.2.4 layers executed by TensorFlow 1.8 ops.  Each entry
 * point below replaces the TF op(s) that one Keras layer / loss / optimizer launches on
 * the hot path; the citation names the reference call site it stands in for
 * (paths relative to the reference root; L/ = localisation_part/, C/ = classification_part/).
 *
 * Conventions (all entry points):
 *   - tensors are caller-owned DEVICE pointers to float32, activations NHWC, conv
 *     kernels HWIO (the Keras layout), Conv2DTranspose kernels (kh,kw,out,in);
 *   - `ld_*` = floats between consecutive pixels (>= channels: lets a tensor be a
 *     channel slice of a wider concat buffer);
 *   - `stream` is a hipStream_t passed as void*; nothing here allocates or synchronises, so
 *     calls are capturable in a hipGraph;
 *   - state: every launch is a function of its arguments and of THREE library settings, all
 *     safe to read and write from any thread and none of them touched by a compute call:
 *     the arithmetic mode (a process default, dj_set_compute_mode, that a thread overrides
 *     for its own launches with dj_set_thread_compute_mode -- two models of different modes,
 *     or two threads, do not disturb each other), the per-geometry launch overrides of the
 *     autotuner (dj_conv2d_tune_set: a mutex-guarded table keyed by geometry AND arithmetic
 *     mode; an entry only selects among kernels that compute the same result), and the test
 *     switch dj_set_fast_path.  The last error text (dj_last_error) is per thread;
 *   - return 0 on success, <0 on error (message: dj_last_error()); never throws.
 */
#ifndef DJ_HIP_H
#define DJ_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* dj_last_error(void);
/* Version of this interface: bumped whenever an entry point is added or the meaning of an argument changes
 * (2: the `beta` / `relu` bit fields, the workspace and BatchNormalization-backward-statistics entry points, the per-thread
 * arithmetic mode; 3: storage-type codes for 16-bit tensors in HBM, the tuner direction 9; 4: one entry point per
 * convolution GEMM, taking an argument struct; their `_ws` / `_addrelu` / `_bn` / `_bnbwd` / `_relumask` / `_t` forms are gone;
 * 5: `dj_conv_fwd_args.bn` and `dj_bn_train` are gone).  A binding
 * written for one version must refuse a library that reports another (jpeg_detection_resnet_ssd_amd/_lib.py does). */
#define DJ_ABI_VERSION 5
int dj_abi_version(void);

/* Storage type of a tensor in HBM, passed next to each ACTIVATION / GRADIENT tensor: the `dt_*` fields of the convolution
 * argument structs, and the `dt_*` arguments of the elementwise entry points whose name ends in `_t`.
 * Everything is fp32 unless such a code says otherwise (BASELINE config 5, "fp16-input / fp32-accumulate": under
 * K.set_floatx('float16') the backbone's conv outputs and block sums are held as fp16, their gradients as bf16 -- the
 * exponent range gradients need --; weights, their gradients, the optimizer state, BatchNormalization statistics and all
 * arithmetic outside the MFMA operands stay fp32).  `ld_*` are in ELEMENTS of the tensor they describe.
 * In the three convolution GEMMs 16-bit tensors exist in arithmetic mode 1 only; a 16-bit operand needs the branch-free
 * kernel's preconditions (channel counts that are multiples of 32, 16-byte aligned bases, stride-1 or 1x1 input gradients)
 * and is an error otherwise -- never a silent conversion pass.  A 16-bit RESULT is written by one K range: such a launch is
 * never split over workgroups, whatever the tuner registered. */
#define DJ_F32 0
#define DJ_F16 1
#define DJ_BF16 2

/* Geometry of one keras.layers.Conv2D (third-party; used at
 * L/models/keras_ssd300_dct_j2d_resnet.py:77-96,128-160,483-545,562-675).  TF 'same'
 * padding is resolved by the caller into pad_top/pad_left (asymmetric for even kernels). */
typedef struct dj_conv2d_desc {
  int batch;
  int in_h, in_w, in_c;
  int out_h, out_w, out_c;
  int kernel_h, kernel_w;
  int stride_h, stride_w;
  int dilation_h, dilation_w;
  int pad_top, pad_left;
  int ld_x; /* pixel stride of x / dx */
  int ld_y; /* pixel stride of y / dy */
} dj_conv2d_desc;

/* Leading dimension of the `stats` partial buffer ([rows][2][out_c] floats): one row per 64 output
 * pixels, independent of the tile configuration. */
int dj_conv2d_fwd_stats_rows(const dj_conv2d_desc* d);

/* y = act(conv(pro(x), w) + bias).  Replaces Conv2D.call (TF conv2d + bias_add [+ relu]).  One entry point; an all-zero
 * dj_conv_fwd_args means fp32 tensors and no option, and an option is selected by its pointer.
 * Keras call sites: L/models/keras_ssd300_dct_j2d_resnet.py:77-99,128-163. */
#define DJ_CONV_RELU 1            /* fused ReLU epilogue */
#define DJ_CONV_Y_ZEROED 2        /* y is all zeros on entry: a split-K launch (atomic accumulation) does not clear it first */
#define DJ_CONV_STATS_MAY_SPLIT 4 /* with `workspace`: a launch with `stats` is tuned like one without and may be split (its
                                   * statistics then come from the reduction); otherwise a launch with `stats` is never split */
typedef struct dj_conv_fwd_args {
  /* operands: x fp32 | fp16; w the fp32 master weights or their fp16 shadow (dj_shadow_weights); y fp32 | fp16 (rounded
   * AFTER the fp32 bias / ReLU / statistics epilogue) */
  const void* x;
  int dt_x;
  const void* w;
  int dt_w;
  const float* bias; /* optional */
  void* y;
  int dt_y;
  /* pro_scale / pro_shift ([in_c], optional, together): x is read as x*scale+shift (then ReLU if pro_relu) on in-bounds
   * pixels only -- the BatchNormalization+Activation that Keras runs between two convs (L/models/...resnet.py:80-81,90-91)
   * folded into the load */
  const float* pro_scale;
  const float* pro_shift;
  int pro_relu;
  int flags; /* DJ_CONV_RELU | DJ_CONV_Y_ZEROED | DJ_CONV_STATS_MAY_SPLIT */
  /* optional, [dj_conv2d_fwd_stats_rows(d)][2][out_c]: per-row-tile column sums / sums of squares of conv(x,w) WITHOUT
   * bias, consumed by dj_bn_train_finalize (training-mode BatchNormalization statistics) */
  float* stats;
  /* res != NULL: residual Add + ReLU evaluated inside the consumer (the first 1x1 conv of the next bottleneck block,
   * L/models/keras_ssd300_dct_j2d_resnet.py:96-99 then :66-68): the conv's input is
   *   a[m][c] = relu(x[m][c]*pro_scale[c] + pro_shift[c] + res[m][c]*res_scale[c] + res_shift[c])
   * (res_scale/res_shift NULL: res taken as is -- an identity shortcut; pro_scale/pro_shift are required and pro_relu is
   * taken as 1; res has x's storage type), computed while the A tile is staged; when sum_out != NULL (fp32 | fp16,
   * dt_sum) the tensor `a` -- the output of Add()+Activation('relu') that later layers and the backward pass read -- is
   * stored there by the same launch.  Only for 1x1, stride-1, unpadded convs with in_c % 32 == 0
   * (dj_conv2d_fwd_addrelu_supported() != 0); any other geometry is an error, never a silent slow path. */
  const void* res;
  int ld_res;
  const float* res_scale;
  const float* res_shift;
  void* sum_out;
  int ld_sum;
  int dt_sum;
  /* workspace != NULL: a caller-owned workspace (the reference's TF convolution is bit-reproducible in the forward pass,
   * L/models/keras_ssd300_dct_j2d_resnet.py:481-675 are the small-map layers this matters for): when the tuned launch
   * splits its reduction over workgroups and workspace_floats >= dj_conv2d_fwd_workspace_floats(d, ...), the K chunks
   * store their partial tiles to the workspace and a second kernel adds them in a fixed order, adds the bias, applies
   * ReLU and -- if `stats` is given -- takes the BatchNormalization statistics of the sum; without (enough) workspace a
   * split launch accumulates with fp32 atomics in arrival order. */
  float* workspace;
  long workspace_floats;
} dj_conv_fwd_args;
int dj_conv2d_nhwc_fwd(const dj_conv2d_desc* d, const dj_conv_fwd_args* a, void* stream);
/* floats of workspace that make the CURRENT tuning choice for this geometry run without atomics (0: not split; < 0: bad
 * descriptor) */
long dj_conv2d_fwd_workspace_floats(const dj_conv2d_desc* d, int may_split_stats);
int dj_conv2d_fwd_addrelu_supported(const dj_conv2d_desc* d);

/* dx (+)= conv_transpose(dy, w) [+ bias].  Gradient of Conv2D w.r.t. its input (TF
 * Conv2DBackpropInput); with `bias` it is also the forward of keras.layers.Conv2DTranspose
 * (L/models/...resnet.py:1709-1711), whose (kh,kw,out,in) kernel is the HWIO kernel of
 * the convolution it transposes.  An all-zero dj_conv_dgrad_args means fp32 tensors and no option. */
#define DJ_DGRAD_NO_SPLIT 2
typedef struct dj_conv_dgrad_args {
  /* operands: dy fp32 | bf16; w the fp32 master weights or their bf16 shadow (dj_shadow_weights); dx any type (bf16 for
   * the gradient of a fp16 activation; accumulates in that type when flags & 1) */
  const void* dy;
  int dt_dy;
  const void* w;
  int dt_w;
  const float* bias; /* optional */
  void* dx;
  int dt_dx;
  /* bit 0 = accumulate into dx; DJ_DGRAD_NO_SPLIT = never split the reduction over workgroups (a split launch adds with
   * fp32 atomics in arrival order; the forward use as Conv2DTranspose sets it so that the forward pass stays
   * bit-reproducible) */
  int flags;
  /* partial != NULL: the BatchNormalization BACKWARD statistics of the tensor this launch produces.  dx is then
   * g = dL/d relu(bn(z)) for the BatchNormalization layer whose ONLY consumer is this convolution
   * (L/models/keras_ssd300_dct_j2d_resnet.py:77-96: conv -> BatchNormalization -> Activation('relu') -> conv inside the
   * bottleneck blocks); z [batch*in_h*in_w][ld_z] (fp32 | fp16, required) is that layer's input, mean / invstd (required)
   * its saved batch statistics, scale / shift its affine (both NULL: no ReLU behind it, nothing is masked).  Besides
   * storing dx the epilogue writes
   *   partial[r][0][c] = sum g_m,   partial[r][1][c] = sum g_m * (z - mean[c]) * invstd[c],   g_m = g where z*scale+shift > 0
   * over rows 64 r .. 64 r + 63, partial = [ceil(batch*in_h*in_w / 64)][2][in_c]: what dj_bn_bwd_reduce(mask_mode 2 / 0)
   * computes in a pass of its own over g and z, in the layout dj_bn_bwd_finalize reads.  One K range per tile; `bias` and
   * the accumulate bit are errors; not for strided 1x1 convolutions (their dx is scattered). */
  const void* z;
  int ld_z;
  int dt_z;
  const float* mean;
  const float* invstd;
  const float* scale;
  const float* shift;
  float* partial;
  /* mask_x != NULL: the epilogue also applies the ReLU mask of the tensor it differentiates:
   *   dx[m][c] = mask_x[m][c] > 0 ? conv_transpose(dy, w)[m][c] (+ bias[c]) (+ dx[m][c] when flags & 1) : 0
   * mask_x [batch*in_h*in_w][ld_mask] is the convolution's own forward input x = relu(Add(...)) -- the output of a
   * residual block (L/models/keras_ssd300_dct_j2d_resnet.py:96-99).  When this launch is the LAST writer of that block's
   * output gradient, the gradient is masked once, where it is completed: the BatchNormalization backward passes of the
   * block read it unmasked-mode (mask_mode 0, no read of x) and an identity shortcut shares the buffer.  Exactly the
   * values of a plain launch followed by dj_relu_bwd in place.  One K range per tile: DJ_ERR_ARG when the tuning entry of
   * direction 1 registers a split reduction, for the strided 1x1 scatter form, in the 16-bit arithmetic modes (fp32
   * tensors only) and together with `partial`; dj_conv2d_dgrad_relumask_supported() != 0 says beforehand that none of
   * the first three applies.  Takes the tile variant of direction 1's tuning entry; geometries outside the branch-free
   * kernels' preconditions run the generic kernel. */
  const float* mask_x;
  int ld_mask;
} dj_conv_dgrad_args;
int dj_conv2d_nhwc_dgrad(const dj_conv2d_desc* d, const dj_conv_dgrad_args* a, void* stream);
int dj_conv2d_dgrad_relumask_supported(const dj_conv2d_desc* d);

/* Debug/test switch: 0 forces the generic (branchy, any-shape) implicit-GEMM kernel, 1 (default) lets the
 * launcher pick the branch-free buffer-load kernel whenever its alignment preconditions hold. */
void dj_set_fast_path(int enable);

/* Debug/test switch: 0 sends the convolutions with taps, padding, stride or dilation -- of both branch-free kernel
 * families, fp32 MFMA and split-bf16 (float32x3 / float32x6) -- to the kernels that redo their gather arithmetic every
 * K-step, 1 (default) lets the launcher pick the variants that cache per-tap row offsets (forward, input gradient) or
 * walk the pixel incrementally (weight gradient).  The twins sum the same products in the same order: their results are
 * bit-equal.  The bounds-free variant of the unpadded 1x1 convolutions is not behind this switch. */
void dj_set_gather_variants(int enable);

/* Arithmetic of the implicit-GEMM kernels: 0 = fp32 (default; what every parity claim at 1e-3 refers to): fp32 tensors,
 * fp32 results, from whichever of two kernel families the tuning table names for a geometry -- v_mfma_f32_32x32x2_f32, or
 * the split-bf16 kernels of mode 4 (measured against the fp64 oracle the two are equally far from it, 1.4e-7 .. 4.6e-7
 * rel-L2 per GEMM; configuration indices [N, 2N) of dj_conv2d_tune_set select the latter);
 * 5 = fp32 MFMA instructions only (indices [0, N); the behaviour of mode 0 before round 3's split kernels);
 * 4 ("float32x6") = every product as six bf16 MFMAs on operands split into three bf16 pieces when they go to LDS
 * (hi*hi + hi*mid + mid*hi + hi*lo + mid*mid + lo*hi; dropped: 2^-24 of a product), fp32 accumulation: fp32 results at
 * 6/16 of the fp32 MFMA's matrix-pipe time; 3 ("float32x3") = two pieces, three MFMAs: ~4e-6 rel-L2 per GEMM;
 * (BASELINE config 5, "fp16 MFMA":) 1 = forward GEMMs round both operands to fp16 and gradient GEMMs (dgrad, wgrad,
 * Conv2DTranspose forward) to bf16 as the fragments leave LDS, v_mfma_f32_32x32x8_{f16,bf16} with fp32 accumulation;
 * 2 = bf16 in every GEMM.  Tensors in HBM (activations, weights = the fp32 master copy, gradients, optimizer state)
 * stay fp32 in every mode.  Sets the process-wide default; returns the previous default. */
int dj_set_compute_mode(int mode);
/* Override for the calling thread's launches (-1: follow the process default); returns the previous override.
 * dj_get_compute_mode reports the mode the calling thread's next launch would use. */
int dj_set_thread_compute_mode(int mode);
int dj_get_compute_mode(void);

/* Launch-configuration overrides per conv geometry, filled by the plan-time autotuner: `dir` 0 fwd, 1 dgrad,
 * 2 wgrad (+4: forward that takes BN statistics; 9: the input gradient that takes BN backward statistics (`partial`), which runs other
 * kernels than a plain input gradient and is never split -- without an entry of its own it takes the tile shape of the
 * dir-1 entry); cfg in [0, dj_conv2d_tune_configs()) selects the tile shape
 * (128x128, 128x64, 64x64, 128x32) and schedule variant -- in mode 0 the count is twice that of the other modes, the upper
 * half naming the split-bf16 (float32x6) variants --, `splits` the split-K factor; cfg < 0 removes the override. */
int dj_conv2d_tune_configs(void);
int dj_conv2d_tune_set(int dir, const dj_conv2d_desc* d, int cfg, int splits);
int dj_conv2d_default_config(int dir, const dj_conv2d_desc* d, int* cfg, int* splits);

/* dw = sum over pixels pro(x)^T dy  (TF Conv2DBackpropFilter).  dw is HWIO, overwritten: always the fp32 gradient of the
 * master weights.  The pixel reduction is split over workgroups that accumulate with fp32 atomics. */
typedef struct dj_conv_wgrad_args {
  const void* x;  /* fp32 | fp16 */
  int dt_x;
  const void* dy; /* fp32 | bf16 */
  int dt_dy;
  float* dw;
  const float* pro_scale; /* as in dj_conv_fwd_args */
  const float* pro_shift;
  int pro_relu;
  int dw_zeroed; /* 1 promises dw already holds zeros (the engine clears its whole flat gradient buffer once per step
                  * instead of one memset per layer) */
} dj_conv_wgrad_args;
int dj_conv2d_nhwc_wgrad(const dj_conv2d_desc* d, const dj_conv_wgrad_args* a, void* stream);

/* `w` of the forward and input-gradient GEMMs: the fp32 master weights, or their 16-bit shadow in the type the GEMM
 * multiplies in (fp16 forward, bf16 input gradient), refreshed once per step by dj_shadow_weights: w16[i] = fp16(w[i]) and /
 * or wbf[i] = bf16(w[i]) for i < n (n a multiple of 4; either output may be NULL). */
int dj_shadow_weights(const float* w, void* w16, void* wbf, long n, void* stream);

/* ---- blocked column reductions (two-stage, deterministic) ------------------------- */
/* Rows of the `partial` buffers written by the *_partial / *_reduce entry points for a
 * [rows][C] operand: partial is [dj_reduce_rows(rows)][2][C] floats. */
int dj_reduce_rows(long rows);
/* partial[blk][0][c] = sum x, partial[blk][1][c] = sum x^2 over the block's rows.  Batch statistics of
 * a BatchNormalization whose input is not a conv output (input BNs, L/models/...resnet.py:446,458,1716). */
int dj_colstats_partial(const float* x, long rows, int C, int ld, float* partial, void* stream);
/* partial[blk][0][c] = sum dy (bias gradient of Conv2D / Dense: TF BiasAddGrad). */
int dj_colsum_partial(const float* dy, long rows, int C, int ld, float* partial, void* stream);
/* out[c] (+)= sum_blk partial[blk][which][c] (accumulated in double). */
int dj_colreduce_finalize(const float* partial, int nrows, int C, int which, float* out, int beta, void* stream);
/* out[c] (+)= sum over rows of x[r][c] in one launch -- bias gradients (BiasAddGrad) of the SSD head convs, whose
 * gradient tensors have at most a few thousand rows. */
int dj_colsum_direct(const float* x, long rows, int C, int ld, float* out, int beta, void* stream);
/* dj_colsum_direct for up to DJ_COLSUM_PARTS tensors in one launch (the bias gradients of the SSD head convolutions,
 * deferred to the end of the backward pass). */
#define DJ_COLSUM_PARTS 32
typedef struct dj_colsum_part {
  const float* x;
  float* out;
  long rows;
  int C, ld, beta;
} dj_colsum_part;
int dj_colsum_multi(const dj_colsum_part* parts, int n_parts, void* stream);

/* ---- keras.layers.BatchNormalization(axis=3) (Keras 2.2.4 defaults eps 1e-3, momentum 0.99) ----
 * Training forward = statistics (conv epilogue `stats` or dj_colstats_partial) -> dj_bn_train_finalize
 * -> (scale, shift); the normalisation itself is applied by the consumer (conv prologue or
 * dj_affine_act).  `conv_bias` (optional) is the bias the producing conv added AFTER its statistics
 * were taken.  moving_* (optional) are updated in place (variance Bessel-corrected, as
 * tf.nn.fused_batch_norm reports it). */
int dj_bn_train_finalize(const float* partial, int nrows, long count, const float* conv_bias, const float* gamma,
                         const float* beta, float eps, float momentum, float* moving_mean, float* moving_var,
                         float* scale, float* shift, float* save_mean, float* save_invstd, int C, void* stream);
/* Inference mode: scale = gamma*rsqrt(moving_var+eps), shift = beta - moving_mean*scale. */
int dj_bn_infer_coeffs(const float* gamma, const float* beta, const float* moving_mean, const float* moving_var,
                       float eps, float* scale, float* shift, int C, void* stream);
/* y = act(x*scale+shift [+ res*res_scale+res_shift]) -- BatchNormalization apply, Activation('relu'),
 * Add()+Activation('relu') (L/models/...resnet.py:96-99,160-163) in one pass.  Null scale = identity. */
int dj_affine_act(const float* x, int ldx, const float* scale, const float* shift, const float* res, int ldres,
                  const float* res_scale, const float* res_shift, float* y, int ldy, long rows, int C, int relu,
                  void* stream);
/* Backward of BN(+ReLU): dy is masked by the ReLU (mask_mode 0 none, 1: y > 0 with y the materialised
 * ReLU output, 2: z*scale+shift > 0), partial[blk] = (sum dy_m, sum dy_m*xhat). */
int dj_bn_bwd_reduce(const float* dy, int ld_dy, const float* z, int ld_z, const float* y, int ld_y,
                     const float* mean, const float* invstd, const float* scale, const float* shift, int mask_mode,
                     long rows, int C, float* partial, void* stream);
/* dgamma, dbeta and k0,k1,k2 with dz = k0*dy_m + k1*z + k2. */
int dj_bn_bwd_finalize(const float* partial, int nrows, long count, const float* gamma, const float* mean,
                       const float* invstd, float* dgamma, float* dbeta, float* k0, float* k1, float* k2, int C,
                       void* stream);
int dj_bn_bwd_apply(const float* dy, int ld_dy, const float* z, int ld_z, const float* y, int ld_y,
                    const float* scale, const float* shift, int mask_mode, const float* k0, const float* k1,
                    const float* k2, float* dz, int ld_dz, long rows, int C, float* dmasked, int ld_dm, int dm_beta,
                    void* stream);
/* ... optional second output of dj_bn_bwd_apply: dmasked[r][c] (+)= dy_m, the ReLU-masked upstream gradient itself --
 * after Add()+Activation('relu') that is the identity shortcut's gradient, written in the same pass (no dj_relu_bwd). */
/* dx (+)= dy * [y > 0]  (Activation('relu') gradient; `activation="relu"` convs of the SSD head). */
int dj_relu_bwd(const float* dy, int ld_dy, const float* y, int ld_y, float* dx, int ld_dx, long rows, int C,
                int beta, void* stream);
/* dst[r][c] (+)= src[r][c]: Concatenate / Reshape+Concatenate(axis=1) and their gradients
 * (L/models/...resnet.py:461,836-879,1713-1714). */
int dj_copy2d(const float* src, long ld_src, float* dst, long ld_dst, long rows, long cols, int beta, void* stream);
/* The same for up to DJ_COPY_PARTS (src, dst) pairs in one launch: Concatenate(axis=1) over the six SSD sources and its
 * gradient (L/models/keras_ssd300_dct_j2d_resnet.py:825-879). */
#define DJ_COPY_PARTS 8
typedef struct dj_copy_part {
  const float* src;
  float* dst;
  long ld_src, ld_dst, rows, cols;
  int beta; /* 1: dst += src */
} dj_copy_part;
int dj_copy2d_multi(const dj_copy_part* parts, int n_parts, void* stream);
/* The elementwise passes above over tensors that carry their storage type (each tensor pointer is followed by its DJ_F32 /
 * DJ_F16 / DJ_BF16 code; any mix; arithmetic in fp32, one rounding where a 16-bit tensor is written).  Same Keras call
 * sites: BatchNormalization / Activation / Add at L/models/keras_ssd300_dct_j2d_resnet.py:80-99,135-163. */
int dj_affine_act_t(const void* x, int dt_x, int ldx, const float* scale, const float* shift, const void* res, int dt_res,
                    int ldres, const float* res_scale, const float* res_shift, void* y, int dt_y, int ldy, long rows, int C,
                    int relu, void* stream);
int dj_bn_bwd_reduce_t(const void* dy, int dt_dy, int ld_dy, const void* z, int dt_z, int ld_z, const void* y, int dt_y,
                       int ld_y, const float* mean, const float* invstd, const float* scale, const float* shift,
                       int mask_mode, long rows, int C, float* partial, void* stream);
int dj_bn_bwd_apply_t(const void* dy, int dt_dy, int ld_dy, const void* z, int dt_z, int ld_z, const void* y, int dt_y,
                      int ld_y, const float* scale, const float* shift, int mask_mode, const float* k0, const float* k1,
                      const float* k2, void* dz, int dt_dz, int ld_dz, long rows, int C, void* dmasked, int dt_dm, int ld_dm,
                      int dm_beta, void* stream);
int dj_relu_bwd_t(const void* dy, int dt_dy, int ld_dy, const void* y, int dt_y, int ld_y, void* dx, int dt_dx, int ld_dx,
                  long rows, int C, int beta, void* stream);
/* dst (+)= src with a change of storage type on the way: a 16-bit backbone tensor handed to a layer that works on fp32
 * (L2Normalization, pooling, Concatenate), and the gradient coming back. */
int dj_copy2d_t(const void* src, int dt_src, long ld_src, void* dst, int dt_dst, long ld_dst, long rows, long cols, int beta,
                void* stream);
/* UpSampling2D() nearest x2 (L/models/...resnet.py:1669) written into a channel slice. */
int dj_upsample2x(const float* x, int ldx, float* y, int ldy, int B, int H, int W, int C, void* stream);

/* ---- L2Normalization (L/keras_layers/keras_layer_L2Normalization.py:61-63) ---- */
int dj_l2norm_fwd(const float* x, int ldx, const float* gamma, float* y, int ldy, float* rnorm, long rows, int C,
                  void* stream);
/* dx (optional, (+)=) and dgamma_partial (optional, [dj_reduce_rows(rows)][2][C], slot 0). */
int dj_l2norm_bwd(const float* dy, int ld_dy, const float* x, int ldx, const float* gamma, const float* rnorm,
                  float* dx, int ld_dx, float* dgamma_partial, long rows, int C, int beta, void* stream);

/* ---- keras.layers.MaxPooling2D: `pool5_ssd` (3,3)/1/'same' (L/models/...resnet.py:481,1110) and the ResNet50RGB
 * stem ZeroPadding2D(1) + (3,3)/2 (C/vgg_jpeg_keras/networks/resnet_dct.py:165-314).  pt/pl = leading pads;
 * pad_zero = 1 when the padding comes from a ZeroPadding2D (zeros take part in the max), 0 for TF 'same'/'valid'.
 * The gradient goes to the first maximum of each window in row-major order.  `argmax` (optional, B*OH*OW*C bytes):
 * forward stores each window's winning tap there and backward reads it instead of rescanning the windows
 * (then `x` may be NULL in backward). ---- */
int dj_maxpool2d_fwd(const float* x, float* y, int B, int H, int W, int C, int OH, int OW, int kh, int kw, int sh,
                     int sw, int pt, int pl, int pad_zero, unsigned char* argmax, void* stream);
int dj_maxpool2d_bwd(const float* x, const float* dy, float* dx, int B, int H, int W, int C, int OH, int OW, int kh,
                     int kw, int sh, int sw, int pt, int pl, int pad_zero, int beta, const unsigned char* argmax,
                     void* stream);

/* ---- Activation('softmax') on the last axis (L/models/...resnet.py:873; Dense(..., softmax)) ---- */
int dj_softmax_fwd(const float* x, float* y, long rows, int C, void* stream);
int dj_softmax_bwd(const float* p, const float* dp, long ld_dp, float* dx, long rows, int C, int beta, void* stream);

/* ---- SSDLoss.compute_loss (L/keras_loss_function/keras_ssd_loss.py:98-211) ----
 * y_true / y_pred: [nbox][n_cls+12] with nbox = batch * boxes-per-image; mining is batch-wide.
 * out5 = {loss (already the Keras batch mean), n_positive, n_negative_kept, class part, loc part}. */
long dj_ssd_loss_workspace_floats(long nbox);
int dj_ssd_loss_fwd(const float* y_true, const float* y_pred, long nbox, int n_cls, int neg_pos_ratio, int n_neg_min,
                    float alpha, float* workspace, float* out5, void* stream);
int dj_ssd_loss_bwd(const float* y_true, const float* y_pred, long nbox, int n_cls, float alpha, float upstream,
                    const float* workspace, const float* out5, float* d_pred, void* stream);

/* ---- keras.losses.categorical_crossentropy on probabilities (C/config/resnet/config_file.py:64) ---- */
int dj_categorical_crossentropy(const float* y_true, const float* probs, long rows, int C, float upstream,
                                float* loss_rows, float* d_probs, float* out_mean, void* stream);

/* ---- keras.optimizers.SGD.get_updates (L/training_dct_pascal_j2d_resnet.py:152; C/config/resnet/config_file.py:58-63),
 * Adam.get_updates and Adadelta.get_updates (Keras 2.2.4; L/evaluation.py:102, L/inference.py:104 build
 * Adam(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-08, decay=0.0); C/template_keras/config/template_config.py imports
 * Adadelta), each with the l2 kernel_regularizer gradient (2*l2*p) and the data-parallel 1/world_size folded in.
 * keras/optimizers.py states the three in numpy (sgd_host, adam_host, adadelta_host); the entry points equal that
 * statement bit for bit: fp32 throughout, every operation rounded once in the order written, and no fma but the two that
 * the SGD statement writes.
 * dj_sgd_momentum_update:  g' = fma(g, grad_scale, (l2 + l2) * p);   v = momentum * v - lr_t * g'
 *                      p = nesterov ? fma(momentum, v, p) - lr_t * g' : p + v
 *   with lr_t = lr / (1 + decay * iterations) computed by the caller.
 * Adam and Adadelta round both products of their effective gradient:
 *     g' = g * grad_scale + (2 * l2) * p
 * dj_adam_update:      m = beta_1 * m + (1 - beta_1) * g';   v = beta_2 * v + (1 - beta_2) * (g' * g')
 *                      vhat != NULL (amsgrad): vhat = max(vhat, v), a NaN on either side giving NaN, and d = vhat; else d = v
 *                      p = p - (lr_t * m) / (sqrt(d) + epsilon)
 *   with 1 - beta in fp32 and lr_t = lr / (1 + decay * iterations) * sqrt(1 - beta_2^t) / (1 - beta_1^t), t = iterations + 1,
 *   computed by the caller (Adam.step_size()).
 * dj_adadelta_update:  a = rho * a + one_minus_rho * (g' * g');   u = (g' * sqrt(d + epsilon)) / sqrt(a + epsilon)
 *                      p = p - lr * u;   d = rho * d + one_minus_rho * (u * u)
 *   with lr = lr / (1 + decay * iterations) and one_minus_rho = (float)(1.0 - rho), subtracted in double as Keras does with
 *   its Python float, both computed by the caller.
 * RMSprop, Adagrad, Adamax and Nadam (Keras 2.2.4 get_updates; rmsprop_host, adagrad_host, adamax_host, nadam_host) on
 * the same g'; lr below is lr / (1 + decay * iterations), t = iterations + 1, 1 - rho and 1 - beta are subtracted in fp32:
 * dj_rmsprop_update:   a = rho * a + (1 - rho) * (g' * g');   p = p - (lr * g') / (sqrt(a) + epsilon)
 * dj_adagrad_update:   a = a + g' * g';                       p = p - (lr * g') / (sqrt(a) + epsilon)
 * dj_adamax_update:    m = beta_1 * m + (1 - beta_1) * g';    u = max(beta_2 * u, |g'|), a NaN on either side giving NaN
 *                      p = p - (lr_t * m) / (u + epsilon)     with lr_t = lr / (1 - beta_1^t) (Adamax.step_size())
 * dj_nadam_update:     m and v as Adam's;   mbar = one_minus_mc_t * (g' * c_g) + mc_t1 * (m * c_m)
 *                      p = p - (lr * mbar) / (sqrt(v * c_v) + epsilon)
 *   with mc(i) = beta_1 * (1 - 0.5 * 0.96^(i * schedule_decay)), S = mc(1) * ... * mc(t), c_g = 1 / (1 - S),
 *   c_m = 1 / (1 - S * mc(t + 1)), c_v = 1 / (1 - beta_2^t), one_minus_mc_t = 1 - mc(t), mc_t1 = mc(t + 1), computed in
 *   double by the caller (Nadam.step_scalars()): products with reciprocals where Keras divides.
 * All of them.  sumsq != NULL: sumsq[0] += sum(p^2) before the update, in one fp32 addition.  One thread per four
 * consecutive elements in a grid-stride loop of at most dj_optim_groups_per_pass() threads; 16-byte accesses when every
 * pointer is 16-byte aligned, element by element otherwise.  DJ_ERR_ARG for a null pointer (vhat and sumsq excepted),
 * n <= 0, or buffers that overlap. ---- */
long dj_optim_groups_per_pass(void);
int dj_sgd_momentum_update(float* param, const float* grad, float* velocity, long n, float lr_t, float momentum,
                           int nesterov, float l2, float grad_scale, float* sumsq /* may be NULL */, void* stream);
int dj_adam_update(float* param, const float* grad, float* m, float* v, float* vhat /* NULL: no amsgrad */, long n,
                   float lr_t, float beta_1, float beta_2, float epsilon, float l2, float grad_scale,
                   float* sumsq /* may be NULL */, void* stream);
int dj_adadelta_update(float* param, const float* grad, float* accum, float* delta_accum, long n, float lr, float rho,
                       float one_minus_rho, float epsilon, float l2, float grad_scale, float* sumsq /* may be NULL */,
                       void* stream);
int dj_rmsprop_update(float* param, const float* grad, float* accum, long n, float lr, float rho, float epsilon, float l2,
                      float grad_scale, float* sumsq /* may be NULL */, void* stream);
int dj_adagrad_update(float* param, const float* grad, float* accum, long n, float lr, float epsilon, float l2,
                      float grad_scale, float* sumsq /* may be NULL */, void* stream);
int dj_adamax_update(float* param, const float* grad, float* m, float* u, long n, float lr_t, float beta_1, float beta_2,
                     float epsilon, float l2, float grad_scale, float* sumsq /* may be NULL */, void* stream);
int dj_nadam_update(float* param, const float* grad, float* m, float* v, long n, float lr, float beta_1, float beta_2,
                    float epsilon, float c_g, float c_m, float c_v, float one_minus_mc_t, float mc_t1, float l2,
                    float grad_scale, float* sumsq /* may be NULL */, void* stream);

/* ---- DecodeDetections (L/keras_layers/keras_layer_DecodeDetections.py:109-265; numpy twin
 * L/ssd_encoder_decoder/ssd_output_decoder.py:111-226): y_pred [batch][n_boxes][n_classes+12] (centroid offsets, anchors,
 * variances in the last 12 columns) -> out [batch][top_k][6] = (class, confidence, xmin, ymin, xmax, ymax) sorted by
 * confidence, zero padded.  Per class: confidence > thresh, greedy NMS (drop IoU > iou_threshold), at most
 * nms_max_output_size.  Limits: n_boxes <= 12288, (n_classes-1)*nms_max_output_size <= 8192. ---- */
long dj_decode_detections_workspace_floats(int batch, int n_boxes, int n_classes, int nms_max_output_size);
int dj_decode_detections(const float* y_pred, int batch, int n_boxes, int n_classes, float confidence_thresh,
                         float iou_threshold, int top_k, int nms_max_output_size, int normalize_coords, int img_height,
                         int img_width, float* workspace, float* out, void* stream);

/* ---- DecodeDetectionsFast (L/keras_layers/keras_layer_DecodeDetectionsFast.py:108-215, mode='inference_fast'): each box
 * keeps its arg-max class and that confidence, background boxes are dropped, threshold, ONE class-agnostic greedy NMS
 * (at most nms_max_output_size <= 8192), top-k.  Same tensors and output layout as dj_decode_detections. ---- */
long dj_decode_detections_fast_workspace_floats(int batch, int n_boxes, int nms_max_output_size);
int dj_decode_detections_fast(const float* y_pred, int batch, int n_boxes, int n_classes, float confidence_thresh,
                              float iou_threshold, int top_k, int nms_max_output_size, int normalize_coords,
                              int img_height, int img_width, float* workspace, float* out, void* stream);

/* ---- SSDInputEncoder.__call__ for coords='centroids' (L/ssd_encoder_decoder/ssd_input_encoder.py:277-418,
 * matching_utils.py:22-116, L/bounding_box_utils/bounding_box_utils.py:283-383): labels [batch][max_gt][5] =
 * (class id, xmin, ymin, xmax, ymax) in pixels (float64, as the reference computes), n_gt [batch] valid rows,
 * anchors [n_boxes][8] = template anchor (cx, cy, w, h) + 4 variances (float64) -> y_true [batch][n_boxes]
 * [n_classes + 12] fp32.  n_classes includes the background class.  border_pixels: 0 'half', 1 'include', -1
 * 'exclude'; multi = 1 for matching_type 'multi'.  Limits: max_gt <= 128, n_boxes <= 12288.  Degenerate boxes
 * (xmax <= xmin ...) must be rejected by the caller, as the reference raises DegenerateBoxError on the host. ---- */
int dj_ssd_encode_targets(const double* labels, const int* n_gt, int batch, int max_gt, const double* anchors,
                          int n_boxes, int n_classes, int img_height, int img_width, int normalize_coords,
                          int border_pixels, int multi, double pos_iou_threshold, double neg_iou_limit,
                          int background_id, float* y_true, void* stream);

/* ---- GlobalAveragePooling2D (C/vgg_jpeg_keras/networks/resnet_dct.py:415) ---- */
int dj_global_avg_pool_fwd(const float* x, float* y, int B, int HW, int C, void* stream);
int dj_global_avg_pool_bwd(const float* dy, float* dx, int B, int HW, int C, int beta, void* stream);

/* ---- RGB batch -> de-quantised JPEG DCT coefficient tensors, what `Image.fromarray(x).save(f, format="jpeg")` followed by
 * `jpeg2dct.numpy.loads` yields (L/data_generator/object_detection_2d_data_generator_dct_j2d.py:1167-1195), bit for bit and
 * without the file in between: libjpeg's integer RGB->YCbCr, 4:2:0 box downsampling, "slow" integer forward DCT and
 * quantisation, then the multiplication by the table again (normalized != 0) or the bare level (normalized == 0).
 * rgb: DEVICE [batch][height][width][3] bytes, `stride_bytes` between pixel rows, images dense (height * stride_bytes apart).
 * luma_table / chroma_table: HOST pointers to 64 entries in natural (row-major) order, each 1..255; they travel as kernel
 * arguments, so the call stays capturable.  Outputs are float32 NHWC block tensors, channel 8*u+v = vertical frequency u,
 * horizontal frequency v: out_y [batch][ceil(h/8)][ceil(w/8)] pixels of ld_y floats, out_cb / out_cr
 * [batch][ceil(ceil(h/2)/8)][ceil(ceil(w/2)/8)] pixels of ld_cb / ld_cr floats (each >= 64: Cb and Cr may be the two
 * channel halves of one 128-channel tensor).  Only the 64 channels of each pixel are written. ---- */
int dj_rgb_to_dct(const unsigned char* rgb, int batch, int height, int width, long stride_bytes,
                  const unsigned short* luma_table, const unsigned short* chroma_table, int normalized, float* out_y,
                  long ld_y, float* out_cb, long ld_cb, float* out_cr, long ld_cr, void* stream);

/* ---- Decoded RGB images of different sizes -> one [batch][target][target][3] uint8 tensor: `im.resize(...)`, `im.crop(...)`
 * and `im.transpose(FLIP_LEFT_RIGHT)` of the classifier generators (C/vgg_jpeg_keras/generators/generators.py:141-167,
 * :299-325), bit for bit what Pillow's two-pass resampler leaves: per pass and sample
 * clip8((2^21 + sum_k pixel[first + k] * tap[k]) >> 22) in 32-bit integers, a uint8 image between the passes.  The taps are a
 * function of the two sizes and the filter alone; the caller computes them (data/image_prep.py:resample_coeffs) and passes
 * them in an int32 pool: per axis `bounds` = one (first source index, tap count) pair per sample of the RESIZED axis and
 * `taps` = one row of `ksize` ints per sample.  An axis whose size is unchanged (Pillow skips the pass) is passed as one
 * tap of 2^22 per sample.  Only the target x target window at (crop_x, crop_y) of the resized image is computed: the
 * horizontal pass runs over source rows row0 .. row0 + n_rows - 1, which must cover what the window's vertical taps read,
 * and leaves n_rows x target pixels at scratch + scratch_offset; images' scratch regions come in batch order and do not
 * overlap (dj_image_prep_scratch_bytes: the size when each region is rounded up to 64 bytes).
 * src / desc_dev / pool_dev / out / scratch are DEVICE pointers; desc_host / pool_host are HOST copies of the same
 * descriptors and pool, read during the call only: every index the kernels will form is checked against the buffer sizes
 * before anything is launched (an error writes nothing), and the grid is sized from them -- no synchronisation, so the
 * call stays capturable.  out: images target * out_stride_bytes apart, only the 3 * target bytes of each row are written. ---- */
typedef struct dj_image_prep_desc {
  long src_offset;     /* bytes from `src` to the image's first pixel */
  long src_stride;     /* bytes between its pixel rows, >= 3 * src_w */
  long scratch_offset; /* bytes from `scratch` to this image's horizontal-pass rows */
  int src_h, src_w;
  int res_h, res_w;    /* size after the resize */
  int crop_y, crop_x;  /* origin of the window in the resized image */
  int flip;            /* != 0: the window is mirrored left-right */
  int h_bounds, h_taps, h_ksize; /* pool offsets (in ints) of the horizontal bounds and taps, ints per tap row */
  int v_bounds, v_taps, v_ksize;
  int row0, n_rows;    /* source rows the horizontal pass produces */
} dj_image_prep_desc;
long dj_image_prep_scratch_bytes(const dj_image_prep_desc* desc_host, int batch, int target);
int dj_image_prep(const unsigned char* src, long src_bytes, const dj_image_prep_desc* desc_dev,
                  const dj_image_prep_desc* desc_host, int batch, const int* pool_dev, const int* pool_host, long pool_ints,
                  int target, unsigned char* out, long out_stride_bytes, unsigned char* scratch, long scratch_bytes,
                  void* stream);

/* ---- Photometric augmentation of a [batch][height][width][3] uint8 tensor IN PLACE: the `saturation`, `brightness`,
 * `contrast` and `lighting` callables of the classifier generators (C/vgg_jpeg_keras/generators/helper.py:12-45), bit for bit
 * what numpy computes in float64 (data/photometric.py:photometric_host states the contract: the grey value is
 * fma(b, 0.114, fma(g, 0.587, r * 0.299)), the mean of `contrast` is numpy's pairwise sum / n, `lighting` works from exact
 * integer moments; every operation ends in clip to [0, 255] and truncation to uint8).  Image i runs ops[i].n_ops operations
 * in order: param[k][0] is alpha for saturation / brightness / contrast, param[k][0..2] the three normal draws times the
 * standard deviation for lighting.  pixels / ops_dev / shift_out are DEVICE pointers, ops_host the HOST copy of the same
 * lists, read during the call only: an unknown code, more than DJ_PHOTO_MAX_OPS operations or a parameter that is not finite
 * is an error, and an error writes nothing.  pixels: `stride_bytes` between pixel rows, images height * stride_bytes apart,
 * only the 3 * width bytes of each row are touched; height * width <= 2^18.  shift_out (optional, [batch][3] doubles)
 * receives the per-channel shift the image's last lighting operation added (zeros when it has none).  One launch, no
 * synchronisation: the call stays capturable. ---- */
#define DJ_PHOTO_MAX_OPS 4
#define DJ_PHOTO_SATURATION 1
#define DJ_PHOTO_BRIGHTNESS 2
#define DJ_PHOTO_CONTRAST 3
#define DJ_PHOTO_LIGHTING 4
typedef struct dj_photometric_ops {
  int n_ops;
  int code[DJ_PHOTO_MAX_OPS];
  int reserved;
  double param[DJ_PHOTO_MAX_OPS][3];
} dj_photometric_ops;
int dj_photometric(unsigned char* pixels, int batch, int height, int width, long stride_bytes,
                   const dj_photometric_ops* ops_dev, const dj_photometric_ops* ops_host, double* shift_out, void* stream);

/* ---- A window of each decoded RGB image on a constant background, optionally mirrored, resized -> one
 * [batch][out_h][out_w][3] uint8 tensor: the expand, crop, flip and resize stages of the SSD augmentation chain composed
 * (data/ssd_augment.py), bit for bit what data/patch_resize.py:patch_resize_host states in numpy: the window is a canvas of
 * `background` with the image under it pasted in, mirrored left-right when `flip` is set, then resized as Pillow's
 * Image.resize does, with dj_image_prep's arithmetic (two passes, clip8((2^21 + sum_k pixel[first + k] * tap[k]) >> 22), a
 * uint8 image between them).  Bounds and taps come from the caller in an int32 pool as for dj_image_prep, here per axis for
 * window size -> output size: `bounds` = one (first window sample, tap count) pair per OUTPUT sample, `taps` = one row of
 * `ksize` ints per output sample; an unchanged axis, and Pillow's NEAREST, travel as one tap of 2^22 per sample.
 * Only the rectangle of the image that the window covers needs to be staged: src_h x src_w is that rectangle (0 x 0 when
 * the window misses the image: every sample is background) and the window origin is relative to it, so it may be negative
 * and the window may extend past either far edge.  The horizontal pass leaves win_h x out_w pixels at scratch +
 * scratch_offset; images' scratch regions come in batch order and do not overlap (dj_patch_resize_scratch_bytes: the size
 * when each region is rounded up to 64 bytes).  Pointers, the host copies, the checks before anything is launched (an error
 * writes nothing) and capturability as for dj_image_prep.  out: images out_h * out_stride_bytes apart, only the 3 * out_w
 * bytes of each row are written. ---- */
typedef struct dj_patch_resize_desc {
  long src_offset;     /* bytes from `src` to the staged rectangle's first pixel */
  long src_stride;     /* bytes between its pixel rows, >= 3 * src_w */
  long scratch_offset; /* bytes from `scratch` to this image's horizontal-pass rows */
  int src_h, src_w;    /* size of the staged rectangle */
  int win_y0, win_x0;  /* origin of the window relative to the staged rectangle, any sign */
  int win_h, win_w;
  int flip;            /* != 0: the window is mirrored left-right before the resize */
  int background;      /* r | g << 8 | b << 16 */
  int h_bounds, h_taps, h_ksize; /* pool offsets (in ints) of the bounds and taps for win_w -> out_w, ints per tap row */
  int v_bounds, v_taps, v_ksize; /* the same for win_h -> out_h */
} dj_patch_resize_desc;
long dj_patch_resize_scratch_bytes(const dj_patch_resize_desc* desc_host, int batch, int out_w);
int dj_patch_resize(const unsigned char* src, long src_bytes, const dj_patch_resize_desc* desc_dev,
                    const dj_patch_resize_desc* desc_host, int batch, const int* pool_dev, const int* pool_host,
                    long pool_ints, int out_h, int out_w, unsigned char* out, long out_stride_bytes, unsigned char* scratch,
                    long scratch_bytes, void* stream);

/* ---- The photometric stage of the SSD augmentation chain (`SSDPhotometricDistortions`) IN PLACE on the staged rectangles of
 * a ragged batch, before dj_patch_resize reads them: byte for byte what data/ssd_photometric.py:ssd_photometric_host states
 * in numpy.  Per pixel, with everything between bytes in float32, every operation rounding on its own and bytes made by
 * rounding half to even:
 *   sequence 1: brightness, contrast, ->u8, RGB->HSV, saturation, hue, ->u8, HSV->RGB, channel order
 *   sequence 2: brightness, ->u8, RGB->HSV, saturation, hue, ->u8, HSV->RGB, contrast, ->u8, channel order
 * brightness clip(x + delta, 0, 255), contrast clip(127.5 + factor * (x - 127.5), 0, 255), saturation clip(S * factor, 0, 255),
 * hue remainder(H + delta, 180) with the divisor's sign; the colour conversions are OpenCV's 8-bit ones (H in 0..180) as that
 * module restates them, and they run whatever `flags` selects.  Output channel k is channel order[k] of the result.
 * The rectangles are those of the dj_patch_resize descriptors (src_offset, src_stride, src_h, src_w; nothing else of a
 * descriptor is read): only the 3 * src_w bytes of each staged row are touched, and an image with a 0 x 0 rectangle costs
 * nothing.  src / desc_dev / params_dev are DEVICE pointers, desc_host / params_host the HOST copies, read during the call
 * only and checked before anything is launched: a sequence other than 1 or 2, unknown flags, a parameter that is not finite
 * (those of operations that are off included: they travel as zero), an order that is no permutation of (0, 1, 2), a
 * rectangle that leaves `src_bytes` or holds 2^31 pixels or more is an error, and an error writes nothing.  One launch, no
 * synchronisation: the call stays capturable. ---- */
#define DJ_SSD_PHOTO_BRIGHTNESS 1
#define DJ_SSD_PHOTO_CONTRAST 2
#define DJ_SSD_PHOTO_SATURATION 4
#define DJ_SSD_PHOTO_HUE 8
typedef struct dj_ssd_photo_params {
  int sequence;        /* 1 or 2 */
  int flags;           /* DJ_SSD_PHOTO_* of the operations that were drawn */
  float brightness;    /* delta */
  float contrast;      /* factor */
  float saturation;    /* factor */
  float hue;           /* delta */
  int order[3];
  int reserved;
} dj_ssd_photo_params;
int dj_ssd_photometric(unsigned char* src, long src_bytes, const dj_patch_resize_desc* desc_dev,
                       const dj_patch_resize_desc* desc_host, const dj_ssd_photo_params* params_dev,
                       const dj_ssd_photo_params* params_host, int batch, void* stream);

/* ---- RGB pixels of baseline / extended-sequential JPEG files from their entropy-decoded RAW (not de-quantised) int16
 * coefficient planes (include/dj_jpeg_decode.h: dj_jpeg_read_raw_batch), byte for byte what data/jpeg_pixels.py:jpeg_pixels_host
 * states in numpy and Pillow's Image.open(f).convert("RGB") returns: coefficient * table in int32, libjpeg's integer "slow"
 * inverse DCT (13-bit constants; column pass descaled by 11 bits, row pass by 18, + 128, clamp), the triangle upsampling
 * filters for a chroma component wider than 2 samples (neighbours past the component's real down-sampled extent are the
 * edge sample) and plain replication for a narrower one, the 16-bit fixed-point YCbCr -> RGB; one component is gray,
 * replicated.  Per image only the rectangle rows [ya, yb) x columns [xa, xb) is reconstructed, into dst + dst_offset with
 * rows dst_stride apart: where a staging plan would have copied decoded pixels.  Component c's plane is blocks_h[c] x
 * blocks_w[c] x 64 values in natural order at coef + coef_offset[c] (bytes, even) and its table 64 ints at tables +
 * table_offset + 64 c.  The inverse DCT runs over block rows [by0, by1) x columns [bx0, bx1) of each component -- at least
 * the blocks the rectangle's samples and their filter neighbours lie in -- and leaves them as a uint8 plane of
 * 8 (bx1 - bx0) bytes per row at scratch + sample_offset[c] (a multiple of 8); these regions come in (image, component)
 * order and do not overlap.  coef / desc_dev / tables / dst / scratch are DEVICE pointers, desc_host the HOST copy of the
 * descriptors, read during the call only: every offset, grid, range and rectangle is checked against the sizes given
 * before anything is launched, and an error writes nothing.  Two launches, no synchronisation: capturable. ---- */
typedef struct dj_jpeg_pixels_desc {
  long coef_offset[3];
  long sample_offset[3];
  long dst_offset;
  long dst_stride;       /* >= 3 * (xb - xa) */
  int table_offset;      /* ints */
  int n_components;      /* 1 (gray) or 3 (YCbCr) */
  int h_samp, v_samp;    /* luma over chroma: 1x1, 2x1 or 2x2 (1x1 for gray) */
  int height, width;     /* of the image */
  int ya, yb, xa, xb;
  int blocks_h[3], blocks_w[3];
  int by0[3], by1[3], bx0[3], bx1[3];
} dj_jpeg_pixels_desc;
int dj_jpeg_pixels(const unsigned char* coef, long coef_bytes, const dj_jpeg_pixels_desc* desc_dev,
                   const dj_jpeg_pixels_desc* desc_host, int n, const int* tables, long table_ints, unsigned char* dst,
                   long dst_bytes, unsigned char* scratch, long scratch_bytes, void* stream);

/* ---- The networks' DCT input tensors from the files' OWN coefficients: a window of each file's raw int16 planes (as
 * dj_jpeg_read_raw_batch left them), de-quantised and optionally mirrored, scattered into the float32 inputs -- bit for bit
 * what data/coefficient_inputs.py:coefficient_inputs_host states.  Each value is (float)(int16)(coefficient * table entry):
 * the product in int32, wrapped to int16 as the host reader's emission does, then converted.  Image i fills output blocks
 * [i][0..yh)[0..yw) of out_y from its luma blocks (by0[0] + r, bx0[0] + c) and [i][0..ch)[0..cw) of out_cb / out_cr from its
 * chroma blocks (by0[c] + r, bx0[c] + c); with flip != 0 output block column j takes window column n_cols - 1 - j and every
 * coefficient of odd horizontal frequency (natural index k with k & 1) is negated in int16 (jpegtran's lossless mirror).
 * A one-component image fills out_cb and out_cr with zeros: EVERY element of the three outputs is written.  Block (r, c)
 * of image i lies 64 floats at out + ((i * rows + r) * cols + c) * ld; ld_* >= 64 (Cb and Cr may be the two halves of one
 * 128-channel tensor) and *_floats is what may be written from each pointer.  Component c's plane is blocks_h[c] x
 * blocks_w[c] x 64 values in natural order at coef + coef_offset[c] (bytes, a multiple of 16; coef itself 16-byte aligned)
 * and its table 64 ints at tables + table_offset + 64 c (tables 16-byte aligned, table_offset a multiple of 4).  An output
 * whose pointer is 16-byte aligned and whose ld is a multiple of 4 is written with 16-byte stores, any other element by
 * element.  coef / desc_dev / tables / out_* are DEVICE pointers, desc_host the HOST copy of the descriptors, read during
 * the call only: every offset, grid, window, table offset and stride is checked against the sizes given before anything is
 * launched, and an error launches nothing and writes nothing.  One launch, no synchronisation: capturable. ---- */
typedef struct dj_jpeg_dct_desc {
  long coef_offset[3];             /* bytes */
  int blocks_h[3], blocks_w[3];    /* the file's block grids */
  int by0[3], bx0[3];              /* window origin, in blocks */
  int table_offset;                /* ints */
  int n_components;                /* 1 (gray) or 3 (YCbCr, luma 2x2 over chroma) */
  int flip;                        /* 0 or 1 */
} dj_jpeg_dct_desc;
int dj_jpeg_dct_inputs(const unsigned char* coef, long coef_bytes, const dj_jpeg_dct_desc* desc_dev,
                       const dj_jpeg_dct_desc* desc_host, int n, const int* tables, long table_ints, int yh, int yw, int ch,
                       int cw, float* out_y, long ld_y, long y_floats, float* out_cb, long ld_cb, long cb_floats,
                       float* out_cr, long ld_cr, long cr_floats, void* stream);

/* ---- Huffman entropy decoding of restart-interval JPEG files, one lane per restart interval ("segment"), to the RAW int16
 * planes dj_jpeg_read_raw_batch would have written -- bit for bit what data/entropy_decode.py:entropy_decode_host states
 * (its docstring holds the rules: the bit source with FF 00 unstuffing, the DC and AC rules of the host reader's
 * decode_block, the statuses 1..4, "a failing block and every later block of its segment are zero").  The host half is
 * dj_jpeg_scan_segments (include/dj_jpeg_segments.h), which finds the segments and builds the tables.
 * bytes: the files' bytes, anywhere inside `n_bytes`; segment record s = bytes [begin, end), the file it belongs to and
 * the MCUs it holds ([first_mcu, first_mcu + n_mcus) of that file, in scan order).  File descriptor i: component c's plane
 * is blocks_h[c] x blocks_w[c] x 64 values in natural order at out + plane_offset[c] (bytes, a multiple of 16; out itself
 * 16-byte aligned), of which plane_capacity[c] values are the caller's; h_blocks / v_blocks are its blocks per MCU,
 * dc_table / ac_table index the file's tables (0..3), which start at table `table_first` of `tables` (n_tables tables of
 * DJ_JPEG_HUFF_BYTES = 896 bytes in the device form of dj_jpeg_segments.h, `tables` 16-byte aligned); its segments are
 * records [seg_first, seg_first + n_segments) and must tile its mcus_x * mcus_y MCUs in order.
 * EVERY element of every plane is written (zeros included), and status[s] = 0 or 1..4 for every segment.
 * bytes / desc_dev / seg_dev / tables / out / status are DEVICE pointers; desc_host and seg_host the HOST copies of the
 * descriptors and records, read during the call only: every byte range, plane offset and capacity, table index, block
 * and MCU count is checked against the sizes given before anything is launched, and an error launches nothing and writes
 * nothing.  The kernel clips every read to [0, n_bytes) and every store to the plane's capacity and out_bytes again, from
 * what it reads on the device, so device data that differs from the host copies gives wrong values and a status, never
 * an access outside the buffers given.  One launch, no synchronisation: capturable. ---- */
typedef struct dj_jpeg_entropy_desc {
  long plane_offset[3];            /* bytes */
  long plane_capacity[3];          /* int16 values */
  int blocks_h[3], blocks_w[3];
  int h_blocks[3], v_blocks[3];    /* blocks per MCU across / down */
  int dc_table[3], ac_table[3];    /* 0..3 */
  int table_first;                 /* tables */
  int n_components;                /* 1 or 3 */
  int mcus_x, mcus_y;
  int seg_first, n_segments;
} dj_jpeg_entropy_desc;
typedef struct dj_jpeg_entropy_seg {
  long begin, end;                 /* bytes */
  int file;
  int first_mcu, n_mcus;
  int reserved;                    /* dj_jpeg_entropy_decode_chunked: the segment's first chunk; otherwise unused */
} dj_jpeg_entropy_seg;
int dj_jpeg_entropy_decode(const unsigned char* bytes, long n_bytes, const dj_jpeg_entropy_desc* desc_dev,
                           const dj_jpeg_entropy_desc* desc_host, int n_files, const dj_jpeg_entropy_seg* seg_dev,
                           const dj_jpeg_entropy_seg* seg_host, int n_segments, const unsigned char* tables, int n_tables,
                           unsigned char* out, long out_bytes, int* status, void* stream);

/* ---- The same planes and statuses for files WITHOUT restart intervals (and for files with them), by chunks: a segment is
 * cut every `chunk_bytes` raw bytes (a multiple of 16 in 16..4096; at most 65536 chunks a segment), the chunks are decoded
 * in parallel from guessed states and synchronised by a bounded fixed-point iteration whose result is the sequential
 * decode -- data/entropy_decode.py:chunked_decode_host states the scheme, csrc/dj_jpeg_entropy_chunked.hip runs it.  The
 * host half is dj_jpeg_scan_segments_unmarked (include/dj_jpeg_segments.h).
 * Arguments, checks and guarantees of dj_jpeg_entropy_decode, and in addition: record s's `reserved` is the number of
 * chunks of the segments in front of it (segment s has max(1, ceil((end - begin) / chunk_bytes)) chunks); `scratch` is a
 * DEVICE buffer, 16-byte aligned, of at least dj_jpeg_entropy_chunked_scratch_bytes(chunks, files, segments, blocks) bytes
 * (blocks: the sum over the files of mcus_x * mcus_y * blocks per MCU), whose contents need not survive between calls;
 * `rounds` (DEVICE, may be null) receives per segment the synchronisation rounds it took, at most its chunk count.
 * Five launches on `stream`, no synchronisation: capturable. ---- */
long dj_jpeg_entropy_chunked_scratch_bytes(long n_chunks, long n_files, long n_segments, long n_blocks);
int dj_jpeg_entropy_decode_chunked(const unsigned char* bytes, long n_bytes, const dj_jpeg_entropy_desc* desc_dev,
                                   const dj_jpeg_entropy_desc* desc_host, int n_files, const dj_jpeg_entropy_seg* seg_dev,
                                   const dj_jpeg_entropy_seg* seg_host, int n_segments, const unsigned char* tables, int n_tables,
                                   unsigned char* out, long out_bytes, int* status, int chunk_bytes, unsigned char* scratch,
                                   long scratch_bytes, int* rounds, void* stream);

/* ---- Pascal-VOC evaluation (L/eval_utils/average_precision_evaluator.py:570-925): `Evaluator.match_predictions`,
 * `compute_precision_recall` and `compute_average_precisions(mode='sample')` with results equal bit for bit to the host
 * methods (float64, their operation order; eval_utils/device_matching.py packs the inputs and restates the segment-wise
 * computation in numpy).  All pointers are DEVICE pointers.
 * Predictions of classes 1..n_classes lie one class after another, each class in rank order (confidence descending, equal
 * confidences in list order): class c occupies [class_offsets[c], class_offsets[c + 1]) of pred_boxes [n_pred][4] =
 * (xmin, ymin, xmax, ymax) float32 and of every per-prediction output; class_offsets has n_classes + 2 entries.  A segment
 * is one (class, image) pair with predictions: seg_ranks[seg_offsets[s] .. seg_offsets[s + 1]) holds their ranks within
 * the class, increasing.  Ground truth: gt_boxes [n_gt][4] float64, gt_class, gt_neutral (bytes), image i owning rows
 * [gt_offsets[i], gt_offsets[i + 1]), at most 4096 per image (max_gt_per_image is the caller's maximum, checked).
 * dj_eval_match: one wave per segment walks its predictions in rank order; IoU as iou(gt, pred, coords='corners',
 * mode='element-wise', border_pixels), np.argmax over the image's rows of the class (first maximum, a NaN wins), then
 * false positive when there is no such row or best < matching_iou_threshold, nothing when the row is neutral and
 * use_neutral != 0, true positive when the row is free (it is taken then), false positive otherwise.  tp / fp [n_pred]
 * int32 receive the flags at class_offsets[c] + rank; the caller zeroes them first.
 * dj_eval_precision_recall_ap: one block per class: cum_tp / cum_fp (running sums of the flags), precision = tp / (tp + fp)
 * where tp + fp > 0 else 0, recall = tp / num_gt[c] (num_gt: n_classes + 1 doubles), and ap[c] (n_classes + 1 doubles,
 * entry 0 untouched) = (sum over the num_recall_points <= 1024 thresholds t, in order, of max{precision : recall >= t} or 0)
 * / num_recall_points.  Both are one launch without synchronisation. ---- */
int dj_eval_match(const float* pred_boxes, const int* seg_ranks, const int* seg_offsets, const int* seg_class,
                  const int* seg_image, int n_segments, const int* class_offsets, int n_classes, int n_pred,
                  const double* gt_boxes, const int* gt_class, const unsigned char* gt_neutral, const int* gt_offsets,
                  int n_images, int n_gt, int max_gt_per_image, int use_neutral, double matching_iou_threshold,
                  int border_pixels, int* tp, int* fp, void* stream);
int dj_eval_precision_recall_ap(const int* tp, const int* fp, const int* class_offsets, int n_classes, int n_pred,
                                const double* num_gt, const double* thresholds, int num_recall_points, int* cum_tp,
                                int* cum_fp, double* precision, double* recall, double* ap, void* stream);

/* ---- The stages in front of dj_eval_match (L/eval_utils/average_precision_evaluator.py:262-470, the loop of
 * `predict_on_dataset`, and the prediction half of device_matching.py:pack_evaluation), equal bit for bit to the host and
 * stated in numpy by device_matching.py:collect_host / rank_host.  Device pointers unless said otherwise; neither entry
 * point synchronises with the host.  counters [4] int32, zeroed by the caller once per evaluation: [0] records appended,
 * [1] errors (a class id that is no integer in 1..n_classes, a NaN confidence), [2] segments, [3] records dropped for lack
 * of room (the host-side capacity check keeps it 0).
 * dj_eval_collect: decoded [batch][rows][6] float32 = (class id, conf, xmin, ymin, xmax, ymax) as DecodeDetections leaves
 * it, rows with class id 0 are padding (anywhere among the rows).  Of the first n_valid images every other row is appended
 * behind counters[0], image after image and rows in their order, to the record arrays of `capacity` entries: rec_class,
 * rec_image (desc.image_index), rec_ordinal (first_ordinal + the image's place in the batch: which collected image the row
 * came from), rec_conf float32, rec_conf64 (the same before its conversion to float32), rec_boxes [capacity][4] float32.
 * desc_host [batch] lives on the HOST and travels in the kernel arguments (one launch per 128 images).  kind 1 is the
 * inverse of `Resize`: y = rintf(y * scale_y), x = rintf(x * scale_x) in float32, the product rounded before rintf; kind
 * 0 leaves the box alone.  Then every coordinate becomes (float)(rint(10.0 * v) / 10.0) in float64, CPython's
 * round(float(v), 1), and with conf_digits d in 1..8 the confidence rint(10^d * conf) / 10^d (conf_digits 0: unchanged).
 * boxes_final != 0: the boxes are stored as they are (the host applied the transforms and the rounding); the confidence
 * is treated as always.  Refused unless (first_ordinal + n_valid) * rows <= capacity, which bounds counters[0]; the kernel
 * itself never writes past capacity.
 * dj_eval_rank: the counters[0] records -> class_offsets [n_classes + 2], pred_class / pred_image / pred_conf / pred_boxes
 * (class after class, within a class confidence descending with -0.0 == 0.0 and equal confidences in record order),
 * seg_class / seg_image / seg_offsets [capacity + 1] / seg_ranks as dj_eval_match reads them, segments ordered by
 * (class, image); counters[2] receives their number.  Every per-prediction array has `capacity` entries, of which the first
 * counters[0] are written.  workspace: dj_eval_rank_workspace_bytes(capacity, n_classes) bytes, 8-byte aligned.  Sorting is
 * done here (tiles of 1024 keys in LDS, then merge passes), on unique 64-bit keys, so the result does not depend on the
 * run. ---- */
typedef struct {
  int image_index;     /* position of the image's id in data_generator.image_ids */
  int kind;            /* 0 identity, 1 resize */
  float scale_y;       /* img_height / out_height rounded to float32 */
  float scale_x;       /* img_width / out_width rounded to float32 */
} dj_eval_collect_desc;
int dj_eval_collect(const float* decoded, int batch, int rows, int n_valid, const dj_eval_collect_desc* desc_host,
                    int first_ordinal, int n_classes, int n_images, int conf_digits, int boxes_final, int* rec_class,
                    int* rec_image, int* rec_ordinal, float* rec_conf, double* rec_conf64, float* rec_boxes, long capacity,
                    int* counters, void* stream);
long dj_eval_rank_workspace_bytes(long capacity, int n_classes);
int dj_eval_rank(const int* rec_class, const int* rec_image, const float* rec_conf, const float* rec_boxes, long capacity,
                 int n_classes, int n_images, int* counters, int* class_offsets, int* pred_class, int* pred_image,
                 float* pred_conf, float* pred_boxes, int* seg_class, int* seg_image, int* seg_offsets, int* seg_ranks,
                 void* workspace, long workspace_bytes, void* stream);

/* ---- Validation metrics of a classifier, accumulated over a whole pass of a generator (Model.evaluate_generator and the
 * validation sweep of fit_generator; C/vgg_jpeg_keras/evaluation/evaluators.py:13-22, C/config/resnet/config_file.py:19-22).
 * keras/metrics.py:classification_counts_host states the counting in numpy; the counts here equal it exactly.
 * y_true / probs: contiguous float32 [rows][C] on the device.  Per row t = np.argmax(y_true[row]) (the first maximum, a NaN
 * counts as the maximum) and p_t = probs[row][t].  Entry q of ks_host (n_k <= 8 ints on the HOST, read during the call: they
 * travel in the kernel arguments) with k >= 1 is tf.nn.in_top_k, which Keras 2.2.4's top_k_categorical_accuracy calls: a hit
 * iff p_t is finite and fewer than k classes have a probability > p_t, so classes tied with the target all count as in the
 * top k and a NaN elsewhere in the row is not counted; k == 0 is categorical_accuracy: a hit iff np.argmax(probs[row]) == t.
 * counts [1 + n_k] int64: [0] += rows, [1 + q] += hits of entry q.  acc [2] float64: with loss_mean (device, the mean loss
 * of the batch as the loss entry points leave it; may be NULL) acc[0] += loss_weight * (double)loss_mean[0], the product
 * rounded before the sum, and acc[1] += loss_weight.  With rows == 0, or y_true / probs NULL, only the loss is accumulated.
 * The caller zeroes acc and counts once per pass.  One launch, no synchronisation; hit counts are added as integers and the
 * loss term by one thread, so the result does not depend on the grid, and successive calls on one stream add in call
 * order.  Refused before any launch: n_k outside 0..8, a k outside 0..C (a loss-only call with rows == 0 and C <= 0 states
 * no C: there only a negative k), rows < 0, C <= 0 with rows > 0, acc or counts NULL. ---- */
int dj_eval_accumulate(const float* y_true, const float* probs, long rows, int C, const int* ks_host, int n_k,
                       const float* loss_mean, double loss_weight, double* acc, long long* counts, void* stream);

/* ---- Dropout (keras.layers.Dropout in training plans; C/vgg_jpeg_keras/networks/networks_dct.py, the two layers between
 * fc1, fc2 and predictions).  keras/dropout.py states it in numpy; both entry points equal that statement bit for bit.
 * No state and no stored mask: element i of a contiguous float32 tensor of n elements is kept iff lane (i & 3) of
 * Philox4x32-10(counter = (lo32(i >> 2), hi32(i >> 2), ctr2, ctr3), key = (key0, key1)) is >= threshold, so the mask of an
 * element does not depend on n and the backward pass regenerates the forward's mask from the same six words.  The layer
 * packs key0 = its seed, key1 = the data-parallel rank, (ctr2, ctr3) = the low and high half of the optimizer's step
 * count; threshold = min(int(rate * 2^32), 2^32 - 1) and scale = (float)(1 / (1 - rate)) are computed on the host.
 * dj_dropout_fwd: y[i] = (x[i] * scale) * keep_i with keep_i 0.0f / 1.0f -- a product, so an Inf or NaN at a dropped
 * position gives NaN; y == x is allowed.  dj_dropout_bwd: dx[i] = (dy[i] * scale) * keep_i, added to dx[i] when beta == 1.
 * One thread per four consecutive elements in a grid-stride loop of at most dj_dropout_groups_per_pass() threads; 16-byte
 * loads and stores when both pointers are 16-byte aligned, element by element otherwise and in the n % 4 tail.  Refused
 * before any launch: a NULL pointer, n <= 0, beta outside {0, 1}. ---- */
long dj_dropout_groups_per_pass(void);
int dj_dropout_fwd(const float* x, float* y, long n, unsigned threshold, float scale, unsigned key0, unsigned key1,
                   unsigned ctr2, unsigned ctr3, void* stream);
int dj_dropout_bwd(const float* dy, float* dx, long n, unsigned threshold, float scale, unsigned key0, unsigned key1,
                   unsigned ctr2, unsigned ctr3, int beta, void* stream);

/* ---- Keras' ImageDataGenerator on a [batch][height][width][3] uint8 tensor -> float32 NHWC: the affine warp, the flips and
 * the standardisation that `ImageDataGenerator(...).flow_from_directory(...)` of the RGB ResNet50 applies to every loaded
 * image (C/config/resnetRGB/config_file.py:157-172; per image Keras runs scipy.ndimage.affine_transform(order=1,
 * mode='nearest') once per channel, in float64).  data/rgb_warp.py:affine_warp_host states the warp and rgb_warp_host the
 * whole call; the result equals them bit for bit.  Per image one record: m = the top two rows of the recentred matrix M,
 * row-major; identity != 0: no warp, the pixel's own value; flip_cols / flip_rows: mirror the warped image.  For the pixel
 * (i, j) of the warped image, everything in float64 with every product and sum rounded on its own:
 *   r = (m[0]*i + m[1]*j) + m[2], c = (m[3]*i + m[4]*j) + m[5], both clipped to the image; r0 = floor(r), tr = r - r0,
 *   r1 = min(r0 + 1, height - 1) (columns alike); value = (((x[r0,c0]*(1-tr))*(1-tc) + (x[r0,c1]*(1-tr))*tc)
 *   + (x[r1,c0]*tr)*(1-tc)) + (x[r1,c1]*tr)*tc, rounded once to float32.
 * Output pixel (i, j) is the warped pixel (flip_rows ? height-1-i : i, flip_cols ? width-1-j : j).  Then, in float32:
 * preprocess == DJ_RGB_PREP_CAFFE reverses the channels and subtracts (103.939f, 116.779f, 123.68f); has_rescale != 0
 * multiplies by `rescale`.  pixels (dense packed RGB) / rec_dev / out are DEVICE pointers, rec_host the HOST copy of the
 * records, read during the call only.  out: `out_row_stride` floats between pixel rows, images height * out_row_stride
 * apart, only the 3 * width floats of each row are written.  One thread per four consecutive pixels: three 16-byte stores
 * where `out` is 16-byte aligned and, with strided rows, out_row_stride is a multiple of 4; element by element otherwise and
 * in the tail of a run.  Refused before any launch: a NULL pointer, batch / height / width < 1 or a side above 32768,
 * out_row_stride < 3 * width, an unknown preprocess code, a matrix entry of a non-identity record that is not finite.
 * One launch, no synchronisation: the call stays capturable. ---- */
#define DJ_RGB_PREP_NONE 0
#define DJ_RGB_PREP_CAFFE 1
typedef struct dj_rgb_warp_record {
  double m[6];
  int identity, flip_cols, flip_rows, reserved;
} dj_rgb_warp_record;
int dj_rgb_warp(const unsigned char* pixels, int batch, int height, int width, const dj_rgb_warp_record* rec_dev,
                const dj_rgb_warp_record* rec_host, int preprocess, int has_rescale, float rescale, float* out,
                long out_row_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif
