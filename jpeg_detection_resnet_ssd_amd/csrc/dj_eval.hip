// Pascal-VOC evaluation on device: greedy matching of ranked detections to ground truth, then cumulative counts, precision /
// recall and the sampled average precision.  Restates eval_utils/average_precision_evaluator.py (`match_predictions`,
// `compute_precision_recall`, `compute_average_precisions` with mode='sample') and bounding_box_utils.iou (coords='corners',
// mode='element-wise') in their own float64 arithmetic and operation order (IEEE double operators, FMA contraction off), so
// every decision -- np.argmax's first maximum, a NaN overlap winning it, `<` against the threshold -- is the host's and the
// results are equal bit for bit.  eval_utils/device_matching.py packs the inputs and states the same computation in numpy
// (`match_packed_host`).  Greedy matching is sequential only inside one (class, image) pair: one wave per pair.
#include "../../include/dj_hip.h"
#include "dj_common.h"

// every product below must be rounded before it is added to anything (numpy evaluates op by op)
#pragma clang fp contract(off)

#define DJ_EVAL_WAVES 4          // waves (= segments) per block of dj_eval_match
#define DJ_EVAL_MAX_GT 4096      // ground-truth rows per image: bit c of a lane's `taken` mask is row 64 * c + lane
#define DJ_EVAL_PR_THREADS 256
#define DJ_EVAL_PR_ITEMS 4       // consecutive ranks per thread and chunk of the scan
#define DJ_EVAL_PR_GROUP 8       // recall thresholds per sweep over the curves
#define DJ_EVAL_MAX_POINTS 1024  // recall thresholds of the sampled AP (their maxima live in LDS)
#define DJ_EVAL_NONE 0x7fffffff

// np.maximum / np.minimum: a NaN operand is the result (fmax / fmin would drop it)
__device__ __forceinline__ double ev_max(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a >= b ? a : b)); }
__device__ __forceinline__ double ev_min(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a <= b ? a : b)); }

// does (ov, oi) come before (v, i) in np.argmax's order?  A NaN beats every number, equal values (and two NaNs) go to the
// lower index, DJ_EVAL_NONE marks "no candidate yet".
__device__ __forceinline__ bool ev_better(double ov, int oi, double v, int i) {
  if (oi == DJ_EVAL_NONE) return false;
  if (i == DJ_EVAL_NONE) return true;
  const bool on = ov != ov, n = v != v;
  if (on != n) return on;
  if (on) return oi < i;
  return ov > v || (ov == v && oi < i);
}

struct DjEvalMatchParams {
  const float* pred_boxes;   // [n_pred][4] xmin, ymin, xmax, ymax, classes one after another, each in rank order
  const int* seg_ranks;      // [n_pred] ranks (within the class) of every segment's predictions, increasing
  const int* seg_offsets;    // [n_segments + 1] into seg_ranks
  const int* seg_class;      // [n_segments]
  const int* seg_image;      // [n_segments]
  const int* class_offsets;  // [n_classes + 2] first prediction of class c; [c + 1] its end
  const double* gt_boxes;    // [n_gt][4]
  const int* gt_class;       // [n_gt]
  const unsigned char* gt_neutral;  // [n_gt]
  const int* gt_offsets;     // [n_images + 1]
  int* tp;
  int* fp;
  int n_segments, n_classes, n_images, n_pred, n_gt, use_neutral;
  double threshold, d;
};

__global__ __launch_bounds__(64 * DJ_EVAL_WAVES) void dj_eval_match_kernel(DjEvalMatchParams p) {
  const int lane = threadIdx.x & 63;
  const int seg = blockIdx.x * DJ_EVAL_WAVES + (threadIdx.x >> 6);
  if (seg >= p.n_segments) return;     // whole waves leave; the kernel has no block-wide barrier
  const int cls = p.seg_class[seg], img = p.seg_image[seg];
  const int s0 = p.seg_offsets[seg], s1 = p.seg_offsets[seg + 1];
  // a malformed packing must not become an out-of-bounds access: such a segment is skipped (its flags stay zero)
  if (cls < 1 || cls > p.n_classes || img < 0 || img >= p.n_images || s0 < 0 || s1 > p.n_pred || s0 > s1) return;
  const int base = p.class_offsets[cls], class_end = p.class_offsets[cls + 1];
  if (base < 0 || class_end > p.n_pred || base > class_end) return;
  const int g0 = p.gt_offsets[img];
  int n_gt = p.gt_offsets[img + 1] - g0;
  if (g0 < 0 || n_gt < 0 || g0 + n_gt > p.n_gt) n_gt = 0;
  n_gt = min(n_gt, DJ_EVAL_MAX_GT);
  const int n_chunks = (n_gt + 63) >> 6;
  const double d = p.d;

  // the first 64 rows of the image stay in registers (nearly every image has fewer); later rows are re-read per prediction
  bool mine0 = lane < n_gt && p.gt_class[g0 + lane] == cls;
  double r0x0 = 0.0, r0y0 = 0.0, r0x1 = 0.0, r0y1 = 0.0, r0a = 0.0;
  if (mine0) {
    const double* g = p.gt_boxes + (size_t)(g0 + lane) * 4;
    r0x0 = g[0], r0y0 = g[1], r0x1 = g[2], r0y1 = g[3];
    r0a = ((r0x1 - r0x0) + d) * ((r0y1 - r0y0) + d);
  }
  unsigned long long taken = 0;     // bit c: row 64 * c + lane already has its detection

  for (int k0 = s0; k0 < s1; k0 += 64) {
    const int cnt = min(64, s1 - k0);
    int pos = -1;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
    if (lane < cnt) {
      const int r = p.seg_ranks[k0 + lane];
      if (r >= 0 && r < class_end - base) {
        pos = base + r;
        const float* b = p.pred_boxes + (size_t)pos * 4;
        b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
      }
    }
    int my_tp = 0, my_fp = 0;
    for (int j = 0; j < cnt; ++j) {
      if (__shfl(pos, j) < 0) continue;
      const double px0 = (double)__shfl(b0, j), py0 = (double)__shfl(b1, j);
      const double px1 = (double)__shfl(b2, j), py1 = (double)__shfl(b3, j);
      const double a2 = ((px1 - px0) + d) * ((py1 - py0) + d);
      double bv = 0.0;
      int bi = DJ_EVAL_NONE;
      for (int c = 0; c < n_chunks; ++c) {
        const int row = c * 64 + lane;
        bool m = mine0;
        double x0 = r0x0, y0 = r0y0, x1 = r0x1, y1 = r0y1, a1 = r0a;
        if (c > 0) {
          m = row < n_gt && p.gt_class[g0 + row] == cls;
          if (m) {
            const double* g = p.gt_boxes + (size_t)(g0 + row) * 4;
            x0 = g[0], y0 = g[1], x1 = g[2], y1 = g[3];
            a1 = ((x1 - x0) + d) * ((y1 - y0) + d);
          }
        }
        if (m) {
          // iou(): the intersection always uses the 'half' rule (+ 0), the areas use border_pixels
          const double w = ev_max(0.0, (ev_min(x1, px1) - ev_max(x0, px0)) + 0.0);
          const double h = ev_max(0.0, (ev_min(y1, py1) - ev_max(y0, py0)) + 0.0);
          const double inter = w * h;
          const double v = inter / ((a1 + a2) - inter);
          if (ev_better(v, row, bv, bi)) {
            bv = v;
            bi = row;
          }
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (ev_better(ov, oi, bv, bi)) {
          bv = ov;
          bi = oi;
        }
      }
      // (bv, bi) is now the same in every lane, so the branches below are taken by the whole wave
      int tp = 0, fp = 0;
      if (bi == DJ_EVAL_NONE) {
        fp = 1;                                      // no ground truth of this class in the image
      } else if (bv < p.threshold) {
        fp = 1;                                      // `<`: equality matches, a NaN goes on
      } else if (!(p.use_neutral && p.gt_neutral[g0 + bi])) {
        const int owner = bi & 63, ch = bi >> 6;
        int was = 0;
        if (lane == owner) {
          was = (int)((taken >> ch) & 1ull);
          taken |= 1ull << ch;
        }
        was = __shfl(was, owner);
        if (was)
          fp = 1;                                    // duplicate detection of an already detected object
        else
          tp = 1;
      }                                              // else: matched a neutral box, neither
      if (lane == j) {
        my_tp = tp;
        my_fp = fp;
      }
    }
    if (pos >= 0) {
      p.tp[pos] = my_tp;
      p.fp[pos] = my_fp;
    }
  }
}

extern "C" int dj_eval_match(const float* pred_boxes, const int* seg_ranks, const int* seg_offsets, const int* seg_class,
                             const int* seg_image, int n_segments, const int* class_offsets, int n_classes, int n_pred,
                             const double* gt_boxes, const int* gt_class, const unsigned char* gt_neutral,
                             const int* gt_offsets, int n_images, int n_gt, int max_gt_per_image, int use_neutral,
                             double matching_iou_threshold, int border_pixels, int* tp, int* fp, void* stream) {
  DJ_CHECK_ARG(n_segments >= 0 && n_classes >= 1 && n_pred >= 0 && n_images >= 0 && n_gt >= 0, "eval_match: bad sizes");
  DJ_CHECK_ARG(border_pixels >= -1 && border_pixels <= 1, "eval_match: border_pixels must be -1 (exclude), 0 (half), 1 (include)");
  DJ_CHECK_ARG(max_gt_per_image >= 0 && max_gt_per_image <= DJ_EVAL_MAX_GT,
               "eval_match: at most %d ground-truth boxes per image", DJ_EVAL_MAX_GT);
  if (n_segments == 0) return DJ_OK;
  DJ_CHECK_ARG(pred_boxes && seg_ranks && seg_offsets && seg_class && seg_image && class_offsets && gt_offsets && tp && fp,
               "eval_match: null tensor");
  DJ_CHECK_ARG(n_gt == 0 || (gt_boxes && gt_class && gt_neutral), "eval_match: null ground-truth tensor");
  DjEvalMatchParams p;
  p.pred_boxes = pred_boxes;
  p.seg_ranks = seg_ranks;
  p.seg_offsets = seg_offsets;
  p.seg_class = seg_class;
  p.seg_image = seg_image;
  p.class_offsets = class_offsets;
  p.gt_boxes = gt_boxes;
  p.gt_class = gt_class;
  p.gt_neutral = gt_neutral;
  p.gt_offsets = gt_offsets;
  p.tp = tp;
  p.fp = fp;
  p.n_segments = n_segments;
  p.n_classes = n_classes;
  p.n_images = n_images;
  p.n_pred = n_pred;
  p.n_gt = n_gt;
  p.use_neutral = use_neutral ? 1 : 0;
  p.threshold = matching_iou_threshold;
  p.d = (double)border_pixels;
  hipLaunchKernelGGL(dj_eval_match_kernel, dim3(dj_cdiv(n_segments, DJ_EVAL_WAVES)), dim3(64 * DJ_EVAL_WAVES), 0,
                     (hipStream_t)stream, p);
  DJ_CHECK_LAUNCH("dj_eval_match");
  return DJ_OK;
}

// One block per class.  Pass 1: chunked scan of the flags with a carry -> cumulative counts, precision and recall per rank.
// Pass 2: per recall threshold the maximum precision over recall >= t, taken by the whole block over the curves it has just
// written (a max is order-independent, hence exact), DJ_EVAL_PR_GROUP thresholds per sweep; thread 0 then adds the maxima
// in threshold order.
__global__ __launch_bounds__(DJ_EVAL_PR_THREADS) void dj_eval_pr_ap_kernel(
    const int* __restrict__ tp, const int* __restrict__ fp, const int* __restrict__ class_offsets, int n_pred,
    const double* __restrict__ num_gt, const double* __restrict__ thresholds, int n_points, int* __restrict__ cum_tp,
    int* __restrict__ cum_fp, double* precision, double* recall, double* __restrict__ ap) {
  constexpr int kWaves = DJ_EVAL_PR_THREADS / 64;
  __shared__ int wave_tp[kWaves], wave_fp[kWaves];
  __shared__ double s_red[DJ_EVAL_PR_GROUP][kWaves];
  __shared__ double s_thr[DJ_EVAL_MAX_POINTS], s_max[DJ_EVAL_MAX_POINTS];
  const int cls = blockIdx.x + 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int b0 = class_offsets[cls], b1 = class_offsets[cls + 1];
  if (b0 < 0 || b1 > n_pred || b0 > b1) b0 = b1 = 0;     // uniform over the block
  const double ng = num_gt[cls];
  for (int j = tid; j < n_points; j += DJ_EVAL_PR_THREADS) s_thr[j] = thresholds[j];

  // ---- pass 1: thread t of a chunk owns DJ_EVAL_PR_ITEMS consecutive ranks ----
  int carry_tp = 0, carry_fp = 0;
  for (int c0 = b0; c0 < b1; c0 += DJ_EVAL_PR_THREADS * DJ_EVAL_PR_ITEMS) {
    const int i0 = c0 + tid * DJ_EVAL_PR_ITEMS;
    int t[DJ_EVAL_PR_ITEMS], f[DJ_EVAL_PR_ITEMS];
    int st = 0, sf = 0;
#pragma unroll
    for (int k = 0; k < DJ_EVAL_PR_ITEMS; ++k) {
      if (i0 + k < b1) {
        st += tp[i0 + k];
        sf += fp[i0 + k];
      }
      t[k] = st;
      f[k] = sf;
    }
    int it = st, jf = sf;        // inclusive scan of the threads' totals over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int ot = __shfl_up(it, o), of = __shfl_up(jf, o);
      if (lane >= o) {
        it += ot;
        jf += of;
      }
    }
    if (lane == 63) {
      wave_tp[wave] = it;
      wave_fp[wave] = jf;
    }
    __syncthreads();
    int base_tp = carry_tp + it - st, base_fp = carry_fp + jf - sf;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) {
        base_tp += wave_tp[w];
        base_fp += wave_fp[w];
      }
      carry_tp += wave_tp[w];
      carry_fp += wave_fp[w];
    }
#pragma unroll
    for (int k = 0; k < DJ_EVAL_PR_ITEMS; ++k) {
      const int i = i0 + k;
      if (i < b1) {
        const int ct = base_tp + t[k], cf = base_fp + f[k];
        cum_tp[i] = ct;
        cum_fp[i] = cf;
        const double dt = (double)ct, df = (double)cf, s = dt + df;
        precision[i] = s > 0.0 ? dt / s : 0.0;
        recall[i] = dt / ng;     // num_gt == 0: IEEE gives the host's NaN (0/0) or inf
      }
    }
    __syncthreads();             // wave_tp / wave_fp are rewritten by the next chunk
  }
  __threadfence_block();         // the curves below are read by other threads of the block than those that wrote them
  __syncthreads();

  // ---- pass 2 ----
  for (int j0 = 0; j0 < n_points; j0 += DJ_EVAL_PR_GROUP) {
    double thr[DJ_EVAL_PR_GROUP], m[DJ_EVAL_PR_GROUP];
    bool live[DJ_EVAL_PR_GROUP];
#pragma unroll
    for (int g = 0; g < DJ_EVAL_PR_GROUP; ++g) {
      live[g] = j0 + g < n_points;
      thr[g] = live[g] ? s_thr[j0 + g] : 0.0;
      m[g] = 0.0;                // precision is never negative: the maximum over nothing, 0.0, is the start value
    }
    for (int i = b0 + tid; i < b1; i += DJ_EVAL_PR_THREADS) {
      const double r = recall[i], pr = precision[i];
#pragma unroll
      for (int g = 0; g < DJ_EVAL_PR_GROUP; ++g)
        if (live[g] && r >= thr[g] && pr > m[g]) m[g] = pr;
    }
#pragma unroll
    for (int g = 0; g < DJ_EVAL_PR_GROUP; ++g) {
      double v = m[g];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        if (ov > v) v = ov;
      }
      if (lane == 0) s_red[g][wave] = v;
    }
    __syncthreads();
    if (tid < DJ_EVAL_PR_GROUP && j0 + tid < n_points) {
      double v = s_red[tid][0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w)
        if (s_red[tid][w] > v) v = s_red[tid][w];
      s_max[j0 + tid] = v;
    }
    __syncthreads();
  }
  if (tid == 0) {
    double a = 0.0;
    for (int j = 0; j < n_points; ++j) a = a + s_max[j];
    ap[cls] = a / (double)n_points;
  }
}

extern "C" int dj_eval_precision_recall_ap(const int* tp, const int* fp, const int* class_offsets, int n_classes, int n_pred,
                                           const double* num_gt, const double* thresholds, int num_recall_points,
                                           int* cum_tp, int* cum_fp, double* precision, double* recall, double* ap,
                                           void* stream) {
  DJ_CHECK_ARG(n_classes >= 1 && n_pred >= 0, "eval_precision_recall_ap: bad sizes");
  DJ_CHECK_ARG(num_recall_points >= 1 && num_recall_points <= DJ_EVAL_MAX_POINTS,
               "eval_precision_recall_ap: num_recall_points must be 1..%d", DJ_EVAL_MAX_POINTS);
  DJ_CHECK_ARG(class_offsets && num_gt && thresholds && ap, "eval_precision_recall_ap: null tensor");
  DJ_CHECK_ARG(n_pred == 0 || (tp && fp && cum_tp && cum_fp && precision && recall), "eval_precision_recall_ap: null tensor");
  hipLaunchKernelGGL(dj_eval_pr_ap_kernel, dim3(n_classes), dim3(DJ_EVAL_PR_THREADS), 0, (hipStream_t)stream, tp, fp,
                     class_offsets, n_pred, num_gt, thresholds, num_recall_points, cum_tp, cum_fp, precision, recall, ap);
  DJ_CHECK_LAUNCH("dj_eval_precision_recall_ap");
  return DJ_OK;
}
