// Pascal-VOC evaluation on device, the stages in front of dj_eval_match (dj_eval.hip): the decoded batches of the
// DecodeDetections layer are collected into flat record arrays (dj_eval_collect, one launch per batch), and the records are
// ranked and segmented into the arrays of eval_utils/device_matching.py:PackedEvaluation (dj_eval_rank).  Restates the loop
// of `Evaluator.predict_on_dataset` (padding mask, the inverse of `Resize`, `round(float(v), 1)`) and the prediction half
// of `pack_evaluation`; `collect_host` / `rank_host` of device_matching.py state the same in numpy.  Every output is an
// integer or a float whose bits are determined, and nothing here synchronises with the host: the number of records lives
// in counters[0] on the device, and every grid is sized by the capacity.
#include "../../include/dj_hip.h"
#include "dj_common.h"

// the resize product is rounded to float32 before rintf, the decimal rounding's product before rint (numpy, op by op)
#pragma clang fp contract(off)

#define DJ_EVC_THREADS 256
#define DJ_EVC_MAX_BATCH 128     // descriptors travel by value in the kernel arguments
#define DJ_EVC_TILE 1024         // keys sorted in LDS by one block (8 KB)

typedef unsigned long long ev_u64;

struct DjEvalCollectParams {
  const float* decoded;
  int* rec_class;
  int* rec_image;
  int* rec_ordinal;
  float* rec_conf;
  double* rec_conf64;
  float* rec_boxes;
  int* counters;
  double conf_scale;             // 10^conf_digits
  int rows, n_valid, first_ordinal, n_classes, conf_digits, boxes_final, capacity;
  dj_eval_collect_desc desc[DJ_EVC_MAX_BATCH];
};

// exclusive scan of `v` over the block's DJ_EVC_THREADS threads (all of them call it); *total = the block's sum
__device__ __forceinline__ int ev_block_scan(int v, int* s_wave, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < DJ_EVC_THREADS / 64; ++w) {
    if (w < wave) off += s_wave[w];
    tot += s_wave[w];
  }
  __syncthreads();               // s_wave is free for the next call
  *total = tot;
  return off + inc - v;
}

// CPython's round(float(v), d) of a float32 v, d <= 8: scale * v is exact in a double, rint is half-even, one division
__device__ __forceinline__ double ev_round_decimal(float v, double scale) { return rint(scale * (double)v) / scale; }

// One block: the batch's rows in their order, the kept ones appended behind counters[0] (a stable compaction in chunks of
// DJ_EVC_THREADS rows with a carry).  The next launch on the stream continues where this one stopped.
__global__ __launch_bounds__(DJ_EVC_THREADS) void dj_eval_collect_kernel(DjEvalCollectParams p) {
  __shared__ int s_wave[DJ_EVC_THREADS / 64];
  const int tid = threadIdx.x;
  const int total = p.n_valid * p.rows;
  int base = p.counters[0];
  int errors = 0, dropped = 0;
  const float max_class = (float)p.n_classes;
  for (int c0 = 0; c0 < total; c0 += DJ_EVC_THREADS) {
    const int i = c0 + tid;
    bool keep = false;
    const float* row = p.decoded + (size_t)(i < total ? i : 0) * 6;
    float cls_f = 0.f;
    if (i < total) {
      cls_f = row[0];
      if (cls_f != 0.f) {        // the host's padding mask: a NaN class id is not padding
        keep = cls_f == floorf(cls_f) && cls_f >= 1.f && cls_f <= max_class;
        if (!keep) ++errors;
      }
    }
    int chunk = 0;
    const int slot = base + ev_block_scan(keep ? 1 : 0, s_wave, &chunk);
    if (keep) {
      if (slot < p.capacity) {
        const int img = i / p.rows;
        const dj_eval_collect_desc d = p.desc[img];
        float x0 = row[2], y0 = row[3], x1 = row[4], y1 = row[5];
        if (!p.boxes_final) {
          if (d.kind == 1) {     // Resize's inverter: np.round(labels * float32(scale), 0) on the float32 array
            y0 = rintf(y0 * d.scale_y);
            y1 = rintf(y1 * d.scale_y);
            x0 = rintf(x0 * d.scale_x);
            x1 = rintf(x1 * d.scale_x);
          }
          x0 = (float)ev_round_decimal(x0, 10.0);
          y0 = (float)ev_round_decimal(y0, 10.0);
          x1 = (float)ev_round_decimal(x1, 10.0);
          y1 = (float)ev_round_decimal(y1, 10.0);
        }
        const float conf = row[1];
        const double conf64 = p.conf_digits > 0 ? ev_round_decimal(conf, p.conf_scale) : (double)conf;
        p.rec_class[slot] = (int)cls_f;
        p.rec_image[slot] = d.image_index;
        p.rec_ordinal[slot] = p.first_ordinal + img;
        p.rec_conf[slot] = p.conf_digits > 0 ? (float)conf64 : conf;
        p.rec_conf64[slot] = conf64;
        float* b = p.rec_boxes + (size_t)slot * 4;
        b[0] = x0, b[1] = y0, b[2] = x1, b[3] = y1;
      } else {
        ++dropped;               // the host's capacity check makes this unreachable; never write past the arrays
      }
    }
    base += chunk;
  }
  if (errors) atomicAdd(&p.counters[1], errors);
  if (dropped) atomicAdd(&p.counters[3], dropped);
  if (tid == 0) p.counters[0] = base < p.capacity ? base : p.capacity;
}

extern "C" int dj_eval_collect(const float* decoded, int batch, int rows, int n_valid, const dj_eval_collect_desc* desc_host,
                               int first_ordinal, int n_classes, int n_images, int conf_digits, int boxes_final,
                               int* rec_class, int* rec_image, int* rec_ordinal, float* rec_conf, double* rec_conf64,
                               float* rec_boxes, long capacity, int* counters, void* stream) {
  DJ_CHECK_ARG(batch >= 0 && rows >= 1 && n_valid >= 0 && n_valid <= batch, "eval_collect: bad sizes");
  DJ_CHECK_ARG(n_classes >= 1 && n_images >= 0 && first_ordinal >= 0, "eval_collect: bad sizes");
  DJ_CHECK_ARG(conf_digits >= 0 && conf_digits <= 8, "eval_collect: conf_digits must be 0..8");
  DJ_CHECK_ARG(capacity >= 1 && capacity < 2147483647L, "eval_collect: capacity must be 1..2^31-2");
  // every earlier image appended at most `rows` records: with this bound the arrays cannot overflow
  DJ_CHECK_ARG(((long)first_ordinal + n_valid) * rows <= capacity,
               "eval_collect: %ld records may not fit the capacity %ld", ((long)first_ordinal + n_valid) * rows, capacity);
  if (n_valid == 0) return DJ_OK;
  DJ_CHECK_ARG(decoded && desc_host && rec_class && rec_image && rec_ordinal && rec_conf && rec_conf64 && rec_boxes && counters,
               "eval_collect: null tensor");
  for (int k = 0; k < n_valid; ++k) {
    DJ_CHECK_ARG(desc_host[k].kind == 0 || desc_host[k].kind == 1, "eval_collect: image %d: unknown transform %d", k,
                 desc_host[k].kind);
    DJ_CHECK_ARG(desc_host[k].image_index >= 0 && desc_host[k].image_index < n_images,
                 "eval_collect: image %d: index %d outside the dataset", k, desc_host[k].image_index);
  }
  DjEvalCollectParams p;
  p.rec_class = rec_class;
  p.rec_image = rec_image;
  p.rec_ordinal = rec_ordinal;
  p.rec_conf = rec_conf;
  p.rec_conf64 = rec_conf64;
  p.rec_boxes = rec_boxes;
  p.counters = counters;
  p.conf_scale = 1.0;
  for (int k = 0; k < conf_digits; ++k) p.conf_scale *= 10.0;     // exact
  p.rows = rows;
  p.n_classes = n_classes;
  p.conf_digits = conf_digits;
  p.boxes_final = boxes_final ? 1 : 0;
  p.capacity = (int)capacity;
  // one launch per batch of up to DJ_EVC_MAX_BATCH images; a larger batch is appended piece by piece, in order
  for (int k0 = 0; k0 < n_valid; k0 += DJ_EVC_MAX_BATCH) {
    const int nb = n_valid - k0 < DJ_EVC_MAX_BATCH ? n_valid - k0 : DJ_EVC_MAX_BATCH;
    DJ_CHECK_ARG((long)nb * rows < 2147483647L, "eval_collect: too many rows per launch");
    p.decoded = decoded + (size_t)k0 * rows * 6;
    p.n_valid = nb;
    p.first_ordinal = first_ordinal + k0;
    for (int k = 0; k < DJ_EVC_MAX_BATCH; ++k) p.desc[k] = desc_host[k0 + (k < nb ? k : 0)];
    hipLaunchKernelGGL(dj_eval_collect_kernel, dim3(1), dim3(DJ_EVC_THREADS), 0, (hipStream_t)stream, p);
    DJ_CHECK_LAUNCH("dj_eval_collect");
  }
  return DJ_OK;
}

// ---- dj_eval_rank ------------------------------------------------------------------------------------------------------------
// Three sorts of unique 64-bit keys whose low word is the position the key was made at:
//   1. (descending-order confidence key, list position)      -> the global rank r of every record
//   2. (class, r)                                            -> the predictions, class after class in rank order
//   3. (class * n_images + image, prediction position p)     -> the segments, ranks increasing inside each
// Unique keys make every correct sort give the one answer.  A sort is a bitonic sort of tiles in LDS and merge passes in
// which every key finds its place by a binary search in the neighbouring run.

// confidence -> a key that ascends as the confidence descends; -0.0 and 0.0 are one confidence
__device__ __forceinline__ unsigned ev_conf_key(float conf) {
  unsigned u = conf == 0.f ? 0u : __float_as_uint(conf);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~u;
}

__global__ __launch_bounds__(DJ_EVC_THREADS) void dj_eval_rank_keys_kernel(const int* __restrict__ rec_class,
                                                                           const float* __restrict__ rec_conf,
                                                                           int* counters, int* class_counts, int n_classes,
                                                                           ev_u64* __restrict__ keys) {
  const int n = counters[0];
  const int i = blockIdx.x * DJ_EVC_THREADS + threadIdx.x;
  if (i >= n) return;
  const float conf = rec_conf[i];
  int cls = rec_class[i];
  bool bad = conf != conf;                                   // a NaN confidence has no rank
  if (cls < 1 || cls > n_classes) {                          // records not made by dj_eval_collect: stay in bounds
    bad = true;
    cls = cls < 1 ? 1 : n_classes;
  }
  if (bad) atomicAdd(&counters[1], 1);
  atomicAdd(&class_counts[cls], 1);
  keys[i] = ((ev_u64)ev_conf_key(conf) << 32) | (unsigned)i;
}

__global__ __launch_bounds__(DJ_EVC_THREADS) void dj_eval_rank_tile_sort_kernel(ev_u64* keys, const int* counters) {
  __shared__ ev_u64 s[DJ_EVC_TILE];
  const int n = counters[0];
  const int t0 = blockIdx.x * DJ_EVC_TILE;
  if (t0 >= n) return;                                       // uniform over the block
  for (int k = threadIdx.x; k < DJ_EVC_TILE; k += DJ_EVC_THREADS)
    s[k] = t0 + k < n ? keys[t0 + k] : ~0ull;                // no key is all ones: its low word is a position < 2^31
  __syncthreads();
  for (int k = 2; k <= DJ_EVC_TILE; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < DJ_EVC_TILE / 2; t += DJ_EVC_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int l = i | j;
        const bool up = (i & k) == 0;
        const ev_u64 a = s[i], b = s[l];
        if ((a > b) == up) {
          s[i] = b;
          s[l] = a;
        }
      }
      __syncthreads();
    }
  }
  for (int k = threadIdx.x; k < DJ_EVC_TILE; k += DJ_EVC_THREADS)
    if (t0 + k < n) keys[t0 + k] = s[k];
}

// runs of `run` keys, sorted: [s, mid) and [mid, e) are merged into out[s, e)
__global__ __launch_bounds__(DJ_EVC_THREADS) void dj_eval_rank_merge_kernel(const ev_u64* __restrict__ in,
                                                                            ev_u64* __restrict__ out, const int* counters,
                                                                            long run) {
  const long n = counters[0];
  const long i = (long)blockIdx.x * DJ_EVC_THREADS + threadIdx.x;
  if (i >= n) return;
  const long s = i / (2 * run) * (2 * run);
  const long mid = s + run < n ? s + run : n;
  const long e = s + 2 * run < n ? s + 2 * run : n;
  const ev_u64 key = in[i];
  long lo, hi, own;
  if (i < mid) {
    lo = mid, hi = e, own = i - s;
  } else {
    lo = s, hi = mid, own = i - mid;
  }
  const long first = lo;
  while (lo < hi) {                                          // the keys of the other run below this one
    const long m = (lo + hi) >> 1;
    if (in[m] < key)
      lo = m + 1;
    else
      hi = m;
  }
  out[s + own + (lo - first)] = key;
}

__global__ __launch_bounds__(DJ_EVC_THREADS) void dj_eval_rank_class_keys_kernel(const ev_u64* __restrict__ by_conf,
                                                                                 const int* __restrict__ rec_class,
                                                                                 const int* counters, int n_classes,
                                                                                 ev_u64* __restrict__ keys) {
  const int n = counters[0];
  const int r = blockIdx.x * DJ_EVC_THREADS + threadIdx.x;
  if (r >= n) return;
  const int i = (int)(unsigned)by_conf[r];
  int cls = rec_class[i];
  cls = cls < 1 ? 1 : (cls > n_classes ? n_classes : cls);
  keys[r] = ((ev_u64)(unsigned)cls << 32) | (unsigned)r;
}

struct DjEvalGatherParams {
  const ev_u64* by_conf;
  const ev_u64* by_class;
  const int* rec_class;
  const int* rec_image;
  const float* rec_conf;
  const float* rec_boxes;
  const int* counters;
  const int* class_counts;
  int* class_offsets;
  int* pred_class;
  int* pred_image;
  float* pred_conf;
  float* pred_boxes;
  ev_u64* keys;
  int n_classes, n_images;
};

__global__ __launch_bounds__(DJ_EVC_THREADS) void dj_eval_rank_gather_kernel(DjEvalGatherParams p) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {                 // also when there is no record at all
    int sum = 0;
    p.class_offsets[0] = 0;
    for (int c = 1; c <= p.n_classes + 1; ++c) {
      p.class_offsets[c] = sum;
      if (c <= p.n_classes) sum += p.class_counts[c];
    }
  }
  const int n = p.counters[0];
  const int q = blockIdx.x * DJ_EVC_THREADS + threadIdx.x;
  if (q >= n) return;
  const int r = (int)(unsigned)p.by_class[q];
  const int i = (int)(unsigned)p.by_conf[r];
  int cls = p.rec_class[i], img = p.rec_image[i];
  p.pred_class[q] = cls;
  p.pred_image[q] = img;
  p.pred_conf[q] = p.rec_conf[i];
  const float* b = p.rec_boxes + (size_t)i * 4;
  float* o = p.pred_boxes + (size_t)q * 4;
  o[0] = b[0], o[1] = b[1], o[2] = b[2], o[3] = b[3];
  cls = cls < 1 ? 1 : (cls > p.n_classes ? p.n_classes : cls);
  img = img < 0 ? 0 : (img >= p.n_images ? p.n_images - 1 : img);
  p.keys[q] = ((ev_u64)(unsigned)(cls * p.n_images + img) << 32) | (unsigned)q;
}

// is position q of the keys sorted by (class, image) the first of its segment?
__device__ __forceinline__ bool ev_segment_head(const ev_u64* keys, int q) {
  return q == 0 || (keys[q] >> 32) != (keys[q - 1] >> 32);
}

__global__ __launch_bounds__(DJ_EVC_THREADS) void dj_eval_rank_seg_count_kernel(const ev_u64* __restrict__ keys,
                                                                                const int* counters, int* block_sums) {
  __shared__ int s_wave[DJ_EVC_THREADS / 64];
  const int n = counters[0];
  const int q = blockIdx.x * DJ_EVC_THREADS + threadIdx.x;
  int total = 0;
  ev_block_scan(q < n && ev_segment_head(keys, q) ? 1 : 0, s_wave, &total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// one block: the blocks' counts -> their exclusive sums, in place; the total is the number of segments
__global__ __launch_bounds__(DJ_EVC_THREADS) void dj_eval_rank_seg_scan_kernel(int* block_sums, int n_blocks, int* counters,
                                                                               int* seg_offsets) {
  __shared__ int s_wave[DJ_EVC_THREADS / 64];
  int carry = 0;
  for (int b0 = 0; b0 < n_blocks; b0 += DJ_EVC_THREADS) {
    const int b = b0 + threadIdx.x;
    const int v = b < n_blocks ? block_sums[b] : 0;
    int chunk = 0;
    const int ex = ev_block_scan(v, s_wave, &chunk);
    if (b < n_blocks) block_sums[b] = carry + ex;
    carry += chunk;
  }
  if (threadIdx.x == 0) {
    counters[2] = carry;
    seg_offsets[carry] = counters[0];
  }
}

__global__ __launch_bounds__(DJ_EVC_THREADS) void dj_eval_rank_seg_write_kernel(
    const ev_u64* __restrict__ keys, const int* counters, const int* __restrict__ block_sums,
    const int* __restrict__ class_offsets, int n_images, int* __restrict__ seg_class, int* __restrict__ seg_image,
    int* __restrict__ seg_offsets, int* __restrict__ seg_ranks) {
  __shared__ int s_wave[DJ_EVC_THREADS / 64];
  const int n = counters[0];
  const int q = blockIdx.x * DJ_EVC_THREADS + threadIdx.x;
  const bool head = q < n && ev_segment_head(keys, q);
  int total = 0;
  const int seg = block_sums[blockIdx.x] + ev_block_scan(head ? 1 : 0, s_wave, &total);
  if (q >= n) return;
  const ev_u64 key = keys[q];
  const int pair = (int)(key >> 32), pos = (int)(unsigned)key;
  const int cls = pair / n_images;
  seg_ranks[q] = pos - class_offsets[cls];
  if (head) {
    seg_class[seg] = cls;
    seg_image[seg] = pair - cls * n_images;
    seg_offsets[seg] = q;
  }
}

static long ev_align(long v) { return (v + 255) / 256 * 256; }

extern "C" long dj_eval_rank_workspace_bytes(long capacity, int n_classes) {
  if (capacity < 1 || n_classes < 1) return 0;
  return 4 * ev_align(capacity * 8) + ev_align(((long)n_classes + 2) * 4) + ev_align(((capacity + DJ_EVC_THREADS - 1) / DJ_EVC_THREADS) * 4);
}

// tiles, then merge passes until one run covers the capacity: `a` holds the keys, `b` is scratch; -> the sorted buffer
static ev_u64* ev_sort(ev_u64* a, ev_u64* b, long capacity, const int* counters, hipStream_t stream) {
  hipLaunchKernelGGL(dj_eval_rank_tile_sort_kernel, dim3(dj_cdiv(capacity, DJ_EVC_TILE)), dim3(DJ_EVC_THREADS), 0, stream, a,
                     counters);
  for (long run = DJ_EVC_TILE; run < capacity; run *= 2) {
    hipLaunchKernelGGL(dj_eval_rank_merge_kernel, dim3(dj_cdiv(capacity, DJ_EVC_THREADS)), dim3(DJ_EVC_THREADS), 0, stream, a, b,
                       counters, run);
    ev_u64* t = a;
    a = b;
    b = t;
  }
  return a;
}

extern "C" int dj_eval_rank(const int* rec_class, const int* rec_image, const float* rec_conf, const float* rec_boxes,
                            long capacity, int n_classes, int n_images, int* counters, int* class_offsets, int* pred_class,
                            int* pred_image, float* pred_conf, float* pred_boxes, int* seg_class, int* seg_image,
                            int* seg_offsets, int* seg_ranks, void* workspace, long workspace_bytes, void* stream) {
  DJ_CHECK_ARG(capacity >= 1 && capacity < 2147483647L, "eval_rank: capacity must be 1..2^31-2");
  DJ_CHECK_ARG(n_classes >= 1 && n_images >= 1, "eval_rank: bad sizes");
  DJ_CHECK_ARG(((long)n_classes + 1) * n_images < 2147483647L, "eval_rank: (n_classes + 1) * n_images must stay below 2^31");
  DJ_CHECK_ARG(rec_class && rec_image && rec_conf && rec_boxes && counters && class_offsets && pred_class && pred_image &&
                   pred_conf && pred_boxes && seg_class && seg_image && seg_offsets && seg_ranks && workspace,
               "eval_rank: null tensor");
  DJ_CHECK_ARG(workspace_bytes >= dj_eval_rank_workspace_bytes(capacity, n_classes) && ((uintptr_t)workspace & 7) == 0,
               "eval_rank: workspace too small or misaligned (need %ld bytes)", dj_eval_rank_workspace_bytes(capacity, n_classes));
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)workspace;
  ev_u64* buf[4];
  for (int k = 0; k < 4; ++k) buf[k] = (ev_u64*)(w + k * ev_align(capacity * 8));
  int* class_counts = (int*)(w + 4 * ev_align(capacity * 8));
  int* block_sums = (int*)((char*)class_counts + ev_align(((long)n_classes + 2) * 4));
  const int n_blocks = dj_cdiv(capacity, DJ_EVC_THREADS);
  const dim3 grid(n_blocks), block(DJ_EVC_THREADS);
  if (hipMemsetAsync(class_counts, 0, ((size_t)n_classes + 2) * 4, st) != hipSuccess) {
    dj_set_error("eval_rank: hipMemsetAsync failed");
    return DJ_ERR_HIP;
  }
  hipLaunchKernelGGL(dj_eval_rank_keys_kernel, grid, block, 0, st, rec_class, rec_conf, counters, class_counts, n_classes,
                     buf[0]);
  ev_u64* by_conf = ev_sort(buf[0], buf[1], capacity, counters, st);
  ev_u64* spare1 = by_conf == buf[0] ? buf[1] : buf[0];
  hipLaunchKernelGGL(dj_eval_rank_class_keys_kernel, grid, block, 0, st, by_conf, rec_class, counters, n_classes, buf[2]);
  ev_u64* by_class = ev_sort(buf[2], buf[3], capacity, counters, st);
  ev_u64* spare2 = by_class == buf[2] ? buf[3] : buf[2];
  DjEvalGatherParams g;
  g.by_conf = by_conf;
  g.by_class = by_class;
  g.rec_class = rec_class;
  g.rec_image = rec_image;
  g.rec_conf = rec_conf;
  g.rec_boxes = rec_boxes;
  g.counters = counters;
  g.class_counts = class_counts;
  g.class_offsets = class_offsets;
  g.pred_class = pred_class;
  g.pred_image = pred_image;
  g.pred_conf = pred_conf;
  g.pred_boxes = pred_boxes;
  g.keys = spare1;
  g.n_classes = n_classes;
  g.n_images = n_images;
  hipLaunchKernelGGL(dj_eval_rank_gather_kernel, grid, block, 0, st, g);
  // by_conf and by_class are read for the last time above: sort 3 may use both spare buffers
  ev_u64* by_segment = ev_sort(spare1, spare2, capacity, counters, st);
  hipLaunchKernelGGL(dj_eval_rank_seg_count_kernel, grid, block, 0, st, by_segment, counters, block_sums);
  hipLaunchKernelGGL(dj_eval_rank_seg_scan_kernel, dim3(1), block, 0, st, block_sums, n_blocks, counters, seg_offsets);
  hipLaunchKernelGGL(dj_eval_rank_seg_write_kernel, grid, block, 0, st, by_segment, counters, block_sums, class_offsets, n_images,
                     seg_class, seg_image, seg_offsets, seg_ranks);
  DJ_CHECK_LAUNCH("dj_eval_rank");
  return DJ_OK;
}
