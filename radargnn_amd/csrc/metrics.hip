// Evaluation metrics on the device: what the reference's evaluators compute after the post-processor.
//   aligned box IoU (torchvision.ops.box_iou)          postprocessor/torchmetrics_mean_ap.py:114
//   greedy matching of detections to ground truth       postprocessor/torchmetrics_mean_ap.py:505-551, 612-747
//   recall / precision / score tables of the mAP        postprocessor/torchmetrics_mean_ap.py:898-973
//   confusion matrix of the node labels                 postprocessor/metrics.py:136-196
// Everything is packed over the whole list of frames with int64 offset arrays (the layout of rgnn_point_iou); no kernel
// is launched per frame or per class.  Only the area range "all" exists: no ground-truth box and no detection is ever
// "ignored" (true for finite boxes; the COCO pixel ranges small / medium / large mean nothing in metres).
//
// UNPINNED: the box IoU restates torchvision.ops.box_iou from its documented formula; it was never executed against
// torchvision (the restatement it is compared with bit for bit is held to a float64 evaluation of the same geometry).
// The reference orders equal scores with an unstable torch.sort.  This project decides, and tests/test_gpu_metrics_edges.py
// holds it: the order is that of torch.sort(descending, stable) -- NaN first, -0.0 and 0.0 tie, ties by ascending position.
// The file is built with -ffp-contract=off like the rest of the library: no fused multiply-adds.
#include "common.h"
#include <math.h>

namespace {

// index f of the segment of ptr [n_seg + 1] (ascending) that holds position x; the last such f when empty segments share it
__device__ __forceinline__ int64_t segment_of(const int64_t* __restrict__ ptr, int64_t n_seg, int64_t x) {
  int64_t lo = 0, hi = n_seg;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (ptr[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------------------------------------------------------------
// a. Aligned box IoU, one lane per pair, float32 throughout:
//    inter = clamp(min(x2) - max(x1), 0) * clamp(min(y2) - max(y1), 0);  iou = inter / (area_p + area_g - inter)
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_box_iou(const float* __restrict__ bp, const int64_t* __restrict__ pred_ptr,
                                                const float* __restrict__ bg, const int64_t* __restrict__ gt_ptr, int64_t n_frames,
                                                const int64_t* __restrict__ out_ptr, int64_t total, float* __restrict__ iou) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int64_t f = segment_of(out_ptr, n_frames, t);
  const int64_t g_count = gt_ptr[f + 1] - gt_ptr[f];
  const int64_t local = t - out_ptr[f];
  const float* a = bp + (pred_ptr[f] + local / g_count) * 4;
  const float* b = bg + (gt_ptr[f] + local % g_count) * 4;
  const float area_a = (a[2] - a[0]) * (a[3] - a[1]);
  const float area_b = (b[2] - b[0]) * (b[3] - b[1]);
  const float w = fminf(a[2], b[2]) - fmaxf(a[0], b[0]);
  const float h = fminf(a[3], b[3]) - fmaxf(a[1], b[1]);
  const float inter = (w > 0.0f ? w : 0.0f) * (h > 0.0f ? h : 0.0f);
  iou[t] = inter / ((area_a + area_b) - inter);
}

// ------------------------------------------------------------------------------------------------------------------
// b. Greedy matching.  One wave per (frame, class).  The class's detections and ground-truth boxes of the frame are
//    compacted into LDS (in frame order), the detections ranked by descending score (ties by position; NaN first, -0.0 and
//    0.0 tie: the key of rgnn_sort_scores), and for every threshold the first max_det of them walk through the ground truth
//    in rank order: lanes across the ground-truth boxes, value = 0 for a matched box and the IoU otherwise, wave argmax
//    (lowest position on ties), matched iff the maximum is strictly greater than the threshold.  A NaN IoU anywhere in the
//    detection's row of the class leaves it unmatched (argmax returns the NaN, and NaN > t is false).
//    A (frame, class) list longer than MATCH_CAP does nothing but set bit 0 of *status: the host refuses the call.
// ------------------------------------------------------------------------------------------------------------------
constexpr int MATCH_CAP = 2048;                               // boxes of one class in one frame (predicted; ground truth)

__device__ __forceinline__ unsigned score_key32(float v) {
  if (v != v) return 0xffffffffu;
  if (v == 0.0f) v = 0.0f;
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct MatchParams {
  const void* iou;
  int iou_is_f32;
  const int64_t *pred_ptr, *gt_ptr, *out_ptr;
  const int32_t* det_labels;
  const float* det_scores;
  int64_t n_pred;
  const int32_t* gt_labels;
  const int32_t* classes;
  int n_classes;
  const double* thresholds;
  int n_thresholds, max_det;
  int32_t* rank;
  unsigned char* matched;
  int32_t* status;
};

__global__ __launch_bounds__(64) void k_map_match(MatchParams p) {
  __shared__ int det_idx[MATCH_CAP];
  __shared__ unsigned det_key[MATCH_CAP];
  __shared__ int det_ord[MATCH_CAP];
  __shared__ int gt_idx[MATCH_CAP];
  __shared__ unsigned char gt_used[MATCH_CAP];
  const int lane = threadIdx.x;
  const int64_t f = blockIdx.x / p.n_classes;
  const int32_t c = p.classes[blockIdx.x % p.n_classes];
  const int64_t p0 = p.pred_ptr[f], g0 = p.gt_ptr[f];
  const int np = (int)(p.pred_ptr[f + 1] - p0), ng_all = (int)(p.gt_ptr[f + 1] - g0);
  const unsigned long long below = (1ull << lane) - 1ull;
  int nd = 0;
  for (int base = 0; base < np; base += 64) {
    const int i = base + lane;
    const bool is = i < np && p.det_labels[p0 + i] == c;
    const unsigned long long m = __ballot(is);
    const int slot = nd + __popcll(m & below);
    if (is && slot < MATCH_CAP) {
      det_idx[slot] = i;
      det_key[slot] = score_key32(p.det_scores[p0 + i]);
    }
    nd += __popcll(m);
  }
  if (nd == 0) return;                                        // (the whole wave)
  int ng = 0;
  for (int base = 0; base < ng_all; base += 64) {
    const int i = base + lane;
    const bool is = i < ng_all && p.gt_labels[g0 + i] == c;
    const unsigned long long m = __ballot(is);
    const int slot = ng + __popcll(m & below);
    if (is && slot < MATCH_CAP) gt_idx[slot] = i;
    ng += __popcll(m);
  }
  if (nd > MATCH_CAP || ng > MATCH_CAP) {                     // over capacity: nothing was written past the arrays
    if (lane == 0) atomicOr(p.status, 1);
    return;
  }
  __syncthreads();
  for (int a = lane; a < nd; a += 64) {
    const unsigned ka = det_key[a];
    int r = 0;
    for (int b = 0; b < nd; b++) {
      const unsigned kb = det_key[b];
      r += (kb > ka || (kb == ka && b < a)) ? 1 : 0;
    }
    p.rank[p0 + det_idx[a]] = r < p.max_det ? r : -1;
    det_ord[r] = det_idx[a];
  }
  __syncthreads();
  if (ng == 0) return;
  const int n_use = nd < p.max_det ? nd : p.max_det;
  const int64_t m0 = p.out_ptr[f];
  for (int t = 0; t < p.n_thresholds; t++) {
    const double thr = p.iou_is_f32 ? (double)(float)p.thresholds[t] : p.thresholds[t];
    for (int g = lane; g < ng; g += 64) gt_used[g] = 0;
    __syncthreads();
    for (int d = 0; d < n_use; d++) {
      const int64_t row = m0 + (int64_t)det_ord[d] * ng_all;
      double best = -1.0;
      int pos = 0x7fffffff;
      bool nan = false;
      for (int g = lane; g < ng; g += 64) {
        const double raw = p.iou_is_f32 ? (double)((const float*)p.iou)[row + gt_idx[g]] : ((const double*)p.iou)[row + gt_idx[g]];
        nan = nan || raw != raw;
        const double v = gt_used[g] ? 0.0 : raw;
        if (v > best) { best = v; pos = g; }
      }
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {
        const double ob = __shfl_xor(best, s);
        const int op = __shfl_xor(pos, s);
        if (ob > best || (ob == best && op < pos)) { best = ob; pos = op; }
      }
      const bool hit = !__any(nan) && pos < ng && best > thr;
      if (hit && lane == 0) {
        gt_used[pos] = 1;
        p.matched[(int64_t)t * p.n_pred + p0 + det_ord[d]] = 1;
      }
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// c. Curves.  One block per (class, threshold, max_det).  `order` lists the detections class by class (cls_ptr [2, K]: where
//    each class begins and ends in it), inside a class by descending score (stable, so equal scores go by frame, then rank); a block
//    reads its own class's segment only.  The block counts the class's ground truth (npig), its selected
//    detections (rank < max_det) and their matches, then walks the order from the END: the counts left of a detection are the
//    totals minus the counts right of it, the precision envelope is the running maximum from the right, and the detection
//    that raises tp to c serves every recall threshold r with fl((c - 1) / npig) < r <= fl(c / npig) -- the first index with
//    rc >= r (searchsorted, right = False); the first selected detection also serves every r <= its own recall.  Thresholds no
//    detection serves keep precision 0 and score 0.  Recall thresholds must ascend.
// ------------------------------------------------------------------------------------------------------------------
constexpr int CURVE_THREADS = 256;
constexpr int CURVE_MAX_REC = 1024;

struct CurveParams {
  const int64_t* order;
  const int64_t* cls_ptr;
  const int32_t* det_labels;
  const float* det_scores;
  const int32_t* rank;
  const unsigned char* matched;
  int64_t n_pred;
  const int32_t* gt_labels;
  int64_t n_gt;
  const int32_t* classes;
  int n_classes;
  int n_thresholds;
  const int32_t* max_dets;
  int n_max_dets;
  const float* rec;
  int n_rec;
  float *precision, *scores, *recall;
};

__global__ __launch_bounds__(CURVE_THREADS) void k_map_curves(CurveParams p) {
  __shared__ float s_prec[CURVE_MAX_REC], s_score[CURVE_MAX_REC];
  __shared__ int s_tp[CURVE_THREADS], s_n[CURVE_THREADS];
  __shared__ float s_mx[CURVE_THREADS];
  __shared__ int s_count[3];
  const int tid = threadIdx.x;
  const int im = blockIdx.x % p.n_max_dets;
  const int it = (blockIdx.x / p.n_max_dets) % p.n_thresholds;
  const int ik = blockIdx.x / (p.n_max_dets * p.n_thresholds);
  const int32_t c = p.classes[ik];
  const int max_det = p.max_dets[im];
  const unsigned char* matched = p.matched + (int64_t)it * p.n_pred;
  if (tid < 3) s_count[tid] = 0;
  for (int r = tid; r < p.n_rec; r += CURVE_THREADS) { s_prec[r] = 0.0f; s_score[r] = 0.0f; }
  __syncthreads();
  int my_g = 0, my_n = 0, my_tp = 0;
  for (int64_t g = tid; g < p.n_gt; g += CURVE_THREADS) my_g += p.gt_labels[g] == c;
  const int64_t seg_lo = p.cls_ptr[ik], seg_n = p.cls_ptr[p.n_classes + ik] - seg_lo;
  const int64_t* order = p.order + seg_lo;
  for (int64_t i = tid; i < seg_n; i += CURVE_THREADS) {
    const int64_t id = order[i];
    const int rk = p.rank[id];
    const bool sel = p.det_labels[id] == c && rk >= 0 && rk < max_det;
    my_n += sel;
    my_tp += sel && matched[id];
  }
  if (my_g) atomicAdd(&s_count[0], my_g);
  if (my_n) atomicAdd(&s_count[1], my_n);
  if (my_tp) atomicAdd(&s_count[2], my_tp);
  __syncthreads();
  const int npig = s_count[0], n_sel = s_count[1], tp_total = s_count[2];
  const int64_t cell = ((int64_t)ik) * p.n_max_dets + im;                        // [.., K, M]
  const int64_t stride_r = (int64_t)p.n_classes * p.n_max_dets;
  float* out_p = p.precision + (int64_t)it * p.n_rec * stride_r + cell;
  float* out_s = p.scores + (int64_t)it * p.n_rec * stride_r + cell;
  float* out_r = p.recall + (int64_t)it * stride_r + cell;
  if (npig == 0) {                                                               // no ground truth of the class: all stay -1
    for (int r = tid; r < p.n_rec; r += CURVE_THREADS) { out_p[r * stride_r] = -1.0f; out_s[r * stride_r] = -1.0f; }
    if (tid == 0) *out_r = -1.0f;
    return;
  }
  const float npig_f = (float)npig;
  int carry_tp = 0, carry_n = 0;
  float carry_mx = -1.0f;
  for (int64_t base = 0; base < seg_n && carry_n < n_sel; base += CURVE_THREADS) {
    const int64_t j = base + tid;
    int64_t id = 0;
    bool sel = false, tpf = false;
    if (j < seg_n) {
      id = order[seg_n - 1 - j];
      const int rk = p.rank[id];
      sel = p.det_labels[id] == c && rk >= 0 && rk < max_det;
      tpf = sel && matched[id];
    }
    s_tp[tid] = tpf; s_n[tid] = sel;
    __syncthreads();
    for (int s = 1; s < CURVE_THREADS; s <<= 1) {
      const int a = tid >= s ? s_tp[tid - s] : 0, b = tid >= s ? s_n[tid - s] : 0;
      __syncthreads();
      s_tp[tid] += a; s_n[tid] += b;
      __syncthreads();
    }
    const int right_tp = carry_tp + s_tp[tid] - (tpf ? 1 : 0);                   // matches strictly right of this detection
    const int n_i = n_sel - (carry_n + s_n[tid] - 1);                            // selected detections up to and including it
    const int tp_i = tp_total - right_tp, fp_i = n_i - tp_i;
    const float pr = sel ? (float)tp_i / (((float)fp_i + (float)tp_i) + 2.220446049250313e-16f) : -1.0f;
    s_mx[tid] = pr;
    __syncthreads();
    for (int s = 1; s < CURVE_THREADS; s <<= 1) {
      const float a = tid >= s ? s_mx[tid - s] : -1.0f;
      __syncthreads();
      s_mx[tid] = fmaxf(s_mx[tid], a);
      __syncthreads();
    }
    const float env = fmaxf(s_mx[tid], carry_mx);
    if (sel && (tpf || n_i == 1)) {
      const float rc_cur = (float)tp_i / npig_f;
      int lo = 0;
      if (n_i != 1) {                                                            // first threshold > fl((tp - 1) / npig)
        const float rc_prev = (float)(tp_i - 1) / npig_f;
        int hi = p.n_rec;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (p.rec[mid] > rc_prev) hi = mid; else lo = mid + 1;
        }
      }
      const float sc = p.det_scores[id];
      for (int r = lo; r < p.n_rec && p.rec[r] <= rc_cur; r++) { s_prec[r] = env; s_score[r] = sc; }
    }
    carry_tp += s_tp[CURVE_THREADS - 1];
    carry_n += s_n[CURVE_THREADS - 1];
    carry_mx = fmaxf(carry_mx, s_mx[CURVE_THREADS - 1]);
    __syncthreads();
  }
  __syncthreads();
  for (int r = tid; r < p.n_rec; r += CURVE_THREADS) { out_p[r * stride_r] = s_prec[r]; out_s[r * stride_r] = s_score[r]; }
  if (tid == 0) *out_r = n_sel ? (float)tp_total / npig_f : 0.0f;
}

// ------------------------------------------------------------------------------------------------------------------
// d. Confusion matrix: rows = true label, columns = predicted label.  Labels are float64, truncated towards zero like
//    astype(int); a node with a label outside 0 .. K-1 is left out; a NaN label sets bit 0 of *status.  Histogram in LDS per
//    work-group, then one atomic add per non-zero cell.
// ------------------------------------------------------------------------------------------------------------------
constexpr int CONF_MAX_K = 64;

__global__ __launch_bounds__(256) void k_confusion(const double* __restrict__ y_true, const double* __restrict__ y_pred, int64_t n,
                                                  int k, unsigned long long* __restrict__ out, int32_t* __restrict__ status) {
  __shared__ unsigned hist[CONF_MAX_K * CONF_MAX_K];
  const int cells = k * k;
  for (int i = threadIdx.x; i < cells; i += blockDim.x) hist[i] = 0u;
  __syncthreads();
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double a = y_true[i], b = y_pred[i];
    if (a != a || b != b) { bad = true; continue; }
    const double ta = trunc(a), tb = trunc(b);
    if (ta >= 0.0 && ta < (double)k && tb >= 0.0 && tb < (double)k) atomicAdd(&hist[(int)ta * k + (int)tb], 1u);
  }
  if (bad) atomicOr(status, 1);
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += blockDim.x)
    if (hist[i]) atomicAdd(&out[i], (unsigned long long)hist[i]);
}

}  // namespace

extern "C" int rgnn_box_iou(const float* boxes_pred, const int64_t* pred_ptr, const float* boxes_gt, const int64_t* gt_ptr,
                            int64_t n_frames, const int64_t* out_ptr, int64_t n_out, float* iou, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n_frames >= 1 && n_out >= 0, "bad sizes");
  if (n_out == 0) return RGNN_OK;
  RGNN_CHECK_ARG(boxes_pred && pred_ptr && boxes_gt && gt_ptr && out_ptr && iou, "null pointers");
  hipLaunchKernelGGL(k_box_iou, dim3(rgnn_blocks(n_out, 256)), dim3(256), 0, (hipStream_t)stream, boxes_pred, pred_ptr, boxes_gt,
                     gt_ptr, n_frames, out_ptr, n_out, iou);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

extern "C" int32_t rgnn_map_match_capacity(void) { return MATCH_CAP; }

extern "C" int rgnn_map_match(const void* iou, int32_t iou_is_f32, const int64_t* pred_ptr, const int64_t* gt_ptr,
                              const int64_t* out_ptr, int64_t n_frames, const int32_t* det_labels, const float* det_scores, int64_t n_pred, const int32_t* gt_labels,
                              const int32_t* classes, int32_t n_classes, const double* thresholds, int32_t n_thresholds,
                              int32_t max_det, int32_t* rank, uint8_t* matched, int32_t* status, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n_frames >= 1 && n_pred >= 0 && n_classes >= 0 && n_thresholds >= 0 && max_det >= 1, "bad sizes");
  RGNN_CHECK_ARG(status, "null status");
  RGNN_CHECK_ARG(n_frames * (int64_t)(n_classes > 0 ? n_classes : 1) < ((int64_t)1 << 31), "too many (frame, class) pairs");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess) {
    rgnn_set_error("rgnn_map_match: clearing the status word failed");
    return RGNN_ERR_LAUNCH;
  }
  if (n_pred == 0) return RGNN_OK;
  RGNN_CHECK_ARG(pred_ptr && gt_ptr && out_ptr && det_labels && det_scores && rank && (matched || n_thresholds == 0), "null pointers");
  if (hipMemsetAsync(rank, 0xff, (size_t)n_pred * sizeof(int32_t), s) != hipSuccess ||
      (n_thresholds > 0 && hipMemsetAsync(matched, 0, (size_t)n_pred * (size_t)n_thresholds, s) != hipSuccess)) {
    rgnn_set_error("rgnn_map_match: clearing the outputs failed");
    return RGNN_ERR_LAUNCH;
  }
  if (n_classes == 0) return RGNN_OK;
  RGNN_CHECK_ARG(classes && (thresholds || n_thresholds == 0), "null pointers");    // (gt_labels / iou may be null without ground truth)
  MatchParams p{iou, (int)iou_is_f32, pred_ptr, gt_ptr, out_ptr, det_labels, det_scores, n_pred, gt_labels, classes, (int)n_classes,
                thresholds, (int)n_thresholds, (int)max_det, rank, matched, status};
  hipLaunchKernelGGL(k_map_match, dim3((unsigned)(n_frames * n_classes)), dim3(64), 0, s, p);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

extern "C" int rgnn_map_curves(const int64_t* order, const int64_t* cls_ptr, const int32_t* det_labels, const float* det_scores, const int32_t* rank,
                               const uint8_t* matched, int64_t n_pred, const int32_t* gt_labels, int64_t n_gt, const int32_t* classes,
                               int32_t n_classes, int32_t n_thresholds, const int32_t* max_dets, int32_t n_max_dets, const float* rec,
                               int32_t n_rec, float* precision, float* scores, float* recall, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n_pred >= 0 && n_gt >= 0 && n_classes >= 0 && n_thresholds >= 0 && n_max_dets >= 1 && n_rec >= 1, "bad sizes");
  if (n_rec > CURVE_MAX_REC) {
    rgnn_set_error("rgnn_map_curves: at most %d recall thresholds (got %d)", CURVE_MAX_REC, (int)n_rec);
    return RGNN_ERR_UNSUPPORTED;
  }
  RGNN_CHECK_ARG(n_pred < ((int64_t)1 << 31) && n_gt < ((int64_t)1 << 31), "too many boxes");
  const int64_t blocks = (int64_t)n_classes * n_thresholds * n_max_dets;
  if (blocks == 0) return RGNN_OK;
  RGNN_CHECK_ARG(blocks < ((int64_t)1 << 31), "too many curves");
  RGNN_CHECK_ARG(classes && cls_ptr && max_dets && rec && precision && scores && recall && (gt_labels || n_gt == 0) &&
                 ((order && det_labels && det_scores && rank && matched) || n_pred == 0), "null pointers");
  CurveParams p{order, cls_ptr, det_labels, det_scores, rank, matched, n_pred, gt_labels, n_gt, classes, (int)n_classes, (int)n_thresholds,
                max_dets, (int)n_max_dets, rec, (int)n_rec, precision, scores, recall};
  hipLaunchKernelGGL(k_map_curves, dim3((unsigned)blocks), dim3(CURVE_THREADS), 0, (hipStream_t)stream, p);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

extern "C" int rgnn_confusion_matrix(const double* y_true, const double* y_pred, int64_t n, int32_t n_classes, int64_t* matrix,
                                     int32_t* status, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n >= 0 && n_classes >= 1, "bad sizes");
  if (n_classes > CONF_MAX_K) {
    rgnn_set_error("rgnn_confusion_matrix: at most %d classes (got %d)", CONF_MAX_K, (int)n_classes);
    return RGNN_ERR_UNSUPPORTED;
  }
  RGNN_CHECK_ARG(matrix && status && ((y_true && y_pred) || n == 0), "null pointers");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(matrix, 0, (size_t)n_classes * n_classes * sizeof(int64_t), s) != hipSuccess ||
      hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess) {
    rgnn_set_error("rgnn_confusion_matrix: clearing the outputs failed");
    return RGNN_ERR_LAUNCH;
  }
  if (n == 0) return RGNN_OK;
  const unsigned blocks = rgnn_blocks(n, 256) < 1024u ? rgnn_blocks(n, 256) : 1024u;
  hipLaunchKernelGGL(k_confusion, dim3(blocks), dim3(256), 0, s, y_true, y_pred, n, (int)n_classes, (unsigned long long*)matrix, status);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}
