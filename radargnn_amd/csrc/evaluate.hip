// Evaluation on the device: the ground-truth duplicate removal and the point IoU the reference scores its mAP with.
//   GroundTruthExtractor.remove_duplicate_boxes    postprocessor/postprocessing.py:552-575
//   point_iou and its helpers                     utils/math.py:61-211
// Everything is batched over frames by offset arrays (int64 [n_frames + 1]); results are bit-exact restatements of the
// reference's float64 arithmetic (the library is built with -ffp-contract=off: no fused multiply-adds).
#include "common.h"
#include <math.h>

namespace {

constexpr double PI_D = 3.141592653589793;

// index f of the segment of ptr [n_seg + 1] (ascending) that holds position x: ptr[f] <= x < ptr[f + 1]; the last such
// f when empty segments share the offset
__device__ __forceinline__ int64_t segment_of(const int64_t* __restrict__ ptr, int64_t n_seg, int64_t x) {
  int64_t lo = 0, hi = n_seg;                  // invariant: ptr[lo] <= x < ptr[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (ptr[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------------------------------------------------------------
// Duplicate removal.  Box j of a frame goes iff some box i < j of the same frame matches it -- whether i was itself
// removed or not (the reference collects the indices first, then deletes): all 8 corner values ==, or the sum of the 8
// absolute differences < 0.1, summed as numpy's pairwise sum adds 8 contiguous float64 values.  Labels are not compared;
// equal inf corners match through ==; NaN never matches.
// One lane per box j; the rows i of the block's frames are staged through LDS 256 at a time, and the block stops as soon
// as every lane has its answer.
// ------------------------------------------------------------------------------------------------------------------
constexpr int DEDUP_BLOCK = 256;

__device__ __forceinline__ bool boxes_match(const double* a, const double* b) {
  bool eq = true;
  double d[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    eq = eq && (a[k] == b[k]);
    d[k] = fabs(a[k] - b[k]);
  }
  const double sum = ((d[0] + d[1]) + (d[2] + d[3])) + ((d[4] + d[5]) + (d[6] + d[7]));
  return eq || sum < 0.1;
}

__global__ __launch_bounds__(DEDUP_BLOCK) void k_dedup(const double* __restrict__ corners, const int64_t* __restrict__ box_ptr,
                                                      int64_t n_frames, int64_t m, int32_t* __restrict__ keep) {
  __shared__ double rows[DEDUP_BLOCK][9];                    // 9: odd stride, no bank conflicts on the broadcast reads
  const int t = threadIdx.x;
  const int64_t j0 = (int64_t)blockIdx.x * DEDUP_BLOCK;
  const int64_t j = j0 + t;
  const bool valid = j < m;
  const int64_t last = (j0 + DEDUP_BLOCK < m ? j0 + DEDUP_BLOCK : m) - 1;
  const int64_t start = valid ? box_ptr[segment_of(box_ptr, n_frames, j)] : 0;
  const int64_t lo = box_ptr[segment_of(box_ptr, n_frames, j0)];     // first row any lane of the block can compare with
  double mine[8];
  if (valid)
    for (int k = 0; k < 8; k++) mine[k] = corners[j * 8 + k];
  bool found = false;
  for (int64_t i0 = lo; i0 < last; i0 += DEDUP_BLOCK) {
    const int64_t r = i0 + t;
    if (r < m)
      for (int k = 0; k < 8; k++) rows[t][k] = corners[r * 8 + k];
    __syncthreads();
    if (valid && !found) {
      const int64_t a = start > i0 ? start : i0;
      const int64_t b = j < i0 + DEDUP_BLOCK ? j : i0 + DEDUP_BLOCK;
      for (int64_t i = a; i < b; i++)
        if (boxes_match(rows[i - i0], mine)) { found = true; break; }
    }
    const bool done = !valid || found || j <= i0 + DEDUP_BLOCK;
    if (__syncthreads_and(done)) break;                       // (also the barrier before the next tile overwrites rows)
  }
  if (valid) keep[j] = found ? 0 : 1;
}

// ------------------------------------------------------------------------------------------------------------------
// Point IoU (utils/math.py:176-211).  Per frame, for every (predicted, ground-truth) box pair:
//   A, B = the frame's points inside each box;  tp = |set(A) & set(B)| over (x, y) TUPLES, fp = |A| - tp, fn = |B| - tp
//   iou = tp / (tp + fp + fn), or 0.00001 when that sum is 0.
// Three kernels:
//   k_canonical_points  one block per frame: the frame's (x, y) keys sorted in LDS (bitonic, key then index); the first
//                       point of every run of equal keys is its coordinate's "canonical" point.  -0.0 and 0.0 share a key
//                       (they are equal tuples).  Bitmap per frame, 64 points per word.
//   k_points_in_boxes   one bit per (box, point): aligned [x_min, y_min, x_max, y_max], inclusive comparisons; rotated
//                       [x, y, l, w, theta deg], corners as get_box_corners and the area test of is_point_in_rect in
//                       float64, in the reference's expression order.  A wave ballots 64 points into one word.
//   k_point_iou         one lane per pair: popcounts of A & B & canonical, A and B.
// Membership depends on the coordinates only, so a coordinate lies in both boxes iff its canonical point does: tp counts
// the distinct coordinates, |A| and |B| count every point.
// ------------------------------------------------------------------------------------------------------------------
constexpr int CANON_MAX = 8192;                              // points per frame (LDS: 12 B per point)
constexpr int CANON_THREADS = 1024;

__device__ __forceinline__ unsigned long long point_key(float x, float y) {
  if (x == 0.0f) x = 0.0f;                                   // -0.0 -> 0.0
  if (y == 0.0f) y = 0.0f;
  return ((unsigned long long)__float_as_uint(x) << 32) | (unsigned long long)__float_as_uint(y);
}

__global__ __launch_bounds__(CANON_THREADS) void k_canonical_points(const float* __restrict__ points, const int64_t* __restrict__ frame_ptr,
                                                                    int words, unsigned long long* __restrict__ canon) {
  __shared__ unsigned long long sk[CANON_MAX];
  __shared__ unsigned si[CANON_MAX];
  __shared__ unsigned long long bits[CANON_MAX / 64];
  const int64_t f = blockIdx.x;
  const int64_t base = frame_ptr[f];
  const int n = (int)(frame_ptr[f + 1] - base);
  int padded = 1;
  while (padded < n) padded <<= 1;
  for (int t = threadIdx.x; t < padded; t += CANON_THREADS) {
    if (t < n) { sk[t] = point_key(points[2 * (base + t)], points[2 * (base + t) + 1]); si[t] = (unsigned)t; }
    else { sk[t] = ~0ull; si[t] = 0xffffffffu; }             // padding sorts after every real point
  }
  for (int w = threadIdx.x; w < CANON_MAX / 64; w += CANON_THREADS) bits[w] = 0ull;
  __syncthreads();
  for (int k = 2; k <= padded; k <<= 1) {
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int t = threadIdx.x; t < padded; t += CANON_THREADS) {
        const int p = t ^ jj;
        if (p > t) {
          const bool up = (t & k) == 0;
          const unsigned long long ka = sk[t], kb = sk[p];
          const unsigned ia = si[t], ib = si[p];
          const bool b_first = kb < ka || (kb == ka && ib < ia);
          if (b_first == up) { sk[t] = kb; si[t] = ib; sk[p] = ka; si[p] = ia; }
        }
      }
      __syncthreads();
    }
  }
  for (int t = threadIdx.x; t < n; t += CANON_THREADS)
    if (t == 0 || sk[t - 1] != sk[t]) atomicOr(&bits[si[t] >> 6], 1ull << (si[t] & 63));
  __syncthreads();
  for (int w = threadIdx.x; w < words; w += CANON_THREADS)
    canon[f * words + w] = w < CANON_MAX / 64 ? bits[w] : 0ull;
}

// is_point_in_rect (utils/math.py:61-99) on the corners of get_box_corners (:9-45); NaN anywhere -> false
__device__ __forceinline__ bool in_rect(const double (&cx)[4], const double (&cy)[4], double abcd, double xP, double yP) {
  const double xA = cx[0], yA = cy[0], xB = cx[1], yB = cy[1], xC = cx[2], yC = cy[2], xD = cx[3], yD = cy[3];
  const double abp = 0.5 * fabs(xA * (yB - yP) + xB * (yP - yA) + xP * (yA - yB));
  const double bcp = 0.5 * fabs(xB * (yC - yP) + xC * (yP - yB) + xP * (yB - yC));
  const double cdp = 0.5 * fabs(xC * (yD - yP) + xD * (yP - yC) + xP * (yC - yD));
  const double dap = 0.5 * fabs(xD * (yA - yP) + xA * (yP - yD) + xP * (yD - yA));
  const double sum_tri = abp + bcp + cdp + dap;
  return (sum_tri - abcd) < 1e-6;
}

// grid (boxes, ceil(words / 4)), 4 waves per block, one word per wave
template <bool ROTATED>
__global__ __launch_bounds__(256) void k_points_in_boxes(const float* __restrict__ boxes, const int64_t* __restrict__ box_ptr,
                                                        int64_t n_frames, const float* __restrict__ points,
                                                        const int64_t* __restrict__ frame_ptr, int words,
                                                        unsigned long long* __restrict__ mask) {
  const int64_t b = blockIdx.x;
  const int w = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= words) return;                                    // (whole waves)
  const int64_t f = segment_of(box_ptr, n_frames, b);
  const int64_t base = frame_ptr[f], n = frame_ptr[f + 1] - base;
  const int64_t q = (int64_t)w * 64 + lane;
  bool in = false;
  if (q < n) {
    const float px = points[2 * (base + q)], py = points[2 * (base + q) + 1];
    if constexpr (!ROTATED) {
      const float* bx = boxes + b * 4;
      in = px >= bx[0] && px <= bx[2] && py >= bx[1] && py <= bx[3];
    } else {
      const float* bx = boxes + b * 5;
      const double x = bx[0], y = bx[1], l = bx[2], wd = bx[3], theta = bx[4];
      const double ox[4] = {l / 2, l / 2, -l / 2, -l / 2}, oy[4] = {wd / 2, -wd / 2, -wd / 2, wd / 2};
      const double rad = (theta * PI_D) / 180;
      const double c = cos(rad), s = sin(rad);
      double cx[4], cy[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        cx[k] = (c * ox[k] + (-s) * oy[k]) + x;
        cy[k] = (s * ox[k] + c * oy[k]) + y;
      }
      const double abcd = 0.5 * fabs((cy[0] - cy[2]) * (cx[3] - cx[1]) + (cy[1] - cy[3]) * (cx[0] - cx[2]));
      in = in_rect(cx, cy, abcd, (double)px, (double)py);
    }
  }
  const unsigned long long word = __ballot(in);
  if (lane == 0) mask[b * words + w] = word;
}

__global__ __launch_bounds__(256) void k_point_iou(const unsigned long long* __restrict__ mask_pred, const int64_t* __restrict__ pred_ptr,
                                                  const unsigned long long* __restrict__ mask_gt, const int64_t* __restrict__ gt_ptr,
                                                  const unsigned long long* __restrict__ canon, const int64_t* __restrict__ frame_ptr,
                                                  int64_t n_frames, int words, const int64_t* __restrict__ out_ptr, int64_t total,
                                                  double* __restrict__ iou) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int64_t f = segment_of(out_ptr, n_frames, t);
  const int64_t g_count = gt_ptr[f + 1] - gt_ptr[f];
  const int64_t local = t - out_ptr[f];
  const int64_t p = pred_ptr[f] + local / g_count, g = gt_ptr[f] + local % g_count;
  const int fw = (int)((frame_ptr[f + 1] - frame_ptr[f] + 63) / 64);
  const unsigned long long* A = mask_pred + p * words;
  const unsigned long long* B = mask_gt + g * words;
  const unsigned long long* C = canon + f * words;
  long long tp = 0, na = 0, nb = 0;
  for (int w = 0; w < fw; w++) {
    const unsigned long long a = A[w], b = B[w];
    tp += __popcll(a & b & C[w]);
    na += __popcll(a);
    nb += __popcll(b);
  }
  const long long fp = na - tp, fn = nb - tp, sum = tp + fp + fn;
  iou[t] = sum != 0 ? (double)tp / (double)sum : 0.00001;
}

}  // namespace

extern "C" int rgnn_remove_duplicate_boxes(const double* corners, const int64_t* box_ptr, int64_t n_frames, int64_t m,
                                           int32_t* keep, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(m >= 0 && n_frames >= 1, "bad sizes");
  if (m == 0) return RGNN_OK;
  RGNN_CHECK_ARG(corners && box_ptr && keep, "null pointers");
  hipLaunchKernelGGL(k_dedup, dim3(rgnn_blocks(m, DEDUP_BLOCK)), dim3(DEDUP_BLOCK), 0, (hipStream_t)stream, corners, box_ptr,
                     n_frames, m, keep);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

extern "C" int64_t rgnn_point_iou_tmp_bytes(int64_t n_frames, int32_t words, int64_t n_pred, int64_t n_gt) {
  return (n_frames + n_pred + n_gt) * (int64_t)words * 8;
}

extern "C" int rgnn_point_iou(const float* boxes_pred, const int64_t* pred_ptr, int64_t n_pred, const float* boxes_gt,
                              const int64_t* gt_ptr, int64_t n_gt, int32_t rotated, const float* points, const int64_t* frame_ptr,
                              int64_t n_frames, int32_t max_frame_points, const int64_t* out_ptr, int64_t n_out, double* iou,
                              void* tmp, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n_frames >= 1 && n_pred >= 0 && n_gt >= 0 && n_out >= 0 && max_frame_points >= 0, "bad sizes");
  if (max_frame_points > CANON_MAX) {
    rgnn_set_error("rgnn_point_iou: at most %d points per frame (got %d)", CANON_MAX, (int)max_frame_points);
    return RGNN_ERR_UNSUPPORTED;
  }
  if (n_out == 0) return RGNN_OK;
  const int words = (max_frame_points + 63) / 64;
  RGNN_CHECK_ARG(boxes_pred && pred_ptr && boxes_gt && gt_ptr && frame_ptr && out_ptr && iou && (points || words == 0) && tmp,
                 "null pointers");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* canon = (unsigned long long*)tmp;
  unsigned long long* mpred = canon + n_frames * words;
  unsigned long long* mgt = mpred + n_pred * words;
  if (words > 0) {
    hipLaunchKernelGGL(k_canonical_points, dim3((unsigned)n_frames), dim3(CANON_THREADS), 0, s, points, frame_ptr, words, canon);
    const dim3 grid_p((unsigned)n_pred, (unsigned)((words + 3) / 4)), grid_g((unsigned)n_gt, (unsigned)((words + 3) / 4));
    if (rotated) {
      hipLaunchKernelGGL(k_points_in_boxes<true>, grid_p, dim3(256), 0, s, boxes_pred, pred_ptr, n_frames, points, frame_ptr, words, mpred);
      hipLaunchKernelGGL(k_points_in_boxes<true>, grid_g, dim3(256), 0, s, boxes_gt, gt_ptr, n_frames, points, frame_ptr, words, mgt);
    } else {
      hipLaunchKernelGGL(k_points_in_boxes<false>, grid_p, dim3(256), 0, s, boxes_pred, pred_ptr, n_frames, points, frame_ptr, words, mpred);
      hipLaunchKernelGGL(k_points_in_boxes<false>, grid_g, dim3(256), 0, s, boxes_gt, gt_ptr, n_frames, points, frame_ptr, words, mgt);
    }
  }
  hipLaunchKernelGGL(k_point_iou, dim3(rgnn_blocks(n_out, 256)), dim3(256), 0, s, mpred, pred_ptr, mgt, gt_ptr, canon, frame_ptr,
                     n_frames, words, out_ptr, n_out, iou);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}
