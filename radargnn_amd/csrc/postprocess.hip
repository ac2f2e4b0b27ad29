// Post-processor front half on the device: what the reference does per graph in numpy loops after the
// forward pass -- PredictionExtractor.get_predicted_label / get_prediction_scores / get_clutter_scores and
// get_absolute_object_bounding_box_predictions (postprocessor/postprocessing.py:177-196,198-319), with the box algebra of
// preprocessor/bounding_box.py:21-66 (absolute rotated), :68-153 (E(n)-invariant), :156-199 (relative rotated), :275-312
// (relative aligned) and :566-589 (inverse of the sin-smoothed angle).
//
// One thread per node: label = FIRST index of the row maximum, score = that maximum, keep flag from the three removal
// rules, and the four corners of the absolute box.  The box arithmetic runs in float64 on the float32 predictions (numpy
// scalars of the reference's pinned numpy 1.x promote to float64 with Python floats); the threshold comparisons keep the
// reference's dtypes: background probability float32 >= float32(threshold), score float64 <= float64 threshold.
// HBM-bound: reads 4 (K + W + 2) bytes per node, writes 76.
#include "common.h"
#include <math.h>
#include <type_traits>

namespace {

constexpr double PI_D = 3.141592653589793;

struct DecodeParams {
  const float* prob; int64_t ldp; int K;
  const float* bb; int64_t ldb; int W;
  const float* pos;
  const int32_t* nn;
  int64_t n;
  int bg_index; float max_bg;
  const double* min_score; int n_min;
  int invariance;            // 0 none, 1 translation, 2 en
  int adapt_angle;
  int32_t* label; float* score; int32_t* keep; double* corners;
};

__device__ __forceinline__ double round5(double x) { return rint(x * 100000.0) / 100000.0; }   // np.round(x, 5)

// The absolute box of node i (box algebra of preprocessor/bounding_box.py, see the head of this file): corners c1..c4
// (x, y) in float64 into corners[8 i ..].  Shared by the prediction and the ground-truth decode.
__device__ __forceinline__ void decode_box(const float* __restrict__ bb, int64_t ldb, int W, const float* __restrict__ pos,
                                           const int32_t* __restrict__ nn, int invariance, int adapt_angle, int64_t i,
                                           double* __restrict__ corners) {
  const float* b = bb + i * ldb;
  const double px = (double)pos[2 * i], py = (double)pos[2 * i + 1];
  double cx, cy, hl, hw, theta_deg = 0.0;
  bool rotate = false;
  if (W == 4) {                                        // relative aligned box: bounding_box.py:275-312
    cx = px + (double)b[0]; cy = py + (double)b[1];
    hl = (double)b[2] / 2; hw = (double)b[3] / 2;
  } else if (invariance != 2) {
    hl = (double)b[2] / 2; hw = (double)b[3] / 2;
    double th = (double)b[4];
    if (adapt_angle) {                                 // invert_bb_orientation_angle_adaption, bounding_box.py:566-589
      th = fmax(fmin(th, 1.0), -1.0);
      th = asin(th);
      if (th < 0) th = th + PI_D;
    }
    theta_deg = th * 180 / PI_D;
    rotate = true;
    if (invariance == 1) { cx = px + (double)b[0]; cy = py + (double)b[1]; }      // relative rotated :156-199
    else { cx = (double)b[0]; cy = (double)b[1]; }                                  // absolute rotated :21-66
  } else {                                               // E(n)-invariant representation: bounding_box.py:97-153
    const int32_t j = nn[i];
    const double vx = (double)pos[2 * (int64_t)j] - px, vy = (double)pos[2 * (int64_t)j + 1] - py;
    const double nrm = sqrt(vx * vx + vy * vy);
    const double th_nn = atan2(vy / nrm, vx / nrm) * 180 / PI_D;
    const double d = (double)b[0];
    const double th_pc_rel = (double)b[1] * 180 / PI_D, th_dir_rel = (double)b[4] * 180 / PI_D;
    double th_dir = round5(th_dir_rel + th_nn);
    while (th_dir < 0) th_dir = 360 + th_dir;
    while (th_dir >= 180) th_dir = th_dir - 180;
    double th_pc = th_pc_rel + th_nn;
    while (th_pc > 360) th_pc = th_pc - 360;
    const double xc = d * cos((th_pc * PI_D) / 180), yc = d * sin((th_pc * PI_D) / 180);
    hl = (double)b[2] / 2; hw = (double)b[3] / 2;
    theta_deg = th_dir;
    rotate = true;
    cx = px + xc; cy = py + yc;
  }
  double c = 1.0, s = 0.0;
  if (rotate) {
    const double rad = (theta_deg * PI_D) / 180;
    c = cos(rad); s = sin(rad);
  }
  const double ox[4] = {hl, hl, -hl, -hl}, oy[4] = {hw, -hw, -hw, hw};              // c1..c4 before rotation
  double* out = corners + i * 8;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const double rx = rotate ? c * ox[q] + (-s) * oy[q] : ox[q];
    const double ry = rotate ? s * ox[q] + c * oy[q] : oy[q];
    out[2 * q] = rx + cx;
    out[2 * q + 1] = ry + cy;
  }
}

__global__ __launch_bounds__(256) void k_decode(const DecodeParams p) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const float* pr = p.prob + i * p.ldp;
  int best = 0;
  float m = pr[0];
  for (int k = 1; k < p.K; k++) {
    const float v = pr[k];
    if (v > m) { m = v; best = k; }                     // np.where(vec == max)[0][0]: the first maximum
  }
  bool remove = false;
  if (p.bg_index >= 0 && p.bg_index < p.K) remove = pr[p.bg_index] >= p.max_bg;     // postprocessing.py:222
  remove = remove || best == p.bg_index;                                            // :223
  if (best < p.n_min) remove = remove || ((double)m <= p.min_score[best]);          // :227-228
  p.label[i] = best;
  p.score[i] = m;
  p.keep[i] = remove ? 0 : 1;

  decode_box(p.bb, p.ldb, p.W, p.pos, p.nn, p.invariance, p.adapt_angle, i, p.corners);
}

// Ground truth (GroundTruthExtractor.get_absolute_object_bounding_boxes, postprocessor/postprocessing.py:447-551): a node
// is kept when its label (float32) != bg_index; no score filter, and the angle is never adapted.
__global__ __launch_bounds__(256) void k_decode_ground_truth(const float* __restrict__ labels, int64_t ldl,
                                                             const float* __restrict__ bb, int64_t ldb, int W,
                                                             const float* __restrict__ pos, const int32_t* __restrict__ nn,
                                                             int64_t n, int bg_index, int invariance, int32_t* __restrict__ keep,
                                                             double* __restrict__ corners) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  keep[i] = (double)labels[i * ldl] != (double)bg_index ? 1 : 0;     // np.where(class_labels == bg_index): NaN is kept
  decode_box(bb, ldb, W, pos, nn, invariance, 0, i, corners);
}

}  // namespace

extern "C" int rgnn_decode_predictions(const float* class_prob, int64_t ldp, int32_t n_classes, const float* boxes,
                                       int64_t ldb, int32_t box_width, const float* pos, const int32_t* nn_index, int64_t n,
                                       int32_t bg_index, float max_score_for_background, const double* min_object_score,
                                       int32_t n_min_scores, int32_t invariance, int32_t adapt_orientation_angle,
                                       int32_t* label, float* score, int32_t* keep, double* corners, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n >= 0 && n_classes >= 1, "bad sizes");
  RGNN_CHECK_ARG(box_width == 4 || box_width == 5, "boxes are [x, y, dx, dy] or [x, y, l, w, theta]");
  RGNN_CHECK_ARG(invariance >= 0 && invariance <= 2, "invariance: 0 none, 1 translation, 2 en");
  if (n == 0) return RGNN_OK;
  RGNN_CHECK_ARG(!(invariance == 2 && box_width == 5) || nn_index != nullptr, "the en representation needs nearest neighbours");
  RGNN_CHECK_ARG(n_min_scores == 0 || min_object_score != nullptr, "null thresholds");
  RGNN_CHECK_ARG(class_prob && boxes && pos && label && score && keep && corners, "null pointers");
  DecodeParams p{class_prob, ldp, n_classes, boxes, ldb, box_width, pos, nn_index, n, bg_index, max_score_for_background,
                 min_object_score, n_min_scores, invariance, adapt_orientation_angle, label, score, keep, corners};
  hipLaunchKernelGGL(k_decode, dim3(rgnn_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, p);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

extern "C" int rgnn_decode_ground_truth(const float* labels, int64_t ldl, const float* boxes, int64_t ldb, int32_t box_width,
                                        const float* pos, const int32_t* nn_index, int64_t n, int32_t bg_index,
                                        int32_t invariance, int32_t* keep, double* corners, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n >= 0, "bad sizes");
  RGNN_CHECK_ARG(box_width == 4 || box_width == 5, "boxes are [x, y, dx, dy] or [x, y, l, w, theta]");
  RGNN_CHECK_ARG(invariance >= 0 && invariance <= 2, "invariance: 0 none, 1 translation, 2 en");
  if (n == 0) return RGNN_OK;
  RGNN_CHECK_ARG(!(invariance == 2 && box_width == 5) || nn_index != nullptr, "the en representation needs nearest neighbours");
  RGNN_CHECK_ARG(labels && boxes && pos && keep && corners, "null pointers");
  hipLaunchKernelGGL(k_decode_ground_truth, dim3(rgnn_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, labels, ldl, boxes, ldb,
                     (int)box_width, pos, nn_index, n, (int)bg_index, (int)invariance, keep, corners);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Non-maximum suppression (BoxSuppressor.apply_nms, postprocessor/postprocessing.py:336-431): greedy, by descending score;
// a box is dropped when its IoU with an already kept box exceeds the threshold.
//   kind 0  aligned boxes [x_min, y_min, x_max, y_max] float32 -- torchvision.ops.nms: suppress when IoU >  threshold
//   kind 1  rotated boxes [x, y, l, w, theta(deg)]     float64 -- detectron2 nms_rotated (CPU): suppress when IoU >= threshold
// Two kernels: (1) the M x M "j is suppressed by i" bit matrix over the score-sorted boxes, 64 x 64 tiles, one row per lane,
// the 64 column boxes of a tile staged in LDS; (2) one work-group walks the sorted boxes 64 at a time: the in-tile greedy
// pass runs on the tile's diagonal words with wave broadcasts, then the rows of the boxes kept are OR-ed into the
// `removed` bitmap (LDS) by all threads.  Rotated IoU: the rectangle of box 1 clipped by the four half-planes of box 2
// (Sutherland-Hodgman, <= 8 vertices), shoelace area -- the same quantity detectron2 obtains via intersection points +
// convex hull.
// ------------------------------------------------------------------------------------------------------------------
namespace {

__device__ __forceinline__ float iou_aligned(const float* a, const float* b) {
  const float area_a = (a[2] - a[0]) * (a[3] - a[1]), area_b = (b[2] - b[0]) * (b[3] - b[1]);
  const float w = fmaxf(0.f, fminf(a[2], b[2]) - fmaxf(a[0], b[0]));
  const float h = fmaxf(0.f, fminf(a[3], b[3]) - fmaxf(a[1], b[1]));
  const float inter = w * h;
  return inter / (area_a + area_b - inter);
}

// Corner convention of detectron2's box_iou_rotated (get_rotated_vertices in layers/csrc/box_iou_rotated/
// box_iou_rotated_utils.h, image coordinates with y pointing down): the long side points along (cos t, -sin t),
//   pts[0] = ctr + l/2 (cos, -sin) + w/2 (sin, cos).
// The reference hands theta_x = atan2(v_y, v_x) of its y-up frame straight to nms_rotated (postprocessing.py:356-370), so
// what it suppresses on are the IoUs of boxes mirrored about their own centre -- and a mirrored pair overlaps differently
// from the original pair unless the boxes are axis aligned.  Parity with the reference means reproducing that.
__device__ __forceinline__ void rect_vertices(double x, double y, double l, double w, double deg, double (&vx)[4], double (&vy)[4]) {
  const double t = deg * PI_D / 180;
  const double c = cos(t), s = -sin(t), a = l / 2, b = w / 2;
  vx[0] = x + a * c - b * s; vy[0] = y + a * s + b * c;      // (one orientation; the clipping below works with |area|)
  vx[1] = x - a * c - b * s; vy[1] = y - a * s + b * c;
  vx[2] = x - a * c + b * s; vy[2] = y - a * s - b * c;
  vx[3] = x + a * c + b * s; vy[3] = y + a * s - b * c;
}

__device__ double iou_rotated(const double* p, const double* q) {
  const double area_p = p[2] * p[3], area_q = q[2] * q[3];
  if (area_p < 1e-14 || area_q < 1e-14) return 0.0;
  const double sx = (p[0] + q[0]) / 2, sy = (p[1] + q[1]) / 2;     // work around the common centre (precision)
  double ax[4], ay[4], bx[4], by[4];
  rect_vertices(p[0] - sx, p[1] - sy, p[2], p[3], p[4], ax, ay);
  rect_vertices(q[0] - sx, q[1] - sy, q[2], q[3], q[4], bx, by);
  double px[8], py[8], qx[8], qy[8];
  int n = 4;
  for (int i = 0; i < 4; i++) { px[i] = ax[i]; py[i] = ay[i]; }
  for (int e = 0; e < 4 && n > 0; e++) {
    const double ex = bx[(e + 1) & 3] - bx[e], ey = by[(e + 1) & 3] - by[e];
    int m = 0;
    for (int i = 0; i < n; i++) {
      const int k = (i + 1 == n) ? 0 : i + 1;
      const double d0 = ex * (py[i] - by[e]) - ey * (px[i] - bx[e]);      // >= 0: inside (left of the edge)
      const double d1 = ex * (py[k] - by[e]) - ey * (px[k] - bx[e]);
      // (a convex polygon gains at most one vertex per clip edge; rounding in near-degenerate inputs could produce more
      // sign changes, so the writes are bounded by the array, not by the geometry)
      if (d0 >= 0 && m < 8) { qx[m] = px[i]; qy[m] = py[i]; m++; }
      if ((d0 >= 0) != (d1 >= 0) && m < 8) {
        const double t = d0 / (d0 - d1);
        qx[m] = px[i] + t * (px[k] - px[i]); qy[m] = py[i] + t * (py[k] - py[i]); m++;
      }
    }
    n = m < 8 ? m : 8;
    for (int i = 0; i < n; i++) { px[i] = qx[i]; py[i] = qy[i]; }
  }
  double inter = 0.0;
  for (int i = 0; i < n; i++) {
    const int k = (i + 1 == n) ? 0 : i + 1;
    inter += px[i] * py[k] - px[k] * py[i];
  }
  inter = fabs(inter) / 2;
  return inter / (area_p + area_q - inter);
}

template <int KIND>
__global__ __launch_bounds__(64) void k_nms_mask(const void* __restrict__ boxes_, const int64_t* __restrict__ order, int64_t m,
                                                double thr, unsigned long long* __restrict__ mask, int words) {
  using T = typename std::conditional<KIND == 0, float, double>::type;
  constexpr int BW = KIND == 0 ? 4 : 5;
  const T* boxes = (const T*)boxes_;
  const int bi = blockIdx.y, bj = blockIdx.x, lane = threadIdx.x;
  const int64_t i = (int64_t)bi * 64 + lane;
  if (bj < bi) {                                           // columns before the row: never suppressed by it
    if (i < m) mask[i * words + bj] = 0ull;
    return;
  }
  __shared__ T col[64][BW];
  const int64_t jc = (int64_t)bj * 64 + lane;
  if (jc < m) {
    const T* src = boxes + order[jc] * BW;
    for (int c = 0; c < BW; c++) col[lane][c] = src[c];
  }
  __syncthreads();
  if (i >= m) return;
  T mine[BW];
  const T* src = boxes + order[i] * BW;
  for (int c = 0; c < BW; c++) mine[c] = src[c];
  unsigned long long bits = 0ull;
  const int ncol = (int)((m - (int64_t)bj * 64 < 64) ? m - (int64_t)bj * 64 : 64);
  for (int c = 0; c < ncol; c++) {
    const int64_t j = (int64_t)bj * 64 + c;
    if (j <= i) continue;
    bool hit;
    if constexpr (KIND == 0) hit = iou_aligned(mine, col[c]) > (float)thr;
    else hit = iou_rotated(mine, col[c]) >= thr;
    if (hit) bits |= 1ull << c;
  }
  mask[i * words + bj] = bits;
}

constexpr int NMS_MAX_WORDS = 2048;     // 131 072 boxes per call

__global__ __launch_bounds__(256) void k_nms_reduce(const unsigned long long* __restrict__ mask, const int64_t* __restrict__ order,
                                                   int64_t m, int words, int64_t* __restrict__ keep, int64_t* __restrict__ count) {
  __shared__ unsigned long long removed[NMS_MAX_WORDS];
  __shared__ unsigned long long kept_bits;
  const int t = threadIdx.x, lane = t & 63;
  for (int w = t; w < words; w += 256) removed[w] = 0ull;
  __syncthreads();
  int64_t n_keep = 0;
  for (int b = 0; b < words; b++) {
    if (t < 64) {                                          // in-tile greedy pass on the diagonal words (wave 0)
      const int64_t i = (int64_t)b * 64 + lane;
      const unsigned long long diag = (i < m) ? mask[i * words + b] : 0ull;
      unsigned long long cur = removed[b], kb = 0ull;
      const int nrow = (int)((m - (int64_t)b * 64 < 64) ? m - (int64_t)b * 64 : 64);
      for (int l = 0; l < nrow; l++) {
        const unsigned long long row = __shfl(diag, l, 64);
        if (!((cur >> l) & 1ull)) { kb |= 1ull << l; cur |= row; }
      }
      if ((kb >> lane) & 1ull) keep[n_keep + __popcll(kb & ((1ull << lane) - 1ull))] = order[i];
      if (lane == 0) kept_bits = kb;
    }
    __syncthreads();
    const unsigned long long kb = kept_bits;
    n_keep += __popcll(kb);
    for (int w = b + 1 + t; w < words; w += 256) {         // rows of the boxes kept suppress the later tiles
      unsigned long long acc = removed[w], rest = kb;
      while (rest) {
        const int l = __ffsll((long long)rest) - 1;
        rest &= rest - 1;
        acc |= mask[((int64_t)b * 64 + l) * words + w];
      }
      removed[w] = acc;
    }
    __syncthreads();
  }
  if (t == 0) *count = n_keep;
}

}  // namespace

namespace {
// BoundingBox.get_to_two_point_representation / get_absolute_rotated_box_representations (preprocessor/bounding_box.py:447-
// 540) for all boxes at once: [x_min, y_min, x_max, y_max] and [x_centre, y_centre, l, w, theta in [0, 180]] per box.
// l / w: the two shorter of the distances corner 1 -> corners 2, 3, 4 (the longest is the diagonal); theta: direction of
// the side of length l; a box whose l matches none of the three (NaN corners) becomes the reference's default [0,0,1,1,0].
// One box: corners c[8] -> two_point tp[4] and / or rotated o[5] (either may be null).  Shared by k_box_repr and the segmented
// suppression kernel, so both see the same bits.
__device__ __forceinline__ void box_repr(const double* __restrict__ c, double* __restrict__ tp, double* __restrict__ o) {
  double x[4], y[4];
  for (int q = 0; q < 4; q++) { x[q] = c[2 * q]; y[q] = c[2 * q + 1]; }
  if (tp) {
    tp[0] = fmin(fmin(x[0], x[1]), fmin(x[2], x[3]));
    tp[1] = fmin(fmin(y[0], y[1]), fmin(y[2], y[3]));
    tp[2] = fmax(fmax(x[0], x[1]), fmax(x[2], x[3]));
    tp[3] = fmax(fmax(y[0], y[1]), fmax(y[2], y[3]));
  }
  if (o) {
    double d[3];
    for (int q = 0; q < 3; q++) {
      const double dx = x[0] - x[q + 1], dy = y[0] - y[q + 1];
      d[q] = sqrt(dx * dx + dy * dy);
    }
    int iw = 0;                                            // min(d), first occurrence; then min of the other two
    if (d[1] < d[iw]) iw = 1;
    if (d[2] < d[iw]) iw = 2;
    int il = -1;
    for (int q = 0; q < 3; q++)
      if (q != iw && (il < 0 || d[q] < d[il])) il = q;
    const double w = d[iw], l = d[il];
    int side = -1;                                         // first of d1, d2, d3 equal to l
    for (int q = 2; q >= 0; q--)
      if (d[q] == l) side = q;
    if (side < 0) { o[0] = 0; o[1] = 0; o[2] = 1; o[3] = 1; o[4] = 0; return; }
    const double vx = x[0] - x[side + 1], vy = y[0] - y[side + 1];
    const double nrm = sqrt(vx * vx + vy * vy);
    double theta = atan2(vy / nrm, vx / nrm) * 180 / PI_D;
    if (theta < 0) theta = 180 + theta;
    o[0] = (x[0] + x[1] + x[2] + x[3]) / 4;
    o[1] = (y[0] + y[1] + y[2] + y[3]) / 4;
    o[2] = l; o[3] = w; o[4] = theta;
  }
}

__global__ __launch_bounds__(256) void k_box_repr(const double* __restrict__ corners, int64_t m, double* __restrict__ two_point,
                                                 double* __restrict__ rotated) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  box_repr(corners + i * 8, two_point ? two_point + i * 4 : nullptr, rotated ? rotated + i * 5 : nullptr);
}
}  // namespace

extern "C" int rgnn_box_representations(const double* corners, int64_t m, double* two_point, double* rotated, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(m >= 0, "bad sizes");
  if (m == 0) return RGNN_OK;
  RGNN_CHECK_ARG(corners && (two_point || rotated), "null pointers");
  hipLaunchKernelGGL(k_box_repr, dim3(rgnn_blocks(m, 256)), dim3(256), 0, (hipStream_t)stream, corners, m, two_point, rotated);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

// ------------------------------------------------------------------------------------------------
// Score order for NMS: box ids by descending score, ties by ascending id (a stable descending sort; torchvision / detectron2 sort
// the scores first, postprocessing.py:336-435).  Bitonic network over (key, id) pairs: chunks of SORT_CHUNK pairs are sorted in
// LDS by one launch; for more boxes every merge stage runs its long-distance steps as one launch each and its short-distance
// steps in LDS again.  NaN scores order as the largest value (torch.sort's convention).
// ------------------------------------------------------------------------------------------------
namespace {
constexpr int SORT_CHUNK = 4096;
__device__ __forceinline__ unsigned long long score_key(double v) {
  if (v != v) return ~0ull;                                    // NaN: first
  if (v == 0.0) v = 0.0;                                       // -0.0 and +0.0 tie (a comparison sort cannot tell them apart)
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);         // order-preserving: larger score <-> larger key
}
// a goes before b: larger key first, equal keys by ascending id
__device__ __forceinline__ bool sort_before(unsigned long long ka, unsigned ia, unsigned long long kb, unsigned ib) {
  return ka > kb || (ka == kb && ia < ib);
}
// MODE 0: load scores, sort the chunk completely (stages k <= SORT_CHUNK); MODE 1: steps j < SORT_CHUNK of stage k on loaded pairs
template <int MODE>
__global__ __launch_bounds__(1024) void k_sort_chunk(const void* __restrict__ scores, int is_f64, int64_t m, int64_t padded,
                                                    unsigned long long* __restrict__ keys, unsigned* __restrict__ ids, int64_t k_stage) {
  __shared__ unsigned long long sk[SORT_CHUNK];
  __shared__ unsigned si[SORT_CHUNK];
  const int64_t base = (int64_t)blockIdx.x * SORT_CHUNK;
  for (int t = threadIdx.x; t < SORT_CHUNK; t += blockDim.x) {
    const int64_t i = base + t;
    if (MODE == 0) {
      if (i < m) {
        const double v = is_f64 ? ((const double*)scores)[i] : (double)((const float*)scores)[i];
        sk[t] = score_key(v); si[t] = (unsigned)i;
      } else { sk[t] = 0ull; si[t] = 0xffffffffu; }            // padding: after every real pair
    } else { sk[t] = keys[i]; si[t] = ids[i]; }
  }
  __syncthreads();
  const int64_t k_lo = MODE == 0 ? 2 : k_stage, k_hi = MODE == 0 ? SORT_CHUNK : k_stage;
  for (int64_t k = k_lo; k <= k_hi; k <<= 1) {
    for (int j = (int)((k >> 1) < SORT_CHUNK ? (k >> 1) : (SORT_CHUNK >> 1)); j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < SORT_CHUNK; t += blockDim.x) {
        const int p = t ^ j;
        if (p > t) {
          const bool up = (((base + t) & k) == 0);             // this pair belongs to an ascending (in sort_before order) run
          const unsigned long long ka = sk[t], kb = sk[p];
          const unsigned ia = si[t], ib = si[p];
          if (sort_before(kb, ib, ka, ia) == up) { sk[t] = kb; si[t] = ib; sk[p] = ka; si[p] = ia; }
        }
      }
      __syncthreads();
    }
  }
  for (int t = threadIdx.x; t < SORT_CHUNK; t += blockDim.x) { keys[base + t] = sk[t]; ids[base + t] = si[t]; }
}
__global__ __launch_bounds__(256) void k_sort_step(unsigned long long* __restrict__ keys, unsigned* __restrict__ ids, int64_t padded,
                                                  int64_t j, int64_t k) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= padded) return;
  const int64_t p = t ^ j;
  if (p <= t) return;
  const bool up = ((t & k) == 0);
  const unsigned long long ka = keys[t], kb = keys[p];
  const unsigned ia = ids[t], ib = ids[p];
  if (sort_before(kb, ib, ka, ia) == up) { keys[t] = kb; ids[t] = ib; keys[p] = ka; ids[p] = ia; }
}
__global__ __launch_bounds__(256) void k_sort_emit(const unsigned* __restrict__ ids, int64_t m, int64_t* __restrict__ order) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < m) order[t] = (int64_t)ids[t];
}
}  // namespace

static int64_t sort_padded(int64_t m) {
  int64_t p = SORT_CHUNK;
  while (p < m) p <<= 1;
  return p;
}
extern "C" int64_t rgnn_sort_scores_tmp_bytes(int64_t m) { return sort_padded(m) * 12 + 256; }

extern "C" int rgnn_sort_scores(const void* scores, int32_t is_f64, int64_t m, int64_t* order, void* tmp, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(m >= 0 && m < ((int64_t)1 << 31), "bad size");
  if (m == 0) return RGNN_OK;
  RGNN_CHECK_ARG(scores && order && tmp, "null pointers");
  const int64_t padded = sort_padded(m);
  unsigned long long* keys = (unsigned long long*)tmp;
  unsigned* ids = (unsigned*)((char*)tmp + padded * 8);
  hipStream_t s = (hipStream_t)stream;
  const unsigned chunks = (unsigned)(padded / SORT_CHUNK);
  hipLaunchKernelGGL(k_sort_chunk<0>, dim3(chunks), dim3(1024), 0, s, scores, (int)is_f64, m, padded, keys, ids, (int64_t)0);
  for (int64_t k = 2 * SORT_CHUNK; k <= padded; k <<= 1) {
    for (int64_t j = k >> 1; j >= SORT_CHUNK; j >>= 1)
      hipLaunchKernelGGL(k_sort_step, dim3(rgnn_blocks(padded, 256)), dim3(256), 0, s, keys, ids, padded, j, k);
    hipLaunchKernelGGL(k_sort_chunk<1>, dim3(chunks), dim3(1024), 0, s, scores, (int)is_f64, m, padded, keys, ids, k);
  }
  hipLaunchKernelGGL(k_sort_emit, dim3(rgnn_blocks(m, 256)), dim3(256), 0, s, (const unsigned*)ids, m, order);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

extern "C" int64_t rgnn_nms_mask_words(int64_t m) { return m * ((m + 63) / 64); }

extern "C" int rgnn_nms(const void* boxes, int32_t kind, const int64_t* order, int64_t m, double iou_threshold,
                        uint64_t* mask_tmp, int64_t* keep, int64_t* count, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(kind == 0 || kind == 1, "kind: 0 aligned float32 [m, 4], 1 rotated float64 [m, 5]");
  RGNN_CHECK_ARG(m >= 0 && count != nullptr, "bad sizes");
  if (m == 0) {
    hipMemsetAsync(count, 0, 8, (hipStream_t)stream);
    return RGNN_OK;
  }
  RGNN_CHECK_ARG(boxes && order && mask_tmp && keep, "null pointers");
  const int words = (int)((m + 63) / 64);
  if (words > NMS_MAX_WORDS) {
    rgnn_set_error("rgnn_nms: at most %d boxes per call (got %lld)", NMS_MAX_WORDS * 64, (long long)m);
    return RGNN_ERR_UNSUPPORTED;
  }
  if (kind == 0)
    hipLaunchKernelGGL(k_nms_mask<0>, dim3(words, words), dim3(64), 0, (hipStream_t)stream, boxes, order, m, iou_threshold,
                       (unsigned long long*)mask_tmp, words);
  else
    hipLaunchKernelGGL(k_nms_mask<1>, dim3(words, words), dim3(64), 0, (hipStream_t)stream, boxes, order, m, iou_threshold,
                       (unsigned long long*)mask_tmp, words);
  hipLaunchKernelGGL(k_nms_reduce, dim3(1), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)mask_tmp, order, m,
                     words, keep, count);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Segmented suppression: what Postprocessor._finish -> BoxSuppressor.apply_nms computes for one frame, for every frame of a
// batch in two launches, whatever the number of frames.  k_nms_frames, one work-group per frame: (1) order-preserving
// compaction of the frame's nodes with keep != 0 into the frame's own slots [frame_ptr[f], ...); (2) box_repr per candidate,
// the frame's own minimum (NaN propagates, as torch.min) and shift; (3) bitonic sort of (score_key, candidate) in LDS, the
// order of rgnn_sort_scores; (4) the greedy walk of k_nms_reduce, 64 sorted candidates at a time, with the IoUs computed
// where they are needed instead of an M x M mask: the tile's diagonal (the tile's boxes staged in LDS; lane = row, the waves
// share the columns), then every later candidate not yet removed against the boxes the tile kept (lane = candidate, the
// waves share the kept boxes).  The earlier box is the first argument of the IoU, as in k_nms_mask; rotated pairs too far
// apart to touch are decided without it (far_apart), the others are collected and evaluated one pair per lane.
// k_nms_frames_emit: offsets of the kept boxes of every frame and the gathered outputs.  A frame of more than SORT_CHUNK
// candidates is left empty (its candidate count tells the host).
// ------------------------------------------------------------------------------------------------------------------
namespace {
constexpr int NMSF_THREADS = 1024;
constexpr int NMSF_WAVES = NMSF_THREADS / 64;

struct NmsFramesParams {
  const int32_t* label; const float* score; const int32_t* keep; const double* corners;
  const int64_t* frame_ptr; int64_t n; int64_t n_frames;
  double thr;
  int32_t* cand_node;        // [n]    slot -> node id; the slots of frame f start at frame_ptr[f]
  int32_t* kept_slot;        // [n]    slots kept, in suppression order, from frame_ptr[f]
  double* rep64;             // [n, 5] float64 representation (shifted in place for rotated boxes)
  float* rep32;              // [n, 4] aligned boxes: the shifted matrix rounded to float32
  double* shift;             // [n_frames]
  int32_t* kept_cnt;         // [n_frames]
  int64_t* node_out; double* labels_out; void* scores_out; void* corners_out;
  int64_t* meta;             // kept_ptr [n_frames + 1] | candidates per frame [n_frames]
};

// Rotated boxes whose centres lie further apart than their circumscribed circles reach, by a margin (5e-5 of that reach) far
// above the rounding of iou_rotated's own arithmetic (1e-16 of the coordinates about the pair's common centre): the clip in
// iou_rotated leaves nothing, so it returns 0, at most a sliver of rounding; for a threshold above NMSF_FAR_MIN_THR
// `iou_rotated(p, q) >= thr` is then false and the evaluation is skipped (at radar densities that is nearly every pair).
// NaN or infinite input compares false here and takes the full evaluation.
constexpr double NMSF_FAR_MIN_THR = 1e-9;
__device__ __forceinline__ double circumradius(const double* b) { return 0.5 * sqrt(b[2] * b[2] + b[3] * b[3]); }
__device__ __forceinline__ bool far_apart(const double* p, double rp, const double* q, double rq) {
  const double dx = p[0] - q[0], dy = p[1] - q[1], r = rp + rq;
  return dx * dx + dy * dy > 1.0001 * (r * r);
}

// One body of iou_rotated for the four places of k_nms_frames that need it (inlined four times it spills 1 KB per lane).
__device__ __noinline__ bool rotated_hit(const double* p, const double* q, double thr) { return iou_rotated(p, q) >= thr; }

__device__ __forceinline__ int64_t clamp_ptr(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int KIND>
__global__ __launch_bounds__(NMSF_THREADS) void k_nms_frames(const NmsFramesParams p) {
  using T = typename std::conditional<KIND == 0, float, double>::type;
  constexpr int BW = KIND == 0 ? 4 : 5;
  __shared__ unsigned long long sk[SORT_CHUNK];
  __shared__ unsigned si[SORT_CHUNK];
  __shared__ unsigned long long removed[SORT_CHUNK / 64];
  __shared__ unsigned long long diag[64];
  __shared__ T tbox[64][BW];
  __shared__ double tbox_r[64];
  __shared__ int kidx[64];
  __shared__ int n_pairs;
  __shared__ double red_min[NMSF_WAVES];
  __shared__ int red_i[NMSF_WAVES];
  __shared__ unsigned long long kept_bits;
  const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t a = clamp_ptr(p.frame_ptr[f], 0, p.n), b = clamp_ptr(p.frame_ptr[f + 1], a, p.n);

  // (1) candidates, in node order
  int m = 0;
  for (int64_t base = a; base < b; base += NMSF_THREADS) {
    const int64_t i = base + t;
    const bool flag = i < b && p.keep[i] != 0;
    const unsigned long long bal = __ballot(flag);
    if (lane == 0) red_i[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < NMSF_WAVES; w++) {
      const int c = red_i[w];
      if (w < wave) before += c;
      total += c;
    }
    if (flag) p.cand_node[a + m + before + __popcll(bal & ((1ull << lane) - 1ull))] = (int32_t)i;
    m += total;
    __syncthreads();
  }
  if (t == 0) p.meta[p.n_frames + 1 + f] = m;
  if (m == 0 || m > SORT_CHUNK) {
    if (t == 0) { p.kept_cnt[f] = 0; p.shift[f] = 0.0; }
    return;
  }

  // (2) representation, the frame's minimum and shift (postprocessing.py:358-361, 391-394)
  double lo = INFINITY;
  bool has_nan = false;
  for (int c = t; c < m; c += NMSF_THREADS) {
    const int64_t slot = a + c;
    const double* src = p.corners + (int64_t)p.cand_node[slot] * 8;
    double r[5];
    if constexpr (KIND == 0) box_repr(src, r, nullptr);
    else box_repr(src, nullptr, r);
    constexpr int NMIN = KIND == 0 ? 4 : 2;
    for (int q = 0; q < NMIN; q++) {
      if (r[q] != r[q]) has_nan = true;
      else lo = fmin(lo, r[q]);
    }
    for (int q = 0; q < BW; q++) p.rep64[slot * 5 + q] = r[q];
  }
  for (int o = 32; o > 0; o >>= 1) lo = fmin(lo, __shfl_xor(lo, o, 64));
  const bool wave_nan = __ballot(has_nan) != 0ull;
  if (lane == 0) { red_min[wave] = lo; red_i[wave] = wave_nan ? 1 : 0; }
  for (int w = t; w < SORT_CHUNK / 64; w += NMSF_THREADS) removed[w] = 0ull;
  __syncthreads();
  bool any_nan = false;
  for (int w = 0; w < NMSF_WAVES; w++) { lo = fmin(lo, red_min[w]); any_nan = any_nan || red_i[w] != 0; }
  const double shift = (!any_nan && lo < 0) ? fabs(lo) + 100.0 : 0.0;
  if (t == 0) p.shift[f] = shift;
  for (int c = t; c < m; c += NMSF_THREADS) {           // (the rows this thread wrote above)
    const int64_t slot = a + c;
    if constexpr (KIND == 1) {
      if (shift != 0.0) { p.rep64[slot * 5] += shift; p.rep64[slot * 5 + 1] += shift; }
    } else {
      for (int q = 0; q < 4; q++) {
        const double v = p.rep64[slot * 5 + q];
        p.rep32[slot * 4 + q] = (float)(shift != 0.0 ? v + shift : v);
      }
    }
  }

  // (3) order: the network of k_sort_chunk over the next power of two (padding sorts after every real pair)
  int p2 = 1;
  while (p2 < m) p2 <<= 1;
  for (int c = t; c < p2; c += NMSF_THREADS) {
    if (c < m) { sk[c] = score_key((double)p.score[p.cand_node[a + c]]); si[c] = (unsigned)c; }
    else { sk[c] = 0ull; si[c] = 0xffffffffu; }
  }
  __syncthreads();
  for (int k = 2; k <= p2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int c = t; c < p2; c += NMSF_THREADS) {
        const int q = c ^ j;
        if (q > c) {
          const bool up = ((c & k) == 0);
          const unsigned long long ka = sk[c], kb = sk[q];
          const unsigned ia = si[c], ib = si[q];
          if (sort_before(kb, ib, ka, ia) == up) { sk[c] = kb; si[c] = ib; sk[q] = ka; si[q] = ia; }
        }
      }
      __syncthreads();
    }
  }

  // (4) greedy suppression over the sorted candidates.  Rotated pairs that may touch wait in a list (the space of the sort
  // keys, which are dead) and get their IoU one pair per lane: evaluated where they are found, a wave would run iou_rotated
  // for one or two of its lanes.  A full list only means that the rest is evaluated in place.
  const T* rep = KIND == 0 ? (const T*)p.rep32 : (const T*)p.rep64;
  const float thr32 = (float)p.thr;
  const bool skip_far = p.thr > NMSF_FAR_MIN_THR;
  volatile unsigned long long* removed_now = removed;
  unsigned* pairs = (unsigned*)sk;                         // (first << 16) | second
  constexpr int PAIR_CAP = SORT_CHUNK * 2;
  int n_keep = 0;
  const int tiles = (m + 63) / 64;
  for (int bt = 0; bt < tiles; bt++) {
    const int nrow = m - bt * 64 < 64 ? m - bt * 64 : 64;
    if (t < 64) {                                          // the tile's boxes
      diag[t] = 0ull;
      if (t < nrow) {
        const T* src = rep + (a + si[bt * 64 + t]) * BW;
        for (int q = 0; q < BW; q++) tbox[t][q] = src[q];
        if constexpr (KIND == 1) tbox_r[t] = circumradius(tbox[t]);
      }
      if (t == 0) n_pairs = 0;
    }
    __syncthreads();
    const unsigned long long cur0 = removed[bt];
    if (lane < nrow && !((cur0 >> lane) & 1ull)) {       // diagonal tile: row = lane, the waves share the columns
      unsigned long long bits = 0ull;
      for (int c = lane + 1 + wave; c < nrow; c += NMSF_WAVES) {
        if ((cur0 >> c) & 1ull) continue;
        if constexpr (KIND == 0) {
          if (iou_aligned(tbox[lane], tbox[c]) > thr32) bits |= 1ull << c;
        } else if (!(skip_far && far_apart(tbox[lane], tbox_r[lane], tbox[c], tbox_r[c]))) {
          const int e = atomicAdd(&n_pairs, 1);
          if (e < PAIR_CAP) pairs[e] = ((unsigned)lane << 16) | (unsigned)c;
          else if (rotated_hit(tbox[lane], tbox[c], p.thr)) bits |= 1ull << c;
        }
      }
      if (bits) atomicOr(&diag[lane], bits);
    }
    if constexpr (KIND == 1) {
      __syncthreads();
      const int np = n_pairs < PAIR_CAP ? n_pairs : PAIR_CAP;
      for (int e = t; e < np; e += NMSF_THREADS) {
        const int row = (int)(pairs[e] >> 16), c = (int)(pairs[e] & 0xffffu);
        if (rotated_hit(tbox[row], tbox[c], p.thr)) atomicOr(&diag[row], 1ull << c);
      }
    }
    __syncthreads();
    if (t < 64) {                                          // in-tile greedy pass (wave 0), as k_nms_reduce
      const unsigned long long d = diag[lane];
      unsigned long long cur = cur0, kb = 0ull;
      for (int l = 0; l < nrow; l++) {
        const unsigned long long row = __shfl(d, l, 64);
        if (!((cur >> l) & 1ull)) { kb |= 1ull << l; cur |= row; }
      }
      if ((kb >> lane) & 1ull) {
        const int rank = __popcll(kb & ((1ull << lane) - 1ull));
        p.kept_slot[a + n_keep + rank] = (int32_t)(a + si[bt * 64 + lane]);
        kidx[rank] = lane;
      }
      if (lane == 0) { kept_bits = kb; n_pairs = 0; }
    }
    __syncthreads();
    const unsigned long long kb = kept_bits;
    const int nk = __popcll(kb);
    n_keep += nk;
    for (int j0 = (bt + 1) * 64; j0 < m; j0 += 64) {       // later candidates: lane = candidate, the waves share the kept boxes
      const int j = j0 + lane;
      if (j < m && wave < nk && !((removed_now[j0 >> 6] >> lane) & 1ull)) {
        T mine[BW];
        const T* src = rep + (a + si[j]) * BW;
        for (int q = 0; q < BW; q++) mine[q] = src[q];
        bool hit = false;
        if constexpr (KIND == 0) {
          for (int r = wave; r < nk && !hit; r += NMSF_WAVES) hit = iou_aligned(tbox[kidx[r]], mine) > thr32;
        } else {
          const double my_r = circumradius(mine);
          for (int r = wave; r < nk; r += NMSF_WAVES) {
            const int k = kidx[r];
            if (skip_far && far_apart(tbox[k], tbox_r[k], mine, my_r)) continue;
            const int e = atomicAdd(&n_pairs, 1);
            if (e < PAIR_CAP) pairs[e] = ((unsigned)j << 16) | (unsigned)k;
            else if (!hit) hit = rotated_hit(tbox[k], mine, p.thr);
          }
        }
        if (hit) atomicOr(&removed[j0 >> 6], 1ull << lane);
      }
    }
    if constexpr (KIND == 1) {
      __syncthreads();
      const int np = n_pairs < PAIR_CAP ? n_pairs : PAIR_CAP;
      for (int e = t; e < np; e += NMSF_THREADS) {
        const int j = (int)(pairs[e] >> 16), k = (int)(pairs[e] & 0xffffu);
        if ((removed_now[j >> 6] >> (j & 63)) & 1ull) continue;
        T mine[BW];
        const T* src = rep + (a + si[j]) * BW;
        for (int q = 0; q < BW; q++) mine[q] = src[q];
        if (rotated_hit(tbox[k], mine, p.thr)) atomicOr(&removed[j >> 6], 1ull << (j & 63));
      }
    }
    __syncthreads();
  }
  if (t == 0) p.kept_cnt[f] = n_keep;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_nms_frames_emit(const NmsFramesParams p) {
  __shared__ long long red[256];
  const int f = blockIdx.x, t = threadIdx.x;
  long long part = 0;
  for (int i = t; i < f; i += 256) part += p.kept_cnt[i];
  red[t] = part;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const int64_t offset = red[0];
  const int cnt = p.kept_cnt[f];
  if (t == 0) {
    p.meta[f] = offset;
    if (f == p.n_frames - 1) p.meta[f + 1] = offset + cnt;
  }
  const int64_t a = clamp_ptr(p.frame_ptr[f], 0, p.n);
  const double shift = p.shift[f];
  for (int k = t; k < cnt; k += 256) {
    const int64_t slot = p.kept_slot[a + k], node = p.cand_node[slot], o = offset + k;
    p.node_out[o] = node;
    p.labels_out[o] = (double)p.label[node];
    if constexpr (KIND == 1) {                             // rotated: the decoded corners, float64 scores
      ((double*)p.scores_out)[o] = (double)p.score[node];
      for (int q = 0; q < 8; q++) ((double*)p.corners_out)[o * 8 + q] = p.corners[node * 8 + q];
    } else {                                               // aligned: rebuilt from the float32 matrix (postprocessing.py:416-423)
      ((float*)p.scores_out)[o] = p.score[node];
      float v[4];
      for (int q = 0; q < 4; q++) v[q] = p.rep32[slot * 4 + q];
      if (shift != 0.0) {
        const float s32 = (float)shift;
        for (int q = 0; q < 4; q++) v[q] = v[q] - s32;
      }
      float* out = (float*)p.corners_out + o * 8;
      out[0] = v[0]; out[1] = v[1]; out[2] = v[0]; out[3] = v[3];
      out[4] = v[2]; out[5] = v[1]; out[6] = v[2]; out[7] = v[3];
    }
  }
}

struct NmsFramesTmp { int64_t cand_node, kept_slot, rep64, rep32, shift, kept_cnt, total; };
NmsFramesTmp nms_frames_tmp(int64_t n, int64_t n_frames) {
  NmsFramesTmp l;
  int64_t at = 0;
  auto take = [&](int64_t bytes) { const int64_t here = at; at = rgnn_align_up(at + bytes, 256); return here; };
  l.cand_node = take(n * 4);
  l.kept_slot = take(n * 4);
  l.rep64 = take(n * 40);
  l.rep32 = take(n * 16);
  l.shift = take(n_frames * 8);
  l.kept_cnt = take(n_frames * 4);
  l.total = at + 256;
  return l;
}
}  // namespace

extern "C" int64_t rgnn_nms_frames_max_candidates(void) { return SORT_CHUNK; }

extern "C" int64_t rgnn_nms_frames_tmp_bytes(int64_t n, int64_t n_frames) {
  return nms_frames_tmp(n < 0 ? 0 : n, n_frames < 0 ? 0 : n_frames).total;
}

extern "C" int rgnn_nms_frames(const int32_t* label, const float* score, const int32_t* keep, const double* corners,
                               const int64_t* frame_ptr, int64_t n, int64_t n_frames, int32_t kind, double iou_threshold,
                               void* tmp, int64_t* node, double* labels_out, void* scores_out, void* corners_out, int64_t* meta,
                               rgnn_stream_t stream) {
  RGNN_CHECK_ARG(kind == 0 || kind == 1, "kind: 0 aligned (float32 corners and scores out), 1 rotated (float64 out)");
  RGNN_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31) && n_frames >= 0 && n_frames < ((int64_t)1 << 31), "bad sizes");
  RGNN_CHECK_ARG(meta != nullptr, "null pointers");
  if (n_frames == 0) {
    hipMemsetAsync(meta, 0, 8, (hipStream_t)stream);
    return RGNN_OK;
  }
  RGNN_CHECK_ARG(frame_ptr && tmp, "null pointers");
  RGNN_CHECK_ARG(n == 0 || (label && score && keep && corners && node && labels_out && scores_out && corners_out), "null pointers");
  const NmsFramesTmp l = nms_frames_tmp(n, n_frames);
  char* base = (char*)tmp;
  NmsFramesParams p{label, score, keep, corners, frame_ptr, n, n_frames, iou_threshold,
                    (int32_t*)(base + l.cand_node), (int32_t*)(base + l.kept_slot), (double*)(base + l.rep64),
                    (float*)(base + l.rep32), (double*)(base + l.shift), (int32_t*)(base + l.kept_cnt),
                    node, labels_out, scores_out, corners_out, meta};
  hipStream_t s = (hipStream_t)stream;
  if (kind == 0) {
    hipLaunchKernelGGL(k_nms_frames<0>, dim3((unsigned)n_frames), dim3(NMSF_THREADS), 0, s, p);
    hipLaunchKernelGGL(k_nms_frames_emit<0>, dim3((unsigned)n_frames), dim3(256), 0, s, p);
  } else {
    hipLaunchKernelGGL(k_nms_frames<1>, dim3((unsigned)n_frames), dim3(NMSF_THREADS), 0, s, p);
    hipLaunchKernelGGL(k_nms_frames_emit<1>, dim3((unsigned)n_frames), dim3(256), 0, s, p);
  }
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}
