// The nuScenes detection evaluation on the device: what the reference's NuscenesEvaluator does after the post-processor.
//   submission records of the predicted boxes            postprocessor/nuscenes/utils.py:11-140,246-309
//   range / point-count / bike-rack filter of the boxes  devkit eval/common/loaders.py add_center_dist, filter_eval_boxes
//   greedy centre-distance matching and the TP errors    devkit eval/detection/algo.py accumulate (the inner loop), eval/common/utils.py
//   precision / confidence / TP-error tables             devkit eval/detection/algo.py accumulate (after the loop), utils.py cummean
// Everything is packed over the whole list of samples with int64 offset arrays; no kernel is launched per sample or per class.
// float64 throughout, built with -ffp-contract=off like the rest of the library: no fused multiply-adds.
//
// UNPINNED: neither the nuscenes-devkit nor pyquaternion was ever executed against this file.  The semantics are restated from their
// published sources: the rotation matrix of a quaternion is that of the NORMALISED quaternion (the convention of nuscenes.hip),
// pyquaternion's yaw_pitch_roll[0] is atan2(2 (w z - x y), 1 - 2 (y^2 + z^2)), the devkit's quaternion_yaw is the atan2 of the first
// column of the rotation matrix, np.interp takes the LAST interval whose left end is <= x.  np.interp's fall-back for a NaN result
// (infinite slopes, non-finite tables) is not restated: every table here is finite.
#include "common.h"
#include <math.h>

namespace {

constexpr double PI_D = 3.141592653589793;

// index f of the segment of ptr [n_seg + 1] (ascending) that holds position x; the last such f when empty segments share it
__device__ __forceinline__ int64_t segment_of(const int64_t* __restrict__ ptr, int64_t n_seg, int64_t x) {
  int64_t lo = 0, hi = n_seg;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (ptr[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void quat_unit(const double* q, double& w, double& x, double& y, double& z) {
  w = q[0]; x = q[1]; y = q[2]; z = q[3];
  const double n = sqrt(((w * w + x * x) + y * y) + z * z);
  w = w / n; x = x / n; y = y / n; z = z / n;
}

// Rotation matrix (row-major) of the quaternion q = (w, x, y, z) after normalising it (the statement of nuscenes.hip).
__device__ __forceinline__ void quat_matrix(const double* q, double* R) {
  double w, x, y, z;
  quat_unit(q, w, x, y, z);
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w);     R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w);     R[7] = 2 * (y * z + x * w);     R[8] = 1 - 2 * (x * x + y * y);
}

// ------------------------------------------------------------------------------------------------------------------
// 1. Submission records, one thread per box (utils.py:246-309): vehicle frame -> global frame with the sample's ego pose.
// ------------------------------------------------------------------------------------------------------------------
struct SubParams {
  const double* boxes; const int32_t* labels; int64_t n; const int64_t* box_ptr; int64_t n_samples;
  const double *ego_t, *ego_r, *heights; int n_heights;
  double *translation, *size, *rotation, *yaw; int32_t* status;
};

__global__ __launch_bounds__(256) void k_nse_submission(const SubParams p) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= p.n) return;
  const int32_t label = p.labels[m];
  if (label < 1 || label >= p.n_heights) {                  // 'void' or no name at all: the devkit would refuse the record
    atomicOr(p.status, RGNN_NUSC_EVAL_BAD_LABEL);
    return;
  }
  const int64_t s = segment_of(p.box_ptr, p.n_samples, m);
  const double* b = p.boxes + 5 * m;
  const double h = p.heights[label];
  double R[9], w, x, y, z;
  quat_matrix(p.ego_r + 4 * s, R);
  quat_unit(p.ego_r + 4 * s, w, x, y, z);
  const double yaw_e = atan2(2 * (w * z - x * y), 1 - 2 * (y * y + z * z));
  const double bx = b[0], by = b[1], bz = 0.0;
  p.translation[3 * m] = ((R[0] * bx + R[1] * by) + R[2] * bz) + p.ego_t[3 * s];
  p.translation[3 * m + 1] = ((R[3] * bx + R[4] * by) + R[5] * bz) + p.ego_t[3 * s + 1];
  p.translation[3 * m + 2] = (((R[6] * bx + R[7] * by) + R[8] * bz) + p.ego_t[3 * s + 2]) + h / 2;
  p.size[3 * m] = b[3]; p.size[3 * m + 1] = b[2]; p.size[3 * m + 2] = h;
  const double angle = b[4] * (PI_D / 180.0) + yaw_e;
  const double sn = sin(angle / 2);
  p.rotation[4 * m] = cos(angle / 2); p.rotation[4 * m + 1] = 0.0 * sn; p.rotation[4 * m + 2] = 0.0 * sn; p.rotation[4 * m + 3] = sn;
  p.yaw[m] = angle;
}

// ------------------------------------------------------------------------------------------------------------------
// 2. Filter, one thread per box; predictions (score given) and ground truth (num_pts given) alike.
// ------------------------------------------------------------------------------------------------------------------
struct FilterParams {
  const double* trans; const int32_t* name; int64_t n; const int64_t* ptr; int64_t n_samples;
  const double *ego_t, *class_range; int n_names;
  const int32_t* num_pts; const double* score; int max_boxes;
  const double *rack_c, *rack_s, *rack_r; const int64_t* rack_ptr; int64_t n_racks; int bicycle, motorcycle;
  uint8_t* keep; int32_t* status;
};

// the devkit's points_in_box on one point (wlh_factor 1): the projections of v = pt - corner 0 on the three edges that leave
// corner 0 lie inside [0, |edge|^2], both ends included
__device__ __forceinline__ bool in_box(const double* c, const double* wlh, const double* q, const double* pt) {
  double R[9];
  quat_matrix(q, R);
  const double hw = wlh[0] / 2, hl = wlh[1] / 2, hh = wlh[2] / 2;
  const double sx[4] = {hl, -hl, hl, hl}, sy[4] = {hw, hw, -hw, hw}, sz[4] = {hh, hh, hh, -hh};       // corners 0, 4, 1, 3
  double k[4][3];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int r = 0; r < 3; r++) k[a][r] = ((R[3 * r] * sx[a] + R[3 * r + 1] * sy[a]) + R[3 * r + 2] * sz[a]) + c[r];
  const double v[3] = {pt[0] - k[0][0], pt[1] - k[0][1], pt[2] - k[0][2]};
  bool in = true;
#pragma unroll
  for (int a = 1; a < 4; a++) {
    const double e0 = k[a][0] - k[0][0], e1 = k[a][1] - k[0][1], e2 = k[a][2] - k[0][2];
    const double ev = (e0 * v[0] + e1 * v[1]) + e2 * v[2], ee = (e0 * e0 + e1 * e1) + e2 * e2;
    in = in && 0.0 <= ev && ev <= ee;
  }
  return in;
}

__global__ __launch_bounds__(256) void k_nse_filter(const FilterParams p) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const int64_t s = segment_of(p.ptr, p.n_samples, i);
  if (p.max_boxes > 0 && p.ptr[s + 1] - p.ptr[s] > (int64_t)p.max_boxes) atomicOr(p.status, RGNN_NUSC_EVAL_TOO_MANY_BOXES);
  if (p.score && p.score[i] != p.score[i]) atomicOr(p.status, RGNN_NUSC_EVAL_NAN_SCORE);
  const int32_t nm = p.name[i];
  if (nm < 1 || nm >= p.n_names) {                          // no detection class: ground truth drops it, a prediction is an error
    if (p.score) atomicOr(p.status, RGNN_NUSC_EVAL_BAD_LABEL);
    p.keep[i] = 0;
    return;
  }
  const double dx = p.trans[3 * i] - p.ego_t[3 * s], dy = p.trans[3 * i + 1] - p.ego_t[3 * s + 1];
  bool k = sqrt(dx * dx + dy * dy) < p.class_range[nm];
  if (p.num_pts) k = k && p.num_pts[i] > 0;
  if (k && p.rack_ptr && (nm == p.bicycle || nm == p.motorcycle)) {
    int64_t a = p.rack_ptr[s], b = p.rack_ptr[s + 1];
    if (a < 0) a = 0;
    if (b > p.n_racks) b = p.n_racks;
    for (int64_t r = a; r < b && k; r++)
      if (in_box(p.rack_c + 3 * r, p.rack_s + 3 * r, p.rack_r + 4 * r, p.trans + 3 * i)) k = false;
  }
  p.keep[i] = k ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------------
// 3. Matching.  One wave per (sample, class, threshold).  The class's kept ground truth of the sample is compacted into LDS (in
//    list order); the sample's predictions are walked in the order the caller hands over (descending score, equal scores by
//    DESCENDING position), those of another class or dropped by the filter skipped.  Per prediction: lanes across the ground truth
//    not yet taken, minimum centre distance, lowest position on ties, matched iff the minimum is strictly below the threshold.
//    More than MATCH_CAP ground-truth boxes of one class in one sample set a status bit and leave the sample's class unmatched.
// ------------------------------------------------------------------------------------------------------------------
constexpr int MATCH_CAP = 512;

struct MatchParams {
  rgnn_eval_boxes pred, gt;
  int64_t n_samples;
  const int64_t* order;
  const int32_t* classes; int n_classes;
  const double* thresholds; int n_thresholds, tp_index;
  int barrier;
  int32_t* match; double* tp_err; int32_t* status;
};

// Python's float modulo for a positive divisor
__device__ __forceinline__ double py_mod(double a, double b) {
  double r = fmod(a, b);
  if (r != 0.0 && r < 0.0) r += b;
  return r;
}

__device__ __forceinline__ double quat_yaw(const double* q) {           // atan2 of the first column of the rotation matrix
  double w, x, y, z;
  quat_unit(q, w, x, y, z);
  return atan2(2 * (x * y + z * w), 1 - 2 * (y * y + z * z));
}

__global__ __launch_bounds__(RGNN_WAVE) void k_nse_match(const MatchParams p) {
  __shared__ int g_idx[MATCH_CAP];
  __shared__ double g_x[MATCH_CAP], g_y[MATCH_CAP];
  __shared__ unsigned char g_used[MATCH_CAP];
  const int lane = threadIdx.x;
  const int t = blockIdx.x % p.n_thresholds;
  const int32_t c = p.classes[(blockIdx.x / p.n_thresholds) % p.n_classes];
  const int64_t s = blockIdx.x / (p.n_thresholds * p.n_classes);
  const int64_t p0 = p.pred.ptr[s], p1 = p.pred.ptr[s + 1], g0 = p.gt.ptr[s], g1 = p.gt.ptr[s + 1];
  if (p0 < 0 || p1 < p0 || p1 > p.pred.n || g0 < 0 || g1 < g0 || g1 > p.gt.n) {
    if (lane == 0) atomicOr(p.status, RGNN_NUSC_EVAL_BAD_PTR);
    return;
  }
  if (p1 == p0) return;
  const unsigned long long below = (1ull << lane) - 1ull;
  int ng = 0;
  for (int64_t base = g0; base < g1; base += RGNN_WAVE) {
    const int64_t i = base + lane;
    const bool is = i < g1 && p.gt.name[i] == c && p.gt.keep[i];
    const unsigned long long m = __ballot(is);
    const int slot = ng + __popcll(m & below);
    if (is && slot < MATCH_CAP) {
      g_idx[slot] = (int)(i - g0);
      g_x[slot] = p.gt.translation[3 * i];
      g_y[slot] = p.gt.translation[3 * i + 1];
      g_used[slot] = 0;
    }
    ng += __popcll(m);
  }
  if (ng > MATCH_CAP) {                                      // over capacity: nothing was written past the arrays
    if (lane == 0) atomicOr(p.status, RGNN_NUSC_EVAL_GT_OVERFLOW);
    return;
  }
  if (ng == 0) return;
  __syncthreads();
  const double thr = p.thresholds[t];
  for (int64_t q = p0; q < p1; q++) {
    const int64_t id = p.order[q];
    if (id < p0 || id >= p1 || p.pred.name[id] != c || !p.pred.keep[id]) continue;          // (the whole wave)
    const double px = p.pred.translation[3 * id], py = p.pred.translation[3 * id + 1];
    double best = INFINITY;
    int pos = 0x7fffffff;
    for (int g = lane; g < ng; g += RGNN_WAVE) {
      if (g_used[g]) continue;
      const double dx = px - g_x[g], dy = py - g_y[g];
      const double d = sqrt(dx * dx + dy * dy);
      if (d < best) { best = d; pos = g; }
    }
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) {
      const double ob = __shfl_xor(best, sft);
      const int op = __shfl_xor(pos, sft);
      if (ob < best || (ob == best && op < pos)) { best = ob; pos = op; }
    }
    const bool hit = pos < ng && best < thr;
    if (hit && lane == 0) {
      g_used[pos] = 1;
      const int64_t g = g0 + g_idx[pos];
      p.match[(int64_t)t * p.pred.n + id] = (int32_t)g;
      if (t == p.tp_index) {
        const double *sa = p.gt.size + 3 * g, *sr = p.pred.size + 3 * id;
        const double va = (sa[0] * sa[1]) * sa[2], vr = (sr[0] * sr[1]) * sr[2];
        const double inter = (fmin(sa[0], sr[0]) * fmin(sa[1], sr[1])) * fmin(sa[2], sr[2]);
        const double period = c == p.barrier ? PI_D : 2 * PI_D;
        double diff = py_mod((quat_yaw(p.gt.rotation + 4 * g) - quat_yaw(p.pred.rotation + 4 * id)) + period / 2, period) - period / 2;
        if (diff > PI_D) diff = diff - 2 * PI_D;
        const double vx = p.pred.velocity[2 * id] - p.gt.velocity[2 * g], vy = p.pred.velocity[2 * id + 1] - p.gt.velocity[2 * g + 1];
        const int32_t ga = p.gt.attribute[g];
        p.tp_err[id] = best;
        p.tp_err[p.pred.n + id] = 1 - inter / ((va + vr) - inter);
        p.tp_err[2 * p.pred.n + id] = fabs(diff);
        p.tp_err[3 * p.pred.n + id] = sqrt(vx * vx + vy * vy);
        p.tp_err[4 * p.pred.n + id] = ga < 0 ? (double)NAN : (ga == p.pred.attribute[id] ? 0.0 : 1.0);
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------------
// 4. Curves.  One work-group per (class, threshold).  `order` lists the KEPT predictions class by class (cls_ptr [2, C]), inside
//    a class by descending score over all samples (equal scores by descending position).  Pass 1 walks the class's segment in
//    chunks of CURVE_THREADS with one block scan per chunk over eleven columns at once: the match flag, and for the dist_th_tp
//    threshold the five errors (NaN as 0) with their not-NaN flags.  It leaves the running tp count of every prediction, and for
//    the matched ones their confidence and the five running means, in the workspace.  Pass 2: one thread per recall grid point
//    finds the last prediction with recall <= x by bisection (np.interp).  Pass 3 (dist_th_tp only): one thread per (error, grid
//    point) resamples the running mean at the interpolated confidence, the arrays read backwards as the devkit reverses them.
// ------------------------------------------------------------------------------------------------------------------
constexpr int CURVE_THREADS = 256;
constexpr int CURVE_MAX_GRID = 128;
constexpr int N_ERR = 5;

struct CurveParams {
  const int64_t *order, *cls_ptr;
  const double* score; const int32_t* match; const double* tp_err; int64_t n_pred;
  const int32_t* gt_name; const uint8_t* gt_keep; int64_t n_gt;
  const int32_t* classes; int n_classes, n_thresholds, tp_index;
  const double* grid; int n_grid;
  double *precision, *confidence, *tp_curve;
  int32_t* cumtp; double *mconf, *cm;
};

__global__ __launch_bounds__(CURVE_THREADS) void k_nse_curves(const CurveParams p) {
  __shared__ int s_i[N_ERR + 1][CURVE_THREADS];
  __shared__ double s_d[N_ERR][CURVE_THREADS];
  __shared__ double s_conf[CURVE_MAX_GRID];
  __shared__ int s_npos;
  const int tid = threadIdx.x;
  const int it = blockIdx.x % p.n_thresholds, ic = blockIdx.x / p.n_thresholds;
  const int32_t c = p.classes[ic];
  const bool tp_block = it == p.tp_index;
  if (tid == 0) s_npos = 0;
  __syncthreads();
  int my_g = 0;
  for (int64_t g = tid; g < p.n_gt; g += CURVE_THREADS) my_g += p.gt_name[g] == c && p.gt_keep[g];
  if (my_g) atomicAdd(&s_npos, my_g);
  __syncthreads();
  const int npos = s_npos;
  const int64_t seg_lo = p.cls_ptr[ic], n = p.cls_ptr[p.n_classes + ic] - seg_lo;
  double* out_p = p.precision + ((int64_t)ic * p.n_thresholds + it) * p.n_grid;
  double* out_c = p.confidence + ((int64_t)ic * p.n_thresholds + it) * p.n_grid;
  double* out_e = p.tp_curve + (int64_t)ic * N_ERR * p.n_grid;
  int c_i[N_ERR + 1] = {0, 0, 0, 0, 0, 0};
  double c_d[N_ERR] = {0, 0, 0, 0, 0};
  if (npos > 0) {
    const int64_t* order = p.order + seg_lo;
    const int32_t* match = p.match + (int64_t)it * p.n_pred;
    int32_t* cumtp = p.cumtp + (int64_t)it * p.n_pred + seg_lo;
    for (int64_t base = 0; base < n; base += CURVE_THREADS) {
      const int64_t j = base + tid;
      int64_t id = 0;
      bool mt = false;
      int v_i[N_ERR + 1] = {0, 0, 0, 0, 0, 0};
      double v_d[N_ERR] = {0, 0, 0, 0, 0};
      if (j < n) {
        id = order[j];
        mt = match[id] >= 0;
        v_i[0] = mt;
        if (tp_block && mt) {
#pragma unroll
          for (int e = 0; e < N_ERR; e++) {
            const double v = p.tp_err[(int64_t)e * p.n_pred + id];
            const bool nan = v != v;
            v_d[e] = nan ? 0.0 : v;
            v_i[1 + e] = nan ? 0 : 1;
          }
        }
      }
#pragma unroll
      for (int e = 0; e <= N_ERR; e++) s_i[e][tid] = v_i[e];
#pragma unroll
      for (int e = 0; e < N_ERR; e++) s_d[e][tid] = v_d[e];
      __syncthreads();
      for (int sft = 1; sft < CURVE_THREADS; sft <<= 1) {
        int a_i[N_ERR + 1];
        double a_d[N_ERR];
#pragma unroll
        for (int e = 0; e <= N_ERR; e++) a_i[e] = tid >= sft ? s_i[e][tid - sft] : 0;
#pragma unroll
        for (int e = 0; e < N_ERR; e++) a_d[e] = tid >= sft ? s_d[e][tid - sft] : 0.0;
        __syncthreads();
#pragma unroll
        for (int e = 0; e <= N_ERR; e++) s_i[e][tid] += a_i[e];
#pragma unroll
        for (int e = 0; e < N_ERR; e++) s_d[e][tid] += a_d[e];
        __syncthreads();
      }
      if (j < n) {
        const int tp_j = c_i[0] + s_i[0][tid];
        cumtp[j] = tp_j;
        if (tp_block && mt) {
          const int64_t q = seg_lo + tp_j - 1;
          p.mconf[q] = p.score[id];
#pragma unroll
          for (int e = 0; e < N_ERR; e++) {
            const int cnt = c_i[1 + e] + s_i[1 + e][tid];
            p.cm[(int64_t)e * p.n_pred + q] = cnt > 0 ? (c_d[e] + s_d[e][tid]) / (double)cnt : 0.0;
          }
        }
      }
#pragma unroll
      for (int e = 0; e <= N_ERR; e++) c_i[e] += s_i[e][CURVE_THREADS - 1];
#pragma unroll
      for (int e = 0; e < N_ERR; e++) c_d[e] += s_d[e][CURVE_THREADS - 1];
      __syncthreads();
    }
  }
  const int m = c_i[0];
  if (npos == 0 || m == 0) {                                  // the devkit's no_predictions tables
    for (int k = tid; k < p.n_grid; k += CURVE_THREADS) { out_p[k] = 0.0; out_c[k] = 0.0; }
    if (tp_block)
      for (int k = tid; k < N_ERR * p.n_grid; k += CURVE_THREADS) out_e[k] = 1.0;
    return;
  }
  __syncthreads();                                            // the workspace written above is read by other threads below
  {
    const int64_t* order = p.order + seg_lo;
    const int32_t* ct = p.cumtp + (int64_t)it * p.n_pred + seg_lo;
    const double dn = (double)npos;
    for (int k = tid; k < p.n_grid; k += CURVE_THREADS) {
      const double x = p.grid[k];
      double pr = 0.0, cf = 0.0;
      if (x < (double)ct[0] / dn) {
        pr = (double)ct[0] / 1.0; cf = p.score[order[0]];
      } else if (!(x > (double)ct[n - 1] / dn)) {
        int64_t lo = 0, hi = n;
        while (hi - lo > 1) {
          const int64_t mid = (lo + hi) >> 1;
          if ((double)ct[mid] / dn <= x) lo = mid; else hi = mid;
        }
        const double xj = (double)ct[lo] / dn;
        const double pj = (double)ct[lo] / (double)(lo + 1), cj = p.score[order[lo]];
        if (lo == n - 1 || xj == x) {
          pr = pj; cf = cj;
        } else {
          const double xn = (double)ct[lo + 1] / dn;
          const double pn = (double)ct[lo + 1] / (double)(lo + 2), cn = p.score[order[lo + 1]];
          pr = ((pn - pj) / (xn - xj)) * (x - xj) + pj;
          cf = ((cn - cj) / (xn - xj)) * (x - xj) + cj;
        }
      }
      out_p[k] = pr; out_c[k] = cf; s_conf[k] = cf;
    }
  }
  if (!tp_block) return;
  __syncthreads();
  const double* mc = p.mconf + seg_lo;
  for (int idx = tid; idx < N_ERR * p.n_grid; idx += CURVE_THREADS) {
    const int e = idx / p.n_grid, k = idx % p.n_grid;
    const double* f = p.cm + (int64_t)e * p.n_pred + seg_lo;
    double val;
    if (c_i[1 + e] == 0) {                                    // every value NaN: cummean is all ones
      val = 1.0;
    } else {
      const double x = s_conf[k];
      if (x < mc[m - 1]) val = f[m - 1];
      else if (x > mc[0]) val = f[0];
      else {
        int lo = -1, hi = m - 1;                              // the first q with mc[q] <= x (mc does not rise)
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (mc[mid] <= x) hi = mid; else lo = mid;
        }
        if (hi == 0 || mc[hi] == x) val = f[hi];
        else val = ((f[hi - 1] - f[hi]) / (mc[hi - 1] - mc[hi])) * (x - mc[hi]) + f[hi];
      }
    }
    out_e[idx] = val;
  }
}

inline bool clear_status(int32_t* status, hipStream_t s) { return hipMemsetAsync(status, 0, sizeof(int32_t), s) == hipSuccess; }

}  // namespace

extern "C" int rgnn_nuscenes_submission(const double* boxes, const int32_t* labels, int64_t n_boxes, const int64_t* box_ptr,
                                        int64_t n_samples, const double* ego_translation, const double* ego_rotation,
                                        const double* heights, int32_t n_heights, double* translation, double* size, double* rotation,
                                        double* yaw, int32_t* status, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n_boxes >= 0 && n_samples >= 0 && n_heights >= 0, "bad sizes");
  RGNN_CHECK_ARG(status, "null status");
  hipStream_t s = (hipStream_t)stream;
  if (!clear_status(status, s)) {
    rgnn_set_error("rgnn_nuscenes_submission: clearing the status word failed");
    return RGNN_ERR_LAUNCH;
  }
  if (n_boxes == 0) return RGNN_OK;
  RGNN_CHECK_ARG(n_samples >= 1, "boxes without a sample");
  RGNN_CHECK_ARG(boxes && labels && box_ptr && ego_translation && ego_rotation && heights && translation && size && rotation && yaw,
                 "null pointers");
  const SubParams p{boxes, labels, n_boxes, box_ptr, n_samples, ego_translation, ego_rotation, heights, (int)n_heights,
                    translation, size, rotation, yaw, status};
  hipLaunchKernelGGL(k_nse_submission, dim3(rgnn_blocks(n_boxes, 256)), dim3(256), 0, s, p);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

extern "C" int rgnn_detection_filter(const double* translation, const int32_t* name, int64_t n_boxes, const int64_t* ptr,
                                     int64_t n_samples, const double* ego_translation, const double* class_range, int32_t n_names,
                                     const int32_t* num_pts, const double* score, int32_t max_boxes, const double* rack_center,
                                     const double* rack_size, const double* rack_rotation, const int64_t* rack_ptr, int64_t n_racks,
                                     int32_t bicycle, int32_t motorcycle, uint8_t* keep, int32_t* status, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n_boxes >= 0 && n_samples >= 0 && n_names >= 0 && n_racks >= 0, "bad sizes");
  RGNN_CHECK_ARG(status, "null status");
  hipStream_t s = (hipStream_t)stream;
  if (!clear_status(status, s)) {
    rgnn_set_error("rgnn_detection_filter: clearing the status word failed");
    return RGNN_ERR_LAUNCH;
  }
  if (n_boxes == 0) return RGNN_OK;
  RGNN_CHECK_ARG(n_samples >= 1, "boxes without a sample");
  RGNN_CHECK_ARG(translation && name && ptr && ego_translation && class_range && keep, "null pointers");
  RGNN_CHECK_ARG(!rack_ptr || n_racks == 0 || (rack_center && rack_size && rack_rotation), "bike racks without their boxes");
  const FilterParams p{translation, name, n_boxes, ptr, n_samples, ego_translation, class_range, (int)n_names, num_pts, score,
                       (int)max_boxes, rack_center, rack_size, rack_rotation, rack_ptr, n_racks, (int)bicycle, (int)motorcycle,
                       keep, status};
  hipLaunchKernelGGL(k_nse_filter, dim3(rgnn_blocks(n_boxes, 256)), dim3(256), 0, s, p);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

extern "C" int32_t rgnn_center_match_capacity(void) { return MATCH_CAP; }

extern "C" int rgnn_center_match(const rgnn_eval_boxes* pred, const rgnn_eval_boxes* gt, int64_t n_samples, const int64_t* order,
                                 const int32_t* classes, int32_t n_classes, const double* thresholds, int32_t n_thresholds,
                                 int32_t tp_index, int32_t barrier, int32_t* match, double* tp_err, int32_t* status,
                                 rgnn_stream_t stream) {
  RGNN_CHECK_ARG(pred && gt, "null box lists");
  RGNN_CHECK_ARG(n_samples >= 0 && pred->n >= 0 && gt->n >= 0 && n_classes >= 0 && n_thresholds >= 0, "bad sizes");
  RGNN_CHECK_ARG(tp_index >= 0 && (tp_index < n_thresholds || n_thresholds == 0), "tp_index is no threshold");
  RGNN_CHECK_ARG(status, "null status");
  RGNN_CHECK_ARG(pred->n < ((int64_t)1 << 31) && gt->n < ((int64_t)1 << 31), "too many boxes");
  const int64_t waves = n_samples * (int64_t)n_classes * (int64_t)n_thresholds;
  RGNN_CHECK_ARG(waves < ((int64_t)1 << 31), "too many (sample, class, threshold) triples");
  hipStream_t s = (hipStream_t)stream;
  if (!clear_status(status, s)) {
    rgnn_set_error("rgnn_center_match: clearing the status word failed");
    return RGNN_ERR_LAUNCH;
  }
  if (pred->n == 0) return RGNN_OK;
  RGNN_CHECK_ARG((match || n_thresholds == 0) && tp_err, "null outputs");
  // all bits set: -1 in match, NaN in tp_err
  if ((n_thresholds > 0 && hipMemsetAsync(match, 0xff, (size_t)pred->n * (size_t)n_thresholds * sizeof(int32_t), s) != hipSuccess) ||
      hipMemsetAsync(tp_err, 0xff, (size_t)pred->n * N_ERR * sizeof(double), s) != hipSuccess) {
    rgnn_set_error("rgnn_center_match: clearing the outputs failed");
    return RGNN_ERR_LAUNCH;
  }
  if (waves == 0 || gt->n == 0) return RGNN_OK;
  RGNN_CHECK_ARG(pred->translation && pred->size && pred->rotation && pred->velocity && pred->name && pred->attribute && pred->keep &&
                 pred->ptr && gt->translation && gt->size && gt->rotation && gt->velocity && gt->name && gt->attribute && gt->keep &&
                 gt->ptr && order && classes && thresholds, "null pointers");
  const MatchParams p{*pred, *gt, n_samples, order, classes, (int)n_classes, thresholds, (int)n_thresholds, (int)tp_index,
                      (int)barrier, match, tp_err, status};
  hipLaunchKernelGGL(k_nse_match, dim3((unsigned)waves), dim3(RGNN_WAVE), 0, s, p);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

extern "C" int64_t rgnn_detection_curves_tmp_bytes(int64_t n_pred, int32_t n_thresholds) {
  if (n_pred < 0 || n_thresholds < 0) return -1;
  return rgnn_align_up(n_pred * (int64_t)n_thresholds * (int64_t)sizeof(int32_t), 8) + n_pred * (N_ERR + 1) * (int64_t)sizeof(double);
}

extern "C" int rgnn_detection_curves(const int64_t* order, const int64_t* cls_ptr, const double* score, const int32_t* match,
                                     const double* tp_err, int64_t n_pred, const int32_t* gt_name, const uint8_t* gt_keep,
                                     int64_t n_gt, const int32_t* classes, int32_t n_classes, int32_t n_thresholds, int32_t tp_index,
                                     const double* grid, int32_t n_grid, double* precision, double* confidence, double* tp_err_curve,
                                     void* tmp, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n_pred >= 0 && n_gt >= 0 && n_classes >= 0 && n_thresholds >= 0 && n_grid >= 1, "bad sizes");
  RGNN_CHECK_ARG(tp_index >= 0 && (tp_index < n_thresholds || n_thresholds == 0), "tp_index is no threshold");
  if (n_grid > CURVE_MAX_GRID) {
    rgnn_set_error("rgnn_detection_curves: at most %d recall grid points (got %d)", CURVE_MAX_GRID, (int)n_grid);
    return RGNN_ERR_UNSUPPORTED;
  }
  RGNN_CHECK_ARG(n_pred < ((int64_t)1 << 31) && n_gt < ((int64_t)1 << 31), "too many boxes");
  const int64_t blocks = (int64_t)n_classes * n_thresholds;
  if (blocks == 0) return RGNN_OK;
  RGNN_CHECK_ARG(classes && cls_ptr && grid && precision && confidence && tp_err_curve && ((gt_name && gt_keep) || n_gt == 0) &&
                 ((order && score && match && tp_err && tmp) || n_pred == 0), "null pointers");
  int32_t* cumtp = (int32_t*)tmp;
  double* mconf = (double*)((char*)tmp + rgnn_align_up(n_pred * (int64_t)n_thresholds * (int64_t)sizeof(int32_t), 8));
  const CurveParams p{order, cls_ptr, score, match, tp_err, n_pred, gt_name, gt_keep, n_gt, classes, (int)n_classes,
                      (int)n_thresholds, (int)tp_index, grid, (int)n_grid, precision, confidence, tp_err_curve, cumtp, mconf,
                      mconf + n_pred};
  hipLaunchKernelGGL(k_nse_curves, dim3((unsigned)blocks), dim3(CURVE_THREADS), 0, (hipStream_t)stream, p);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}
