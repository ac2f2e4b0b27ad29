// Ground-truth box targets on the device: GroundTruthCreator.create_2D_bounding_boxes
// (preprocessor/radarscenes/dataset_creation.py:232-521) -- per tracked object the convex hull of its points, the minimum-area
// rectangle flush with a hull edge (utils/math.py:304-439) and, per point, that rectangle relative to the point in one of four
// encodings (preprocessor/bounding_box.py:205-272, 344-416).  The inverse of rgnn_decode_ground_truth (postprocess.hip).
//
// One wave64 (one work-group) per object; the objects of the whole batch arrive in CSR form, so ONE launch serves any number of
// frames and objects.
//   staging     the object's points once into LDS as float64, x and y in arrays of their own: lane l reads 8 bytes at 8 l, so a
//               32-lane half covers all 64 banks once (conflict-free ds_read_b64); the reads of the hull loops below are wave
//               broadcasts of one address.
//   hull        gift wrap with wave reductions (DESIGN.md "Ground-truth targets"): from the lowest (x, y) point, every step takes the
//               point that has all others on its left -- lanes scan the points, a 6-stage xor butterfly on the INDEX reduces them
//               with the orientation test as the comparator (collinear: the farther one; coincident: the lower slot).  The comparator
//               is commutative bit for bit (a b' - a' b negates exactly), so every lane ends with the same winner.  At most n steps.
//   rectangle   lanes across hull edges; each projects all hull vertices onto its edge's unit vector and the orthogonal one
//               (bounding_area, utils/math.py:330-347); wave argmin of the area, the lowest hull position wins ties.
//   encoding    lanes across the object's points, each writes its own row.
// float64 throughout, separate multiplies and adds (the file is built with -ffp-contract=off like the rest of the library).
// Nothing here depends on scheduling: the only atomic is the OR into the status word.
//
// Cost: an object of n points and h hull vertices takes h (n / 64 + 6) comparator steps and h^2 / 64 projection steps, all on LDS
// broadcasts -- latency-bound chains of a few thousand cycles per wave, far below the float64 vector rate and below HBM (16 n bytes
// in, 40 n out).  What bounds a batch is the number of resident waves: 20 KB of LDS per object = 8 objects per CU at a time.
#include "common.h"
#include <math.h>

namespace {

constexpr int GT_CAP = 1024;                 // points of one object the LDS stage holds (RGNN_STATUS_GT_OBJECT_TOO_LARGE beyond)
constexpr double PI_D = 3.141592653589793;

struct GtParams {
  const double* pos; int64_t n;
  const int64_t* obj_ptr; const int32_t* obj_rows; int64_t n_rows;
  const int32_t* nn;
  int aligned, invariance;
  double* out; double* rect; int32_t* status;
};

__device__ __forceinline__ double round5(double x) { return rint(x * 100000.0) / 100000.0; }   // np.round(x, 5)
__device__ __forceinline__ double deg_of(double y, double x) { return atan2(y, x) * 180 / PI_D; }

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmin(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}

// The better of two candidates for "lowest (x, y), lowest slot"; -1 = none.
__device__ __forceinline__ int lower_point(int a, int b, const double* sx, const double* sy) {
  if (a < 0) return b;
  if (b < 0) return a;
  const double ax = sx[a], ay = sy[a], bx = sx[b], by = sy[b];
  if (ax != bx) return bx < ax ? b : a;
  if (ay != by) return by < ay ? b : a;
  return a < b ? a : b;
}

// The better of two candidates for the next hull vertex after (cx, cy), counter-clockwise: the one that has the other on its left;
// collinear: the farther one; the same place: the lower slot.  Symmetric in (a, b) bit for bit.
__device__ __forceinline__ int wrap_better(int a, int b, double cx, double cy, const double* sx, const double* sy) {
  if (a < 0) return b;
  if (b < 0) return a;
  const double ax = sx[a] - cx, ay = sy[a] - cy, bx = sx[b] - cx, by = sy[b] - cy;
  const double p = ax * by, q = ay * bx;
  if (p < q) return b;                                  // cross(a - c, b - c) < 0: b lies to the right of c -> a
  if (p > q) return a;
  const double da = ax * ax + ay * ay, db = bx * bx + by * by;
  if (db > da) return b;
  if (da > db) return a;
  return a < b ? a : b;
}

// min / max of the projections of the hull vertices on the unit vector of hull edge k and on its orthogonal (bounding_area)
struct EdgeRect { double ux, uy, ox, oy, min_p, len_p, min_o, len_o, area; };

__device__ __forceinline__ EdgeRect edge_rect(int k, int h, const int32_t* hull, const double* sx, const double* sy) {
  EdgeRect r;
  const int i0 = hull[k], i1 = hull[k + 1 == h ? 0 : k + 1];
  const double x0 = sx[i0], y0 = sy[i0], x1 = sx[i1], y1 = sy[i1];
  const double dis = sqrt((x0 - x1) * (x0 - x1) + (y0 - y1) * (y0 - y1));
  r.ux = (x1 - x0) / dis; r.uy = (y1 - y0) / dis;
  r.ox = -1 * r.uy; r.oy = r.ux;
  double min_p = INFINITY, max_p = -INFINITY, min_o = INFINITY, max_o = -INFINITY;
  for (int v = 0; v < h; v++) {
    const int i = hull[v];
    const double px = sx[i], py = sy[i];
    const double dp = r.ux * px + r.uy * py, dq = r.ox * px + r.oy * py;
    min_p = fmin(min_p, dp); max_p = fmax(max_p, dp);
    min_o = fmin(min_o, dq); max_o = fmax(max_o, dq);
  }
  r.min_p = min_p; r.min_o = min_o;
  r.len_p = max_p - min_p; r.len_o = max_o - min_o;
  r.area = r.len_p * r.len_o;
  return r;
}

__global__ __launch_bounds__(64) void k_gt_boxes(const GtParams p) {
  __shared__ double sx[GT_CAP];
  __shared__ double sy[GT_CAP];
  __shared__ int32_t hull[GT_CAP];
  const int lane = threadIdx.x;
  const int64_t o = blockIdx.x;
  const int64_t begin = p.obj_ptr[o], m64 = p.obj_ptr[o + 1] - begin;
  if (m64 <= 0) return;
  if (begin < 0 || begin + m64 > p.n_rows) {     // an offset outside the row list: refused, never read
    if (lane == 0) atomicOr(p.status, RGNN_STATUS_GT_DEGENERATE_OBJECT);
    return;
  }
  if (m64 > GT_CAP) {
    if (lane == 0) atomicOr(p.status, RGNN_STATUS_GT_OBJECT_TOO_LARGE);
    return;
  }
  const int m = (int)m64;
  const int32_t* rows = p.obj_rows + begin;

  bool bad = false;
  for (int j = lane; j < m; j += 64) {
    const int64_t r = rows[j];
    const bool ok = r >= 0 && r < p.n;
    bad = bad || !ok;
    sx[j] = ok ? p.pos[2 * r] : 0.0;
    sy[j] = ok ? p.pos[2 * r + 1] : 0.0;
  }
  __syncthreads();
  bool refuse = __any(bad);                    // a row outside the point array: refused like a degenerate object, never read

  // the object's absolute rectangle [cx, cy, l, w, theta in degrees), the same in every lane
  double cx = 0, cy = 0, l = 0.5, w = 0.5, theta = 0;
  if (!refuse && p.aligned) {
    if (m > 1) {
      double x_min = INFINITY, x_max = -INFINITY, y_min = INFINITY, y_max = -INFINITY;
      for (int j = lane; j < m; j += 64) {
        x_min = fmin(x_min, sx[j]); x_max = fmax(x_max, sx[j]);
        y_min = fmin(y_min, sy[j]); y_max = fmax(y_max, sy[j]);
      }
      x_min = wave_min(x_min); x_max = wave_max(x_max); y_min = wave_min(y_min); y_max = wave_max(y_max);
      // corners (x_min, y_min), (x_min, y_max), (x_max, y_min), (x_max, y_max) averaged in that order (utils/math.py:284-299,
      // bounding_box.py:396-416)
      cx = (((x_min + x_min) + x_max) + x_max) / 4;
      cy = (((y_min + y_max) + y_min) + y_max) / 4;
      l = fabs(x_min - x_max); w = fabs(y_min - y_max);
    } else {
      cx = sx[0]; cy = sy[0];
    }
  } else if (!refuse && m == 1) {
    cx = sx[0]; cy = sy[0];
  } else if (!refuse && m == 2) {               // dataset_creation.py:345-367: p1 is the lower row
    const double vx = sx[1] - sx[0], vy = sy[1] - sy[0];
    const double nrm = sqrt(vx * vx + vy * vy);
    if (!(nrm > 0)) {
      refuse = true;
    } else {
      cx = (sx[0] + sx[1]) / 2; cy = (sy[0] + sy[1]) / 2;
      theta = deg_of(vy / nrm, vx / nrm);
      if (theta < 0) theta = 180 + theta;
      if (theta >= 180) theta = theta - 180;
      l = nrm;
    }
  } else if (!refuse) {
    // ---- hull: gift wrap, counter-clockwise from the lowest (x, y) point
    int start = -1;
    for (int j = lane; j < m; j += 64) start = lower_point(start, j, sx, sy);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) start = lower_point(start, __shfl_xor(start, off), sx, sy);
    start = __shfl(start, 0);
    int h = 0, cur = start;
    bool closed = false;
    for (int it = 0; it < m; it++) {
      if (lane == 0) hull[h] = cur;
      h++;
      const double px = sx[cur], py = sy[cur];
      int next = -1;
      for (int j = lane; j < m; j += 64)
        if (sx[j] != px || sy[j] != py) next = wrap_better(next, j, px, py, sx, sy);
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) next = wrap_better(next, __shfl_xor(next, off), px, py, sx, sy);
      next = __shfl(next, 0);
      if (next < 0 || next == start) { closed = true; break; }
      cur = next;
    }
    __syncthreads();
    if (!closed || h < 3) {
      refuse = true;                              // all points on one line or in one place (or a walk that never closed: NaNs)
    } else {
      // ---- candidate rectangles: lanes across hull edges
      double best_area = INFINITY;
      int best_k = 0x7fffffff;
      for (int k = lane; k < h; k += 64) {
        const double a = edge_rect(k, h, hull, sx, sy).area;
        if (a < best_area) { best_area = a; best_k = k; }
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const double oa = __shfl_xor(best_area, off);
        const int ok = __shfl_xor(best_k, off);
        if (oa < best_area || (oa == best_area && ok < best_k)) { best_area = oa; best_k = ok; }
      }
      best_k = __shfl(best_k, 0);
      if (best_k >= h) {
        refuse = true;                            // no finite area at all
      } else {
        const EdgeRect r = edge_rect(best_k, h, hull, sx, sy);
        if (!(r.area > 0)) {
          refuse = true;
        } else {
          const double cp = r.min_p + r.len_p / 2, co = r.min_o + r.len_o / 2;
          cx = cp * r.ux + co * r.ox;
          cy = cp * r.uy + co * r.oy;
          const bool along = r.len_p >= r.len_o;      // the longer side gives the direction
          l = along ? r.len_p : r.len_o;
          w = along ? r.len_o : r.len_p;
          theta = along ? deg_of(r.uy, r.ux) : deg_of(r.oy, r.ox);
          if (theta < 0) theta = 180 + theta;
          if (theta >= 180) theta = theta - 180;
        }
      }
    }
  }
  if (refuse) {
    if (lane == 0) atomicOr(p.status, RGNN_STATUS_GT_DEGENERATE_OBJECT);
    return;
  }
  if (p.rect != nullptr && lane == 0) {
    double* r = p.rect + o * 5;
    r[0] = cx; r[1] = cy; r[2] = l; r[3] = w; r[4] = theta;
  }

  // ---- encoding: lanes across the object's points
  const int width = p.aligned ? 4 : 5;
  for (int j = lane; j < m; j += 64) {
    const int64_t row = rows[j];
    double* out = p.out + row * width;
    const double px = sx[j], py = sy[j];
    if (p.aligned) {
      out[0] = m == 1 ? 0.0 : cx - px;
      out[1] = m == 1 ? 0.0 : cy - py;
      out[2] = l; out[3] = w;
      continue;
    }
    if (m == 1) {                                 // dataset_creation.py:323-343
      out[0] = p.invariance == 0 ? px : 0.0;
      out[1] = p.invariance == 0 ? py : 0.0;
      out[2] = 0.5; out[3] = 0.5; out[4] = 0.0;
      continue;
    }
    const double xr = cx - px, yr = cy - py;
    if (p.invariance == 0) {                      // :390-391 (two points: the centre itself), :434-437 (the point plus its offset)
      out[0] = m == 2 ? cx : px + xr;
      out[1] = m == 2 ? cy : py + yr;
      out[2] = l; out[3] = w; out[4] = (theta * PI_D) / 180;
    } else if (p.invariance == 1) {
      out[0] = xr; out[1] = yr; out[2] = l; out[3] = w; out[4] = (theta * PI_D) / 180;
    } else {                                      // bounding_box.py:205-272
      const int64_t q = p.nn[row];
      if (q < 0 || q >= p.n) continue;            // no neighbour (a frame of one point): the row stays NaN
      const double vx = p.pos[2 * q] - px, vy = p.pos[2 * q + 1] - py;
      const double vn = sqrt(vx * vx + vy * vy);
      const double th_nn = deg_of(vy / vn, vx / vn);
      const double t = tan((theta * PI_D) / 180);
      const double dn = sqrt(1.0 + t * t);
      double a = round5(deg_of(t / dn, 1.0 / dn) - th_nn);
      if (a < 0) a = 360 + a;
      if (a >= 180) a = a - 180;
      const double d = sqrt(xr * xr + yr * yr);
      double b = 0.0;
      if (d != 0) {
        b = round5(deg_of(yr / d, xr / d) - th_nn);
        if (b < 0) b = 360 + b;
      }
      out[0] = d; out[1] = (b * PI_D) / 180; out[2] = l; out[3] = w; out[4] = (a * PI_D) / 180;
    }
  }
}

}  // namespace

extern "C" int32_t rgnn_gt_object_cap(void) { return GT_CAP; }

extern "C" int rgnn_create_gt_boxes(const double* pos, int64_t n, const int64_t* obj_ptr, const int32_t* obj_rows, int64_t n_rows,
                                    int64_t n_obj,                                    const int32_t* nn_index, int32_t aligned, int32_t invariance, double* out, double* rect,
                                    int32_t* status, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n >= 0 && n_rows >= 0 && n_obj >= 0 && n_obj < 2147483647, "bad sizes");
  RGNN_CHECK_ARG(invariance >= 0 && invariance <= 2, "invariance: 0 none, 1 translation, 2 en");
  if (n_obj == 0) return RGNN_OK;
  RGNN_CHECK_ARG(aligned || invariance != 2 || nn_index != nullptr, "the en representation needs nearest neighbours");
  RGNN_CHECK_ARG(pos && obj_ptr && obj_rows && out && status, "null pointers");
  const GtParams p{pos, n, obj_ptr, obj_rows, n_rows, aligned ? nullptr : nn_index, aligned ? 1 : 0, (int)invariance, out, rect, status};
  hipLaunchKernelGGL(k_gt_boxes, dim3((unsigned)n_obj), dim3(64), 0, (hipStream_t)stream, p);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}
