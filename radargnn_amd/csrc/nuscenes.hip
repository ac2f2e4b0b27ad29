// nuScenes samples into labelled point clouds on the device: get_sensor_points, crop_point_cloud, crop_bounding_boxes, get_labels
// (preprocessor/nuscenes/dataset_creation.py:121-165,189-201,241-278), extended_points_in_box (utils.py:22-48) and
// convert_bounding_boxes (conversion.py:112-187) with the rotated rectangle of preprocessor/bounding_box.py:344-394 -- the step in
// front of the graph build for the nuScenes half.  Three stages, float64 throughout, separate multiplies and adds (the file is
// built with -ffp-contract=off like the rest of the library):
//   points   one work-group per sample walks the sample's chunks (one chunk = the rows of one sensor) in tiles of NS_BLOCK rows:
//            rotate channels 0-2 and add the translation, rotate channels 8-9 by the upper-left 2 x 2, crop (a row goes only if it
//            lies strictly outside a limit), z is dropped.  A masked, order-preserving compaction in three launches -- count, scan,
//            write -- like preprocess.hip; count and write are ONE template, so they cannot disagree.
//   boxes    one wave per sample, lanes across its boxes: boxes without points go, the rest move to the vehicle frame
//            (c_v = R_e^T (c - t_e), R_v = R_e^T R_box), a centre on or outside a crop limit goes; survivors keep list order
//            (ballot ranks) and stay in their sample's segment [box_ptr[s], box_ptr[s] + box_count[s]) of the record array, so no
//            scan is needed.  Per survivor one record of NS_REC doubles: the membership geometry from corners(wlh_factor)
//            (p1, i, j as 3-vectors and their norms) and the rectangle from the bottom corners of corners(1).
//   label    one work-group per sample, lanes across points; the sample's records pass through LDS in stages of NS_STAGE boxes
//            (every lane reads the same record: broadcasts, no bank conflicts).  A point walks the boxes in list order and keeps
//            the LAST hit; it then writes its label and its five box columns in one of the three encodings.
// Nothing depends on scheduling: the only atomic is the OR into the status word.
//
// Cost.  points: 19 x 8 bytes in per row and pass (only 5 channels in the count pass), 72 bytes out: HBM-bound at any real size.
// boxes: 100 bytes in, 160 out, ~300 flops per box: launch latency.  label: P_s x K_s membership tests of 16 flops with two
// divisions each on LDS broadcasts -- for nuScenes (a few hundred points, a few dozen boxes per sample) 10^4 tests per work-group,
// bound by the float64 division rate of one CU; a batch of samples fills the machine with one work-group per sample.
#include "common.h"
#include <math.h>

namespace {

constexpr int NS_BLOCK = 256;                  // rows per tile = threads per work-group (points, label)
constexpr int NS_WAVES = NS_BLOCK / RGNN_WAVE;
constexpr int NS_REC = 20;                     // doubles per prepared box (160 bytes)
constexpr int NS_STAGE = 64;                   // boxes per LDS stage (10 KB)
constexpr int NS_CHANNELS = 19;
constexpr double PI_D = 3.141592653589793;

// record layout
enum { R_P1 = 0, R_I = 3, R_J = 6, R_NI = 9, R_NJ = 10, R_CX = 11, R_CY = 12, R_L = 13, R_W = 14, R_THETA = 15, R_LABEL = 16,
       R_SRC = 17 };

__device__ __forceinline__ double round5(double x) { return rint(x * 100000.0) / 100000.0; }   // np.round(x, 5)
__device__ __forceinline__ double deg_of(double y, double x) { return atan2(y, x) * 180 / PI_D; }

// Rotation matrix (row-major) of the quaternion q = (w, x, y, z) after normalising it.
__device__ __forceinline__ void quat_matrix(const double* q, double* R) {
  double w = q[0], x = q[1], y = q[2], z = q[3];
  const double n = sqrt(((w * w + x * x) + y * y) + z * z);
  w = w / n; x = x / n; y = y / n; z = z / n;
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w);     R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w);     R[7] = 2 * (y * z + x * w);     R[8] = 1 - 2 * (x * x + y * y);
}

// ---------------------------------------------------------------------------------------------------------------- points
struct NpParams {
  const double* pts; int64_t n_total;
  const int64_t* chunk_ptr; const int32_t* chunk_sample; const double* chunk_rot; const double* chunk_trans; int64_t n_chunks;
  int64_t n_samples;
  int32_t crop; double xlim, ylim;
  int64_t* counts;                             // [n_samples] (tmp)
  int64_t* frame_ptr;                          // [n_samples + 1]
  int64_t n_cap;
  double* X; double* V; double* V_cc; double* rcs; double* ts; int32_t* src_row;
  int32_t* status;
};

// The first chunk of sample s in the non-decreasing chunk_sample (an unsorted list only yields another index inside the list).
__device__ __forceinline__ int64_t first_chunk(const NpParams& p, int64_t s) {
  int64_t lo = 0, hi = p.n_chunks;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (p.chunk_sample[mid] < s) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <bool WRITE>
__global__ __launch_bounds__(NS_BLOCK) void k_ns_points(const NpParams p) {
  __shared__ int wsum[NS_WAVES];
  const int lane = threadIdx.x & (RGNN_WAVE - 1), wave = threadIdx.x / RGNN_WAVE;
  const int64_t s = blockIdx.x;
  int64_t base = WRITE ? p.frame_ptr[s] : 0;
  for (int64_t c = first_chunk(p, s); c < p.n_chunks && p.chunk_sample[c] == s; c++) {
    const int64_t a = p.chunk_ptr[c], b = p.chunk_ptr[c + 1];
    if (a < 0 || b < a || b > p.n_total) continue;          // refused by k_ns_scan's check of the lists, never read
    double R[9];
    quat_matrix(p.chunk_rot + 4 * c, R);
    const double tx = p.chunk_trans[3 * c], ty = p.chunk_trans[3 * c + 1];
    for (int64_t t = a; t < b; t += NS_BLOCK) {
      const int64_t r = t + threadIdx.x;
      bool keep = false;
      double x = 0, y = 0, vx = 0, vy = 0;
      if (r < b) {
        const double px = p.pts[r], py = p.pts[p.n_total + r], pz = p.pts[2 * p.n_total + r];
        x = ((R[0] * px + R[1] * py) + R[2] * pz) + tx;
        y = ((R[3] * px + R[4] * py) + R[5] * pz) + ty;
        keep = !(p.crop && (x > p.xlim || x < -p.xlim || y > p.ylim || y < -p.ylim));
        if (WRITE) {
          const double ux = p.pts[8 * p.n_total + r], uy = p.pts[9 * p.n_total + r];
          vx = R[0] * ux + R[1] * uy;
          vy = R[3] * ux + R[4] * uy;
        }
      }
      const unsigned long long bal = __ballot(keep);
      if (lane == 0) wsum[wave] = __popcll(bal);
      __syncthreads();
      int below = 0, all = 0;
#pragma unroll
      for (int i = 0; i < NS_WAVES; i++) {
        const int v = wsum[i];
        below += i < wave ? v : 0;
        all += v;
      }
      if (WRITE) {
        const int64_t at = base + below + __popcll(bal & ((1ull << lane) - 1ull));
        if (keep && at < p.n_cap) {                        // (always true for outputs sized for n_total and lists that pass the check)
          p.X[2 * at] = x; p.X[2 * at + 1] = y;
          p.V[2 * at] = vx; p.V[2 * at + 1] = vy;
          p.V_cc[2 * at] = p.pts[6 * p.n_total + r]; p.V_cc[2 * at + 1] = p.pts[7 * p.n_total + r];
          p.rcs[at] = p.pts[5 * p.n_total + r];
          p.ts[at] = p.pts[18 * p.n_total + r];
          p.src_row[at] = (int32_t)r;
        }
      }
      base += all;
      __syncthreads();                                     // wsum is rewritten by the next tile
    }
  }
  if (!WRITE && threadIdx.x == 0) p.counts[s] = base;
}

// counts -> frame_ptr (one wave), and the check of the chunk lists.
__global__ __launch_bounds__(RGNN_WAVE) void k_ns_scan(const NpParams p) {
  const int lane = threadIdx.x;
  bool bad = false;
  for (int64_t c = lane; c < p.n_chunks; c += RGNN_WAVE) {
    const int64_t s = p.chunk_sample[c], a = p.chunk_ptr[c], b = p.chunk_ptr[c + 1];
    bad = bad || s < 0 || s >= p.n_samples || (c > 0 && p.chunk_sample[c - 1] > s) || a < 0 || b < a || b > p.n_total;
  }
  if (__any(bad) && lane == 0) atomicOr(p.status, RGNN_STATUS_NUSC_BAD_CHUNK);
  long long carry = 0;
  if (lane == 0) p.frame_ptr[0] = 0;
  for (int64_t c = 0; c < p.n_samples; c += RGNN_WAVE) {
    const int64_t i = c + lane;
    long long v = i < p.n_samples ? (long long)p.counts[i] : 0;
#pragma unroll
    for (int off = 1; off < RGNN_WAVE; off <<= 1) {
      const long long u = __shfl_up(v, off);
      if (lane >= off) v += u;
    }
    if (i < p.n_samples) p.frame_ptr[i + 1] = carry + v;
    carry += __shfl(v, RGNN_WAVE - 1);
  }
}

// ----------------------------------------------------------------------------------------------------------------- boxes
struct NbParams {
  const double* center; const double* size; const double* rot; const int32_t* label; const int32_t* npts;
  const int64_t* box_ptr; int64_t n_boxes; int64_t n_samples;
  const double* ego_t; const double* ego_r;
  int32_t crop; double xlim, ylim, factor;
  double* rec; int32_t* box_count; int32_t* status;
};

// corner (sx, sy, sz) hl, hw, hh of a box with rotation R and centre c: R . (sx hl, sy hw, sz hh) + c  (devkit Box.corners)
__device__ __forceinline__ void corner(const double* R, const double* c, double bx, double by, double bz, double* o) {
  o[0] = ((R[0] * bx + R[1] * by) + R[2] * bz) + c[0];
  o[1] = ((R[3] * bx + R[4] * by) + R[5] * bz) + c[1];
  o[2] = ((R[6] * bx + R[7] * by) + R[8] * bz) + c[2];
}

__global__ __launch_bounds__(RGNN_WAVE) void k_ns_boxes(const NbParams p) {
  const int lane = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int64_t a = p.box_ptr[s], b = p.box_ptr[s + 1];
  if (a < 0 || b < a || b > p.n_boxes) {                   // offsets outside the box list: the sample has no boxes
    if (lane == 0) { atomicOr(p.status, RGNN_STATUS_NUSC_BAD_BOX_PTR); p.box_count[s] = 0; }
    return;
  }
  double Re[9];
  quat_matrix(p.ego_r + 4 * s, Re);
  const double t0 = p.ego_t[3 * s], t1 = p.ego_t[3 * s + 1], t2 = p.ego_t[3 * s + 2];
  int64_t base = a;
  for (int64_t t = a; t < b; t += RGNN_WAVE) {
    const int64_t m = t + lane;
    bool keep = false;
    double Rv[9], cv[3], wlh[3] = {0, 0, 0};
    if (m < b) {
      keep = p.npts[m] > 0;
      const double d0 = p.center[3 * m] + -t0, d1 = p.center[3 * m + 1] + -t1, d2 = p.center[3 * m + 2] + -t2;
#pragma unroll
      for (int r = 0; r < 3; r++) cv[r] = (Re[r] * d0 + Re[3 + r] * d1) + Re[6 + r] * d2;          // R_e^T (c - t_e)
      if (p.crop && !(-p.xlim < cv[0] && cv[0] < p.xlim && -p.ylim < cv[1] && cv[1] < p.ylim)) keep = false;
      double Rb[9];
      quat_matrix(p.rot + 4 * m, Rb);
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Rv[3 * r + c] = (Re[r] * Rb[c] + Re[3 + r] * Rb[3 + c]) + Re[6 + r] * Rb[6 + c];   // R_e^T R_box
      wlh[0] = p.size[3 * m]; wlh[1] = p.size[3 * m + 1]; wlh[2] = p.size[3 * m + 2];
    }
    const unsigned long long bal = __ballot(keep);
    if (keep) {
      double* o = p.rec + (base + __popcll(bal & ((1ull << lane) - 1ull))) * NS_REC;      // base + rank <= m < n_boxes
      // membership geometry from corners(wlh_factor): p1 = corner 0, i = corner 4 - p1, j = corner 1 - p1
      const double hw = (wlh[0] * p.factor) / 2, hl = (wlh[1] * p.factor) / 2, hh = (wlh[2] * p.factor) / 2;
      double c0[3], c4[3], c1[3];
      corner(Rv, cv, hl, hw, hh, c0);
      corner(Rv, cv, -hl, hw, hh, c4);
      corner(Rv, cv, hl, -hw, hh, c1);
      const double i0 = c4[0] - c0[0], i1 = c4[1] - c0[1], i2 = c4[2] - c0[2];
      const double j0 = c1[0] - c0[0], j1 = c1[1] - c0[1], j2 = c1[2] - c0[2];
      o[R_P1] = c0[0]; o[R_P1 + 1] = c0[1]; o[R_P1 + 2] = c0[2];
      o[R_I] = i0; o[R_I + 1] = i1; o[R_I + 2] = i2;
      o[R_J] = j0; o[R_J + 1] = j1; o[R_J + 2] = j2;
      o[R_NI] = sqrt((i0 * i0 + i1 * i1) + i2 * i2);
      o[R_NJ] = sqrt((j0 * j0 + j1 * j1) + j2 * j2);
      // rectangle from the bottom corners [2, 3, 7, 6] of corners(1), x and y only (bounding_box.py:344-394)
      const double gw = wlh[0] / 2, gl = wlh[1] / 2, gh = wlh[2] / 2;
      double p1[3], p2[3], p3[3], p4[3];
      corner(Rv, cv, gl, -gw, -gh, p1);
      corner(Rv, cv, gl, gw, -gh, p2);
      corner(Rv, cv, -gl, gw, -gh, p3);
      corner(Rv, cv, -gl, -gw, -gh, p4);
      const double a2x = p1[0] - p2[0], a2y = p1[1] - p2[1], a3x = p1[0] - p3[0], a3y = p1[1] - p3[1];
      const double a4x = p1[0] - p4[0], a4y = p1[1] - p4[1];
      const double e1 = sqrt(a2x * a2x + a2y * a2y), e2 = sqrt(a3x * a3x + a3y * a3y), e3 = sqrt(a4x * a4x + a4y * a4y);
      // w = min(d), d.remove(w), l = min(d): the first smallest goes, the smaller of the other two is the length
      double w = e1, ra = e2, rb = e3;
      if (e2 < w) { w = e2; ra = e1; rb = e3; }
      if (e3 < w) { w = e3; ra = e1; rb = e2; }
      const double l = rb < ra ? rb : ra;
      double vx, vy;                                       // the reference's == chain, in its order
      if (l == e1) { vx = a2x; vy = a2y; } else if (l == e2) { vx = a3x; vy = a3y; } else { vx = a4x; vy = a4y; }
      const double vn = sqrt(vx * vx + vy * vy);
      double theta = deg_of(vy / vn, vx / vn);
      if (theta < 0) theta = 180 + theta;                  // not wrapped at 180
      o[R_CX] = (((p1[0] + p2[0]) + p3[0]) + p4[0]) / 4;
      o[R_CY] = (((p1[1] + p2[1]) + p3[1]) + p4[1]) / 4;
      o[R_L] = l; o[R_W] = w; o[R_THETA] = theta;
      o[R_LABEL] = (double)p.label[m];
      o[R_SRC] = (double)m;
      o[18] = 0.0; o[19] = 0.0;
    }
    base += __popcll(bal);
  }
  if (lane == 0) p.box_count[s] = (int32_t)(base - a);
}

// ----------------------------------------------------------------------------------------------------------------- label
struct NlParams {
  const double* pos; int64_t n; const int64_t* frame_ptr; int64_t n_samples;
  const double* rec; const int64_t* box_ptr; const int32_t* box_count; int64_t n_boxes;
  const int32_t* nn; int32_t invariance; double offset;
  int32_t* label; double* out; int32_t* hit; int32_t* status;
};

__global__ __launch_bounds__(NS_BLOCK) void k_ns_label(const NlParams p) {
  __shared__ double sb[NS_STAGE * NS_REC];
  const int64_t s = blockIdx.x;
  const int64_t a = p.frame_ptr[s], b = p.frame_ptr[s + 1];
  if (a < 0 || b < a || b > p.n) {                         // (uniform in the work-group)
    if (threadIdx.x == 0) atomicOr(p.status, RGNN_STATUS_NUSC_BAD_CHUNK);
    return;
  }
  int64_t seg = p.box_ptr[s], nb = p.box_count[s];
  if (seg < 0 || nb < 0 || seg > p.n_boxes || nb > p.n_boxes - seg) {
    if (threadIdx.x == 0) atomicOr(p.status, RGNN_STATUS_NUSC_BAD_BOX_PTR);
    nb = 0; seg = 0;
  }
  const double NaN = nan("");
  for (int64_t t = a; t < b; t += NS_BLOCK) {
    const int64_t row = t + threadIdx.x;
    const bool live = row < b;
    const double px = live ? p.pos[2 * row] : 0.0, py = live ? p.pos[2 * row + 1] : 0.0;
    int best = -1;
    double cx = 0, cy = 0, l = 0, w = 0, theta = 0, lab = 0, src = -1;
    for (int64_t k0 = 0; k0 < nb; k0 += NS_STAGE) {
      const int cnt = (int)(nb - k0 < NS_STAGE ? nb - k0 : NS_STAGE);
      __syncthreads();                                     // the previous stage has been read
      for (int i = threadIdx.x; i < cnt * NS_REC; i += NS_BLOCK) sb[i] = p.rec[(seg + k0) * NS_REC + i];
      __syncthreads();
      if (live) {
        for (int k = 0; k < cnt; k++) {
          const double* r = sb + k * NS_REC;
          const double v0 = px - r[R_P1], v1 = py - r[R_P1 + 1], v2 = 0.0 - r[R_P1 + 2];
          const double ni = r[R_NI], nj = r[R_NJ];
          const double iv = ((r[R_I] * v0 + r[R_I + 1] * v1) + r[R_I + 2] * v2) / ni;
          const double jv = ((r[R_J] * v0 + r[R_J + 1] * v1) + r[R_J + 2] * v2) / nj;
          if (0 - p.offset <= iv && iv <= ni + p.offset && 0 - p.offset <= jv && jv <= nj + p.offset) {
            best = (int)(k0 + k);
            cx = r[R_CX]; cy = r[R_CY]; l = r[R_L]; w = r[R_W]; theta = r[R_THETA]; lab = r[R_LABEL]; src = r[R_SRC];
          }
        }
      }
    }
    if (!live) continue;                                   // (the loop bounds above are uniform: every lane meets every barrier)
    p.label[row] = best < 0 ? 0 : (int32_t)lab;
    if (p.hit != nullptr) p.hit[row] = (int32_t)src;
    double* out = p.out + row * 5;
    double o0 = NaN, o1 = NaN, o2 = NaN, o3 = NaN, o4 = NaN;
    if (best >= 0) {
      const double xr = cx - px, yr = cy - py;
      if (p.invariance == 0) {                             // conversion.py:166-169
        o0 = px + xr; o1 = py + yr; o2 = l; o3 = w; o4 = (theta * PI_D) / 180;
      } else if (p.invariance == 1) {                      // :171-173
        o0 = xr; o1 = yr; o2 = l; o3 = w; o4 = (theta * PI_D) / 180;
      } else {                                             // bounding_box.py:205-272, as groundtruth.hip
        const int64_t q = p.nn[row];
        if (q >= 0 && q < p.n) {
          const double vx = p.pos[2 * q] - px, vy = p.pos[2 * q + 1] - py;
          const double vn = sqrt(vx * vx + vy * vy);
          const double th_nn = deg_of(vy / vn, vx / vn);
          const double tt = tan((theta * PI_D) / 180);
          const double dn = sqrt(1.0 + tt * tt);
          double an = round5(deg_of(tt / dn, 1.0 / dn) - th_nn);
          if (an < 0) an = 360 + an;
          if (an >= 180) an = an - 180;
          const double d = sqrt(xr * xr + yr * yr);
          double bn = 0.0;
          if (d != 0) {
            bn = round5(deg_of(yr / d, xr / d) - th_nn);
            if (bn < 0) bn = 360 + bn;
          }
          o0 = d; o1 = (bn * PI_D) / 180; o2 = l; o3 = w; o4 = (an * PI_D) / 180;
        }
      }
    }
    out[0] = o0; out[1] = o1; out[2] = o2; out[3] = o3; out[4] = o4;
  }
}

}  // namespace

extern "C" int32_t rgnn_nusc_box_record_doubles(void) { return NS_REC; }

extern "C" int64_t rgnn_nusc_points_tmp_bytes(int64_t n_samples) { return 8 * (n_samples > 0 ? n_samples : 1); }

extern "C" int rgnn_nusc_points(const double* points, int64_t n_total, const int64_t* chunk_ptr, const int32_t* chunk_sample,
                                const double* chunk_rotation, const double* chunk_translation, int64_t n_chunks, int64_t n_samples,
                                int32_t crop, double xlim, double ylim, int64_t* frame_ptr, int64_t n_cap, double* X, double* V,
                                double* V_cc, double* rcs, double* timestamp, int32_t* src_row, int32_t* status, void* tmp,
                                rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n_total >= 0 && n_total < 2147483647 && n_chunks >= 0 && n_chunks < 2147483647 && n_samples >= 0 &&
                 n_samples < 2147483647 && n_cap >= 0, "bad sizes");
  RGNN_CHECK_ARG(frame_ptr && status && tmp && chunk_ptr, "null pointers");
  RGNN_CHECK_ARG(n_chunks == 0 || (chunk_sample && chunk_rotation && chunk_translation), "null chunk lists");
  RGNN_CHECK_ARG(n_total == 0 || points, "null points");
  RGNN_CHECK_ARG(n_cap == 0 || (X && V && V_cc && rcs && timestamp && src_row), "null outputs");
  const NpParams p{points, n_total, chunk_ptr, chunk_sample, chunk_rotation, chunk_translation, n_chunks, n_samples, crop ? 1 : 0,
                   xlim, ylim, (int64_t*)tmp, frame_ptr, n_cap, X, V, V_cc, rcs, timestamp, src_row, status};
  hipStream_t s = (hipStream_t)stream;
  if (n_samples > 0) {
    hipLaunchKernelGGL(k_ns_points<false>, dim3((unsigned)n_samples), dim3(NS_BLOCK), 0, s, p);
    RGNN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_ns_scan, dim3(1), dim3(RGNN_WAVE), 0, s, p);
  RGNN_CHECK_LAUNCH();
  if (n_samples > 0 && n_cap > 0) {
    hipLaunchKernelGGL(k_ns_points<true>, dim3((unsigned)n_samples), dim3(NS_BLOCK), 0, s, p);
    RGNN_CHECK_LAUNCH();
  }
  return RGNN_OK;
}

extern "C" int rgnn_nusc_boxes(const double* box_center, const double* box_size, const double* box_rotation, const int32_t* box_label,
                               const int32_t* box_points, const int64_t* box_ptr, int64_t n_boxes, int64_t n_samples,
                               const double* ego_translation, const double* ego_rotation, int32_t crop, double xlim, double ylim,
                               double wlh_factor, double* records, int32_t* box_count, int32_t* status, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n_boxes >= 0 && n_boxes < 2147483647 && n_samples >= 0 && n_samples < 2147483647, "bad sizes");
  if (n_samples == 0) return RGNN_OK;
  RGNN_CHECK_ARG(box_ptr && ego_translation && ego_rotation && box_count && status, "null pointers");
  RGNN_CHECK_ARG(n_boxes == 0 || (box_center && box_size && box_rotation && box_label && box_points && records), "null box lists");
  const NbParams p{box_center, box_size, box_rotation, box_label, box_points, box_ptr, n_boxes, n_samples, ego_translation,
                   ego_rotation, crop ? 1 : 0, xlim, ylim, wlh_factor, records, box_count, status};
  hipLaunchKernelGGL(k_ns_boxes, dim3((unsigned)n_samples), dim3(RGNN_WAVE), 0, (hipStream_t)stream, p);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

extern "C" int rgnn_nusc_label_points(const double* pos, int64_t n, const int64_t* frame_ptr, int64_t n_samples, const double* records,
                                      const int64_t* box_ptr, const int32_t* box_count, int64_t n_boxes, const int32_t* nn_index,
                                      int32_t invariance, double wlh_offset, int32_t* label, double* out, int32_t* hit,
                                      int32_t* status, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n >= 0 && n_boxes >= 0 && n_samples >= 0 && n_samples < 2147483647, "bad sizes");
  RGNN_CHECK_ARG(invariance >= 0 && invariance <= 2, "invariance: 0 none, 1 translation, 2 en");
  if (n_samples == 0) return RGNN_OK;
  RGNN_CHECK_ARG(frame_ptr && box_ptr && box_count && status, "null pointers");
  RGNN_CHECK_ARG(n == 0 || (pos && label && out), "null point arrays");
  RGNN_CHECK_ARG(n_boxes == 0 || records, "null records");
  RGNN_CHECK_ARG(invariance != 2 || n == 0 || nn_index, "the en representation needs nearest neighbours");
  const NlParams p{pos, n, frame_ptr, n_samples, records, box_ptr, box_count, n_boxes, nn_index, (int)invariance, wlh_offset,
                   label, out, hit, status};
  hipLaunchKernelGGL(k_ns_label, dim3((unsigned)n_samples), dim3(NS_BLOCK), 0, (hipStream_t)stream, p);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}
