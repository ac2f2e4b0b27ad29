// Rigid motions of frames and collated graphs (gfx950): p' = R(a_f) p + t_f, v' = R(a_f) v per frame f, R = [[c, -s], [s, c]],
// a_f in radians, counter-clockwise.  Three entry points, one launch each, no temporaries (rgnn.h "rigid motions"):
//   rgnn_rigid_points        a FrameBatch's X and V (float64), the frame of a row found in frame_ptr (empty frames are legal)
//   rgnn_rigid_graph_nodes   a collated Batch's node rows: pos, vel, the moving columns of x and the box columns of y (float32)
//   rgnn_rigid_graph_edges   the moving columns of edge_attr (float32)
// The graph kernels write ONLY the columns that move: the caller hands them a copy of x / y / edge_attr, and every other column of
// that copy (the label, lengths, widths, invariant features, the en encoding, aligned boxes) is never touched.
//
// Arithmetic: float64 from the stored operands, separate multiplies and adds (the library is built with -ffp-contract=off), one
// rounding at the store.  sin and cos are the two plain double calls, not sincos: the same two functions a torch.sin / torch.cos of
// a float64 device tensor evaluates, which is what the tests measure their error bar with.
// Exact-zero rule: an angle of exactly 0 skips the rotation and a shift component of exactly 0 skips its addition, so the stored
// bits survive (x + 0.0 would turn -0.0 into +0.0, and a NaN's payload is not a function of the arithmetic).
//
// One thread per row, 16 - 64 bytes in and out per row; cos and sin are evaluated once per frame and block (block_motion), so the
// passes stay bandwidth-bound.  C2 batch (192 000 nodes, 800 000 edges): 8 and 9 us (MEASUREMENTS 8p).
#include "common.h"
#include <math.h>

namespace {

constexpr double PI_D = 3.141592653589793;

struct Codes {
  int32_t n;
  int32_t c[RGNN_MAX_FEATURE_CODES];
};

struct Motion {
  double a, c, s, tx, ty;
  bool rotates;
};

__device__ __forceinline__ void trig_of(double a, double& c, double& s) {
  c = a != 0.0 ? cos(a) : 1.0;
  s = a != 0.0 ? sin(a) : 0.0;
}

// The motion of frame f (-1: this thread has no row, it gets the identity).  EVERY thread of the block calls this, once: the
// rows of a block belong to a handful of frames, so the block evaluates cos and sin once per frame it meets -- thread t for frame
// lo + t, lo the block's lowest frame -- and the rows read them from LDS (broadcasts); a double sin + cos per row would make these
// passes VALU-bound.  A frame more than 256 above lo (rows out of order, runs of empty frames) is evaluated by its own thread: the
// same two calls on the same angle, the same bits.
__device__ __forceinline__ Motion block_motion(const double* __restrict__ angle, const double* __restrict__ shift, int f) {
  __shared__ double tab[2 * 256];
  __shared__ int lo_s, hi_s;
  if (threadIdx.x == 0) { lo_s = 0x7fffffff; hi_s = -1; }
  __syncthreads();
  int lo = f < 0 ? 0x7fffffff : f, hi = f;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    lo = min(lo, __shfl_xor(lo, off));
    hi = max(hi, __shfl_xor(hi, off));
  }
  if ((threadIdx.x & 63) == 0) { atomicMin(&lo_s, lo); atomicMax(&hi_s, hi); }
  __syncthreads();
  lo = lo_s; hi = hi_s;
  if (hi >= 0 && threadIdx.x <= (unsigned)(hi - lo)) trig_of(angle[lo + (int)threadIdx.x], tab[2 * threadIdx.x], tab[2 * threadIdx.x + 1]);
  __syncthreads();
  Motion m{0.0, 1.0, 0.0, 0.0, 0.0, false};
  if (f < 0) return m;
  m.a = angle[f];
  m.rotates = m.a != 0.0;
  if (f - lo < 256) { m.c = tab[2 * (f - lo)]; m.s = tab[2 * (f - lo) + 1]; }
  else trig_of(m.a, m.c, m.s);
  m.tx = shift ? shift[2 * (int64_t)f] : 0.0;
  m.ty = shift ? shift[2 * (int64_t)f + 1] : 0.0;
  return m;
}

__device__ __forceinline__ void rotate(const Motion& m, double x, double y, double& rx, double& ry) {
  rx = m.rotates ? m.c * x - m.s * y : x;
  ry = m.rotates ? m.s * x + m.c * y : y;
}

__device__ __forceinline__ void move(const Motion& m, double x, double y, double& rx, double& ry) {
  rotate(m, x, y, rx, ry);
  if (m.tx != 0.0) rx = rx + m.tx;
  if (m.ty != 0.0) ry = ry + m.ty;
}

// theta + a folded into [0, pi) in double (fmod is exact), rounded once; a result that rounds up to float32(pi) is stored as 0
__device__ __forceinline__ float wrap_theta(double theta, double a) {
  double t = fmod(theta + a, PI_D);
  if (t < 0.0) t = t + PI_D;
  if (t >= PI_D) t = t - PI_D;
  const float r = (float)t;
  return r >= (float)PI_D ? 0.0f : r;
}

// the frame of row i: the last f with frame_ptr[f] <= i (frames of no rows are stepped over)
__device__ __forceinline__ int64_t frame_of(const int64_t* __restrict__ frame_ptr, int64_t n_frames, int64_t i) {
  int64_t lo = 0, hi = n_frames;                       // invariant: frame_ptr[lo] <= i < frame_ptr[hi]
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (frame_ptr[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_rigid_points(const double* __restrict__ X, const double* __restrict__ V,
                                                     const int64_t* __restrict__ frame_ptr, int64_t n, int64_t n_frames,
                                                     const double* __restrict__ angle, const double* __restrict__ shift,
                                                     double* __restrict__ X_out, double* __restrict__ V_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool framed = i < n && i >= frame_ptr[0] && i < frame_ptr[n_frames];     // a row outside every frame is copied
  const Motion m = block_motion(angle, shift, framed ? (int)frame_of(frame_ptr, n_frames, i) : -1);
  if (i >= n) return;
  const double2 x = ((const double2*)X)[i];
  double2 o;
  move(m, x.x, x.y, o.x, o.y);
  ((double2*)X_out)[i] = o;
  if (V) {
    const double2 v = ((const double2*)V)[i];
    rotate(m, v.x, v.y, o.x, o.y);
    ((double2*)V_out)[i] = o;
  }
}

struct NodeParams {
  const float* pos; const float* vel;
  const float* x; int64_t ldx; Codes codes;
  const float* y; int64_t ldy; int box_width, invariance;
  const int64_t* batch; int64_t n, n_graphs;
  const double* angle; const double* shift;
  float* pos_out; float* vel_out; float* x_out; int64_t ldxo; float* y_out; int64_t ldyo;
};

__global__ __launch_bounds__(256) void k_rigid_graph_nodes(const NodeParams p) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t f = i < p.n ? p.batch[i] : -1;
  const bool known = f >= 0 && f < p.n_graphs;           // a row of no graph: pos / vel copied, nothing else written
  const Motion m = block_motion(p.angle, p.shift, known ? (int)f : -1);
  if (i >= p.n) return;
  double rx, ry;
  if (p.pos_out) {
    const float2 q = ((const float2*)p.pos)[i];
    move(m, (double)q.x, (double)q.y, rx, ry);
    ((float2*)p.pos_out)[i] = make_float2((float)rx, (float)ry);
  }
  if (p.vel_out) {
    const float2 q = ((const float2*)p.vel)[i];
    rotate(m, (double)q.x, (double)q.y, rx, ry);
    ((float2*)p.vel_out)[i] = make_float2((float)rx, (float)ry);
  }
  if (!known) return;
  const bool moves = m.rotates || m.tx != 0.0 || m.ty != 0.0;
  if (p.x_out && moves) {
    const float* xi = p.x + i * p.ldx;
    float* xo = p.x_out + i * p.ldxo;
    int w = 0;
    for (int c = 0; c < p.codes.n; c++) {
      switch (p.codes.c[c]) {
        case RGNN_NF_SPATIAL_COORDINATES:
          move(m, (double)xi[w], (double)xi[w + 1], rx, ry);
          xo[w] = (float)rx; xo[w + 1] = (float)ry;
          w += 2;
          break;
        case RGNN_NF_VELOCITY_VECTOR:
          if (m.rotates) {
            rotate(m, (double)xi[w], (double)xi[w + 1], rx, ry);
            xo[w] = (float)rx; xo[w + 1] = (float)ry;
          }
          w += 2;
          break;
        default: w += 1; break;
      }
    }
  }
  // rotated boxes [c0, c1, l, w, theta] behind the label; the en encoding (2) and aligned boxes (4 columns) do not move
  if (p.y_out && moves && p.box_width == 5 && p.invariance != 2) {
    const float* yi = p.y + i * p.ldy + 1;
    float* yo = p.y_out + i * p.ldyo + 1;
    if (!isnan(yi[0])) {                                  // background rows carry NaN boxes: left as they are
      if (p.invariance == 0) move(m, (double)yi[0], (double)yi[1], rx, ry);      // none: the centre is a point
      else rotate(m, (double)yi[0], (double)yi[1], rx, ry);                      // translation: centre - point is a difference
      if (p.invariance == 0 || m.rotates) { yo[0] = (float)rx; yo[1] = (float)ry; }
      if (m.rotates) yo[4] = wrap_theta((double)yi[4], m.a);
    }
  }
}

struct EdgeParams {
  const float* attr; int64_t lda; Codes codes; int undirected;
  const int64_t* edge_index; int64_t n_edges;
  const int64_t* batch; int64_t n, n_graphs;
  const double* angle;
  const float* pos; const float* vel;
  float* out; int64_t ldo;
};

__global__ __launch_bounds__(256) void k_rigid_graph_edges(const EdgeParams p) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = e < p.n_edges ? p.edge_index[e] : -1, j = e < p.n_edges ? p.edge_index[p.n_edges + e] : -1;
  int64_t f = -1;                                          // an edge with an end outside the node rows: its row stays as it is
  if (i >= 0 && i < p.n && j >= 0 && j < p.n) f = p.batch[i];
  const Motion m = block_motion(p.angle, nullptr, f >= 0 && f < p.n_graphs ? (int)f : -1);
  if (!m.rotates) return;                                  // no row, no graph, or angle 0; differences do not see the shift
  const float* ai = p.attr + e * p.lda;
  float* ao = p.out + e * p.ldo;
  int w = 0;
  for (int c = 0; c < p.codes.n; c++) {
    const int code = p.codes.c[c];
    if (code == RGNN_EF_RELATIVE_POSITION || code == RGNN_EF_RELATIVE_VELOCITY) {
      double rx, ry;
      if (!p.undirected) {
        rotate(m, (double)ai[w], (double)ai[w + 1], rx, ry);
      } else {                                             // |q_i - q_j| forgot its signs: again from the batch's own rows
        const float* q = code == RGNN_EF_RELATIVE_POSITION ? p.pos : p.vel;
        const float2 qi = ((const float2*)q)[i], qj = ((const float2*)q)[j];
        rotate(m, (double)qi.x - (double)qj.x, (double)qi.y - (double)qj.y, rx, ry);
        rx = fabs(rx); ry = fabs(ry);
      }
      ao[w] = (float)rx; ao[w + 1] = (float)ry;
      w += 2;
    } else {
      w += code == RGNN_EF_POINT_PAIR ? 4 : 1;
    }
  }
}

bool load_codes(const int32_t* codes, int32_t n_codes, int max_code, Codes& out) {
  if (n_codes < 0 || n_codes > RGNN_MAX_FEATURE_CODES || (n_codes > 0 && codes == nullptr)) return false;
  out.n = n_codes;
  for (int k = 0; k < n_codes; k++) {
    if (codes[k] < 0 || codes[k] > max_code) return false;
    out.c[k] = codes[k];
  }
  return true;
}

int node_width(const Codes& c) {
  int w = 0;
  for (int k = 0; k < c.n; k++) w += (c.c[k] == RGNN_NF_VELOCITY_VECTOR || c.c[k] == RGNN_NF_SPATIAL_COORDINATES) ? 2 : 1;
  return w;
}

int edge_width(const Codes& c) {
  int w = 0;
  for (int k = 0; k < c.n; k++)
    w += c.c[k] == RGNN_EF_POINT_PAIR ? 4 : (c.c[k] == RGNN_EF_RELATIVE_POSITION || c.c[k] == RGNN_EF_RELATIVE_VELOCITY) ? 2 : 1;
  return w;
}

}  // namespace

extern "C" int rgnn_rigid_points(const double* X, const double* V, const int64_t* frame_ptr, int64_t n, int64_t n_frames,
                                 const double* angle, const double* shift, double* X_out, double* V_out, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n >= 0 && n_frames >= 0 && n_frames < 2147483647, "bad sizes");
  if (n == 0) return RGNN_OK;
  RGNN_CHECK_ARG(n_frames >= 1, "rows but no frame");
  RGNN_CHECK_ARG(X && X_out && frame_ptr && angle && shift, "null pointers");
  RGNN_CHECK_ARG((V == nullptr) == (V_out == nullptr), "V and V_out come together");
  RGNN_CHECK_ARG(X != X_out && (V == nullptr || V != V_out), "out of place only");
  hipLaunchKernelGGL(k_rigid_points, dim3(rgnn_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, X, V, frame_ptr, n, n_frames,
                     angle, shift, X_out, V_out);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

extern "C" int rgnn_rigid_graph_nodes(const float* pos, const float* vel, const float* x, int64_t ldx, const int32_t* node_codes,
                                      int32_t n_codes, const float* y, int64_t ldy, int32_t box_width, int32_t invariance,
                                      const int64_t* batch, int64_t n, int64_t n_graphs, const double* angle, const double* shift,
                                      float* pos_out, float* vel_out, float* x_out, int64_t ldxo, float* y_out, int64_t ldyo,
                                      rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n >= 0 && n_graphs >= 0 && n_graphs < 2147483647, "bad sizes");
  RGNN_CHECK_ARG(invariance >= 0 && invariance <= 2, "invariance: 0 none, 1 translation, 2 en");
  NodeParams p{};
  RGNN_CHECK_ARG(load_codes(node_codes, n_codes, RGNN_NF_SPATIAL_COORDINATES, p.codes), "bad node feature codes");
  RGNN_CHECK_ARG((pos == nullptr) == (pos_out == nullptr) && (vel == nullptr) == (vel_out == nullptr) &&
                 (x == nullptr) == (x_out == nullptr) && (y == nullptr) == (y_out == nullptr), "every input comes with its output");
  RGNN_CHECK_ARG(x == nullptr || (ldx >= node_width(p.codes) && ldxo >= node_width(p.codes)), "x is narrower than its feature list");
  RGNN_CHECK_ARG(y == nullptr || ((box_width == 4 || box_width == 5) && ldy >= 1 + box_width && ldyo >= 1 + box_width),
                 "y is [label | 4 or 5 box columns]");
  RGNN_CHECK_ARG((pos == nullptr || pos != pos_out) && (vel == nullptr || vel != vel_out), "pos and vel move out of place");
  if (n == 0) return RGNN_OK;
  RGNN_CHECK_ARG(batch && angle && shift, "null pointers");
  p.pos = pos; p.vel = vel; p.x = x; p.ldx = ldx; p.y = y; p.ldy = ldy; p.box_width = box_width; p.invariance = invariance;
  p.batch = batch; p.n = n; p.n_graphs = n_graphs; p.angle = angle; p.shift = shift;
  p.pos_out = pos_out; p.vel_out = vel_out; p.x_out = x_out; p.ldxo = ldxo; p.y_out = y_out; p.ldyo = ldyo;
  hipLaunchKernelGGL(k_rigid_graph_nodes, dim3(rgnn_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, p);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

extern "C" int rgnn_rigid_graph_edges(const float* edge_attr, int64_t lda, const int32_t* edge_codes, int32_t n_codes,
                                      int32_t undirected, const int64_t* edge_index, int64_t n_edges, const int64_t* batch, int64_t n,
                                      int64_t n_graphs, const double* angle, const float* pos, const float* vel, float* out,
                                      int64_t ldo, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n_edges >= 0 && n >= 0 && n_graphs >= 0 && n_graphs < 2147483647, "bad sizes");
  EdgeParams p{};
  RGNN_CHECK_ARG(load_codes(edge_codes, n_codes, RGNN_EF_RELATIVE_VELOCITY, p.codes), "bad edge feature codes");
  RGNN_CHECK_ARG(lda >= edge_width(p.codes) && ldo >= edge_width(p.codes), "edge_attr is narrower than its feature list");
  if (n_edges == 0) return RGNN_OK;
  RGNN_CHECK_ARG(edge_attr && out && edge_index && batch && angle, "null pointers");
  bool need_pos = false, need_vel = false;
  for (int k = 0; k < p.codes.n; k++) {
    need_pos = need_pos || (undirected && p.codes.c[k] == RGNN_EF_RELATIVE_POSITION);
    need_vel = need_vel || (undirected && p.codes.c[k] == RGNN_EF_RELATIVE_VELOCITY);
  }
  RGNN_CHECK_ARG((!need_pos || pos) && (!need_vel || vel), "undirected relative features are recomputed from pos / vel");
  p.attr = edge_attr; p.lda = lda; p.undirected = undirected ? 1 : 0; p.edge_index = edge_index; p.n_edges = n_edges;
  p.batch = batch; p.n = n; p.n_graphs = n_graphs; p.angle = angle; p.pos = pos; p.vel = vel; p.out = out; p.ldo = ldo;
  hipLaunchKernelGGL(k_rigid_graph_edges, dim3(rgnn_blocks(n_edges, 256)), dim3(256), 0, (hipStream_t)stream, p);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}
