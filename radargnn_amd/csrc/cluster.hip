// Clustering on the device: batched DBSCAN labels over the rows of the radius search, and per-cluster class scores.
//
// k_dbscan_frames -- ONE work-group (1024 threads) per frame; the frame's union-find parent array lives in LDS.
//   LDS budget: 4 bytes per point of the frame (the parent word, which also carries "not core" and, at the end, the cluster number) =
//   DB_LDS_NODES * 4 = 96 KB dynamic (opt-in above 64 KB through hipFuncSetAttribute, the form k_csr_frames of graph.hip uses), plus
//   68 bytes static for the scan over the 16 waves: 96.1 of the CU's 160 KB, one work-group per CU.  Nothing else is staged: the rows
//   (rowptr / col / group) are read from HBM where they lie, three passes at most (count, union, border rows only).
//   No work-group reads anything another work-group wrote in this launch: a frame is finished by the block that began it, and a frame
//   of more than DB_LDS_NODES points is refused (RGNN_STATUS_DBSCAN_FRAME_TOO_LARGE), never spilled to a global parent array -- the
//   L2s of the eight XCDs are not coherent, and a find loop that retries on a stale global parent could spin for ever.
//
//   Steps of a block (a barrier between each; every barrier is outside all divergent control flow, and every early return is taken by
//   the whole block because its condition reads block-uniform values only):
//     1 core      thread per point: walk its row, count the neighbours that exist (in the frame, not itself, same group >= 0);
//                 parent[i] = i for a core point, -1 otherwise.
//     2 union     thread per core point: for every core neighbour, hook the LARGER root under the SMALLER with an LDS compare-and-swap.
//                 parent[x] <= x always, so the trees have no cycles and every tree's root is its minimum; a component's surviving root
//                 is therefore its smallest row whatever order the threads arrive in.
//     3 flatten   thread per core point: parent[i] = root(i).
//     4 number    exclusive scan of "is a root" in row order: every wave takes a contiguous slice of the frame, ballots 64 rows at a
//                 time, the 16 slice totals are scanned through LDS; the root's word becomes -2 - number.
//     5 labels    core: the number at its root; otherwise the minimum number over its core neighbours (the final core labels, nothing
//                 else), -1 without one.
//   Loop bounds (n_f = points of the frame, at most DB_LDS_NODES):
//     find        follows parent[x] < x: at most n_f - 1 steps (bounded by the tree height).
//     union retry a failed compare-and-swap means another thread hooked that root meanwhile; at most n_f - 1 hooks ever succeed in a
//                 frame, so at most n_f retries.  Both loops also carry n_f as an explicit trip limit.
//     rows        rowptr[i + 1] - rowptr[i] entries, checked against [0, n_edges] before the walk.
//   The result is a function of the input alone; the kernel does no floating-point work.
//
// k_cluster_scores -- one wave64 per cluster over the CSR of rgnn_group_objects: mean class probabilities in float64.  Lane l adds the
//   members l, l + 64, ... in that order, a 6-stage xor butterfly adds the lanes (a + b is commutative bit for bit, so every lane ends
//   with the same sum): a fixed order, no atomics.
#include "common.h"
#include <math.h>

namespace {

constexpr int DB_THREADS = 1024;
constexpr int DB_WAVES = DB_THREADS / RGNN_WAVE;
constexpr int DB_LDS_NODES = 24 * 1024;              // 96 KB of parent words

__device__ __forceinline__ int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// Root of x (x is core: parent[x] >= 0) with path halving.  Only non-roots are rewritten, and only with one of their ancestors, so a
// racing hook (which writes roots only) and racing halvings leave every word pointing at an ancestor.  At most `limit` steps.
__device__ __forceinline__ int db_find(int* parent, int x, int limit) {
  for (int step = 0; step < limit; ++step) {
    const int p = lds_load(parent + x);
    if (p == x) break;
    const int gp = lds_load(parent + p);
    if (gp != p) lds_store(parent + x, gp);
    x = gp;
  }
  return x;
}

__device__ __forceinline__ int db_root(const int* parent, int x, int limit) {      // read-only find
  for (int step = 0; step < limit; ++step) {
    const int p = lds_load(parent + x);
    if (p == x) break;
    x = p;
  }
  return x;
}

struct DbRow { int begin, len; };

// The entries of row `row` (global id), or an empty row (and *bad) if its offsets do not lie inside col.
__device__ __forceinline__ DbRow db_row(const int32_t* __restrict__ rowptr, int64_t row, int64_t n_edges, bool* bad) {
  const int64_t a = rowptr[row], b = rowptr[row + 1];
  if (a < 0 || b < a || b > n_edges) {
    *bad = true;
    return {0, 0};
  }
  return {(int)a, (int)(b - a)};
}

// Local index of neighbour entry j of point i (local), or -1 if that entry is no neighbour: outside the frame (sets *bad), the point
// itself, or of another group.
__device__ __forceinline__ int db_neighbour(int32_t j, int64_t base, int nf, int i, const int32_t* __restrict__ group, int32_t gi, bool* bad) {
  const int64_t lj = (int64_t)j - base;
  if (lj < 0 || lj >= nf) {
    *bad = true;
    return -1;
  }
  if ((int)lj == i) return -1;
  if (group != nullptr && group[base + lj] != gi) return -1;
  return (int)lj;
}

__global__ __launch_bounds__(DB_THREADS) void k_dbscan_frames(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                            int64_t n, int64_t n_edges, const int64_t* __restrict__ frame_ptr,
                                                            int32_t min_samples, const int32_t* __restrict__ group,
                                                            int32_t* __restrict__ labels, uint8_t* __restrict__ core,
                                                            int32_t* __restrict__ n_clusters, int32_t* __restrict__ status) {
  extern __shared__ int parent[];                 // [n_f]
  __shared__ int wave_total[DB_WAVES + 1];
  const int tid = threadIdx.x, lane = tid & (RGNN_WAVE - 1), wave = tid / RGNN_WAVE;
  const int f = blockIdx.x;
  const int64_t base = frame_ptr[f], end = frame_ptr[f + 1];
  // (block-uniform from here to the first barrier: every thread of the block takes the same branch)
  if (base < 0 || end < base || end > n) {        // a frame outside the points: nothing of it is read or written
    if (tid == 0) {
      atomicOr(status, RGNN_STATUS_DBSCAN_BAD_ROW);
      n_clusters[f] = 0;
    }
    return;
  }
  if (end - base > DB_LDS_NODES) {
    for (int64_t i = base + tid; i < end; i += DB_THREADS) {
      labels[i] = -1;
      core[i] = 0;
    }
    if (tid == 0) {
      atomicOr(status, RGNN_STATUS_DBSCAN_FRAME_TOO_LARGE);
      n_clusters[f] = 0;
    }
    return;
  }
  const int nf = (int)(end - base);
  bool bad = false;

  // 1 core points
  for (int i = tid; i < nf; i += DB_THREADS) {
    const int32_t gi = group != nullptr ? group[base + i] : 0;
    int count = 0;
    if (gi >= 0) {
      const DbRow row = db_row(rowptr, base + i, n_edges, &bad);
      for (int e = 0; e < row.len; ++e) count += db_neighbour(col[row.begin + e], base, nf, i, group, gi, &bad) >= 0;
    }
    parent[i] = (gi >= 0 && (int64_t)count + 1 >= (int64_t)min_samples) ? i : -1;
  }
  __syncthreads();

  // 2 union over core-core edges
  for (int i = tid; i < nf; i += DB_THREADS) {
    if (lds_load(parent + i) < 0) continue;                       // (core-ness never changes after step 1)
    const int32_t gi = group != nullptr ? group[base + i] : 0;
    const DbRow row = db_row(rowptr, base + i, n_edges, &bad);
    for (int e = 0; e < row.len; ++e) {
      const int j = db_neighbour(col[row.begin + e], base, nf, i, group, gi, &bad);
      if (j < 0 || lds_load(parent + j) < 0) continue;
      int a = i, b = j;
      for (int attempt = 0; attempt <= nf; ++attempt) {           // (see "union retry" above)
        a = db_find(parent, a, nf);
        b = db_find(parent, b, nf);
        if (a == b) break;
        if (a < b) {
          const int t = a;
          a = b;
          b = t;
        }
        if (atomicCAS(parent + a, a, b) == a) break;              // the larger root goes under the smaller
      }
    }
  }
  __syncthreads();

  // 3 flatten (a word is only ever replaced by an ancestor of its point, so concurrent readers still reach the root)
  for (int i = tid; i < nf; i += DB_THREADS) {
    if (lds_load(parent + i) < 0) continue;
    lds_store(parent + i, db_root(parent, i, nf));
  }
  __syncthreads();

  // 4 number the roots in row order: wave w owns the rows [w * slice, (w + 1) * slice), slice a multiple of 64
  const int slice = (nf + DB_THREADS - 1) / DB_THREADS * RGNN_WAVE;
  const int s0 = wave * slice < nf ? wave * slice : nf, s1 = s0 + slice < nf ? s0 + slice : nf;
  int roots = 0;
  for (int t0 = s0; t0 < s1; t0 += RGNN_WAVE) {                   // (wave-uniform trip count: the ballots are taken by whole waves)
    const int i = t0 + lane;
    roots += __popcll(__ballot(i < s1 && parent[i] == i));
  }
  if (lane == 0) wave_total[wave] = roots;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int w = 0; w < DB_WAVES; ++w) {
      const int c = wave_total[w];
      wave_total[w] = run;
      run += c;
    }
    wave_total[DB_WAVES] = run;
    n_clusters[f] = run;
  }
  __syncthreads();
  int number = wave_total[wave];
  for (int t0 = s0; t0 < s1; t0 += RGNN_WAVE) {
    const int i = t0 + lane;
    const bool is_root = i < s1 && parent[i] == i;
    const unsigned long long m = __ballot(is_root);
    if (is_root) parent[i] = -2 - (number + __popcll(m & ((1ull << lane) - 1)));     // (only rows of this wave's slice are touched)
    number += __popcll(m);
  }
  __syncthreads();

  // 5 labels: parent[i] is now -1 (not core), -2 - number (a root) or the root's row
  for (int i = tid; i < nf; i += DB_THREADS) {
    const int p = parent[i];
    int label = -1;
    if (p <= -2) {
      label = -2 - p;
    } else if (p >= 0) {
      label = -2 - parent[p];
    } else {
      const int32_t gi = group != nullptr ? group[base + i] : 0;
      if (gi >= 0) {
        const DbRow row = db_row(rowptr, base + i, n_edges, &bad);
        for (int e = 0; e < row.len; ++e) {
          const int j = db_neighbour(col[row.begin + e], base, nf, i, group, gi, &bad);
          if (j < 0) continue;
          int q = parent[j];
          if (q == -1) continue;
          if (q >= 0) q = parent[q];
          const int lj = -2 - q;
          if (label < 0 || lj < label) label = lj;
        }
      }
    }
    labels[base + i] = label;
    core[base + i] = p != -1 ? 1 : 0;
  }
  if (bad) atomicOr(status, RGNN_STATUS_DBSCAN_BAD_ROW);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__global__ __launch_bounds__(RGNN_WAVE) void k_cluster_scores(const float* __restrict__ prob, int64_t ldp, int32_t n_classes, int64_t n,
                                                            const int64_t* __restrict__ obj_ptr, const int32_t* __restrict__ obj_rows,
                                                            int64_t n_rows, const int32_t* __restrict__ group, int32_t bg_index,
                                                            int32_t per_class, double* __restrict__ mean, int32_t* __restrict__ cls,
                                                            double* __restrict__ score) {
  const int lane = threadIdx.x;
  const int64_t o = blockIdx.x;
  int64_t begin = obj_ptr[o], m = obj_ptr[o + 1] - begin;
  if (begin < 0 || m < 0 || begin + m > n_rows) m = 0;            // offsets outside the row list: an empty cluster (NaN means)
  const int32_t* rows = obj_rows + begin;
  int32_t first = -1;                                             // the cluster's first valid member row
  int64_t valid = 0;
  for (int64_t t = lane; t < m; t += RGNN_WAVE) {
    const int32_t r = rows[t];
    valid += r >= 0 && r < n;
  }
  for (int64_t t = 0; t < m && first < 0; ++t) {                  // (wave-uniform: every lane reads the same entries)
    const int32_t r = rows[t];
    if (r >= 0 && r < n) first = r;
  }
  const double count = wave_sum((double)valid);                   // (integers below 2^53: exact in any order)
  int32_t best = -1;
  double best_mean = 0.0;
  const int32_t own = per_class && group != nullptr && first >= 0 ? group[first] : -1;
  for (int32_t k = 0; k < n_classes; ++k) {
    double s = 0.0;
    for (int64_t t = lane; t < m; t += RGNN_WAVE) {
      const int32_t r = rows[t];
      if (r >= 0 && r < n) s += (double)prob[(int64_t)r * ldp + k];
    }
    const double mu = wave_sum(s) / count;
    if (lane == 0) mean[o * n_classes + k] = mu;
    if (per_class) {
      if (k == own) {
        best = k;
        best_mean = mu;
      }
    } else if (k != bg_index && (best < 0 || mu > best_mean)) {   // strict: the lowest k wins a tie
      best = k;
      best_mean = mu;
    }
  }
  if (lane == 0) {
    cls[o] = per_class ? own : best;
    score[o] = best >= 0 ? best_mean : nan("");
  }
}

}  // namespace

extern "C" int32_t rgnn_dbscan_max_frame_points(void) { return DB_LDS_NODES; }

extern "C" int rgnn_dbscan_labels(const int32_t* rowptr, const int32_t* col, int64_t n, int64_t n_edges, const int64_t* frame_ptr,
                                  int64_t n_frames, int32_t min_samples, const int32_t* group, int32_t* labels, uint8_t* core,
                                  int32_t* n_clusters, int32_t* status, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n >= 0 && n < 2147483647 && n_edges >= 0 && n_edges < ((int64_t)1 << 31) && n_frames >= 0 && n_frames < 2147483647,
                 "bad sizes");
  RGNN_CHECK_ARG(min_samples >= 1, "min_samples must be at least 1");
  if (n_frames == 0) return RGNN_OK;
  RGNN_CHECK_ARG(rowptr && frame_ptr && n_clusters && status && (n == 0 || (labels && core)) && (n_edges == 0 || col), "null pointers");
  static RgnnOncePerDevice attr_once;                       // (per kernel and device: common.h)
  if (attr_once.first()) hipFuncSetAttribute((const void*)k_dbscan_frames, hipFuncAttributeMaxDynamicSharedMemorySize, DB_LDS_NODES * 4);
  hipLaunchKernelGGL(k_dbscan_frames, dim3((unsigned)n_frames), dim3(DB_THREADS), (size_t)DB_LDS_NODES * 4, (hipStream_t)stream, rowptr,
                     col, n, n_edges, frame_ptr, min_samples, group, labels, core, n_clusters, status);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

extern "C" int rgnn_cluster_scores(const float* prob, int64_t ldp, int32_t n_classes, int64_t n, const int64_t* obj_ptr,
                                   const int32_t* obj_rows, int64_t n_rows, int64_t n_obj, const int32_t* group, int32_t bg_index,
                                   int32_t per_class, double* mean, int32_t* cls, double* score, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n >= 0 && n < 2147483647 && n_rows >= 0 && n_obj >= 0 && n_obj < 2147483647, "bad sizes");
  RGNN_CHECK_ARG(n_classes >= 1 && ldp >= n_classes, "prob must be [n, n_classes] with a row stride of at least n_classes");
  if (n_obj == 0) return RGNN_OK;
  RGNN_CHECK_ARG(prob && obj_ptr && obj_rows && mean && cls && score, "null pointers");
  RGNN_CHECK_ARG(!per_class || group, "per_class needs the points' groups");
  hipLaunchKernelGGL(k_cluster_scores, dim3((unsigned)n_obj), dim3(RGNN_WAVE), 0, (hipStream_t)stream, prob, ldp, n_classes, n, obj_ptr,
                     obj_rows, n_rows, group, bg_index, per_class ? 1 : 0, mean, cls, score);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}
