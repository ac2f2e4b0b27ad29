// Subgraphs of a collated batch (radargnn_amd/subgraph.py; PyG: torch_geometric.utils.subgraph / dropout_node / dropout_edge, which
// index with boolean masks and relabel on the host side of torch): an order-preserving compaction of the node rows and the edges
// of a batch with relabelling, by the library's count -> scan -> fill protocol (rgnn.h):
//
//     flags    flags[i] = node i is kept (i < N); flags[N + e] = edge e is kept: its own flag, both ends kept, and the edge sound
//              (ends inside [0, N), both in one graph, the graph inside [0, B), not before its predecessor's graph)
//     scan     rgnn_exclusive_scan_i32 over the N + E flags: scan[i] is the new id of a kept node i (new_id[i] = flags[i] ?
//              scan[i] : -1), scan[N + e] - scan[N] the new place of a kept edge e
//     offsets  ptr'[g] = scan[ptr[g]], _edge_ptr' = scan of the kept edges per graph, and {N', E', status, 0} in one 16-byte word
//              group: the ONE host read of the operation
//     fill     edge_index' = (scan[s], scan[t]), batch', the maps node_ids / edge_ids
//     gather   out[r'] = in[ids[r']] for rows of w 4-byte words, one launch per attribute (collate.hip's precedent)
//
// Pure memory traffic.  No kernel waits on another work-group, every loop is bounded by a shape or by the wave size, the only
// atomics are integer adds / ors whose result does not depend on their order, and the inputs are never written.  Every value read
// from edge_index, batch, ptr or an id map is range-checked before it is used as an index.
#include "common.h"

namespace {

constexpr int SG_THREADS = 256;

__global__ __launch_bounds__(SG_THREADS) void k_subgraph_flags(const int64_t* __restrict__ ei, int64_t n_edges,
                                                              const int64_t* __restrict__ batch, int64_t n, int64_t n_graphs,
                                                              const uint8_t* __restrict__ keep_nodes,
                                                              const uint8_t* __restrict__ keep_edges, int32_t* __restrict__ flags,
                                                              int32_t* __restrict__ graph_edges, int32_t* __restrict__ status) {
  const int64_t idx = (int64_t)blockIdx.x * SG_THREADS + threadIdx.x;
  int64_t g = -1;                                            // graph of a KEPT edge, -1 for every other thread
  if (idx < n) {
    flags[idx] = keep_nodes ? (keep_nodes[idx] != 0 ? 1 : 0) : 1;
  } else if (idx < n + n_edges) {
    const int64_t e = idx - n;
    const int64_t s = ei[e], t = ei[n_edges + e];
    int bits = 0;
    bool keep = false;
    if ((uint64_t)s >= (uint64_t)n || (uint64_t)t >= (uint64_t)n) {
      bits = RGNN_STATUS_SUBGRAPH_BAD_ENDPOINT;
    } else {
      const int64_t gs = batch[s], gt = batch[t];
      if ((uint64_t)gs >= (uint64_t)n_graphs) {
        bits = RGNN_STATUS_SUBGRAPH_BAD_GRAPH;
      } else if (gs != gt) {
        bits = RGNN_STATUS_SUBGRAPH_CROSS_GRAPH;
      } else {
        const int64_t sp = e > 0 ? ei[e - 1] : -1;           // the predecessor's source, if it is one
        if ((uint64_t)sp < (uint64_t)n && batch[sp] > gs) {
          bits = RGNN_STATUS_SUBGRAPH_EDGE_ORDER;
        } else {
          keep = (!keep_edges || keep_edges[e] != 0) && (!keep_nodes || (keep_nodes[s] != 0 && keep_nodes[t] != 0));
          if (keep) g = gs;
        }
      }
    }
    flags[idx] = keep ? 1 : 0;
    if (bits) atomicOr(status, bits);
  }
  // kept edges per graph: the lanes of a wave that hold the same graph add once (an ordered edge list: one or two adds a wave);
  // at most 64 rounds, every round retires a lane.  Whole waves get here: nobody has returned.
  const int lane = threadIdx.x & (RGNN_WAVE - 1);
  bool active = g >= 0;
  for (int round = 0; round < RGNN_WAVE; round++) {
    const unsigned long long todo = __ballot(active);
    if (!todo) break;
    const int leader = __ffsll((long long)todo) - 1;
    const int64_t gl = __shfl(g, leader, RGNN_WAVE);
    const bool mine = active && g == gl;
    const unsigned long long same = __ballot(mine);
    if (lane == leader) atomicAdd(&graph_edges[gl], __popcll(same));
    if (mine) active = false;
  }
}

// block-wide inclusive scan of one value per thread (SG_THREADS threads); *total = the block's sum
__device__ __forceinline__ int sg_block_scan(int v, int* total) {
  __shared__ int wave_sums[SG_THREADS / RGNN_WAVE];
  const int lane = threadIdx.x & (RGNN_WAVE - 1), w = threadIdx.x / RGNN_WAVE;
  int inc = v;
#pragma unroll
  for (int off = 1; off < RGNN_WAVE; off <<= 1) {
    const int t = __shfl_up(inc, off, RGNN_WAVE);
    if (lane >= off) inc += t;
  }
  if (lane == RGNN_WAVE - 1) wave_sums[w] = inc;
  __syncthreads();
  int add = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < SG_THREADS / RGNN_WAVE; i++) {
    const int s = wave_sums[i];
    if (i < w) add += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return inc + add;
}

// ONE block: the offsets of the result and the totals
__global__ __launch_bounds__(SG_THREADS) void k_subgraph_offsets(const int32_t* __restrict__ scan,
                                                                const int32_t* __restrict__ graph_edges,
                                                                const int64_t* __restrict__ ptr, int64_t n, int64_t n_edges,
                                                                int64_t n_graphs, int64_t* __restrict__ ptr_out,
                                                                int64_t* __restrict__ edge_ptr_out, int32_t* __restrict__ totals,
                                                                int32_t* __restrict__ status) {
  int64_t carry = 0;
  for (int64_t start = 0; start <= n_graphs; start += SG_THREADS) {
    const int64_t g = start + threadIdx.x;
    const int v = g < n_graphs ? graph_edges[g] : 0;
    int tot;
    const int inc = sg_block_scan(v, &tot);
    if (g <= n_graphs) {
      edge_ptr_out[g] = carry + inc - v;
      int64_t p = ptr[g];
      if (p < 0 || p > n) {
        atomicOr(status, RGNN_STATUS_SUBGRAPH_BAD_GRAPH);
        p = p < 0 ? 0 : n;
      }
      ptr_out[g] = scan[p];
    }
    carry += tot;
  }
  __syncthreads();                                           // (this block's own atomicOr above: performed at L2 before the read below)
  if (threadIdx.x == 0) {
    totals[0] = scan[n];
    totals[1] = scan[n + n_edges] - scan[n];
    totals[2] = atomicOr(status, 0);
    totals[3] = 0;
  }
}

__global__ __launch_bounds__(SG_THREADS) void k_subgraph_fill(const int64_t* __restrict__ ei, int64_t n_edges,
                                                             const int64_t* __restrict__ batch, int64_t n,
                                                             const int32_t* __restrict__ flags, const int32_t* __restrict__ scan,
                                                             int64_t n_out, int64_t e_out, int64_t* __restrict__ ei_out,
                                                             int64_t* __restrict__ batch_out, int32_t* __restrict__ new_id,
                                                             int64_t* __restrict__ node_ids, int64_t* __restrict__ edge_ids) {
  const int64_t idx = (int64_t)blockIdx.x * SG_THREADS + threadIdx.x;
  if (idx < n) {
    const bool keep = flags[idx] != 0;
    const int64_t p = scan[idx];
    if (new_id) new_id[idx] = keep ? (int32_t)p : -1;
    if (!keep || p >= n_out) return;                         // (p >= n_out: outputs sized for another mask -- nothing is written there)
    if (batch_out) batch_out[p] = batch[idx];
    if (node_ids) node_ids[p] = idx;
  } else if (idx < n + n_edges) {
    if (!flags[idx]) return;
    const int64_t e = idx - n;
    const int64_t p = (int64_t)scan[idx] - scan[n];
    const int64_t s = ei[e], t = ei[n_edges + e];
    if (p < 0 || p >= e_out || (uint64_t)s >= (uint64_t)n || (uint64_t)t >= (uint64_t)n) return;
    if (ei_out) {
      ei_out[p] = scan[s];
      ei_out[e_out + p] = scan[t];
    }
    if (edge_ids) edge_ids[p] = e;
  }
}

// out[r, :] = src[ids[r], :], rows of `width` words; VEC words per lane (4: one 16-byte load and store)
template <int VEC, typename T>
__global__ __launch_bounds__(SG_THREADS) void k_gather_rows(const T* __restrict__ src, int64_t ld_src, int width,
                                                           const int64_t* __restrict__ ids, int64_t n_out, int64_t n_in,
                                                           T* __restrict__ out) {
  const int per_row = width / VEC;
  const int64_t idx = (int64_t)blockIdx.x * SG_THREADS + threadIdx.x;
  if (idx >= n_out * per_row) return;
  const int64_t r = idx / per_row;
  const int c = (int)(idx - r * per_row);
  const int64_t id = ids[r];
  if ((uint64_t)id >= (uint64_t)n_in) return;               // (an id map that is not this source's: the row is left unwritten)
  out[idx] = src[id * (ld_src / VEC) + c];
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(SG_THREADS) void k_edge_pair_mask(const int64_t* __restrict__ ei, int64_t n_edges, int64_t n,
                                                              const int64_t* __restrict__ seed, uint32_t threshold,
                                                              uint8_t* __restrict__ mask) {
  const int64_t e = (int64_t)blockIdx.x * SG_THREADS + threadIdx.x;
  if (e >= n_edges) return;
  const int64_t s = ei[e], t = ei[n_edges + e];
  if ((uint64_t)s >= (uint64_t)n || (uint64_t)t >= (uint64_t)n) {
    mask[e] = 0;
    return;
  }
  const uint64_t lo = (uint64_t)(s < t ? s : t), hi = (uint64_t)(s < t ? t : s);
  const uint64_t draw = mix64(mix64((uint64_t)seed[0]) ^ ((lo << 32) | hi)) >> 40;
  mask[e] = draw >= (uint64_t)threshold ? 1 : 0;
}

__global__ __launch_bounds__(SG_THREADS) void k_store_degree_column(const int32_t* __restrict__ degree, int64_t n,
                                                                   float* __restrict__ x, int64_t ldx, int column) {
  const int64_t i = (int64_t)blockIdx.x * SG_THREADS + threadIdx.x;
  if (i < n) x[i * ldx + column] = (float)degree[i];
}

}  // namespace

static bool sg_sizes_ok(int64_t n, int64_t n_edges) {
  return n >= 0 && n_edges >= 0 && n < (1ll << 31) && n_edges < (1ll << 31) && n + n_edges + 1 < (1ll << 31);
}

extern "C" int rgnn_subgraph_flags(const int64_t* edge_index, int64_t n_edges, const int64_t* batch, int64_t n, int64_t n_graphs,
                                   const uint8_t* keep_nodes, const uint8_t* keep_edges, int32_t* flags, int32_t* graph_edges,
                                   int32_t* status, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(sg_sizes_ok(n, n_edges), "N + E + 1 must stay below 2^31");
  RGNN_CHECK_ARG(n_graphs >= 0 && n_graphs < (1ll << 31), "bad graph count");
  if (n + n_edges == 0) return RGNN_OK;
  RGNN_CHECK_ARG(flags && status, "null pointers");
  RGNN_CHECK_ARG(n_edges == 0 || (edge_index && batch && graph_edges), "edges need edge_index, batch and graph_edges");
  hipLaunchKernelGGL(k_subgraph_flags, dim3(rgnn_blocks(n + n_edges, SG_THREADS)), dim3(SG_THREADS), 0, (hipStream_t)stream,
                     edge_index, n_edges, batch, n, n_graphs, keep_nodes, keep_edges, flags, graph_edges, status);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

extern "C" int rgnn_subgraph_offsets(const int32_t* scan, const int32_t* graph_edges, const int64_t* ptr, int64_t n, int64_t n_edges,
                                     int64_t n_graphs, int64_t* ptr_out, int64_t* edge_ptr_out, int32_t* totals, int32_t* status,
                                     rgnn_stream_t stream) {
  RGNN_CHECK_ARG(sg_sizes_ok(n, n_edges), "N + E + 1 must stay below 2^31");
  RGNN_CHECK_ARG(n_graphs >= 0 && n_graphs < (1ll << 31), "bad graph count");
  RGNN_CHECK_ARG(scan && ptr && ptr_out && edge_ptr_out && totals && status && (n_graphs == 0 || graph_edges), "null pointers");
  hipLaunchKernelGGL(k_subgraph_offsets, dim3(1), dim3(SG_THREADS), 0, (hipStream_t)stream, scan, graph_edges, ptr, n, n_edges,
                     n_graphs, ptr_out, edge_ptr_out, totals, status);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

extern "C" int rgnn_subgraph_fill(const int64_t* edge_index, int64_t n_edges, const int64_t* batch, int64_t n, const int32_t* flags,
                                  const int32_t* scan, int64_t n_out, int64_t e_out, int64_t* edge_index_out, int64_t* batch_out,
                                  int32_t* new_id, int64_t* node_ids, int64_t* edge_ids, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(sg_sizes_ok(n, n_edges), "N + E + 1 must stay below 2^31");
  RGNN_CHECK_ARG(n_out >= 0 && n_out <= n && e_out >= 0 && e_out <= n_edges, "the result cannot be larger than the input");
  if (n + n_edges == 0) return RGNN_OK;
  RGNN_CHECK_ARG(flags && scan, "null pointers");
  RGNN_CHECK_ARG(n_edges == 0 || edge_index, "edges need edge_index");
  RGNN_CHECK_ARG(!batch_out || batch, "batch_out needs batch");
  hipLaunchKernelGGL(k_subgraph_fill, dim3(rgnn_blocks(n + n_edges, SG_THREADS)), dim3(SG_THREADS), 0, (hipStream_t)stream,
                     edge_index, n_edges, batch, n, flags, scan, n_out, e_out, edge_index_out, batch_out, new_id, node_ids,
                     edge_ids);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

extern "C" int rgnn_subgraph_gather_rows(const void* src, int64_t ld_src, int32_t width, const int64_t* ids, int64_t n_out,
                                         int64_t n_in, void* out, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n_out >= 0 && n_in >= 0 && width >= 1 && ld_src >= width, "bad sizes");
  RGNN_CHECK_ARG(n_out < (1ll << 31) && n_in < (1ll << 31), "more than 2^31 rows");
  if (n_out == 0) return RGNN_OK;
  RGNN_CHECK_ARG(src && ids && out, "null pointers");
  RGNN_CHECK_ARG((((uintptr_t)src | (uintptr_t)out) & 3) == 0, "rows must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const bool wide = width % 4 == 0 && ld_src % 4 == 0 && (((uintptr_t)src | (uintptr_t)out) & 15) == 0;
  if (wide)
    hipLaunchKernelGGL((k_gather_rows<4, uint4>), dim3(rgnn_blocks(n_out * (width / 4), SG_THREADS)), dim3(SG_THREADS), 0, s,
                       (const uint4*)src, ld_src, (int)width, ids, n_out, n_in, (uint4*)out);
  else
    hipLaunchKernelGGL((k_gather_rows<1, uint32_t>), dim3(rgnn_blocks(n_out * width, SG_THREADS)), dim3(SG_THREADS), 0, s,
                       (const uint32_t*)src, ld_src, (int)width, ids, n_out, n_in, (uint32_t*)out);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

extern "C" int rgnn_edge_pair_mask(const int64_t* edge_index, int64_t n_edges, int64_t n, const int64_t* seed, int32_t threshold,
                                   uint8_t* mask_out, rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n_edges >= 0 && n >= 0 && n <= (1ll << 32), "bad sizes (node ids are packed into 32 bits)");
  RGNN_CHECK_ARG(threshold >= 0 && threshold <= (1 << 24), "threshold must lie in [0, 2^24]");
  if (n_edges == 0) return RGNN_OK;
  RGNN_CHECK_ARG(edge_index && seed && mask_out, "null pointers");
  hipLaunchKernelGGL(k_edge_pair_mask, dim3(rgnn_blocks(n_edges, SG_THREADS)), dim3(SG_THREADS), 0, (hipStream_t)stream,
                     edge_index, n_edges, n, seed, (uint32_t)threshold, mask_out);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}

extern "C" int rgnn_store_degree_column(const int32_t* degree, int64_t n, float* x, int64_t ldx, int32_t column,
                                        rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n >= 0 && column >= 0 && ldx > column, "bad sizes");
  if (n == 0) return RGNN_OK;
  RGNN_CHECK_ARG(degree && x, "null pointers");
  hipLaunchKernelGGL(k_store_degree_column, dim3(rgnn_blocks(n, SG_THREADS)), dim3(SG_THREADS), 0, (hipStream_t)stream, degree, n,
                     x, ldx, (int)column);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}
