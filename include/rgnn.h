/*
 * rgnn.h -- C-ABI of librgnn.so: the MI355X (gfx950) hot path of RadarGNN.
 *
 * Scope: per-frame graph construction (k-NN / radius), undirected degree,
 * edge / node feature extraction and the DetNetBasic forward pass (MPNNConv / RadarPointGNNConv
 * message passing, train-mode BatchNorm, dense MLPs).  Every entry point below names the piece of
 * the reference (paths relative to /root/reference/src/gnnradarobjectdetection/) or of its
 * third-party native dependency that it replaces.
 *
 * Conventions
 *  - plain C, no C++ types, no exceptions cross the boundary;
 *  - every pointer marked [dev] is a device (HBM) pointer owned by the caller; the library never
 *    allocates, frees or retains memory (the caller -- PyTorch in this repo -- owns all buffers);
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no entry point
 *    synchronises the device or the stream;
 *  - return value 0 = ok, negative = error (see rgnn_last_error(), thread-local);
 *  - data-dependent output sizes use the count -> scan -> fill protocol so the caller allocates
 *    exactly (radius graph);
 *  - index dtype: int32 for CSR structures (E < 2^31), int64 only where the reference hands
 *    int64 over (`edge_index`, preprocessor/radarscenes/dataset_creation.py:805);
 *  - device-side failures (k >= frame size, |dot| > 1 + 1e-3, hash overflow) are reported through
 *    a caller-provided [dev] int32 status word that the caller reads when it next synchronises.
 */
#ifndef RGNN_H
#define RGNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* rgnn_stream_t; /* hipStream_t */

/* ---------------------------------------------------------------- error codes / status bits */
#define RGNN_OK 0
#define RGNN_ERR_INVALID_ARGUMENT (-1)
#define RGNN_ERR_LAUNCH (-2)
#define RGNN_ERR_UNSUPPORTED (-3)

#define RGNN_STATUS_KNN_TOO_FEW_POINTS 1 /* a frame has n_f <= k: sklearn raises ValueError              */
#define RGNN_STATUS_DOT_PRODUCT 2        /* graph_constructor/features.py:56,77,91 "Error in dot product" */
#define RGNN_STATUS_TIME_INDEX_OVERFLOW 4 /* more distinct timestamps in a frame than the LDS table holds  */
#define RGNN_STATUS_EDGE_COUNT_CHANGED 8 /* rgnn_radius_graph_fill / rgnn_radius_graph_rows with status, rgnn_radius_graph_rows_direct,
                                          * rgnn_radius_rows_commit: rowptr[n] != the n_edges the caller sized for (rows_direct also:
                                          * a row whose length is no longer the committed one) */
#define RGNN_STATUS_NOT_SYMMETRIC 16     /* rgnn_csr_by_target_symmetric: an edge (s,t) without its twin (t,s)               */
#define RGNN_STATUS_SPLITK_TIMEOUT 32    /* a dense launch gave up waiting for a partial tile of another work-group (see splitk_ws) */
#define RGNN_STATUS_GT_OBJECT_TOO_LARGE 64   /* rgnn_create_gt_boxes: an object of more than rgnn_gt_object_cap() points; its rows are not written */
#define RGNN_STATUS_GT_DEGENERATE_OBJECT 128 /* rgnn_create_gt_boxes: two coincident points, or >= 3 points whose hull has no area (the reference
                                              * divides by zero / raises QhullError); its rows are not written */
#define RGNN_STATUS_PREPROCESS_BAD_ROW 256   /* rgnn_accumulate_frames: a sensor_id / label_id outside its table (the row is dropped), or a
                                              * window whose row range does not lie inside the table (the frame is empty) */
#define RGNN_STATUS_NUSC_BAD_CHUNK 512       /* rgnn_nusc_points: chunk_sample not non-decreasing inside [0, n_samples), or chunk_ptr not
                                              * rising inside [0, n_total] (such a chunk is left out); rgnn_nusc_label_points: a frame_ptr
                                              * range outside the points (the sample is left unwritten) */
#define RGNN_STATUS_NUSC_BAD_BOX_PTR 1024    /* rgnn_nusc_boxes / rgnn_nusc_label_points: a sample's box offsets do not lie inside the box
                                              * list (the sample is treated as one without boxes) */

#define RGNN_STATUS_DBSCAN_FRAME_TOO_LARGE 2048 /* rgnn_dbscan_labels: a frame of more than rgnn_dbscan_max_frame_points() points; its rows get
                                              * label -1 and core 0, its n_clusters 0 */
#define RGNN_STATUS_DBSCAN_BAD_ROW 4096      /* rgnn_dbscan_labels: an entry of col outside its row's frame (skipped), a row whose offsets do
                                              * not lie inside [0, n_edges] (taken as empty) or a frame outside the points (left unwritten) */

#define RGNN_SPLITK_TIMEOUT_WORD 1000    /* index of the time-out counter in the flag area of rgnn_linear_args.splitk_ws */

const char* rgnn_version(void);
const char* rgnn_last_error(void);

/* The library reads its environment switches (RGNN_LINEAR_FP32, RGNN_DMA_TN, ...: experiment and A/B knobs, none needed in normal
 * use) once per call site and caches them.  A process that changes one of them after its first launch calls this to have every
 * site read its variable again on its next use (tools/x3_bench, bench.py's fp32-MFMA line).  Thread-safe; no reference counterpart
 * (the reference has no such switches). */
void rgnn_env_reload(void);

/* Profiling hook: arms two hipEvent_t (passed as void*) that the NEXT call of rgnn_linear_fwd / rgnn_mpnn_aggregate on
 * this thread records immediately before / after its kernel launch on the launch stream (bench.py uses it to time the
 * dominant kernels without Python between the event and the launch).  NULL disarms. */
void rgnn_profile_next_launch(void* ev_start, void* ev_stop);

/* Side streams of the host layer (radargnn_amd/ops.py independent_stream; the reference runs everything on one stream,
 * postprocessor/inference.py:48-68): a plain non-blocking HIP stream on the CURRENT device / its destruction (NULL: no-op).  The host
 * layer creates candidates here, keeps the one it has seen running beside every stream already in use (ROCm maps streams onto four
 * hardware queues; two streams on one queue serialise) and destroys the others -- torch's own pool of 32 streams cannot be given back. */
int rgnn_stream_create(rgnn_stream_t* out);
int rgnn_stream_destroy(rgnn_stream_t stream);

/* ================================================================ generic device primitives */

/* out[i] = sum_{j<i} in[j], i in [0, n]; out has n+1 entries (out[n] = total).  tmp: [dev] scratch of
 * rgnn_scan_tmp_bytes(n) bytes.  Used for cell offsets, radius rowptr, CSR-by-target rowptr. */
int64_t rgnn_scan_tmp_bytes(int64_t n);
int rgnn_exclusive_scan_i32(const int32_t* in, int32_t* out, int64_t n, void* tmp, rgnn_stream_t stream);

/* ================================================================ graph construction
 * Replaces graph_constructor/graph.py:52-82 (sklearn kneighbors_graph / radius_neighbors_graph on a
 * KDTree64 + scipy toarray()/nonzero()).  A batch is B frames laid back to back: X is [n, dim] row-major
 * float64 (dim 2 = "X", dim 4 = "XV": radarscenes/dataset_creation.py:203-206), frame_ptr [B+1] int64.
 * Neighbours are only searched inside a point's own frame; indices written are GLOBAL row numbers (PyG
 * batch numbering, utils/data_handling.py:30).
 *
 * Distances are float64, sum_j (a_j-b_j)^2 accumulated in dimension order with separate multiply and
 * add (no FMA), radius test inclusive d2 <= r*r -- bit-identical decisions to the KD-tree.            */

/* Host-side descriptor of one batch and its grid-hash workspace; filled by the caller, never retained. */
typedef struct rgnn_grid {
  const double* X;          /* [dev] [n, dim] float64 */
  int32_t dim;              /* 2 ("X"), 4 ("XV") or 8 (wider distance bases, zero-padded to 8 columns by the caller: the reference
                             * measures over ALL columns it is given, graph.py:45-50,57-58; cells are binned on the first two) */
  int64_t n;
  const int64_t* frame_ptr; /* [dev] [n_frames + 1] */
  int64_t n_frames;
  void* ws;                 /* [dev] opaque, rgnn_grid_workspace_bytes(n, n_frames, dim) bytes */
  int64_t ws_bytes;
} rgnn_grid;

int64_t rgnn_grid_workspace_bytes(int64_t n, int64_t n_frames, int32_t dim);

/* Bin the points of every frame into a uniform grid on the first two coordinates.
 *   cell_size > 0 : radius mode, cells no smaller than cell_size (3x3 neighbourhood covers radius r = cell_size)
 *   cell_size <= 0: kNN mode, cell edge chosen per frame for ~pts_per_cell points per cell
 * max_frame_points > 0: a hint -- no frame of the batch holds more points than this (the caller's host copy of the frame sizes).
 * Frames of moderate size are then binned by ONE launch -- one block per frame: bounding box, grid, cell histogram, local scan,
 * cell order -- instead of five; 0 = no promise (the general path).  Same cells either way. */
int rgnn_grid_build(const rgnn_grid* g, double cell_size, double pts_per_cell, int64_t max_frame_points, rgnn_stream_t stream);
/* Where the cell order (int32 [n]: point rows in grid-cell order) and its inverse (int32 [n]: position of point i in that
 * order) lie inside the workspace, as byte offsets: valid after rgnn_grid_build, for as long as the workspace is. */
int rgnn_grid_order_offsets(int64_t n, int64_t n_frames, int32_t dim, int64_t* order_offset /*host*/, int64_t* rank_offset /*host*/);

/* Replayed (captured) steps: search + fill of a radius graph whose rows are already known -- `rowptr_committed` [n + 1] as
 * rgnn_radius_rows_commit keeps it (rowptr_committed[n] must equal n_edges).  ONE launch behind the grid build: a point's row is
 * searched once and, if it has the committed length, written in ascending order to col / edge_index (/ relative_position) at the
 * committed place; a row of another length keeps its previous contents and raises RGNN_STATUS_EDGE_COUNT_CHANGED in `status`
 * (the points changed under the captured graph).  If rowptr_committed[n] != n_edges -- what col / edge_index / relative_position /
 * tmp were sized for -- the launch writes nothing at all and raises the same bit, like the guarded rgnn_radius_graph_rows.
 * Replaces, for those steps, rgnn_radius_graph_count + the scan +
 * rgnn_radius_rows_commit + rgnn_radius_graph_rows; same rows, same order, same values.  tmp: int32 [n_edges] scratch (rows of more
 * than 128 neighbours).  Reference: graph.py:68-82 (radius_neighbors_graph + nonzero), graph.py:199-200 (relative_position). */
int rgnn_radius_graph_rows_direct(const rgnn_grid* g, double r, const int32_t* rowptr_committed, int32_t* col, int64_t* edge_index,
                                  int64_t n_edges, int32_t* tmp, int32_t* status, float* relative_position, int32_t undirected,
                                  rgnn_stream_t stream);

/* Radius graph, pass 1: deg[i] = |{j != i in frame(i) : d2(i,j) <= r*r}|  (int32 [n]).  Also leaves the first 32
 * neighbours of every point in the grid workspace for pass 2. */
int rgnn_radius_graph_count(const rgnn_grid* g, double r, int32_t* deg /*[dev]*/, rgnn_stream_t stream);
/* Radius graph, pass 2: rowptr = exclusive scan of deg ([n+1]); col[rowptr[i]..rowptr[i+1]) = neighbours of
 * i, ascending.  Optionally also writes edge_index int64 [2,E] (row 0 = i "query", row 1 = j "neighbour",
 * graph.py:61-63 + dataset_creation.py:805); pass NULL to skip.  E = rowptr[n] is passed by the caller.
 * Must follow rgnn_radius_graph_count on the same grid (same workspace, same r): rows of up to 32 neighbours are copied
 * from what that pass found, denser rows are searched again.
 * status != NULL: the guarded form, for a caller that sized col / edge_index for an edge count it did NOT just read back (a
 * captured HIP graph replayed on a resident batch): if rowptr[n] differs from n_edges the kernels write nothing -- the buffers
 * keep their previous contents -- and status gets RGNN_STATUS_EDGE_COUNT_CHANGED.  NULL: unguarded. */
int rgnn_radius_graph_fill(const rgnn_grid* g, double r, const int32_t* rowptr /*[dev]*/, int32_t* col /*[dev]*/,
                           int64_t* edge_index /*[dev] or NULL*/, int64_t n_edges, int32_t* tmp /*[dev] int32 [2*E]*/,
                           int32_t* status /*[dev] or NULL*/, rgnn_stream_t stream);
/* Fill pass in ONE launch: finished rows (col ascending, edge_index) and, when relative_position != NULL, the edge attributes
 * [x_i - x_j, y_i - y_j] (graph.py:199-200; |.| of both when undirected != 0) as float [n_edges, 2] in edge order -- what
 * rgnn_radius_graph_fill + rgnn_edge_features(relative_position) produce in three launches.  status != NULL:
 * the guarded form (rowptr[n] must equal n_edges, else nothing is written and RGNN_STATUS_EDGE_COUNT_CHANGED is set).
 * tmp: [dev] int32 [n_edges] scratch. */
int rgnn_radius_graph_rows(const rgnn_grid* g, double r, const int32_t* rowptr /*[dev]*/, int32_t* col /*[dev]*/,
                           int64_t* edge_index /*[dev] or NULL*/, int64_t n_edges, int32_t* tmp /*[dev]*/,
                           int32_t* status /*[dev] or NULL*/, float* relative_position /*[dev] or NULL*/, int32_t undirected,
                           rgnn_stream_t stream);
/* Companion of the guarded fill for everything DOWNSTREAM of it in a replayed step (CSR by target, chunk table, the edge
 * kernels: all sized for n_edges): rowptr_new is what this replay's count + scan produced.  If rowptr_new[n] == n_edges it is
 * copied to rowptr_committed; otherwise rowptr_committed keeps the rows of the last replay that matched -- consistent with the
 * col / edge_index the guarded fill then leaves untouched -- and status gets RGNN_STATUS_EDGE_COUNT_CHANGED (also when
 * n_edges == 0).  Downstream kernels read rowptr_committed only, so a replay on modified points computes on the previous
 * graph instead of walking rows that no longer fit its buffers. */
int rgnn_radius_rows_commit(const int32_t* rowptr_new /*[dev] n+1*/, int64_t n, int64_t n_edges,
                            int32_t* rowptr_committed /*[dev] n+1*/, int32_t* status /*[dev]*/,
                            const int32_t* deg_new /*[dev] n or NULL*/, int32_t* deg_committed /*[dev] n or NULL: the row
                            lengths travel with the rows (degree feature, lists of nodes with / without edges)*/,
                            rgnn_stream_t stream);

/* Radius graph with a neighbour cap, 1 <= k <= 128 (anything else: RGNN_ERR_INVALID_ARGUMENT): with S_i the row of the radius graph
 * (j != i, same frame, d2 <= r*r), row i is S_i when |S_i| <= k and otherwise the k entries of S_i smallest under the key (d2, j) --
 * distance ascending, a tie at the cut to the smaller index: the order of rgnn_knn_graph.  Rows are stored with ascending neighbour
 * ids, like rgnn_radius_graph_rows.  The graph is a function of the points alone (no atomics decide anything) and, unlike the radius
 * graph, NOT symmetric.  No reference counterpart (PyG's radius_graph(max_num_neighbors) truncates arbitrarily).
 * Protocol (same grid, same r and k in both calls):
 *   rgnn_radius_graph_capped_count   full[i] = |S_i| (int32 [n]) and lens (int32 [2 n]): lens[i] = min(|S_i|, k), lens[n + i] = the
 *                                    row's scratch entries in pass 2 (|S_i| for rows of more than 128 candidates, else 0);
 *   rgnn_exclusive_scan_i32          ptr (int32 [2 n + 1]) = scan of lens: ptr[0 .. n] is the rowptr, E = ptr[n], and the scratch
 *                                    holds n_spill = ptr[2 n] - ptr[n] entries -- both totals in one host read;
 *   rgnn_radius_graph_capped_rows    col int32 [E], edge_index int64 [2, E] or NULL.  spill: [dev] 12 * n_spill bytes, 8-byte
 *                                    aligned (NULL when n_spill == 0). */
int rgnn_radius_graph_capped_count(const rgnn_grid* g, double r, int32_t k, int32_t* full /*[dev] n*/, int32_t* lens /*[dev] 2 n*/,
                                   rgnn_stream_t stream);
int rgnn_radius_graph_capped_rows(const rgnn_grid* g, double r, int32_t k, const int32_t* full /*[dev] n*/,
                                  const int32_t* ptr /*[dev] 2 n + 1*/, int32_t* col /*[dev]*/, int64_t* edge_index /*[dev] or NULL*/,
                                  int64_t n_edges, void* spill /*[dev] or NULL*/, int64_t n_spill, rgnn_stream_t stream);

/* k nearest neighbours excluding self; nbr int32 [n,k], each row ordered (distance asc, index asc).  Optionally writes edge_index
 * int64 [2, n*k].  status gets RGNN_STATUS_KNN_TOO_FEW_POINTS if a frame has <= k points (rows of that frame are filled with -1).
 * Replaces sklearn kneighbors_graph behind graph_constructor/graph.py:52-66.  The write-out can do more (the team kernel has the
 * query's coordinates and the neighbour ids in hand), k <= 64 with either:
 *   relative_position != NULL: float [n k, 2] edge attributes [x_i - x_j, y_i - y_j] in edge order (graph.py:199-200; |.| when
 *     undirected != 0) -- what rgnn_edge_features(relative_position) computes in a launch of its own;
 *   degree_init != NULL: int32 [n] preset with the out-degree k, the starting point of rgnn_undirected_degree_preset.
 * max_frame_points > 0 (the hint rgnn_grid_build was given): frames of at most 1 024 points (nuScenes-shaped sweeps: ~300) with
 * 3 <= k <= 32 are searched by brute force per frame -- one wave per query, every point of the frame evaluated with the KD-tree's
 * float64 arithmetic, the k-th smallest distance found by a binary search over the distance bits -- instead of the walk over the
 * grid; same rows bit for bit.  0, or anything else: the walk over the grid. */
int rgnn_knn_graph(const rgnn_grid* g, int32_t k, int64_t max_frame_points, int32_t* nbr /*[dev]*/,
                   int64_t* edge_index /*[dev] or NULL*/, int32_t* status /*[dev]*/, float* relative_position /*[dev] or NULL*/,
                   int32_t undirected, int32_t* degree_init /*[dev] or NULL*/, rgnn_stream_t stream);
/* rgnn_undirected_degree for a `degree` array that already holds the out-degrees (rgnn_knn_graph degree_init): one launch. */
int rgnn_undirected_degree_preset(const int32_t* rowptr, const int32_t* col, int64_t n, int32_t* degree, rgnn_stream_t stream);
/* The same number for the rows of a kNN search (nbr int32 [n, k]) from the CSR by target of its edge list (rgnn_csr_by_target:
 * rowptr_t / src_sorted / node_order): k + in-degree - |{in-edges (s -> i) with s in nbr[i]}|; no atomics, every target's own row
 * is fetched once.  k <= 64.  Matches Graph.get_degree on the kNN adjacency (graph_constructor/graph.py:93-96). */
int rgnn_knn_degree_from_csr(const int32_t* rowptr_t, const int32_t* src_sorted, const int32_t* node_order, const int32_t* nbr, int64_t n,
                             int32_t k, int32_t* degree, rgnn_stream_t stream);
/* order[p] = global row of the p-th point in grid-cell order (frames back to back, cells row-major inside a
 * frame): a spatially coherent visiting order for the message-passing kernels (rgnn_mpnn_aggregate). */
int rgnn_grid_cell_order(const rgnn_grid* g, int32_t* order /*[dev] [n]*/, rgnn_stream_t stream);

/* Undirected degree: |{j : (i,j) in E or (j,i) in E}| for a CSR (rowptr,col) of the directed edges.
 * Replaces graph.py:93-96 (networkx Graph built from the dense adjacency). */
int rgnn_undirected_degree(const int32_t* rowptr, const int32_t* col, int64_t n, int32_t* degree_out, rgnn_stream_t stream);

/* Out-degree of every node as a rowptr: rowptr_s[p + 1] - rowptr_s[p] = number of edges whose SOURCE (edge_index row 0) is
 * the node at position p (position = rank[node], or the node id when rank is NULL).  With rgnn_split_targets this gives the
 * list of nodes that have outgoing edges -- the only rows of the source term Q = X W_j^T anybody gathers.  tmp: as for
 * rgnn_csr_by_target. */
int rgnn_source_rowptr(const int64_t* edge_index /*[dev] [2,E]*/, int64_t n, int64_t n_edges, const int32_t* rank /*[dev] or NULL*/,
                       int32_t* rowptr_s /*[dev] [n+1]*/, void* tmp, rgnn_stream_t stream);

/* rank[order[p]] = p (inverse of a visiting order such as rgnn_grid_cell_order's). */
int rgnn_invert_permutation(const int32_t* order, int64_t n, int32_t* rank, rgnn_stream_t stream);

/* CSR keyed on the aggregation target edge_index[1] (PyG flow source_to_target: messages of edge e are
 * reduced at edge_index[1][e]).  Stable: inside a segment edges keep ascending edge id, so sums are
 * deterministic.  Outputs rowptr_t int32 [n+1], src_sorted int32 [E] (= edge_index[0][perm]), perm int32 [E].
 * target_rank (optional, [dev] int32 [n]): segments are laid out in visiting order -- segment p holds the
 * edges whose target t has target_rank[t] == p -- so a kernel that visits targets in that order streams the
 * edge arrays contiguously.  NULL = natural order (segment t = target t).
 * ordered == 0: without the stable order inside the segments -- the places the fill's atomics hand out are the result (perm and
 * src_sorted agree with each other; which of a target's in-edges comes first varies from run to run).  For reductions that do not
 * depend on that order -- max aggregation (torch-scatter max behind mpnn_layers.py:88): one pass over the edges less.
 * tmp: [dev] of rgnn_csr_by_target_tmp_bytes(n, E) bytes. */
int64_t rgnn_csr_by_target_tmp_bytes(int64_t n, int64_t n_edges);
int rgnn_csr_by_target(const int64_t* edge_index /*[dev] [2,E]*/, int64_t n, int64_t n_edges,
                       const int32_t* target_rank /*[dev] [n] or NULL*/, int32_t* rowptr_t, int32_t* src_sorted, int32_t* perm,
                       void* tmp, int32_t ordered, rgnn_stream_t stream);

/* rgnn_csr_by_target for a batch of frames whose graph has UNIFORM out-degree k with edges grouped by source (kNN graphs:
 * edge e = i k + j; n_edges == n k): ONE launch, one block per frame -- histogram, scan, fill and stable ordering are local to a
 * frame because its edges are a contiguous slice and all their targets lie inside it.  max_frame_points: the caller's largest
 * frame (<= 24 576).  Optionally leaves in_degree int32 [n] (node numbering) and frame_nonempty int32 [n_frames] (nodes with
 * incoming edges per frame) behind -- the inputs of rgnn_split_by_degree_frames.  perm_tmp: [dev] int32 [n_edges] scratch.
 * Same rowptr_t / src_sorted / perm as rgnn_csr_by_target (ordered). */
int rgnn_csr_by_target_frames(const int64_t* edge_index, int64_t n, int64_t n_edges, int64_t k, const int64_t* frame_ptr,
                              int64_t n_frames, int64_t max_frame_points, const int32_t* target_rank /*[dev] or NULL*/,
                              int32_t* rowptr_t, int32_t* src_sorted, int32_t* perm, int32_t* perm_tmp,
                              int32_t* in_degree /*or NULL*/, int32_t* frame_nonempty /*or NULL*/, rgnn_stream_t stream);
/* The same result for a SYMMETRIC graph ((s,t) present <=> (t,s) present: radius graphs) whose edges are grouped by their
 * source in ascending source order with ascending targets inside a group -- exactly what rgnn_radius_graph_fill emits;
 * rowptr_src [dev] int32 [n+1] is that grouping (the search's rowptr).  A node's in-degree is then its row length and an
 * edge's place in its target's segment is the rank of its source in the target's row: no histogram, no atomics, no sort --
 * three small kernels instead of six.  Identical outputs to rgnn_csr_by_target (tests/test_gpu_graph.py).  If some (t,s) is
 * missing, *status (optional) gets RGNN_STATUS_NOT_SYMMETRIC and that edge is left out.  tmp: as above.
 * With edges, exactly ONE of perm and own_edge is given (else RGNN_ERR_INVALID_ARGUMENT).  own_edge (r03) instead of perm: no
 * twin search -- the slot of the in-edge (i -> t) receives the id of the OUT-edge (t -> i).  For callers whose edge attributes are
 * antisymmetric under reversal -- relative_position in directed mode: attr(i -> t) = -attr(t -> i), exactly -- the target-ordered
 * attributes are then -attr[own_edge[slot]].  SYMMETRY IS NOT CHECKED on that path (an edge (t -> i) without (i -> t) would
 * silently appear as an in-edge with negated attributes; RGNN_STATUS_NOT_SYMMETRIC is never set for a missing twin): only for
 * edge lists that are symmetric by construction -- the output of rgnn_radius_graph_fill. */
int rgnn_csr_by_target_symmetric(const int64_t* edge_index /*[dev] [2,E]*/, const int32_t* rowptr_src, int64_t n,
                                 int64_t n_edges, const int32_t* target_rank, int32_t* rowptr_t, int32_t* src_sorted,
                                 int32_t* perm /*[dev] or NULL*/, int32_t* own_edge /*[dev] or NULL*/, void* tmp,
                                 int32_t* status /*[dev] or NULL*/, rgnn_stream_t stream);

/* ================================================================ features
 * Edge feature codes, concatenated in list order (graph.py:139-223).                                  */
#define RGNN_EF_POINT_PAIR 0          /* 4: d, theta(v1,v2), theta(d,v1), theta(d,v2)  features.py:6-122 */
#define RGNN_EF_SPATIAL_DISTANCE 1    /* 1 */
#define RGNN_EF_VELOCITY_DISTANCE 2   /* 1 */
#define RGNN_EF_RELATIVE_POSITION 3   /* 2: X_i - X_j, i = E[:,0], j = E[:,1] */
#define RGNN_EF_RELATIVE_VELOCITY 4   /* 2 */
/* Node feature codes (graph.py:225-275). */
#define RGNN_NF_RCS 0
#define RGNN_NF_TIME_INDEX 1
#define RGNN_NF_DEGREE 2
#define RGNN_NF_VELOCITY_LENGTH 3
#define RGNN_NF_VELOCITY_VECTOR 4     /* 2 */
#define RGNN_NF_SPATIAL_COORDINATES 5 /* 2 */
#define RGNN_MAX_FEATURE_CODES 16

/* out[e, :] for every edge; X,V float64 [n,2]; edge_index int64 [2,E]; out row-major [E, width] where width
 * is implied by the codes; out_is_f64 selects float64 (GeometricGraph.E_feat) or float32 (create_graph_data,
 * dataset_creation.py:806).  undirected != 0 selects edge_mode "undirected". */
int rgnn_edge_features(const double* X, const double* V, const int64_t* edge_index, int64_t n_edges,
                       const int32_t* codes /*host*/, int32_t n_codes, int32_t undirected, void* out,
                       int32_t out_is_f64, int32_t* status /*[dev]*/, rgnn_stream_t stream);

/* The same features for the REVERSED edges at the rows of a list: out[s] = features(E[1][e], E[0][e]) with e = reversed_of[s]
 * (int32 [n_rows]).  With reversed_of = the own_edge list of rgnn_csr_by_target_symmetric this is the attribute list in target
 * order of a symmetric graph -- bit-identical to gathering every in-edge's own row (same arithmetic, same end points) -- without the
 * search for the twin's edge id.  Replaces the same reference lines as rgnn_edge_features (graph.py:139-223) plus the re-ordering that
 * torch_geometric's scatter makes unnecessary there. */
int rgnn_edge_features_reversed(const double* X, const double* V, const int64_t* edge_index, int64_t n_edges,
                                const int32_t* reversed_of, int64_t n_rows, const int32_t* codes, int32_t n_codes,
                                int32_t undirected, void* out, int32_t out_is_f64, int32_t* status, rgnn_stream_t stream);

/* Node feature matrix (graph.py:225-275): any of rcs/time_index [n] float64, degree int32 [n] may be NULL when
 * its code is not requested. */
int rgnn_node_features(const double* X, const double* V, const double* rcs, const double* time_index,
                       const int32_t* degree, int64_t n, const int32_t* codes /*host*/, int32_t n_codes, void* out,
                       int32_t out_is_f64, rgnn_stream_t stream);

/* time_index[i] = rank of timestamp[i] among the sorted distinct timestamps of its frame
 * (radarscenes/dataset_creation.py:214-223, nuscenes/conversion.py:94-103).  The timestamps must be NaN-free: the reference never
 * produces one, and a NaN has no rank (it is also the bit pattern of an empty slot of the hash set).  A frame with more than 3 072
 * distinct timestamps sets RGNN_STATUS_TIME_INDEX_OVERFLOW in *status; the time_index of that call is then not to be used. */
int rgnn_time_index(const double* timestamp, const int64_t* frame_ptr, int64_t n_frames, double* time_index,
                    int32_t* status /*[dev]*/, rgnn_stream_t stream);
/* rgnn_time_index for batches with LARGE frames (one 100 000-point cloud: one block per frame walks it alone in 160 us): the points
 * are spread over the chip -- a hash set of the frame's distinct timestamps in the caller's workspace (rgnn_time_index_ws_bytes),
 * one sort per frame, one rank look-up per point; same indices (dataset_creation.py:214-223: rank among np.unique of the frame). */
int64_t rgnn_time_index_ws_bytes(int64_t n_frames);
int rgnn_time_index_ws(const double* timestamp, const int64_t* frame_ptr, int64_t n_frames, int64_t n, double* time_index,
                       int32_t* status, void* ws /*[dev] rgnn_time_index_ws_bytes, 16-byte aligned*/, int64_t ws_bytes,
                       rgnn_stream_t stream);
/* rgnn_time_index + rgnn_node_features in one launch (one block per frame): the time index of a point goes straight into its
 * column of the feature row; same values as the two calls (graph.py:225-275, dataset_creation.py:214-223).  frame_nonempty, when
 * given, is ALWAYS filled for all n_frames frames (0 for an empty frame) -- also when there is no feature row to write (n == 0,
 * where degree may be NULL, or an empty feature list) --, so rgnn_split_by_degree_frames never reads an unwritten count. */
int rgnn_node_features_time_index(const double* X, const double* V, const double* rcs, const double* timestamp,
                                  const int64_t* frame_ptr, int64_t n_frames, const int32_t* degree /*[dev] or NULL*/, int64_t n,
                                  const int32_t* codes /*host*/, int32_t n_codes, void* out, int32_t out_is_f64,
                                  int32_t* status /*[dev]*/, int32_t* frame_nonempty /*[dev] int32 [n_frames] or NULL: nodes with
                                  degree > 0 per frame, for rgnn_split_by_degree_frames*/, rgnn_stream_t stream);
/* rgnn_split_targets_by_node for a SYMMETRIC graph (radius graphs: a node has incoming edges iff its own row is not empty) from
 * the degrees and the per-frame counts rgnn_node_features_time_index left behind: one launch (one block per frame) instead of
 * four.  Same lists, counts and slots. */
int rgnn_split_by_degree_frames(const int32_t* degree, const int64_t* frame_ptr, int64_t n_frames, const int32_t* frame_nonempty,
                                int32_t* list_empty, int64_t* count_empty, int32_t* slot_of_node /*or NULL*/,
                                int32_t* list_nonempty, int64_t* count_nonempty, rgnn_stream_t stream);

/* What the host reads back of a radius graph before it sizes the edge arrays (frames.build_graphs: one 8-byte copy per batch):
 * out2[0] = rowptr[n] (the edge count of rgnn_radius_graph_count + scan), out2[1] = edges in rows longer than `threshold` (symmetric
 * graph: in-degree = row length; radargnn_amd/gnn/mpnn_layers.py picks the form of the max aggregation by that share).  One launch. */
int rgnn_radius_counts(const int32_t* deg, int64_t n, const int32_t* rowptr, int32_t threshold, int32_t* out2, rgnn_stream_t stream);

/* ================================================================ dense layers (fp32, MFMA)
 * out[m, n] = act( sum_k A'[m,k] * W[n,k] + bias[n] ) (+ residual[m,n])
 * Replaces ATen addmm behind torch_geometric.nn.dense.linear.Linear (gnn/gnn_models.py:137-178,
 * gnn/mpnn_layers.py:64-74,89-90).  A' is the row-concatenation [A1 | A2] (torch.cat([x, m_emb], -1) at
 * mpnn_layers.py:89 without materialising it); W rows n < w_split come from W1, rows n >= w_split from W2
 * (lets one launch produce several projections of the same input).  If col_stats != NULL the kernel also
 * writes the column statistics (RGNN_STAT_ROWS floats per column and 128-row panel) of the stored `out`, the input of the
 * train-mode BatchNorm that follows every conv (gnn_models.py:126). */
/* Column statistics are kept per panel of 128 rows as RGNN_STAT_ROWS floats per column: {count of rows, a pivot taken from the
 * data, s1 = sum of (v - pivot), s2 = sum of (v - pivot)^2}.  Sums of small differences are exact or nearly so, so a column
 * whose spread is tiny against its mean loses nothing to cancellation or to the rounding of a mean (a constant column: s1 == s2
 * == 0 exactly); consumers form mean and variance in float64 (a zero-filled panel counts nothing).  (r03 kept {sum, sum of
 * squares} in float32: 1e-7 (mean / std)^2 relative in the variance.) */
#define RGNN_STAT_ROWS 4
/* A BatchNorm-apply table is RGNN_AFFINE_ROWS rows of n floats: {mean_hi, g, t} with y = (x - mean_hi) g + t, mean_hi = fl(mean),
 * g = fl(gamma / sqrt(var + eps)), t = fl(beta - (mean - mean_hi) g).  (r03 kept {scale, shift} and evaluated x scale + shift,
 * like ATen's CPU kernel: the rounding of mean * scale shows as 6e-8 |mean| / std in the normalised value.) */
#define RGNN_AFFINE_ROWS 3
typedef struct rgnn_linear_args {
  const float* A1; int64_t lda1; int32_t k1;    /* [M,k1]  */
  const float* A2; int64_t lda2; int32_t k2;    /* [M,k2] or NULL/0 */
  const float* W1; const float* W2; int64_t ldw; int32_t w_split; /* W rows have k1+k2 contiguous floats */
  const float* bias1; const float* bias2;       /* bias for rows < w_split / >= w_split; NULL = 0 */
  const float* residual; int64_t ldr;           /* added after the activation (RadarPointGNNConv h + x) */
  float* out; int64_t ldo;
  int64_t m; int32_t n;
  int32_t relu_out;
  float* col_stats;                             /* [panels, RGNN_STAT_ROWS, n] fp32 or NULL; panels = rgnn_linear_stat_panels(m) */
  /* Row subsets (all optional): tile row r works on matrix row row_index[r] of A1/A2/residual/out; the number of
   * rows is read from device memory (m_dev, with m an upper bound used for the launch geometry); accumulate: out +=
   * result (no col_stats with it).  Panels of col_stats that receive no rows are not written: zero the buffer first, or hand
   * the launch's row count to rgnn_batchnorm_finalize (rows_a / rows_b). */
  const int32_t* row_index;
  const int64_t* m_dev;
  int32_t accumulate;
  int32_t gather_only;               /* with row_index: gather the A rows only, write a compact [count, n] result */
  const int32_t* residual_index;     /* per output row: row of `residual` to add, -1 = none (NULL: same row) */
  /* Optional: the weight [W1; W2] pre-split into three bf16 planes by rgnn_linear_split_weights (3 n kp uint16, laid
   * out [kp / 32][3][n][32], kp = rgnn_linear_planes_kp(k1 + k2)).  When given (and no residual / row_index is used) the product runs on the
   * bf16 matrix pipe as a six-term split product with fp32 accumulation -- as accurate as the fp32 MFMA path (see
   * linear.hip), about twice as fast.  W1 / W2 must still be passed (they define the layer). */
  const void* W_planes;
  int32_t w_planes_kp;
  /* Optional [dev] scratch of rgnn_linear_splitk_ws_bytes() bytes, ZEROED once by the caller and then left to the library
   * (every launch leaves its flag words zero again).  With it the LDS-DMA kernel divides the (tile, k-step) units of a launch
   * evenly over the work-groups instead of dealing whole tiles (no partial tile rounds); a tile cut between two work-groups
   * is handed over through this scratch and accumulated in the order of the undivided tile: results are bit-identical with
   * and without it.  One launch at a time per scratch buffer (launches on one stream qualify).
   * A work-group that waits for a partial tile longer than ~1 s gives up (a wrong tile is a better failure than a device that
   * never comes back) and counts it in int32 word RGNN_SPLITK_TIMEOUT_WORD of the flag area, i.e. at byte offset
   * rgnn_linear_splitk_ws_bytes() - 4096 + 4 * RGNN_SPLITK_TIMEOUT_WORD of the scratch: callers that read device status words
   * back should read this one too (radargnn_amd: GraphBatch.check() raises RGNN_STATUS_SPLITK_TIMEOUT). */
  void* splitk_ws;
  int64_t splitk_ws_bytes;
  /* Optional: the A1 operand is act((A1 - mean) g + t) per column -- the train-mode BatchNorm + ReLU that precedes the layer
   * (gnn_models.py:126-128), applied to the activation fragment on its way into the matrix pipe instead of in a pass of its
   * own over [M, k1].  a1_scale_shift: [dev] float [RGNN_AFFINE_ROWS, k1] (what rgnn_batchnorm_finalize writes: A1' = act((A1 - mean_hi) g + t));
   * a1_relu: clamp at 0 afterwards.  The LDS-DMA kernel and the fp32 kernel on buffer-descriptor operands do this: ask rgnn_linear_fwd_fuses_a1_affine(args) first and
   * otherwise apply rgnn_scale_shift_act to A1 (rgnn_linear_fwd returns RGNN_ERR_UNSUPPORTED rather than ignore it). */
  const float* a1_scale_shift;
  int32_t a1_relu;
  /* relu_out applies to the output columns >= relu_from_col only (0: all).  Lets one launch compute the first Linear of
   * both heads (gnn_models.py:131-132: logits without activation | hidden layer of the box head with ReLU) from one pass
   * over the node features.  Not on the <= 8-wide-input kernel (the call then takes the general one). */
  int32_t relu_from_col;
  /* Optional (r03): the f16x2 form of the LDS-DMA kernel -- every fp32 operand as TWO f16 terms after an exact power-of-two
   * pre-scale, THREE matrix-pipe products per fp32 product instead of the six of the bf16x3 form (a = h + l carries 22
   * significand bits; the dropped l l' term is <= 2^-22 |a a'|: as accurate as the fp32 MFMA kernel).  Taken when the launch
   * qualifies for the LDS-DMA kernel (rgnn_linear_fwd_path) and all of these are given:
   *   W_planes_f16: rgnn_linear_planes_f16_bytes(n, k1 + k2) bytes written by rgnn_linear_split_weights_f16;
   *   a1_bound / a2_bound: [dev] bounds (RGNN_BOUND_SLOTS floats each, see below) holding an UPPER BOUND of |A1'| (A1 after a1_scale_shift / a1_relu) and of |A2|
   *     (a2_bound only when k2 > 0).  Elements beyond the bound overflow to infinity; a bound up to 2^19 above the tensor's
   *     typical magnitude costs no accuracy.  Producers: out_absmax of the launch that wrote the operand,
   *     rgnn_mpnn_aggregate's out_absmax, rgnn_batchnorm_finalize's out_bound for an operand behind a1_scale_shift.
   * out_absmax: [dev] bound (RGNN_BOUND_SLOTS floats), raised to max |out| over everything this launch stores (zero it first; LDS-DMA kernel
   *   only, either form: rgnn_linear_fwd returns RGNN_ERR_UNSUPPORTED if another kernel would take the launch). */
  const void* W_planes_f16;
  const float* a1_bound;
  const float* a2_bound;
  float* out_absmax;
  /* Optional (r03), with row_index AND a1_scale_shift: per-SEGMENT scale / shift -- the train-mode BatchNorm of a batch whose
   * frames are normalised with their OWN statistics (the reference's one-frame-per-forward inference loop, evaluate.py:40 +
   * gnn_models.py:124-128), still applied on the way into the matrix pipe.  a1_scale_shift is then [S, RGNN_AFFINE_ROWS, k1]
   * (rgnn_batchnorm_segments_from_panels) and a1_panel_segment: [dev] int32 [ceil(m / 256)] names the table of every 256-row
   * tile of the row list -- the list keeps a segment's rows inside tiles of their own, padded with -1 entries
   * (rgnn_pad_list_by_segment writes list and map).  LDS-DMA kernel only: rgnn_linear_fwd_fuses_a1_affine says whether the
   * launch qualifies.  A row_index entry of -1 is an absent row there: nothing is read, stored or counted for it -- ON THE LDS-DMA
   * KERNEL ONLY (rgnn_linear_fwd_path != 0), with or without tables; no other kernel checks, so ask before handing over a padded
   * list.  As for every
   * row list, m bounds the matrix rows the list may name; the padded list itself may be longer (*m_dev > m is fine), and
   * col_stats then needs rgnn_linear_stat_panels(*m_dev) panels. */
  const int32_t* a1_panel_segment;
} rgnn_linear_args;
/* A "bound" in this header is an array of RGNN_BOUND_SLOTS floats in device memory, zeroed by the caller before its first
 * producer runs: producers raise individual slots (atomic max, one slot per work-group), consumers take the maximum over all
 * slots.  To hand in a bound computed elsewhere, write it to slot 0 and zero the rest. */
#define RGNN_BOUND_SLOTS 256
enum { RGNN_LINEAR_PATH_OTHER = 0, RGNN_LINEAR_PATH_DMA_BF16X3 = 1, RGNN_LINEAR_PATH_DMA_F16X2 = 2 };
/* Which kernel family rgnn_linear_fwd would launch for these arguments (host-side, no launch). */
int32_t rgnn_linear_fwd_path(const rgnn_linear_args* args /*host*/);
int64_t rgnn_linear_planes_f16_bytes(int32_t n, int32_t k);
int rgnn_linear_split_weights_f16(const float* W1, const float* W2, int64_t ldw, int32_t w_split, int32_t n, int32_t k,
                                  void* planes /*[dev] rgnn_linear_planes_f16_bytes(n, k) bytes*/, rgnn_stream_t stream);
int32_t rgnn_linear_fwd_fuses_a1_affine(const rgnn_linear_args* args /*host*/);
/* The launch plan rgnn_linear_fwd would follow for these arguments (host-side, no launch, nothing behind the pointers is read);
 * the two queries above are views of the same plan.  out: {RGNN_LINEAR_FAMILY_*, operand form of the split-product families
 * (RGNN_LINEAR_PATH_DMA_BF16X3 / _F16X2, else 0), columns of a tile, column tiles (both 0 on the <= 8-wide-input kernel), row-subset
 * instance, operands through buffer descriptors, a1_scale_shift applied by the kernel (per-segment tables if a1_panel_segment
 * is given, else one table), split-K scratch used}.  RGNN_LINEAR_FAMILY_NONE: rgnn_linear_fwd launches nothing or refuses. */
enum { RGNN_LINEAR_FAMILY_NONE = 0, RGNN_LINEAR_FAMILY_TINY = 1, RGNN_LINEAR_FAMILY_FP32 = 2, RGNN_LINEAR_FAMILY_X3 = 3,
       RGNN_LINEAR_FAMILY_DMA = 4 };
void rgnn_linear_fwd_plan(const rgnn_linear_args* args /*host*/, int32_t out[8] /*host*/);
int64_t rgnn_linear_splitk_ws_bytes(void);
int64_t rgnn_linear_stat_panels(int64_t m);
int32_t rgnn_linear_planes_kp(int32_t k);
int rgnn_linear_split_weights(const float* W1, const float* W2, int64_t ldw, int32_t w_split, int32_t n, int32_t k,
                              void* planes /*[dev] uint16, 3 n kp of them*/, rgnn_stream_t stream);
int rgnn_linear_fwd(const rgnn_linear_args* args /*host*/, rgnn_stream_t stream);
/* Two INDEPENDENT dense launches (neither reads what the other writes, their output rows are disjoint) handed over together:
 * the same results, bit for bit, as rgnn_linear_fwd(second) followed by rgnn_linear_fwd(first) -- output rows, col_stats panels
 * and out_absmax slots.  Where both are row-subset launches of the LDS-DMA kernel's f16x2 form on its static tile schedule (no
 * per-segment tables, no residual / accumulate / gather_only, no use of splitk_ws whatever *m_dev holds) and their column-tile
 * widths are a pair the library is built for (the conv layers' source term beside their isolated-row update: n = 464 | 224,
 * 464 | 128, 272 | 64), they run as ONE grid: the launch with more tiles in front, the other one's work-groups starting on
 * compute units as the first one's retire, instead of behind its last, partly filled tile round.  Neither part waits for the
 * other.  Any other pair, RGNN_NO_LINEAR_PAIR in the environment, or armed profiling events (rgnn_profile_next_launch): the two
 * launches.  rgnn_linear_fwd_pair_fuses: 1 if the pair would run as one grid (host-side, no launch). */
int32_t rgnn_linear_fwd_pair_fuses(const rgnn_linear_args* first /*host*/, const rgnn_linear_args* second /*host*/);
int rgnn_linear_fwd_pair(const rgnn_linear_args* first /*host*/, const rgnn_linear_args* second /*host*/, rgnn_stream_t stream);

/* Three Linear layers back to back in one pass: out = act3(W3 relu(W2 relu(W1 x + b1) + b2) + b3) for k0 <= 8 inputs and layers
 * of 32, 64 and 128 columns -- DetNetBasic's node embedding (gnn_models.py:137-178, node_feature_embedding_layer_dimensions
 * [32, 64, 128, ...]; rgnn_embed3_supported says whether a shape qualifies).  W1 fp32 [n1, k0] (row stride ldw1); W2 / W3 as the
 * f16 planes rgnn_linear_split_weights_f16 writes for [n2, n1] / [n3, n2]; layers 2 and 3 run in the f16x2 form of
 * rgnn_linear_fwd, pre-scaled per 32-row block from maxima computed on the way.  out_absmax: optional bound of |out| (see
 * RGNN_BOUND_SLOTS). */
int32_t rgnn_embed3_supported(int32_t k0, int32_t n1, int32_t n2, int32_t n3);
int rgnn_embed3(const float* x, int64_t ldx, int32_t k0, const float* W1, int64_t ldw1, const float* b1, int32_t n1,
                const void* W2_planes_f16, const float* b2, int32_t n2, const void* W3_planes_f16, const float* b3, int32_t n3,
                int32_t relu3, int64_t m, float* out, int64_t ldo, float* out_absmax, rgnn_stream_t stream);
/* Two tiny Linear layers back to back on (optionally gathered) rows: out[r] = act2(W2 act1(W1 a[row_index[r]] + b1) + b2),
 * k0 <= 8 inputs, n1 <= 8 hidden, n2 <= 16 outputs; row_index NULL = identity.  The hidden layers of DetNetBasic's edge
 * embedding (gnn_models.py:48-52,137-178) on the edge attributes in CSR-by-target order: one pass instead of
 * rgnn_gather_rows_f32 + two rgnn_linear_fwd launches, same bits. */
int rgnn_tiny_mlp2(const float* A, int64_t lda, int32_t k0, const int32_t* row_index /*[dev] or NULL*/, int64_t m,
                   const float* W1, int64_t ldw1, const float* b1, int32_t n1, int32_t relu1, const float* W2, int64_t ldw2,
                   const float* b2, int32_t n2, int32_t relu2, float* out, int64_t ldo, rgnn_stream_t stream);

/* ================================================================ BatchNorm1d (gnn_models.py:71-73,126-128)
 * Training: combine col_stats (float64) -> batch mean / biased variance -> the apply table {mean_hi, g, t} (RGNN_AFFINE_ROWS);
 * running stats updated with momentum and the unbiased variance; num_batches_tracked += 1.
 * Eval (training == 0): the table from the running statistics, col_stats ignored.
 * The rows of a layer may come from TWO row-subset launches (mpnn_layers.py:89-90 on the targets with and without incoming
 * edges), each with a col_stats buffer of its own: stats_b may be NULL (one part); rows_a / rows_b ([dev], optional) are the
 * m_dev row counts of those launches -- only the ceil(rows / 128) panels a launch really wrote are read, so the buffers need no
 * zero fill.  Bound for the f16x2 dense form (rgnn_linear_args.a1_bound; both optional, out_bound needs in_bound): in_bound [dev]
 * (a bound, RGNN_BOUND_SLOTS floats) holds an upper bound B of |x| over the matrix the statistics were taken of (the producing
 * launches' out_absmax); out_bound ([dev] bound, zeroed by the caller) receives max over the columns of
 * |g| (B + |mean_hi|) + |t| -- an upper bound of |(x - mean_hi) g + t|, hence of the ReLU of it. */
int rgnn_batchnorm_finalize(const float* stats_a, int64_t panels_a, const int64_t* rows_a /*[dev] or NULL*/,
                            const float* stats_b /*or NULL*/, int64_t panels_b, const int64_t* rows_b /*[dev] or NULL*/,
                            int64_t m, int32_t n, const float* gamma, const float* beta, float* running_mean,
                            float* running_var, int64_t* num_batches_tracked, int32_t training, float momentum, float eps,
                            float* scale_shift /*[RGNN_AFFINE_ROWS,n]*/, const float* in_bound /*or NULL*/,
                            float* out_bound /*or NULL*/, rgnn_stream_t stream);
/* Train-mode BatchNorm with statistics PER SEGMENT of rows -- segment f = rows [seg_ptr[f], seg_ptr[f + 1]), one segment per
 * radar frame of a batch.  The reference runs inference one frame per forward and never calls .eval() (evaluate.py:40,
 * postprocessor/inference.py:57-62, gnn/gnn_models.py:124-128): every frame is normalised with its own batch statistics; this
 * reproduces that in a batched launch.  table [dev] float [n_seg, RGNN_AFFINE_ROWS, n] receives the apply table of every segment; the running
 * statistics are walked through the segments in order (what a loop of single-frame forwards does), num_batches_tracked grows
 * by the number of non-empty segments.  seg_sums: [dev] scratch, double [n_seg, 2, n]; on return it holds {mean, unbiased
 * variance} per (segment, column) (zeros for an empty segment) -- the exact statistics rgnn_bn_segments_bwd reads.  in_bound /
 * out_bound: as in rgnn_batchnorm_finalize (optional). */
int rgnn_batchnorm_segments(const float* x, int64_t ldx, const int64_t* seg_ptr /*[dev] n_seg + 1*/, int64_t n_seg, int32_t n,
                            const float* gamma, const float* beta, float* running_mean, float* running_var,
                            int64_t* num_batches_tracked, float momentum, float eps, double* seg_sums, float* table,
                            const float* in_bound, float* out_bound, rgnn_stream_t stream);
/* rgnn_batchnorm_segments + rgnn_scale_shift_act_segments in two launches instead of three: the block that sums a (segment,
 * 64-channel slab) also normalises it (its second pass over the slab hits L2), y = act((x - mean_hi) g + t); the second launch walks
 * the running statistics, writes the table and the bound as rgnn_batchnorm_segments does.  y != x. */
int rgnn_batchnorm_act_segments(const float* x, int64_t ldx, const int64_t* seg_ptr, int64_t n_seg, int32_t n, const float* gamma,
                                const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                float momentum, float eps, int32_t relu, double* seg_sums, float* table, float* y, int64_t ldy,
                                const float* in_bound, float* out_bound, rgnn_stream_t stream);
/* The same table from column statistics the dense launches already left behind (rgnn_linear_args.col_stats: one partial per
 * 128-row panel of the launch's row list) instead of a pass over x -- for row lists padded per segment
 * (rgnn_pad_list_by_segment): segment f owns panels [panel_start_a[f], panel_start_a[f + 1]) of list a and likewise of list b
 * (b optional: the conv layers run two launches, targets with and without edges).  seg_ptr: rows per segment as above (the
 * counts the variances divide by).  seg_sums: scratch, double [n_seg, 2, n]. */
int rgnn_batchnorm_segments_from_panels(const float* stats_a, const int32_t* panel_start_a, const float* stats_b,
                                        const int32_t* panel_start_b, const int64_t* seg_ptr, int64_t n_seg, int32_t n,
                                        const float* gamma, const float* beta, float* running_mean, float* running_var,
                                        int64_t* num_batches_tracked, float momentum, float eps, double* seg_sums, float* table,
                                        const float* in_bound, float* out_bound, rgnn_stream_t stream);
/* An ascending row list cut at the segment borders and padded with -1 so that every segment starts a 256-row tile of its own:
 * list int32 [*count] ascending, seg_ptr int64 [n_seg + 1] (row ranges of the segments) -> out_list (room for *count + 256 n_seg
 * entries), *out_count, tile_segment int32 [out_count / 256] (rgnn_linear_args.a1_panel_segment), stat_panel_start int32
 * [n_seg + 1] in units of the 128-row statistics panels (rgnn_batchnorm_segments_from_panels).  All [dev]. */
int rgnn_pad_list_by_segment(const int32_t* list, const int64_t* count, const int64_t* seg_ptr, int64_t n_seg, int32_t* out_list,
                             int64_t* out_count, int32_t* tile_segment, int32_t* stat_panel_start, rgnn_stream_t stream);
/* Two lists over the same segments in ONE launch (a batch's targets with / without edges). */
int rgnn_pad_list_pair_by_segment(const int32_t* list_a, const int64_t* count_a, const int32_t* list_b, const int64_t* count_b,
                                  const int64_t* seg_ptr, int64_t n_seg, int32_t* out_list_a, int64_t* out_count_a,
                                  int32_t* tile_segment_a, int32_t* stat_panel_start_a, int32_t* out_list_b, int64_t* out_count_b,
                                  int32_t* tile_segment_b, int32_t* stat_panel_start_b, rgnn_stream_t stream);
/* y[r] = (x[r] - mean_hi[seg(r)]) g[seg(r)] + t[seg(r)], optional ReLU, with the table of rgnn_batchnorm_segments; in place allowed. */
int rgnn_scale_shift_act_segments(const float* x, int64_t ldx, const float* table, const int64_t* seg_ptr, int64_t n_seg,
                                  int64_t m, int32_t n, int32_t relu, float* y, int64_t ldy, rgnn_stream_t stream);
/* Column statistics of an arbitrary [m,n] matrix in the panel layout above (BatchNorm on an input that did not
 * come out of rgnn_linear_fwd, e.g. BatchNorm modules called on their own). */
int rgnn_column_stats(const float* x, int64_t ldx, int64_t m, int32_t n, float* col_stats /*[panels,RGNN_STAT_ROWS,n]*/,
                      rgnn_stream_t stream);
/* y = (x - mean_hi) g + t with a table of rgnn_batchnorm_finalize, optional ReLU (F.relu, gnn_models.py:128); in place allowed. */
int rgnn_scale_shift_act(const float* x, int64_t ldx, const float* scale_shift, int64_t m, int32_t n, int32_t relu,
                         float* y, int64_t ldy, rgnn_stream_t stream);

/* ================================================================ message passing
 * Fused gather + per-edge linear + segmented reduce for a message MLP that is a single Linear
 * (pre_layers == 1, mpnn_layers.py:64-68), using linearity:
 *   reduce_e( W_i x_t + W_j x_s + W_e a_e + b ) = P[t] (.) + reduce_e( Q[s_e] + W_e a_e )
 * P (may be NULL: RadarPointGNNConv has no x_i term, only `p_bias`) and Q are node-wise projections
 * produced by rgnn_linear_fwd.  Edges are visited in CSR-by-target order; `edge_attr_sorted` is
 * edge_attr[perm].  aggr: 0 = max, 1 = mean, 2 = add; empty segments give exactly 0 (torch-scatter).
 * aggr 3 = min, 4 = var, 5 = std (torch_geometric 2.1 nn/aggr/basic.py), per channel over the messages m_e of a segment of cnt edges:
 *   min: P + b + min_e(Q[s_e] + W_e a_e) on targets with edges, exactly 0 on the others;
 *   var: mean_e(m_e^2) - (mean_e m_e)^2, not clamped, 0 on empty segments;   std: sqrt(relu(var) + 1e-5), sqrt(1e-5) on empty segments.
 *   var and std do not change when every message of a segment is shifted by the same amount: P AND p_bias ARE IGNORED for codes 4
 *   and 5 (never read; pass NULL).  The sums run over d_e = m_e - m_0 (m_0: the segment's first message in CSR order), var =
 *   sum d^2 / cnt - (sum d / cnt)^2: a segment of one edge or of equal messages gives exactly 0 (std: exactly sqrtf(1e-5f)).
 *   These codes write every row (RGNN_MPNN_SKIP_EMPTY_ROWS is accepted and has no effect) and track out_absmax in the kernel.
 * `node_order` (with a CSR built with the matching `target_rank`) only changes the order in which targets are
 * processed (cache locality), never the result: segment p of the CSR belongs to target node_order[p].
 * Replaces MessagePassing.propagate (index_select gathers + cat + addmm + scatter) at
 * mpnn_layers.py:88,94-101 / :173,179-184.
 * flags: RGNN_MPNN_SKIP_EMPTY_ROWS -- rows of `out` that belong to targets without incoming edges may be left unwritten (callers
 * that run the update only on the other rows -- rgnn_split_targets -- never read them; it saves their share of the output traffic).
 * out_absmax ([dev] bound of RGNN_BOUND_SLOTS floats, zeroed by the caller; NULL = not wanted): the maximum of |out| over the rows
 * written -- the bound the f16x2 dense form wants for its A2 operand (rgnn_linear_args.a2_bound).  The fused max kernel tracks it
 * per lane at no measurable cost; other kernels are followed by one pass over `out`. */
#define RGNN_AGGR_MAX 0
#define RGNN_AGGR_MEAN 1
#define RGNN_AGGR_ADD 2
#define RGNN_AGGR_MIN 3
#define RGNN_AGGR_VAR 4
#define RGNN_AGGR_STD 5
#define RGNN_MPNN_SKIP_EMPTY_ROWS 1
int rgnn_mpnn_aggregate(const float* P, int64_t ldp, const float* p_bias, const float* Q, int64_t ldq,
                        const float* We /*[d, de], row stride ldwe*/, int64_t ldwe, const float* edge_attr_sorted,
                        int32_t de, const int32_t* rowptr_t, const int32_t* src_sorted,
                        const int32_t* node_order /*[dev] [n] visiting order of the targets, or NULL*/,
                        const int32_t* chunk_start /*[dev] from rgnn_mpnn_partition, or NULL*/, int32_t n_chunks, int64_t n,
                        int32_t d, int32_t aggr, float* out, int64_t ldo, int32_t flags, float* out_absmax /*[dev] or NULL*/,
                        rgnn_stream_t stream);
/* Max aggregation without a target term, recording the winners for the backward pass: arg_out uint16 [n, d] receives, per
 * target with incoming edges and channel, the index INSIDE the target's segment of the first edge that attains the maximum
 * (in-degrees must stay below 65 536).  Only the fused max kernel can record them (d % 8 == 0, 16-byte aligned rows, chunk
 * table given, de <= 8): *arg_written (host, required) says what ran -- bit 0 = winners recorded (if clear, out is complete but
 * arg_out is untouched and rgnn_mpnn_max_bwd recomputes the winners), bit 1 = max |out| raised into out_absmax (NULL = not
 * wanted; over the rows written), so that the update GEMM of a TRAINING forward takes the f16x2 form like the inference one. */
int rgnn_mpnn_aggregate_max_arg(const float* p_bias, const float* Q, int64_t ldq, const float* We, int64_t ldwe,
                                const float* edge_attr_sorted, int32_t de, const int32_t* rowptr_t, const int32_t* src_sorted,
                                const int32_t* node_order, const int32_t* chunk_start, int32_t n_chunks, int64_t n, int32_t d,
                                float* out, int64_t ldo, uint16_t* arg_out, int32_t flags, int32_t* arg_written /*host*/,
                                float* out_absmax /*[dev] or NULL*/, rgnn_stream_t stream);

/* ---- window form of the max aggregation (mpnn_tiles.hip; what the folded layers run on graphs it pays for) ---------------------
 * The same sum as rgnn_mpnn_aggregate with aggr = max, P = NULL and de <= 8 (the folded layers the models ship), computed
 * 32 edges x 32 channels at a time: the gathered Q values are the accumulator's initial value of v_mfma_f32_32x32x16_bf16 and
 * W_e z_e comes from the matrix pipe, z and W_e each split exactly into three bf16 terms (six products, fp32 accumulate:
 * ~2^-22 |z||w| from the fp32 chain of the per-edge kernel -- a frame's low bits therefore depend on which kernel its batch's
 * density and size select).  The rows of Q are not gathered per edge: a window of ~15-40 consecutive targets (<= 8 streams of
 * <= 64 slots, every target padded to a multiple of 4 slots with repeated edges and packed whole into a stream) stages its
 * DISTINCT sources (<= 176) in LDS once per 32-channel tile (LDS-DMA, double-buffered) and the accumulators are initialised from
 * there.  In grid-cell order a window names each source ~5 times, so the L2 -> CU traffic falls from E rows to ~E / 5.  Windows
 * are pipelined across each other (r05): the next window's descriptors and first row stage are requested while this one runs.
 * Targets with more than 64 padded slots and targets a full window leaves over go through a per-target kernel (none on
 * r = 1 m graphs, a few dozen per k = 20 batch).
 *   plan: [dev] int32 [rgnn_mpnn_win_plan_ints(n, n_edges)], 16-byte aligned, filled by rgnn_mpnn_win_plan from the CSR by target
 *         (rowptr_t / src_sorted / node_order as for rgnn_mpnn_aggregate); once per graph, shared by all layers; holds the ticket
 *         counters and a weight scratch: ONE LAUNCH AT A TIME PER PLAN (two streams need two plans).
 * Returns RGNN_ERR_UNSUPPORTED for de > 8, d > 2048, n >= 2^24, Q rows not 16-byte aligned (ldq % 4, base address), rows of
 * 2^24 bytes or more, matrices or a plan of 2 GiB or more: the caller then takes rgnn_mpnn_aggregate
 * (radargnn_amd/gnn/mpnn_layers.py mirrors these limits).
 * flags / out_absmax as for rgnn_mpnn_aggregate.  Matches gnn/mpnn_layers.py:94-101 + torch-scatter max (hoisted form).
 * wplanes: the kernel's operand image of one layer's weights -- per 32-channel tile the three bf16 terms of W_e [d, de <= 8] and the
 * bias -- depends on the weights only.  NULL: built into the plan's scratch in front of the launch (5 us); a caller that keeps it
 * per weight version builds it once with rgnn_mpnn_win_wplanes ([dev] rgnn_mpnn_win_wplanes_bytes(d) bytes, 16-byte aligned) and
 * passes it with the SAME We / p_bias (the per-target kernel still reads them). */
int64_t rgnn_mpnn_win_plan_ints(int64_t n, int64_t n_edges);
/* diagnostics: the words of a built plan that hold the number of targets left to the per-target kernel / of windows made */
void rgnn_mpnn_win_plan_counters(int64_t n, int64_t n_edges, int64_t* leftover_word /*host*/, int64_t* windows_word /*host*/);
int rgnn_mpnn_win_plan(const int32_t* rowptr_t, const int32_t* src_sorted, const int32_t* node_order, int64_t n, int64_t n_edges,
                       int32_t* plan, rgnn_stream_t stream);
int64_t rgnn_mpnn_win_wplanes_bytes(int32_t d);
int rgnn_mpnn_win_wplanes(const float* We, int64_t ldwe, int32_t de, int32_t d, const float* p_bias, void* planes, rgnn_stream_t stream);
int rgnn_mpnn_aggregate_win(const float* p_bias, const float* Q, int64_t ldq, const float* We, int64_t ldwe,
                            const float* edge_attr_sorted, int32_t de, const int32_t* rowptr_t, const int32_t* src_sorted,
                            const int32_t* node_order, int32_t* plan, int64_t n, int64_t n_edges, int32_t d, float* out, int64_t ldo,
                            int32_t flags, float* out_absmax, const void* wplanes /*[dev] or NULL*/, rgnn_stream_t stream);

/* Targets without incoming edges, in visiting order: list[0..count) = node ids (node_order[p] or p) of the empty CSR
 * segments; count is written to device memory (int64).  Deterministic (scan based).  flags_tmp: int32 [n],
 * scan_tmp: rgnn_scan_tmp_bytes(n) bytes, pos_tmp: int32 [n+1]. */
int rgnn_empty_targets(const int32_t* rowptr_t, const int32_t* node_order, int64_t n, int32_t* flags_tmp,
                       int32_t* pos_tmp, void* scan_tmp, int32_t* list, int64_t* count,
                       int32_t* slot_of_node /*[n] or NULL: position in `list`, -1 for targets with edges*/,
                       rgnn_stream_t stream);

/* Same, additionally the complement: list_nonempty[0..count_nonempty) = the targets WITH incoming edges, in visiting
 * order.  On a symmetric edge set (radius graphs) these are also the only nodes that occur as a source, so the dense
 * layers of a conv can be restricted to them (rgnn_linear_fwd row_index / m_dev) and the others take a cheaper path. */
int rgnn_split_targets(const int32_t* rowptr_t, const int32_t* node_order, int64_t n, int32_t* flags_tmp, int32_t* pos_tmp,
                       void* scan_tmp, int32_t* list, int64_t* count, int32_t* slot_of_node, int32_t* list_nonempty,
                       int64_t* count_nonempty, rgnn_stream_t stream);

/* The same two lists in ascending NODE order instead of visiting order (rank [dev] int32 [n]: CSR segment of node i is
 * rank[i]; NULL = identity).  What the row-subset launches of rgnn_linear_fwd want: they then stream the activation matrix
 * front to back (the grid-cell visiting order jumps around inside every frame; measured 7 % slower). */
int rgnn_split_targets_by_node(const int32_t* rowptr_t, const int32_t* rank, int64_t n, int32_t* flags_tmp, int32_t* pos_tmp,
                               void* scan_tmp, int32_t* list, int64_t* count, int32_t* slot_of_node,
                               int32_t* list_nonempty, int64_t* count_nonempty, rgnn_stream_t stream);

/* Work-balanced split of the CSR-by-target into chunks of ~80 units of (edges + 2 targets): chunk_start int32
 * [rgnn_mpnn_num_chunks(n, E) + 1 + 1024]: the table, followed by 1024 ints of ticket counters (persistent waves pull
 * chunks per XCD) that rgnn_mpnn_partition zeroes and every rgnn_mpnn_aggregate / rgnn_mpnn_edge_hidden launch leaves
 * zeroed again -- one launch at a time per table.  Computed once per graph, shared by all layers. */
int32_t rgnn_mpnn_num_chunks(int64_t n, int64_t n_edges);
/* The tuning values behind the chunk count: work units per chunk (80 on full batches, finer -- down to 16 -- on graphs
 * too small to fill the chip at 80) and the weight of one target in units
 * (num_chunks = ceil((E + weight * n) / units) + 1).  Exposed so callers and tests need not hard-code them. */
int32_t rgnn_mpnn_work_units(int64_t n, int64_t n_edges);
int32_t rgnn_mpnn_target_weight(int64_t n, int64_t n_edges);
int rgnn_mpnn_partition(const int32_t* rowptr_t, int64_t n, int64_t n_edges, int32_t* chunk_start, rgnn_stream_t stream);

/* General path (pre_layers > 1): first message layer per edge, hidden[e,:] = relu?(P[t_e] + Q[s_e] + W_e a_e),
 * rows in CSR-by-target order, then rgnn_linear_fwd on the [E,d] rows, then rgnn_segment_reduce (aggr 0 .. 5 as above, literally over
 * the rows of a segment: nothing is hoisted or ignored here). */
int rgnn_mpnn_edge_hidden(const float* P, int64_t ldp, const float* p_bias, const float* Q, int64_t ldq,
                          const float* We, int64_t ldwe, const float* edge_attr_sorted, int32_t de,
                          const int32_t* rowptr_t, const int32_t* src_sorted, const int32_t* node_order,
                          const int32_t* chunk_start, int32_t n_chunks, int64_t n, int32_t d, int32_t relu, float* hidden,
                          int64_t ldh, rgnn_stream_t stream);
int rgnn_segment_reduce(const float* rows, int64_t ldr, const int32_t* rowptr_t, const int32_t* node_order, int64_t n,
                        int32_t d, int32_t aggr, float* out, int64_t ldo, rgnn_stream_t stream);

/* out[i,:] = in[perm[i],:] for rows of `width` 4-byte elements (edge_attr -> CSR-by-target order). */
int rgnn_gather_rows_f32(const float* in, int64_t ldi, const int32_t* perm, int64_t n_rows, int32_t width, float* out,
                         int64_t ldo, rgnn_stream_t stream);

/* Row softmax of the class logits (postprocessor/inference.py:46,62). */
int rgnn_softmax_rows(const float* x, int64_t ldx, int64_t m, int32_t n, float* y, int64_t ldy, rgnn_stream_t stream);

/* The epilogue of one prediction step (postprocessor/inference.py:51-68) in one launch, for the rows r < n of the step:
 *   prob[r, :n_classes]        = softmax(cls[r, :n_classes])   -- the statements of rgnn_softmax_rows: bit-equal to it
 *   bb_out[r, :box_width]      = bb[r, :box_width]
 *   class_true[r]              = y[r, 0]                       -- y: float32 or float64 (y_is_f64), moved word for word
 *   bb_true[r, :target_width]  = y[r, 1 : 1 + target_width]
 * The outputs are rows of whole-split buffers: the caller passes their pointers advanced to the step's first row.  Leading
 * dimensions count elements of the matrix's own type (ldy and ldt: of y's).  y may be NULL: class_true and bb_true are then
 * not touched.  n == 0 returns RGNN_OK without a launch. */
int rgnn_predict_rows(const float* cls, int64_t ldc, int32_t n_classes, const float* bb, int64_t ldb, int32_t box_width,
                      const void* y, int64_t ldy, int32_t y_is_f64, int32_t target_width, int64_t n, float* prob, int64_t ldp,
                      float* bb_out, int64_t ldo, void* class_true, void* bb_true, int64_t ldt, rgnn_stream_t stream);

/* ================================================================ batches of graphs resident in HBM
 * Device-side replacement of torch_geometric's DataLoader collation (utils/data_handling.py:30 -> Batch.from_data_list)
 * and of the per-batch host-to-device copy (postprocessor/inference.py:57): the processed dataset lives in HBM as
 * concatenated tensors, a batch is a list of n_seg graph ids.  All offset tables are int64 on the device:
 *   seg_src_row[s]  first row (node or edge) of selected graph s in the resident tensor,
 *   seg_dst_ptr[s]  first row of graph s in the batch, seg_dst_ptr[n_seg] = n_rows (non-decreasing; empty graphs allowed).
 * rgnn_collate_rows copies rows of `width` 4-byte words (x, edge_attr, y, pos, vel) and, when batch_out != NULL, writes
 * PyG's `batch` vector (graph slot of every row).  rgnn_collate_edges copies both rows of the int64 edge_index [2, E]
 * (row stride ld) and adds seg_node_shift[s] = first batch row of graph s (PyG: `edge_index += cumulative num_nodes`). */
int rgnn_collate_rows(const void* src, int64_t ld_src, int32_t width, const int64_t* seg_src_row, const int64_t* seg_dst_ptr,
                      int32_t n_seg, int64_t n_rows, void* out, int64_t ld_out, int64_t* batch_out, rgnn_stream_t stream);
int rgnn_collate_edges(const int64_t* src_edge_index, int64_t ld_src, const int64_t* seg_src_edge,
                       const int64_t* seg_dst_eptr, const int64_t* seg_node_shift, int32_t n_seg, int64_t n_edges,
                       int64_t* out, int64_t ld_out, rgnn_stream_t stream);

/* Host side of a STREAMED batch (no device work, no stream; the reference collates on the host: utils/data_handling.py:30 DataLoader
 * -> Batch.from_data_list, then `data.to(device)`, postprocessor/inference.py:57).  The float64 point arrays of n_frames frames, wherever
 * they lie in host memory, are laid back to back into ONE block, so that a batch goes up in one copy:
 *   block = X [n, 2] | V [n, 2] | rcs [n] | timestamp [n] | frame_ptr [n_frames + 1] (int64),   n = sum n_points,
 *   byte offsets 0, 16 n, 32 n, 40 n, 48 n;  block_bytes >= 48 n + 8 (n_frames + 1)  (RGNN_INVALID_ARGUMENT otherwise).
 * addr: [n_frames][4] host pointers {X, V, rcs, timestamp} of contiguous float64 arrays ([n_f, 2], [n_f, 2], [n_f], [n_f]).
 * Meant to be called WITHOUT the interpreter lock from a loader thread (ctypes releases it). */
int rgnn_stage_frames(int64_t n_frames, const void* const* addr, const int64_t* n_points, void* block, int64_t block_bytes);

/* ================================================================ post-processor front half
 * Per node of one graph / batch: predicted label (first index of the row maximum of class_prob [n, n_classes]), its
 * score, the keep flag of PredictionExtractor.get_absolute_object_bounding_box_predictions
 * (postprocessor/postprocessing.py:198-319: removed when class_prob[:, bg_index] >= max_score_for_background, when the
 * label is bg_index, or when score <= min_object_score[label] for label < n_min_scores) and the four corners
 * (c1x, c1y, ..., c4x, c4y; float64) of the absolute box decoded from boxes [n, 4] (relative aligned) or [n, 5]
 * (invariance 0: absolute rotated, 1: relative rotated, 2: E(n)-invariant, which needs nn_index = nearest other point of
 * every node, rgnn_knn_graph with k = 1); box algebra of preprocessor/bounding_box.py.  pos: float32 [n, 2] contiguous.
 * adapt_orientation_angle: the angle was trained as sin(theta shifted to [-pi/2, pi/2]) (bounding_box.py:566-589). */
int rgnn_decode_predictions(const float* class_prob, int64_t ldp, int32_t n_classes, const float* boxes, int64_t ldb,
                            int32_t box_width, const float* pos, const int32_t* nn_index, int64_t n, int32_t bg_index,
                            float max_score_for_background, const double* min_object_score, int32_t n_min_scores,
                            int32_t invariance, int32_t adapt_orientation_angle, int32_t* label, float* score,
                            int32_t* keep, double* corners, rgnn_stream_t stream);

/* Non-maximum suppression of one graph's boxes (BoxSuppressor.apply_nms, postprocessor/postprocessing.py:336-431).
 * kind 0: aligned boxes [x_min, y_min, x_max, y_max] float32 [m, 4], torchvision.ops.nms semantics (suppress IoU > t);
 * kind 1: rotated boxes [x, y, l, w, theta in degrees] float64 [m, 5], detectron2 nms_rotated semantics (IoU >= t).
 * order: int64 [m] box ids by descending score (stable); mask_tmp: rgnn_nms_mask_words(m) 64-bit words of workspace;
 * keep: int64 [m] receives the ids kept, by descending score; count: their number (device). */
/* Box ids by descending score, ties by ascending id (a stable descending sort; NaN first): the order rgnn_nms wants -- what
 * torchvision.ops.nms / detectron2 nms_rotated compute with a library sort before their suppression pass
 * (postprocessor/postprocessing.py:336-435).  scores: [dev] float32 or float64 [m]; order: [dev] int64 [m];
 * tmp: [dev] rgnn_sort_scores_tmp_bytes(m) bytes. */
int64_t rgnn_sort_scores_tmp_bytes(int64_t m);
int rgnn_sort_scores(const void* scores, int32_t is_f64, int64_t m, int64_t* order, void* tmp, rgnn_stream_t stream);
int64_t rgnn_nms_mask_words(int64_t m);
/* corners float64 [m, 4, 2] -> two_point float64 [m, 4] ([x_min, y_min, x_max, y_max]) and / or rotated float64 [m, 5]
 * ([x, y, l, w, theta in degrees, 0..180]); BoundingBox.get_two_point_representations /
 * get_absolute_rotated_box_representations, preprocessor/bounding_box.py:447-540.  Either output may be NULL. */
int rgnn_box_representations(const double* corners, int64_t m, double* two_point, double* rotated, rgnn_stream_t stream);
int rgnn_nms(const void* boxes, int32_t kind, const int64_t* order, int64_t m, double iou_threshold, uint64_t* mask_tmp,
             int64_t* keep, int64_t* count, rgnn_stream_t stream);
/* Segmented suppression: for every frame of a batch what nonzero(keep) -> rgnn_box_representations -> the reference's shift
 * of negative coordinates (postprocessing.py:358-361, 391-394; the frame's OWN minimum) -> rgnn_sort_scores -> rgnn_nms compute
 * for that frame alone, bit for bit, in two launches whatever n_frames is.  label / score / keep / corners: the outputs of
 * rgnn_decode_predictions for all n nodes; frame_ptr: [dev] int64 [n_frames + 1] node offsets.  kind as in rgnn_nms: 0 aligned
 * (scores_out float32 [n], corners_out float32 [n, 4, 2] rebuilt from the float32 two-point matrix minus the float32 shift, corner
 * order (x0,y0) (x0,y1) (x1,y0) (x1,y1)), 1 rotated (scores_out float64 [n], corners_out float64 [n, 4, 2] copied from corners).
 * node: int64 [n] node ids kept, frame after frame, in suppression order; labels_out: float64 [n]; only the first
 * meta[n_frames] entries of the four outputs are written.  meta: [dev] int64 [2 n_frames + 1] = offsets of the frames' kept boxes
 * [n_frames + 1] | candidates (keep != 0) per frame [n_frames].  A frame of more than rgnn_nms_frames_max_candidates()
 * candidates is left empty: the caller sees its count in meta and runs it through rgnn_nms.
 * tmp: [dev] rgnn_nms_frames_tmp_bytes(n, n_frames) bytes. */
int64_t rgnn_nms_frames_max_candidates(void);
int64_t rgnn_nms_frames_tmp_bytes(int64_t n, int64_t n_frames);
int rgnn_nms_frames(const int32_t* label, const float* score, const int32_t* keep, const double* corners,
                    const int64_t* frame_ptr, int64_t n, int64_t n_frames, int32_t kind, double iou_threshold, void* tmp,
                    int64_t* node, double* labels_out, void* scores_out, void* corners_out, int64_t* meta, rgnn_stream_t stream);

/* ================================================================ evaluation: ground truth and point IoU
 * Ground-truth boxes of one graph / batch (GroundTruthExtractor.get_absolute_object_bounding_boxes,
 * postprocessor/postprocessing.py:447-551): keep = (labels[i * ldl] != bg_index) (float32 labels, NaN kept) and the four
 * corners of every node's absolute box, the box algebra of rgnn_decode_predictions without the angle adaption.
 * keep: [dev] int32 [n]; corners: [dev] float64 [n, 4, 2]. */
int rgnn_decode_ground_truth(const float* labels, int64_t ldl, const float* boxes, int64_t ldb, int32_t box_width,
                             const float* pos, const int32_t* nn_index, int64_t n, int32_t bg_index, int32_t invariance,
                             int32_t* keep, double* corners, rgnn_stream_t stream);
/* Duplicate ground-truth boxes (GroundTruthExtractor.remove_duplicate_boxes, postprocessing.py:552-575): box j of a frame
 * is dropped iff some box i < j of the same frame (dropped or not) has all 8 corners == or a float64 sum of the 8 absolute
 * differences (numpy's pairwise order) < 0.1.  corners: [dev] float64 [m, 4, 2]; box_ptr: [dev] int64 [n_frames + 1] box
 * offsets of the frames; keep: [dev] int32 [m], 1 = kept. */
int rgnn_remove_duplicate_boxes(const double* corners, const int64_t* box_ptr, int64_t n_frames, int64_t m, int32_t* keep,
                                rgnn_stream_t stream);
/* Point IoU matrices of a batch of frames (point_iou, utils/math.py:176-211): for frame f, iou[out_ptr[f] + p * G_f + g]
 * (float64, row-major [P_f, G_f]) of predicted box p and ground-truth box g: tp = distinct (x, y) coordinates inside both,
 * fp / fn = points inside one box minus tp, tp / (tp + fp + fn) or 0.00001 when that is 0.  Boxes float32: aligned
 * [x_min, y_min, x_max, y_max] (rotated = 0) or [x, y, l, w, theta in degrees] (rotated = 1, is_point_in_rect's area test
 * in float64); pred_ptr / gt_ptr / frame_ptr / out_ptr: [dev] int64 [n_frames + 1] offsets of the boxes, of the points
 * (float32 [N, 2]) and of the matrices (n_out = out_ptr[n_frames]); max_frame_points: the largest frame, at most 8192;
 * tmp: [dev] rgnn_point_iou_tmp_bytes(n_frames, ceil(max_frame_points / 64), n_pred, n_gt) bytes. */
int64_t rgnn_point_iou_tmp_bytes(int64_t n_frames, int32_t words, int64_t n_pred, int64_t n_gt);
int rgnn_point_iou(const float* boxes_pred, const int64_t* pred_ptr, int64_t n_pred, const float* boxes_gt, const int64_t* gt_ptr,
                   int64_t n_gt, int32_t rotated, const float* points, const int64_t* frame_ptr, int64_t n_frames,
                   int32_t max_frame_points, const int64_t* out_ptr, int64_t n_out, double* iou, void* tmp, rgnn_stream_t stream);

/* ---------------------------------------------------------------- evaluation metrics (csrc/metrics.hip)
 * What the reference's evaluators compute after the post-processor (postprocessor/metrics.py:12-196 on
 * postprocessor/torchmetrics_mean_ap.py:410-1030), packed over all frames by the offset arrays of rgnn_point_iou: no entry
 * point here launches per frame or per class.  Only the area range "all" exists (nothing is ever "ignored").
 *
 * Aligned box IoU (compute_iou with use_point_iou = False, torchmetrics_mean_ap.py:114: torchvision.ops.box_iou): for frame f,
 * iou[out_ptr[f] + p * G_f + g] (float32) of [x_min, y_min, x_max, y_max] float32 boxes,
 * inter / (area_p + area_g - inter) with inter = clamp(min(x2) - max(x1), 0) * clamp(min(y2) - max(y1), 0), all float32, no
 * fused multiply-add.  A restatement of torchvision's documented formula, NOT pinned by an executed torchvision. */
int rgnn_box_iou(const float* boxes_pred, const int64_t* pred_ptr, const float* boxes_gt, const int64_t* gt_ptr, int64_t n_frames,
                 const int64_t* out_ptr, int64_t n_out, float* iou, rgnn_stream_t stream);
/* Greedy matching (_compute_iou, _evaluate_image, _find_best_gt_match, torchmetrics_mean_ap.py:505-551, 612-747), one wave per
 * (frame, class of `classes`).  iou: the packed matrices, float64 (iou_is_f32 = 0, rgnn_point_iou) or float32 (1, rgnn_box_iou).
 * The class's detections of the frame by descending score (ties: ascending position -- the reference's torch.sort leaves ties
 * unpinned; NaN first), cut to max_det; for every threshold, in that order: the maximum over the class's ground-truth boxes of
 * (0 if already matched, else the IoU), lowest position on ties; matched iff it is strictly greater than the threshold (float64
 * comparison; for float32 IoUs the threshold is rounded to float32 first).  rank: [dev] int32 [n_pred], the detection's rank in
 * its (frame, class) list or -1 beyond max_det; matched: [dev] uint8 [n_thresholds, n_pred].  Both are cleared here.
 * Capacity: rgnn_map_match_capacity() (2048) detections and as many ground-truth boxes of ONE class in one frame.  The lists
 * are counted on the device: a longer one sets bit 0 of *status ([dev] int32, cleared here) and that (frame, class) pair is
 * left unmatched with rank -1; the caller reads the word and refuses the result. */
int32_t rgnn_map_match_capacity(void);
int rgnn_map_match(const void* iou, int32_t iou_is_f32, const int64_t* pred_ptr, const int64_t* gt_ptr, const int64_t* out_ptr,
                   int64_t n_frames, const int32_t* det_labels, const float* det_scores,
                   int64_t n_pred, const int32_t* gt_labels, const int32_t* classes, int32_t n_classes, const double* thresholds,
                   int32_t n_thresholds, int32_t max_det, int32_t* rank, uint8_t* matched, int32_t* status, rgnn_stream_t stream);
/* Recall / precision / score tables (__calculate_recall_precision_scores, torchmetrics_mean_ap.py:898-973), one work-group per
 * (class, threshold, max_det).  order: [dev] int64 [n_pred], the detections class by class in the order of `classes`, inside a
 * class by descending score, stable (two passes of rgnn_sort_scores); cls_ptr: [dev] int64 [2, n_classes], where each class
 * begins and ends in `order` (a work-group reads its own class's segment only);
 * rank / matched: from rgnn_map_match; max_dets: [dev] int32 [n_max_dets]; rec: [dev] float32 [n_rec] ascending recall
 * thresholds (at most 1024).  Per curve: the class's detections with rank < max_det in that order, tp / fp running counts as
 * float32, rc = tp / npig, pr = tp / (fp + tp + 2.220446049250313e-16) (IEEE division), pr made non-increasing by the running
 * maximum from the right, and per recall threshold r the first index with rc >= r.
 * precision, scores: [dev] float32 [n_thresholds, n_rec, n_classes, n_max_dets]; recall: [dev] float32 [n_thresholds, n_classes,
 * n_max_dets]; every entry is written: -1 for a class without ground truth, else the value or 0. */
int rgnn_map_curves(const int64_t* order, const int64_t* cls_ptr, const int32_t* det_labels, const float* det_scores, const int32_t* rank,
                    const uint8_t* matched, int64_t n_pred, const int32_t* gt_labels, int64_t n_gt, const int32_t* classes,
                    int32_t n_classes, int32_t n_thresholds, const int32_t* max_dets, int32_t n_max_dets, const float* rec,
                    int32_t n_rec, float* precision, float* scores, float* recall, rgnn_stream_t stream);
/* Confusion matrix of the node labels (SegmentationMetrics, metrics.py:136-196: sklearn's confusion_matrix with
 * labels = range(n_classes)): matrix [dev] int64 [n_classes, n_classes], rows = true label, columns = predicted label, cleared
 * here.  y_true / y_pred: [dev] float64 [n], truncated towards zero (astype(int)); a node with a label outside
 * 0 .. n_classes - 1 is left out; a NaN label sets bit 0 of *status ([dev] int32, cleared here).  At most 64 classes. */
int rgnn_confusion_matrix(const double* y_true, const double* y_pred, int64_t n, int32_t n_classes, int64_t* matrix,
                          int32_t* status, rgnn_stream_t stream);

/* ================================================================ backward pass (training: gnn/trainer.py:176-231)
 * What autograd derives for the reference's op-by-op forward, for the fused forward kernels above.  The dense-layer
 * gradients are GEMMs: dX = dY W runs on rgnn_linear_fwd with the transposed weight, dW = dY^T X on rgnn_wgrad
 * (csrc/wgrad.hip: split-K MFMA kernel of this library; no BLAS anywhere in the product since r02). */

/* ReLU fused into a dense-layer epilogue: dx = (y > 0) ? dy : 0 over `count` contiguous floats (16-byte aligned). */
int rgnn_relu_bwd(const float* dy, const float* y, float* dx, int64_t count, rgnn_stream_t stream);

/* Train-mode BatchNorm1d backward, reduction half: per 128-row panel the column sums of g and g*h, where
 * g = dy (no ReLU: y == NULL and table == NULL) or dy masked by the fused ReLU that followed, and h = the BatchNorm input.  The
 * mask is y > 0 (y = the ReLU's output) or, with table ([RGNN_AFFINE_ROWS, n] of rgnn_batchnorm_finalize, the forward pass's apply
 * table), recomputed as fmaf(h - mean_hi, g, t) > 0 -- the bits of y as rgnn_scale_shift_act (or the A-operand path of
 * rgnn_linear_fwd) produced them; a quarter to a third fewer bytes per pass.
 * partial: float [panels, 2, n], panels = rgnn_linear_stat_panels(m). */
int rgnn_bn_bwd_stats(const float* dy, int64_t lddy, const float* y /*or NULL*/, int64_t ldy, const float* table /*or NULL*/,
                      const float* h, int64_t ldh, int64_t m, int32_t n, float* partial, rgnn_stream_t stream);
/* ... elementwise half: dx = A[c] g + B[c] h + C[c], coef = [A | B | C] (3 n floats) with
 * A = gamma rstd, B = -gamma rstd^2 S/m, C = -gamma rstd sum(g)/m + gamma rstd^2 mean S/m, S = sum g xhat; y / table as above.
 * dx_absmax (a bound, RGNN_BOUND_SLOTS words zeroed by the caller; NULL = not wanted) is raised to max |dx|: the dgrad launches
 * that read dx then take the f16x2 form. */
int rgnn_bn_bwd_apply(const float* dy, int64_t lddy, const float* y /*or NULL*/, int64_t ldy, const float* table /*or NULL*/,
                      const float* h, int64_t ldh, const float* coef, int64_t m, int32_t n, float* dx, int64_t lddx,
                      float* dx_absmax /*or NULL*/, rgnn_stream_t stream);
/* The [3, n] coefficients of rgnn_bn_bwd_apply plus d gamma / d beta in one launch (float64 inside): from the forward column
 * statistics of the layer input (fwd_stats [panels_f, RGNN_STAT_ROWS, n], use_batch = 1) or the running statistics (use_batch = 0) and the
 * partial sums of rgnn_bn_bwd_stats (bwd_part [panels_b, 2, n]).  dgamma / dbeta may be NULL. */
int rgnn_bn_bwd_coef(const float* fwd_stats, int64_t panels_f, const float* running_mean, const float* running_var,
                     const float* bwd_part, int64_t panels_b, int64_t m, int32_t n, const float* gamma, float eps,
                     int32_t use_batch, float* coef, float* dgamma, float* dbeta, rgnn_stream_t stream);
/* Backward of the segment-scoped BatchNorm (rgnn_batchnorm_segments / rgnn_batchnorm_act_segments): segment s = rows
 * [seg_ptr[s], seg_ptr[s + 1]) of m_s rows has its own statistics, so with g = dy (y == NULL) or dy masked by y > 0 (y = the saved
 * output behind the fused ReLU) and xhat = (h - mu_s) r_s:
 *     dx = gamma r_s (g - S1 / m_s - xhat S2 / m_s),  S1 = sum_rows g,  S2 = sum_rows g xhat,  dgamma = sum_s S2,  dbeta = sum_s S1.
 * seg_stats: the forward's seg_sums as those entry points LEAVE it, double [n_seg, 2, n] = {mean, unbiased variance} per
 * (segment, column) -- exact statistics, never the fp32 apply table divided by gamma.  A segment without rows contributes
 * nothing; a segment of one row gets dx = 0 exactly, adds its g to dbeta and nothing to dgamma.  Rows outside every segment are
 * not written.  seg_ptr is read on the device and every row range is clamped to [0, m].
 * Workspace: seg_bsums, double [n_seg, 2, n] (S1, S2 per segment and column; written, then summed in segment order).
 * Two launches: one block per (segment, 64-column slab) sums the slab, finishes its coefficients in float64 and writes dx (16-byte
 * accesses when n and every row stride are multiples of 4 floats and the pointers 16-byte aligned; any width, stride and alignment
 * otherwise); a thread per column adds dgamma / dbeta over the segments (skipped when both are NULL).  Deterministic: fixed
 * summation order, no floating-point atomics.  dx_absmax: as in rgnn_bn_bwd_apply. */
int rgnn_bn_segments_bwd(const float* dy, int64_t lddy, const float* y /*or NULL*/, int64_t ldy, const float* h, int64_t ldh,
                         const int64_t* seg_ptr /*[dev] n_seg + 1*/, int64_t n_seg, int64_t m, int32_t n,
                         const double* seg_stats, const float* gamma /*or NULL*/, float eps, double* seg_bsums, float* dx,
                         int64_t lddx, float* dgamma /*or NULL*/, float* dbeta /*or NULL*/, float* dx_absmax /*or NULL*/,
                         rgnn_stream_t stream);

/* Backward of rgnn_segment_reduce: d_rows [E, d] (every row is written; rows of the forward input are needed for the
 * arg-max: the first row of a segment attaining the maximum receives dM[t, c]; mean / add: every row, / deg; min: the first row
 * attaining the minimum; var: dM 2 (row - mean) / cnt; std: dM (row - mean) / (cnt std) where var > 0, else 0). */
int rgnn_segment_reduce_bwd(const float* dM, int64_t lddm, const float* rows, int64_t ldr, const int32_t* rowptr_t,
                            const int32_t* node_order, int64_t n, int32_t d, int32_t aggr, float* d_rows, int64_t lddr,
                            rgnn_stream_t stream);

/* The same backward for max aggregation on the shipped shapes (d % 8 == 0, d <= 512, 1 <= de <= 8, in-degrees < 65 536), with
 * the edge half as two kernels that keep their reductions inside a lane (dW_e: lanes = channels; d_edge_attr: lanes = edges
 * scanning their target's arg row).  Per sorted edge e: tgt_sorted[e] its target node, eloc_sorted[e] its index inside the
 * target's segment; per out-edge j of the source CSR: tloc[j] = eloc_sorted[tpos[j]].  arg: uint16 [n, d], the index (inside
 * the segment) of the edge that won channel c of target t -- recorded by the forward pass (arg_is_valid = 1) or recomputed
 * here from Q / W_e / the attributes (0).  dwe_partial: float [rgnn_mpnn_bwd_slots(n), d, de].  dq_absmax (a bound; NULL = not
 * wanted) is raised to max |dQ|. */
int32_t rgnn_mpnn_max_bwd_supported(int32_t d, int32_t de);
int rgnn_mpnn_max_bwd(const float* dM, int64_t lddm, const float* Q, int64_t ldq, const float* We, int64_t ldwe,
                      const float* edge_attr_sorted, int32_t de, const int32_t* rowptr_t, const int32_t* src_sorted,
                      const int32_t* tgt_sorted, const int32_t* eloc_sorted, const int32_t* node_order, int64_t n, int32_t d,
                      const int32_t* rowptr_s, const int32_t* tnode, const int32_t* tloc, int64_t n_edges, uint16_t* arg,
                      int32_t arg_is_valid, float* dwe_partial, float* dQ, int64_t lddq, float* d_edge_attr, float* dWe,
                      float* dq_absmax /*or NULL*/, rgnn_stream_t stream);

/* Weight gradient of a dense layer: dW[n, k] = sum_m G[m, n] * [A1 | A2][m, k] (G = gradient of the layer output after
 * the activation mask, A = the layer input), fp32 MFMA, reduction over the rows split into
 * rgnn_linear_wgrad_slabs(m, n, k1 + k2) slabs whose partial tiles go to `partial` (float [slabs, n, k1 + k2]) and are
 * summed into dW [n, k1 + k2] (row-major, contiguous) by a second kernel: no atomics, deterministic.
 * Widths and row strides must be multiples of 4 floats, pointers 16-byte aligned. */
int32_t rgnn_linear_wgrad_slabs(int64_t m, int32_t n, int32_t k);
int rgnn_linear_wgrad(const float* G, int64_t ldg, const float* A1, int64_t lda1, int32_t k1, const float* A2, int64_t lda2,
                      int32_t k2, int64_t m, int32_t n, float* partial, float* dW, rgnn_stream_t stream);

/* The same gradient on the bf16 matrix pipe (three-term split of both operands, six MFMA products per fp32 product, fp32
 * accumulate: the forward kernels' arithmetic), for any widths and row strides:
 *   dW[n, k] = sum_r G[row(r), n] * [A1 | A2 | 1][row(r), k],   row(r) = row_index ? row_index[r] : r,  r < (m_dev ? *m_dev : m)
 * with_ones appends a column of ones to the input, so dW[:, k1 + k2] is the bias gradient (column sums of G over the same
 * rows).  partial: float [rgnn_wgrad_slabs(m, n, k1, k2, with_ones), n, k1 + k2 + with_ones]; dW [n, k1 + k2 + with_ones]
 * row-major.  Deterministic (slab partials summed by a second kernel, no atomics).  m = 0: dW is zeroed (the sum over nothing;
 * G / A may be NULL then).
 * The f16x2 form when every operand block comes with a bound (g_bound, a1_bound if k1 > 0, a2_bound if k2 > 0: arrays of
 * RGNN_BOUND_SLOTS floats bounding |G| / |A1| / |A2| over the rows read): both operands pre-scaled by exact powers of two, split into
 * two f16 terms, three MFMA products (l h', h l', h h') -- the forward kernels' f16x2 arithmetic; the column of ones is carried as
 * 2^14 after the pre-scale.  Any bound NULL: the bf16x3 form. */
int32_t rgnn_wgrad_slabs(int64_t m, int32_t n, int32_t k1, int32_t k2, int32_t with_ones);
int rgnn_wgrad(const float* G, int64_t ldg, int32_t n, const float* A1, int64_t lda1, int32_t k1, const float* A2, int64_t lda2,
               int32_t k2, int32_t with_ones, int64_t m, const int32_t* row_index /*[dev] or NULL*/,
               const int64_t* m_dev /*[dev] or NULL*/, const float* g_bound /*or NULL*/, const float* a1_bound /*or NULL*/,
               const float* a2_bound /*or NULL*/, float* partial, float* dW, rgnn_stream_t stream);

/* Backward of rgnn_mpnn_aggregate without its target term: M[t] = aggr_{e -> t}(Q[s_e] + W_e a_e) (0 for empty
 * segments).  max: the gradient of (t, c) goes to the first edge attaining the maximum (torch-scatter arg_out).
 * Two kernels, no atomics on the node gradient:
 *   edge half  -- over the CSR by target (same rowptr_t / src_sorted / node_order as the forward): d_edge_attr [E, de]
 *                 and dWe [d, de] (both written), and for max the winning edge
 *                 position per (t, c) in arg_tmp int32 [n, d];
 *   node half  -- over the CSR by SOURCE of the same edges (rowptr_s [n+1], segments in the same node_order;
 *                 tnode[j] = target of out-edge j, tpos[j] = position of that edge in the target-sorted list):
 *                 dQ [n, d] is written for every node.
 * target_scale: float [n], 1 / in-degree (mean only, else NULL).  dwe_partial: float [rgnn_mpnn_bwd_slots(n), d, de]
 * workspace (every persistent wave group stores its share of dW_e, a last kernel sums them into dWe: no atomics).
 * min (3): as max with the comparison turned round (arg_tmp int32 [n, d]: the first edge attaining the minimum).
 * var (4) / std (5): every edge receives g_e = A[t] (m_e - mean[t]), A = dM 2 / cnt (var) or dM 1[var > 0] / (cnt std) (std), m_e
 * recomputed from Q[s_e] + W_e a_e; d_edge_attr_e = W_e^T g_e, dWe = sum g_e a_e^T, dQ[s] = sum over the out-edges of s of g_e in
 * fixed order.  For these two codes arg_tmp is a FLOAT workspace of 2 n d words (16-byte aligned for the vector form): a pre-pass
 * writes A into its first half and mean into its second; target_scale is not read. */
int64_t rgnn_mpnn_bwd_slots(int64_t n);
/* waves per segment of the edge half (1, 2 or 4); dea_partial: float [split, E, de] workspace when split > 1 */
int32_t rgnn_mpnn_bwd_split(int32_t d);
int rgnn_mpnn_aggregate_bwd(const float* dM, int64_t lddm, const float* Q, int64_t ldq, const float* We, int64_t ldwe,
                            const float* edge_attr_sorted, int32_t de, const int32_t* rowptr_t, const int32_t* src_sorted,
                            const int32_t* node_order, int64_t n, int32_t d, int32_t aggr, const int32_t* rowptr_s,
                            const int32_t* tnode, const int32_t* tpos, const float* target_scale, int64_t n_edges,
                            int32_t* arg_tmp, float* dwe_partial, float* dea_partial, float* dQ, int64_t lddq,
                            float* d_edge_attr, float* dWe, rgnn_stream_t stream);

/* ================================================================ detection loss (training: gnn/trainer.py:181-222)
 * loss = cls_loss_weight * CrossEntropyLoss(weight = class_weight)(cls, label) + bb_loss_weight * mean over the nodes
 * with label != bg_index of HuberLoss(delta)(y[:, 1:], boxes) -- the reference's per-node Python loop (trainer.py:193-201)
 * as one pass.  y: float32 [n, 1 + box_width] (label | box), class_weight: float32 [n_classes] or NULL.
 * partial_tmp: 4 * rgnn_detection_loss_blocks(n) doubles; sums: 4 doubles (sum w nll, sum w, sum huber, number of object
 * nodes; kept for the backward pass); loss_out: 3 floats (loss, loss_cls, loss_bb).  A batch without objects or with a NaN
 * box term contributes loss_bb = 0 (trainer.py:203-217).  _bwd writes d loss / d cls and d loss / d boxes scaled by
 * grad_loss[0] (NULL: 1). */
int64_t rgnn_detection_loss_blocks(int64_t n);
int rgnn_detection_loss(const float* cls, int64_t ldc, int32_t n_classes, const float* boxes, int64_t ldb, int32_t box_width,
                        const float* y, int64_t ldy, const float* class_weight, int64_t n, int32_t bg_index, float delta,
                        float cls_loss_weight, float bb_loss_weight, double* partial_tmp, double* sums, float* loss_out,
                        rgnn_stream_t stream);
int rgnn_detection_loss_bwd(const float* cls, int64_t ldc, int32_t n_classes, const float* boxes, int64_t ldb,
                            int32_t box_width, const float* y, int64_t ldy, const float* class_weight, int64_t n,
                            int32_t bg_index, float delta, float cls_loss_weight, float bb_loss_weight, const double* sums,
                            const float* grad_loss, float* d_cls, int64_t lddc, float* d_boxes, int64_t lddb,
                            rgnn_stream_t stream);
/* The same loss with one result per group of rows -- group g = rows [group_ptr[g], group_ptr[g + 1]), group_ptr int64
 * [n_groups + 1] on the device, every range clamped to [0, n] -- for steps that run several loader batches through one forward:
 * the reference's loss is a per-loader-batch quantity.  sums: double [n_groups, 4], loss_out: float [n_groups, 3], per group as
 * above (the weighted mean over the group's nodes; loss_bb = 0 for a group without object nodes or with a NaN Huber sum; an
 * empty group has loss_cls = NaN like an empty batch).  One launch, no workspace.
 * _bwd: d (sum_g coef[g] loss_g) / d cls and / d boxes, coef float [n_groups] on the device (NULL: all ones); rows outside every
 * group get zeros.  Deterministic, no atomics. */
int rgnn_detection_loss_segments(const float* cls, int64_t ldc, int32_t n_classes, const float* boxes, int64_t ldb,
                                 int32_t box_width, const float* y, int64_t ldy, const float* class_weight, int64_t n,
                                 const int64_t* group_ptr, int64_t n_groups, int32_t bg_index, float delta, float cls_loss_weight,
                                 float bb_loss_weight, double* sums, float* loss_out, rgnn_stream_t stream);
int rgnn_detection_loss_segments_bwd(const float* cls, int64_t ldc, int32_t n_classes, const float* boxes, int64_t ldb,
                                     int32_t box_width, const float* y, int64_t ldy, const float* class_weight, int64_t n,
                                     const int64_t* group_ptr, int64_t n_groups, int32_t bg_index, float delta,
                                     float cls_loss_weight, float bb_loss_weight, const double* sums, const float* coef,
                                     float* d_cls, int64_t lddc, float* d_boxes, int64_t lddb, rgnn_stream_t stream);

/* ================================================================ ground-truth box targets (csrc/groundtruth.hip)
 * GroundTruthCreator.create_2D_bounding_boxes (preprocessor/radarscenes/dataset_creation.py:232-521): the box columns of `y`, the
 * inverse of rgnn_decode_ground_truth.  The objects of the whole batch come in CSR form: object o owns the point rows
 * obj_rows[obj_ptr[o] .. obj_ptr[o + 1]) (int32 [n_rows], ascending inside an object: "p1" of a two-point object is the lower
 * row); pos: float64 [n, 2].  Per object: aligned != 0: the min / max box of its points (utils/math.py:284-299); otherwise the
 * minimum-area rectangle flush with an edge of the convex hull (utils/math.py:304-439; 1 point: a 0.5 x 0.5 box at the point,
 * 2 points: midpoint, their distance x 0.5 along p2 - p1).  Per point of the object, out[row] (float64, [n, 4] aligned or [n, 5]):
 *   aligned                 [x_c - x, y_c - y, dx, dy]
 *   invariance 0 none       [x_c, y_c, l, w, theta]            (theta of the long side in rad, [0, pi))
 *   invariance 1 translation[x_c - x, y_c - y, l, w, theta]
 *   invariance 2 en         [d, angle(nn -> centre), l, w, angle(nn -> long side)]  (bounding_box.py:205-272; nn_index int32 [n]: the
 *                           nearest other point of every point's frame, rgnn_knn_graph with k = 1; may be NULL otherwise)
 * Rows of points that belong to no object are NOT written: the caller pre-fills out (and rect) with NaN.
 * rect (optional): float64 [n_obj, 5], the object's absolute rectangle [x_c, y_c, l, w, theta in degrees, 0 <= theta < 180]
 * (aligned: [x_c, y_c, dx, dy, 0]).
 * An object of more than rgnn_gt_object_cap() (1024) points, a degenerate one (see the status bits), or one whose offsets / rows
 * point outside the arrays is left unwritten and raises its bit in *status; all other objects are written as usual.
 * One launch (one wave per object), no synchronisation; the result does not depend on scheduling. */
int32_t rgnn_gt_object_cap(void);
int rgnn_create_gt_boxes(const double* pos, int64_t n, const int64_t* obj_ptr, const int32_t* obj_rows, int64_t n_rows,
                         int64_t n_obj, const int32_t* nn_index /*[dev] or NULL*/, int32_t aligned, int32_t invariance,
                         double* out, double* rect /*[dev] or NULL*/, int32_t* status /*[dev]*/, rgnn_stream_t stream);

/* ================================================================ clustering (csrc/cluster.hip)
 * DBSCAN labels of every frame of a batch over the rows of the radius search -- what sklearn.cluster.DBSCAN(eps, min_samples,
 * algorithm="kd_tree").fit(points of the frame) returns in labels_ and core_sample_indices_, entry for entry, when rowptr / col are
 * the rows of rgnn_radius_graph_rows at r = eps.  No reference counterpart (the RadarScenes baselines cluster on the host).
 * Inputs ([dev]): rowptr int32 [n + 1], col int32 [n_edges] (global row ids; the search writes them ascending per row, the kernel does
 * not rely on the order), frame_ptr int64 [n_frames + 1] (frame f = rows [frame_ptr[f], frame_ptr[f + 1])), group int32 [n] or NULL.
 * The rule, per frame, without any tolerance:
 *   neighbourhood  S_i = the entries j of row i with j != i, j in i's frame and group[j] == group[i]; a point with group < 0 takes no
 *                  part (label -1, not core, nobody's neighbour).  NULL: one group per frame.
 *   core           |S_i| + 1 >= min_samples (min_samples counts the point itself, as in scikit-learn).
 *   cluster        a connected component of the core points under the edges between two core points (an entry (i, j) joins i and j,
 *                  whether or not row j lists i); its root is its smallest row.
 *   numbering      the clusters of a frame are numbered 0, 1, ... by ascending root, across groups; every frame starts at 0.
 *   labels         core: the cluster's number; not core with a core neighbour: the smallest number among its core neighbours; else -1.
 * Outputs ([dev]): labels int32 [n], core uint8 [n] (0 / 1), n_clusters int32 [n_frames]; *status gets the bits below (the caller
 * zeroes it).  One launch, one work-group per frame, the frame's union-find array in LDS (4 bytes per point, 96 KB): a frame of more
 * than rgnn_dbscan_max_frame_points() (24 576) points raises RGNN_STATUS_DBSCAN_FRAME_TOO_LARGE, its rows get label -1 and core 0
 * and its n_clusters 0; the other frames are written as usual.  There is no path through global memory for larger frames: no
 * work-group ever reads what another wrote in the same launch.  An entry of col outside its row's frame is skipped, a row whose
 * offsets leave [0, n_edges] counts as empty, a frame outside [0, n] is left unwritten (n_clusters 0); each raises
 * RGNN_STATUS_DBSCAN_BAD_ROW and is never used as an index.  Every loop is bounded by the frame's size or a row's length; convergence
 * is never decided on the host.  The result is a function of the inputs alone (no floating-point work, no order-dependent atomics). */
int32_t rgnn_dbscan_max_frame_points(void);
int rgnn_dbscan_labels(const int32_t* rowptr, const int32_t* col, int64_t n, int64_t n_edges, const int64_t* frame_ptr,
                       int64_t n_frames, int32_t min_samples, const int32_t* group /*[dev] or NULL*/, int32_t* labels, uint8_t* core,
                       int32_t* n_clusters, int32_t* status /*[dev]*/, rgnn_stream_t stream);

/* Class scores of clusters: cluster o owns the point rows obj_rows[obj_ptr[o] .. obj_ptr[o + 1]) (the CSR of the Python layer's
 * group_objects; int64 [n_obj + 1], int32 [n_rows]); prob: float32 [n, n_classes] with row stride ldp.  mean[o, k] (float64
 * [n_obj, n_classes]) = the mean of prob[row, k] over the members, summed in float64 in a fixed order (one wave per cluster: lane l
 * adds the members l, l + 64, ... in that order, then a xor butterfly over the lanes), so the same input gives the same bits.
 * per_class != 0: cls[o] = group[first member] (group int32 [n], required), score[o] = mean[o, cls[o]] (NaN if that is no column).
 * per_class == 0: cls[o] = the k != bg_index with the largest mean, the lowest k on ties (-1 and NaN if there is none).
 * Rows outside [0, n) are left out of the mean; a cluster without members gets NaN means. */
int rgnn_cluster_scores(const float* prob, int64_t ldp, int32_t n_classes, int64_t n, const int64_t* obj_ptr, const int32_t* obj_rows,
                        int64_t n_rows, int64_t n_obj, const int32_t* group /*[dev] or NULL*/, int32_t bg_index, int32_t per_class,
                        double* mean, int32_t* cls, double* score, rgnn_stream_t stream);

/* ---------------------------------------------------------------- point-cloud frames of a sequence (csrc/preprocess.hip)
 * create_point_cloud_frames + SceneCollection.process + PointCloudProcessor.transform (preprocessor/radarscenes/
 * dataset_creation.py:159-184,716-783, scene_collection.py:36-156,185-230) behind the host's window plan: frame w is the rows
 * [win_rows[2 w], win_rows[2 w + 1]) of the detection table (ranges may overlap and may be empty) that survive the filter, in row
 * order.  Table columns as RadarScenes stores them ([dev], n_rows each); sensor_yaw: [dev] double [n_sensors] indexed by sensor_id;
 * label_map: [dev] int32 [n_labels] indexed by label_id, the reduced class or -1 = drop.
 * Per row, in float64: X = (x_cc, y_cc); angle = azimuth_sc + sensor_yaw[sensor_id]; V = vr_compensated * (cos angle, sin angle),
 * one multiply per component, nothing fused.  A row is dropped if crop != 0 and (|y| > sides or x > front or x < 0) -- strict, so
 * NaN coordinates and -0.0 stay --, if its label maps to -1, or if a component of V is NaN.
 * Outputs ([dev], caller-owned): frame_ptr int64 [n_win + 1]; per survivor, windows in order and rows in order inside a window:
 * X, V double [., 2], rcs_out, timestamp_out double, label_out (the mapped class), track_out, src_row (the row of the table) int32.
 * They hold n_cap rows: size them for the sum of the windows' rows (the host knows it) and narrow them to frame_ptr[n_win] after
 * reading it; nothing is ever written at or beyond n_cap.
 * A sensor_id / label_id outside its table drops the row, a window outside the table is left empty; both raise
 * RGNN_STATUS_PREPROCESS_BAD_ROW in *status, everything else is written as usual.
 * Three launches (count, scan, write), no host read, no waiting between work-groups; the result does not depend on scheduling.
 * tmp: [dev] rgnn_accumulate_frames_tmp_bytes(n_win) bytes. */
int64_t rgnn_accumulate_frames_tmp_bytes(int64_t n_win);
int rgnn_accumulate_frames(const int64_t* timestamp, const uint8_t* sensor_id, const float* azimuth_sc, const float* rcs,
                           const float* vr_compensated, const float* x_cc, const float* y_cc, const uint8_t* label_id,
                           const int32_t* track, int64_t n_rows, const int64_t* win_rows, int64_t n_win,
                           const double* sensor_yaw, int32_t n_sensors, const int32_t* label_map, int32_t n_labels,
                           int32_t crop, double front, double sides, int64_t* frame_ptr, int64_t n_cap, double* X, double* V,
                           double* rcs_out, double* timestamp_out, int32_t* label_out, int32_t* track_out, int32_t* src_row,
                           int32_t* status, void* tmp, rgnn_stream_t stream);

/* ---------------------------------------------------------------- nuScenes samples into labelled point clouds (csrc/nuscenes.hip)
 * preprocessor/nuscenes/dataset_creation.py:121-165,189-201,241-278, utils.py:6-48, conversion.py:112-187.  float64 throughout.
 *
 * rgnn_nusc_points: points is channel-major [19, n_total] (the devkit's 18 radar channels, the timestamp beneath), laid out in
 * chunks -- one per (sample, sensor), rows [chunk_ptr[c], chunk_ptr[c + 1]) -- with chunk_sample int32 [n_chunks] non-decreasing,
 * chunk_rotation [n_chunks, 4] (quaternion w, x, y, z; normalised here) and chunk_translation [n_chunks, 3].  Per row: channels
 * 0-2 are rotated and translated, channels 8-9 rotated by the upper-left 2 x 2; with crop != 0 a row is dropped if x > xlim,
 * x < -xlim, y > ylim or y < -ylim (a row on a limit stays, NaN stays).  Outputs per survivor, samples in order and rows in order
 * inside a sample: X (x, y), V (channels 8-9), V_cc (channels 6-7) double [., 2], rcs (channel 5), timestamp (channel 18) double,
 * src_row int32; frame_ptr int64 [n_samples + 1].  They hold n_cap rows (size for n_total); nothing is written at or beyond n_cap.
 * Lists that fail the check raise RGNN_STATUS_NUSC_BAD_CHUNK; a chunk outside the points is left out.
 * Three launches (count, scan, write); tmp: [dev] rgnn_nusc_points_tmp_bytes(n_samples) bytes.
 *
 * rgnn_nusc_boxes: boxes in the global frame (box_center, box_size = w, l, h [n_boxes, 3], box_rotation [n_boxes, 4], box_label,
 * box_points int32), sample s owning [box_ptr[s], box_ptr[s + 1]); ego pose per sample.  A box with box_points <= 0 is dropped; the
 * others move to the vehicle frame (c_v = R_e^T (c - t_e), R_v = R_e^T R_box); with crop != 0 a box stays only if
 * -xlim < c_v.x < xlim and -ylim < c_v.y < ylim.  Survivors keep list order and are written as records of
 * rgnn_nusc_box_record_doubles() (20) doubles into records [n_boxes, 20] at [box_ptr[s], box_ptr[s] + box_count[s]):
 *   0-2 p1 = corner 0 of corners(wlh_factor), 3-5 i = corner 4 - p1, 6-8 j = corner 1 - p1, 9 |i|, 10 |j|,
 *   11-15 the rectangle of the bottom corners of corners(1): x_c, y_c, l, w, theta in degrees (0 <= theta <= 180),
 *   16 label, 17 the box's index in the input list, 18-19 zero.
 * One launch (one wave per sample).
 *
 * rgnn_nusc_label_points: per point of sample s (rows [frame_ptr[s], frame_ptr[s + 1]) of pos [n, 2]) the LAST record of the sample, in
 * list order, with -offset <= i.v / |i| <= |i| + offset and the same for j, v = (x, y, 0) - p1.  label int32 [n] gets its label (0:
 * none), out double [n, 5] its box in encoding 0 none [x_c, y_c, l, w, theta], 1 translation [x_c - x, y_c - y, l, w, theta] or 2 en
 * [d, angle(nn -> centre), l, w, angle(nn -> long side)] (nn_index int32 [n], else NULL), NaN without a hit; hit (optional) int32 [n]
 * the winning box's index in the input list or -1.  One launch (one work-group per sample, records staged through LDS). */
int32_t rgnn_nusc_box_record_doubles(void);
int64_t rgnn_nusc_points_tmp_bytes(int64_t n_samples);
int rgnn_nusc_points(const double* points, int64_t n_total, const int64_t* chunk_ptr, const int32_t* chunk_sample,
                     const double* chunk_rotation, const double* chunk_translation, int64_t n_chunks, int64_t n_samples,
                     int32_t crop, double xlim, double ylim, int64_t* frame_ptr, int64_t n_cap, double* X, double* V, double* V_cc,
                     double* rcs, double* timestamp, int32_t* src_row, int32_t* status, void* tmp, rgnn_stream_t stream);
int rgnn_nusc_boxes(const double* box_center, const double* box_size, const double* box_rotation, const int32_t* box_label,
                    const int32_t* box_points, const int64_t* box_ptr, int64_t n_boxes, int64_t n_samples,
                    const double* ego_translation, const double* ego_rotation, int32_t crop, double xlim, double ylim,
                    double wlh_factor, double* records, int32_t* box_count, int32_t* status, rgnn_stream_t stream);
int rgnn_nusc_label_points(const double* pos, int64_t n, const int64_t* frame_ptr, int64_t n_samples, const double* records,
                           const int64_t* box_ptr, const int32_t* box_count, int64_t n_boxes, const int32_t* nn_index /*[dev] or NULL*/,
                           int32_t invariance, double wlh_offset, int32_t* label, double* out, int32_t* hit /*[dev] or NULL*/,
                           int32_t* status /*[dev]*/, rgnn_stream_t stream);

/* ---------------------------------------------------------------- nuScenes detection evaluation (csrc/nuscenes_eval.hip)
 * What the reference's NuscenesEvaluator runs after the post-processor (postprocessor/nuscenes/evaluation.py:41-74): the submission
 * records (postprocessor/nuscenes/utils.py:11-140,246-309) and the devkit's DetectionEval (eval/common/loaders.py add_center_dist /
 * filter_eval_boxes, eval/detection/algo.py accumulate / calc_ap / calc_tp, eval/common/utils.py center_distance / scale_iou /
 * yaw_diff / angle_diff / cummean).  float64, no fused multiply-add.  NOT PINNED BY AN EXECUTED DEVKIT: the semantics are restated
 * from the published sources (see the head of csrc/nuscenes_eval.hip); tests hold the kernels to a numpy restatement of the same
 * statements.  Every function clears its own status word ([dev] int32) and ORs the bits below into it; the caller reads it once.
 *
 * Names are int32 codes into the reference's label list (utils.py:172-184: 0 'void', 1 'barrier', 2 'bicycle', 3 'bus', 4 'car',
 * 5 'construction_vehicle', 6 'motorcycle', 7 'pedestrian', 8 'traffic_cone', 9 'trailer', 10 'truck'); attributes are int32 codes
 * the caller chooses, a negative one standing for ''.
 *
 * rgnn_nuscenes_submission (utils.py:246-309), one thread per box.  boxes [n_boxes, 5] = (x, y, l, w, theta in degrees) in the
 * vehicle frame (rgnn_box_representations), labels int32, sample s owning [box_ptr[s], box_ptr[s + 1]) with the LIDAR_TOP ego pose
 * ego_translation [n_samples, 3] / ego_rotation [n_samples, 4] (w, x, y, z; normalised here); heights [n_heights] by label
 * (get_bounding_box_size).  translation = R (x, y, 0) + t_e with z raised by h / 2; size = (w, l, h); angle = theta pi / 180 + yaw_e
 * with yaw_e = atan2(2 (w z - x y), 1 - 2 (y^2 + z^2)) (pyquaternion's yaw_pitch_roll[0]); rotation = (cos(angle / 2), 0, 0,
 * sin(angle / 2)); yaw = angle.  A label < 1 or >= n_heights raises RGNN_NUSC_EVAL_BAD_LABEL and its rows stay unwritten.
 *
 * rgnn_detection_filter (add_center_dist, filter_eval_boxes), one thread per box, for predictions (score given, num_pts NULL) and
 * ground truth (num_pts given, score NULL) alike.  keep uint8 [n_boxes] = sqrt(dx^2 + dy^2) of translation - ego_translation is
 * strictly below class_range[name], and num_pts > 0 where given, and -- for the names `bicycle` / `motorcycle`, where rack_ptr
 * (int64 [n_samples + 1]) is given -- the centre lies in no bike-rack box of the sample (the devkit's points_in_box: the
 * projections on the three edges of corner 0 lie in [0, |edge|^2], ends included; rack_size = w, l, h).  A name < 1 or >= n_names
 * is dropped and, for a prediction, raises RGNN_NUSC_EVAL_BAD_LABEL.  max_boxes > 0: a sample with more boxes raises
 * RGNN_NUSC_EVAL_TOO_MANY_BOXES (the devkit's assert); a NaN score raises RGNN_NUSC_EVAL_NAN_SCORE.
 *
 * rgnn_center_match (accumulate's loop), one wave per (sample, class of `classes`, threshold).  order: [dev] int64 [pred.n], the
 * predictions sample by sample, inside a sample by descending score with equal scores by DESCENDING position (the devkit sorts
 * (score, index) ascending and reverses): rgnn_sort_scores on the reversed array, then a stable pass by sample.  Per prediction of
 * the class that the filter kept, in that order: the minimum xy centre distance over the sample's kept ground truth of the class
 * not yet taken at this threshold, lowest position on ties; matched iff it is strictly below the threshold.  Thresholds are
 * independent passes.  match: int32 [n_thresholds, pred.n], the ground-truth box's index or -1; tp_err: [5, pred.n] for threshold
 * tp_index only -- centre distance, 1 - scale IoU, |yaw difference| (period 2 pi, pi for the name `barrier`), xy velocity
 * difference, attribute error (NaN for a ground-truth attribute < 0, else 0 / 1) -- NaN where unmatched.  Both are cleared here.
 * Capacity: rgnn_center_match_capacity() (512) kept ground-truth boxes of ONE class in one sample, counted on the device: more
 * raise RGNN_NUSC_EVAL_GT_OVERFLOW and leave that pair unmatched.  Offsets outside the lists raise RGNN_NUSC_EVAL_BAD_PTR.
 *
 * rgnn_detection_curves (accumulate after the loop, cummean), one work-group per (class, threshold).  order: [dev] int64, the KEPT
 * predictions class by class in the order of `classes`, inside a class by descending score over all samples (equal scores by
 * descending position); cls_ptr: int64 [2, n_classes], where each class begins and ends in it.  npos = the class's kept ground
 * truth.  npos == 0 or no match at the threshold: precision 0, confidence 0, errors 1.  Otherwise tp = running count of matches,
 * prec = tp / (tp + fp), rec = tp / npos, and precision / confidence = np.interp(grid, rec, ., right = 0): the LAST j with
 * rec[j] <= x; x < rec[0] gives the first value; j last or rec[j] == x gives value j; else (f[j+1] - f[j]) / (rec[j+1] - rec[j])
 * (x - rec[j]) + f[j].  For threshold tp_index, each error's running mean over the matched predictions that are not NaN (0
 * before the first, all ones if every value is NaN) is resampled at the interpolated confidence by np.interp over the reversed
 * arrays.  precision, confidence: [n_classes, n_thresholds, n_grid]; tp_err_curve: [n_classes, 5, n_grid]; grid: [n_grid]
 * ascending (at most 128); tmp: [dev] rgnn_detection_curves_tmp_bytes(n_pred, n_thresholds) bytes. */
#define RGNN_NUSC_EVAL_BAD_LABEL 1
#define RGNN_NUSC_EVAL_TOO_MANY_BOXES 2
#define RGNN_NUSC_EVAL_NAN_SCORE 4
#define RGNN_NUSC_EVAL_GT_OVERFLOW 8
#define RGNN_NUSC_EVAL_BAD_PTR 16
typedef struct rgnn_eval_boxes {
  const double* translation; /* [n, 3] global frame                */
  const double* size;        /* [n, 3] w, l, h                     */
  const double* rotation;    /* [n, 4] w, x, y, z                  */
  const double* velocity;    /* [n, 2] may be NaN                  */
  const int32_t* name;       /* [n]                                */
  const int32_t* attribute;  /* [n] negative: ''                   */
  const uint8_t* keep;       /* [n] rgnn_detection_filter          */
  const int64_t* ptr;        /* [n_samples + 1]                    */
  int64_t n;
} rgnn_eval_boxes;
int rgnn_nuscenes_submission(const double* boxes, const int32_t* labels, int64_t n_boxes, const int64_t* box_ptr, int64_t n_samples,
                             const double* ego_translation, const double* ego_rotation, const double* heights, int32_t n_heights,
                             double* translation, double* size, double* rotation, double* yaw, int32_t* status, rgnn_stream_t stream);
int rgnn_detection_filter(const double* translation, const int32_t* name, int64_t n_boxes, const int64_t* ptr, int64_t n_samples,
                          const double* ego_translation, const double* class_range, int32_t n_names,
                          const int32_t* num_pts /*[dev] or NULL*/, const double* score /*[dev] or NULL*/, int32_t max_boxes,
                          const double* rack_center, const double* rack_size, const double* rack_rotation,
                          const int64_t* rack_ptr /*[dev] or NULL*/, int64_t n_racks, int32_t bicycle, int32_t motorcycle,
                          uint8_t* keep, int32_t* status, rgnn_stream_t stream);
int32_t rgnn_center_match_capacity(void);
int rgnn_center_match(const rgnn_eval_boxes* pred, const rgnn_eval_boxes* gt, int64_t n_samples, const int64_t* order,
                      const int32_t* classes, int32_t n_classes, const double* thresholds, int32_t n_thresholds, int32_t tp_index,
                      int32_t barrier, int32_t* match, double* tp_err, int32_t* status, rgnn_stream_t stream);
int64_t rgnn_detection_curves_tmp_bytes(int64_t n_pred, int32_t n_thresholds);
int rgnn_detection_curves(const int64_t* order, const int64_t* cls_ptr, const double* score, const int32_t* match,
                          const double* tp_err, int64_t n_pred, const int32_t* gt_name, const uint8_t* gt_keep, int64_t n_gt,
                          const int32_t* classes, int32_t n_classes, int32_t n_thresholds, int32_t tp_index, const double* grid,
                          int32_t n_grid, double* precision, double* confidence, double* tp_err_curve, void* tmp,
                          rgnn_stream_t stream);

/* ---------------------------------------------------------------- optimizer step and target re-encoding (csrc/optim.hip)
 * rgnn_adam_step: torch.optim.Adam with amsgrad and maximize off and the weight decay added to the gradient, for n_tensors float32
 * tensors at once.  The tables are HOST arrays of length n_tensors, read before the call returns: device pointers of the parameter,
 * its gradient and its two moment tensors (contiguous, numel[i] floats each, 4-byte aligned, any offset inside an allocation), the
 * step count t of each tensor INCLUDING this step (>= 1), its learning rate and weight decay.  Per element, evaluated in double from
 * the float32 operands with every stored value rounded once:
 *   g = grad + wd p;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g g;
 *   p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * The tables travel as kernel arguments: ceil(n / capacity) launches for the n tensors that are not empty, capacity =
 * rgnn_adam_capacity (64); *launches (host, optional) receives the number made.  No allocation, no copy, no synchronisation.
 *
 * rgnn_adapt_orientation_angle: adapt_bb_orientation_angle (preprocessor/bounding_box.py:536-563) on y = [n, width] float32 rows
 * (label | box, width >= 6), out of place: every row is copied bit for bit, and where y[i, 1] is not NaN, out[i, 5] =
 * sin(y[i, 5] > pi / 2 ? y[i, 5] - pi : y[i, 5]), compared, subtracted and evaluated in double, rounded once.  One launch. */
int32_t rgnn_adam_capacity(void);
int rgnn_adam_step(int64_t n_tensors, void* const* param, const void* const* grad, void* const* exp_avg, void* const* exp_avg_sq,
                   const int64_t* numel, const int64_t* step, const double* lr, const double* weight_decay, double beta1,
                   double beta2, double eps, int32_t* launches /*[host] or NULL*/, rgnn_stream_t stream);
int rgnn_adapt_orientation_angle(const float* y, int64_t ldy, float* out, int64_t ldo, int64_t n, int32_t width,
                                 rgnn_stream_t stream);

/* ---------------------------------------------------------------- rigid motions (csrc/transform.hip)
 * The motion of frame (graph) f: p' = R(a_f) p + t_f for points, v' = R(a_f) v for velocities and differences, R = [[c, -s], [s, c]],
 * angle[f] = a_f in radians, counter-clockwise, shift[f] = t_f; angle float64 [B], shift float64 [B, 2], both on the device.
 * Everything is evaluated in double from the stored operands (separate multiplies and adds) and rounded once at the store.  An
 * angle of exactly 0 keeps every rotated quantity bit for bit, a shift component of exactly 0 is not added: the identity motion
 * returns the input bits.  One launch each, no temporaries, no host read.
 *
 * rgnn_rigid_points: X, V float64 [n, 2] -> X_out, V_out (V and V_out may both be NULL); row i belongs to the frame f with
 * frame_ptr[f] <= i < frame_ptr[f + 1] (int64 [n_frames + 1]; frames of no rows are legal).  Out of place.
 *
 * rgnn_rigid_graph_nodes: the node rows of a collated batch; batch int64 [n] = the graph of every row.  pos / vel float32 [n, 2]
 * -> pos_out / vel_out, whole rows, out of place.  x (row stride ldx, columns as the node feature codes list them) and y =
 * [label | box] (row stride ldy, box_width 4 or 5): the caller passes COPIES as x_out / y_out and the kernel writes only what
 * moves -- spatial_coordinates (moved as a point), velocity_vector (rotated); of a rotated box [c0, c1, l, w, theta] (box_width 5,
 * theta in [0, pi)) with invariance 0 (none) the centre as a point, with invariance 1 (translation) the offset c - p rotated, and
 * theta' = theta + a folded into [0, pi) in double, a result that rounds to float32(pi) stored as 0.  Rows whose first box column
 * is NaN (background), the en encoding (2), aligned boxes (box_width 4), the label and every other feature are never written.
 * Any of the pairs pos, vel, x, y may be NULL.
 *
 * rgnn_rigid_graph_edges: edge_attr (row stride lda, columns as the edge feature codes list them), `out` a COPY of it; the graph
 * of edge e is batch[edge_index[0, e]].  relative_position / relative_velocity: directed -- the stored 2-vector rotated;
 * undirected -- |R (q_i - q_j)| per component from the batch's ORIGINAL pos / vel float32 [n, 2], i = edge_index[0, e],
 * j = edge_index[1, e].  Nothing else is written; edges of a graph whose angle is 0, or with an end outside [0, n), keep their
 * rows. */
int rgnn_rigid_points(const double* X, const double* V, const int64_t* frame_ptr, int64_t n, int64_t n_frames, const double* angle,
                      const double* shift, double* X_out, double* V_out, rgnn_stream_t stream);
int rgnn_rigid_graph_nodes(const float* pos, const float* vel, const float* x, int64_t ldx, const int32_t* node_codes /*host*/,
                           int32_t n_codes, const float* y, int64_t ldy, int32_t box_width, int32_t invariance,
                           const int64_t* batch, int64_t n, int64_t n_graphs, const double* angle, const double* shift,
                           float* pos_out, float* vel_out, float* x_out, int64_t ldxo, float* y_out, int64_t ldyo,
                           rgnn_stream_t stream);
int rgnn_rigid_graph_edges(const float* edge_attr, int64_t lda, const int32_t* edge_codes /*host*/, int32_t n_codes,
                           int32_t undirected, const int64_t* edge_index, int64_t n_edges, const int64_t* batch, int64_t n,
                           int64_t n_graphs, const double* angle, const float* pos, const float* vel, float* out, int64_t ldo,
                           rgnn_stream_t stream);

/* ---------------------------------------------------------------- subgraphs (csrc/subgraph.hip)
 * A part of a collated batch: the nodes i with keep_nodes[i] != 0 and the edges e = (s, t) with keep_edges[e] != 0 whose two ends are
 * kept, in their order, relabelled (PyG: torch_geometric.utils.subgraph with relabel_nodes, dropout_node, dropout_edge; no reference
 * counterpart).  edge_index int64 [2, E] (row stride E), batch int64 [N] = the graph of every node, ptr int64 [B + 1] = the node
 * offsets, keep_nodes uint8 [N] or NULL (all), keep_edges uint8 [E] or NULL (all); N + E + 1 < 2^31 (else
 * RGNN_ERR_INVALID_ARGUMENT).  The count -> scan -> fill protocol, every buffer the caller's:
 *   rgnn_subgraph_flags      flags int32 [N + E]: flags[i] = node i is kept, flags[N + e] = edge e is kept; graph_edges int32 [B],
 *                            ZEROED BY THE CALLER: the kept edges of every graph (of their source's graph); one launch;
 *   rgnn_exclusive_scan_i32  scan int32 [N + E + 1] of flags: new_id[i] = flags[i] ? scan[i] : -1 is the relabelling, a kept edge e
 *                            goes to place scan[N + e] - scan[N];
 *   rgnn_subgraph_offsets    ptr_out int64 [B + 1]: ptr_out[g] = scan[ptr[g]], the kept nodes of the graphs before g; edge_ptr_out
 *                            int64 [B + 1]: the kept edges whose source lies in a graph before g; totals int32 [4] = {N', E', the
 *                            status word as it stands, 0} -- the caller sizes the outputs AND learns of bad input by ONE 16-byte
 *                            host read, the only one of the operation; one launch of one work-group;
 *   rgnn_subgraph_fill       edge_index_out int64 [2, E'] (row stride E') = (new_id[s], new_id[t]), batch_out int64 [N'] = batch of the
 *                            kept nodes, new_id int32 [N], node_ids int64 [N'] / edge_ids int64 [E'] = the original positions; any
 *                            output may be NULL; n_out = N', e_out = E' as read (a place outside them is not written); one launch;
 *   rgnn_subgraph_gather_rows  out[r, :] = src[ids[r], :] for r < n_out: rows of `width` 4-byte words, row stride ld_src words in
 *                            src, `width` in out; ids as node_ids / edge_ids; 16 bytes per lane when width and ld_src are
 *                            multiples of 4 and both bases 16-byte aligned, else one word per lane; one launch per attribute.
 * Every index is range-checked before it is used as one.  An edge is dropped, whatever the masks say, and its bit is raised in
 * `status`, when an end lies outside [0, N) (BAD_ENDPOINT), the graph of its source lies outside [0, B) (BAD_GRAPH), its ends
 * lie in two graphs (CROSS_GRAPH), or the source of the edge before it is a node of a LATER graph (EDGE_ORDER: the edge list of a
 * collated batch is grouped by graph, ascending; the first edge of every descent is the one dropped).  A ptr[g] outside [0, N] is
 * clamped and raises BAD_GRAPH.  An id outside [0, n_in) leaves its row of the gather unwritten.
 * No kernel waits on another work-group, every loop is bounded by a shape or the wave size, the atomics are integer adds and ors
 * (the result does not depend on scheduling), and no input is ever written.
 *
 * rgnn_edge_pair_mask: mask_out[e] uint8 = keep edge e, decided by the UNORDERED pair of its ends so that (s, t) and (t, s) fall
 * together (DropEdge on symmetric and undirected graphs).  With lo = min(s, t), hi = max(s, t), arithmetic mod 2^64 and
 *   mix(z): z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31)
 * draw = mix(mix(seed) ^ ((lo << 32) | hi)) >> 40 (24 bits) and keep = draw >= threshold, threshold = floor(p 2^24) in [0, 2^24]:
 * p = 0 keeps every edge, p = 1 none.  seed: [dev] int64 [1], never read by the host.  An edge with an end outside [0, N) gets 0;
 * N <= 2^32.  One launch.
 *
 * rgnn_store_degree_column: x[i, column] = (float)degree[i] for i < n (x float32, row stride ldx): the `degree` node feature
 * rewritten after rgnn_undirected_degree on the kept graph.  One launch. */
#define RGNN_STATUS_SUBGRAPH_BAD_ENDPOINT 8192
#define RGNN_STATUS_SUBGRAPH_CROSS_GRAPH 16384
#define RGNN_STATUS_SUBGRAPH_EDGE_ORDER 32768
#define RGNN_STATUS_SUBGRAPH_BAD_GRAPH 65536
int rgnn_subgraph_flags(const int64_t* edge_index, int64_t n_edges, const int64_t* batch, int64_t n, int64_t n_graphs,
                        const uint8_t* keep_nodes /*[dev] or NULL*/, const uint8_t* keep_edges /*[dev] or NULL*/, int32_t* flags,
                        int32_t* graph_edges, int32_t* status, rgnn_stream_t stream);
int rgnn_subgraph_offsets(const int32_t* scan, const int32_t* graph_edges, const int64_t* ptr, int64_t n, int64_t n_edges,
                          int64_t n_graphs, int64_t* ptr_out, int64_t* edge_ptr_out, int32_t* totals, int32_t* status,
                          rgnn_stream_t stream);
int rgnn_subgraph_fill(const int64_t* edge_index, int64_t n_edges, const int64_t* batch, int64_t n, const int32_t* flags,
                       const int32_t* scan, int64_t n_out, int64_t e_out, int64_t* edge_index_out, int64_t* batch_out,
                       int32_t* new_id, int64_t* node_ids, int64_t* edge_ids, rgnn_stream_t stream);
int rgnn_subgraph_gather_rows(const void* src, int64_t ld_src, int32_t width, const int64_t* ids, int64_t n_out, int64_t n_in,
                              void* out, rgnn_stream_t stream);
int rgnn_edge_pair_mask(const int64_t* edge_index, int64_t n_edges, int64_t n, const int64_t* seed /*[dev] int64 [1]*/,
                        int32_t threshold, uint8_t* mask_out, rgnn_stream_t stream);
int rgnn_store_degree_column(const int32_t* degree, int64_t n, float* x, int64_t ldx, int32_t column, rgnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RGNN_H */
