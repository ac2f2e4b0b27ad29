"""Inputs that sit ON the edges of the feature, time-index and row-list kernels (csrc/features.hip), with plain numpy expectations:
pure numpy builders shared by tests/test_gpu_feature_edges.py (the kernels against these expectations) and
tests/test_feature_edge_cases.py (proof, on the CPU alone, that every input really stands on the edge it is named for).  Needs
neither torch nor a GPU.

Expectations come from oracle/graph_oracle.py (edge_features, node_features) or from a few lines of numpy here (np.unique per
frame, np.nonzero, list padding); nothing comes from the code under test.  Everything is deterministic."""
import numpy as np

from oracle import graph_oracle as go

# numbers of csrc/features.hip that the builders aim at (restated: the CPU test ties the inputs to them)
TI_THREADS = 1024                  # k_time_index: threads per frame
TI_ROUND = 4 * TI_THREADS          # ... points per round of its two frame walks
TI_CAP = 4096                      # hash slots
TI_MAX_UNIQUE = 3072               # distinct timestamps of a frame; one more raises STATUS_TIME_INDEX_OVERFLOW
TI_HASH_MUL = 0x9E3779B97F4A7C15
TI_SPREAD_HINT = 16385             # the smallest max_frame_points that selects the spread-out chain
TI_SPREAD_MAX_FRAMES = 1024        # ops.time_index drops the hint above this many frames
SPLIT_STRIP = 1024                 # k_split_frames: nodes per strip, and the stride of its sum over earlier frames
PAD_ROWS = 256                     # k_pad_list_segments: tile rows, and the stride of its prefix loop over segments
PANEL_ROWS = 128                   # csrc/common.h RGNN_STAT_PANEL_ROWS
COUNT_TRIP = 4 * 4 * 1024          # k_radius_counts: entries per trip of the 16-byte loop (4 loads x 4 entries x 1024 threads)
COUNT_SATURATED = 0x7FFFFFFF
MAX_FEATURE_CODES = 16             # rgnn.h RGNN_MAX_FEATURE_CODES

EDGE_NAMES = ("point_pair_features", "spatial_euclidean_distance", "velocity_euclidean_distance", "relative_position",
              "relative_velocity")
NODE_NAMES = ("rcs", "time_index", "degree", "velocity_vector_length", "velocity_vector", "spatial_coordinates")


# ------------------------------------------------------------------------------------------------ comparing
def bits(a):
    """The bit patterns of a float array as integers of the same width, every NaN folded into one pattern: equal bits <=> equal
    values, the sign of zero included, NaN equal to NaN."""
    a = np.ascontiguousarray(a)
    out = a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]).copy()
    out[np.isnan(a)] = -1
    return out


def ulp_distance(a, b):
    """Largest distance in units of the last place between two finite arrays of one float type (0 where the bits agree)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    it = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    ia, ib = a.view(it).astype(np.int64), b.view(it).astype(np.int64)
    lowest = np.int64(np.iinfo(it).min)
    ia, ib = np.where(ia < 0, lowest - ia, ia), np.where(ib < 0, lowest - ib, ib)      # monotone in the value
    return int(np.abs(ia - ib).max()) if ia.size else 0


def rotations(names):
    names = list(names)
    return [names[s:] + names[:s] for s in range(len(names))]


def edge_columns(names):
    """-> (columns held to bit equality, angle columns) of the feature list's output."""
    exact, angle, w = [], [], 0
    for nm in names:
        if nm == "point_pair_features":
            exact.append(w); angle += [w + 1, w + 2, w + 3]
        else:
            exact += list(range(w, w + go.EDGE_FEATURE_WIDTH[nm]))
        w += go.EDGE_FEATURE_WIDTH[nm]
    return np.array(exact, dtype=np.int64), np.array(angle, dtype=np.int64)


def ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ time index
TI_FRAME_SIZES = (0, 0, 1, 1023, 1024, 1025, 0, 4095, 4096, 4097, 8193, 0)
TI_VALUE_KINDS = ("equal", "descending", "zeros", "infinities", "tiniest", "neighbours", "negatives", "microseconds")
TI_DISTINCT_COUNTS = (1, 2, TI_MAX_UNIQUE - 1, TI_MAX_UNIQUE)


def ti_values(kind, n, seed=0):
    """n timestamps of one kind (see TI_VALUE_KINDS); at most 2 048 distinct values, so no frame size overflows the set."""
    rng = np.random.Generator(np.random.PCG64(900 + seed))
    i = np.arange(n, dtype=np.int64)
    if kind == "equal":
        return np.full(n, 1.5e15 + 7.0)
    if kind == "descending":                           # all distinct up to 2 048 points, strictly falling
        return (np.float64(n) - (i % 2048).astype(np.float64)) * 0.125
    if kind == "zeros":                                # 0.0 and -0.0 are ONE value for np.unique; a neighbour on either side
        return np.array([0.0, -0.0, -0.0, 0.0, 1.0, -1.0])[(i * 5 + seed) % 6]
    if kind == "infinities":
        return np.array([np.inf, -np.inf, 0.0, 1.7976931348623157e308, -1.7976931348623157e308, np.inf])[(i * 7 + seed) % 6]
    if kind == "tiniest":                              # the two smallest subnormals around the two zeros
        return np.array([5e-324, -5e-324, 0.0, -0.0, 1e-323, -1e-323])[(i * 11 + seed) % 6]
    if kind == "neighbours":                           # pairs t, nextafter(t): distinct values one ulp apart
        t = np.array([1.0, -3.0, 1.5e15, 0.1, -1e-300])[(i // 2) % 5]
        return np.where(i % 2 == 0, t, np.nextafter(t, np.inf))
    if kind == "negatives":
        return -np.abs(rng.integers(1, 1500, size=n).astype(np.float64)) * 0.5
    if kind == "microseconds":                         # RadarScenes timestamps: integers around 1.5e15
        return 1.5e15 + rng.integers(0, 40, size=n).astype(np.float64) * 17.0
    raise ValueError(kind)


def ti_round_values(n, seed=0):
    """n timestamps in a scrambled order (at most 2 048 distinct) whose LAST one is the frame's only largest: a walk that drops
    the last point of a round loses a distinct value, and that point's own rank is the highest, not 0."""
    i = np.arange(n, dtype=np.int64)
    v = ((i * 389 + seed) % max(min(n, 2048), 1)).astype(np.float64) * 0.25 - 100.0
    v[-1:] = 1e6 + seed
    return v


def ti_size_batch():
    """One batch with the frame sizes TI_FRAME_SIZES (round edges of the frame walk; empty frames in front, at the back and
    doubled).  -> (timestamps [n], frame_ptr [F + 1])."""
    return np.concatenate([ti_round_values(n, seed=f) for f, n in enumerate(TI_FRAME_SIZES)]), ptr_of(TI_FRAME_SIZES)


def ti_value_batch(n=301):
    """One frame per kind of TI_VALUE_KINDS, n points each, an empty frame between any two."""
    parts, sizes = [], []
    for s, kind in enumerate(TI_VALUE_KINDS):
        parts.append(ti_values(kind, n, seed=50 + s)); sizes += [n, 0]
    return np.concatenate(parts), ptr_of(sizes)


def ti_distinct_frame(distinct, n, seed=0):
    """n >= distinct points holding exactly `distinct` distinct timestamps (quarter steps around zero), shuffled."""
    rng = np.random.Generator(np.random.PCG64(1300 + seed))
    vals = (np.arange(distinct, dtype=np.float64) - distinct // 2) * 0.25
    idx = np.concatenate([np.arange(distinct), rng.integers(0, distinct, size=n - distinct)])
    return vals[rng.permutation(idx)]


def ti_distinct_batch():
    """Frames with 1, 2, 3 071 and 3 072 distinct values (the last two: just below and AT the limit of the set), each with
    repeats, 3 072 also without."""
    frames = [ti_distinct_frame(1, 40), ti_distinct_frame(2, 1100, 1), ti_distinct_frame(TI_MAX_UNIQUE - 1, 4200, 2),
              ti_distinct_frame(TI_MAX_UNIQUE, 4100, 3), ti_distinct_frame(TI_MAX_UNIQUE, TI_MAX_UNIQUE, 4)]
    return np.concatenate(frames), ptr_of([len(f) for f in frames])


def ti_overflow_batch():
    """A frame with 3 073 distinct values (one beyond the limit) between two small ones."""
    frames = [ti_distinct_frame(3, 20, 5), ti_distinct_frame(TI_MAX_UNIQUE + 1, TI_MAX_UNIQUE + 30, 6), ti_distinct_frame(2, 10, 7)]
    return np.concatenate(frames), ptr_of([len(f) for f in frames])


def ti_slot(t):
    """The home slot of timestamps in the kernels' hash set: the top 12 bits of key * 0x9E3779B97F4A7C15 mod 2^64 (the key is the
    bit pattern, -0.0 folded into 0.0)."""
    t = np.where(np.asarray(t, dtype=np.float64) == 0.0, 0.0, np.asarray(t, dtype=np.float64))
    with np.errstate(over="ignore"):
        return ((np.ascontiguousarray(t).view(np.uint64) * np.uint64(TI_HASH_MUL)) >> np.uint64(52)).astype(np.int64)


def ti_last_slot_values(limit=1 << 18):
    """Every k * 0.5, 0 <= k < limit, whose home slot is the table's last one (4 095)."""
    v = np.arange(limit, dtype=np.float64) * 0.5
    return v[ti_slot(v) == TI_CAP - 1]


def ti_wrap_batch():
    """A frame whose probe chains cross from slot 4 095 to slot 0: every timestamp with home slot 4 095 among k / 2, k < 2^18 (62 of
    them, so the chain runs over slots 4 095, 0, 1, ... 60), three copies of each, mixed with 500 ordinary values; beside it a frame
    of the colliding values alone and a small ordinary frame."""
    rng = np.random.Generator(np.random.PCG64(1700))
    hot = ti_last_slot_values()
    plain = np.arange(500, dtype=np.float64) * 0.5 + 1000.25
    mixed = np.concatenate([hot, plain, hot, plain[:200], hot])
    mixed = mixed[rng.permutation(len(mixed))]
    alone = np.concatenate([hot[::-1], hot])
    frames = [ti_distinct_frame(5, 64, 8), mixed, alone]
    return np.concatenate(frames), ptr_of([len(f) for f in frames])


def ti_many_frames(n_frames=TI_SPREAD_MAX_FRAMES + 1):
    """n_frames tiny frames (0 ... 3 points, values from a pool of four with -0.0 / 0.0 among them)."""
    rng = np.random.Generator(np.random.PCG64(1900))
    sizes = rng.integers(0, 4, size=n_frames)
    sizes[[0, 1, n_frames - 1]] = (0, 3, 2)
    pool = np.array([0.0, -0.0, 2.5, -7.0])
    return pool[rng.integers(0, 4, size=int(sizes.sum()))], ptr_of(sizes)


def ti_expected(ts, ptr):
    """np.unique(..., return_inverse=True) per frame -> float64 [n]."""
    out = np.zeros(len(ts), dtype=np.float64)
    for f in range(len(ptr) - 1):
        lo, hi = int(ptr[f]), int(ptr[f + 1])
        if hi > lo:
            out[lo:hi] = np.unique(ts[lo:hi], return_inverse=True)[1].reshape(-1)
    return out


def ti_distinct_per_frame(ts, ptr):
    return [len(np.unique(ts[int(ptr[f]):int(ptr[f + 1])])) for f in range(len(ptr) - 1)]


# ------------------------------------------------------------------------------------------------ edge features
EDGE_SIZES = (0, 1, 255, 256, 257, 513)               # one thread per edge, 256 per block
LATTICE_VARIANTS = ("parallel", "antiparallel", "perpendicular", "parallel_perpendicular", "perpendicular_parallel",
                    "parallel_antiparallel")
DEGENERATE_ROWS = ("coincident", "self_loop", "zero_velocity_first", "zero_velocity_second", "zero_velocity_both",
                   "negative_zero")


def lattice_vectors():
    """The 168 non-zero vectors of the integer lattice [-6, 6]^2."""
    g = np.arange(-6, 7, dtype=np.float64)
    c = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    return c[(c != 0).any(axis=1)]


def lattice_case(variant):
    """Row k: an edge from the origin to lattice vector c_k (nodes 2k and 2k + 1), both ways ((2k, 2k + 1) in the first half of
    the edge list, (2k + 1, 2k) in the second); the two velocities are c_k itself (parallel), -c_k (anti-parallel) or c_k turned
    by 90 degrees (perpendicular), as the variant names them for (first end, second end).  -> X [336, 2], V [336, 2], E [336, 2]."""
    c = lattice_vectors()
    turn = {"parallel": c, "antiparallel": -c, "perpendicular": np.stack([-c[:, 1], c[:, 0]], 1)}
    a, _, b = variant.partition("_")
    X = np.zeros((2 * len(c), 2))
    V = np.zeros((2 * len(c), 2))
    X[1::2] = c
    V[0::2], V[1::2] = turn[a], turn[b or a]
    k = np.arange(len(c), dtype=np.int64)
    E = np.concatenate([np.stack([2 * k, 2 * k + 1], 1), np.stack([2 * k + 1, 2 * k], 1)])
    return X, V, E


def unit_self_dots():
    """u . u of every normalised lattice vector, in the oracle's arithmetic: what acos sees for a velocity parallel to its edge."""
    u = go._unit_or_zero(lattice_vectors())
    return go._dot2(u, u)


def degenerate_case():
    """One edge (both ways, except the self loop) per name of DEGENERATE_ROWS.  -> X, V, E, {name: rows of E}."""
    X = np.array([[1.5, -2.0], [1.5, -2.0],            # 0, 1   coincident end points, both moving
                  [3.0, 4.0],                            # 2      a self loop
                  [0.0, 0.0], [2.0, 1.0],                # 3, 4   zero velocity at node 3
                  [-1.0, 5.0], [2.5, 5.0],               # 5, 6   zero velocity at both
                  [-0.0, 2.0], [-0.0, -3.0]])            # 7, 8   -0.0 components in X and V
    V = np.array([[1.0, 2.0], [-2.0, 0.5], [0.5, -1.5], [0.0, 0.0], [1.0, -1.0], [0.0, 0.0], [-0.0, 0.0], [-0.0, 2.0], [3.0, -0.0]])
    E = np.array([[0, 1], [1, 0], [2, 2], [3, 4], [4, 3], [5, 6], [6, 5], [7, 8], [8, 7]], dtype=np.int64)
    rows = {"coincident": [0, 1], "self_loop": [2], "zero_velocity_first": [3], "zero_velocity_second": [4],
            "zero_velocity_both": [5, 6], "negative_zero": [7, 8]}
    return X, V, E, rows


def extreme_case():
    """Coordinates and velocities of 1e39 (finite in float64; every float32 cast of a difference, a distance or a coordinate is
    inf) and differences of 1e-46 and 1e-45 (float32: zero, and the smallest subnormal).  -> X, V, E."""
    X = np.array([[1e39, 0.0], [0.0, -1e39], [-1e39, 1e39], [1.0, 1.0], [1.0 + 2.0 ** -40, 1.0],
                  [0.0, 0.0], [1e-46, 0.0], [0.0, -1e-45], [1e-46, 1e-46]])
    V = np.array([[1e39, 1e39], [-1e39, 0.0], [0.0, 1e39], [1e-46, 0.0], [0.0, 1e-46],
                  [1e-46, 1e-46], [0.0, 0.0], [-1e-45, 0.0], [1e39, -1e-46]])
    pairs = [(0, 1), (1, 2), (0, 2), (0, 3), (3, 4), (5, 6), (5, 7), (6, 7), (6, 8), (5, 8), (2, 5)]
    E = np.array(pairs + [(j, i) for i, j in pairs], dtype=np.int64)
    return X, V, E


def generic_case(n=64):
    """n points and velocities with full 53-bit mantissas, a ring of edges both ways: products that round, so x x + y y with a
    fused multiply-add is another number than with a multiply and an add.  -> X, V, E."""
    rng = np.random.Generator(np.random.PCG64(2100))
    X, V = rng.normal(size=(n, 2)) * 30.0, rng.normal(size=(n, 2)) * 7.0
    k = np.arange(n, dtype=np.int64)
    E = np.concatenate([np.stack([k, (k + 1) % n], 1), np.stack([(k + 1) % n, k], 1)])
    return X, V, E


def stack_cases(cases):
    """Several (X, V, E) as one graph: node ids shifted."""
    Xs, Vs, Es, off = [], [], [], 0
    for X, V, E in cases:
        Xs.append(X); Vs.append(V); Es.append(E + off)
        off += len(X)
    return np.concatenate(Xs), np.concatenate(Vs), np.concatenate(Es)


def edge_pool():
    """Every lattice variant, the degenerate rows, the float extremes and the generic ring as one graph of 2 175 edges."""
    return stack_cases([lattice_case(v) for v in LATTICE_VARIANTS] + [degenerate_case()[:3], extreme_case(), generic_case()])


def sized_edges(n_edges):
    """n_edges edges of the pool, taken with a stride that visits every kind of row.  -> X, V, E [n_edges, 2]."""
    X, V, E = edge_pool()
    return X, V, E[(np.arange(n_edges, dtype=np.int64) * 37) % len(E)]


def edge_lists():
    """The feature lists of the issue: each name alone, all five in their five rotations, sixteen names (16 x point-pair: 64
    columns; and the five names repeated up to sixteen)."""
    return ([[nm] for nm in EDGE_NAMES] + rotations(EDGE_NAMES) + [["point_pair_features"] * MAX_FEATURE_CODES]
            + [[EDGE_NAMES[(3 * s) % 5] for s in range(MAX_FEATURE_CODES)]])


def reversed_lists(n_edges):
    """reversed_of lists for an edge list of n_edges > 300 edges: a permuted subset, one with repeats, and 0 / 1 / 257 rows."""
    rng = np.random.Generator(np.random.PCG64(2300))
    return {"permuted_subset": rng.permutation(n_edges)[:n_edges // 2].astype(np.int32),
            "repeats": rng.integers(0, 9, size=300).astype(np.int32) * (n_edges // 9),
            "rows_0": np.zeros(0, dtype=np.int32), "rows_1": np.array([n_edges - 1], dtype=np.int32),
            "rows_257": rng.integers(0, n_edges, size=257).astype(np.int32)}


# ------------------------------------------------------------------------------------------------ node features
NODE_SIZES = (0, 1, 255, 256, 257)
DEGREE_EDGES = (0, 2 ** 24 + 1, 2 ** 31 - 1)           # the last two are not float32 numbers: the cast rounds


def node_case(n):
    """n nodes in three frames (the middle one empty): lattice and extreme coordinates and velocities, rcs with -0.0, +-inf and
    NaN passed through, degrees 0, 2^24 + 1 and 2^31 - 1 among small ones, a free-standing time-index column, and timestamps.
    -> dict of X, V, rcs, time_index, degree (int32), timestamp, frame_ptr."""
    rng = np.random.Generator(np.random.PCG64(2900 + n))
    i = np.arange(n, dtype=np.int64)
    c = lattice_vectors()
    X = c[(i * 5) % len(c)] * 0.75
    V = c[(i * 11 + 3) % len(c)] * 1.3
    V[i % 2 == 0] = rng.normal(size=((n + 1) // 2, 2)) * 7.0                       # full mantissas: squares that round
    special = np.array([[1e39, -1e39], [1e-46, -0.0], [0.0, 1e-45], [3.0, 4.0]])
    X[i % 7 == 3] = special[(i[i % 7 == 3] // 7) % 4]
    V[i % 5 == 1] = special[(i[i % 5 == 1] // 5) % 4]
    rcs = rng.normal(size=n) * 10.0
    rcs_special = np.array([-0.0, np.inf, -np.inf, np.nan, 1e39, 1e-46])
    rcs[i % 3 == 0] = rcs_special[(i[i % 3 == 0] // 3) % 6]
    degree = rng.integers(0, 90, size=n).astype(np.int64)
    degree[i % 4 == 0] = np.array(DEGREE_EDGES)[(i[i % 4 == 0] // 4) % 3]
    tidx = ((i * 13) % 29).astype(np.float64)
    ts = 1.5e15 + ((i * 7) % 5).astype(np.float64) * 1000.0
    cut = n // 2
    return dict(X=X, V=V, rcs=rcs, time_index=tidx, degree=degree.astype(np.int32), timestamp=ts,
                frame_ptr=np.array([0, cut, cut, n], dtype=np.int64))


def node_lists():
    return ([[nm] for nm in NODE_NAMES] + rotations(NODE_NAMES) + [[NODE_NAMES[(5 * s + 1) % 6] for s in range(MAX_FEATURE_CODES)]])


def node_expected(case, names, time_index):
    return go.node_features(case["X"], case["V"], {"rcs": case["rcs"], "time_index": time_index}, case["degree"], names)


# ------------------------------------------------------------------------------------------------ frame split
SPLIT_FRAME_SIZES = (0, 1, 1023, 1024, 1025, 0, 0, 2049, 1)
DEGREE_PATTERNS = ("all_zero", "all_positive", "alternating", "last_only", "first_only")


def split_many_frame_sizes(n_frames=SPLIT_STRIP + 6):
    rng = np.random.Generator(np.random.PCG64(3100))
    sizes = rng.integers(0, 4, size=n_frames)
    sizes[[0, n_frames - 1]] = (2, 1)
    return sizes


def degree_pattern(pattern, n):
    i = np.arange(n)
    deg = {"all_zero": np.zeros(n), "all_positive": 1 + i % 5, "alternating": (i % 2) * (1 + i % 3),
           "last_only": (i == n - 1) * 4, "first_only": (i == 0) * 2}[pattern]
    return deg.astype(np.int32)


def split_expected(degree, ptr):
    """-> dict: frame_nonempty [F], list_nonempty, list_empty, the two counts, slot [n] (-1 on nodes with edges, the node's place
    in list_empty elsewhere)."""
    ne, e = np.nonzero(degree > 0)[0], np.nonzero(degree == 0)[0]
    slot = np.full(len(degree), -1, dtype=np.int32)
    slot[e] = np.arange(len(e))
    frame = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    return dict(frame_nonempty=np.bincount(frame[ne], minlength=len(ptr) - 1).astype(np.int32), list_nonempty=ne.astype(np.int32),
                list_empty=e.astype(np.int32), count_nonempty=len(ne), count_empty=len(e), slot=slot)


# ------------------------------------------------------------------------------------------------ padded lists
PAD_ENTRY_COUNTS = (0, 1, 255, 256, 257, 512)
PAD_GARBAGE = 123456


def pad_case(entries, ranges, tail=300, end_before_last=False):
    """A list with entries[s] ids inside segment s, whose row range holds ranges[s] >= entries[s] rows (the ids spread over the
    range, its first and last row taken when there are two or more), in a buffer `tail` entries longer than the list and full of
    garbage there.  end_before_last: the last segment keeps its rows and loses its entries.
    -> (buffer int32, count, seg_ptr int64 [S + 1])."""
    seg = ptr_of(ranges)
    ids = []
    for s, k in enumerate(entries):
        if end_before_last and s == len(entries) - 1:
            k = 0
        assert k <= ranges[s]
        if k:
            ids.append(seg[s] + (np.arange(k, dtype=np.int64) * (ranges[s] - 1)) // max(k - 1, 1))
    ids = np.concatenate(ids).astype(np.int32) if ids else np.zeros(0, dtype=np.int32)
    buf = np.full(len(ids) + tail, PAD_GARBAGE, dtype=np.int32)
    buf[:len(ids)] = ids
    return buf, len(ids), seg


def pad_cases():
    """name -> (buffer, count, seg_ptr)."""
    cases = {}
    for k in PAD_ENTRY_COUNTS:                                         # one segment; the whole list inside one segment
        cases[f"one_segment_{k}"] = pad_case([k], [max(k, 1) + 3])
    cases["one_segment_no_rows"] = pad_case([0], [0])
    many = [PAD_ENTRY_COUNTS[s % 6] for s in range(PAD_ROWS + 1)]      # 257 segments, every entry count, empty row ranges among them
    ranges = [0 if s % 12 == 0 else k + 1 + (s % 3) for s, k in enumerate(many)]
    cases["257_segments"] = pad_case(many, ranges)
    cases["257_segments_short_list"] = pad_case(many[:-1] + [257], ranges[:-1] + [300], end_before_last=True)
    inside = [0] * 6 + [512] + [0] * 4
    cases["all_in_one_of_eleven"] = pad_case(inside, [7, 0, 300, 1, 0, 256, 600, 0, 0, 255, 2])
    cases["count_zero"] = pad_case([0] * 5, [10, 0, 256, 257, 1])
    return cases


def pad_expected(buf, count, seg):
    """The padding of tests/test_gpu_frame_bn.py::test_pad_list_by_segment_against_numpy.
    -> (padded list, tile -> segment, panel start of every segment and the end, in panels of 128 rows)."""
    ids = buf[:count]
    want, want_tiles, want_start = [], [], []
    for f in range(len(seg) - 1):
        part = ids[(ids >= seg[f]) & (ids < seg[f + 1])]
        plen = (len(part) + PAD_ROWS - 1) // PAD_ROWS * PAD_ROWS
        want_start.append(len(want) // PANEL_ROWS)
        want += list(part) + [-1] * (plen - len(part))
        want_tiles += [f] * (plen // PAD_ROWS)
    want_start.append(len(want) // PANEL_ROWS)
    return np.array(want, dtype=np.int32), np.array(want_tiles, dtype=np.int32), np.array(want_start, dtype=np.int32)


# ------------------------------------------------------------------------------------------------ counts
COUNT_SIZES = (0, 1, 3, 4, 5, 4095, 4096, 4097, 16383, 16384, 16385, 65535, 65536, 65537, 65543)
COUNT_THRESHOLD = 60


def count_degrees(n, threshold=COUNT_THRESHOLD):
    """n degrees around the threshold: equal to it (not counted), one above (counted), 0, and others on both sides; the last
    entry is one above, so a lost tail entry changes the sum."""
    i = np.arange(n, dtype=np.int64)
    deg = np.array([threshold, threshold + 1, 0, 1, max(threshold - 1, 0), 3 * threshold + 2, threshold])[(i * 3 + i // 7) % 7]
    if n:
        deg[-1] = threshold + 1
    return deg.astype(np.int32)


def count_expected(deg, threshold):
    return min(int(deg.astype(np.int64)[deg > threshold].sum()), COUNT_SATURATED)


def count_saturating():
    return np.full(4096, 2 ** 20, dtype=np.int32)
