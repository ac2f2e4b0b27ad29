"""Hand-built CSRs-by-target that sit ON the thresholds of the window form of the max aggregation and of its plan
(csrc/mpnn_tiles.hip), the inputs that go with them, and the reference M[t] = b + max_e(Q[s_e] + W_e a_e) in three
precisions.  Shared by tests/test_gpu_mpnn_win_edges.py (the kernels against the reference) and
tests/test_mpnn_csr_cases.py (proof, on the CPU alone, that every case is what it says and reaches the line it names).
Needs no GPU.  Everything is deterministic (fixed PCG64 seeds).

Every graph the other tests hand to the plan comes out of the project's own neighbour search; these do not: in-degrees
are chosen one by one, sources are placed so that a window holds exactly as many distinct rows as the case needs.

Integer inputs: Q, W_e, a and b hold small integers, so the three-term bf16 split of the kernel is exact and every sum
stays far below 2^24 -- the kernels must return the int64 reference bit for bit.  Every source s carries a bonus of
BONUS on channel s % d, and a target's sources are distinct mod d at the case's own width: every edge is then the strict
unique maximum of at least one output element (``edge_win_counts``), so no edge can be dropped, mispaired or replaced by
a neighbour without changing an output.  The ``negative`` variant shifts every message below zero: a padded slot filled
with zero instead of a repeated edge would win every maximum."""
import functools
from collections import Counter

import numpy as np
import torch

# constants of csrc/mpnn_tiles.hip, restated by hand (a change there must break the cases visibly, not move them along)
WN_PAD = 4            # :139  a target's slots are padded to a multiple of this
WN_STREAM = 64        # :422  WN_BIG: slots per stream; more padded slots than this -> the per-target kernel
WN_STREAMS = 8        # :84   WN_SLOTS = 512 = 8 streams x 64
WN_SEG = 512          # :424  positions per greedy segment; a window never spans two
WN_UMAX = 176         # :144  distinct source rows a window may hold; more -> the whole window goes per target
WN_SCAN_THREADS = 1024  # :505 k_win_segbase: per = ceil(n_seg / 1024) segments per thread
WN_TICKET_BLOCKS = 768  # :823-825 256 * per_cu work-groups at most: more windows than this and every queue hands out several each
HASH_MUL, HASH_SHIFT, HASH_SIZE = 2654435761, 22, 1024     # :613 bucket of a source id in k_win_pack's table
LEFT_BLOCK, LEFT_REQ = 64, 8                               # :686, :693 k_win_leftover: edges per block, rows per request
TILE_CHANNELS, LEFT_CHANNELS, D_MAX, DE_MAX = 32, 512, 2048, 8   # :8, :669, :794

BONUS = 1000          # on channel s % d of source s: beats |Q| <= 8 plus |W a| <= 8 * 2 * 3
NEG_SHIFT = 4096      # the negative variant: every message <= 8 + BONUS + 48 - 4096 < 0
GROUP = 128           # consecutive positions that draw their sources from one pool of ids (a window holds <= 128 targets)


class Case:
    def __init__(self, name, deg, d, aim, de=8, explicit=None, focus=None, seed=0, order=True, exempt_duplicates=False):
        self.name, self.aim, self.d, self.de, self.focus = name, aim, int(d), int(de), focus
        deg = np.asarray(deg, dtype=np.int64)
        self.n = int(deg.shape[0])
        rng = np.random.Generator(np.random.PCG64(9000 + seed))
        self.rowptr_np = np.concatenate(([0], np.cumsum(deg))).astype(np.int64)
        self.src_np = _sources(rng, deg, self.rowptr_np, self.d, explicit or {})
        self.n_edges = int(self.rowptr_np[-1])
        self.rowptr_t = torch.from_numpy(self.rowptr_np.astype(np.int32))
        self.src_sorted = torch.from_numpy(self.src_np.astype(np.int32))
        self.node_order = torch.from_numpy(rng.permutation(self.n).astype(np.int32)) if order else None
        # edges that cannot be a strict winner by construction: copies of one (target, source) pair
        self.exempt = np.zeros(self.n_edges, dtype=bool)
        if exempt_duplicates:
            tgt = np.repeat(np.arange(self.n), deg)
            key = tgt * self.n + self.src_np
            _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
            self.exempt = cnt[inv] > 1

    @property
    def deg(self):
        return np.diff(self.rowptr_np)

    def orders(self):
        """(None, the random permutation): both ``node_order`` variants of the case."""
        return (None, self.node_order)


def _sources(rng, deg, rowptr, d, explicit):
    """Sources of every target: ``explicit[p]`` where given; otherwise deg[p] distinct ids out of a run of consecutive ids (distinct
    mod d: the run is no longer than d) that the GROUP positions around p share -- a window's distinct rows stay far below WN_UMAX
    unless a case says otherwise.  Targets that fit a stream draw from a run of min(d, 64) ids, larger ones from d."""
    n = deg.shape[0]
    src = np.zeros(int(rowptr[-1]), dtype=np.int64)
    small = min(d, WN_STREAM, n)
    for width, sel in ((small, (deg > 0) & (deg <= small)), (min(d, n), deg > small)):
        pos = np.nonzero(sel)[0]
        pos = pos[[p not in explicit for p in pos]] if explicit else pos
        if pos.size == 0:
            continue
        assert int(deg[pos].max()) <= width, "in-degree beyond the case's channel count: sources cannot be distinct mod d"
        offs = np.argsort(rng.random((pos.size, width)), axis=1)[:, :int(deg[pos].max())]
        base = ((pos // GROUP) * 61) % (n - width + 1)
        take = np.arange(offs.shape[1])[None, :] < deg[pos][:, None]
        src[(rowptr[pos][:, None] + np.arange(offs.shape[1])[None, :])[take]] = (base[:, None] + offs)[take]
    for p, s in explicit.items():
        s = np.asarray(s, dtype=np.int64)
        assert s.shape[0] == deg[p]
        src[rowptr[p]:rowptr[p + 1]] = s
    return src


# ------------------------------------------------------------------------------------------------ the plan, restated
def pad4(deg):
    return (np.asarray(deg) + WN_PAD - 1) // WN_PAD * WN_PAD


def first_fit(rowptr):
    """The plan's packing in Python: per segment of WN_SEG positions, in order, a target of pd = pad4(in-degree) slots goes
    into the first of the open window's WN_STREAMS streams with fill + pd <= WN_STREAM; when none has room the window closes and
    the target opens the next.  -> (windows: list of lists of (position, stream, first slot); positions with pd > WN_STREAM)."""
    deg = np.diff(np.asarray(rowptr))
    pd = pad4(deg)
    windows, big = [], [int(p) for p in np.nonzero(pd > WN_STREAM)[0]]
    placed = np.nonzero((pd > 0) & (pd <= WN_STREAM))[0]
    seg_of = placed // WN_SEG
    cur, fill, cur_seg = None, None, -1
    for p, s in zip(placed.tolist(), seg_of.tolist()):
        if s != cur_seg:
            if cur:
                windows.append(cur)
            cur, fill, cur_seg = [], [0] * WN_STREAMS, s
        size = int(pd[p])
        b = next((i for i in range(WN_STREAMS) if fill[i] + size <= WN_STREAM), None)
        if b is None:
            windows.append(cur)
            cur, fill, b = [], [0] * WN_STREAMS, 0
        cur.append((p, b, fill[b]))
        fill[b] += size
    if cur:
        windows.append(cur)
    return windows, big


def window_sources(case, window):
    """Distinct sources of a window of ``first_fit``."""
    return np.unique(np.concatenate([case.src_np[case.rowptr_np[p]:case.rowptr_np[p + 1]] for p, _, _ in window]))


def window_of(windows, position):
    hit = [w for w in windows if any(p == position for p, _, _ in w)]
    assert len(hit) == 1
    return hit[0]


def per_target_expected(case):
    """(targets the per-target kernel takes, windows made): too large for a stream, or in a window of more than WN_UMAX rows."""
    windows, big = first_fit(case.rowptr_np)
    spilled = sum(len(w) for w in windows if window_sources(case, w).shape[0] > WN_UMAX)
    return len(big) + spilled, len(windows)


def n_win_bound(n, n_edges):
    """Windows the plan allocates (win_layout, :435): numbers at or beyond it are dropped by k_win_starts without a word."""
    return (n_edges + 3 * n) // 256 + (n + WN_SEG - 1) // WN_SEG + 2


def hash_bucket(s):
    return ((np.asarray(s, dtype=np.uint64) * np.uint64(HASH_MUL)) & np.uint64(0xffffffff)) >> np.uint64(HASH_SHIFT)


# ------------------------------------------------------------------------------------------------ the cases
def _ordinary(n):
    """In-degrees 1 .. 5 in turn: ordinary windows around the one a case is about."""
    return 1 + (np.arange(n) % 5)


def _degrees_1_to_8(empty_ends):
    reps = 60                                   # 540 positions: crosses a segment boundary
    if empty_ends:
        deg = np.concatenate((np.tile(np.arange(9), reps), [0]))
    else:
        deg = np.tile(np.r_[1:9, 0], reps)[:-1]
    return Case("degrees_1_to_8/" + ("empty_ends" if empty_ends else "nonempty_ends"), deg, 32,
                "k_win_pack: slots min(q, d - 1) of a target of 1 .. 8 edges, pd - d = 0 .. 3 repeated slots; first / last position "
                + ("empty" if empty_ends else "non-empty"), seed=1 + empty_ends)


def _stream_edge():
    body = np.ravel([[k, 1] for k in (60, 61, 63, 64, 65, 68, 69)] * 3)
    deg = np.concatenate((body, np.zeros(128 - body.shape[0], dtype=np.int64)))    # (isolated nodes: the big rows need 80 ids to name)
    return Case("stream_edge", deg, 80, "k_win_pdeg: pd > WN_BIG -- 61 .. 64 edges fill a stream alone, 65 is the per-target kernel's first", seed=3)


def _leftover_blocks():
    deg = _ordinary(1100)
    for i, k in enumerate((65, 71, 72, 73, 127, 128, 129, 1000)):
        deg[40 + 37 * i] = k
    return Case("leftover_blocks", deg, 1024, "k_win_leftover: blocks of 64 edges, 8 rows per request, the tail repeats the last edge", seed=4)


def _all_33():
    return Case("all_33", np.full(600, 33), 64, "win_layout: n_win -- 36 padded slots, one target per stream, 288 slots per closed window", seed=5)


def _all_1(n):
    return Case(f"all_1/{n}", np.ones(n, dtype=np.int64), 32,
                "k_win_greedy / k_win_starts: 128 targets per window, four windows per full segment"
                + ("; more windows than work-groups: every ticket queue wraps" if n > 128 * WN_TICKET_BLOCKS else "; segment edge"), seed=6)


def _distinct(extra):
    n = 3 * WN_SEG
    deg = _ordinary(n)
    deg[WN_SEG:2 * WN_SEG] = 0
    first = WN_SEG
    explicit = {}
    for i in range(44):
        deg[first + i] = 4
        explicit[first + i] = 600 + 4 * i + np.arange(4)             # 176 ids, four consecutive per target
    if extra:
        deg[first + 44] = 1
        explicit[first + 44] = [600 + 176]
    return Case("distinct_177" if extra else "distinct_176", deg, 32,
                "k_win_pack: nU > WN_UMAX -- " + ("177 rows: the window's 45 targets go per target" if extra else "176 rows: the window stays"),
                explicit=explicit, focus=first, seed=7)


def _one_source():
    n = WN_SEG
    explicit = {p: [77] for p in range(128, 256)}
    explicit.update({p: [300 + 5 * (p % 9)] for p in range(256, 384)})
    return Case("one_source", np.ones(n, dtype=np.int64), 32, "k_win_pack: nU = 1 (7 filler row ids) and nU = 9 (7 filler row ids)",
                explicit=explicit, focus=128, seed=8)


@functools.lru_cache(maxsize=None)
def _hash_chain_ids(n):
    b = hash_bucket(np.arange(n))
    counts = np.bincount(b.astype(np.int64), minlength=HASH_SIZE)
    ids = np.nonzero(b == np.uint64(int(np.argmax(counts))))[0]
    groups = [[] for _ in range(44)]                                 # four ids per target, distinct mod 32
    for s in ids.tolist():
        g = next((g for g in groups if len(g) < 4 and all((s - t) % 32 for t in g)), None)
        if g is not None:
            g.append(s)
    assert all(len(g) == 4 for g in groups), "not enough ids below n in one bucket"
    return groups


def _hash_chain():
    n = 392 * WN_SEG                                                 # 200 704 ids: ~196 per bucket
    deg = np.zeros(n, dtype=np.int64)
    deg[:WN_SEG] = _ordinary(WN_SEG)
    deg[2 * WN_SEG:3 * WN_SEG] = _ordinary(WN_SEG)
    explicit = {}
    for i, g in enumerate(_hash_chain_ids(n)):
        deg[WN_SEG + i] = 4
        explicit[WN_SEG + i] = g
    return Case("hash_chain", deg, 32, "k_win_pack: 176 sources in ONE bucket of the open-addressing table: probe chains up to 175 long",
                explicit=explicit, focus=WN_SEG, seed=9)


def _multi_edges_and_self_loops():
    n = 300
    deg = _ordinary(n)
    explicit = {10: [5, 5, 5, 9], 20: [20], 21: [21, 22, 21], 30: 30 + np.arange(8), 31: [31, 31], 299: [299, 0]}
    for p, s in explicit.items():
        deg[p] = len(s)
    return Case("multi_edges_and_self_loops", deg, 32, "k_win_pack: one local row for several slots of a target; a target's own row among its sources",
                explicit=explicit, seed=10, exempt_duplicates=True)


def _many_segments():
    n = 1025 * WN_SEG + 7
    p = np.arange(n)
    deg = np.where(p % 7 == 0, 1 + (p // 7) % 5, 0)
    return Case("many_segments", deg, 32, "k_win_segbase: per = 2 segments per thread (more than 1024 segments)", de=2, seed=11)


def _empty_parts(which):
    if which == "no_edges":
        deg = np.zeros(100, dtype=np.int64)
    else:
        deg = np.concatenate((np.zeros(WN_SEG, dtype=np.int64), 1 + np.arange(WN_SEG) % 3, [3]))
    return Case("empty_graph_parts/" + which, deg, 32,
                "E = 0: nothing but the zero rows" if which == "no_edges" else
                "k_win_greedy: segcnt = 0 for a segment without edges, a full one behind it, a last segment of one position", seed=12)


ALL_1_SIZES = (511, 512, 513, 1025, 128 * WN_TICKET_BLOCKS + 1500)
_BUILDERS = {
    "degrees_1_to_8/nonempty_ends": lambda: _degrees_1_to_8(False),
    "degrees_1_to_8/empty_ends": lambda: _degrees_1_to_8(True),
    "stream_edge": _stream_edge,
    "leftover_blocks": _leftover_blocks,
    "all_33": _all_33,
    **{f"all_1/{n}": (lambda n=n: _all_1(n)) for n in ALL_1_SIZES},
    "distinct_176": lambda: _distinct(False),
    "distinct_177": lambda: _distinct(True),
    "one_source": _one_source,
    "hash_chain": _hash_chain,
    "multi_edges_and_self_loops": _multi_edges_and_self_loops,
    "many_segments": _many_segments,
    "empty_graph_parts/no_edges": lambda: _empty_parts("no_edges"),
    "empty_graph_parts/empty_full_one": lambda: _empty_parts("empty_full_one"),
}
NAMES = tuple(_BUILDERS)
# the in-degree multiset every case claims, written out independently of the builders: {in-degree: targets}
CLAIMED_DEGREES = {
    "degrees_1_to_8/nonempty_ends": {**{k: 60 for k in range(1, 9)}, 0: 59},
    "degrees_1_to_8/empty_ends": {**{k: 60 for k in range(1, 9)}, 0: 61},
    "stream_edge": {**{k: 3 for k in (60, 61, 63, 64, 65, 68, 69)}, 1: 21, 0: 128 - 42},
    "leftover_blocks": {**{k: 1 for k in (65, 71, 72, 73, 127, 128, 129, 1000)}, 1: 220 - 2, 2: 220 - 1, 3: 220 - 2, 4: 220 - 1, 5: 220 - 2},
    "all_33": {33: 600},
    **{f"all_1/{n}": {1: n} for n in ALL_1_SIZES},
    "distinct_176": {0: 512 - 44, 4: 44 + 204, 1: 206, 2: 205, 3: 204, 5: 205},
    "distinct_177": {0: 512 - 45, 4: 44 + 204, 1: 1 + 206, 2: 205, 3: 204, 5: 205},
    "one_source": {1: 512},
    "hash_chain": {0: 389 * 512 + 512 - 44, 4: 44 + 204, 1: 206, 2: 206, 3: 204, 5: 204},
    "multi_edges_and_self_loops": None,        # (filled in below: the ordinary 1 .. 5 pattern with six rows replaced)
    "many_segments": None,
    "empty_graph_parts/no_edges": {0: 100},
    "empty_graph_parts/empty_full_one": {0: 512, 1: 171, 2: 171, 3: 170 + 1},
}


def _claim_multi():
    c = Counter({k: 60 for k in range(1, 6)})
    for p, k in ((10, 4), (20, 1), (21, 3), (30, 8), (31, 2), (299, 2)):
        c[1 + p % 5] -= 1
        c[k] += 1
    return dict(c)


def _claim_many_segments():
    t = (1025 * WN_SEG + 7 + 6) // 7            # every 7th position, in-degrees 1 .. 5 in turn
    c = {1 + k: t // 5 + (1 if k < t % 5 else 0) for k in range(5)}
    c[0] = 1025 * WN_SEG + 7 - t
    return c


CLAIMED_DEGREES["multi_edges_and_self_loops"] = _claim_multi()
CLAIMED_DEGREES["many_segments"] = _claim_many_segments()


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


# ------------------------------------------------------------------------------------------------ inputs
def int_inputs(c, d=None, de=None, with_bias=True, negative=False, seed=0):
    """(Q [n, d], We [d, de] or None, ea [E, de] or None, b [d] or None) as int64 tensors of small integers; see the module docstring."""
    d = c.d if d is None else d
    de = c.de if de is None else de
    g = torch.Generator().manual_seed(77 + seed + 13 * d + de)
    Q = torch.randint(-8, 9, (c.n, d), generator=g, dtype=torch.int64)
    s = torch.arange(c.n)
    Q[s, s % d] += BONUS
    if negative:
        Q -= NEG_SHIFT
    We = torch.randint(-2, 3, (d, de), generator=g, dtype=torch.int64) if de else None
    ea = torch.randint(-3, 4, (c.n_edges, de), generator=g, dtype=torch.int64) if de else None
    b = torch.randint(-4, 5, (d,), generator=g, dtype=torch.int64) if with_bias else None
    return Q, We, ea, b


def float_inputs(c, d=None, de=None, seed=0):
    """Random float32 inputs whose magnitudes run over four decades across the channels (1e-2 .. 1e2)."""
    d = c.d if d is None else d
    de = c.de if de is None else de
    g = torch.Generator().manual_seed(991 + seed + d)
    scale = torch.logspace(-2, 2, d)[torch.randperm(d, generator=g)]
    Q = torch.randn(c.n, d, generator=g) * scale
    We = torch.randn(d, de, generator=g) * scale[:, None] * 0.5
    ea = torch.randn(c.n_edges, de, generator=g)
    b = torch.randn(d, generator=g) * scale
    return Q, We, ea, b


# ------------------------------------------------------------------------------------------------ reference
def _messages(c, Q, We, ea, dtype):
    msg = Q.to(dtype)[torch.from_numpy(c.src_np)]
    if ea is not None and We is not None and ea.shape[1] > 0:
        msg = msg + ea.to(dtype) @ We.to(dtype).t()
    return msg


def _targets(c, order):
    tgt = torch.repeat_interleave(torch.arange(c.n), torch.from_numpy(c.deg))
    return tgt if order is None else order.long()[tgt]


def reference(c, Q, We, ea, b, order=None, dtype=torch.float64):
    """-> (M [n, d] in ``dtype``, has [n] bool): M[node] = b + max over the in-edges of (Q[s_e] + W_e a_e), rows without edges 0, in
    the arithmetic of ``dtype`` (torch.int64 on integer data, torch.float64, or torch.float32: the plain torch evaluation that the
    kernel's error is measured against).  ``order``: position -> node, as the kernels take it."""
    d = Q.shape[1]
    node = _targets(c, order)
    out = torch.zeros((c.n, d), dtype=dtype)
    has = torch.zeros(c.n, dtype=torch.bool)
    if c.n_edges:
        msg = _messages(c, Q, We, ea, dtype)
        out.scatter_reduce_(0, node[:, None].expand(-1, d), msg, "amax", include_self=False)
        has[node] = True
        if b is not None:
            out[has] += b.to(dtype)
    return out, has


def error_scale(c, Q, We, ea, b, order=None):
    """S[node, c] = max_e(|Q[s_e, c]| + sum_k |W[c, k]| |a[e, k]|) + |b[c]| in float64: what an element-wise error is divided by."""
    S, has = reference(c, Q.double().abs(), None if We is None else We.double().abs(), None if ea is None else ea.double().abs(),
                       None if b is None else b.double().abs(), order, torch.float64)
    return S, has


def edge_win_counts(c, Q, We, ea, b=None):
    """Per edge: the number of channels on which that edge ALONE attains its target's maximum (integer data, int64)."""
    if c.n_edges == 0:
        return torch.zeros(0, dtype=torch.int64)
    tgt = _targets(c, None)
    msg = _messages(c, Q, We, ea, torch.int64)
    d = msg.shape[1]
    idx = tgt[:, None].expand(-1, d)
    top = torch.zeros((c.n, d), dtype=torch.int64).scatter_reduce_(0, idx, msg, "amax", include_self=False)
    at_top = msg == top[tgt]
    ties = torch.zeros((c.n, d), dtype=torch.int64).scatter_add_(0, idx, at_top.to(torch.int64))
    return (at_top & (ties[tgt] == 1)).sum(1)
