"""Hand-built graphs that sit ON the thresholds of the backward of the fused aggregation M[t] = aggr_e(Q[s_e] + W_e a_e)
(csrc/backward.hip: k_mpnn_bwd_arg / _edge / _src, the lane-local k_mpnn_bwd_dwe_max / _dea_max / _src_max16, k_reduce_slots,
k_segment_reduce_bwd) and of the forward that records the winners (csrc/mpnn.hip, k_mpnn_max<ARG>), the inputs that go with them,
and the reference gradients in int64 / float64.  Shared by tests/test_gpu_mpnn_bwd_edges.py (the kernels against the reference)
and tests/test_mpnn_bwd_cases.py (proof, on the CPU alone, that every case is what it says).  Needs no GPU; deterministic.

A graph here is a ``mpnn_csr_cases.Case`` (CSR by target with chosen in-degrees, a random ``node_order`` and None) extended by
what the backward reads, all of it built in numpy and never by the library's own CSR builder, so that a mistake there cannot
cancel out: the CSR by source as rgnn.h defines it (``rowptr_s`` in visiting order, ``tnode`` = target node, ``tpos`` = position
in the target-sorted list) and the edge maps of ``TargetCSR.edge_maps()`` (``tgt_sorted``, ``eloc_sorted``, ``tloc``).

Integer inputs (Q in [-8, 8], W_e in [-2, 2], a in [-3, 3], dM in [-4, 4] without zeros: a routed gradient is never invisible) in
three winner layouts:
  spread     the forward module's bonus scheme: source s carries BONUS on channel s % d, so wherever a target's sources are
             distinct mod d every edge is the strict unique maximum of at least one channel;
  all_tie    Q constant and W_e a = 0 (W_e is zero on the odd attribute columns, a on the even ones, so that dW_e and
             d_edge_attr both stay visible): the FIRST edge of every segment must win every channel;
  last_wins  attribute 0 of a segment's last edge is LAST_A and W_e[:, 0] = 2: the unique maximum of every channel sits at index
             in-degree - 1 (needs de >= 1).
``negative`` shifts Q by -NEG_SHIFT as in the forward module.  On such data every gradient is a sum of integers (mean on a graph
whose in-degrees are powers of two: of dyadic rationals), and ``grads`` returns next to every output its sum of |terms|:
below 2^24 (times the largest in-degree for mean) the float32 kernels must return the reference bit for bit in any order of
summation."""
import functools
from collections import Counter

import numpy as np
import torch

import mpnn_csr_cases as mc

# constants of csrc/backward.hip and csrc/mpnn.hip, restated by hand (a change there must break a case visibly)
CAP = 128                 # k_mpnn_bwd_dwe_max: edges per pass through LDS
SMALL_PASS = 8            # ... a pass of cnt * DEP <= 64 floats (DEP = 8) takes the one-element-per-lane branch
BUF = 32                  # k_mpnn_bwd_edge: edges whose d_edge_attr rows wait in LDS
BLK = 60                  # k_mpnn_max: edges consumed per block of 64, rows gathered up to five ahead
SRC_BLOCK, SRC_TRIP = 64, 4      # k_mpnn_bwd_src_max16: out-edges per block, per trip
SLOTS_MAX = 2048          # rgnn_mpnn_bwd_slots: n rounded up to 4 below this, 2048 persistent slots from there
SRC_GRID_N, SRC_GRID_BLOCKS = 8192, 2048     # node half: (n + 3) / 4 blocks below 8192 nodes, 2048 from there
DEA_BLOCK, DEA_BLOCKS = 256, 2048            # k_mpnn_bwd_dea_max: edges per block, blocks at most; grid-stride beyond their product
REDUCE_STRIDE, REDUCE_COLS = 32, 64          # k_reduce_slots: slots per trip of a 16-row group (two of them), columns per block
D_MAX, DE_MAX = 1024, 16                     # rgnn_mpnn_aggregate_bwd
LOC_D_MAX, LOC_DE_MAX, LOC_D_STEP = 512, 8, 8    # rgnn_mpnn_max_bwd_supported

BONUS, NEG_SHIFT = mc.BONUS, mc.NEG_SHIFT
LAST_A = 128              # last_wins: 2 * (LAST_A - 3) beats |Q| differences (16) and 15 other attribute columns (12 each)
TIE_Q = 5
LAYOUTS = ("spread", "all_tie", "last_wins")
EXACT_LIMIT = 1 << 24


class Case(mc.Case):
    """``mc.Case`` plus the by-source view of the same edges.  ``src``: the whole source array where no draw will do."""

    def __init__(self, name, deg, d, aim, src=None, spread_exempt=False, **kw):
        if src is None:
            super().__init__(name, deg, d, aim, **kw)
        else:
            deg = np.asarray(deg, dtype=np.int64)
            super().__init__(name, np.zeros_like(deg), d, aim, **kw)          # (the node_order draw of this seed, no edges yet)
            self.rowptr_np = np.concatenate(([0], np.cumsum(deg))).astype(np.int64)
            self.src_np = np.asarray(src, dtype=np.int64)
            self.n_edges = int(self.rowptr_np[-1])
            assert self.src_np.shape == (self.n_edges,)
            self.rowptr_t = torch.from_numpy(self.rowptr_np.astype(np.int32))
            self.src_sorted = torch.from_numpy(self.src_np.astype(np.int32))
            self.exempt = np.zeros(self.n_edges, dtype=bool)
        self.spread_exempt = spread_exempt          # no claim that every edge wins a channel (sources not distinct mod d)

    # ---- per sorted edge
    @property
    def tgt_pos(self):
        return np.repeat(np.arange(self.n), self.deg)

    @property
    def eloc(self):
        return np.arange(self.n_edges) - self.rowptr_np[self.tgt_pos]

    def order_np(self, order):
        return np.arange(self.n) if order is None else order.numpy().astype(np.int64)

    def tgt_node(self, order):
        return self.order_np(order)[self.tgt_pos]

    def out_deg(self):
        return np.bincount(self.src_np, minlength=self.n)

    def source_csr(self, order):
        """(rowptr_s [n + 1] over the visiting order, tnode [E], tpos [E]) as int32 tensors; a source's out-edges in the order of the
        target-sorted list."""
        rank = np.empty(self.n, dtype=np.int64)
        rank[self.order_np(order)] = np.arange(self.n)
        spos = rank[self.src_np]
        tpos = np.argsort(spos, kind="stable")
        rowptr_s = np.concatenate(([0], np.cumsum(np.bincount(spos, minlength=self.n))))
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32))
        return i32(rowptr_s), i32(self.tgt_node(order)[tpos]), i32(tpos)

    def edge_maps(self, order):
        """(tgt_sorted [E], eloc_sorted [E], tloc [E]) as int32 tensors."""
        tpos = self.source_csr(order)[2].numpy().astype(np.int64)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32))
        return i32(self.tgt_node(order)), i32(self.eloc), i32(self.eloc[tpos])

    def inv_deg(self, order):
        """1 / in-degree per NODE (float32; 0 where there is none): ``target_scale`` of the mean backward."""
        out = torch.zeros(self.n, dtype=torch.float32)
        dg = torch.from_numpy(self.deg)
        node = torch.from_numpy(self.order_np(order))
        out[node[dg > 0]] = 1.0 / dg[dg > 0].to(torch.float32)
        return out


# ------------------------------------------------------------------------------------------------ the cases
IN_DEGREES = (1, 7, 8, 9, 31, 32, 33, 59, 60, 61, 63, 64, 65, 119, 120, 121, 127, 128, 129, 136, 137, 255, 256, 257, 300)
OUT_DEGREES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 66, 67, 68, 127, 128, 129, 130)
SLOT_SIZES = (13, 16, 17, 20, 29, 32, 33, 36, 48, 49)
SLOT_WIDTHS = ((1, 1), (21, 3), (8, 8), (13, 5))          # d * de = 1, 63, 64, 65: one block of k_reduce_slots, its last column, two blocks
SEGMENT_SIZES = (2047, 2048, 2049, 4097, 6145)            # 1, 1, 2, 3, 4 segments for the first wave (2048 slots)
SRC_GRID_SIZES = (8191, 8192, 8193)
POW2 = tuple(1 << i for i in range(9))


def _in_degrees(empty_ends):
    body, k = [], 0
    for s in IN_DEGREES:
        body.append(s)
        for _ in range(9):
            body.append(1 + k % 5)
            k += 1
        body += [0, 0]
    deg = [0] + body if empty_ends else body + [3]
    return Case("in_degrees/" + ("empty_ends" if empty_ends else "nonempty_ends"), deg, 512,
                "k_mpnn_bwd_dwe_max: passes of 128 edges, a last pass of 1 .. 8 edges (129 .. 136) on the one-element-per-lane branch, the "
                "prefetch behind either branch; k_mpnn_max: blocks of 60 edges; k_mpnn_bwd_edge: the 32-edge buffer flushed inside a segment",
                seed=21 + empty_ends)


def _out_degrees():
    n = 140
    explicit = {p: [h for h in range(len(OUT_DEGREES)) if p < OUT_DEGREES[h]] for p in range(n)}
    deg = [len(explicit[p]) for p in range(n)]
    return Case("out_degrees", deg, 16, "k_mpnn_bwd_src_max16: out-edges in blocks of 64, trips of 4 whose unused slots repeat the last edge "
                "with the index 0x10000; hub h is a source of position p iff p < out-degree[h]", de=3, explicit=explicit, seed=23)


_TINY = {
    1: ([1], {0: [0]}),                                     # a single self-loop
    2: ([2, 0], {0: [1, 0]}),                               # a single target holding all edges
    3: ([1, 0, 2], {0: [2], 2: [0, 1]}),
    4: ([1, 1, 1, 1], {p: [(p + 1) % 4] for p in range(4)}),
    5: ([0, 2, 0, 3, 0], {1: [0, 4], 3: [2, 1, 3]}),
}


def _tiny(n):
    deg, explicit = _TINY[n]
    return Case(f"tiny/{n}", deg, 8, "rgnn_mpnn_bwd_slots: 4 or 8 slots, waves without a segment store zeros", explicit=explicit, seed=30 + n)


def _slots(n):
    return Case(f"slots/{n}", 1 + np.arange(n) % 2, 8, "k_reduce_slots: strides of 32 slots with a tail of up to 16 + 16, 64 columns per block",
                seed=40 + n)


def _many_segments(n):
    deg = np.arange(n) % 6
    for i in range(8):
        deg[100 + 97 * i] = 33 + i
    return Case(f"many_segments_per_wave/{n}", deg, 64, "k_mpnn_bwd_edge: the three-deep pipeline m0 / m1 / m2 over 1 .. 4 segments per wave, "
                "the 32-edge buffer carried across segments; k_mpnn_bwd_dwe_max: pn < n", seed=50 + n % 7)


def _src_grid(n):
    return Case(f"src_grid/{n}", 1 + np.arange(n) % 3, 4, "node half: (n + 3) / 4 blocks below 8192 nodes, 2048 grid-striding blocks from there",
                de=2, seed=60 + n % 5)


def _dea_grid_stride():
    n, k = 8200, 64
    src = (np.arange(n * k) * 13 + 5) % n                   # 64 distinct sources per target, every node 64 out-edges
    return Case("dea_grid_stride", np.full(n, k), 8, "k_mpnn_bwd_dea_max: E = 524 800 > 2048 blocks x 256 edges: the grid-stride trip",
                src=src, de=1, seed=70, spread_exempt=True)


def _multi():
    n = 300
    deg = 1 + (np.arange(n) % 5)
    explicit = {10: [5, 5, 5, 9], 20: [20], 21: [21, 22, 21], 30: 30 + np.arange(8), 31: [31, 31], 299: [299, 0]}
    for p, s in explicit.items():
        deg[p] = len(s)
    return Case("multi_edges_and_self_loops", deg, 32, "duplicate (source, target) pairs tie exactly: the first copy wins; a node among its own sources",
                explicit=explicit, seed=80, exempt_duplicates=True)


def _no_edges():
    return Case("no_edges", np.zeros(100, dtype=np.int64), 32, "E = 0: zeros and nothing else", seed=81)


def _empty_then_full():
    return Case("empty_then_full", np.concatenate((np.zeros(199, dtype=np.int64), [129])), 256,
                "a run of 199 empty targets, then one of 129 edges at the last position (one full pass and one edge)", seed=82)


def _pow2():
    deg = np.zeros(300, dtype=np.int64)
    deg[1::3] = 1
    deg[2::6] = 2
    deg[5::12] = 4
    for i, k in enumerate(POW2):
        deg[30 * i] = k
    return Case("pow2_degrees", deg, 256, "mean: every non-zero in-degree a power of two (1 .. 256), 1 / deg exact", seed=83)


_BUILDERS = {
    "in_degrees/nonempty_ends": lambda: _in_degrees(False),
    "in_degrees/empty_ends": lambda: _in_degrees(True),
    "out_degrees": _out_degrees,
    **{f"tiny/{n}": (lambda n=n: _tiny(n)) for n in _TINY},
    **{f"slots/{n}": (lambda n=n: _slots(n)) for n in SLOT_SIZES},
    **{f"many_segments_per_wave/{n}": (lambda n=n: _many_segments(n)) for n in SEGMENT_SIZES},
    **{f"src_grid/{n}": (lambda n=n: _src_grid(n)) for n in SRC_GRID_SIZES},
    "dea_grid_stride": _dea_grid_stride,
    "multi_edges_and_self_loops": _multi,
    "no_edges": _no_edges,
    "empty_then_full": _empty_then_full,
    "pow2_degrees": _pow2,
}
NAMES = tuple(_BUILDERS)
IN_DEGREE_CASES = ("in_degrees/nonempty_ends", "in_degrees/empty_ends")
TINY_CASES = tuple(f"tiny/{n}" for n in _TINY)
SLOT_CASES = tuple(f"slots/{n}" for n in SLOT_SIZES)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


# the degree multisets every case claims, written out independently of the builders: {degree: nodes}
def _claim_in_degrees(empty_ends):
    c = Counter({k: 45 for k in range(1, 6)})               # 25 x 9 ordinary targets, 1 .. 5 in turn
    c.update(IN_DEGREES)
    c[0] = 50 + (1 if empty_ends else 0)
    if not empty_ends:
        c[3] += 1
    return dict(c)


def _claim_many_segments(n):
    c = Counter({k: n // 6 + (1 if k < n % 6 else 0) for k in range(6)})
    for i, k in enumerate((4, 5, 0, 1, 2, 3, 4, 5)):        # (100 + 97 i) % 6
        c[k] -= 1
        c[33 + i] += 1
    return dict(c)


def _claim_multi():
    c = Counter({k: 60 for k in range(1, 6)})
    for p, k in ((10, 4), (20, 1), (21, 3), (30, 8), (31, 2), (299, 2)):
        c[1 + p % 5] -= 1
        c[k] += 1
    return dict(c)


CLAIMED_IN_DEGREES = {
    "in_degrees/nonempty_ends": _claim_in_degrees(False),
    "in_degrees/empty_ends": _claim_in_degrees(True),
    "out_degrees": {15: 1, 14: 1, 13: 1, 12: 1, 11: 1, 10: 58, 9: 1, 8: 1, 7: 1, 6: 1, 5: 1, 4: 59, 3: 1, 2: 1, 1: 1, 0: 10},
    "tiny/1": {1: 1}, "tiny/2": {2: 1, 0: 1}, "tiny/3": {1: 1, 0: 1, 2: 1}, "tiny/4": {1: 4}, "tiny/5": {0: 3, 2: 1, 3: 1},
    **{f"slots/{n}": {1: (n + 1) // 2, 2: n // 2} for n in SLOT_SIZES},
    **{f"many_segments_per_wave/{n}": _claim_many_segments(n) for n in SEGMENT_SIZES},
    **{f"src_grid/{n}": {1 + k: n // 3 + (1 if k < n % 3 else 0) for k in range(3)} for n in SRC_GRID_SIZES},
    "dea_grid_stride": {64: 8200},
    "multi_edges_and_self_loops": _claim_multi(),
    "no_edges": {0: 100},
    "empty_then_full": {0: 199, 129: 1},
    "pow2_degrees": None,                                    # (checked as a set: {0} + the powers of two, each of 1 .. 256 present)
}
# out-degrees, for the cases that choose them (in the others the sources are drawn; their multiset only has to add up to E)
CLAIMED_OUT_DEGREES = {
    "out_degrees": {**{k: 1 for k in OUT_DEGREES if k}, 0: 140 - 15},
    "tiny/1": {1: 1}, "tiny/2": {1: 2}, "tiny/3": {1: 3}, "tiny/4": {1: 4}, "tiny/5": {1: 5},
    "dea_grid_stride": {64: 8200},
    "no_edges": {0: 100},
}
SPREAD_EXEMPT = ("dea_grid_stride",)                        # ... and the copies in multi_edges_and_self_loops (Case.exempt)


# ------------------------------------------------------------------------------------------------ inputs
def grad_inputs(c, d=None, seed=0):
    """dM [n, d] int64 in [-4, 4] without zeros."""
    d = c.d if d is None else d
    g = torch.Generator().manual_seed(4242 + seed + 7 * d)
    mag = torch.randint(1, 5, (c.n, d), generator=g, dtype=torch.int64)
    sign = torch.randint(0, 2, (c.n, d), generator=g, dtype=torch.int64) * 2 - 1
    return mag * sign


def int_inputs(c, layout="spread", d=None, de=None, negative=False, seed=0):
    """(Q [n, d], We [d, de] or None, ea [E, de] or None, dM [n, d]) as int64 tensors; see the module docstring."""
    assert layout in LAYOUTS
    Q, We, ea, _ = mc.int_inputs(c, d=d, de=de, with_bias=False, negative=negative, seed=seed)
    d = Q.shape[1]
    if layout == "all_tie":
        Q = torch.full_like(Q, TIE_Q - (NEG_SHIFT if negative else 0))
        if We is not None:
            We[:, 1::2] = 0
            ea[:, 0::2] = 0                                  # (de = 1: a = 0, dW_e = 0 is all there is to see of it)
    elif layout == "last_wins":
        assert We is not None, "last_wins needs an attribute column"
        s = torch.arange(c.n)
        Q[s, s % d] -= BONUS                                 # no bonus: the attributes decide
        We[:, 0] = 2
        last = torch.from_numpy(c.rowptr_np[1:][c.deg > 0] - 1)
        ea[last, 0] = LAST_A
    return Q, We, ea, grad_inputs(c, d, seed)


def float_inputs(c, d=None, de=None, seed=0):
    """``mc.float_inputs`` (magnitudes over four decades across the channels) without the bias, plus a float32 dM."""
    Q, We, ea, _ = mc.float_inputs(c, d=d, de=de, seed=seed)
    g = torch.Generator().manual_seed(313 + seed + Q.shape[1])
    return Q, We, ea, torch.randn(c.n, Q.shape[1], generator=g)


# ------------------------------------------------------------------------------------------------ reference
def first_id(c, Q, We, ea, order=None, dtype=torch.int64):
    """-> (loc [n, d] int64 per NODE: the lowest in-segment index that attains the maximum of Q[s_e] + W_e a_e, -1 on nodes
    without in-edges; strict [n, d] bool: that maximum is attained once)."""
    d = Q.shape[1]
    loc = torch.full((c.n, d), -1, dtype=torch.int64)
    strict = torch.zeros((c.n, d), dtype=torch.bool)
    if c.n_edges == 0:
        return loc, strict
    msg = mc._messages(c, Q, We, ea, dtype)
    node = torch.from_numpy(c.tgt_node(order))
    idx = node[:, None].expand(-1, d)
    top = torch.zeros((c.n, d), dtype=dtype).scatter_reduce_(0, idx, msg, "amax", include_self=False)
    at_top = msg == top[node]
    el = torch.from_numpy(c.eloc)[:, None].expand(-1, d)
    big = torch.iinfo(torch.int64).max
    low = torch.full((c.n, d), big, dtype=torch.int64).scatter_reduce_(0, idx, torch.where(at_top, el, big), "amin", include_self=True)
    has = torch.zeros(c.n, dtype=torch.bool)
    has[node] = True
    loc[has] = low[has]
    strict[has] = (torch.zeros((c.n, d), dtype=torch.int64).scatter_add_(0, idx, at_top.to(torch.int64)) == 1)[has]
    return loc, strict


def edge_gradient(c, dM, aggr, order=None, loc=None, dtype=torch.float64):
    """G [E, d]: what edge e receives of dM[target of e] -- max: the channels whose winner ``loc`` names it; mean: 1 / in-degree of
    it; add: all of it."""
    node = torch.from_numpy(c.tgt_node(order))
    G = dM.to(dtype)[node]
    if aggr == "max":
        G = torch.where(loc[node] == torch.from_numpy(c.eloc)[:, None], G, torch.zeros((), dtype=dtype))
    elif aggr == "mean":
        G = G / torch.from_numpy(c.deg[c.tgt_pos]).to(dtype)[:, None]
    return G


def grads(c, dM, We, ea, aggr, order=None, loc=None, dtype=torch.float64):
    """-> ((dQ [n, d], d_edge_attr [E, de] or None, dW_e [d, de] or None), the same three as sums of |terms|), all in ``dtype``
    (float64: exact on the integer data of this module, every partial sum is far below 2^53; cast with ``.to(torch.int64)``).
    max: routed through the winners ``loc`` ([n, d] per node, in-segment indices)."""
    out = []
    for absolute in (False, True):
        f = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))
        G = edge_gradient(c, dM, aggr, order, loc, dtype)
        G = G.abs() if absolute else G
        dQ = torch.zeros((c.n, dM.shape[1]), dtype=dtype).index_add_(0, torch.from_numpy(c.src_np), G)
        if We is None or ea is None or ea.shape[1] == 0:
            out.append((dQ, None, None))
        else:
            out.append((dQ, G @ f(We), G.t() @ f(ea)))
    return out[0], out[1]


def naive_grads(c, Q, We, ea, dM, aggr, order=None):
    """The same gradients by a per-edge Python loop over exact integers / fractions scaled by the in-degree (numpy int64 rows).
    mean is returned times the least common multiple of the in-degrees -> (dQ, dea, dWe, loc, scale)."""
    d = Q.shape[1]
    de = 0 if ea is None else ea.shape[1]
    Qn, dMn = Q.numpy(), dM.numpy()
    Wn = None if We is None else We.numpy()
    an = None if ea is None else ea.numpy()
    nodes = c.order_np(order)
    scale = int(np.lcm.reduce(c.deg[c.deg > 0])) if (aggr == "mean" and c.n_edges) else 1
    dQ = np.zeros((c.n, d), dtype=np.int64)
    dea = np.zeros((c.n_edges, de), dtype=np.int64)
    dWe = np.zeros((d, de), dtype=np.int64)
    loc = np.full((c.n, d), -1, dtype=np.int64)
    for p in range(c.n):
        r0, r1 = int(c.rowptr_np[p]), int(c.rowptr_np[p + 1])
        t = int(nodes[p])
        best = None
        for e in range(r0, r1):
            m = Qn[c.src_np[e]].copy()
            if de:
                m += Wn @ an[e]
            if best is None:
                best, loc[t] = m, 0
            else:
                better = m > best
                best = np.where(better, m, best)
                loc[t][better] = e - r0
        for e in range(r0, r1):
            if aggr == "max":
                g = np.where(loc[t] == e - r0, dMn[t], 0)
            else:
                g = dMn[t] * (scale // (r1 - r0) if aggr == "mean" else 1)
            dQ[c.src_np[e]] += g
            if de:
                dea[e] = g @ Wn
                dWe += np.outer(g, an[e])
    return dQ, dea, dWe, loc, scale


# ------------------------------------------------------------------------------------------------ segment_reduce_bwd
def row_inputs(c, d, seed=0):
    """(rows [E, d] int64 in [-3, 3]: exact ties in nearly every segment of two or more rows, dM [n, d])."""
    g = torch.Generator().manual_seed(555 + seed + d)
    return torch.randint(-3, 4, (c.n_edges, d), generator=g, dtype=torch.int64), grad_inputs(c, d, seed)


def segment_reduce_grads(c, rows, dM, aggr, order=None, dtype=torch.float64):
    """d_rows [E, d]: max -- dM[t, c] to the first row of the segment that attains the maximum, 0 to the others."""
    loc = None
    if aggr == "max":
        d = rows.shape[1]
        node = torch.from_numpy(c.tgt_node(order))
        idx = node[:, None].expand(-1, d)
        top = torch.zeros((c.n, d), dtype=rows.dtype).scatter_reduce_(0, idx, rows, "amax", include_self=False)
        el = torch.from_numpy(c.eloc)[:, None].expand(-1, d)
        big = torch.iinfo(torch.int64).max
        loc = torch.full((c.n, d), big, dtype=torch.int64).scatter_reduce_(0, idx, torch.where(rows == top[node], el, big), "amin")
    return edge_gradient(c, dM, aggr, order, loc, dtype)
