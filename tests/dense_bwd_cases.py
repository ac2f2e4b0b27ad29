"""Hand-built operands that sit ON the edges of the dense half of the backward pass -- the weight gradient dW = G^T [A1 | A2 | 1]
(csrc/wgrad.hip: k_wgrad_x3<false> bf16x3, k_wgrad_x3<true> f16x2, the three k_wgrad_narrow instances, k_wg_reduce), the ReLU and
BatchNorm backward (csrc/backward.hip: k_relu_bwd, k_bn_bwd_stats, k_bn_bwd_apply<VEC>) and its coefficients (csrc/norm.hip:
k_bn_bwd_coef, k_bn_bwd_coef4) -- with their references in int64 / float64.  Shared by tests/test_gpu_wgrad_edges.py and
tests/test_gpu_bn_bwd_edges.py (the kernels against the references) and tests/test_dense_bwd_cases.py (proof, on the CPU alone,
that every case is what it says).  Needs no GPU; deterministic.

All operand values are integers stored as float32, laid out so that every output is a sum of integers whose sum of |terms| stays
below 2^24: a correct float32 kernel must then return the int64 reference BIT FOR BIT in any order of summation, with or without
FMA contraction -- and every indexing mistake becomes a failing equality.  Layouts (``LAYOUTS``):
  small     G in [-7, 7] without 0, A in [-7, 7], dense: pins h h' (exact up to 2^18 rows: 49 * 262 145 < 2^24)
  mid       odd magnitudes in [257, 1023] with random sign, G on at most MID_ROWS active rows, A dense: bf16 round-to-nearest
            leaves a nonzero m and l = 0, so h h', h m', m h', m m' carry the value and the omitted products are 0
  low_g     G odd in [2^16, 2^20) on at most LOW_ROWS active rows, A in {+-1, +-2} dense (only h'): pins l h', m h', h h'
  low_a     low_g with the roles swapped (A nonzero on the active rows only): pins h l' and the mirrored terms
  low_g16 / low_a16   for the f16x2 form: odd in [2^11, 2^20) on one side, powers of two on the other: l h', h l', h h' (l l' = 0)
Active rows are placed on purpose: rows 0 and M - 1, both sides of the 16-row step edges inside the first and the last step, both
sides of a slab edge, the rest at random."""
import zlib
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

# ---- constants of csrc/wgrad.hip, csrc/backward.hip, csrc/norm.hip and rgnn.h, restated by hand (a change there must break a case)
TILE_N, TILE_K = 128, 256          # output tile of k_wgrad_x3
STEP = 16                          # rows of one step
LIVE = 32                          # columns of a live group (g_live / a_live)
WAVE_COLS = 64                     # a wave's column run of the virtual k axis: one descriptor per run
SLAB_MIN, SLAB_BUDGET, SLAB_ROWS = 8, 512, 256   # rgnn_wgrad_slabs: minimum and multiple of 8, 512 / tiles, about 256 rows per slab
WGN_BLOCKS, NARROW_ROWS = 256, 1024              # k_wgrad_narrow: blocks at most, rows per block below that
NARROW_THREADS = 256
NARROW_CLASSES = ((16, 9), (8, 17), (32, 6))     # wg_narrow_class: (n, kt) at most, first match wins
RED_GROUPS, RED_TRIP, RED_COLS = 16, 32, 64      # k_wg_reduce: slab groups, slabs per trip of a group (two of them), columns per block
PANEL, PANEL_GROUP = 128, 32       # k_bn_bwd_stats: rows per panel, rows per wave group inside it
STATS_COLS = 64                    # ... columns per block
COEF_GROUPS = (64, 256)            # panel groups of k_bn_bwd_coef / k_bn_bwd_coef4
COEF_CH = 16                       # k_bn_bwd_coef: channels per block
BOUND_SLOTS = 256
APPLY_MAX_BLOCKS = 256 * 16        # k_bn_bwd_apply: grid-stride beyond this
EXACT_LIMIT = 1 << 24

MID_ROWS, LOW_ROWS = 14, 8         # (14 * (1023 * 1.01)^2 < 2^24: the split pieces' |h| + |m| may exceed |x| by 2^-7)
LAYOUTS = ("small", "mid", "low_g", "low_a")
LAYOUTS_F16 = ("small", "low_g16", "low_a16")
FILL = 3.0                         # what rows and columns OUTSIDE the operands hold (finite: a stray read changes the result)


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ geometry, from the constants
def virtual_k(k1, k2, ones):
    o1, o2 = (1, 0) if (ones and k2 == 0) else (0, 1 if ones else 0)
    k1p = ceil_div(k1 + o1, WAVE_COLS) * WAVE_COLS
    return k1p, k1p + ceil_div(k2 + o2, WAVE_COLS) * WAVE_COLS


def tiles(n, k1, k2, ones):
    return ceil_div(n, TILE_N), ceil_div(virtual_k(k1, k2, ones)[1], TILE_K)


def narrow_class(n, k1, k2, ones):
    if k2 != 0 or n <= 0:
        return 0
    kt = k1 + (1 if ones else 0)
    for i, (nn, kk) in enumerate(NARROW_CLASSES):
        if n <= nn and kt <= kk:
            return i + 1
    return 0


def slabs(m, n, k1, k2, ones):
    if narrow_class(n, k1, k2, ones):
        return 512
    nt, kt = tiles(n, k1, k2, ones)
    if nt * kt == 0:
        return SLAB_MIN
    s = SLAB_BUDGET // (nt * kt) // 8 * 8
    s = min(s, ceil_div(ceil_div(m, SLAB_ROWS), 8) * 8)
    return max(s, SLAB_MIN)


def slab_steps(m_eff, n_slabs):
    """Steps of every slab, and which slabs START past the last step."""
    total = ceil_div(m_eff, STEP)
    per = ceil_div(total, n_slabs) if total else 0
    steps, past = [], []
    for s in range(n_slabs):
        beg = s * per
        end = min(beg + per, total)
        steps.append(max(end - beg, 0))
        past.append(beg >= total)
    return steps, past, per


def a_live(k1, k2, ones):
    """Per 32-column group of the virtual k axis (all k tiles): does the kernel multiply it?"""
    o1, o2 = (1, 0) if (ones and k2 == 0) else (0, 1 if ones else 0)
    k1p, kv = virtual_k(k1, k2, ones)
    width = ceil_div(kv, TILE_K) * TILE_K
    return [(c0 < k1 + o1) or (c0 >= k1p and c0 - k1p < k2 + o2) for c0 in range(0, width, LIVE)]


def virtual_columns(k1, k2, ones):
    """Virtual column of every column of dW."""
    k1p, _ = virtual_k(k1, k2, ones)
    o1 = 1 if (ones and k2 == 0) else 0
    return list(range(k1 + o1)) + [k1p + u for u in range(k2 + (1 if (ones and k2 > 0) else 0))]


def narrow_blocks(m):
    return max(1, min(WGN_BLOCKS, ceil_div(m, NARROW_ROWS)))


def narrow_trips(m):
    """Trips of the busiest thread through the grid-stride loop of k_wgrad_narrow."""
    return ceil_div(m, narrow_blocks(m) * NARROW_THREADS)


def reduce_paths(n_slabs):
    """(some group runs the paired loop, some group takes the `s < slabs` tail behind it, some group takes the tail alone)."""
    loop = tail_after = tail_alone = False
    for g in range(RED_GROUPS):
        s, looped = g, False
        while s + RED_GROUPS < n_slabs:
            s += RED_TRIP
            looped = True
        loop |= looped
        if s < n_slabs:
            tail_after |= looped
            tail_alone |= not looped
    return loop, tail_after, tail_alone


def vec_path(width, ld, offset_floats):
    """The 16-byte path of k_wgrad_narrow (gvec / avec) and of k_bn_bwd_apply<VEC>: width and stride multiples of 4 floats, base on
    the 16-byte grid (allocations are; a view is where its offset is a multiple of 4 floats)."""
    return width > 0 and width % 4 == 0 and ld % 4 == 0 and offset_floats % 4 == 0


def stat_panels(m):
    return ceil_div(m, PANEL)


# ------------------------------------------------------------------------------------------------ the split emulations
def bf16_round(x):
    """float32 -> nearest bf16 (ties to even), returned as float32; finite inputs."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u >> 16) & 1) + np.uint32(0x7fff)
    return ((u + r) & np.uint32(0xffff0000)).view(np.float32)


def split3(x):
    x = np.asarray(x, dtype=np.float32)
    h = bf16_round(x)
    r1 = (x - h).astype(np.float32)
    m = bf16_round(r1)
    r2 = (r1 - m).astype(np.float32)
    return {"h": h, "m": m, "l": bf16_round(r2)}


def split2(x):
    x = np.asarray(x, dtype=np.float32)
    h = x.astype(np.float16).astype(np.float32)
    return {"h": h, "l": (x - h).astype(np.float32).astype(np.float16).astype(np.float32)}


BF16X3_PRODUCTS = (("l", "h"), ("h", "l"), ("m", "m"), ("m", "h"), ("h", "m"), ("h", "h"))      # (piece of G, piece of A), kernel order
BF16X3_OMITTED = (("m", "l"), ("l", "m"), ("l", "l"))
F16X2_PRODUCTS = (("l", "h"), ("h", "l"), ("h", "h"))
F16X2_OMITTED = (("l", "l"),)


def _piece_sum(gp, ap, products):
    """(sum, sum of |terms|) in float64 of the products of split pieces: every piece and product is exact in float64 here."""
    tot = abs_tot = 0.0
    for pg, pa in products:
        tot = tot + gp[pg].astype(np.float64).T @ ap[pa].astype(np.float64)
        abs_tot = abs_tot + np.abs(gp[pg]).astype(np.float64).T @ np.abs(ap[pa]).astype(np.float64)
    return tot, abs_tot


def emulate_bf16x3(G, A, products=BF16X3_PRODUCTS):
    """G [m, n], A [m, K] (the column of ones included by the caller) -> what the bf16x3 kernel sums, in exact arithmetic."""
    return _piece_sum(split3(G), split3(A), products)


def scale_exp(bound):
    """wg_scale_exp: biased exponent se with bound * 2^(se - 127) in [2^14, 2^15)."""
    be = (int(np.float32(bound).view(np.uint32)) >> 23) & 255
    return min(268 - be, 253)


def emulate_f16x2(G, A, g_bound, a_bound, ones, products=F16X2_PRODUCTS):
    """The f16x2 form: both operands pre-scaled by the powers of two the kernel derives from the bounds, two f16 pieces each, the
    column of ones (``ones``: appended here) holding 2^14 after the pre-scale; the epilogue's powers of two undone in float64.
    -> (sum, sum of |terms| in units of the smallest product of pieces of each output)."""
    seg, sea = scale_exp(g_bound), scale_exp(a_bound)
    g_mul, a_mul = 2.0 ** (seg - 127), 2.0 ** (sea - 127)
    Gs = (np.asarray(G, dtype=np.float64) * g_mul).astype(np.float32)
    As = (np.asarray(A, dtype=np.float64) * a_mul).astype(np.float32)
    assert np.array_equal(Gs.astype(np.float64), np.asarray(G, dtype=np.float64) * g_mul)      # (the pre-scale is exact)
    assert np.array_equal(As.astype(np.float64), np.asarray(A, dtype=np.float64) * a_mul)
    out_mul = np.full(A.shape[1] + (1 if ones else 0), 2.0 ** (127 - seg) * 2.0 ** (127 - sea))
    if ones:
        As = np.concatenate([As, np.full((As.shape[0], 1), 2.0 ** 14, dtype=np.float32)], axis=1)
        out_mul[-1] = 2.0 ** (127 - seg) * 2.0 ** -14
    gp, ap = split2(Gs), split2(As)
    tot, abs_tot = _piece_sum(gp, ap, products)
    unit_g = _unit(np.concatenate([gp["h"], gp["l"]]))
    unit_a = _unit(np.concatenate([ap["h"], ap["l"]]))
    return tot * out_mul, abs_tot / (unit_g[:, None] * unit_a[None, :])


def _unit(x):
    """Per column: the largest power of two that divides every nonzero entry (1 for an all-zero column); entries are dyadic with
    their lowest bit at 2^-40 or above."""
    q = np.abs(np.asarray(x, dtype=np.float64)) * 2.0 ** 40
    i = q.astype(np.int64)
    assert np.array_equal(i.astype(np.float64), q)
    low = np.where(i > 0, i & -i, np.int64(1) << 62)
    low = low.min(axis=0)
    return np.where(low == (np.int64(1) << 62), 1.0, low.astype(np.float64) * 2.0 ** -40)


# ------------------------------------------------------------------------------------------------ weight-gradient cases
@dataclass
class Case:
    """One launch geometry.  ``m``: rows (of the row list, where there is one).  ``ones``: the bias column of the case as stated (the
    GPU tests run every case with and without).  ``row_list``: None or (kind, count) with kind in perm / reversed / repeat and
    count = None (no m_dev) or the device-side row count.  ``views``: operand -> (column offset, columns behind) inside a wider
    matrix.  ``expect``: the kernel the stated form takes."""
    name: str
    m: int
    n: int
    k1: int
    k2: int = 0
    ones: bool = True
    row_list: Optional[tuple] = None
    views: dict = field(default_factory=dict)
    aim: str = ""
    expect: str = "x3"
    layouts: tuple = LAYOUTS

    @property
    def m_eff(self):
        if self.row_list is None or self.row_list[1] is None:
            return self.m
        return self.row_list[1]

    def slabs(self, ones=None):
        return slabs(self.m, self.n, self.k1, self.k2, self.ones if ones is None else ones)

    def kernel(self, ones):
        """The kernel a launch of this case takes (a row list always takes the MFMA kernel)."""
        c = 0 if self.row_list is not None else narrow_class(self.n, self.k1, self.k2, ones)
        return "narrow%d" % c if c else "x3"


N_SWEEP = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 160)
K1_SWEEP = (1, 31, 32, 33, 63, 64, 65, 127, 128, 255, 256, 257)
K12_SWEEP = ((1, 1), (64, 63), (64, 64), (63, 1), (65, 64), (192, 64), (200, 1), (128, 129))
K2_ONLY = ((0, 5), (0, 64))
M_SWEEP = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 144, 256, 257, 384, 385)


def _geometry_cases():
    cs = []
    for n in N_SWEEP:
        cs.append(Case(f"n{n}", 70, n, 40, aim="g_live groups, wn halves" + (", nt = 2" if n > TILE_N else "")))
    for k1 in K1_SWEEP:
        cs.append(Case(f"k{k1}", 70, 40, k1, aim="k axis of one block: where the bias column lands"))
    for k1, k2 in K12_SWEEP:
        cs.append(Case(f"k{k1}+{k2}", 200, 40, k1, k2, aim="k axis of two blocks: descriptor per 64 columns"))
    for m in M_SWEEP:
        cs.append(Case(f"m{m}", m, 33, 20, aim="steps per slab on 8 slabs"))
    cs.append(Case("m2049_n129", 2049, 129, 20, aim="16 slabs x 2 tiles: XCD-to-slab mapping"))
    L = 300
    for nm, rl, m in (("short", ("perm", 211), L), ("count0", ("perm", 0), L), ("count1", ("perm", 1), L), ("count17", ("perm", 17), L),
                      ("full", ("perm", L), L), ("nocount", ("perm", None), L), ("reversed", ("reversed", None), L),
                      ("sparse", ("perm", 40), 4100)):
        cs.append(Case(f"rows_{nm}", m, 33, 20, 12, row_list=rl, aim="row list: " + nm))
    cs.append(Case("rows_repeat", L, 33, 20, 12, row_list=("repeat", 250), layouts=("small",), aim="repeated rows count twice"))
    cs.append(Case("view_a1", 130, 40, 37, 12, views={"a1": (1, 2)}, aim="A1 = columns [1 : 1 + k1] of a wider matrix"))
    cs.append(Case("view_g", 130, 40, 37, 12, views={"g": (2, 3)}, aim="G a column view"))
    cs.append(Case("view_a2", 130, 40, 37, 12, views={"a2": (0, 3)}, aim="A2 with a stride that is no multiple of 4"))
    return cs


def _narrow_cases():
    cs = []
    for n, kt, ex in ((16, 9, "narrow1"), (16, 10, "x3"), (17, 9, "x3"), (8, 17, "narrow2"), (8, 18, "x3"), (9, 17, "x3"),
                      (32, 6, "narrow3"), (32, 7, "x3"), (33, 6, "x3"), (17, 6, "narrow3"), (1, 1, "narrow1")):
        cs.append(Case(f"class_n{n}_kt{kt}", 300, n, kt, ones=False, expect=ex, aim="class boundary"))
    forms = (("aligned", {}), ("offgrid", {"g": (1, 3), "a1": (1, 3)}), ("oddstride", {"g": (0, 1), "a1": (0, 1)}))
    for n, k1 in ((4, 8), (8, 8), (12, 8), (16, 8), (8, 4), (8, 12), (8, 16)):
        for fn, vw in forms:
            cs.append(Case(f"vec_n{n}_k{k1}_{fn}", 300, n, k1, ones=False, views=dict(vw),
                           expect="narrow1" if k1 <= 9 else "narrow2", aim="16-byte path against the scalar path"))
    for m in (1, 255, 256, 257, 1024, 1025, 16385, 32769):
        cs.append(Case(f"narrow_m{m}", m, 16, 8, ones=False, expect="narrow1", aim="blocks of the narrow launch, tails of the reduce",
                       layouts=LAYOUTS if m <= 1025 else ("small", "mid")))
    cs.append(Case("narrow_m262145", 262145, 16, 9, ones=False, expect="narrow1", layouts=("small",), aim="second grid-stride trip"))
    for n, k1 in ((1, 1), (7, 9), (8, 8), (5, 13)):
        cs.append(Case(f"width{n * k1}", 300, n, k1, ones=False, expect="narrow%d" % narrow_class(n, k1, 0, 0),
                       aim="width edge of k_wg_reduce"))
    return cs


GEOMETRY_CASES = _geometry_cases()
NARROW_CASES = _narrow_cases()
K2_ONLY_CASES = [Case(f"k0+{k2}", 70, 40, 0, k2, aim="A1 null") for _, k2 in K2_ONLY]


def by_name(name):
    return next(c for c in GEOMETRY_CASES + NARROW_CASES + K2_ONLY_CASES if c.name == name)


def active_positions(m_eff, edge, cap, rng):
    """Positions (in the row sequence) of the active rows: the ends, both sides of the step edges inside the first and the last
    step, both sides of the slab (or block) edge at ``edge``, the rest at random."""
    if m_eff == 0:
        return np.zeros(0, dtype=np.int64)
    last0 = (ceil_div(m_eff, STEP) - 1) * STEP
    want = [0, m_eff - 1, STEP - 1, STEP, last0 - 1, last0, edge - 1, edge]
    pos = []
    for p in want:
        if 0 <= p < m_eff and p not in pos:
            pos.append(p)
    rest = [p for p in rng.permutation(m_eff)[:2 * cap + 8].tolist() if p not in pos]
    return np.array((pos + rest)[:cap], dtype=np.int64)


def _odd(rng, lo, hi, shape):
    mag = rng.integers(lo, hi, size=shape) | 1
    return mag * rng.choice([-1, 1], size=shape)


class Operands:
    """Operands of one (case, layout): matrices embedded in wider allocations, the row list, the int64 reference."""

    def __init__(self, case, layout, a1_scale=1):
        self.case, self.layout = case, layout
        rng = np.random.default_rng(zlib.crc32(f"{case.name}/{layout}".encode()))
        m, n, k1, k2 = case.m, case.n, case.k1, case.k2
        if case.row_list is None:
            self.row_index, self.count = None, None
            self.rows_alloc = ceil_div(m, STEP) * STEP if m else 0       # (the allocation holds the rows up to the next step edge)
            eff = np.arange(m)
        else:
            kind, count = case.row_list
            R = m + m // 2 + 5
            if kind == "repeat":
                lst = rng.integers(0, max(R // 4, 1), size=m)
            else:
                lst = rng.permutation(R)[:m]
                if kind == "reversed":
                    lst = np.sort(lst)[::-1]
            self.count = count
            cnt = m if count is None else count
            eff = lst[:cnt].copy()
            lst = lst.copy()
            lst[cnt:] = -7
            self.row_index = lst.astype(np.int32)
            self.rows_alloc = R
        self.eff = eff.astype(np.int64)
        R = self.rows_alloc
        edge = slab_steps(len(eff), case.slabs(True))[2] * STEP if case.kernel(True) == "x3" else NARROW_THREADS
        cap = {"small": 0, "mid": MID_ROWS}.get(layout, LOW_ROWS)
        pos = active_positions(len(eff), edge, cap, rng)
        self.active_pos = pos
        act = np.unique(eff[pos]) if len(pos) else np.zeros(0, dtype=np.int64)       # matrix rows that carry the capped operand
        K = k1 + k2

        def capped(width, lo, hi):
            x = np.zeros((R, width), dtype=np.int64)
            for i, r in enumerate(act):
                x[r] = _odd(rng, lo, hi if i % 2 == 0 else max(hi // 2, lo + 2), width)   # (every other row one bit lower: sum below 2^24)
            return x

        if layout == "small":
            G = rng.integers(1, 8, size=(R, n)) * rng.choice([-1, 1], size=(R, n))
            A = rng.integers(-7, 8, size=(R, K))
        elif layout == "mid":
            G = np.zeros((R, n), dtype=np.int64)
            G[act] = _odd(rng, 257, 1024, (len(act), n))
            A = _odd(rng, 257, 1024, (R, K))
        elif layout in ("low_g", "low_g16"):
            G = capped(n, 1 << (16 if layout == "low_g" else 11), 1 << 20)
            A = rng.choice([-2, -1, 1, 2], size=(R, K))
        elif layout in ("low_a", "low_a16"):
            G = rng.choice([-2, -1, 1, 2], size=(R, n))
            A = capped(K, 1 << (16 if layout == "low_a" else 11), 1 << 20)
        else:
            raise ValueError(layout)
        A = A.astype(np.int64)
        A[:, :k1] *= a1_scale
        self.G, self.A1, self.A2 = G.astype(np.int64), A[:, :k1], A[:, k1:]
        self.off = {k: case.views.get(k, (0, 0)) for k in ("g", "a1", "a2")}

    # ---- what the launch reads
    def wide(self, which, poison=False):
        """The wider float32 matrix that holds operand ``which``; everything outside the operand -- the columns around the view, the
        rows the launch does not select -- holds FILL, or NaN with ``poison``."""
        x = {"g": self.G, "a1": self.A1, "a2": self.A2}[which]
        off, extra = self.off[which]
        bad = np.float32(np.nan) if poison else np.float32(FILL)
        w = np.full((self.rows_alloc, off + x.shape[1] + extra), bad, dtype=np.float32)
        sel = np.zeros(self.rows_alloc, dtype=bool)
        sel[self.eff] = True
        w[sel, off:off + x.shape[1]] = x[sel].astype(np.float32)
        return w

    def row_index_for(self, poison=False):
        """The row list; with ``poison`` its unused tail names a row the launch does not select (NaN there) instead of -7."""
        if self.row_index is None:
            return None
        lst = self.row_index.copy()
        if poison:
            unsel = np.setdiff1d(np.arange(self.rows_alloc), self.eff)
            lst[lst < 0] = unsel[0]
        return lst

    def operand(self, ones):
        A = np.concatenate([self.A1[self.eff], self.A2[self.eff]], axis=1)
        if ones:
            A = np.concatenate([A, np.ones((len(self.eff), 1), dtype=np.int64)], axis=1)
        return self.G[self.eff], A

    def reference(self, ones):
        """(dW int64 [n, Kt], sum of |terms| of every output)."""
        G, A = self.operand(ones)
        return G.T @ A, np.abs(G).T @ np.abs(A)

    def bounds(self):
        """Exact maxima (float) of |G|, |A1|, |A2| over the rows of the launch."""
        mx = lambda x: float(np.abs(x[self.eff]).max()) if x[self.eff].size else 0.0
        return mx(self.G), mx(self.A1), mx(self.A2)


# ------------------------------------------------------------------------------------------------ BatchNorm / ReLU backward cases
BN_M = (1, 31, 32, 33, 96, 97, 127, 128, 129, 257)
BN_N = (1, 3, 4, 63, 64, 65, 128, 130)
BN_MASKS = ("none", "y", "table")
RELU_COUNTS = (1, 3, 4, 5, 1023, 1024, 1025, 1027)
DENORM_MIN = np.float32(1e-45)


def special_y(rng, shape):
    """y drawn from {positive, negative, +0, -0, NaN, the smallest positive denormal}; (y, the mask y > 0)."""
    vals = np.array([1.5, -2.0, 0.0, -0.0, np.nan, DENORM_MIN], dtype=np.float32)
    pick = rng.integers(0, len(vals), size=shape)
    flat = pick.reshape(-1)
    flat[:min(len(vals), flat.size)] = np.arange(len(vals))[:flat.size]          # (every kind occurs where there is room)
    y = vals[pick]
    return y, (pick == 0) | (pick == 5)


class BnCase:
    """dy in [-4, 4], h in [-8, 8], one of three masks; coefficients A, B, C in quarters (integers and powers of two)."""

    def __init__(self, m, n, mask):
        self.m, self.n, self.mask = m, n, mask
        rng = np.random.default_rng(zlib.crc32(f"bn/{m}/{n}/{mask}".encode()))
        self.dy = rng.integers(-4, 5, size=(m, n))
        self.h = rng.integers(-8, 9, size=(m, n))
        self.y = self.table = None
        keep = np.ones((m, n), dtype=bool)
        if mask == "y":
            self.y, keep = special_y(rng, (m, n))
        elif mask == "table":
            mu = rng.integers(-2, 3, size=n)
            g = rng.choice([-1, 0, 1, 2], size=n)
            if n > 1:
                g[0] = 1
            zr = np.argsort(self.h, axis=0, kind="stable")[m // 2]                  # the row whose y is exactly 0 in column c: a median
            t = -(self.h[zr, np.arange(n)] - mu) * g
            self.table = np.stack([mu, g, t]).astype(np.float32)
            self.y_table = (self.h - mu) * g + t                                    # int64: exact, and so is the kernel's fmaf
            keep = self.y_table > 0
        self.keep = keep
        self.g = np.where(keep, self.dy, 0)
        self.coef4 = np.stack([rng.choice([4, 8, -4, 2, 1], size=n), rng.integers(-8, 9, size=n), rng.integers(-16, 17, size=n)])

    @property
    def coef(self):
        return (self.coef4 / 4.0).astype(np.float32)

    def stats_reference(self):
        """int64 [panels, 2, n]: per 128-row panel the column sums of g and of g h."""
        P = max(stat_panels(self.m), 1)
        out = np.zeros((P, 2, self.n), dtype=np.int64)
        for p in range(P):
            sl = slice(p * PANEL, min((p + 1) * PANEL, self.m))
            out[p, 0] = self.g[sl].sum(0)
            out[p, 1] = (self.g[sl] * self.h[sl]).sum(0)
        return out

    def dx_reference(self):
        """float64, exact: (A4 g + B4 h + C4) / 4 in int64."""
        return (self.coef4[0] * self.g + self.coef4[1] * self.h + self.coef4[2]).astype(np.float64) / 4.0


# ------------------------------------------------------------------------------------------------ coefficient cases
COEF_N = (1, 3, 4, 15, 16, 17, 33, 64)
COEF_PANELS = (1, 63, 64, 65, 255, 256, 257)
COEF_EPS = 1e-5
COEF_PANEL_ROWS = 8


class CoefCase:
    """Synthetic inputs of rgnn_bn_bwd_coef: integer partial sums, forward statistics {count, pivot, sum (v - pivot), sum (v - pivot)^2}
    of integer data (8 rows per panel, 3 in the last; with three panels or more the second is EMPTY: count 0 behind garbage sums)."""

    def __init__(self, n, panels, with_gamma, train):
        self.n, self.panels, self.with_gamma, self.train = n, panels, with_gamma, train
        rng = np.random.default_rng(zlib.crc32(f"coef/{n}/{panels}".encode()))
        self.bwd_part = rng.integers(-50, 51, size=(panels, 2, n)).astype(np.float32)
        counts = np.full(panels, COEF_PANEL_ROWS)
        counts[-1] = 3
        if panels >= 3:
            counts[1] = 0
        self.m = int(counts.sum())
        self.v = rng.integers(-8, 9, size=(self.m, n)).astype(np.float64) + np.arange(n) % 5          # (column means differ)
        st = np.zeros((panels, 4, n))
        r = 0
        for p, c in enumerate(counts):
            if c == 0:
                st[p] = [[0.0] * n, [99.0] * n, [99.0] * n, [99.0] * n]
                continue
            blk = self.v[r:r + c]
            piv = blk[0]
            st[p] = [np.full(n, float(c)), piv, (blk - piv).sum(0), ((blk - piv) ** 2).sum(0)]
            r += c
        self.fwd_stats = st.astype(np.float32)
        assert np.array_equal(self.fwd_stats.astype(np.float64), st)
        self.gamma = rng.choice([0.5, 1.0, 2.0, -1.5, 3.0], size=n).astype(np.float32) if with_gamma else None
        self.running_mean = rng.integers(-3, 4, size=n).astype(np.float32)
        self.running_var = rng.choice([0.25, 1.0, 4.0, 9.0], size=n).astype(np.float32)

    def reference(self):
        """The header's formula in float64 -> dict name -> (value, sum of the absolute terms of its expression)."""
        b1 = self.bwd_part[:, 0].astype(np.float64).sum(0)
        b2 = self.bwd_part[:, 1].astype(np.float64).sum(0)
        if self.train:
            mean = self.v.mean(0)
            var = ((self.v - mean) ** 2).mean(0)
        else:
            mean, var = self.running_mean.astype(np.float64), self.running_var.astype(np.float64)
        rstd = 1.0 / np.sqrt(var + np.float64(np.float32(COEF_EPS)))
        gm = self.gamma.astype(np.float64) if self.gamma is not None else np.ones(self.n)
        m = float(self.m)
        sx = (b2 - mean * b1) * rstd
        sx_abs = (np.abs(b2) + np.abs(mean * b1)) * rstd
        A = gm * rstd
        z = np.zeros(self.n)
        if self.train:
            B = -gm * rstd * rstd * sx / m
            B_abs = np.abs(gm) * rstd * rstd * sx_abs / m
            C = -gm * rstd * b1 / m + gm * rstd * rstd * mean * sx / m
            C_abs = np.abs(gm * rstd * b1 / m) + np.abs(gm * rstd * rstd * mean) * sx_abs / m
        else:
            B = C = B_abs = C_abs = z
        return {"A": (A, np.abs(A)), "B": (B, B_abs), "C": (C, C_abs), "dgamma": (sx, sx_abs), "dbeta": (b1, np.abs(b1))}


def coef_bar(value, abs_terms):
    """One float32 ulp of the reference plus 2^-40 of the absolute terms of its expression."""
    ulp = np.spacing(np.abs(value).astype(np.float32)).astype(np.float64)
    return ulp + 2.0 ** -40 * abs_terms
