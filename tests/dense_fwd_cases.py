"""Hand-built operands that sit ON the edges of the forward dense layer rgnn_linear_fwd (csrc/linear.hip: k_linear_tiny, the fp32
MFMA kernel k_linear and the register-staged split product k_linear_x3; csrc/linear_dma.hip: the LDS-DMA kernel k_linear_dma in
its bf16x3 and f16x2 forms; csrc/linear_common.h: the epilogue they share), with their references in int64 / float64.  Shared by
tests/test_gpu_dense_fwd_edges.py (the kernels against the references) and tests/test_dense_fwd_cases.py (proof, on the CPU alone,
that every case is what it says and reaches the planned instance it claims).  Needs no GPU; deterministic.

All operand values are integers stored as float32 -- A1, A2, W, bias, residual; BatchNorm-apply tables hold integer mean_hi and t
and g in {0.5, 1, 2} with (x - mean_hi) even wherever g = 0.5 -- laid out so that every output is a sum of integers whose
sum |terms| + |bias| + |residual| stays below 2^24: a correct kernel returns the int64 reference BIT FOR BIT in any order of
summation, under any schedule, and every indexing mistake becomes a failing equality.  Layouts:
  small     a, w in +-[1, amp] (amp <= 7), dense; ``w_nnz`` keeps a column's weights on that many k (statistics cases: the panel
            sums must be exact about any pivot).  Pins h h'.
  mid       odd magnitudes in [257, 1023], A on at most MID_K reduction indices per row, W dense: bf16 rounding leaves a nonzero m
            and l = 0, so h h', h m', m h' and m m' carry the value and the omitted products are 0
  low_a     A odd in [2^16, 2^20) on at most LOW_K indices per row, W in {+-1, +-2} (only h'): pins l h', m h', h h'
  low_w     the roles swapped (W carries the wide values on LOW_K indices per column): pins h l', h m', h h'
  low_a16 / low_w16   for the f16x2 form: odd in [2^11, 2^20) against powers of two: l h' / h l' next to h h' (l l' = 0)
The active reduction indices are placed on purpose: 0 and K - 1, both sides of the first 16-k and 32-k step edge, both sides of the
A1 | A2 split, the last step's first index; the rest at random.

Poison: every operand is a view into a wider and longer allocation whose row padding (lda > k), rows no launch names and -- for
row lists -- the tail beyond the count hold NaN (-7 in a list); the output is pre-filled with SENTINEL and the reference says which
words may change."""
import zlib
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from dense_bwd_cases import BF16X3_PRODUCTS, EXACT_LIMIT, F16X2_PRODUCTS, _odd, ceil_div, scale_exp, split2, split3

# ---- constants of the kernels, restated by hand with the line they come from (a change there must break a case, not move it)
BM = 128                  # linear_common.h:31 (= RGNN_STAT_PANEL_ROWS, common.h:14): rows of an fp32 tile and of a statistics panel
BK = 32                   # linear_common.h:32: k per step of k_linear / k_linear_x3; planes are padded to it (rgnn_linear_planes_kp)
DMA_BK = 16               # linear_dma.hip:72
DMA_BM_MAX = 256          # linear_dma.hip:71: rows of an LDS-DMA tile (also of a k_linear_x3 tile: linear.hip:1133-1136)
DMA_SK_MAX_FILL = 88      # linear_dma.hip:79
LDS_BYTES = 160 * 1024    # linear_common.h:34
AFFINE_ROWS, STAT_ROWS, BOUND_SLOTS = 3, 4, 256           # rgnn.h:335, :331, :414
SPLITK_TIMEOUT_WORD = 1000                                # rgnn.h:58
SPLITK_FLAG_BYTES = 4096                                  # linear.hip:1075: the flag area behind the 256 x 256 KiB slots
ERR_UNSUPPORTED = -3                                      # rgnn.h:39
NONE, TINY, FP32, X3, DMA = range(5)                      # rgnn.h:427 RGNN_LINEAR_FAMILY_*
LIM = (1 << 31) - 64                                      # linear.hip:972
FP32_LADDER = ((64, 128), (32, 64), (0, 32))              # linear.hip:1045: n > 64 -> 128, n > 32 -> 64, else 32
X3_LADDER = FP32_LADDER                                   # linear.hip:1027 (+ the 256-wide tile, :1025-1026)
DMA_TOP = {"bf16x3": 7, "f16x2": 8}                       # linear_dma.hip:761
TINY_GRID_BLOCKS = 4096                                   # linear.hip:1102: k_linear_tiny walks its rows with a grid stride beyond this

SENTINEL = np.float32(-(2.0 ** 25))    # what `out` holds before the launch: no exact result reaches it
STAT_SENTINEL = np.float32(-77.0)
LIST_TAIL = -7
MID_K, LOW_K = 14, 8                   # (14 * (1023 * 1.01)^2 < 2^24; 4 * 2^20 * 2 + 4 * 2^19 * 2 < 2^24)
SWITCHES = ("RGNN_DMA_NO_SMALL_M", "RGNN_DMA_NOPSK", "RGNN_DMA_NOSK", "RGNN_X3_NODMA", "RGNN_LINEAR_FP32", "RGNN_LINEAR_NO_F16",
            "RGNN_LINEAR_NO_BUFL", "RGNN_LINEAR_NO_DIRECT", "RGNN_LINEAR_NO_TINY")


# ------------------------------------------------------------------------------------------------ the dispatch rules, restated
def ladder(n):
    return next(w for lo, w in FP32_LADDER if n > lo)


def fp32_tile(n, k, bufl, row_index):
    """linear.hip:1036-1045: the wide_tn instances (96 .. 224 columns) where they pad 5 % fewer columns than 128-wide tiles."""
    tn = 0
    if bufl and not row_index and 128 < n <= 512 and k >= 192:
        base = ceil_div(n, 128) * 128
        best = base
        for t in range(3, 8):
            padded = ceil_div(n, 32 * t) * 32 * t
            if padded < best or (padded == best and tn):
                best, tn = padded, t
        if best * 100 > base * 95:
            tn = 0
    return 32 * tn if tn else ladder(n)


def x3_tile(n):
    """linear.hip:1025-1027."""
    pad_w, pad_n = ceil_div(n, 256) * 256, ceil_div(n, 128) * 128
    return 256 if (n > 128 and pad_w * 100 <= pad_n * 107) else ladder(n)


def dma_pick_tn(n, m, form, no_small_m):
    """linear_dma.hip:760-784 (without RGNN_DMA_TN, which this suite never sets)."""
    top = DMA_TOP[form]
    best = 2
    if 64 < n <= 96:
        best = 3
    if n > 96:
        best, best_pad = top, ceil_div(n, 32 * top) * 32 * top
        for tn in range(top - 1, 2, -1):
            pad = ceil_div(n, 32 * tn) * 32 * tn
            if pad < best_pad:
                best_pad, best = pad, tn
    mt = ceil_div(m, DMA_BM_MAX)
    if mt * ceil_div(n, 32 * best) >= 192 or no_small_m:
        return best
    best_t, pick = 1e30, best
    for tn in range(2, top + 1):
        tiles = mt * ceil_div(n, 32 * tn)
        t = ceil_div(tiles, 256) * (0.35 + 0.2 * tn)
        if t < best_t - 1e-9:
            best_t, pick = t, tn
    return pick


def stat_lds_floats(waves, bn):
    return waves * bn * 3 + waves                          # stats.h:44-45


def dma_lds_bytes(tn, form):
    """linear_dma.hip:88-112 for eight waves: the LDS of an instance without the scale / shift tables."""
    bn, npl = 32 * tn, (2 if form == "f16x2" else 3)
    ks = 2 if npl == 2 else 1                              # double steps: the f16x2 form (dma_ks, tn <= 8)
    if ks == 2:
        a_ring, dw, w_stage = (3 if tn <= 5 else 2), 1, ks * npl * bn * 2 * 16
    else:
        a_ring, dw = 2 + 2, 2
        w_stage = ceil_div(npl * bn * 2, 512) * 512 * 16
    return a_ring * ks * (256 * DMA_BK * 4) + (dw + 1) * w_stage + stat_lds_floats(8, bn) * 4 + 256 * 4


def dma_schedule(m_count, n, k, tn, form, m_launch, ws, nopsk):
    """The three schedule conditions of k_linear_dma (linear_dma.hip:189-208) under the grid of launch_dma (:739-742), per XCD:
    -> set of (schedule, S) over the XCDs that have work; schedule in static / streamk / psk."""
    bn = 32 * tn
    nt = ceil_div(n, bn)
    ks = 2 if form == "f16x2" else 1
    nk = ceil_div(k, ks * DMA_BK)
    tiles = ceil_div(m_launch, DMA_BM_MAX) * nt
    grid = 256
    if grid > tiles and (tn > 4 or not ws or nopsk or 2 * tiles > grid):
        grid = tiles
    g8 = ceil_div(grid, 8)
    mt = ceil_div(m_count, DMA_BM_MAX)
    max_items = ceil_div(mt, 8) * nt
    out = set()
    for xcd in range(8):
        n_items = (ceil_div(mt - xcd, 8) if mt > xcd else 0) * nt
        if n_items == 0:
            continue
        rounds = ceil_div(n_items, g8)
        sk = (ws and nt == 1 and n_items >= g8 and nk >= 8 and n_items * 100 < rounds * g8 * DMA_SK_MAX_FILL
              and np.float32(n_items) / np.float32(g8) + np.float32(2.0) * bn / np.float32(k + bn) + np.float32(0.25) < np.float32(rounds))
        s = 1
        if tn <= 4 and not sk and ws and 2 * max_items <= g8 and nk >= 8 and not nopsk:
            s = min(g8 // max_items, 8, nk // 4)
        out.add(("streamk", 1) if sk else ("psk", s) if s > 1 else ("static", 1))
    return out


def aligned16(addr):
    return addr % 16 == 0


# ------------------------------------------------------------------------------------------------ cases
DEFAULT_VIEW = (4, 4)      # (floats in front of the operand inside its row, floats behind it): 16-byte aligned, poison on both sides


@dataclass
class Case:
    """One launch.  ``m``: rows of the matrices (rgnn_linear_args.m).  ``form``: the operands handed over -- fp32 (no planes), bf16x3
    (bf16 planes), f16x2 (both plane sets and the bounds).  ``rows``: None or (kind, count) -- kind in asc / perm / holes / tile-1 /
    long / nocount, count = *m_dev.  ``views``: operand (a1 a2 w out res b1 b2) -> (floats in front, floats behind) inside a wider
    row.  ``expect``: the row rgnn_linear_fwd_plan must answer.  ``schedule``: LDS-DMA cases, what dma_schedule must say."""
    name: str
    m: int
    n: int
    k1: int
    k2: int = 0
    form: str = "fp32"
    layout: str = "small"
    amp: tuple = (7, 7)
    w_nnz: Optional[int] = None
    env: tuple = ()
    relu: bool = True
    relu_from: int = 0
    bias: bool = True
    w_split: Optional[int] = None
    residual: Optional[str] = None        # "same" | "index" (residual_index with -1 entries)
    rows: Optional[tuple] = None
    accumulate: bool = False
    gather_only: bool = False
    stats: bool = False
    absmax: bool = False
    affine: Optional[str] = None          # "batch" | "segments" (per-segment tables: the list comes from ops.pad_list_by_segment)
    a1_relu: bool = True
    segments: tuple = ()                  # affine == "segments": row borders of the segments
    ws: bool = False
    views: dict = field(default_factory=dict)
    bound_mul: float = 1.0
    zero_a: bool = False
    expect: tuple = ()
    schedule: tuple = ()
    rc: int = 0
    vec: Optional[bool] = None            # claims checked against the restated rules (None: no claim)
    fast: Optional[bool] = None
    direct: Optional[bool] = None
    aim: str = ""

    @property
    def k(self):
        return self.k1 + self.k2

    @property
    def subset_count(self):
        """Rows of the row list the launch walks (M of the kernels), or m."""
        if self.rows is None or self.rows[1] is None:
            return self.m
        return self.rows[1]

    def view(self, which):
        return self.views.get(which, DEFAULT_VIEW)

    def ld(self, which):
        off, extra = self.view(which)
        width = {"a1": self.k1, "a2": self.k2, "w": self.k, "out": self.n, "res": self.n}[which]
        return off + width + extra

    def no_small_m(self):
        return "RGNN_DMA_NO_SMALL_M" in self.env

    def out_rows(self):
        return self.m + 3                                   # rows of the `out` allocation: three more than any launch may write


def fields(c, base, kp, ws_bytes):
    """The rgnn_linear_args fields of case ``c`` given the BASE ADDRESS of every allocation (``base``: name -> int; made-up ones
    on the CPU, data_ptr() on the device) -- one function, so that the plan the CPU test proves is the plan the GPU test runs."""
    at = lambda which: base[which] + 4 * c.view(which)[0]
    one_w = c.w_split is None
    f = dict(A1=at("a1") if c.k1 else None, lda1=c.ld("a1") if c.k1 else 0, k1=c.k1,
             A2=at("a2") if c.k2 else None, lda2=c.ld("a2") if c.k2 else 0, k2=c.k2,
             W1=at("w"), W2=None if one_w else at("w") + 4 * c.w_split * c.ld("w"), ldw=c.ld("w"), w_split=c.n if one_w else c.w_split,
             bias1=base["b1"] + 4 * c.view("b1")[0] if c.bias else None,
             bias2=base["b2"] + 4 * c.view("b2")[0] if (c.bias and not one_w) else None,
             residual=at("res") if c.residual else None, ldr=c.ld("res") if c.residual else 0,
             out=at("out"), ldo=c.ld("out"), m=c.m, n=c.n, relu_out=1 if c.relu else 0,
             col_stats=base["stats"] if c.stats else None,
             row_index=base["rows"] if c.rows else None,
             m_dev=base["mdev"] if (c.rows and (c.rows[1] is not None or c.affine == "segments")) else None,
             accumulate=1 if c.accumulate else 0, gather_only=1 if c.gather_only else 0,
             residual_index=base["resindex"] if c.residual == "index" else None,
             W_planes=base["planes"] if c.form != "fp32" else None, w_planes_kp=kp if c.form != "fp32" else 0,
             splitk_ws=base["ws"] if c.ws else None, splitk_ws_bytes=ws_bytes if c.ws else 0,
             a1_scale_shift=base["table"] if c.affine else None, a1_relu=1 if c.a1_relu else 0, relu_from_col=c.relu_from,
             W_planes_f16=base["planes16"] if c.form == "f16x2" else None, a1_bound=base["bound1"] if c.form == "f16x2" else None,
             a2_bound=base["bound2"] if (c.form == "f16x2" and c.k2) else None, out_absmax=base["absmax"] if c.absmax else None,
             a1_panel_segment=base["segs"] if c.affine == "segments" else None)
    return f


ALLOCATIONS = ("a1", "a2", "w", "out", "res", "b1", "b2", "stats", "rows", "mdev", "resindex", "planes", "planes16", "ws", "table",
               "bound1", "bound2", "absmax", "segs")
MADE_UP = {name: (i + 1) << 28 for i, name in enumerate(ALLOCATIONS)}      # 16-byte aligned, 256 MiB apart


def restated(c, f):
    """vec / bufl / fast_epilogue / direct_epilogue of plan_linear (linear.hip:962-980), from the fields."""
    one_w = f["w_split"] >= f["n"]
    k, m, n = f["k1"] + f["k2"], f["m"], f["n"]
    vec = (f["k1"] % 4 == 0 and f["k2"] % 4 == 0 and f["ldw"] % 4 == 0 and aligned16(f["W1"]) and (f["W2"] is None or aligned16(f["W2"]))
           and (f["k1"] == 0 or (f["lda1"] % 4 == 0 and aligned16(f["A1"]))) and (f["k2"] == 0 or (f["lda2"] % 4 == 0 and aligned16(f["A2"]))))
    e1 = ((m - 1) * f["lda1"] + f["k1"]) * 4 if f["k1"] else 0
    e2 = ((m - 1) * f["lda2"] + f["k2"]) * 4 if f["k2"] else 0
    ew = ((n - 1) * f["ldw"] + k) * 4
    eo = ((m - 1) * f["ldo"] + n) * 4
    bufl = (vec and f["k1"] > 0 and one_w and e1 < LIM and e2 < LIM and ew < LIM and (f["k2"] == 0 or f["k1"] % BK == 0)
            and "RGNN_LINEAR_NO_BUFL" not in c.env)
    fast = (n % 4 == 0 and f["ldo"] % 4 == 0 and aligned16(f["out"])
            and (f["residual"] is None or (f["ldr"] % 4 == 0 and aligned16(f["residual"])))
            and (f["bias1"] is None or aligned16(f["bias1"])) and (f["bias2"] is None or aligned16(f["bias2"]))
            and (one_w or f["w_split"] % 4 == 0))
    direct = f["row_index"] is None and f["residual"] is None and eo < LIM and "RGNN_LINEAR_NO_DIRECT" not in c.env
    return dict(vec=vec, bufl=bufl, fast=fast, direct=direct)


# ------------------------------------------------------------------------------------------------ operands
def active_k(k, k1, cap, rng):
    """Reduction indices that carry a capped operand: the ends, both sides of the 16 and 32 step edges, both sides of the A1 | A2
    split, the first index of the last 16-k step, the rest at random -- ``cap`` of them at most."""
    last0 = (ceil_div(k, DMA_BK) - 1) * DMA_BK
    want = [0, k - 1, DMA_BK - 1, DMA_BK, BK - 1, BK, k1 - 1, k1, last0]
    pos = []
    for p in want:
        if 0 <= p < k and p not in pos:
            pos.append(p)
    pos = pos[:cap]
    rest = [p for p in rng.permutation(k).tolist() if p not in pos]
    return np.array(sorted((pos + rest)[:cap]), dtype=np.int64)


def _signed(rng, amp, shape):
    return rng.integers(1, amp + 1, size=shape) * rng.choice([-1, 1], size=shape)


def _capped(rng, rows, k, k1, cap, lo, hi):
    """[rows, k] with odd magnitudes in [lo, hi) on ``cap`` reduction indices per row (every other one a bit lower: the sum stays
    below 2^24), zero elsewhere; half of a row's indices are the placed ones, the rest its own."""
    x = np.zeros((rows, k), dtype=np.int64)
    placed = active_k(k, k1, max(cap // 2, 1), rng)
    for r in range(rows):
        own = [p for p in rng.permutation(k).tolist() if p not in placed][:cap - len(placed)]
        idx = np.concatenate([placed, np.array(own, dtype=np.int64)])[:cap]
        for i, p in enumerate(idx):
            x[r, p] = _odd(rng, lo, hi if i % 2 == 0 else max(hi // 2, lo + 2), 1)[0]
    return x


def row_list(kind, m, count, rng):
    """-> the int32 list (tail beyond the count: LIST_TAIL).  Every matrix row is named once at most."""
    if kind == "nocount":
        return rng.permutation(m).astype(np.int32)
    tail = np.full(37, LIST_TAIL, dtype=np.int64)
    if kind == "asc":
        lst = np.sort(rng.permutation(m)[:count])
    elif kind == "perm":
        lst = rng.permutation(m)[:count]
    elif kind in ("holes", "tile-1"):
        holes = [0, 1, 2, 127, 128, 129, 253, 254, 255] if kind == "holes" else list(range(256, 512))
        lst = np.full(count, -1, dtype=np.int64)
        live = np.array([p for p in range(count) if p not in holes], dtype=np.int64)
        lst[live] = rng.permutation(m)[:len(live)]
    elif kind == "long":                                   # count > m: every row once, between runs of absent rows
        lst = np.full(count, -1, dtype=np.int64)
        pos = np.sort(np.concatenate([[0, count - 1], 1 + rng.permutation(count - 2)[:m - 2]]))
        lst[pos] = rng.permutation(m)
    else:
        raise ValueError(kind)
    assert (lst >= 0).sum() == len(np.unique(lst[lst >= 0]))
    return np.concatenate([lst, tail]).astype(np.int32)


def segment_base_list(c):
    """Per-segment cases: the ascending list handed to ops.pad_list_by_segment -- every row but each seventh."""
    return np.array([r for r in range(c.m) if r % 7 != 3], dtype=np.int32)


def pad_list_emulated(c):
    """What rgnn_pad_list_by_segment makes of segment_base_list (rgnn.h:500-503), for the CPU proofs only -- the GPU test takes
    the library's list: every segment's rows in 256-row tiles of their own, padded with -1.  -> (list, tile_segment)."""
    base, out, tiles = segment_base_list(c), [], []
    for s in range(len(c.segments) - 1):
        rows = base[(base >= c.segments[s]) & (base < c.segments[s + 1])]
        pad = ceil_div(len(rows), DMA_BM_MAX) * DMA_BM_MAX
        out.append(np.concatenate([rows, np.full(pad - len(rows), -1, dtype=np.int32)]))
        tiles += [s] * (pad // DMA_BM_MAX)
    return np.concatenate(out).astype(np.int32), np.array(tiles, dtype=np.int32)


class Operands:
    """Operands of one case: the matrices as int64, their wider float32 allocations, the row list, the references."""

    def __init__(self, c):
        self.c = c
        rng = np.random.default_rng(zlib.crc32(c.name.encode()))
        m, n, k1, k2, k = c.m, c.n, c.k1, c.k2, c.k
        aa, aw = c.amp
        if c.layout == "small":
            A, W = _signed(rng, aa, (m, k)), _signed(rng, aw, (n, k))
            if c.w_nnz is not None and c.w_nnz < k:
                keep = np.zeros((n, k), dtype=bool)
                for col in range(n):
                    keep[col, active_k(k, k1, min(4, c.w_nnz), rng)] = True
                    free = np.flatnonzero(~keep[col])
                    keep[col, rng.permutation(free)[:c.w_nnz - int(keep[col].sum())]] = True
                W = np.where(keep, W, 0)
        elif c.layout == "mid":
            A, W = _capped(rng, m, k, k1, min(MID_K, k), 257, 1024), _odd(rng, 257, 1024, (n, k))
        elif c.layout in ("low_a", "low_a16"):
            A = _capped(rng, m, k, k1, min(LOW_K, k), 1 << (16 if c.layout == "low_a" else 11), 1 << 20)
            W = rng.choice([-2, -1, 1, 2], size=(n, k))
        elif c.layout in ("low_w", "low_w16"):
            A = rng.choice([-2, -1, 1, 2], size=(m, k))
            W = _capped(rng, n, k, k1, min(LOW_K, k), 1 << (16 if c.layout == "low_w" else 11), 1 << 20)
        else:
            raise ValueError(c.layout)
        A, W = A.astype(np.int64), W.astype(np.int64)
        if c.zero_a:
            A[:] = 0
        self.A1, self.A2, self.W = A[:, :k1].copy(), A[:, k1:].copy(), W
        n1 = n if c.w_split is None else c.w_split
        self.bias1 = (np.arange(n1) * 5) % 23 - 11                       # neighbours differ; no period that divides a power of two
        self.bias2 = (np.arange(n - n1) * 7) % 29 - 14
        self.residual = rng.integers(-5, 6, size=(m, n)) if c.residual else None
        self.res_index = None
        if c.residual == "index":                                        # per OUTPUT row: a row of `residual`, or -1
            ri = rng.permutation(m).astype(np.int64)
            ri[rng.permutation(m)[:max(m // 3, 1)]] = -1
            ri[0] = -1
            if m > 1:
                ri[m - 1] = max(ri[m - 1], 0)
            self.res_index = ri.astype(np.int32)
        self.prev = rng.integers(-9, 10, size=(m, n)) if c.accumulate else None
        # ---- the BatchNorm-apply tables: A1 holds x with A1' = act((x - mean_hi) g + t) an integer
        self.table = None
        if c.affine:
            S = max(len(c.segments) - 1, 1)
            mean = rng.integers(-3, 4, size=(S, k1))
            g = rng.choice([0.5, 1.0, 2.0], size=(S, k1))
            t = rng.integers(-3, 4, size=(S, k1))
            self.table = np.stack([mean.astype(np.float64), g, t.astype(np.float64)], axis=1).astype(np.float32)   # [S, 3, k1]
            seg = self.segment_of_row()
            odd = (np.abs(self.A1 - mean[seg]) % 2 == 1) & (g[seg] == 0.5)
            self.A1 = self.A1 + odd                                       # (x - mean_hi) even where g = 0.5
        # ---- the row list
        self.list = None
        if c.rows is not None and c.affine != "segments":
            self.list = row_list(c.rows[0], m, c.rows[1], rng)

    # ---- geometry
    def segment_of_row(self):
        c = self.c
        if c.affine != "segments":
            return np.zeros(c.m, dtype=np.int64)
        return np.searchsorted(np.array(c.segments[1:]), np.arange(c.m), side="right")

    def named_rows(self, lst=None):
        """Matrix rows the launch reads."""
        c = self.c
        if c.rows is None:
            return np.arange(c.m)
        lst = self.list if lst is None else lst
        live = lst[:c.subset_count if c.affine != "segments" else len(lst)]
        return np.unique(live[live >= 0])

    def wide(self, which, lst=None):
        """float32 allocation of operand a1 / a2 / w / res: NaN around the view and on the rows the launch does not name."""
        c = self.c
        x = {"a1": self.A1, "a2": self.A2, "w": self.W, "res": self.residual}[which]
        off, extra = c.view(which)
        w = np.full((x.shape[0], off + x.shape[1] + extra), np.nan, dtype=np.float32)
        sel = np.ones(x.shape[0], dtype=bool)
        if which in ("a1", "a2") and c.rows is not None:
            sel[:] = False
            sel[self.named_rows(lst)] = True
        w[sel, off:off + x.shape[1]] = x[sel].astype(np.float32)
        return w

    def bias_alloc(self, which):
        b = self.bias1 if which == "b1" else self.bias2
        off = self.c.view(which)[0]
        w = np.full(off + len(b) + 4, np.nan, dtype=np.float32)
        w[off:off + len(b)] = b
        return w

    def out_alloc(self):
        """`out` before the launch: SENTINEL, or -- accumulate -- the previous integers on the rows of the matrix."""
        c = self.c
        off, _ = c.view("out")
        w = np.full((c.out_rows(), c.ld("out")), SENTINEL, dtype=np.float32)
        if c.accumulate:
            w[:c.m, off:off + c.n] = self.prev.astype(np.float32)
        return w

    def a1_eff(self, rows):
        """A1' of the given matrix rows: the table applied (float64, exact)."""
        x = self.A1[rows].astype(np.float64)
        if self.table is None:
            return x
        tb = self.table.astype(np.float64)[self.segment_of_row()[rows]]
        y = (x - tb[:, 0]) * tb[:, 1] + tb[:, 2]
        return np.maximum(y, 0.0) if self.c.a1_relu else y

    def bounds(self, lst=None):
        """Exact max |A1'| and max |A2| over the rows the launch reads (times bound_mul: a looser bound is still a bound)."""
        rows = self.named_rows(lst)
        b1 = float(np.abs(self.a1_eff(rows)).max()) if (rows.size and self.c.k1) else 0.0
        b2 = float(np.abs(self.A2[rows]).max()) if (rows.size and self.c.k2) else 0.0
        return b1 * self.c.bound_mul, b2 * self.c.bound_mul

    # ---- references
    def product(self, rows):
        """(sum, sum of |terms|) float64 [len(rows), n] of [A1' | A2] W^T: every product and sum is exact in float64 here."""
        A = np.concatenate([self.a1_eff(rows), self.A2[rows].astype(np.float64)], axis=1)
        W = self.W.astype(np.float64)
        return A @ W.T, np.abs(A) @ np.abs(W).T

    def reference(self, lst=None, count=None):
        """-> dict: out (the whole allocation after the launch, float64), touched (bool, same shape: words the launch stores),
        budget (max over the outputs of sum |terms| + |bias| + |residual| (+ |previous|)), stats [panels, 3, n] float64
        {count, sum, sum of squares} of the stored values per 128-row panel of the launch's rows, panels_written, absmax,
        phantom (max |value| an ABSENT row's lanes compute: the statistics' pivot may be one of them)."""
        c = self.c
        n = c.n
        off, _ = c.view("out")
        bias = np.concatenate([self.bias1, self.bias2]).astype(np.float64) if c.bias else np.zeros(n)
        if c.rows is None:
            pos_rows = np.arange(c.m)
            M = c.m
        else:
            lst = self.list if lst is None else lst
            M = (c.subset_count if count is None else count)
            pos_rows = lst[:M].astype(np.int64)
        live = pos_rows >= 0
        rows = pos_rows[live]
        acc, abs_terms = self.product(rows)
        v = acc + bias
        if c.relu:
            v[:, c.relu_from:] = np.maximum(v[:, c.relu_from:], 0.0)
        dest = np.flatnonzero(live) if c.gather_only else rows
        budget = abs_terms + np.abs(bias)
        if c.residual:
            rrow = self.res_index[dest].astype(np.int64) if c.residual == "index" else dest
            add = np.where((rrow >= 0)[:, None], self.residual[np.maximum(rrow, 0)], 0).astype(np.float64)
            v = v + add
            budget = budget + np.abs(add)
        if c.accumulate:
            v = v + self.prev[dest]
            budget = budget + np.abs(self.prev[dest])
        out = self.out_alloc().astype(np.float64)
        touched = np.zeros(out.shape, dtype=bool)
        out[dest, off:off + n] = v
        touched[dest, off:off + n] = True
        panels = ceil_div(M, BM)
        stats = np.zeros((panels, 3, n))
        panel_of = np.flatnonzero(live) // BM
        for p in range(panels):
            blk = v[panel_of == p]
            stats[p] = [np.full(n, float(len(blk))), blk.sum(0), (blk * blk).sum(0)]
        # an absent row (beyond the count, or a -1 entry) reads zeros: its lanes compute act(t - mean_hi g) W + bias and drop it
        a0 = np.zeros((1, c.k1))
        if self.table is not None:
            tb = self.table.astype(np.float64)
            a0 = tb[:, 2] - tb[:, 0] * tb[:, 1]
            a0 = np.maximum(a0, 0.0) if c.a1_relu else a0
        phantom = float(np.abs(a0 @ self.W[:, :c.k1].astype(np.float64).T + bias).max())
        return dict(out=out, touched=touched, budget=float(budget.max()) if budget.size else 0.0, stats=stats, panels_written=panels,
                    absmax=float(np.abs(v).max()) if v.size else 0.0, phantom=phantom, M=M)

    # ---- the split forms, in exact arithmetic (proof that the integer reference is what the kernel's products sum to)
    def emulate(self, products=None, rows=None):
        """(sum, sum of |terms|) of the products of split pieces the form's kernel adds up: bf16x3 six, f16x2 three (after the
        power-of-two pre-scales, undone here), for the given matrix rows."""
        c = self.c
        rows = np.arange(c.m) if rows is None else rows
        A = np.concatenate([self.a1_eff(rows), self.A2[rows].astype(np.float64)], axis=1)
        W = self.W.astype(np.float64)
        if c.form == "f16x2":
            b1, b2 = self.bounds()
            sa = 2.0 ** (scale_exp(max(b1, b2)) - 127)
            sw = 2.0 ** (scale_exp(float(np.abs(W).max())) - 127)
            A32, W32 = (A * sa).astype(np.float32), (W * sw).astype(np.float32)
            assert np.array_equal(A32.astype(np.float64), A * sa) and np.array_equal(W32.astype(np.float64), W * sw)
            ap, wp, undo = split2(A32), split2(W32), 1.0 / (sa * sw)
            products = F16X2_PRODUCTS if products is None else products
        else:
            ap, wp, undo = split3(A.astype(np.float32)), split3(W.astype(np.float32)), 1.0
            products = BF16X3_PRODUCTS if products is None else products
        tot = abs_tot = 0.0
        for pa, pw in products:                       # (piece of A, piece of W), kernel order
            tot = tot + ap[pa].astype(np.float64) @ wp[pw].astype(np.float64).T
            abs_tot = abs_tot + np.abs(ap[pa]).astype(np.float64) @ np.abs(wp[pw]).astype(np.float64).T
        return tot * undo, abs_tot * undo


# ------------------------------------------------------------------------------------------------ the case lists
def _row(family, form=0, tile=0, nt=0, subset=0, bufl=0, affine=0, split_k=0):
    return (family, form, tile, nt, subset, bufl, affine, split_k)


def _tiny_cases():
    cs = []
    for n in (1, 3, 4, 5, 64):
        for ldo_extra, out_off in ((0, 0), (1, 0), (3, 1)):
            k1 = 8 if n in (4, 64) else 1 if n == 1 else 5
            v4 = n % 4 == 0 and ldo_extra == 0 and out_off == 0
            cs.append(Case(f"tiny_n{n}_ldo+{ldo_extra}_off{out_off}", 4096, n, k1, relu=(n + ldo_extra + out_off) % 2 == 0,
                           views={"out": (out_off, ldo_extra), "a1": (1, 2)}, expect=_row(TINY), fast=v4,
                           aim="k_linear_tiny<%s>" % ("true" if v4 else "false")))
    cs.append(Case("tiny_k1", 4096, 8, 1, views={"out": (0, 0)}, expect=_row(TINY), aim="k = 1"))
    cs.append(Case("tiny_m4095", 4095, 8, 8, views={"out": (0, 0)}, expect=_row(FP32, tile=32, nt=1, bufl=1, affine=1), direct=True,
                   aim="one row short of the tiny kernel: the fp32 kernel"))
    rows = 70000
    assert rows * ceil_div(64, 4) > TINY_GRID_BLOCKS * 256
    cs.append(Case("tiny_gridstride", rows, 64, 8, views={"out": (0, 0)}, expect=_row(TINY, bufl=1), aim="second trip of the grid stride"))
    cs.append(Case("tiny_gridstride_odd", rows, 63, 5, relu=False, views={"out": (0, 1)}, expect=_row(TINY), aim="second trip, scalar stores"))
    return cs


def _fp32_cases():
    cs = []
    F = lambda tile, nt, bufl=1, affine=None: _row(FP32, tile=tile, nt=nt, bufl=bufl, affine=bufl if affine is None else affine)
    # ---- tile ladder: n on both sides of every edge, one short of and one past a tile multiple
    for n in (31, 32, 33, 63, 64, 65, 127, 128, 129, 257):
        t = ladder(n)
        cs.append(Case(f"fp32_n{n}", 129, n, 36, expect=F(t, ceil_div(n, t)), direct=True, aim=f"tile {t}, direct epilogue"))
    for n in (32, 33, 64, 65, 128, 132):
        t = ladder(n)
        cs.append(Case(f"fp32_n{n}_staged", 130, n, 32, residual="same", expect=F(t, ceil_div(n, t)), direct=False,
                       fast=n % 4 == 0, aim=f"tile {t}, staged epilogue"))
    # ---- the wide_tn instances (k >= 192, 128 < n <= 512, buffer descriptors, no row list)
    for n, t in ((260, 96), (140, 160), (180, 192), (200, 224), (440, 224)):
        assert fp32_tile(n, 192, True, False) == t
        cs.append(Case(f"fp32_wide{t}_n{n}", 129, n, 192, amp=(5, 5), expect=F(t, ceil_div(n, t)), direct=True, aim=f"wide_tn {t // 32}"))
    cs.append(Case("fp32_wide160_stats", 257, 140, 192, amp=(2, 2), w_nnz=36, stats=True, expect=F(160, 1), direct=True,
                   aim="the 32 x 160 wave tile keeps the staged epilogue (n % 4 == 0: fast)"))
    cs.append(Case("fp32_wide160_slow", 130, 139, 192, amp=(5, 5), expect=F(160, 1), direct=True, fast=False,
                   aim="... and the per-element one at n % 4 != 0"))
    cs.append(Case("fp32_k188_not_wide", 129, 200, 188, amp=(5, 5), expect=F(128, 2), direct=True, aim="k < 192: the 128 ladder"))
    # ---- m and k edges
    for m in (1, 127, 128, 129):
        cs.append(Case(f"fp32_m{m}", m, 40, 36, expect=F(64, 1), direct=True, aim="row panel edge"))
        cs.append(Case(f"fp32_m{m}_stats", m, 36, 32, amp=(2, 2), stats=True, residual="same", expect=F(64, 1), aim="partial last panel, staged"))
    cs.append(Case("fp32_m300_stats_direct", 300, 40, 32, amp=(2, 2), stats=True, expect=F(64, 1), direct=True, aim="three panels, the last partial"))
    for k in (32, 33, 36, 63, 64, 68):                      # k % 32 in {0, 1, 4, 31}
        cs.append(Case(f"fp32_k{k}", 70, 40, k, expect=F(64, 1, bufl=int(k % 4 == 0)), vec=k % 4 == 0, direct=True, aim=f"k % 32 = {k % 32}"))
    cs.append(Case("fp32_n31_scalar", 70, 31, 33, expect=F(32, 1, bufl=0), vec=False, direct=True, aim="tile 32 on scalar loads"))
    cs.append(Case("fp32_k1", 70, 33, 1, expect=F(64, 1, bufl=0), vec=False, aim="k = 1"))
    for k1, k2 in ((32, 4), (64, 36), (16, 16), (36, 32), (5, 3), (0, 36)):
        bufl = int(k1 % 32 == 0 and k1 > 0 and k2 % 4 == 0)
        cs.append(Case(f"fp32_k{k1}+{k2}", 131, 40, k1, k2, expect=F(64, 1, bufl=bufl), vec=(k1 % 4 == 0 and k2 % 4 == 0),
                       aim="two blocks" + ("" if bufl else ": no descriptors")))
    # ---- the loaders: vec off by an odd stride and by a pointer offset of one float, each operand in turn
    for which in ("a1", "a2", "w"):
        cs.append(Case(f"fp32_oddld_{which}", 131, 40, 32, 36, views={which: (4, 5)}, expect=F(64, 1, bufl=0), vec=False, aim="scalar loads"))
        cs.append(Case(f"fp32_offptr_{which}", 131, 40, 32, 36, views={which: (1, 3)}, expect=F(64, 1, bufl=0), vec=False, aim="scalar loads"))
    cs.append(Case("fp32_nobufl", 131, 40, 32, 36, env=("RGNN_LINEAR_NO_BUFL",), expect=F(64, 1, bufl=0), vec=True, aim="16-byte pointer loads"))
    cs.append(Case("fp32_nobufl_k36", 131, 72, 36, env=("RGNN_LINEAR_NO_BUFL",), expect=F(128, 1, bufl=0), vec=True, aim="... with a partial k-step"))
    cs.append(Case("fp32_nodirect", 131, 40, 36, env=("RGNN_LINEAR_NO_DIRECT",), expect=F(64, 1), direct=False, fast=True, aim="staged epilogue without residual"))
    # ---- fast_epilogue off by each of its conditions in turn (residual given: the staged epilogues)
    base = dict(m=131, n=40, k1=36, residual="same", bias=True)
    cs.append(Case("fp32_fast_on", **base, expect=F(64, 1), fast=True, direct=False, aim="all conditions met"))
    for nm, kw in (("n", dict(n=41)), ("ldo", dict(views={"out": (4, 5)})), ("outptr", dict(views={"out": (1, 3)})),
                   ("ldr", dict(views={"res": (4, 5)})), ("resptr", dict(views={"res": (1, 3)})), ("bias1ptr", dict(views={"b1": (1, 0)})),
                   ("bias2ptr", dict(w_split=20, views={"b2": (1, 0)})), ("wsplit", dict(w_split=22))):
        kw = {**base, **kw}
        one_w = kw.get("w_split") is None
        cs.append(Case(f"fp32_fast_off_{nm}", **kw, expect=F(64, 1, bufl=int(one_w)), fast=False, direct=False, aim="per-element epilogue"))
    cs.append(Case("fp32_ldr_wide", 131, 40, 36, residual="same", views={"res": (8, 24)}, expect=F(64, 1), fast=True, aim="ldr != n"))
    # ---- residual_index with -1, with and without a row list
    cs.append(Case("fp32_resindex", 131, 40, 36, residual="index", expect=F(64, 1), fast=True, aim="residual rows by index, -1 = none"))
    cs.append(Case("fp32_resindex_slow", 131, 41, 36, residual="index", expect=F(64, 1), fast=False, aim="... per-element epilogue"))
    cs.append(Case("fp32_resindex_rows", 200, 40, 36, residual="index", rows=("perm", 131), expect=F(64, 1), fast=True, aim="... behind a row list"))
    cs.append(Case("fp32_resindex_rows_slow", 200, 42, 36, residual="index", rows=("perm", 131), expect=F(64, 1), fast=False, aim="... per-element"))
    cs.append(Case("fp32_resindex_gather", 200, 40, 36, residual="index", rows=("perm", 131), gather_only=True, expect=F(64, 1), fast=True,
                   aim="gather_only: the index is per compact output row"))
    # ---- row lists on the fp32 kernel
    for nm, kw in (("asc", dict(rows=("asc", 131))), ("perm", dict(rows=("perm", 129))), ("nocount", dict(rows=("nocount", None))),
                   ("count0", dict(rows=("perm", 0), stats=True, amp=(2, 2))), ("stats", dict(rows=("perm", 150), stats=True, amp=(2, 2))),
                   ("nobufl", dict(rows=("perm", 131), env=("RGNN_LINEAR_NO_BUFL",))), ("scalar", dict(rows=("perm", 131), views={"a1": (1, 2)}))):
        bufl = int(nm not in ("nobufl", "scalar"))
        cs.append(Case(f"fp32_rows_{nm}", 200, 40, 32, **kw, expect=F(64, 1, bufl=bufl), aim="row list: " + nm))
    cs.append(Case("fp32_accumulate", 200, 40, 36, rows=("perm", 131), accumulate=True, expect=F(64, 1), fast=True, aim="out += result"))
    cs.append(Case("fp32_accumulate_slow", 200, 37, 36, rows=("perm", 131), accumulate=True, expect=F(64, 1), fast=False, aim="... per element"))
    cs.append(Case("fp32_gather_only", 200, 40, 36, rows=("perm", 131), gather_only=True, expect=F(64, 1), fast=True, aim="compact result"))
    cs.append(Case("fp32_gather_only_slow", 200, 39, 36, rows=("perm", 131), gather_only=True, stats=True, amp=(2, 2), expect=F(64, 1),
                   fast=False, aim="... per element, with statistics"))
    # ---- relu_from_col and w_split at tile edges
    for rf in (0, 40, 64, 99):
        cs.append(Case(f"fp32_relufrom{rf}", 70, 100, 36, relu_from=rf, expect=F(128, 1), direct=True, aim="relu_from_col, direct"))
        cs.append(Case(f"fp32_relufrom{rf}_staged", 70, 100, 36, relu_from=rf, residual="same", expect=F(128, 1), fast=True, aim="... fast"))
    cs.append(Case("fp32_relufrom33_slow", 70, 99, 36, relu_from=33, residual="same", expect=F(128, 1), fast=False, aim="... per element"))
    cs.append(Case("fp32_relufrom128_tiles", 70, 200, 36, relu_from=128, expect=F(128, 2), direct=True, aim="on the edge between two tiles"))
    for ws_ in (128, 100, 33):
        cs.append(Case(f"fp32_wsplit{ws_}", 70, 200, 36, w_split=ws_, expect=F(128, 2, bufl=0), direct=True, vec=True,
                       aim="two weight blocks, two biases: " + ("tile edge" if ws_ == 128 else "inside a tile")))
    cs.append(Case("fp32_wsplit100_staged", 70, 200, 36, w_split=100, residual="same", expect=F(128, 2, bufl=0), fast=True, aim="... fast"))
    cs.append(Case("fp32_wsplit33_staged", 70, 200, 36, w_split=33, residual="same", expect=F(128, 2, bufl=0), fast=False, aim="... per element"))
    # ---- a1_scale_shift on the descriptor path
    for relu_ in (True, False):
        cs.append(Case(f"fp32_affine_relu{int(relu_)}", 131, 40, 36, affine="batch", a1_relu=relu_, expect=F(64, 1), aim="table on A1"))
        cs.append(Case(f"fp32_affine_k2_relu{int(relu_)}", 131, 40, 32, 36, affine="batch", a1_relu=relu_, expect=F(64, 1), aim="... A2 untouched"))
    cs.append(Case("fp32_affine_refused", 131, 40, 36, affine="batch", views={"a1": (1, 2)}, expect=F(64, 1, bufl=0), rc=ERR_UNSUPPORTED,
                   aim="no descriptors, no table: refused, not ignored"))
    # ---- planes given, fp32 forced
    cs.append(Case("fp32_forced", 300, 96, 64, form="bf16x3", env=("RGNN_LINEAR_FP32",), expect=F(128, 1, affine=0), aim="RGNN_LINEAR_FP32"))
    return cs


def _x3_cases():
    cs = []
    X = lambda tile, nt, subset=0: _row(X3, form=1, tile=tile, nt=nt, subset=subset, bufl=1)
    # tiles 32 / 64 / 128 / 256, direct and subset; k = 20 or 36: planes padded to kp = 32 / 64 against NaN behind the k columns
    for n, k in ((32, 20), (28, 64), (64, 36), (36, 20), (128, 36), (100, 20), (256, 36), (132, 20), (260, 36)):
        t = x3_tile(n)
        for subset in (0, 1):
            kw = dict(rows=("perm", 257), m=300) if subset else dict(m=257)
            cs.append(Case(f"x3_n{n}_k{k}" + ("_rows" if subset else ""), n=n, k1=k, form="bf16x3", **kw, expect=X(t, ceil_div(n, t), subset),
                           aim=f"k_linear_x3 tile {t}, kp > k"))
    for m in (128, 255, 256, 257):
        cs.append(Case(f"x3_m{m}", m, 72, 36, form="bf16x3", stats=True, amp=(2, 2), expect=X(128, 1), aim="256-row tile edge, two panels"))
        cs.append(Case(f"x3_m{m}_rows", 300, 72, 36, form="bf16x3", rows=("asc", m), stats=True, amp=(2, 2), expect=X(128, 1, 1), aim="... subset"))
    cs.append(Case("x3_nodma", 257, 96, 64, form="bf16x3", env=("RGNN_X3_NODMA",), expect=X(128, 1), aim="RGNN_X3_NODMA at a DMA shape"))
    cs.append(Case("x3_nodma_k2", 257, 160, 32, 48, form="bf16x3", env=("RGNN_X3_NODMA",), expect=X(256, 1), aim="two blocks, 256-wide tile (k-step 16)"))
    cs.append(Case("x3_k2", 257, 40, 32, 20, form="bf16x3", expect=X(64, 1), aim="A2 with a partial step"))
    cs.append(Case("x3_rows_count0", 300, 72, 36, form="bf16x3", rows=("perm", 0), stats=True, amp=(2, 2), expect=X(128, 1, 1), aim="count 0"))
    for lay in ("mid", "low_a", "low_w"):
        cs.append(Case(f"x3_{lay}", 257, 72, 36, form="bf16x3", layout=lay, expect=X(128, 1), aim="split terms"))
        cs.append(Case(f"x3_{lay}_256", 130, 132, 20, form="bf16x3", layout=lay, expect=X(256, 1), aim="split terms, k-step 16"))
    return cs


def _dma_cases():
    cs = []
    NSM = ("RGNN_DMA_NO_SMALL_M",)
    fid = {"bf16x3": 1, "f16x2": 2}

    def D(form, tn, n, subset=0, affine=0, split_k=0):
        return _row(DMA, form=fid[form], tile=32 * tn, nt=ceil_div(n, 32 * tn), subset=subset, bufl=1, affine=affine, split_k=split_k)

    def add(name, m, n, k1, k2=0, form="bf16x3", tn=None, env=NSM, affine_row=1, plan_form=None, **kw):
        plan_form = plan_form or form
        tn_ = dma_pick_tn(n, m, plan_form, "RGNN_DMA_NO_SMALL_M" in env)
        assert tn is None or tn == tn_, (name, tn, tn_)
        subset = int(kw.get("rows") is not None or kw.get("affine") == "segments")
        kw.setdefault("absmax", True)
        kw.setdefault("schedule", (("static", 1),))
        cs.append(Case(name, m, n, k1, k2, form=form, env=env, expect=D(plan_form, tn_, n, subset, affine_row, int(kw.get("ws", False) and "RGNN_DMA_NOSK" not in env)), **kw))

    # ---- every TN, both forms, direct and subset; n ragged against 32 TN where the ladder allows (96 TN' < n <= 32 TN picks TN)
    widths = {2: (33, 64), 3: (65, 96), 4: (97, 128), 5: (129, 160), 6: (161, 192), 7: (193, 224), 8: (225, 256)}
    for form in ("bf16x3", "f16x2"):
        for tn, ns in widths.items():
            if tn > DMA_TOP[form]:
                continue
            for n in ns:
                assert dma_pick_tn(n, 257, form, True) == tn, (form, tn, n)
                add(f"dma_{form}_tn{tn}_n{n}", 257, n, 48, form=form, tn=tn, aim=f"TN {tn}, two row tiles, K = 48")
                add(f"dma_{form}_tn{tn}_n{n}_rows", 300, n, 32, 16, form=form, tn=tn, rows=("holes", 257), stats=(n % 32 != 0),
                    amp=(2, 2), w_nnz=40, aim=f"TN {tn} on a row list with absent rows")
    add("dma_bf16x3_n225_two_tiles", 257, 225, 32, tn=4, aim="bf16x3 stops at 224 columns: 2 x 128, ragged")
    add("dma_bf16x3_n257", 130, 257, 32, tn=3, aim="three tiles of 96")
    add("dma_f16x2_n257", 130, 257, 32, form="f16x2", tn=3, aim="three tiles of 96")
    add("dma_natural_n65", 300, 65, 32, env=(), tn=2, stats=True, amp=(2, 2), aim="few rows: the narrow tile, ONE column in the last tile")
    add("dma_natural_few_rows", 300, 224, 32, env=(), tn=2, aim="few rows: the narrow tile, 4 column tiles x 2 row tiles")
    add("dma_natural_few_rows_f16", 300, 100, 32, form="f16x2", env=(), tn=2, aim="few rows: the narrow tile")
    # ---- m and K edges
    for m in (1, 255, 256, 513):
        for form in ("bf16x3", "f16x2"):
            add(f"dma_{form}_m{m}", m, 72, 32, form=form, tn=3, stats=True, amp=(2, 2), aim="row tile edge, statistics panels")
    for k in (16, 32, 48):
        for form in ("bf16x3", "f16x2"):
            add(f"dma_{form}_k{k}", 257, 40, k, form=form, tn=2, aim="K = %d" % k + (": empty second half of a double step" if k == 48 else ""))
    # (two blocks keep the buffer descriptors only with k1 % 32 == 0: linear.hip:973 -- the split is on a 16 edge that is a 32 edge)
    for k1, k2 in ((32, 16), (32, 32), (64, 16), (32, 48)):
        for form in ("bf16x3", "f16x2"):
            add(f"dma_{form}_k{k1}+{k2}", 257, 72, k1, k2, form=form, tn=3, aim="A1 | A2 split on a 16 edge")
    # ---- split terms
    for lay in ("mid", "low_a", "low_w"):
        add(f"dma_{lay}", 257, 72, 48, layout=lay, tn=3, aim="split terms of the bf16x3 form")
        add(f"dma_{lay}_rows", 300, 100, 32, 16, layout=lay, tn=4, rows=("perm", 257), aim="... subset instance")
    for lay in ("low_a16", "low_w16"):
        add(f"dma_{lay}", 257, 72, 48, form="f16x2", layout=lay, tn=3, aim="split terms of the f16x2 form")
        add(f"dma_{lay}_rows", 300, 100, 32, 16, form="f16x2", layout=lay, tn=4, rows=("perm", 257), aim="... subset instance")
        add(f"dma_{lay}_loose", 257, 72, 48, form="f16x2", layout=lay, tn=3, bound_mul=1024.0, aim="bound 2^10 above the data: still exact")
    add("dma_f16x2_loose_small", 257, 72, 48, form="f16x2", tn=3, bound_mul=1024.0, aim="bound 2^10 above the data")
    add("dma_f16x2_zero", 257, 72, 48, form="f16x2", tn=3, zero_a=True, aim="all-zero activations under bound 0: bias, not NaN")
    add("dma_f16x2_zero_rows", 300, 72, 32, 16, form="f16x2", tn=3, zero_a=True, rows=("holes", 257), aim="... on a row list")
    add("dma_no_f16", 257, 72, 48, form="f16x2", tn=3, env=NSM + ("RGNN_LINEAR_NO_F16",), plan_form="bf16x3",
        aim="RGNN_LINEAR_NO_F16: bf16x3 despite the bounds")
    # ---- row lists
    for form in ("bf16x3", "f16x2"):
        for kind, m, cnt in (("asc", 600, 513), ("perm", 600, 513), ("holes", 600, 513), ("tile-1", 600, 700), ("perm", 300, 0), ("long", 100, 600),
                             ("nocount", 257, None)):
            add(f"dma_{form}_rows_{kind}{'' if cnt is None else cnt}", m, 72, 32, 16, form=form, tn=3, rows=(kind, cnt), stats=True, amp=(2, 2), w_nnz=40,
                aim="row list: " + kind)
    # ---- relu / bias / relu_from on the direct instance (relu_from > 0 on a row list leaves the family)
    add("dma_norelu_nobias", 257, 100, 32, tn=4, relu=False, bias=False, aim="no bias, no clamp")
    add("dma_relufrom33", 257, 100, 32, tn=4, relu_from=33, aim="relu_from_col inside a tile, one past a 32-column group")
    add("dma_relufrom96_two_tiles", 257, 200, 32, env=(), tn=2, relu_from=96, aim="relu_from_col inside the second of four tiles")
    add("dma_f16x2_relufrom64", 257, 100, 32, form="f16x2", tn=4, relu_from=64, aim="relu_from_col on a group edge")
    # ---- the BatchNorm-apply tables
    for form in ("bf16x3", "f16x2"):
        for relu_ in (True, False):
            add(f"dma_{form}_affine_relu{int(relu_)}", 257, 72, 32, 16, form=form, tn=3, affine="batch", a1_relu=relu_, aim="whole-batch table")
        add(f"dma_{form}_affine_rows", 300, 72, 48, form=form, tn=3, affine="batch", rows=("holes", 257), stats=True, amp=(1, 1), w_nnz=5,
            aim="table + absent rows: they compute act(t - mean g) W, store and count nothing")
        for k1 in (16, 512):
            add(f"dma_{form}_segments_k{k1}", 700, 72, k1, 16 if k1 % 32 == 0 else 0, form=form, tn=3, affine="segments", segments=(0, 300, 300, 700), rows=("segments", None),
                stats=True, amp=(1, 1), w_nnz=3, aim="per-segment tables, one segment empty")
    # whole-batch table at the largest k1 that fits next to the tiles, and one step past it
    for form, tn, n in (("bf16x3", 7, 224), ("f16x2", 8, 256)):
        room = (LDS_BYTES - dma_lds_bytes(tn, form)) // (AFFINE_ROWS * 4)
        k_fit = room // 16 * 16
        add(f"dma_{form}_affine_fits_k{k_fit}", 130, n, k_fit, form=form, tn=tn, affine="batch", amp=(1, 1), w_nnz=40,
            aim="the largest table next to the widest tile")
        add(f"dma_{form}_affine_too_wide_k{k_fit + 16}", 130, n, k_fit + 16, form=form, tn=tn, affine="batch", amp=(1, 1), w_nnz=40, affine_row=0,
            rc=ERR_UNSUPPORTED, aim="one step past it: not fused, refused, not launched")
    add("dma_segments_k528_refused", 700, 72, 528, form="bf16x3", tn=3, affine="segments", segments=(0, 300, 700), rows=("segments", None),
        amp=(1, 1), w_nnz=3, affine_row=0, rc=ERR_UNSUPPORTED, aim="per-segment tables past k1 = 512: refused")
    return cs


def streamk_rows(n, k, form):
    """The smallest m whose launch has an XCD on the stream-K hand-over (derived from dma_schedule, not by hand)."""
    tn = dma_pick_tn(n, 1 << 20, form, False)
    for mt in range(8 * 32, 8 * 64):
        m = (mt - 1) * DMA_BM_MAX + 1
        if ("streamk", 1) in dma_schedule(m, n, k, tn, form, m, True, False):
            return m
    raise AssertionError("no stream-K shape")


def _schedule_cases():
    cs = []
    NSM = ("RGNN_DMA_NO_SMALL_M",)
    fid = {"bf16x3": 1, "f16x2": 2}

    def add(name, m, n, k, form, sched, env=NSM, ws=True, **kw):
        tn = dma_pick_tn(n, m, form, "RGNN_DMA_NO_SMALL_M" in env)
        sk = int(ws and "RGNN_DMA_NOSK" not in env)
        cs.append(Case(name, m, n, k, form=form, env=env, ws=ws, absmax=True, schedule=sched,
                       expect=_row(DMA, form=fid[form], tile=32 * tn, nt=ceil_div(n, 32 * tn), subset=int(kw.get("rows") is not None), bufl=1, affine=1, split_k=sk), **kw))

    add("sched_static_ws", 257, 72, 48, "bf16x3", (("static", 1),), aim="scratch given, nk < 8: static")
    add("sched_static_tn5", 257, 160, 256, "f16x2", (("static", 1),), aim="TN > 4: never split")
    add("sched_psk2_f16", 257, 72, 256, "f16x2", (("psk", 2),), aim="parallel split-K, S = nk / 4 = 2")
    add("sched_psk2_bf16", 257, 128, 128, "bf16x3", (("psk", 2),), aim="parallel split-K, S = 2, TN = 4")
    add("sched_psk8_bf16", 257, 72, 512, "bf16x3", (("psk", 8),), amp=(5, 5), aim="parallel split-K at the cap S = 8")
    add("sched_psk8_f16_rows", 300, 40, 1024, "f16x2", (("psk", 8),), amp=(2, 2), rows=("holes", 257), stats=True, w_nnz=40,
        aim="S = 8 on a row list with absent rows, statistics after the combine")
    add("sched_psk4", 200, 100, 256, "bf16x3", (("psk", 4),), aim="S = 4 (nk = 16)")
    add("sched_psk_off_nopsk", 257, 72, 512, "bf16x3", (("static", 1),), env=NSM + ("RGNN_DMA_NOPSK",), amp=(5, 5), aim="RGNN_DMA_NOPSK: undivided")
    add("sched_psk_off_nosk", 257, 72, 512, "bf16x3", (("static", 1),), env=NSM + ("RGNN_DMA_NOSK",), amp=(5, 5), aim="RGNN_DMA_NOSK: scratch unused")
    add("sched_psk_off_nows", 257, 72, 512, "bf16x3", (("static", 1),), ws=False, amp=(5, 5), aim="no scratch: undivided")
    for form in ("f16x2", "bf16x3"):
        m = streamk_rows(64, 256, form)
        add(f"sched_streamk_{form}", m, 64, 256, form, (("static", 1), ("streamk", 1)), env=(), amp=(3, 3),
            aim="stream-K hand-over on the XCD with one panel too many")
    m = streamk_rows(64, 256, "f16x2")
    add("sched_streamk_off_nosk", m, 64, 256, "f16x2", (("static", 1),), env=("RGNN_DMA_NOSK",), amp=(3, 3), aim="RGNN_DMA_NOSK: whole tiles")
    return cs


TINY_CASES, FP32_CASES, X3_CASES, DMA_CASES, SCHEDULE_CASES = _tiny_cases(), _fp32_cases(), _x3_cases(), _dma_cases(), _schedule_cases()
ALL_CASES = TINY_CASES + FP32_CASES + X3_CASES + DMA_CASES + SCHEDULE_CASES
for _c in X3_CASES + DMA_CASES + SCHEDULE_CASES:              # (a split-product launch: 16-byte loads, descriptors)
    _c.vec = True


def by_name(name):
    return next(c for c in ALL_CASES if c.name == name)


# the instances of section "Instances and edges to cover": plan rows projected on (family, form, tile columns, subset)
REQUIRED_INSTANCES = (
    [(TINY, 0, 0, 0)] + [(FP32, 0, t, 0) for t in (32, 64, 128, 96, 160, 192, 224)]
    + [(X3, 1, t, s) for t in (32, 64, 128, 256) for s in (0, 1)]
    + [(DMA, 1, 32 * tn, s) for tn in range(2, 8) for s in (0, 1)] + [(DMA, 2, 32 * tn, s) for tn in range(2, 9) for s in (0, 1)])
# ... and the instances no argument set reaches (never forced): the fp32 wide_tn = 4 instance (launch<128, 4, 1, 1, 4, 1, true>,
# linear.hip:1143: 128-wide tiles pad exactly what the 128 ladder pads, and the choice wants 5 % less), and the four-wave
# work-group form of k_linear_dma (dma_four_waves returns false without RGNN_DMA_WAVES)
UNREACHABLE = ("fp32 wide_tn = 4", "k_linear_dma<TN, IDX, 1, 4> (four-wave work-groups)")
