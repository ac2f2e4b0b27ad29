"""Aggregations min | var | std (RGNN_AGGR_MIN / _VAR / _STD) on the device: the per-edge kernels k_mpnn and k_mpnn_fast at AGGR 3 - 5 (the
latter is the one a launch with a chunk table takes where d % 4 == 0 and de <= 8: every forward case runs with and without the table), the
row kernels k_segment_reduce / k_segment_reduce_bwd at AGGR 3 - 5, the backward kernels (k_mpnn_bwd_arg with the comparison turned round,
k_mpnn_bwd_coef / _edge_var / _src_var) on the hand-built CSRs of tests/mpnn_csr_cases.py and tests/mpnn_bwd_cases.py, and the conv
layers, the model, HotPath and per-frame BatchNorm with the three names.  Reference: tests/aggr_ext_oracle.py (the literal formulas
of torch_geometric 2.1.0 / torch-scatter in torch index ops, float64; the float32 evaluation of the same, target term inside the
message, is the reference-shaped yardstick).

Bars.
* min on integers: bit-equal.
* var / std on small integers (|m| <= 16, in-degrees <= 1000): with d_e = m_e - m_0 every |d_e| <= 32 and every partial sum of d and
  d^2 is an integer below 1000 * 32^2 < 2^24, so the device's two sums are EXACT in fp32 whatever their order.  What is left is the
  epilogue, with u = 2^-24 and E2 = sum d^2 / cnt >= mu^2, |var|:  s2 / cnt (one rounding, <= u E2), mu = s1 / cnt (one rounding),
  mu * mu (relative 3 u), the subtraction (u |var|):  |var_dev - var| <= 5 u E2.  std = sqrt(var + 1e-5f): the sum is rounded once
  (u (var + 1e-5)), the fp32 constant is off by 2.6e-13, the square root is rounded once (2 u allowed):
  |std_dev - std| <= (5 u E2 + u (var + 1e-5) + 2.6e-13) / (2 std) + 2 u std.  All-equal segments: var exactly 0, std exactly the
  fp32 sqrt(1e-5).
* var / std on float data: worst absolute error against float64 <= max((a) the reference-shaped float32 evaluation's own worst
  error on the same case, (b) 1e-5 * max |float64 result|); on the offset case (messages 1e3 + spread 1) inside (b) alone.
* backward: the bar of the mean cases of tests/test_gpu_mpnn_bwd_edges.py -- every element's error divided by its sum of |terms|,
  at most 4 x the same figure of the float32 torch evaluation + 2e-7 -- or the reference-shaped float32 autograd's own figure where
  that is larger.
* layers / model: norm-wise 1e-5 against float64 (or the reference-shaped float32 error where that is larger), parameter gradients
  at the 2e-5 of tests/test_gpu_backward.py."""
import copy
import functools
import math

import numpy as np
import pytest
import torch

import aggr_ext_oracle as ax
import mpnn_bwd_cases as bc
import mpnn_csr_cases as mc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
S0_F32 = torch.tensor(1e-5, dtype=torch.float32).sqrt()                # the fp32 value of sqrt(1e-5), correctly rounded
CHANNELS = (1, 8, 33, 224)
EDGE_WIDTHS = (0, 3, 8)
FWD_CASES = ("degrees_1_to_8/nonempty_ends", "degrees_1_to_8/empty_ends", "all_1/513", "all_33", "leftover_blocks",
             "multi_edges_and_self_loops", "empty_graph_parts/empty_full_one", "empty_graph_parts/no_edges")
BWD_CASES = bc.IN_DEGREE_CASES + bc.TINY_CASES + ("out_degrees", "multi_edges_and_self_loops", "no_edges", "empty_then_full")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    from radargnn_amd import ops as _ops
    return _ops


def f32(t):
    return None if t is None else t.to(torch.float32).cuda()


def normwise(a, b) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


# ------------------------------------------------------------------------------------------------ forward, kernel level
def target_nodes(c, order):
    """Per sorted edge: the NODE it is aggregated at (segment p belongs to node order[p])."""
    tgt = torch.repeat_interleave(torch.arange(c.n), torch.from_numpy(c.deg))
    return tgt if order is None else order.long()[tgt]


def messages(c, Q, We, ea, dtype):
    msg = Q.to(dtype)[torch.from_numpy(c.src_np)]
    if We is not None and ea is not None and ea.shape[1] > 0:
        msg = msg + ea.to(dtype) @ We.to(dtype).t()
    return msg


def reference(c, Q, We, ea, P, b, order, aggr, dtype):
    """aggr_e(P[t] + b + Q[s_e] + W_e a_e) literally (the target term INSIDE the message, as the reference's layers have it)."""
    node = target_nodes(c, order)
    msg = messages(c, Q, We, ea, dtype)
    if b is not None:
        msg = msg + b.to(dtype)
    if P is not None:
        msg = msg + P.to(dtype)[node]
    return ax.reduce_rows(msg, node, c.n, aggr)


def launch(ops, c, order, Q, We, ea, P, b, aggr, chunks=False):
    rowptr, src = c.rowptr_t.cuda(), c.src_sorted.cuda()
    ch = ops.mpnn_partition(rowptr, c.n_edges) if chunks else None
    return ops.mpnn_aggregate(f32(P), f32(b), f32(Q), f32(We), f32(ea), rowptr, src, aggr,
                              node_order=None if order is None else order.cuda(), chunks=ch)


def variants(c):
    """(d, de, node_order, with the target term and the bias) -- every combination."""
    for d in CHANNELS:
        for de in EDGE_WIDTHS:
            for order in c.orders():
                for with_p in (False, True):
                    yield d, de, order, with_p


def small_int_inputs(c, d, de, with_p, seed=0):
    """Q in [-8, 8], W_e and a in [-1, 1] (|W_e a| <= 8, |m| <= 16), P and b in [-4, 4]: float64 tensors of integers."""
    g = torch.Generator().manual_seed(1234 + seed + 17 * d + de)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).double()
    Q = ri(-8, 8, (c.n, d))
    We, ea = (ri(-1, 1, (d, de)), ri(-1, 1, (c.n_edges, de))) if de else (None, None)
    P, b = (ri(-4, 4, (c.n, d)), ri(-4, 4, (d,))) if with_p else (None, None)
    return Q, We, ea, P, b


@pytest.mark.parametrize("name", FWD_CASES)
def test_min_is_bit_equal_on_integers(ops, name):
    """``mc.int_inputs``: every source carries a bonus on one channel; the ``negative`` variant puts every message below zero, so a
    row of a target without edges (exactly 0, not +inf) cannot be mistaken for a minimum, and in the other variant minima of 0 occur."""
    c = mc.case(name)
    zero_minima = 0
    for d, de, order, with_p in variants(c):
        for negative in (False, True):
            Q, We, ea, b = mc.int_inputs(c, d=d, de=de, with_bias=with_p, negative=negative)
            P = torch.randint(-4, 5, (c.n, d), generator=torch.Generator().manual_seed(d + de)) if with_p else None
            exp = reference(c, Q, We, ea, P, b, order, "min", torch.float64)
            has = torch.zeros(c.n, dtype=torch.bool)
            has[target_nodes(c, order)] = True
            for chunks in (False, True):                                     # k_mpnn / (d % 4 == 0) k_mpnn_fast
                out = launch(ops, c, order, Q, We, ea, P, b, "min", chunks=chunks).cpu()
                what = f"{name} d={d} de={de} order={order is not None} P={with_p} negative={negative} chunks={chunks}"
                assert torch.equal(out, exp.to(torch.float32)), f"{what}: {int((out != exp.to(torch.float32)).sum())} elements differ"
                assert bool((out[~has] == 0).all()) and bool(torch.isfinite(out).all()), what
                if negative and not with_p:
                    assert bool((out[has] < 0).all()), what                  # no empty-row zero among the minima
            zero_minima += int((exp[has] == 0).sum())
    if c.n_edges:
        assert zero_minima > 0                                               # real minima of exactly 0 were among the cases


@pytest.mark.parametrize("aggr", ["var", "std"])
@pytest.mark.parametrize("name", FWD_CASES)
def test_var_std_with_exact_sums(ops, name, aggr):
    """Small integers: both device sums are exact, the error is the epilogue's (module docstring).  Single-edge and all-equal
    segments give exactly 0 / exactly sqrt(1e-5)."""
    c = mc.case(name)
    worst = 0.0
    for d, de, order, with_p in variants(c):
        Q, We, ea, P, b = small_int_inputs(c, d, de, with_p)
        node = target_nodes(c, order)
        equal_seg = torch.zeros(c.n, dtype=torch.bool)                       # segments of several edges, all from ONE source
        if name == "multi_edges_and_self_loops":
            for p in (31,):                                                  # sources [31, 31]: equal attributes make equal messages
                lo, hi = int(c.rowptr_np[p]), int(c.rowptr_np[p + 1])
                assert hi - lo == 2 and c.src_np[lo] == c.src_np[lo + 1]
                if ea is not None:
                    ea[lo + 1] = ea[lo]
                equal_seg[p if order is None else int(order[p])] = True
        msg = messages(c, Q, We, ea, torch.float64)
        assert c.n_edges == 0 or float(msg.abs().max()) <= 16
        exp = reference(c, Q, We, ea, P, b, order, aggr, torch.float64)
        var = ax.reduce_rows(msg, node, c.n, "var")
        # E2 = sum (m_e - m_0)^2 / cnt with m_0 the segment's first message in CSR order
        first = torch.from_numpy(c.rowptr_np[:-1].copy())[torch.repeat_interleave(torch.arange(c.n), torch.from_numpy(c.deg))]
        dd = msg - msg[first] if c.n_edges else msg
        cnt = torch.bincount(node, minlength=c.n).clamp(min=1).double().view(-1, 1)
        e2 = torch.zeros((c.n, d), dtype=torch.float64).index_add(0, node, dd * dd) / cnt
        tol = 5 * U * e2
        if aggr == "std":
            std = torch.sqrt(torch.relu(var) + 1e-5)
            tol = (tol + U * (var + 1e-5) + 2.6e-13) / (2 * std) + 2 * U * std
        deg_node = torch.zeros(c.n, dtype=torch.int64)
        deg_node[torch.from_numpy(np.arange(c.n) if order is None else order.numpy().astype(np.int64))] = torch.from_numpy(c.deg)
        flat = (deg_node <= 1) | equal_seg                                  # no edge, one edge, or equal messages
        fill = S0_F32 if aggr == "std" else torch.tensor(0.0)
        for chunks in (False, True):                                         # k_mpnn / (d % 4 == 0, de <= 8) k_mpnn_fast
            out = launch(ops, c, order, Q, We, ea, P, b, aggr, chunks=chunks).cpu()
            err = (out.double() - exp).abs()
            what = f"{name} {aggr} d={d} de={de} order={order is not None} P={with_p} chunks={chunks}"
            assert bool((err <= tol).all()), f"{what}: error {float((err - tol).max()):.3e} above the epilogue bound"
            worst = max(worst, float((err / tol.clamp_min(1e-300))[tol > 0].max()) if bool((tol > 0).any()) else 0.0)
            assert bool((out[flat] == fill).all()), f"{what}: flat segments must give exactly {float(fill)}"
    print(f"\n[aggr_ext] {name} {aggr}: worst error / epilogue bound {worst:.3f}")


@functools.lru_cache(maxsize=None)
def float_case(name, d, de, ordered, with_p):
    c = mc.case(name)
    order = c.node_order if ordered else None
    Q, We, ea, b = mc.float_inputs(c, d=d, de=de)
    P = None
    if with_p:
        P = torch.randn(c.n, d, generator=torch.Generator().manual_seed(d)) * Q.abs().mean(0)
    else:
        b = None
    if de == 0:
        We = ea = None
    refs = {a: (reference(c, Q, We, ea, P, b, order, a, torch.float64), reference(c, Q, We, ea, P, b, order, a, torch.float32)) for a in ("var", "std")}
    return (Q, We, ea, P, b), refs


@pytest.mark.parametrize("aggr", ["var", "std"])
@pytest.mark.parametrize("name", FWD_CASES)
def test_var_std_on_float_data(ops, name, aggr):
    """Magnitudes over four decades across the channels.  The worst error is at most the larger of the reference-shaped float32
    evaluation's own (a) and 1e-5 of the largest result (b)."""
    c = mc.case(name)
    for d, de, order, with_p in variants(c):
        (Q, We, ea, P, b), refs = float_case(name, d, de, order is not None, with_p)
        r64, r32 = refs[aggr]
        a_ = float((r32.double() - r64).abs().max())
        b_ = 1e-5 * float(r64.abs().max())
        for chunks in (False, True):
            out = launch(ops, c, order, Q, We, ea, P, b, aggr, chunks=chunks).cpu()
            e_dev = float((out.double() - r64).abs().max())
            print(f"[aggr_ext] {name} {aggr} d={d} de={de} order={order is not None} P={with_p} chunks={chunks}: device {e_dev:.3e}  (a) {a_:.3e}  (b) {b_:.3e}")
            assert e_dev <= max(a_, b_), (name, aggr, d, de, with_p, chunks, e_dev, a_, b_)


@pytest.mark.parametrize("aggr", ["var", "std"])
@pytest.mark.parametrize("de", EDGE_WIDTHS)
def test_a_common_offset_of_1e3_costs_no_digits(ops, aggr, de):
    """Messages 1e3 + (spread 1), all on the grid of 2^-14 that fp32 has there (Q on multiples of 2^-10, W_e a on multiples of 2^-10):
    every message is exact in fp32 and the same number in float64.  The literal float32 formula loses everything (1e6 - 1e6); the
    device shifts by the first message and must be inside 1e-5 of the largest result, yardstick (a) not consulted."""
    c = mc.case("degrees_1_to_8/empty_ends")
    g = torch.Generator().manual_seed(8 + de)
    for d in CHANNELS:
        Q = 1000.0 + torch.randint(0, 1024, (c.n, d), generator=g).double() / 1024
        We = torch.randint(-2, 3, (d, de), generator=g).double() / 64 if de else None
        ea = torch.randint(-3, 4, (c.n_edges, de), generator=g).double() / 16 if de else None
        msg = messages(c, Q, We, ea, torch.float64)
        assert torch.equal(msg.to(torch.float32).double(), msg)
        for order in c.orders():
            r64 = reference(c, Q, We, ea, None, None, order, aggr, torch.float64)
            r32 = reference(c, Q, We, ea, None, None, order, aggr, torch.float32)
            a_, b_ = float((r32.double() - r64).abs().max()), 1e-5 * float(r64.abs().max())
            assert a_ > 10 * b_                                              # the case is adversarial for the literal float32 formula
            for chunks in (False, True):
                out = launch(ops, c, order, Q, We, ea, None, None, aggr, chunks=chunks).cpu()
                e_dev = float((out.double() - r64).abs().max())
                print(f"[aggr_ext] offset {aggr} d={d} de={de} chunks={chunks}: device {e_dev:.3e}  (a) {a_:.3e}  (b) {b_:.3e}")
                assert e_dev <= b_, (aggr, d, de, chunks, e_dev, b_)


@pytest.mark.parametrize("aggr", ax.AGGRS)
def test_both_per_edge_kernels_give_the_same_bits_past_256_channels(ops, aggr):
    """More than 256 channels: k_mpnn_fast takes two channel groups per lane (min; var / std with at most 4 attributes) or several
    blocks in y (var / std with 5 .. 8 attributes), k_mpnn several passes.  Both do the same operations on a channel in the same
    order: the same bits.  Against float64 at the yardsticks of the float test (min: 1e-5 of the largest result)."""
    for name in ("degrees_1_to_8/empty_ends", "leftover_blocks"):
        c = mc.case(name)
        for d in (260, 520, 772):
            for de in (3, 8):
                (Q, We, ea, P, b), refs = float_case(name, d, de, True, True)
                plain = launch(ops, c, c.node_order, Q, We, ea, P, b, aggr, chunks=False)
                fast = launch(ops, c, c.node_order, Q, We, ea, P, b, aggr, chunks=True)
                assert torch.equal(plain, fast), (name, aggr, d, de, int((plain != fast).sum()))
                if aggr == "min":
                    r64 = reference(c, Q, We, ea, P, b, c.node_order, "min", torch.float64)
                    assert float((fast.cpu().double() - r64).abs().max()) <= 1e-5 * float(r64.abs().max()), (name, d, de)
                else:
                    r64, r32 = refs[aggr]
                    e_dev, a_, b_ = float((fast.cpu().double() - r64).abs().max()), float((r32.double() - r64).abs().max()), 1e-5 * float(r64.abs().max())
                    assert e_dev <= max(a_, b_), (name, aggr, d, de, e_dev, a_, b_)


@pytest.mark.parametrize("aggr", ["var", "std"])
def test_var_std_ignore_the_target_term(ops, aggr):
    c = mc.case("degrees_1_to_8/empty_ends")
    for d in CHANNELS:
        for de in EDGE_WIDTHS:
            (Q, We, ea, _, _), _ = float_case(c.name, d, de, True, False)
            for chunks in (False, True):
                plain = launch(ops, c, c.node_order, Q, We, ea, None, None, aggr, chunks=chunks)
                huge = launch(ops, c, c.node_order, Q, We, ea, torch.full((c.n, d), 3e30), torch.full((d,), -1e30), aggr, chunks=chunks)
                assert torch.equal(plain, huge), (aggr, d, de, chunks)


@pytest.mark.parametrize("aggr", ax.AGGRS)
def test_the_bound_is_the_largest_magnitude_written(ops, aggr):
    for name in ("degrees_1_to_8/empty_ends", "leftover_blocks", "empty_graph_parts/no_edges"):
        c = mc.case(name)
        for d in CHANNELS:
            for with_p in (False, True):
                (Q, We, ea, P, b), _ = float_case(name, d, 3, True, with_p)
                for chunks in (False, True):
                    with ops.bound_tracking("cuda") as pool:
                        assert pool is not None
                        out = launch(ops, c, c.node_order, Q, We, ea, P, b, aggr, chunks=chunks)
                        bound = ops.bound_of(out)
                    assert bound is not None and bound.numel() == ops.BOUND_SLOTS
                    assert float(bound.max()) == float(out.abs().max()), (name, aggr, d, with_p, chunks)


# ------------------------------------------------------------------------------------------------ rows: segment_reduce
@pytest.mark.parametrize("d", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("name", bc.IN_DEGREE_CASES + bc.TINY_CASES + ("no_edges",))
def test_segment_reduce_over_rows(ops, name, d):
    """Integer rows in [-3, 3] (``bc.row_inputs``): min bit-equal, var / std by the epilogue bound (|d_e| <= 6, sums exact), then float
    rows against the two yardsticks.  301 segments (no multiple of the 4 a block takes), segments up to 300 rows, 1 .. 130 channels
    (more than the 64 a wave covers per trip)."""
    c = bc.case(name)
    rows, _ = bc.row_inputs(c, d)
    frows = torch.randn(c.n_edges, d, generator=torch.Generator().manual_seed(d)) * torch.logspace(-2, 2, d) + 3.0
    for order in c.orders():
        node = target_nodes(c, order)
        o = None if order is None else order.cuda()
        for aggr in ax.AGGRS:
            exp = ax.reduce_rows(rows.double(), node, c.n, aggr)
            out = ops.segment_reduce(f32(rows), c.rowptr_t.cuda(), aggr, node_order=o).cpu()
            assert out.shape == (c.n, d)
            if aggr == "min":
                assert torch.equal(out, exp.to(torch.float32)), (name, d)
            else:
                tol = 5 * U * 36.0 * torch.ones_like(exp)
                if aggr == "std":
                    tol = (tol + U * (exp * exp) + 2.6e-13) / (2 * exp) + 2 * U * exp
                assert bool(((out.double() - exp).abs() <= tol).all()), (name, d, aggr, float((out.double() - exp).abs().max()))
            r64 = ax.reduce_rows(frows.double(), node, c.n, aggr)
            r32 = ax.reduce_rows(frows, node, c.n, aggr)
            got = ops.segment_reduce(frows.cuda(), c.rowptr_t.cuda(), aggr, node_order=o).cpu()
            e_dev, a_, b_ = float((got.double() - r64).abs().max()), float((r32.double() - r64).abs().max()), 1e-5 * float(r64.abs().max())
            assert e_dev <= max(a_, b_), (name, d, aggr, e_dev, a_, b_)
            empty = torch.ones(c.n, dtype=torch.bool)
            empty[node] = False
            assert bool((got[empty] == (S0_F32 if aggr == "std" else 0.0)).all())


# ------------------------------------------------------------------------------------------------ backward, kernel level
class BwdGraph:
    def __init__(self, c, ordered):
        self.c = c
        self.order_cpu = c.node_order if ordered else None
        self.rowptr, self.src = c.rowptr_t.cuda(), c.src_sorted.cuda()
        self.order = None if self.order_cpu is None else self.order_cpu.cuda()
        self.source_csr = tuple(t.cuda() for t in c.source_csr(self.order_cpu))
        self.start = torch.zeros(c.n, dtype=torch.int64)
        self.start[torch.from_numpy(c.order_np(self.order_cpu))] = torch.from_numpy(c.rowptr_np[:-1])
        self.has = torch.zeros(c.n, dtype=torch.bool)
        self.has[torch.from_numpy(c.order_np(self.order_cpu))] = torch.from_numpy(c.deg > 0)


@functools.lru_cache(maxsize=None)
def bwd_graph(name, ordered):
    return BwdGraph(bc.case(name), ordered)


def backward(ops, g, inputs, aggr, want_arg=False):
    Q, We, ea, dM = inputs
    arg_out = torch.full((g.c.n, Q.shape[1]), -7, dtype=torch.int32, device="cuda") if want_arg else None
    dQ, dea, dWe = ops.mpnn_aggregate_bwd(f32(dM), f32(Q), f32(We), f32(ea), g.rowptr, g.src, aggr, g.source_csr, node_order=g.order,
                                          arg_out=arg_out)
    loc = None
    if want_arg and g.c.n_edges:
        loc = arg_out.cpu().long() - g.start[:, None]
    return dQ, dea, dWe, loc


def autograd_grads(c, order, Q, We, ea, dM, aggr, dtype):
    """Autograd through the literal formula -> ((dQ, dea, dWe), G [E, d] = d loss / d message), all in ``dtype``."""
    node = torch.from_numpy(c.tgt_node(order))
    Ql = Q.to(dtype).clone().requires_grad_(True)
    Wl = None if We is None else We.to(dtype).clone().requires_grad_(True)
    el = None if ea is None else ea.to(dtype).clone().requires_grad_(True)
    msg = Ql[torch.from_numpy(c.src_np)]
    if Wl is not None:
        msg = msg + el @ Wl.t()
    msg.retain_grad()
    (ax.reduce_rows(msg, node, c.n, aggr) * dM.to(dtype)).sum().backward()
    return (Ql.grad, None if el is None else el.grad, None if Wl is None else Wl.grad), msg.grad


def term_sums(c, G, We, ea):
    """Sum of |terms| of every output element (float64), as ``bc.grads`` defines them."""
    A = G.double().abs()
    dQ = torch.zeros((c.n, G.shape[1]), dtype=torch.float64).index_add_(0, torch.from_numpy(c.src_np), A)
    if We is None:
        return dQ, None, None
    return dQ, A @ We.double().abs(), A.t() @ ea.double().abs()


def assert_no_edges(got, n, d):
    assert got[0].shape == (n, d) and bool((got[0] == 0).all())
    assert got[1] is None or got[1].numel() == 0
    assert got[2] is None or bool((got[2] == 0).all())


@pytest.mark.parametrize("name", BWD_CASES)
def test_min_backward_exact_on_integers(ops, name):
    """min_e m_e = -max_e(-m_e): the winners of ``bc.first_id`` on (Q, W_e) are the first minimisers of (-Q, -W_e).  ``spread``: a
    strict unique minimum per edge; ``all_tie``: the gradient lands on the FIRST edge of every segment and nowhere else."""
    c = bc.case(name)
    for ordered in (False, True):
        g = bwd_graph(name, ordered)
        for layout in ("spread", "all_tie"):
            Q, We, ea, dM = bc.int_inputs(c, layout)
            loc = bc.first_id(c, Q, We, ea, g.order_cpu)[0]
            nQ, nW = -Q, None if We is None else -We
            ref, _ = bc.grads(c, dM, nW, ea, "max", g.order_cpu, loc)
            got = backward(ops, g, (nQ, nW, ea, dM), "min", want_arg=True)
            if c.n_edges == 0:
                assert_no_edges(got, c.n, c.d)
                continue
            assert torch.equal(got[3][g.has], loc[g.has]), (name, layout, ordered)
            if layout == "all_tie":
                assert bool((got[3][g.has] == 0).all())
            for nm, a, b in zip(("dQ", "d_edge_attr", "dW_e"), got[:3], ref):
                assert torch.equal(a.cpu(), b.to(torch.float32)), (name, layout, ordered, nm)


@pytest.mark.parametrize("name", BWD_CASES)
def test_std_backward_is_exactly_zero_where_the_variance_is(ops, name):
    """``all_tie``: every message of a segment is the same number, var = 0 on every channel: no edge, no source and no weight receives
    anything (relu'(0) = 0), not a rounding error's worth.  var's gradient 2 (m_e - mean) / cnt is exactly 0 there as well."""
    c = bc.case(name)
    g = bwd_graph(name, True)
    Q, We, ea, dM = bc.int_inputs(c, "all_tie")
    for aggr in ("std", "var"):
        got = backward(ops, g, (Q, We, ea, dM), aggr)
        if c.n_edges == 0:
            assert_no_edges(got, c.n, c.d)
            continue
        for nm, a in zip(("dQ", "d_edge_attr", "dW_e"), got[:3]):
            assert a is not None and bool((a == 0).all()), (name, aggr, nm, float(a.abs().max()))


def scaled(x, r64, sums):
    on = sums > 0
    assert bool((x[~on] == 0).all())
    return float(((x.double() - r64).abs() / sums)[on].max()) if bool(on.any()) else 0.0


@pytest.mark.parametrize("aggr", ax.AGGRS)
@pytest.mark.parametrize("name", BWD_CASES)
def test_backward_on_float_data(ops, name, aggr):
    """dQ, d_edge_attr and dW_e against float64 autograd of the literal formula at the bar of the mean cases (module docstring).  min is
    routed through the winners the launch itself found (they must be minimisers); e_f32 is the float32 autograd of the same formula --
    at this level, without a target term, also the reference-shaped one."""
    c = bc.case(name)
    g = bwd_graph(name, True)
    Q, We, ea, dM = bc.float_inputs(c)
    got = backward(ops, g, (Q, We, ea, dM), aggr, want_arg=aggr == "min")
    if c.n_edges == 0:
        assert_no_edges(got, c.n, c.d)
        return
    if aggr == "min":
        loc = got[3]
        node = torch.from_numpy(c.tgt_node(g.order_cpu))
        msg = messages(c, Q, We, ea, torch.float64)
        low = ax.reduce_rows(msg, node, c.n, "min")
        pos = (g.start[:, None] + loc)[g.has]                               # CSR position of every winner
        scale = mc.error_scale(c, Q, We, ea, None, g.order_cpu)[0][g.has]
        assert bool(((msg.gather(0, pos) - low[g.has]).abs() <= 4 * U * scale).all())      # a minimiser up to the rounding of a message
        r64, s64 = bc.grads(c, dM.double(), We.double(), ea.double(), "max", g.order_cpu, loc, torch.float64)
        r32, _ = bc.grads(c, dM, We, ea, "max", g.order_cpu, loc, torch.float32)
        sums = s64
    else:
        r64, G = autograd_grads(c, g.order_cpu, Q, We, ea, dM, aggr, torch.float64)
        r32, _ = autograd_grads(c, g.order_cpu, Q, We, ea, dM, aggr, torch.float32)
        sums = term_sums(c, G, We, ea)
    for nm, x, a, b, s in zip(("dQ", "d_edge_attr", "dW_e"), got[:3], r64, r32, sums):
        e_kernel, e_f32 = scaled(x.cpu(), a, s), scaled(b, a, s)
        bar = max(4 * e_f32 + 2e-7, e_f32)
        print(f"\n[aggr_ext] {name} {aggr} {nm}: d={c.d} de={c.de} scaled error kernel {e_kernel:.3e}  float32 autograd {e_f32:.3e}  bar {bar:.3e}")
        assert e_kernel <= bar, (name, aggr, nm, e_kernel, e_f32)


@pytest.mark.parametrize("d,de", [(1, 0), (5, 3), (33, 1), (300, 9), (516, 16)])
def test_backward_across_widths(ops, d, de):
    """Channel counts around the 4-channel groups and the 64-lane passes, edge widths on every DEP instantiation (4, 8, 16), rows that
    take the scalar form (d % 4 != 0)."""
    c = bc.case("out_degrees")
    g = bwd_graph("out_degrees", True)
    Q, We, ea, dM = bc.float_inputs(c, d=d, de=de)
    if de == 0:
        We = ea = None
    for aggr in ("var", "std"):
        got = backward(ops, g, (Q, We, ea, dM), aggr)
        r64, G = autograd_grads(c, g.order_cpu, Q, We, ea, dM, aggr, torch.float64)
        r32, _ = autograd_grads(c, g.order_cpu, Q, We, ea, dM, aggr, torch.float32)
        for nm, x, a, b, s in zip(("dQ", "d_edge_attr", "dW_e"), got[:3], r64, r32, term_sums(c, G, We, ea)):
            if a is None:
                assert x is None
                continue
            e_kernel, e_f32 = scaled(x.cpu(), a, s), scaled(b, a, s)
            assert e_kernel <= max(4 * e_f32 + 2e-7, e_f32), (aggr, d, de, nm, e_kernel, e_f32)


@pytest.mark.parametrize("d", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("name", bc.IN_DEGREE_CASES + bc.TINY_CASES)
def test_segment_reduce_bwd_over_rows(ops, name, d):
    """Integer rows: min bit-exact (exact ties in nearly every segment, the first row takes the gradient); float rows: var / std at the
    bar of the mean cases, every element ONE term."""
    c = bc.case(name)
    rows, dM = bc.row_inputs(c, d)
    frows = torch.randn(c.n_edges, d, generator=torch.Generator().manual_seed(d + 1)) * torch.logspace(-2, 2, d)
    fdM = torch.randn(c.n, d, generator=torch.Generator().manual_seed(d + 2))
    for ordered in (False, True):
        g = bwd_graph(name, ordered)
        node = torch.from_numpy(c.tgt_node(g.order_cpu))
        exp = ax.closed_form_grad(rows.double(), node, c.n, "min", dM.double())
        got = ops.segment_reduce_bwd(f32(dM), f32(rows), g.rowptr, "min", node_order=g.order).cpu()
        assert torch.equal(got, exp.to(torch.float32)), (name, d, ordered)
        for aggr in ("var", "std"):
            def auto(dtype):
                leaf = frows.to(dtype).clone().requires_grad_(True)
                (ax.reduce_rows(leaf, node, c.n, aggr) * fdM.to(dtype)).sum().backward()
                return leaf.grad
            r64, r32 = auto(torch.float64), auto(torch.float32)
            got = ops.segment_reduce_bwd(fdM.cuda(), frows.cuda(), g.rowptr, aggr, node_order=g.order).cpu()
            e_kernel, e_f32 = scaled(got, r64, r64.abs()), scaled(r32, r64, r64.abs())
            assert e_kernel <= max(4 * e_f32 + 2e-7, e_f32), (name, d, aggr, ordered, e_kernel, e_f32)
        flat = ops.segment_reduce_bwd(fdM.cuda(), torch.full((c.n_edges, d), 2.5).cuda(), g.rowptr, "std", node_order=g.order)
        assert bool((flat == 0).all())                                       # var = 0: relu'(0) = 0


# ------------------------------------------------------------------------------------------------ layers and the model
LAYER_CASES = [
    # (conv type, edge encoder, pre_layers, node embedding, edge embedding, conv widths)
    ("MPNNConv", False, 1, [16, 24], [4, 8], [24, 16]),
    ("MPNNConv", False, 2, [16, 24], [4, 8], [24, 16]),
    ("MPNNConv", True, 1, [8, 12], None, [12, 20]),
    ("RadarPointGNNConv", False, 1, [16, 24], [4, 8], [24, 24]),
]
GTOL = 2e-5                                                                  # tests/test_gpu_backward.py
K = 3


def two_frames():
    from radargnn_amd import synthetic
    return [synthetic.small_frame(100, 0), synthetic.small_frame(101, 1)]     # 201 nodes in 2 frames


def build_model(gnn, case, aggr, seed=21):
    conv_type, enc, pre, node_emb, edge_emb, dims = case
    cfg = gnn.GNNArchitectureConfig(
        node_feature_dimension=5, edge_feature_dimension=2, conv_layer_dimensions=dims,
        classification_head_layer_dimensions=[6], regression_head_layer_dimensions=[16, 5],
        initial_node_feature_embedding=node_emb is not None, initial_edge_feature_embedding=edge_emb is not None,
        node_feature_embedding_layer_dimensions=node_emb or [], edge_feature_embedding_layer_dimensions=edge_emb or [],
        conv_layer_type=conv_type, batch_norm_in_mlps=False, conv_use_edge_encoder=enc, aggregation_function=aggr,
        conv_pre_mlp_layer_number=pre, conv_post_mlp_layer_number=1)
    torch.manual_seed(seed)
    model = gnn.DetNetBasic(cfg).cuda()
    with torch.no_grad():
        for bn in model.batch_norms:
            bn.module.weight.uniform_(0.5, 1.5)
            bn.module.bias.uniform_(-0.5, 0.5)
    return model


def in_degree(ei, n):
    return torch.bincount(ei[1].cpu(), minlength=n)


def oracle_run(model, x, ei, ea, conv_type, aggr, rc, rb, dtype, grads):
    sd = {k: (v.detach().cpu().to(dtype).requires_grad_(grads and "running" not in k) if v.is_floating_point() else v.detach().cpu())
          for k, v in model.state_dict().items()}
    c, bb = ax.det_net_basic(x.cpu(), ei.cpu(), ea.cpu(), sd, conv_type, aggr, training=True, dtype=dtype)
    if not grads:
        return c.detach(), bb.detach(), None
    ((c * rc.to(dtype)).sum() + (bb * rb.to(dtype)).sum()).backward()
    return c.detach(), bb.detach(), {k: v.grad for k, v in sd.items() if v.is_floating_point() and v.requires_grad and v.grad is not None}


@pytest.mark.parametrize("aggr", ax.AGGRS)
@pytest.mark.parametrize("case", LAYER_CASES, ids=lambda c: f"{c[0]}-enc{int(c[1])}-pre{c[2]}")
def test_model_forward_backward_hotpath_and_frames(case, aggr):
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    import radargnn_amd.gnn as gnn
    from radargnn_amd import frames as fr
    conv_type = case[0]
    frames = two_frames()
    settings = fr.GraphSettings(algorithm="knn", k=K)
    batch = fr.FrameBatch.from_frames(frames)
    model = build_model(gnn, case, aggr)

    # ---- HotPath (its own kNN graph: some nodes are nobody's neighbour), eager and replayed, against the public forward
    cls_h, bb_h, g = fr.HotPath(copy.deepcopy(model), settings)(batch)
    g.check()
    n = g.x.shape[0]
    assert n == 201 and g.edge_index.shape[1] == n * K
    assert int((in_degree(g.edge_index, n) == 0).sum()) >= 3                   # isolated rows (std: sqrt(1e-5)) reach the BatchNorm
    c_pub, b_pub = copy.deepcopy(model)(g.x, g.edge_index, g.edge_attr)
    assert normwise(c_pub, cls_h) < 1e-6 and normwise(b_pub, bb_h) < 1e-6       # (another visiting order: same values)
    c64, b64, _ = oracle_run(model, g.x, g.edge_index, g.edge_attr, conv_type, aggr, None, None, torch.float64, False)
    c32, b32, _ = oracle_run(model, g.x, g.edge_index, g.edge_attr, conv_type, aggr, None, None, torch.float32, False)
    for nm, dev, r64, r32 in (("logits", cls_h, c64, c32), ("boxes", bb_h, b64, b32)):
        bar = max(1e-5, normwise(r32, r64))
        assert normwise(dev, r64) < bar, (f"{nm}: {normwise(dev, r64):.2e} against float64; bar 1e-5 or the reference-shaped float32 "
                                          f"evaluation's own {normwise(r32, r64):.2e}")
    hot = fr.HotPath(copy.deepcopy(model), settings, use_hip_graphs=True)
    for _ in range(4):
        c_rep, b_rep, _ = hot(batch)
    torch.cuda.synchronize()
    assert hot._graph is not None and torch.equal(c_rep, cls_h) and torch.equal(b_rep, bb_h)

    # ---- a few more isolated nodes by hand: the in-edges of six targets removed
    deg = in_degree(g.edge_index, n)
    victims = (deg > 0).nonzero().view(-1)[::31][:6]
    keep = ~torch.isin(g.edge_index[1].cpu(), victims)
    ei, ea, x = g.edge_index[:, keep.cuda()].contiguous(), g.edge_attr[keep.cuda()].contiguous(), g.x
    assert int((in_degree(ei, n) == 0).sum()) >= 9

    # ---- one training step: outputs and parameter gradients against float64 CPU autograd
    rc, rb = torch.randn(n, 6, generator=torch.Generator().manual_seed(1)), torch.randn(n, 5, generator=torch.Generator().manual_seed(2))
    c64, b64, g64 = oracle_run(model, x, ei, ea, conv_type, aggr, rc, rb, torch.float64, True)
    c32, b32, _ = oracle_run(model, x, ei, ea, conv_type, aggr, rc, rb, torch.float32, False)
    train = copy.deepcopy(model)
    xg, eag = x.clone().requires_grad_(True), ea.clone().requires_grad_(True)
    c, bb = train(xg, ei, eag)
    for nm, dev, r64, r32 in (("logits", c, c64, c32), ("boxes", bb, b64, b32)):
        bar = max(1e-5, normwise(r32, r64))
        assert normwise(dev, r64) < bar, (f"{nm} (recorded forward): {normwise(dev, r64):.2e} against float64; bar 1e-5 or the "
                                          f"reference-shaped float32 evaluation's own {normwise(r32, r64):.2e}")
    ((c * rc.cuda()).sum() + (bb * rb.cuda()).sum()).backward()
    largest = max(float(v.abs().max()) for v in g64.values())
    bad = {}
    for name, p in train.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        ref = g64[name]
        err = float((p.grad.detach().double().cpu() - ref).abs().max())
        zero_grad = float(ref.abs().max()) < 1e-9 * largest                  # (the measure of tests/test_gpu_backward.py)
        rel = err / (largest if zero_grad else max(float(ref.abs().max()), 5e-2 * largest))
        if not rel < GTOL:
            bad[name] = rel
    assert not bad, bad

    # ---- inference forward of the same graph: the recorded forward's values, twice the same bits
    with torch.no_grad():
        a1 = copy.deepcopy(model)(x, ei, ea)
        a2 = copy.deepcopy(model)(x, ei, ea)
    assert torch.equal(a1[0], a2[0]) and torch.equal(a1[1], a2[1])
    assert normwise(a1[0], c64) < max(1e-5, normwise(c32, c64)) and normwise(a1[1], b64) < max(1e-5, normwise(b32, b64))
    again = copy.deepcopy(model)
    xg2, eag2 = x.clone().requires_grad_(True), ea.clone().requires_grad_(True)
    c2, bb2 = again(xg2, ei, eag2)
    ((c2 * rc.cuda()).sum() + (bb2 * rb.cuda()).sum()).backward()
    assert torch.equal(c2, c) and torch.equal(bb2, bb)
    for (name, p), (_, q) in zip(train.named_parameters(), again.named_parameters()):
        assert torch.equal(p.grad, q.grad), name

    # ---- per-frame BatchNorm statistics (frame_ptr=) equal one forward per frame
    with torch.no_grad():
        cf, bf = copy.deepcopy(model)(x, ei, ea, frame_ptr=batch.frame_ptr)
        ptr = batch.frame_ptr.cpu().tolist()
        for f in range(len(frames)):
            lo, hi = ptr[f], ptr[f + 1]
            sel = (ei[0] >= lo) & (ei[0] < hi)
            assert bool(((ei[1][sel] >= lo) & (ei[1][sel] < hi)).all())
            c1, b1 = copy.deepcopy(model)(x[lo:hi].contiguous(), (ei[:, sel] - lo).contiguous(), ea[sel].contiguous())
            assert normwise(cf[lo:hi], c1) < 4e-6 and normwise(bf[lo:hi], b1) < 4e-6, (f, normwise(cf[lo:hi], c1), normwise(bf[lo:hi], b1))


@pytest.mark.parametrize("aggr", ax.AGGRS)
def test_conv_layers_alone(aggr):
    """The two layer classes called on their own (``conv(x, edge_index, edge_attr)``), with and without the edge encoder, one and two
    message layers, on a graph with isolated targets: against the restated layers in float64."""
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    from radargnn_amd.gnn.mpnn_layers import MPNNConv, RadarPointGNNConv
    g = torch.Generator().manual_seed(9)
    n, e, c, de = 203, 610, 12, 3
    ei = torch.stack([torch.randint(0, n, (e,), generator=g), torch.randint(0, n - 7, (e,), generator=g)])    # 7 targets without edges
    x, ea = torch.randn(n, c, generator=g), torch.randn(e, de, generator=g)
    layers = [("mpnn", MPNNConv(c, 20, de, aggr=aggr)), ("mpnn_pre2", MPNNConv(c, 20, de, aggr=aggr, pre_layers=2)),
              ("mpnn_enc", MPNNConv(c, 20, de, aggr=aggr, use_edge_encoder=True)), ("radar", RadarPointGNNConv(c, de, aggr=aggr)),
              ("radar_pre2", RadarPointGNNConv(c, de, aggr=aggr, pre_layers=2))]
    for nm, layer in layers:
        sd = {k: v.detach().clone() for k, v in layer.state_dict().items()}
        layer.cuda()
        fn = ax.radar_point_gnn_conv if nm.startswith("radar") else ax.mpnn_conv
        r64 = fn(x.double(), ei, ea.double(), {k: v.double() for k, v in sd.items()}, "", aggr)
        r32 = fn(x, ei, ea, sd, "", aggr)
        with torch.no_grad():
            out = layer(x.cuda(), ei.cuda(), ea.cuda())
            assert torch.equal(out, layer(x.cuda(), ei.cuda(), ea.cuda())), nm
        bar = max(1e-5, normwise(r32, r64))
        assert normwise(out, r64) < bar, (f"{nm} {aggr}: {normwise(out, r64):.2e} against float64; bar 1e-5 or the reference-shaped "
                                          f"float32 evaluation's own {normwise(r32, r64):.2e}")
