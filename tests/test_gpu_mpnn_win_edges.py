"""The window form of the max aggregation (k_mpnn_win, k_win_leftover) and the five kernels of its plan (csrc/mpnn_tiles.hip) ON
their internal thresholds: hand-built CSRs-by-target that the project's neighbour search would never produce -- in-degrees around
the 4-slot pad, the 64-slot stream and the per-target kernel's blocks of 64 / requests of 8, windows of exactly 176 and 177
distinct source rows, 176 sources in one bucket of the plan's hash table, more than 1024 segments, more windows than work-groups,
empty segments -- called through ``ops.mpnn_win_plan`` / ``ops.mpnn_aggregate_win`` directly.  tests/test_gpu_mpnn_tiles.py
compares the same kernels norm-wise on graphs from the graph builder, which reach these places by accident or not at all.

Inputs and reference: tests/mpnn_csr_cases.py (tests/test_mpnn_csr_cases.py proves on the CPU that every case reaches the line it
names and that every edge is the strict unique maximum of at least one output element).

Bars.  Integer data: bit-exact (``torch.equal`` with the int64 reference cast to float32) -- the three-term bf16 split is exact on
small integers and every sum stays below 2^24, so nothing here is an approximation; both kernels, both ``node_order`` variants, both
``skip_empty_rows`` values, all-positive and all-negative messages.  Float data: element-wise against float64, every element scaled by
S[t, c] = max_e(|Q| + sum_k |w||z|) + |b|, within 4 x the same figure of a plain float32 torch evaluation + 2e-7 (factor and floor of
tests/test_gpu_gnn.py's "not a weaker path").  Which kernel took which target is read out of the plan, not inferred."""
import ctypes as C

import pytest
import torch

import mpnn_csr_cases as mc

pytestmark = pytest.mark.gpu

BOTH_KERNELS = ("stream_edge", "leftover_blocks")               # cases with targets on either side of the 64-slot stream
SWEEP_CASES = ("degrees_1_to_8/nonempty_ends",) + BOTH_KERNELS
CHANNELS = (1, 31, 32, 33, 64, 100, 512, 513, 2048)             # one tile = 32, one per-target pass = 512, the documented limit = 2048


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    from radargnn_amd import ops as _ops
    return _ops


def f32(t):
    return None if t is None else t.to(torch.float32).cuda()


class Graph:
    """A case on the device: CSR, one ``node_order`` variant, its plan."""

    def __init__(self, ops, c, order):
        self.c, self.order_cpu = c, order
        self.rowptr, self.src = c.rowptr_t.cuda(), c.src_sorted.cuda()
        self.order = None if order is None else order.cuda()
        self.ops = ops
        self.plan = self.new_plan()

    def new_plan(self):
        return self.ops.mpnn_win_plan(self.rowptr, self.src, self.order)

    def counters(self, plan=None):
        """(targets on the per-target list, windows made), read out of the plan."""
        from radargnn_amd import _lib
        lw, ww = C.c_int64(), C.c_int64()
        _lib.lib.rgnn_mpnn_win_plan_counters(self.c.n, self.c.n_edges, C.byref(lw), C.byref(ww))
        plan = self.plan if plan is None else plan
        return int(plan[lw.value]), int(plan[ww.value])

    def padded(self, Q):
        out = self.ops.padded_rows(Q.shape[0], Q.shape[1], "cuda")
        out.copy_(Q.to(torch.float32))
        return out

    def win(self, Q, We, ea, b, skip=False, plan=None):
        return self.ops.mpnn_aggregate_win(b, Q, We, ea, self.rowptr, self.src, self.plan if plan is None else plan,
                                           node_order=self.order, skip_empty_rows=skip)

    def per_edge(self, Q, We, ea, b):
        chunks = self.ops.mpnn_partition(self.rowptr, self.c.n_edges)
        return self.ops.mpnn_aggregate(None, b, Q, We, ea, self.rowptr, self.src, "max", node_order=self.order, chunks=chunks)


def check_exact(g, inputs, both_skips=True, per_edge=True, replans=False):
    """Window kernel (+ per-target kernel) == int64 reference on every row with edges, 0 on the others; the per-edge kernel gives the
    same bits.  -> the output (skip_empty_rows = False)."""
    c = g.c
    Q, We, ea, b = inputs
    exp, has = mc.reference(c, Q, We, ea, b, g.order_cpu, torch.int64)
    exp, has = exp.to(torch.float32).cuda(), has.cuda()
    Qd, Wd, ed, bd = g.padded(Q), f32(We), f32(ea), f32(b)
    out = g.win(Qd, Wd, ed, bd, skip=False)
    assert out.shape == exp.shape
    assert torch.equal(out[has], exp[has]), f"{c.name}: {int((out[has] != exp[has]).any(1).sum())} rows differ ({c.aim})"
    assert bool((out[~has] == 0).all())
    if both_skips:
        skipped = g.win(Qd, Wd, ed, bd, skip=True)
        assert torch.equal(skipped[has], exp[has])
    if replans:
        again = g.win(Qd, Wd, ed, bd, skip=False)                    # (the ticket counters were left at zero)
        assert torch.equal(again, out)
        plan2 = g.new_plan()                                         # (the hash order of the distinct sources does not reach the results)
        assert g.counters(plan2) == g.counters()
        assert torch.equal(g.win(Qd, Wd, ed, bd, skip=False, plan=plan2), out)
    if per_edge and c.n_edges:
        ref = g.per_edge(Qd, Wd, ed, bd)
        assert torch.equal(ref, out)
    return out


# ------------------------------------------------------------------------------------------------ exact on integers
@pytest.mark.parametrize("name", [n for n in mc.NAMES if n != "many_segments"])
def test_exact_on_integers(ops, name):
    c = mc.case(name)
    for order in c.orders():
        g = Graph(ops, c, order)
        left, made = g.counters()
        assert (left, made) == mc.per_target_expected(c), c.aim
        for negative in (False, True):
            check_exact(g, mc.int_inputs(c, negative=negative), replans=not negative)


def test_many_segments_exact(ops):
    """n = 1025 * 512 + 7: k_win_segbase scans two segments per thread; every segment holds one window."""
    c = mc.case("many_segments")
    g = Graph(ops, c, c.node_order)
    left, made = g.counters()
    assert left == 0 and made == 1026, (left, made)
    check_exact(g, mc.int_inputs(c), both_skips=False)


@pytest.mark.parametrize("name", SWEEP_CASES)
@pytest.mark.parametrize("d", CHANNELS)
def test_exact_across_channel_counts(ops, name, d):
    c = mc.case(name)
    g = Graph(ops, c, c.node_order)
    for negative in (False, True):
        check_exact(g, mc.int_inputs(c, d=d, negative=negative), both_skips=False)


@pytest.mark.parametrize("name", SWEEP_CASES)
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("de", [0, 1, 3, 8])
def test_exact_across_attribute_widths(ops, name, de, with_bias):
    c = mc.case(name)
    g = Graph(ops, c, c.node_order)
    for negative in (False, True):
        check_exact(g, mc.int_inputs(c, de=de, with_bias=with_bias, negative=negative), both_skips=False)


# ------------------------------------------------------------------------------------------------ which path ran
def test_which_kernel_took_which_target(ops):
    for name in BOTH_KERNELS + ("distinct_176", "distinct_177"):
        c = mc.case(name)
        exp_left, exp_made = mc.per_target_expected(c)
        for order in c.orders():
            left, made = Graph(ops, c, order).counters()
            msg = f"{name}: {left} targets per target, {made} windows made (restated plan: {exp_left}, {exp_made})"
            if name in BOTH_KERNELS:
                assert left == int((c.deg > mc.WN_STREAM).sum()) > 0, msg
            elif name == "distinct_176":
                assert left == 0, msg                                # 176 distinct rows: the window stays
            else:
                assert left == 45, msg                               # 177: exactly its 45 targets go


# ------------------------------------------------------------------------------------------------ vector / scalar attribute reads
@pytest.mark.parametrize("name", SWEEP_CASES + ("multi_edges_and_self_loops",))
def test_misaligned_attributes_give_the_bits_of_the_aligned_call(ops, name):
    """de = 8: rows of 32 bytes read as two float4 per half-wave when the pointer is 16-byte aligned (p.ea_vec), scalar otherwise."""
    c = mc.case(name)
    g = Graph(ops, c, c.node_order)
    Q, We, ea, b = mc.int_inputs(c, de=8)
    aligned = check_exact(g, (Q, We, ea, b), both_skips=False, per_edge=False)
    buf = torch.zeros(c.n_edges * 8 + 4, dtype=torch.float32, device="cuda")
    view = buf[1:1 + c.n_edges * 8].view(c.n_edges, 8)
    view.copy_(ea.to(torch.float32))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    assert f32(ea).data_ptr() % 16 == 0
    got = g.win(g.padded(Q), f32(We), view, f32(b))
    assert torch.equal(got, aligned)


# ------------------------------------------------------------------------------------------------ float data, element-wise
def scaled_error(got, ref64, S, has):
    return float(((got.double() - ref64).abs() / S)[has].max())


@pytest.mark.parametrize("name", SWEEP_CASES)
def test_float_data_element_wise(ops, name):
    """Inputs whose magnitudes run over four decades across the channels; every element against float64, scaled by ITS OWN S[t, c],
    so a row of small values counts as much as the largest.  Yardstick: the same figure of a float32 torch evaluation.
    (Measured figures: MEASUREMENTS.md, window-kernel section.)"""
    c = mc.case(name)
    g = Graph(ops, c, c.node_order)
    Q, We, ea, b = mc.float_inputs(c)
    ref64, has = mc.reference(c, Q.double(), We.double(), ea.double(), b.double(), g.order_cpu, torch.float64)
    ref32, _ = mc.reference(c, Q, We, ea, b, g.order_cpu, torch.float32)
    S, _ = mc.error_scale(c, Q, We, ea, b, g.order_cpu)
    assert float(S[has].min()) > 0
    out = g.win(g.padded(Q), f32(We), f32(ea), f32(b)).cpu()
    e_kernel, e_f32 = scaled_error(out, ref64, S, has), scaled_error(ref32, ref64, S, has)
    left, made = g.counters()
    print(f"\n[mpnn_win_edges] {name}: d={c.d} de={c.de} scaled error kernel {e_kernel:.3e}  float32 torch {e_f32:.3e}  "
          f"bar {4 * e_f32 + 2e-7:.3e}  ({left} targets per target, {made} windows)")
    assert e_kernel <= 4 * e_f32 + 2e-7, (e_kernel, e_f32)
    assert bool((out[~has] == 0).all())


# ------------------------------------------------------------------------------------------------ the bound for the next layer
@pytest.mark.parametrize("where", ["window_row", "per_target_row"])
def test_bound_covers_what_was_stored(ops, where):
    """``out_absmax`` feeds the f16 pre-scale of the next dense layer: too low a bound overflows without a word.  The largest |value|
    is planted once in a row the window kernel writes and once in a row of the per-target kernel.

    What the code implies: k_win_leftover tracks exactly what it stores.  k_mpnn_win<true> does not -- at every group in which EITHER
    half-wave ends a segment both halves contribute |running maximum + bias|, so partial maxima of unfinished segments and the filler
    slots behind a stream's last target (row 0 of the window with edge 0's attributes) enter.  No factor follows from that, only:
    max |out| <= bound <= max_c(max_s |Q[s, c]| + sum_k |W[c, k]| max_e |a[e, k]| + |b[c]|).  Both sides are asserted."""
    c = mc.case("stream_edge")
    g = Graph(ops, c, c.node_order)
    assert 0 < g.counters()[0] < int((c.deg > 0).sum())             # both kernels write rows of this graph
    Q, We, ea, b = mc.int_inputs(c, de=8)
    want = 60 if where == "window_row" else 65
    p = int((c.deg == want).nonzero()[0][1])
    e = int(c.rowptr_np[p + 1]) - 1
    assert e != 0
    ea[e] = 0
    ea[e, 0] = 20000
    We[0, 0] = 2
    exp, has = mc.reference(c, Q, We, ea, b, g.order_cpu, torch.int64)
    node = int(c.node_order[p])
    assert int(exp.abs().max(1).values.argmax()) == node and int(exp.abs().max()) >= 40000 - 1100
    with ops.bound_tracking("cuda") as pool:
        assert pool is not None
        out = g.win(g.padded(Q), f32(We), f32(ea), f32(b))
        bound = ops.bound_of(out)
    assert bound is not None and bound.numel() == ops.BOUND_SLOTS
    assert torch.equal(out[has.cuda()], exp.to(torch.float32).cuda()[has.cuda()])
    stored = float(out[has.cuda()].abs().max())
    limit = float((Q.abs().max(0).values + (We.abs() * ea.abs().max(0).values[None, :]).sum(1) + b.abs()).max())
    assert stored <= float(bound.max()) <= limit, (stored, float(bound.max()), limit)


# ------------------------------------------------------------------------------------------------ refusals
def test_shapes_outside_the_contract_are_refused(ops):
    from radargnn_amd._lib import RgnnError
    c = mc.case("degrees_1_to_8/nonempty_ends")
    g = Graph(ops, c, c.node_order)
    unsupported = r"librgnn error -3"                               # RGNN_ERR_UNSUPPORTED
    Q, We, ea, b = mc.int_inputs(c, d=mc.D_MAX + 1)
    with pytest.raises(RgnnError, match=unsupported):
        g.win(g.padded(Q), f32(We), f32(ea), f32(b))
    Q, We, ea, b = mc.int_inputs(c, de=mc.DE_MAX + 1)
    with pytest.raises(RgnnError, match=unsupported):
        g.win(g.padded(Q), f32(We), f32(ea), f32(b))
    Q, We, ea, b = mc.int_inputs(c, d=33)
    narrow = torch.zeros((c.n, 34), dtype=torch.float32, device="cuda")[:, :33]     # rows 136 bytes apart: not 16-byte aligned
    narrow.copy_(Q.to(torch.float32))
    assert narrow.stride(0) % 4 != 0
    with pytest.raises(RgnnError, match=unsupported):
        g.win(narrow, f32(We), f32(ea), f32(b))
    check_exact(g, mc.int_inputs(c), both_skips=False, per_edge=False)     # (the plan is none the worse for the refused launches)
