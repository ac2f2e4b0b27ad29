"""The backward of the fused aggregation (csrc/backward.hip: rgnn_mpnn_aggregate_bwd, rgnn_mpnn_max_bwd,
rgnn_segment_reduce_bwd) and the forward that records the winners (k_mpnn_max<ARG>, csrc/mpnn.hip) ON their internal thresholds:
hand-built graphs with in-degrees around the 128-edge passes, the 8-edge one-element-per-lane pass, the 32-edge buffer and the
60-edge blocks, out-degrees around the blocks of 64 and trips of 4 of the node half, 1 .. 5 nodes (slots without a segment), slot
counts around k_reduce_slots' strides, 1 .. 4 segments per persistent wave, node counts around the 8192-node grid switch and more
edges than the 2048 x 256 of the d_edge_attr grid -- called through ``ops.mpnn_aggregate_bwd``, ``ops.mpnn_aggregate_max_arg``
and ``ops.segment_reduce_bwd`` directly.  tests/test_gpu_backward_timed_sizes.py compares the same kernels norm-wise on graphs from
the neighbour search, which cannot see one dropped or doubled edge and reaches these places by accident or not at all.

Inputs and reference: tests/mpnn_bwd_cases.py (tests/test_mpnn_bwd_cases.py proves on the CPU that every case is what it says).

Bars.  Integer data: bit-exact (``torch.equal`` with the reference cast to float32) -- every gradient is a sum of integers whose
sum of |terms| stays below 2^24 (proved on the CPU), so nothing is an approximation; the winners are compared index by index with
the first-id reference.  Float data: element-wise against float64, every element scaled by ITS OWN sum of |terms|, within 4 x the
same figure of a plain float32 torch evaluation + 2e-7 (factor and floor of tests/test_gpu_mpnn_win_edges.py and
tests/test_gpu_gnn.py).  Which path ran -- the generic kernels or the lane-local ones -- follows from the dtype of the ``arg_out``
buffer the launch accepts (int32 / int16, ``ops._arg_buffer``): handing in the other one is a TypeError, and that is asserted."""
import functools

import pytest
import torch

import mpnn_bwd_cases as bc
import mpnn_csr_cases as mc

pytestmark = pytest.mark.gpu

SWEEP_CASES = ("in_degrees/nonempty_ends", "out_degrees")
GENERIC_CHANNELS = (1, 3, 4, 5, 252, 256, 260, 508, 512, 516, 768, 772, 1024)
LOCAL_CHANNELS = (8, 16, 248, 256, 264, 504, 512)
SPLIT_CHANNELS = (64, 300, 516)                       # CS = 1, 2 and 4 (nch 3 -> 4: a wave without channels at d = 516)
GENERIC_WIDTHS = (0, 1, 3, 4, 5, 8, 9, 15, 16)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    from radargnn_amd import ops as _ops
    return _ops


def f32(t):
    return None if t is None else t.to(torch.float32).cuda()


class Graph:
    """A case with one ``node_order`` variant on the device."""

    def __init__(self, c, ordered):
        self.c = c
        self.order_cpu = c.node_order if ordered else None
        self.rowptr, self.src = c.rowptr_t.cuda(), c.src_sorted.cuda()
        self.order = None if self.order_cpu is None else self.order_cpu.cuda()
        self.source_csr = tuple(t.cuda() for t in c.source_csr(self.order_cpu))
        self.maps = tuple(t.cuda() for t in c.edge_maps(self.order_cpu))
        self.inv_deg = c.inv_deg(self.order_cpu).cuda()
        self.start = torch.zeros(c.n, dtype=torch.int64)             # CSR position of a NODE's first in-edge
        self.start[torch.from_numpy(c.order_np(self.order_cpu))] = torch.from_numpy(c.rowptr_np[:-1])
        self.has = torch.zeros(c.n, dtype=torch.bool)
        self.has[torch.from_numpy(c.order_np(self.order_cpu))] = torch.from_numpy(c.deg > 0)


@functools.lru_cache(maxsize=None)
def graph(name, ordered):
    return Graph(bc.case(name), ordered)


def local_covers(d, de):
    return d % bc.LOC_D_STEP == 0 and d <= bc.LOC_D_MAX and 1 <= de <= bc.LOC_DE_MAX


@functools.lru_cache(maxsize=None)
def int_reference(name, ordered, layout, negative, d, de, aggr="max"):
    """(inputs, loc, (dQ, dea, dWe) as float32) -- computed once, shared by the generic and the lane-local tests."""
    c = bc.case(name)
    order = c.node_order if ordered else None
    Q, We, ea, dM = bc.int_inputs(c, layout, d=d, de=de, negative=negative)
    loc = bc.first_id(c, Q, We, ea, order)[0] if aggr == "max" else None
    ref, _ = bc.grads(c, dM, We, ea, aggr, order, loc)
    return (Q, We, ea, dM), loc, tuple(None if r is None else r.to(torch.float32) for r in ref)


def backward(ops, g, inputs, aggr, local, arg=None, arg_dtype=None, views=None):
    """-> (dQ, d_edge_attr, dW_e, the winners the launch recomputed as in-segment indices per node, or None).  ``local``: hand in
    the edge maps.  The ``arg_out`` buffer is int16 where the lane-local kernels are expected and int32 otherwise (``arg_dtype``
    overrides): the launch refuses the wrong one."""
    Q, We, ea, dM = inputs
    d, de = Q.shape[1], 0 if ea is None else ea.shape[1]
    Qd, Wd, ed, dMd = (t if t is None or t.is_cuda else f32(t) for t in (Q, We, ea, dM))
    if views:
        Qd, dMd = views(Qd, dMd)
    arg_out = None
    if aggr == "max" and arg is None:
        dtype = arg_dtype or (torch.int16 if (local and local_covers(d, de)) else torch.int32)
        arg_out = torch.full((g.c.n, d), -7, dtype=dtype, device="cuda")
    dQ, dea, dWe = ops.mpnn_aggregate_bwd(dMd, Qd, Wd, ed, g.rowptr, g.src, aggr, g.source_csr, node_order=g.order,
                                          target_scale=g.inv_deg if aggr == "mean" else None, edge_maps=g.maps if local else None,
                                          arg=arg, arg_out=arg_out)
    loc = None
    if arg_out is not None and g.c.n_edges:
        a = arg_out.cpu()
        loc = (a.to(torch.int32) & 0xffff).long() if a.dtype == torch.int16 else a.long() - g.start[:, None]
    return dQ, dea, dWe, loc


def assert_exact(got, ref, what):
    dQ, dea, dWe = got[:3]
    for nm, a, b in (("dQ", dQ, ref[0]), ("d_edge_attr", dea, ref[1]), ("dW_e", dWe, ref[2])):
        if b is None:
            assert a is None, f"{what}: {nm} without edge attributes"
            continue
        a = a.cpu()
        assert a.shape == b.shape, (what, nm, a.shape, b.shape)
        assert torch.equal(a, b), f"{what}: {nm} differs in {int((a != b).sum())} of {a.numel()} elements, first at {(a != b).nonzero()[:3].tolist()}"


def assert_no_edges(got, n, d):
    """E = 0: dQ is [n, d] zeros; an [0, de] attribute tensor counts as no attributes (``ops._mp_common``), so the other two are
    None -- or, should that change, empty and zero."""
    assert got[0].shape == (n, d) and bool((got[0] == 0).all())
    assert got[1] is None or got[1].numel() == 0
    assert got[2] is None or bool((got[2] == 0).all())


def check_max(ops, name, ordered, layout, negative, local, d=None, de=None, recorded=False, arg_dtype=None):
    c = bc.case(name)
    g = graph(name, ordered)
    d = c.d if d is None else d
    de = c.de if de is None else de
    inputs, loc, ref = int_reference(name, ordered, layout, negative, d, de)
    what = f"{name} order={ordered} {layout} negative={negative} d={d} de={de} local={local} ({c.aim})"
    got = backward(ops, g, inputs, "max", local, arg_dtype=arg_dtype)
    if c.n_edges == 0:
        assert_no_edges(got, c.n, d)
        return got
    assert torch.equal(got[3][g.has], loc[g.has]), f"{what}: winners differ on {int((got[3][g.has] != loc[g.has]).sum())} (node, channel) pairs"
    assert_exact(got, ref, what)
    if recorded:
        Q, We, ea, dM = inputs
        chunks = ops.mpnn_partition(g.rowptr, c.n_edges)
        M, arg = ops.mpnn_aggregate_max_arg(None, f32(Q), f32(We), f32(ea), g.rowptr, g.src, node_order=g.order, chunks=chunks)
        expM, has = mc.reference(c, Q, We, ea, None, g.order_cpu, torch.int64)
        assert torch.equal(M.cpu(), expM.to(torch.float32)), what
        if arg is None:                                              # k_mpnn_max records winners for d % 8 == 0, de <= 8 only
            assert d % 8 != 0 or de > 8, what
            return got
        rec = (arg.cpu().to(torch.int32) & 0xffff).long()
        assert torch.equal(rec[g.has], loc[g.has]), f"{what}: recorded winners differ on {int((rec[g.has] != loc[g.has]).sum())} pairs"
        again = backward(ops, g, inputs, "max", local, arg=arg)
        for a, b in zip(again[:3], got[:3]):
            assert torch.equal(a, b), what
    return got


# ------------------------------------------------------------------------------------------------ max: every case
@pytest.mark.parametrize("layout", bc.LAYOUTS)
@pytest.mark.parametrize("name", bc.NAMES)
def test_max_generic_exact(ops, name, layout):
    for ordered in (False, True):
        for negative in (False, True):
            check_max(ops, name, ordered, layout, negative, local=False)


@pytest.mark.parametrize("layout", bc.LAYOUTS)
@pytest.mark.parametrize("name", bc.NAMES)
def test_max_lane_local_exact_with_recomputed_and_recorded_winners(ops, name, layout):
    d = max(bc.case(name).d, bc.LOC_D_STEP)                           # (src_grid: d = 4 is the generic kernels', 8 these)
    assert local_covers(d, bc.case(name).de)
    for ordered in (False, True):
        for negative in (False, True):
            check_max(ops, name, ordered, layout, negative, local=True, d=d, recorded=True)


def test_the_accepted_arg_dtype_tells_the_path(ops):
    """int16 is what the lane-local launch takes and int32 what the generic one takes: the other one is refused before anything runs."""
    for d, de, local, takes in ((16, 3, True, torch.int16), (16, 3, False, torch.int32), (12, 3, True, torch.int32), (520, 3, True, torch.int32),
                                (16, 0, True, torch.int32), (16, 9, True, torch.int32)):
        other = torch.int32 if takes == torch.int16 else torch.int16
        with pytest.raises(TypeError, match="arg_out"):
            check_max(ops, "out_degrees", True, "spread", False, local, d=d, de=de, arg_dtype=other)
        check_max(ops, "out_degrees", True, "spread", False, local, d=d, de=de, arg_dtype=takes)


# ------------------------------------------------------------------------------------------------ sweeps
@pytest.mark.parametrize("d", GENERIC_CHANNELS)
@pytest.mark.parametrize("name", SWEEP_CASES)
def test_generic_across_channel_counts(ops, name, d):
    """Below the largest in-degree (300 / 15) the sources of a target cannot be distinct mod d, so not every edge wins a channel; the
    winners, dQ, d_edge_attr and dW_e are asserted exactly all the same.  d % 4 != 0: the scalar rows."""
    for layout, negative in (("spread", False), ("spread", True), ("all_tie", False), ("last_wins", False)):
        check_max(ops, name, True, layout, negative, local=False, d=d)


@pytest.mark.parametrize("d", LOCAL_CHANNELS + (12, 520))
@pytest.mark.parametrize("name", SWEEP_CASES)
def test_lane_local_across_channel_counts(ops, name, d):
    """d = 12 and d = 520 with the edge maps given fall to the generic kernels (``check_max`` hands in the int32 buffer those take)."""
    for layout, negative in (("spread", False), ("spread", True), ("all_tie", False), ("last_wins", False)):
        check_max(ops, name, True, layout, negative, local=True, d=d, recorded=True)


@pytest.mark.parametrize("de", GENERIC_WIDTHS)
@pytest.mark.parametrize("d", SPLIT_CHANNELS)
@pytest.mark.parametrize("name", SWEEP_CASES)
def test_generic_across_attribute_widths(ops, name, d, de):
    from radargnn_amd import _lib
    assert int(_lib.lib.rgnn_mpnn_bwd_split(d)) == {64: 1, 300: 2, 516: 4}[d]
    for layout, negative in (("spread", False), ("spread", True), ("all_tie", False)) + ((("last_wins", False),) if de else ()):
        check_max(ops, name, True, layout, negative, local=False, d=d, de=de)


@pytest.mark.parametrize("de", range(1, 9))
@pytest.mark.parametrize("name", SWEEP_CASES)
def test_lane_local_across_attribute_widths(ops, name, de):
    for d in (64, 512):
        for layout, negative in (("spread", False), ("spread", True), ("last_wins", False)):
            check_max(ops, name, True, layout, negative, local=True, d=d, de=de, recorded=(d == 512))


@pytest.mark.parametrize("d,de", bc.SLOT_WIDTHS)
@pytest.mark.parametrize("name", bc.SLOT_CASES + bc.TINY_CASES)
def test_slot_partials_across_widths(ops, name, d, de):
    """k_reduce_slots over 4 .. 52 slots and 1, 63, 64, 65 columns of dW_e (at d = 1 two sources cannot differ mod d: exact all the same)."""
    for ordered in (False, True):
        check_max(ops, name, ordered, "spread", False, local=False, d=d, de=de)
        if local_covers(d, de):
            check_max(ops, name, ordered, "spread", False, local=True, d=d, de=de)
    inputs, _, ref = int_reference(name, True, "spread", False, d, de, "add")
    assert_exact(backward(ops, graph(name, True), inputs, "add", False), ref, f"{name} add d={d} de={de}")


# ------------------------------------------------------------------------------------------------ scalar rows
def _strided(t, pad):
    buf = torch.zeros((t.shape[0], t.shape[1] + pad), dtype=torch.float32, device="cuda")
    view = buf[:, :t.shape[1]]
    view.copy_(t)
    return view


def _shifted(t):
    buf = torch.zeros(t.numel() + 4, dtype=torch.float32, device="cuda")
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


VIEWS = {
    "dM_stride": lambda Q, dM: (Q, _strided(dM, 1)),
    "Q_stride": lambda Q, dM: (_strided(Q, 3), dM),
    "both_stride_2": lambda Q, dM: (_strided(Q, 2), _strided(dM, 2)),
    "dM_pointer": lambda Q, dM: (Q, _shifted(dM)),
    "Q_pointer": lambda Q, dM: (_shifted(Q), dM),
}


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("name", SWEEP_CASES + ("multi_edges_and_self_loops",))
def test_unaligned_rows_give_the_bits_of_the_aligned_call(ops, name, view):
    """Rows whose stride is no multiple of 4 floats, or whose first byte is not 16-byte aligned, take the scalar form of the generic
    kernels; with the edge maps given the launch must leave the lane-local kernels (they read 16-byte pieces) for the generic ones,
    which the int32 ``arg_out`` it accepts shows."""
    c = bc.case(name)
    g = graph(name, True)
    for aggr in ("max", "mean", "add"):
        inputs, loc, ref = int_reference(name, True, "spread", False, c.d, c.de, aggr)
        aligned = backward(ops, g, inputs, aggr, False)
        for local in (False, True):
            got = backward(ops, g, inputs, aggr, local, arg_dtype=torch.int32, views=VIEWS[view])
            for a, b in zip(got[:3], aligned[:3]):
                assert torch.equal(a, b), (name, view, aggr, local)
            if aggr == "max":
                assert torch.equal(got[3][g.has], loc[g.has])
        if aggr != "mean":
            assert_exact(aligned, ref, f"{name} {aggr}")
    lane_local = check_max(ops, name, True, "spread", False, local=True)
    for a, b in zip(lane_local[:3], backward(ops, g, int_reference(name, True, "spread", False, c.d, c.de)[0], "max", False)[:3]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ mean and add
@pytest.mark.parametrize("name", bc.NAMES)
def test_add_exact(ops, name):
    c = bc.case(name)
    for ordered in (False, True):
        inputs, _, ref = int_reference(name, ordered, "spread", False, c.d, c.de, "add")
        got = backward(ops, graph(name, ordered), inputs, "add", False)
        if c.n_edges == 0:
            assert_no_edges(got, c.n, c.d)
            continue
        assert_exact(got, ref, f"{name} add order={ordered} ({c.aim})")


@pytest.mark.parametrize("d,de", [(256, 8), (4, 1), (5, 3), (300, 9), (516, 16), (64, 0)])
def test_mean_exact_on_power_of_two_degrees(ops, d, de):
    """1 / deg is exact, every term a multiple of 1 / 256 and every sum of |terms| x 256 below 2^24 (proved on the CPU at the case's
    own width; the other widths only shorten or lengthen the sums over channels: at most 516 x 4 x 2 = 4128)."""
    for ordered in (False, True):
        inputs, _, ref = int_reference("pow2_degrees", ordered, "spread", False, d, de, "mean")
        assert_exact(backward(ops, graph("pow2_degrees", ordered), inputs, "mean", False), ref, f"pow2_degrees mean d={d} de={de} order={ordered}")


def scaled_errors(got, ref64, ref32, sums):
    """max over the elements with a non-zero sum of |terms| of |x - ref64| / sum, for the kernel and for the float32 evaluation;
    elements without terms must be exactly 0."""
    on = sums > 0
    assert bool((got[~on] == 0).all())
    if not bool(on.any()):
        return 0.0, 0.0
    return (float(((got.double() - ref64).abs() / sums)[on].max()), float(((ref32.double() - ref64).abs() / sums)[on].max()))


def check_float(ops, name, aggr, local, label):
    c = bc.case(name)
    g = graph(name, True)
    Q, We, ea, dM = bc.float_inputs(c)
    got = backward(ops, g, (Q, We, ea, dM), aggr, local)
    loc = got[3]
    if aggr == "max":                                                # routed through the kernel's own winners: they must exist
        deg_node = torch.zeros(c.n, dtype=torch.int64)
        deg_node[torch.from_numpy(c.order_np(g.order_cpu))] = torch.from_numpy(c.deg)
        assert bool(((loc >= 0) & (loc < deg_node[:, None]))[g.has].all())
    ref64, sums = bc.grads(c, dM.double(), We.double(), ea.double(), aggr, g.order_cpu, loc, torch.float64)
    ref32, _ = bc.grads(c, dM, We, ea, aggr, g.order_cpu, loc, torch.float32)
    for nm, x, r64, r32, s in zip(("dQ", "d_edge_attr", "dW_e"), got[:3], ref64, ref32, sums):
        e_kernel, e_f32 = scaled_errors(x.cpu(), r64, r32, s)
        print(f"\n[mpnn_bwd_edges] {name} {aggr} {label} {nm}: d={c.d} de={c.de} scaled error kernel {e_kernel:.3e}  float32 torch {e_f32:.3e}  "
              f"bar {4 * e_f32 + 2e-7:.3e}")
        assert e_kernel <= 4 * e_f32 + 2e-7, (name, aggr, nm, e_kernel, e_f32)


@pytest.mark.parametrize("aggr,local", [("mean", False), ("max", False), ("max", True)], ids=["mean", "max_generic", "max_lane_local"])
@pytest.mark.parametrize("name", SWEEP_CASES + ("in_degrees/empty_ends",))
def test_float_data_element_wise(ops, name, aggr, local):
    """Float inputs whose magnitudes run over four decades across the channels.  (Measured figures: MEASUREMENTS.md.)"""
    check_float(ops, name, aggr, local, "lane-local" if local else "generic")


# ------------------------------------------------------------------------------------------------ the bound of dQ
@pytest.mark.parametrize("name", SWEEP_CASES)
def test_bound_of_the_lane_local_dq_is_what_was_stored(ops, name):
    """k_mpnn_bwd_src_max16 raises the bound with the |values| of exactly the four-channel groups it stores, for every node: the bound
    is max |dQ|, not an estimate of it."""
    c = bc.case(name)
    g = graph(name, True)
    Q, We, ea, dM = bc.int_inputs(c, "spread")
    loc, strict = bc.first_id(c, Q, We, ea, g.order_cpu)
    won = strict.nonzero()                                           # (node, channel) pairs with one strict winner
    t, ch = won[len(won) // 2].tolist()
    dM[t, ch] = -20000
    ref, _ = bc.grads(c, dM, We, ea, "max", g.order_cpu, loc)
    assert float(ref[0].abs().max()) >= 10000                        # (the planted value, give or take the few other terms of its sum)
    with ops.bound_tracking("cuda") as pool:
        assert pool is not None
        got = backward(ops, g, (Q, We, ea, dM), "max", True)
        bound = ops.bound_of(got[0])
    assert bound is not None and bound.numel() == ops.BOUND_SLOTS
    assert_exact(got, tuple(r.to(torch.float32) for r in ref), name)
    assert float(bound.max()) == float(got[0].abs().max()) == float(ref[0].abs().max())


# ------------------------------------------------------------------------------------------------ segment_reduce_bwd
@pytest.mark.parametrize("d", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("name", bc.IN_DEGREE_CASES + bc.TINY_CASES + ("pow2_degrees",))
def test_segment_reduce_bwd(ops, name, d):
    """Integer rows in [-3, 3]: exact ties in nearly every segment, the first row wins.  max and add bit-exact; mean bit-exact on the
    power-of-two graph and by the float bar elsewhere (1 / deg is rounded; every element is ONE term, |dM| / deg).  Every row of
    d_rows belongs to a target with in-edges, so every row is defined: none is left out of the comparison."""
    c = bc.case(name)
    rows, dM = bc.row_inputs(c, d)
    for ordered in (False, True):
        g = graph(name, ordered)
        for aggr in ("max", "mean", "add"):
            ref = bc.segment_reduce_grads(c, rows, dM, aggr, g.order_cpu)
            got = ops.segment_reduce_bwd(f32(dM), f32(rows), g.rowptr, aggr, node_order=g.order).cpu()
            assert got.shape == (c.n_edges, d)
            if aggr != "mean" or name == "pow2_degrees":
                assert torch.equal(got, ref.to(torch.float32)), (name, d, aggr, ordered, int((got != ref.to(torch.float32)).sum()))
            else:
                ref32 = bc.segment_reduce_grads(c, rows, dM, aggr, g.order_cpu, torch.float32)
                e_kernel, e_f32 = scaled_errors(got, ref, ref32, ref.abs())
                if d == 65 and ordered:
                    print(f"\n[mpnn_bwd_edges] {name} segment_reduce_bwd mean d={d}: scaled error kernel {e_kernel:.3e}  float32 torch {e_f32:.3e}  "
                          f"bar {4 * e_f32 + 2e-7:.3e}")
                assert e_kernel <= 4 * e_f32 + 2e-7, (name, d, e_kernel, e_f32)


# ------------------------------------------------------------------------------------------------ refusals
def test_shapes_outside_the_contract_are_refused(ops):
    from radargnn_amd._lib import RgnnError
    name = "out_degrees"
    c = bc.case(name)
    g = graph(name, True)
    with pytest.raises(RgnnError, match=r"librgnn error -?\d+: rgnn_mpnn_aggregate_bwd: message width must be <= 1024"):
        backward(ops, g, bc.int_inputs(c, "spread", d=bc.D_MAX + 1), "max", False)
    with pytest.raises(RgnnError, match=r"librgnn error -?\d+: rgnn_mpnn_aggregate_bwd: edge attribute width must be <= 16"):
        backward(ops, g, bc.int_inputs(c, "spread", de=bc.DE_MAX + 1), "max", False)
    with pytest.raises(RgnnError, match=r"edge attribute width must be <= 16"):
        backward(ops, g, bc.int_inputs(c, "spread", de=bc.DE_MAX + 1), "add", True)
    check_max(ops, name, True, "spread", False, local=False)          # (none the worse for the refused launches)
    check_max(ops, name, True, "spread", False, local=True, recorded=True)

