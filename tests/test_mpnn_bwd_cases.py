"""tests/mpnn_bwd_cases.py checked on the CPU alone: every hand-built graph is well formed and has the in- and out-degrees it
claims, its CSR by source and its edge maps describe the edge set of its CSR by target, the vectorised reference equals a per-edge
Python loop and float64 autograd of the forward formula, every sum the kernels have to reproduce bit for bit stays below 2^24, and
the three winner layouts put the winners where they say -- the conditions that let tests/test_gpu_mpnn_bwd_edges.py notice a
dropped, doubled or misrouted gradient."""
from collections import Counter

import numpy as np
import pytest
import torch

import mpnn_bwd_cases as bc
import mpnn_csr_cases as mc

SMALL = [n for n in bc.NAMES if bc.case(n).n_edges <= 1000 and bc.case(n).n_edges * bc.case(n).d <= 40000]
INTEGER_VARIANTS = [(layout, negative) for layout in bc.LAYOUTS for negative in (False, True)]


def _max(t):
    return float(t.max()) if t.numel() else 0.0


def test_constants_match_the_sources():
    """The restated thresholds are the ones in the kernels' text."""
    import os
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "radargnn_amd", "csrc")
    bwd = open(os.path.join(root, "backward.hip")).read()
    fwd = open(os.path.join(root, "mpnn.hip")).read()
    for text, needle in ((bwd, f"constexpr int CAP = {bc.CAP};"), (bwd, f"constexpr int BUF = {bc.BUF};"), (fwd, f"constexpr int BLK = {bc.BLK};"),
                         (bwd, "if (cnt * DEP <= 64)"), (bwd, f"jb += {bc.SRC_BLOCK})"), (bwd, f"i += {bc.SRC_TRIP})"),
                         (bwd, f"n < {bc.SLOTS_MAX} ? n : {bc.SLOTS_MAX}"), (bwd, f"n < {bc.SRC_GRID_N} ? (n + 3) / 4 : {bc.SRC_GRID_BLOCKS}"),
                         (bwd, f"(n_edges + {bc.DEA_BLOCK - 1}) / {bc.DEA_BLOCK}"), (bwd, "blocks > 256 * 8"),
                         (bwd, f"s + 16 < slots; s += {bc.REDUCE_STRIDE}"), (bwd, f"d <= {bc.D_MAX}"), (bwd, f"de <= {bc.DE_MAX}"),
                         (bwd, f"d % {bc.LOC_D_STEP} == 0 && d <= {bc.LOC_D_MAX} && de > 0 && de <= {bc.LOC_DE_MAX}")):
        assert needle in text, needle
    assert bc.DEA_BLOCKS == 256 * 8 and bc.SMALL_PASS * 8 == 64


@pytest.mark.parametrize("name", bc.NAMES)
def test_graph_is_well_formed_and_has_the_claimed_degrees(name):
    c = bc.case(name)
    rp, src = c.rowptr_t.long(), c.src_sorted.long()
    assert c.rowptr_t.dtype == torch.int32 and c.src_sorted.dtype == torch.int32 and rp.numel() == c.n + 1
    assert int(rp[0]) == 0 and int(rp[-1]) == src.numel() == c.n_edges
    assert bool((rp[1:] >= rp[:-1]).all())
    assert c.n_edges == 0 or (int(src.min()) >= 0 and int(src.max()) < c.n)
    got = dict(Counter(c.deg.tolist()))
    if name == "pow2_degrees":
        assert set(got) == {0, *bc.POW2}
    else:
        assert got == {k: v for k, v in bc.CLAIMED_IN_DEGREES[name].items() if v}
    out = dict(Counter(c.out_deg().tolist()))
    assert sum(k * v for k, v in out.items()) == c.n_edges
    if name in bc.CLAIMED_OUT_DEGREES:
        assert out == bc.CLAIMED_OUT_DEGREES[name]
    assert int(c.deg.max(initial=0)) <= 65535
    assert isinstance(c.aim, str) and c.aim and c.d <= bc.D_MAX and c.de <= bc.LOC_DE_MAX
    assert c.node_order.dtype == torch.int32 and torch.equal(c.node_order.long().sort().values, torch.arange(c.n))


def test_the_cases_reach_the_lines_they_name():
    deg = np.concatenate([bc.case(n).deg for n in bc.IN_DEGREE_CASES])
    for k in (bc.SMALL_PASS, bc.SMALL_PASS + 1, bc.BUF - 1, bc.BUF, bc.BUF + 1, bc.BLK - 1, bc.BLK, bc.BLK + 1, 2 * bc.BLK - 1, 2 * bc.BLK, 2 * bc.BLK + 1,
              bc.CAP - 1, bc.CAP, bc.CAP + 1, bc.CAP + bc.SMALL_PASS, bc.CAP + bc.SMALL_PASS + 1, 2 * bc.CAP - 1, 2 * bc.CAP, 2 * bc.CAP + 1, 5 * bc.BLK):
        assert k in deg, k
    for ends, name in ((False, bc.IN_DEGREE_CASES[0]), (True, bc.IN_DEGREE_CASES[1])):
        d = bc.case(name).deg
        assert (d[0] == 0) == ends and (d[-1] == 0) == ends
    out = bc.case("out_degrees").out_deg()
    for k in (0, 1, bc.SRC_TRIP - 1, bc.SRC_TRIP, bc.SRC_TRIP + 1, bc.SRC_BLOCK - 1, bc.SRC_BLOCK, bc.SRC_BLOCK + 1, bc.SRC_BLOCK + bc.SRC_TRIP,
              2 * bc.SRC_BLOCK - 1, 2 * bc.SRC_BLOCK, 2 * bc.SRC_BLOCK + 1, 2 * bc.SRC_BLOCK + 2):
        assert k in out, k
    assert int(bc.case("out_degrees").deg.max()) <= 16
    assert [bc.case(n).n for n in bc.TINY_CASES] == [1, 2, 3, 4, 5]
    assert all(-(-s // 4) * 4 != s for s in (1, 2, 3, 5))                      # slots without a segment
    assert {s % bc.REDUCE_STRIDE for s in (-(-n // 4) * 4 for n in bc.SLOT_SIZES)} >= {16, 20, 0, 4}
    assert sorted(d * de for d, de in bc.SLOT_WIDTHS) == [1, bc.REDUCE_COLS - 1, bc.REDUCE_COLS, bc.REDUCE_COLS + 1]
    assert [-(-n // bc.SLOTS_MAX) for n in bc.SEGMENT_SIZES] == [1, 1, 2, 3, 4]
    assert bc.SRC_GRID_SIZES == (bc.SRC_GRID_N - 1, bc.SRC_GRID_N, bc.SRC_GRID_N + 1)
    big = bc.case("dea_grid_stride")
    assert bc.DEA_BLOCK * bc.DEA_BLOCKS < big.n_edges < bc.DEA_BLOCK * bc.DEA_BLOCKS + 1024
    for n in bc.SEGMENT_SIZES:                                                 # a buffer that is flushed inside a segment and carried across
        d = bc.case(f"many_segments_per_wave/{n}").deg
        assert int(d.max()) > bc.BUF and int((d == 0).sum()) > 0


@pytest.mark.parametrize("name", bc.NAMES)
def test_source_csr_and_edge_maps_describe_the_same_edges(name):
    c = bc.case(name)
    for order in c.orders():
        nodes = c.order_np(order)
        rowptr_s, tnode, tpos = (t.numpy().astype(np.int64) for t in c.source_csr(order))
        tgt_sorted, eloc_sorted, tloc = (t.numpy().astype(np.int64) for t in c.edge_maps(order))
        assert rowptr_s.shape == (c.n + 1,) and rowptr_s[0] == 0 and rowptr_s[-1] == c.n_edges
        assert np.array_equal(np.sort(tpos), np.arange(c.n_edges))             # a permutation
        assert np.array_equal(tloc, eloc_sorted[tpos])
        # the edge set by target: (source node, target node) of every sorted edge; by source: the same pairs, found through tpos
        by_target = np.stack((c.src_np, nodes[np.repeat(np.arange(c.n), c.deg)]), 1)
        src_of_out_edge = nodes[np.repeat(np.arange(c.n), np.diff(rowptr_s))]
        assert np.array_equal(np.stack((src_of_out_edge, tnode), 1), by_target[tpos])
        assert np.array_equal(tgt_sorted, by_target[:, 1])
        assert np.array_equal(np.diff(rowptr_s), c.out_deg()[nodes])           # laid out in visiting order
        # eloc: 0 .. deg - 1 inside every segment
        for p in np.nonzero(c.deg)[0][:50]:
            assert np.array_equal(eloc_sorted[c.rowptr_np[p]:c.rowptr_np[p + 1]], np.arange(c.deg[p]))


@pytest.mark.parametrize("layout,negative", INTEGER_VARIANTS)
@pytest.mark.parametrize("name", SMALL)
def test_reference_equals_a_per_edge_loop(name, layout, negative):
    c = bc.case(name)
    Q, We, ea, dM = bc.int_inputs(c, layout, negative=negative)
    for order in c.orders():
        loc, _ = bc.first_id(c, Q, We, ea, order)
        for aggr in ("max", "mean", "add"):
            dQ, dea, dWe, loc_n, scale = bc.naive_grads(c, Q, We, ea, dM, aggr, order)
            (rQ, rea, rWe), _ = bc.grads(c, dM, We, ea, aggr, order, loc)
            if aggr == "max":
                assert np.array_equal(loc.numpy(), loc_n)
            for got, ref in ((dQ, rQ), (dea, rea), (dWe, rWe)):
                assert np.array_equal(got.astype(np.float64), (ref * scale).round().numpy())
                assert _max(((ref * scale) - (ref * scale).round()).abs()) < 1e-6


def test_the_small_set_covers_every_kind_of_small_case():
    assert set(bc.TINY_CASES) <= set(SMALL) and "slots/13" in SMALL and "multi_edges_and_self_loops" in SMALL and "no_edges" in SMALL


@pytest.mark.parametrize("layout", bc.LAYOUTS)
@pytest.mark.parametrize("name", [n for n in bc.NAMES if n != "dea_grid_stride"])
def test_reference_equals_float64_autograd_where_the_winner_is_strict(name, layout):
    c = bc.case(name)
    if c.n_edges == 0:
        return
    Q, We, ea, dM = bc.int_inputs(c, layout)
    order = c.node_order
    loc, strict = bc.first_id(c, Q, We, ea, order)
    node = torch.from_numpy(c.tgt_node(order))
    Qd, Wd, ad = (t.double().requires_grad_(True) for t in (Q, We, ea))
    msg = Qd[torch.from_numpy(c.src_np)] + ad @ Wd.t()
    msg.retain_grad()
    # (base far below every message: autograd counts a base element EQUAL to the maximum as one of the tied, include_self or not)
    M = torch.full((c.n, c.d), -1e30, dtype=torch.float64).scatter_reduce(0, node[:, None].expand(-1, c.d), msg, "amax", include_self=False)
    ref, has = mc.reference(c, Q, We, ea, None, order, torch.float64)
    assert torch.equal(M[has], ref[has])
    M.backward(dM.double())
    G = bc.edge_gradient(c, dM, "max", order, loc)
    on = strict[node]                                                          # (autograd shares a tied maximum out evenly)
    assert torch.equal(msg.grad[on], G[on])
    # ... and the rest of the chain is linear: autograd of the messages under the reference's per-edge gradient
    Qd.grad = Wd.grad = ad.grad = None
    (Qd[torch.from_numpy(c.src_np)] + ad @ Wd.t()).backward(G)
    (rQ, rea, rWe), _ = bc.grads(c, dM, We, ea, "max", order, loc)
    assert torch.equal(Qd.grad, rQ) and torch.equal(ad.grad, rea) and torch.equal(Wd.grad, rWe)


@pytest.mark.parametrize("name", bc.NAMES)
def test_every_sum_stays_exact_in_float32(name):
    """sum of |terms| < 2^24 for every output of every integer case (mean on the power-of-two graph: times the largest in-degree,
    every term being a multiple of its reciprocal): bit-exactness is derived, not hoped for."""
    c = bc.case(name)
    for layout, negative in INTEGER_VARIANTS:
        Q, We, ea, dM = bc.int_inputs(c, layout, negative=negative)
        loc, _ = bc.first_id(c, Q, We, ea, None)
        for aggr in ("max", "add") + (("mean",) if name == "pow2_degrees" else ()):
            if aggr != "max" and (layout != "spread" or negative):
                continue
            _, sums = bc.grads(c, dM, We, ea, aggr, None, loc)
            factor = int(c.deg.max(initial=1)) if aggr == "mean" else 1
            for s in sums:
                assert s is None or _max(s) * factor < bc.EXACT_LIMIT, (name, layout, aggr, _max(s))
        fwd = mc.error_scale(c, Q, We, ea, None)[0]
        assert _max(fwd) < bc.EXACT_LIMIT


@pytest.mark.parametrize("negative", [False, True], ids=["positive", "negative"])
@pytest.mark.parametrize("name", bc.NAMES)
def test_spread_every_edge_wins_a_channel(name, negative):
    c = bc.case(name)
    Q, We, ea, dM = bc.int_inputs(c, "spread", negative=negative)
    assert bool((dM != 0).all()) and int(dM.abs().max()) <= 4
    if name in bc.SPREAD_EXEMPT:
        assert c.spread_exempt
        return
    assert not c.spread_exempt
    wins = mc.edge_win_counts(c, Q, We, ea)
    exempt = torch.from_numpy(c.exempt)
    assert bool(exempt.any()) == (name == "multi_edges_and_self_loops")
    losers = torch.nonzero((wins == 0) & ~exempt).flatten()
    assert losers.numel() == 0, f"{name}: edges {losers[:8].tolist()} are the maximum of no channel"
    if negative and c.n_edges:
        out, has = mc.reference(c, Q, We, ea, None, None, torch.int64)
        assert int(out[has].max()) < 0


@pytest.mark.parametrize("negative", [False, True], ids=["positive", "negative"])
@pytest.mark.parametrize("name", bc.NAMES)
def test_all_tie_and_last_wins_put_the_winner_where_they_claim(name, negative):
    c = bc.case(name)
    has = torch.from_numpy(c.deg > 0)
    last = torch.from_numpy(c.deg - 1)[:, None].expand(-1, c.d)
    Q, We, ea, _ = bc.int_inputs(c, "all_tie", negative=negative)
    loc, strict = bc.first_id(c, Q, We, ea, None)
    assert bool((loc[has] == 0).all()) and bool((loc[~has] == -1).all())
    assert bool((strict[has] == (last[has] == 0)).all())                       # every edge of a segment ties on every channel
    if c.n_edges:
        assert bool((We != 0).any()) and (c.de == 1 or bool((ea != 0).any()))
    Q, We, ea, _ = bc.int_inputs(c, "last_wins", negative=negative)
    loc, strict = bc.first_id(c, Q, We, ea, None)
    assert bool((loc[has] == last[has]).all()) and bool(strict[has].all())
    if negative and c.n_edges:
        assert int(mc.reference(c, Q, We, ea, None, None, torch.int64)[0][has].max()) < 0
    for de in (1, bc.DE_MAX):                                                  # the margin of LAST_A holds at every attribute width
        Q, We, ea, _ = bc.int_inputs(c, "last_wins", de=de, negative=negative)
        loc, strict = bc.first_id(c, Q, We, ea, None)
        assert bool((loc[has] == last[has]).all()) and bool(strict[has].all())


def test_ties_sit_across_pass_block_and_buffer_borders():
    """all_tie on in_degrees: the winner is index 0 while later passes (128), blocks (60) and buffers (32) hold equal values;
    last_wins: the winner is the last index of segments that end 1 past, on, and 1 before each border."""
    deg = bc.case(bc.IN_DEGREE_CASES[0]).deg
    for border in (bc.BUF, bc.BLK, bc.SRC_BLOCK, bc.CAP, 2 * bc.CAP):
        assert {border - 1, border, border + 1} <= set(deg.tolist())
