"""tests/mpnn_csr_cases.py checked on the CPU alone: every hand-built CSR is well formed, has the in-degrees it claims, reaches
the line of csrc/mpnn_tiles.hip it is named for (by a Python restatement of the plan's first-fit packing), and comes with integer
inputs on which EVERY edge is the strict unique maximum of at least one output element -- the condition that lets
tests/test_gpu_mpnn_win_edges.py notice a dropped, repeated or mispaired edge.  The three forms of the reference agree."""
from collections import Counter

import numpy as np
import pytest
import torch

import mpnn_csr_cases as mc

# the only edges allowed to win nothing: copies of one (target, source) pair, which exist in this case alone
CASES_WITH_DUPLICATE_EDGES = ("multi_edges_and_self_loops",)


@pytest.mark.parametrize("name", mc.NAMES)
def test_csr_is_well_formed_and_has_the_claimed_in_degrees(name):
    c = mc.case(name)
    rp, src = c.rowptr_t.long(), c.src_sorted.long()
    assert c.rowptr_t.dtype == torch.int32 and c.src_sorted.dtype == torch.int32 and rp.numel() == c.n + 1
    assert int(rp[0]) == 0 and int(rp[-1]) == src.numel() == c.n_edges
    assert bool((rp[1:] >= rp[:-1]).all())
    assert c.n_edges == 0 or (int(src.min()) >= 0 and int(src.max()) < c.n)
    claim = {k: v for k, v in mc.CLAIMED_DEGREES[name].items() if v}
    assert dict(Counter(c.deg.tolist())) == claim
    for order in c.orders()[1:]:
        assert order.dtype == torch.int32 and torch.equal(order.long().sort().values, torch.arange(c.n))
    assert isinstance(c.aim, str) and c.aim
    assert c.d <= mc.D_MAX and c.de <= mc.DE_MAX


@pytest.mark.parametrize("negative", [False, True], ids=["positive", "negative"])
@pytest.mark.parametrize("name", mc.NAMES)
def test_every_edge_wins_a_channel(name, negative):
    c = mc.case(name)
    Q, We, ea, b = mc.int_inputs(c, negative=negative)
    wins = mc.edge_win_counts(c, Q, We, ea, b)
    assert wins.numel() == c.n_edges
    exempt = torch.from_numpy(c.exempt)
    assert bool(exempt.any()) == (name in CASES_WITH_DUPLICATE_EDGES)
    losers = torch.nonzero((wins == 0) & ~exempt).flatten()
    assert losers.numel() == 0, f"{name}: edges {losers[:8].tolist()} are the maximum of no channel"
    # what makes it so: a target's sources are distinct mod d (the duplicates of the multi-edge case apart)
    tgt = np.repeat(np.arange(c.n), c.deg)
    key = (tgt * c.d + c.src_np % c.d)[~c.exempt]
    assert np.unique(key).shape[0] == key.shape[0]
    if negative and c.n_edges:
        out, has = mc.reference(c, Q, We, ea, b, None, torch.int64)
        assert int(out[has].max()) < 0          # a padded slot that held 0 would win everywhere


@pytest.mark.parametrize("name", mc.NAMES)
def test_windows_stay_inside_the_allocation_and_the_slot_geometry(name):
    c = mc.case(name)
    windows, big = mc.first_fit(c.rowptr_np)
    assert len(windows) <= mc.n_win_bound(c.n, c.n_edges)
    deg = c.deg
    assert sorted(big) == np.nonzero(deg > mc.WN_STREAM)[0].tolist()
    placed = 0
    for w in windows:
        fill = [0] * mc.WN_STREAMS
        seg = {p // mc.WN_SEG for p, _, _ in w}
        assert len(seg) == 1
        for p, b, off in w:
            assert off == fill[b] and off % mc.WN_PAD == 0
            fill[b] += int(mc.pad4(deg[p]))
        assert max(fill) <= mc.WN_STREAM and len(w) <= mc.WN_STREAMS * mc.WN_STREAM // mc.WN_PAD
        placed += len(w)
    assert placed + len(big) == int((deg > 0).sum())


def test_the_n_win_bound_is_approached_by_the_patterns_named_for_it():
    """in-degree 33 pads to 36: one target per stream, 288 slots per closed window against the 256 the allocation counts on -- the
    closest a CSR comes to win_layout's bound; in-degree 1 pads fourfold, 512 slots per window."""
    c = mc.case("all_33")
    windows, _ = mc.first_fit(c.rowptr_np)
    assert all(len(w) == mc.WN_STREAMS for w in windows[:-1])
    assert len({p // mc.WN_SEG for w in windows for p, _, _ in w}) == 2           # crosses one segment boundary
    assert len(windows) == 64 + 11 and len(windows) <= mc.n_win_bound(c.n, c.n_edges) == 88
    for n in mc.ALL_1_SIZES:
        c = mc.case(f"all_1/{n}")
        windows, _ = mc.first_fit(c.rowptr_np)
        assert len(windows) == sum(-(-min(mc.WN_SEG, n - s) // 128) for s in range(0, n, mc.WN_SEG))
        assert len(windows) <= mc.n_win_bound(c.n, c.n_edges)
    assert len(mc.first_fit(mc.case(f"all_1/{mc.ALL_1_SIZES[-1]}").rowptr_np)[0]) > mc.WN_TICKET_BLOCKS


def test_distinct_sources_of_the_windows_in_question():
    for name, rows, targets, left in (("distinct_176", 176, 44, 0), ("distinct_177", 177, 45, 45), ("hash_chain", 176, 44, 0)):
        c = mc.case(name)
        windows, big = mc.first_fit(c.rowptr_np)
        w = mc.window_of(windows, c.focus)
        assert len(w) == targets and mc.window_sources(c, w).shape[0] == rows
        assert not big and mc.per_target_expected(c)[0] == left
        # ordinary windows before and after
        i = windows.index(w)
        assert 0 < i < len(windows) - 1
        assert all(mc.window_sources(c, v).shape[0] <= mc.WN_UMAX for v in windows if v is not w)
    c = mc.case("hash_chain")
    w = mc.window_of(mc.first_fit(c.rowptr_np)[0], c.focus)
    assert np.unique(mc.hash_bucket(mc.window_sources(c, w))).shape[0] == 1
    c = mc.case("one_source")
    windows, _ = mc.first_fit(c.rowptr_np)
    assert [mc.window_sources(c, w).shape[0] for w in windows[1:3]] == [1, 9] and len(windows) == 4
    assert all(len(w) == 128 for w in windows)


def test_cases_reach_the_thresholds_they_name():
    assert mc.case("many_segments").n > mc.WN_SCAN_THREADS * mc.WN_SEG            # per = 2 in k_win_segbase
    assert len(mc.first_fit(mc.case("many_segments").rowptr_np)[0]) == 1026       # one window in every segment
    deg = set(mc.case("stream_edge").deg.tolist())
    assert {mc.WN_STREAM - 4, mc.WN_STREAM - 3, mc.WN_STREAM - 1, mc.WN_STREAM, mc.WN_STREAM + 1, mc.WN_STREAM + 4, mc.WN_STREAM + 5} <= deg
    deg = set(mc.case("leftover_blocks").deg.tolist())
    assert {mc.LEFT_BLOCK + 1, mc.LEFT_BLOCK + mc.LEFT_REQ - 1, mc.LEFT_BLOCK + mc.LEFT_REQ, mc.LEFT_BLOCK + mc.LEFT_REQ + 1,
            2 * mc.LEFT_BLOCK - 1, 2 * mc.LEFT_BLOCK, 2 * mc.LEFT_BLOCK + 1, 1000} <= deg
    c = mc.case("multi_edges_and_self_loops")
    tgt = np.repeat(np.arange(c.n), c.deg)
    assert int((tgt == c.src_np).sum()) >= 4 and int(c.exempt.sum()) == 3 + 2 + 2
    c = mc.case("empty_graph_parts/empty_full_one")
    assert int(c.deg[:mc.WN_SEG].sum()) == 0 and int((c.deg[mc.WN_SEG:2 * mc.WN_SEG] > 0).sum()) == mc.WN_SEG and c.n % mc.WN_SEG == 1
    assert mc.case("empty_graph_parts/no_edges").n_edges == 0


@pytest.mark.parametrize("name", ["degrees_1_to_8/empty_ends", "stream_edge", "leftover_blocks", "multi_edges_and_self_loops",
                                  "empty_graph_parts/empty_full_one", "empty_graph_parts/no_edges"])
def test_reference_forms_agree_on_integer_data(name):
    c = mc.case(name)
    for negative in (False, True):
        Q, We, ea, b = mc.int_inputs(c, negative=negative)
        for order in c.orders():
            i64, has = mc.reference(c, Q, We, ea, b, order, torch.int64)
            f64, has64 = mc.reference(c, Q, We, ea, b, order, torch.float64)
            f32, has32 = mc.reference(c, Q, We, ea, b, order, torch.float32)
            assert torch.equal(has, has64) and torch.equal(has, has32)
            assert f64.dtype == torch.float64 and f32.dtype == torch.float32
            assert torch.equal(i64.double(), f64) and torch.equal(i64.float(), f32)
            assert int(i64.abs().max()) < 2 ** 24 and bool((i64[~has] == 0).all())
            node = torch.arange(c.n) if order is None else order.long()
            assert torch.equal(has[node], torch.from_numpy(c.deg > 0))


def test_reference_against_a_loop_over_targets():
    c = mc.case("stream_edge")
    Q, We, ea, b = mc.int_inputs(c)
    out, has = mc.reference(c, Q, We, ea, b, c.node_order, torch.int64)
    for p in range(c.n):
        lo, hi = int(c.rowptr_np[p]), int(c.rowptr_np[p + 1])
        node = int(c.node_order[p])
        if hi == lo:
            assert not bool(has[node])
            continue
        msg = Q[torch.from_numpy(c.src_np[lo:hi])] + ea[lo:hi] @ We.t()
        assert torch.equal(out[node], msg.max(0).values + b)
