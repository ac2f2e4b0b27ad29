"""The SEGMENT ENDS of the window kernel (k_mpnn_win, csrc/mpnn_tiles.hip): where a target's slots end, every lane fetches the
target row's store offset from its half-wave's lane with one lane permute, stores under the full exec mask and relies on the
buffer's range check to drop the half that does not end there and the columns beyond d; the running maximum is reset where the
permuted offset is a real one.  The cases put ends where that can go wrong -- in one half only, in both, in neither; at the first and
the last group of a stream; behind a segment that crosses a 16-slot tile; in streams of different lengths; at targets 0 and n - 1 (the
smallest and the largest store offset) -- on hand-built CSRs whose layout in the window is restated (mpnn_csr_cases.first_fit) and
asserted, with both instances of the kernel (with and without the bound of the next layer).

Bars.  Integer data, every sum exact (tests/mpnn_csr_cases.py): ``torch.equal`` with the int64 reference.  ``out`` is allocated HERE
and filled with a value no result can take before the launch: rows of targets without edges and the padding columns of every row
must still hold it (a store that should have been dropped), rows with edges must not (one that was dropped and should not have been).
The bound: max |out| <= bound <= the a-priori limit everywhere; EQUAL to max |out| over the columns < d where the construction
makes every partial maximum and every filler slot a value some target stores (all messages positive, one attribute row for every
edge), with the padding columns of Q filled with values far above it."""
import functools

import numpy as np
import pytest
import torch

import mpnn_csr_cases as mc

pytestmark = pytest.mark.gpu

CHANNELS = (32, 33, 80, 464)        # a whole channel tile, one column past it, a partial last tile, the production width
SENTINEL = 7.5                      # no sum of integers
GPT = 16 // mc.WN_PAD               # groups per 16-slot tile


def _zeros_between(head, tail, n=96):
    """in-degrees: ``head``, then targets without edges up to n positions, then ``tail`` -- positions 0 and n - 1 have edges"""
    return list(head) + [0] * (n - len(head) - len(tail)) + list(tail)


# name -> (in-degrees, {stream: groups that end a segment}, what it is about).  One window each (checked): the plan packs the targets
# with edges first-fit in order, so a run of targets that fills a stream's 64 slots exactly is followed by the next stream.
CASES = {
    # stream 0: padded 4, 12, 4, 44 -> ends at groups 0, 3, 4, 15; stream 1: padded 8, 8, 4, 20, 24 -> 1, 3, 4, 9, 15
    "halves": (_zeros_between([3, 10, 1, 41, 8, 5], [4, 17, 22]), {0: {0, 3, 4, 15}, 1: {1, 3, 4, 9, 15}},
               "group 0: first half only; group 1: second half only; group 2: neither; groups 3, 4, 15: both; group 9: second only"),
    # stream 0: 4, 20, 4, 36; stream 1: 36, 4, 4, 20
    "tile_crossing": (_zeros_between([1, 17, 1, 33, 34], [1, 1, 20]), {0: {0, 5, 6, 15}, 1: {8, 9, 10, 15}},
                      "padded degrees 20 and 36 cross a 16-slot tile, next to targets of in-degree 1"),
    # stream 0: 36 (three tiles, 28 slots free); 32 + 32 do not fit it -> stream 1: four tiles
    "unequal_streams": (_zeros_between([36, 30], [32]), {0: {8}, 1: {7, 15}}, "a wave whose first stream holds three tiles and whose second four"),
    "short_second": (_zeros_between([16, 13, 16, 15, 2], [3]), {0: {3, 7, 11, 15}, 1: {0, 1}}, "four tiles beside one"),
    "empty_stream": (_zeros_between([5], [2]), {0: {1, 2}}, "stream 1 of wave 0 is empty, and so are the streams of waves 1 .. 3"),
    "one_target": ([0] * 40 + [7] + [0] * 55, {0: {1}}, "a window of one target"),
}


@functools.lru_cache(maxsize=None)
def built(name):
    if name == "random_r1m":
        rng = np.random.Generator(np.random.PCG64(41))
        c = mc.Case(name, rng.integers(1, 13, size=560), 64, "in-degrees 1 .. 12 at random: three of four groups end a segment", seed=3)
        assert c.n_edges <= 4000
    elif name == "knn20":
        c = mc.Case(name, [20] * 100, 64, "in-degree 20 throughout: one group in five ends a segment", seed=4)
    else:
        deg, ends, aim = CASES[name]
        c = mc.Case(name, deg, 64, aim, seed=1)
        windows, big = mc.first_fit(c.rowptr_np)
        assert len(windows) == 1 and not big, name
        pd = mc.pad4(c.deg)
        got = {}
        for p, stream, first in windows[0]:
            got.setdefault(stream, set()).add((first + int(pd[p]) - 1) // mc.WN_PAD)
        assert got == ends, (name, got)
        assert c.deg[0] > 0 or name == "one_target"
    assert c.n <= 600 and c.n_edges <= 4000
    return c


ALL = tuple(CASES) + ("random_r1m", "knn20")


@functools.lru_cache(maxsize=None)
def expected(name, d, positive, identity):
    c = built(name)
    Q, We, ea, b = mc.int_inputs(c, d=d)
    if positive:                                                     # every message in (0, 3000): see the module docstring
        Q = Q + 1200
        ea = ea[:1].abs().expand(c.n_edges, -1).contiguous() if c.n_edges else ea
    order = None if identity else c.node_order
    exp, has = mc.reference(c, Q, We, ea, b, order, torch.int64)
    return (Q, We, ea, b), exp.to(torch.float32), has


class Launch:
    """One launch of the window kernel through ``ops.mpnn_aggregate_win`` into an ``out`` allocated here (the function asks
    ``ops.padded_rows`` for it) and filled with SENTINEL, rows with the production stride."""

    def __init__(self, ops, monkeypatch, name, d, bound, positive=False, identity=False, q_padding=None):
        c = built(name)
        (Q, We, ea, b), self.exp, self.has = expected(name, d, positive, identity)
        order = None if identity else c.node_order.cuda()
        rowptr, src = c.rowptr_t.cuda(), c.src_sorted.cuda()
        plan = ops.mpnn_win_plan(rowptr, src, order)
        Qd = ops.padded_rows(c.n, d, "cuda")
        if q_padding is not None and Qd.stride(0) > d:
            torch.as_strided(Qd, (c.n, Qd.stride(0)), (Qd.stride(0), 1)).fill_(q_padding)
        Qd.copy_(Q.to(torch.float32))
        real = ops.padded_rows
        made = []

        def prefilled(m, n, device):
            t = real(m, n, device)
            whole = torch.as_strided(t, (m, t.stride(0)), (t.stride(0), 1)) if m > 1 else t
            whole.fill_(SENTINEL)
            made.append(whole)
            return t

        monkeypatch.setattr(ops, "padded_rows", prefilled)
        f32 = lambda t: None if t is None else t.to(torch.float32).cuda()
        args = (f32(b), Qd, f32(We), f32(ea), rowptr, src, plan)
        if bound:
            with ops.bound_tracking("cuda") as pool:
                assert pool is not None
                self.out = ops.mpnn_aggregate_win(*args, node_order=order, skip_empty_rows=True)
                word = ops.bound_of(self.out)
            assert word is not None
            self.bound = float(word.max())
        else:
            self.out = ops.mpnn_aggregate_win(*args, node_order=order, skip_empty_rows=True)
            assert ops.bound_of(self.out) is None
            self.bound = None
        monkeypatch.setattr(ops, "padded_rows", real)
        assert len(made) == 1
        self.whole, self.d, self.c = made[0].cpu(), d, c
        self.inputs = (Q, We, ea, b)

    def check_rows(self):
        out, d, has = self.whole[:, :self.d], self.d, self.has
        bad = (out[has] != self.exp[has]).any(1)
        assert not bool(bad.any()), f"{self.c.name} d={d}: {int(bad.sum())} of {int(has.sum())} rows differ ({self.c.aim})"
        assert bool((out[~has] == SENTINEL).all()), f"{self.c.name} d={d}: a row of a target without edges was written"
        assert bool((self.whole[:, d:] == SENTINEL).all()), f"{self.c.name} d={d}: a padding column was written"

    def limit(self):
        Q, We, ea, b = self.inputs
        return float((Q.abs().max(0).values + (We.abs() * ea.abs().max(0).values[None, :]).sum(1) + b.abs()).max())


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    from radargnn_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("bound", [False, True], ids=["plain", "bound"])
@pytest.mark.parametrize("d", CHANNELS)
@pytest.mark.parametrize("name", ALL)
def test_ends_store_the_right_rows_and_nothing_else(ops, monkeypatch, name, d, bound):
    """Every row with edges holds the exact maximum, everything else in ``out`` what it held before the launch."""
    run = Launch(ops, monkeypatch, name, d, bound)
    run.check_rows()
    if bound:
        stored = float(run.exp[run.has].abs().max())
        assert stored <= run.bound <= run.limit(), (stored, run.bound, run.limit())


@pytest.mark.parametrize("bound", [False, True], ids=["plain", "bound"])
@pytest.mark.parametrize("d", CHANNELS)
@pytest.mark.parametrize("name", ["halves", "random_r1m"])
def test_targets_0_and_n_minus_1(ops, monkeypatch, name, d, bound):
    """Without a node order position = node: nodes 0 and n - 1 have edges, so offset 0 and the largest offset of ``out`` are stored to
    (neither may be taken for the offset of a group that ends nothing), and the row behind the last one does not exist."""
    c = built(name)
    assert c.deg[0] > 0 and c.deg[-1] > 0
    run = Launch(ops, monkeypatch, name, d, bound, identity=True)
    assert bool(run.has[0]) and bool(run.has[c.n - 1])
    run.check_rows()


@pytest.mark.parametrize("d", CHANNELS)
@pytest.mark.parametrize("name", ["halves", "unequal_streams", "empty_stream", "random_r1m", "knn20"])
def test_bound_is_the_maximum_over_the_columns_below_d(ops, monkeypatch, name, d):
    """All messages positive and one attribute row for every edge: each partial maximum and each filler slot is at most a value that
    some target stores, so the bound must EQUAL max |out| over the columns < d -- with 2^20 in the padding columns of Q, which the
    lanes beyond d of the last channel tile read and must keep out of it."""
    run = Launch(ops, monkeypatch, name, d, True, positive=True, q_padding=float(2 ** 20))
    run.check_rows()
    assert float(run.exp[run.has].min()) > 0
    stored = float(run.exp[run.has].abs().max())
    assert stored < 4000
    assert run.bound == stored, (run.bound, stored)
