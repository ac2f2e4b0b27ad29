"""ops.linear_pair / rgnn_linear_fwd_pair: two independent row-subset dense launches handed over together -- a conv layer's source
term beside its isolated-row update -- run as ONE grid (k_linear_dma_pair) where the library is built for their tile widths.
Every case runs the pair and then the same two launches one after the other ON THE SAME BUFFERS and wants the same bits:
the output rows, the rows neither list names (untouched: they keep the sentinel), both statistics panel sets and the 256 slot
words of both outputs' bounds.  Nothing here is compared against arithmetic of its own: the separate launches are pinned by
tests/test_gpu_dense_fwd_edges.py and tests/test_gpu_gnn.py.

RGNN_DMA_NO_SMALL_M=1 throughout: the planner then picks the column-tile widths of the benchmark's row counts (464 -> 160,
272 -> 96, 224 -> 224, 128 -> 128, 64 -> 64 columns) at the few rows a test can afford -- the widths the pair kernels exist for."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
SIZES = (0, 1, 255, 256, 257)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    from radargnn_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def production_tile_widths(ops, monkeypatch):
    monkeypatch.delenv("RGNN_NO_LINEAR_PAIR", raising=False)
    monkeypatch.setenv("RGNN_DMA_NO_SMALL_M", "1")
    ops.reload_env()                                  # (undone after the test: monkeypatch, then conftest's autouse reload)


class Buffers:
    """x [rows, k] read by both launches; A: out_a = x[list_a] W_a^T (the source term: no bias, row stride padded as the layer
    pads it); B: out_b = x[list_b] W_b^T + b_b with column statistics (the isolated-row update)."""

    def __init__(self, ops, rows, k, n_a, n_b, seed=0):
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *shape: torch.rand(*shape, generator=g)
        self.ops, self.rows, self.k = ops, rows, k
        self.x = (rnd(rows, k) * 4 - 2).cuda()
        self.x_bound = ops.make_bound(torch.tensor(2.0, device="cuda"))
        self.w_a, self.w_b = ((rnd(n_a, k) - 0.5) * 0.2).cuda(), ((rnd(n_b, k) - 0.5) * 0.2).cuda()
        self.b_b = (rnd(n_b) - 0.5).cuda()
        # BatchNorm-apply table {mean, g, t}: |relu((x - mean) g + t)| <= (2 + 0.5) 1.5 + 0.5 < 8
        self.table = torch.stack([rnd(k) - 0.5, rnd(k) + 0.5, rnd(k) - 0.5]).cuda()
        self.table_bound = ops.make_bound(torch.tensor(8.0, device="cuda"))
        self.out_a = ops.padded_rows(rows, n_a, "cuda")
        self.out_b = torch.empty((rows, n_b), dtype=torch.float32, device="cuda")
        self.stats_b = torch.empty((ops.stat_panels(rows) + 1, ops.STAT_ROWS, n_b), dtype=torch.float32, device="cuda")
        self.perm = torch.from_numpy(np.random.default_rng(seed).permutation(rows).astype(np.int32))

    def lists(self, count_a, count_b):
        """Disjoint lists (ascending, as the layers' are) in buffers as long as the matrices have rows -- the wrapper bounds the
        matrix rows by the list's length -- with the counts on the device."""
        assert count_a + count_b <= self.rows
        out = []
        for ids in (self.perm[:count_a], self.perm[self.rows - count_b:] if count_b else self.perm[:0]):
            buf = torch.zeros(self.rows, dtype=torch.int32)
            buf[:ids.numel()] = ids.sort().values
            out += [buf.cuda(), torch.tensor([ids.numel()], dtype=torch.int64, device="cuda"), ids.long()]
        return out

    def calls(self, count_a, count_b, affine):
        la, ca, ids_a, lb, cb, ids_b = self.lists(count_a, count_b)
        aff = dict(a1_affine=self.table) if affine else {}
        first = dict(a1=self.x, w1=self.w_a, out=self.out_a, row_index=la, m_dev=ca, **aff)
        second = dict(a1=self.x, w1=self.w_b, bias1=self.b_b, out=self.out_b, row_index=lb, m_dev=cb, stats_out=self.stats_b, **aff)
        return first, second, ids_a, ids_b

    def reset(self):
        for t in (self.out_a, self.out_b, self.stats_b):
            t.fill_(SENTINEL)


def run(ops, B, first, second, together, fused=None, tables=()):
    """One pass over the buffers inside a fresh bound pool -> everything the two launches leave behind."""
    B.reset()
    with ops.bound_tracking("cuda"):
        ops.set_bound(B.x, B.x_bound)
        for t in (B.table,) + tuple(tables):
            ops.set_bound(t, B.table_bound)
        f16 = ops.COUNTERS.get("f16x2", 0)
        if together:
            assert ops.linear_pair_fuses(first, second) == fused
            before = ops.COUNTERS.get("linear_pair", 0)
            ops.linear_pair(first, second)
            assert ops.COUNTERS.get("linear_pair", 0) - before == (1 if fused else 0)
        else:
            ops.linear(**second)
            ops.linear(**first)
        assert ops.COUNTERS.get("f16x2", 0) - f16 == (4 if together else 2)          # (the query prepares both once more)
        words = [ops.bound_of(first["out"]), ops.bound_of(second["out"])]
        assert words[0] is not None and words[1] is not None and words[0].data_ptr() != words[1].data_ptr()
    torch.cuda.synchronize()
    return {"out_a": B.out_a.clone(), "out_b": B.out_b.clone(), "stats_b": B.stats_b.clone(),
            "bound_a": words[0].clone(), "bound_b": words[1].clone()}


def check(ops, B, first, second, ids_a, ids_b, fused, tables=()):
    pair = run(ops, B, first, second, True, fused, tables)
    apart = run(ops, B, first, second, False, tables=tables)
    for name in pair:
        assert torch.equal(pair[name], apart[name]), \
            f"{name}: {int((pair[name] != apart[name]).sum())} of {pair[name].numel()} words differ between one grid and two launches"
    for out, ids, nm in ((pair["out_a"], ids_a, "first"), (pair["out_b"], ids_b, "second")):
        named = torch.zeros(B.rows, dtype=torch.bool)
        named[ids] = True
        named = named.cuda()
        assert bool((out[~named] == SENTINEL).all()), f"{nm}: a row its list does not name was written"
        assert bool((out[named] != SENTINEL).all()), f"{nm}: a row of its list was not written"
    print(f"bounds {float(pair['bound_a'].max()):.4f} {float(pair['bound_b'].max()):.4f}; "
          f"slots raised {int((pair['bound_a'] > 0).sum())} {int((pair['bound_b'] > 0).sum())}")
    return pair


@pytest.fixture(scope="module")
def layer2(ops):
    return Buffers(ops, 1024, 224, 464, 224, seed=1)


@pytest.mark.parametrize("count_b", SIZES)
@pytest.mark.parametrize("count_a", SIZES)
def test_row_lists_of_every_size(ops, layer2, count_a, count_b):
    """Empty lists, one row, one row short of a 256-row panel, a whole panel, one row more: for each part, counts read from m_dev."""
    first, second, ids_a, ids_b = layer2.calls(count_a, count_b, affine=True)
    check(ops, layer2, first, second, ids_a, ids_b, fused=True)


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "bn_apply_relu"])
@pytest.mark.parametrize("k", [128, 224])
@pytest.mark.parametrize("n_a,n_b", [(464, 224), (464, 128), (272, 64)])
def test_every_built_pair_of_widths(ops, n_a, n_b, k, affine):
    """The three pairs of tile widths the conv layers produce, with and without the BatchNorm-apply table (+ ReLU) on x; column
    statistics on the second part only, as in the layer.  700 + 300 of 1 024 rows: several panels, ragged last ones."""
    B = Buffers(ops, 1024, k, n_a, n_b, seed=n_b + k)
    first, second, ids_a, ids_b = B.calls(700, 300, affine)
    check(ops, B, first, second, ids_a, ids_b, fused=True)


def test_second_part_queues_behind_a_full_device(ops):
    """22 016 rows at N = 464 are 86 panels x 3 column tiles = 258 tiles: the first part takes 256 work-groups, one per compute
    unit, and the second part's work-groups can only start as those retire."""
    B = Buffers(ops, 22016 + 300, 224, 464, 224, seed=5)
    first, second, ids_a, ids_b = B.calls(22016, 300, affine=True)
    check(ops, B, first, second, ids_a, ids_b, fused=True)


def test_unbuilt_width_pair_takes_two_launches(ops):
    """N = 96 for the second part is a 96-column tile: no (160, 96) pair is built."""
    B = Buffers(ops, 1024, 224, 464, 96, seed=6)
    first, second, ids_a, ids_b = B.calls(700, 300, affine=True)
    check(ops, B, first, second, ids_a, ids_b, fused=False)


def test_per_segment_tables_take_two_launches(ops):
    """The first part on a segment-padded list with one BatchNorm-apply table per segment (two tables resident per work-group,
    -1 entries in the list): not a pair the one-grid kernel takes."""
    B = Buffers(ops, 1024, 224, 464, 224, seed=7)
    first, second, ids_a, ids_b = B.calls(600, 300, affine=True)
    seg_ptr = torch.tensor([0, 400, 1024], dtype=torch.int64, device="cuda")
    padded, total, tiles, _ = ops.pad_list_by_segment(first["row_index"][:600].contiguous(), first["m_dev"], seg_ptr)
    tables = torch.stack([B.table, B.table.flip(1)]).contiguous()
    first.update(row_index=padded, m_dev=total, a1_affine=tables, a1_affine_tiles=tiles, padded_row_list=True)
    check(ops, B, first, second, ids_a, ids_b, fused=False, tables=(tables,))


def test_conv_layer_with_and_without_the_pair(ops, monkeypatch):
    """MPNNConv.forward_sorted (folded inference form) on a 2-frame radius graph: RGNN_NO_LINEAR_PAIR set and unset give the same
    h and the same statistics panels, and the pair really ran as one grid when it was allowed to."""
    from radargnn_amd import frames as fr, synthetic
    from radargnn_amd.gnn.mpnn_layers import MPNNConv, TargetCSR
    batch = fr.FrameBatch.from_frames([synthetic.radarscenes_frame(i) for i in range(2)])
    g = fr.build_graphs(batch, fr.GraphSettings(algorithm="radius", k=0, r=1.0))
    n, e = g.x.shape[0], g.edge_index.shape[1]
    torch.manual_seed(8)
    conv = MPNNConv(224, 224, 16).cuda().eval()
    x, ea = torch.randn(n, 224, device="cuda"), torch.randn(e, 16, device="cuda")
    x_bound = ops.make_bound(x.abs().max())

    def forward(no_pair):
        if no_pair:
            monkeypatch.setenv("RGNN_NO_LINEAR_PAIR", "1")
        else:
            monkeypatch.delenv("RGNN_NO_LINEAR_PAIR", raising=False)
        ops.reload_env()
        csr = TargetCSR(g.edge_index, n, order=g.cell_order, symmetric=True)
        before = ops.COUNTERS.get("linear_pair", 0)
        with torch.no_grad(), ops.bound_tracking("cuda"):
            ops.set_bound(x, x_bound)
            h, stats = conv.forward_sorted(x, csr, csr.sort_edge_attr(ea), want_stats=True)
            word = ops.bound_of(h).clone()
        torch.cuda.synchronize()
        parts = []
        for st, count in stats.parts:
            rows = int(count.item())
            assert rows > 0                                           # (the graph has targets with edges and isolated ones)
            parts.append(st[:ops.stat_panels(rows)].clone())
        return h, parts, word, ops.COUNTERS.get("linear_pair", 0) - before

    h1, parts1, word1, fused1 = forward(no_pair=False)
    h0, parts0, word0, fused0 = forward(no_pair=True)
    assert (fused1, fused0) == (1, 0)
    assert torch.equal(h1, h0) and torch.equal(word1, word0)
    assert all(torch.equal(a, b) for a, b in zip(parts1, parts0))
