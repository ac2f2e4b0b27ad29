"""The neighbour search (csrc/graph.hip) ON its internal thresholds: radius ties (d2 == r2), row lengths around the fill pass's
cache / LDS / team limits, grid geometry that runs the coarsening loop or a degenerate branch, exactly translated clouds at
RadarScenes-like global coordinates, every dispatch edge of the kNN entry point, ties at the k-th place under every kNN kernel,
a short frame inside a batch, the frame-size thresholds of the grid build and the split fill.  tests/test_gpu_graph.py compares
the same kernels with the same oracle on random clouds, which hit these places by accident or not at all.

Inputs: tests/graph_edge_inputs.py (tests/test_graph_edge_inputs.py proves on the CPU that each one hits its edge).
Reference: oracle/graph_oracle.py (float64, the KD-tree's arithmetic; kNN rows distance ascending, index ascending).

Bar, everywhere: bit-exact.  ``edge_index.t()`` equals the oracle's edge list entry for entry, ``rowptr[-1]`` its length,
``undirected_degree`` the oracle's; a second kernel path equals the first with ``torch.equal``; ``relative_position`` equals the
float32 cast of the float64 difference.  No tolerances: nothing here is a floating-point approximation.  No coordinate is NaN/Inf."""
import functools

import numpy as np
import pytest
import torch

import graph_edge_inputs as gi
from oracle import graph_oracle as go
from radargnn_amd import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    from radargnn_amd import ops as _ops
    return _ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def batch(frames, basis="X"):
    cat, ptr = synthetic.concat_frames(frames)
    Xb = np.ascontiguousarray(np.concatenate([gi.basis(f, basis) for f in frames], axis=0))
    assert np.isfinite(Xb).all() and np.array_equal(Xb[:, :2], cat.X)
    return Xb, ptr


def oracle_batch_edges(frames, routine, k=None, r=None, basis="X"):
    out, off = [], 0
    for f in frames:
        E = go.build_edges(gi.basis(f, basis), routine, k=k, r=r)
        if E is not None and E.shape[0]:
            out.append(E.astype(np.int64) + off)
        off += f.n
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def oracle_batch_degree(frames, exp):
    off, deg = 0, []
    for f in frames:
        Ef = exp[(exp[:, 0] >= off) & (exp[:, 0] < off + f.n)] - off
        deg.append(go.undirected_degree(Ef, f.n))
        off += f.n
    return np.concatenate(deg)


def rel_expected(Xb, ei, undirected=False):
    e = ei.cpu().numpy()
    d = Xb[e[0]][:, :2] - Xb[e[1]][:, :2]
    return (np.abs(d) if undirected else d).astype(np.float32)


def set_env(ops, monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, str(value))
    ops.reload_env()                                   # (undone after the test: monkeypatch, then conftest's autouse reload)


# ================================================================================================ radius search
def check_radius(ops, frames, r, basis="X", exp=None):
    """ops.radius_graph and count -> fill(relative_position) with the frame size given and with 0, against the oracle.
    -> dict of the device results (of the count / fill path at the given frame size)."""
    Xb, ptr = batch(frames, basis)
    n = Xb.shape[0]
    if exp is None:
        exp = oracle_batch_edges(frames, "radius", r=r, basis=basis)
    X, P = dev(Xb), dev(ptr)
    rowptr, col, ei = ops.radius_graph(X, P, r)
    assert np.array_equal(ei.t().cpu().numpy(), exp)
    assert rowptr[-1].item() == exp.shape[0]
    assert np.array_equal(col.cpu().numpy(), exp[:, 1])
    deg = ops.undirected_degree(rowptr, col, n).cpu().numpy()
    assert np.array_equal(deg, oracle_batch_degree(frames, exp))
    biggest = max(f.n for f in frames)
    keep = None
    for mfp, mode in ((biggest, "directed"), (0, "directed"), (0, "undirected")):
        g, rp = ops.radius_graph_count(X, P, r, max_frame_points=mfp)
        assert torch.equal(rp, rowptr)
        n_edges = int(rp[-1].item())
        c2, e2, rel = ops.radius_graph_fill(g, rp, r, n_edges, relative_position=mode)
        assert torch.equal(c2, col) and torch.equal(e2, ei), (mfp, mode)
        assert np.array_equal(rel.cpu().numpy(), rel_expected(Xb, ei, mode == "undirected")), (mfp, mode)
        if keep is None:
            keep = dict(X=X, P=P, Xb=Xb, rowptr=rp.clone(), col=c2, ei=e2, rel=rel, biggest=biggest, n_edges=n_edges, exp=exp)
    return keep


def tie_batch(spacing, offset=(0.0, 0.0)):
    return [synthetic.nuscenes_frame(5), gi.lattice(24, spacing, offset=offset), synthetic.small_frame(40, 5, duplicates=2),
            synthetic.radarscenes_frame(3, n_clusters=10, pts_per_cluster=20, n_clutter=100)]


@pytest.mark.parametrize("basis", ["X", "XV", "X8"])
@pytest.mark.parametrize("spacing,r,offset", [(0.5, 1.0, (0.0, 0.0)), (0.5, 1.0, (2.0 ** 23, 2.0 ** 23)), (0.1, 0.3, (0.0, 0.0))])
def test_radius_ties_at_the_bound(ops, spacing, r, offset, basis):
    """Item 1: d2 == r2 exactly for thousands of pairs (0.5 lattice, also moved by 2^23), exact ties and misses by a few ulp
    (0.1 lattice, r = 0.3), inside a ragged batch, bases of 2, 4 and 8 columns: the inclusive bound of k_radius / k_radius_rows."""
    frames = tie_batch(spacing, offset)
    out = check_radius(ops, frames, r, basis)
    lo = frames[0].n
    lat = (out["exp"][:, 0] >= lo) & (out["exp"][:, 0] < lo + frames[1].n)
    if basis == "X":
        assert int(lat.sum()) == (6436 if spacing == 0.5 else go.radius_edges(frames[1].X, r).shape[0])
    assert gi.tie_counts(gi.basis(frames[1], basis), r)[0] > 0


def test_radius_row_lengths_at_every_threshold(ops):
    """Item 2: star frames whose hub rows hold exactly 15 ... 513 neighbours (16 lanes x 3 slots, RADIUS_CACHE = 48,
    ROWS_LDS_DIRECT = 128, ROWS_LDS = 512) beside spoke rows of assorted lengths and a clutter frame; count / fill against the
    oracle, then the one-launch search-and-fill at the committed rows against count / fill."""
    frames, hubs = gi.star_batch()
    r = gi.STAR_R
    exp = oracle_batch_edges(frames, "radius", r=r)
    n = sum(f.n for f in frames)
    odeg = np.bincount(exp[:, 0], minlength=n)
    for d, h in hubs.items():
        assert odeg[h] == d
    assert {1, 2, 3} <= set((odeg % 4).tolist())
    out = check_radius(ops, frames, r, exp=exp)
    assert np.array_equal(np.diff(out["rowptr"].cpu().numpy()), odeg)
    X, P, biggest = out["X"], out["P"], out["biggest"]
    for mfp in (biggest, 0):
        static = {}
        g, rowptr = ops.radius_graph_count(X, P, r, static=static, max_frame_points=mfp)
        rows = rowptr.clone()
        for mode in ("directed", "undirected"):
            status = torch.zeros(1, dtype=torch.int32, device=X.device)
            g2 = ops.radius_grid(X, P, r, static, max_frame_points=mfp)
            col2, ei2, rel2 = ops.radius_graph_rows_direct(g2, rows, r, out["n_edges"], status, relative_position=mode)
            torch.cuda.synchronize()
            assert int(status.item()) == 0
            assert torch.equal(col2, out["col"]) and torch.equal(ei2, out["ei"])
            assert np.array_equal(rel2.cpu().numpy(), rel_expected(out["Xb"], out["ei"], mode == "undirected"))
            if mode == "directed":
                assert torch.equal(rel2, out["rel"])


def test_rows_direct_writes_nothing_under_another_edge_total(ops):
    """rgnn_radius_graph_rows_direct with committed rows whose total E is not the n_edges the buffers were sized for (E - 1 and
    E + 1): STATUS_EDGE_COUNT_CHANGED, and not one element of col / edge_index / relative_position written -- what the guarded
    k_radius_rows does.  The star batch: its hub rows of 129 and 513 neighbours take the LDS stage and the global scratch.  Then
    n_edges = E on the same buffers: a clean status and ops.radius_graph_fill's outputs, so the guard refuses nothing it should
    accept.  The C entry point is called directly, because the ops wrapper sizes the buffers from n_edges: here they hold
    max(E, n_edges) edges, so no kernel, guarded or not, writes outside an allocation."""
    import ctypes as C
    from radargnn_amd import _lib
    frames, _ = gi.star_batch()
    r = gi.STAR_R
    Xb, ptr = batch(frames)
    X, P = dev(Xb), dev(ptr)
    static = {}
    g, rowptr = ops.radius_graph_count(X, P, r, static=static)
    rows = rowptr.clone()
    E = int(rows[-1].item())
    assert E > 513
    cap, sentinel = E + 1, -7
    col = torch.full((cap,), sentinel, dtype=torch.int32, device=X.device)
    ei = torch.full((2 * cap,), sentinel, dtype=torch.int64, device=X.device)
    rel = torch.full((cap, 2), float(sentinel), dtype=torch.float32, device=X.device)
    tmp = torch.full((cap,), sentinel, dtype=torch.int32, device=X.device)
    status = torch.zeros(1, dtype=torch.int32, device=X.device)

    def run(n_edges):
        status.zero_()
        _lib.check(_lib.lib.rgnn_radius_graph_rows_direct(C.byref(g.desc), float(r), ops._ptr(rows), ops._ptr(col), ops._ptr(ei), n_edges,
                                                          ops._ptr(tmp), ops._ptr(status), ops._ptr(rel), 0, ops._stream()))
        torch.cuda.synchronize()
        return int(status.item())

    for n_edges in (E - 1, E + 1):
        assert run(n_edges) & ops.STATUS_EDGE_COUNT_CHANGED, n_edges
        assert bool((col == sentinel).all()) and bool((ei == sentinel).all()) and bool((rel == float(sentinel)).all()), n_edges
    assert run(E) == 0
    col0, ei0, rel0 = ops.radius_graph_fill(g, rows, r, E, relative_position="directed")
    assert torch.equal(col[:E], col0) and torch.equal(ei[:2 * E].view(2, E), ei0) and torch.equal(rel[:E], rel0)


def geometry_batch():
    fr = gi.geometry_frames()
    order = ["clusters", "single", "line_h", "empty", "line_v", "coincident", "pair_at_r", "pair_beyond_r", "negative"]
    return [fr[k] for k in order] + [synthetic.small_frame(40, 5, duplicates=2)], order


@pytest.mark.parametrize("basis", ["X", "XV"])
def test_radius_grid_geometry(ops, basis):
    """Item 3: one batch of (a) two clusters a kilometre apart (the h *= 1.5 loop runs a dozen times), (b) a horizontal and a
    vertical line (one-row grids), (c) 60 coincident points (every pair an edge, rows beyond the cache), (d) two points exactly r
    apart and two points nextafter(r) apart, (e) negative coordinates only, (f) a single point and an empty frame."""
    frames, order = geometry_batch()
    r = gi.GEOMETRY_R
    out = check_radius(ops, frames, r, basis)
    if basis == "X":
        E, off = out["exp"], np.concatenate([[0], np.cumsum([f.n for f in frames])])
        per = {name: int(((E[:, 0] >= off[j]) & (E[:, 0] < off[j + 1])).sum()) for j, name in enumerate(order)}
        assert per["pair_at_r"] == 2 and per["pair_beyond_r"] == 0 and per["single"] == 0 and per["empty"] == 0
        assert per["coincident"] == 60 * 59


@functools.lru_cache(maxsize=None)
def translated_oracle():
    """The four exactly translated clouds with the oracle's radius graph (r = 1) and 20 nearest neighbours of each, computed once."""
    clouds = gi.translated_clouds()
    return clouds, [go.radius_edges(c.X, 1.0).astype(np.int64) for c in clouds], [go.knn_neighbours(c.X, 20) for c in clouds]


def test_radius_translation(ops):
    """Item 4: the same cloud (coordinates on a 2^-10 raster) moved by exactly representable offsets of up to 6.5e6 m gives the
    oracle's graph of the moved coordinates, and the same graph every time."""
    clouds, radius_exp, _ = translated_oracle()
    outs = []
    for c, exp in zip(clouds, radius_exp):
        assert np.array_equal(exp, radius_exp[0])
        outs.append(check_radius(ops, [c], 1.0, exp=exp))
    for o in outs[1:]:
        assert torch.equal(o["rowptr"], outs[0]["rowptr"]) and torch.equal(o["col"], outs[0]["col"]) and torch.equal(o["ei"], outs[0]["ei"])
        assert torch.equal(o["rel"], outs[0]["rel"])


@pytest.mark.parametrize("which", ["ties_X", "ties_XV", "ties_X8", "ties_01_X", "stars"])
def test_radius_split_fill_equals_the_fused_fill(ops, which, monkeypatch):
    """Item 5: k_radius<., true> + k_rank_rows (ops.FUSED_RADIUS_ROWS off), plain and guarded, on the tie batches and the star
    batch: the guarded variant leaves the status clear, both give the fused launch's rows and the oracle's."""
    if which == "stars":
        (frames, _), r, basis = gi.star_batch(), gi.STAR_R, "X"
    elif which == "ties_01_X":
        frames, r, basis = tie_batch(0.1), 0.3, "X"
    else:
        frames, r, basis = tie_batch(0.5), 1.0, which.split("_")[1]
    assert ops.FUSED_RADIUS_ROWS
    fused = check_radius(ops, frames, r, basis)
    X, P = fused["X"], fused["P"]
    monkeypatch.setattr(ops, "FUSED_RADIUS_ROWS", False)
    for mfp in (fused["biggest"], 0):
        g, rowptr = ops.radius_graph_count(X, P, r, max_frame_points=mfp)
        assert torch.equal(rowptr, fused["rowptr"])
        col, ei, rel = ops.radius_graph_fill(g, rowptr, r, fused["n_edges"], relative_position="directed")
        assert torch.equal(col, fused["col"]) and torch.equal(ei, fused["ei"]) and torch.equal(rel, fused["rel"])
        status = torch.zeros(1, dtype=torch.int32, device=X.device)
        col, ei = ops.radius_graph_fill(g, rowptr, r, fused["n_edges"], guard_status=status)
        assert int(status.item()) == 0
        assert torch.equal(col, fused["col"]) and torch.equal(ei, fused["ei"])
    monkeypatch.setattr(ops, "FUSED_RADIUS_ROWS", True)
    status = torch.zeros(1, dtype=torch.int32, device=X.device)
    col, ei = ops.radius_graph_fill(g, rowptr, r, fused["n_edges"], guard_status=status)      # the fused launch, guarded
    assert int(status.item()) == 0 and torch.equal(col, fused["col"]) and torch.equal(ei, fused["ei"])


# ================================================================================================ kNN search
def knn_expected(frames, k, basis="X", nbr20=None):
    if nbr20 is not None:                                              # rows (distance asc, index asc): the first k of the first 20
        n = nbr20.shape[0]
        return np.stack([np.repeat(np.arange(n, dtype=np.int64), k), nbr20[:, :k].reshape(-1).astype(np.int64)], 1)
    return oracle_batch_edges(frames, "knn", k=k, basis=basis)


def check_knn(ops, frames, k, basis="X", mfps=None, exp=None, attrs=True):
    """ops.knn_graph at every given frame-size promise against the oracle (rows, degree, and for k <= 64 the relative_position /
    out-degree outputs); the promises against one another.  -> (nbr, ei) of the first."""
    Xb, ptr = batch(frames, basis)
    n = Xb.shape[0]
    if exp is None:
        exp = knn_expected(frames, k, basis)
    X, P = dev(Xb), dev(ptr)
    biggest = max(f.n for f in frames)
    first = None
    for mfp in (mfps if mfps is not None else (0, biggest)):
        nbr, ei, st = ops.knn_graph(X, P, k, max_frame_points=mfp)
        assert st.item() == 0
        assert np.array_equal(ei.t().cpu().numpy(), exp), mfp
        assert np.array_equal(nbr.cpu().numpy().reshape(-1), exp[:, 1]), mfp
        if first is None:
            first = (nbr, ei)
            rowptr = torch.arange(0, n * k + 1, k, dtype=torch.int32, device="cuda")
            deg = ops.undirected_degree(rowptr, nbr.reshape(-1), n).cpu().numpy()
            assert np.array_equal(deg, oracle_batch_degree(frames, exp))
        else:
            assert torch.equal(nbr, first[0]) and torch.equal(ei, first[1]), mfp
        if attrs and k <= 64:
            for mode in ("directed", "undirected"):
                nbr_a, ei_a, st_a, rel, dg = ops.knn_graph(X, P, k, max_frame_points=mfp, relative_position=mode, degree_init=True)
                assert st_a.item() == 0 and torch.equal(nbr_a, first[0]) and torch.equal(ei_a, first[1]), (mfp, mode)
                assert (dg == k).all()
                assert np.array_equal(rel.cpu().numpy(), rel_expected(Xb, ei_a, mode == "undirected")), (mfp, mode)
    return first


@pytest.mark.parametrize("biggest", [320, 321, 512, 513])
@pytest.mark.parametrize("k", [1, 2, 3, 32, 33, 63, 64, 65])
def test_knn_dispatch_edges(ops, k, biggest):
    """Item 6: k below 3 (grid walk), up to / beyond KF_MAXK = 32 (brute force / team), up to / beyond 64 (team / one thread per
    query) x the biggest frame at 320 / 321 / 512 / 513 points (register layouts NV = 5 / 8 / 16, the grid walk above 512), with
    and without the frame-size promise, frames of k + 1 points and of sizes = 1, 7 (mod KF_QPW = 8), bases X and [X, V]."""
    frames = gi.knn_dispatch_frames(k, biggest)
    for basis in ("X", "XV"):
        check_knn(ops, frames, k, basis)


@pytest.mark.parametrize("k", [3, 33])
def test_knn_team_widths(ops, k, monkeypatch):
    """Item 6, RGNN_KNN_TEAM = 0 / 16 / 32: one thread per query and the narrow teams against the default (64 lanes) and the oracle."""
    frames = gi.knn_dispatch_frames(k, 321)
    Xb, ptr = batch(frames)
    X, P = dev(Xb), dev(ptr)
    exp = knn_expected(frames, k)
    nbr0, ei0 = check_knn(ops, frames, k, mfps=(0,), exp=exp)
    for team in (0, 16, 32):
        set_env(ops, monkeypatch, "RGNN_KNN_TEAM", team)
        nbr, ei, st = ops.knn_graph(X, P, k)
        assert st.item() == 0 and torch.equal(nbr, nbr0) and torch.equal(ei, ei0), team
        assert np.array_equal(ei.t().cpu().numpy(), exp), team
        nbr, ei, st, rel, dg = ops.knn_graph(X, P, k, relative_position="directed", degree_init=True)
        assert st.item() == 0 and torch.equal(nbr, nbr0) and torch.equal(ei, ei0) and (dg == k).all(), team
        assert np.array_equal(rel.cpu().numpy(), rel_expected(Xb, ei)), team
    set_env(ops, monkeypatch, "RGNN_KNN_TEAM", None)


@pytest.mark.parametrize("k", [3, 10])
def test_knn_ties_at_the_kth_place_under_every_kernel(ops, k, monkeypatch):
    """Item 7: a 0.5 lattice (equal distances at the k-th place in every interior row) and 40 coincident points among others
    (39 candidates at distance 0, broken by index) through the one-thread kernel, the team kernel and the brute-force kernel.
    (The 22 x 22 lattice fits the brute-force kernel's 512-point limit; the 24 x 24 one rides along on the grid walk.)"""
    small = [gi.lattice(22, 0.5), gi.coincident_among_others(), synthetic.nuscenes_frame(6)]
    large = small + [gi.lattice(24, 0.5)]
    assert max(f.n for f in small) <= 512
    for basis in ("X", "XV"):
        exp_s, exp_l = knn_expected(small, k, basis), knn_expected(large, k, basis)
        set_env(ops, monkeypatch, "RGNN_KNN_TEAM", 0)
        one_s = check_knn(ops, small, k, basis, mfps=(0,), exp=exp_s, attrs=False)              # k_knn
        one_l = check_knn(ops, large, k, basis, mfps=(0,), exp=exp_l, attrs=False)
        set_env(ops, monkeypatch, "RGNN_KNN_TEAM", None)
        team_s = check_knn(ops, small, k, basis, mfps=(0, max(f.n for f in small)), exp=exp_s)    # k_knn_team, then k_knn_frame
        team_l = check_knn(ops, large, k, basis, mfps=(0,), exp=exp_l)
        assert torch.equal(one_s[0], team_s[0]) and torch.equal(one_s[1], team_s[1])
        assert torch.equal(one_l[0], team_l[0]) and torch.equal(one_l[1], team_l[1])


def test_knn_grid_geometry(ops, monkeypatch):
    """Item 8: lines (zero-area branch, one-row grids padded to 8-row tiles), two clusters a kilometre apart and a 1 000 m x 1 mm
    strip, k = 5: the ring walk's termination on coarsened grids, with and without the frame-size promise, team and one thread."""
    fr = gi.geometry_frames()
    frames = [fr["line_h"], fr["clusters"], gi.thin_strip(), fr["line_v"], fr["negative"]]
    exp = knn_expected(frames, 5)
    a = check_knn(ops, frames, 5, exp=exp)
    set_env(ops, monkeypatch, "RGNN_KNN_TEAM", 0)
    b = check_knn(ops, frames, 5, mfps=(0,), exp=exp, attrs=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("k", [10, 20])
def test_knn_translation(ops, k, monkeypatch):
    """Item 8: the exactly translated clouds (offsets up to 6.5e6 m): the termination bound of the ring walk must not depend on
    where the frame lies -- the oracle's rows for every copy, the same rows for all copies, on the grid walk (no frame size) and
    with the frame size given, team kernel and one-thread kernel."""
    clouds, _, nbr20 = translated_oracle()
    outs = []
    for c, nb in zip(clouds, nbr20):
        assert np.array_equal(nb, nbr20[0])
        exp = knn_expected([c], k, nbr20=nb)
        outs.append(check_knn(ops, [c], k, exp=exp, attrs=(k == 10)))
    set_env(ops, monkeypatch, "RGNN_KNN_TEAM", 0)
    for c, nb in zip(clouds, nbr20):
        outs.append(check_knn(ops, [c], k, mfps=(0,), exp=knn_expected([c], k, nbr20=nb), attrs=False))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])


@pytest.mark.parametrize("mfp,team", [(0, None), (0, 0), (50, None)])
def test_knn_short_frames_inside_a_batch(ops, mfp, team, monkeypatch):
    """Item 9: frames of (50, k, 50, k - 1, 1) points, k = 6: the status bit is raised, the 50-point frames' rows are the oracle's,
    every entry of the short frames is -1 with edge_index = (i, -1) -- on the grid walk (team and one thread) and brute force."""
    k = 6
    frames = gi.short_frame_batch(k)
    sizes = [f.n for f in frames]
    assert sizes == [50, k, 50, k - 1, 1]
    Xb, ptr = batch(frames)
    set_env(ops, monkeypatch, "RGNN_KNN_TEAM", team)
    nbr, ei, st = ops.knn_graph(dev(Xb), dev(ptr), k, max_frame_points=mfp)
    assert st.item() == ops.STATUS_KNN_TOO_FEW_POINTS
    nbr, ei = nbr.cpu().numpy(), ei.cpu().numpy()
    assert np.array_equal(ei[0], np.repeat(np.arange(sum(sizes)), k))
    assert np.array_equal(ei[1], nbr.reshape(-1))
    for j, f in enumerate(frames):
        lo, hi = int(ptr[j]), int(ptr[j + 1])
        if f.n > k:
            assert np.array_equal(nbr[lo:hi], go.knn_neighbours(f.X, k) + lo), j
        else:
            assert (nbr[lo:hi] == -1).all(), j


# ================================================================================================ grid-build paths
def nearest_rows(d2, k):
    """Rows (distance asc, index asc) of the k smallest entries of every row of d2 -- the order of go.knn_neighbours, without
    sorting whole rows."""
    kth = np.partition(d2, k, axis=1)[:, k]
    rows = np.empty((d2.shape[0], k), dtype=np.int64)
    for a in range(d2.shape[0]):
        c = np.nonzero(d2[a] <= kth[a])[0]
        rows[a] = c[np.lexsort((c, d2[a, c]))[:k]]
    return rows


@functools.lru_cache(maxsize=None)
def threshold_case(n):
    """A frame of n uniform points beside a 300-point one, with the oracle's radius graph (r = 1) and 4 nearest neighbours: of
    every row up to 4 097 points (go.radius_edges / go.knn_neighbours), of a fixed sample of 1 000 rows above (the same float64
    distances, as test_stress_cloud_radius_properties samples them)."""
    frames = [gi.uniform_square(n), synthetic.nuscenes_frame(12)]
    big, small = frames[0].X, frames[1].X
    if n <= 4097:
        q = np.arange(n)
        E = go.radius_edges(big, 1.0)
        cut = np.searchsorted(E[:, 0], np.arange(n + 1))
        radius_rows = [E[cut[i]:cut[i + 1], 1] for i in range(n)]
        knn_rows = go.knn_neighbours(big, 4)
    else:
        q = np.sort(np.random.default_rng(1).choice(n, 1000, replace=False))
        d2 = go._reduced_distances(big[q], big)
        d2[np.arange(len(q)), q] = np.inf
        radius_rows = [np.nonzero(h)[0] for h in d2 <= 1.0]
        knn_rows = nearest_rows(d2, 4)
    return frames, q, radius_rows, knn_rows, go.radius_edges(small, 1.0).astype(np.int64) + n, go.knn_neighbours(small, 4) + n


@pytest.mark.parametrize("n,no_reg", [(4096, False), (4097, False), (16352, False), (16353, False), (4096, True), (4097, True)])
def test_grid_build_frame_size_thresholds(ops, n, no_reg, monkeypatch):
    """Item 10: 4 096 / 4 097 points (the register-resident block's limit), 16 352 / 16 353 (the LDS cell table's limit; beyond it
    the five-launch path), each beside a 300-point frame: the cell order is a permutation, radius graph and 4-NN rows are equal
    with and without the frame-size promise and equal the oracle's (every row up to 4 097 points, 1 000 sampled rows above);
    4 096 / 4 097 also with the register-resident block switched off."""
    frames, q, radius_rows, knn_rows, small_E, small_nbr = threshold_case(n)
    if no_reg:
        set_env(ops, monkeypatch, "RGNN_GRID_NO_REG", 1)
    Xb, ptr = batch(frames)
    X, P = dev(Xb), dev(ptr)
    total, biggest = Xb.shape[0], max(f.n for f in frames)
    assert biggest == n
    outs = []
    for mfp in (biggest, 0):
        g = ops.GridHash(X, P).build(cell_size=1.0, max_frame_points=mfp)
        order, rank = g.cell_order().clone().long(), g.cell_rank().clone().long()
        ar = torch.arange(total, device=order.device)
        assert torch.equal(torch.sort(order).values, ar) and torch.equal(order[rank], ar)
        gk, rowptr = ops.radius_graph_count(X, P, 1.0, max_frame_points=mfp)
        n_edges = int(rowptr[-1].item())
        col, ei = ops.radius_graph_fill(gk, rowptr, 1.0, n_edges)
        nbr, kei, st = ops.knn_graph(X, P, 4, max_frame_points=mfp)
        assert st.item() == 0
        outs.append((order, rank, rowptr.clone(), col, ei, nbr, kei))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    _, _, rowptr, col, ei, nbr, kei = outs[0]
    rp, cc, nb = rowptr.cpu().numpy(), col.cpu().numpy(), nbr.cpu().numpy()
    assert np.array_equal(ei[1].cpu().numpy(), cc) and np.array_equal(ei[0].cpu().numpy(), np.repeat(np.arange(total), np.diff(rp)))
    assert np.array_equal(kei[1].cpu().numpy(), nb.reshape(-1)) and np.array_equal(kei[0].cpu().numpy(), np.repeat(np.arange(total), 4))
    for a, i in enumerate(q):
        assert np.array_equal(cc[rp[i]:rp[i + 1]], radius_rows[a]), i
    assert np.array_equal(nb[q], knn_rows)
    if len(q) == n:                                                    # the whole graph: edge count and undirected degree too
        assert rp[n] == sum(len(r_) for r_ in radius_rows)
        E_big = np.stack([np.repeat(np.arange(n), np.diff(rp[:n + 1])), cc[:rp[n]]], 1)
        deg = ops.undirected_degree(rowptr, col, total).cpu().numpy()
        assert np.array_equal(deg, np.concatenate([go.undirected_degree(E_big, n), go.undirected_degree(small_E - n, total - n)]))
    assert np.array_equal(np.stack([np.repeat(np.arange(n, total), np.diff(rp[n:])), cc[rp[n]:]], 1), small_E)
    assert np.array_equal(nb[n:], small_nbr)
