"""Non-vacuity of tests/graph_edge_inputs.py: every builder really hits the edge of csrc/graph.hip it is named for, shown from the
float64 oracle and a numpy restatement of k_frame_grid alone (no GPU).  If someone later "simplifies" an input, this fails before
tests/test_gpu_graph_edges.py goes quietly vacuous."""
import numpy as np
import pytest

import graph_edge_inputs as gi
from oracle import graph_oracle as go


def _row_lengths(frames, r, basis="X"):
    out = []
    for f in frames:
        E = go.build_edges(gi.basis(f, basis), "radius", r=r)
        out.append(np.bincount(E[:, 0], minlength=f.n) if E is not None else np.zeros(f.n, np.int64))
    return np.concatenate(out)


def test_lattices_hold_exact_ties_at_the_radius():
    f = gi.lattice(24, 0.5)
    exact, near = gi.tie_counts(f.X, 1.0)
    assert exact >= 2000 and go.radius_edges(f.X, 1.0).shape[0] == 6436 and exact == 2112
    moved = gi.lattice(24, 0.5, offset=(2.0 ** 23, 2.0 ** 23))
    assert gi.tie_counts(moved.X, 1.0) == (exact, near) and go.radius_edges(moved.X, 1.0).shape[0] == 6436
    assert np.array_equal(moved.X - 2.0 ** 23, f.X)
    # a `<` for `<=` would lose every tie: the graph with the ties differs from the graph without them
    d2 = go._reduced_distances(f.X, f.X)
    assert int((d2 < 1.0).sum()) - f.n == 6436 - exact
    g = gi.lattice(24, 0.1)
    exact01, near01 = gi.tie_counts(g.X, 0.3)
    assert exact01 >= 90 and near01 >= 1500 and near01 > exact01         # ties AND misses by a few ulp, on either side
    d2 = go._reduced_distances(g.X, g.X)
    r2 = 0.3 * 0.3
    band = np.abs(d2 - r2) <= 4 * np.spacing(r2)
    assert (band & (d2 > r2)).any() and (band & (d2 < r2)).any()
    # the wider bases keep exact ties (their extra columns are multiples of 0.25)
    for b in ("XV", "X8"):
        assert gi.tie_counts(gi.basis(f, b), 1.0)[0] >= 300, b
        assert gi.tie_counts(gi.basis(g, b), 0.3)[0] >= 8, b
    assert gi.basis(f, "X8").shape == (576, 8) and gi.basis(f, "XV").shape == (576, 4)


@pytest.mark.parametrize("d", gi.STAR_DEGREES)
def test_star_hub_has_exactly_the_named_degree(d):
    f, hub = gi.star(d)
    assert f.n == d + 1 and np.array_equal(f.X[hub], [0.0, 0.0])
    deg = _row_lengths([f], gi.STAR_R)
    assert deg[hub] == d
    assert (np.delete(deg, hub) >= 1).all()                                # every spoke sees at least the hub


def test_star_batch_has_rows_of_every_class():
    frames, hubs = gi.star_batch()
    deg = _row_lengths(frames, gi.STAR_R)
    assert [int(deg[hubs[d]]) for d in gi.STAR_DEGREES] == list(gi.STAR_DEGREES)
    assert set(np.unique(deg % 4)) == {0, 1, 2, 3} and set(np.unique(deg % 16)) == set(range(16))
    for t in (gi.TEAM_LANES, gi.RADIUS_CACHE, gi.ROWS_LDS_DIRECT, gi.ROWS_LDS):       # a row on, below and above every threshold
        assert {t - 1, t, t + 1} <= set(deg.tolist()), t
    # rows of every class inside ONE block of the fill pass (16 consecutive rows per block)
    cls = np.digitize(deg, [1, gi.RADIUS_CACHE + 1, gi.ROWS_LDS_DIRECT + 1, gi.ROWS_LDS + 1])
    mixed = [len(set(cls[b:b + 16])) for b in range(0, len(deg), 16)]
    assert max(mixed) >= 3
    assert any(f.n and go.build_edges(f.X, "radius", r=gi.STAR_R).shape[0] < f.n * 10 for f in frames)    # the clutter frame


def test_geometry_frames_take_the_named_branches_of_the_grid():
    fr = gi.geometry_frames()
    r = gi.GEOMETRY_R
    # radius mode: h starts just above r and grows by 1.5 until the padded grid fits 2 n + 64 cells
    a = gi.frame_grid(fr["clusters"].X, cell_size=r)
    assert a["grows"] >= 10 and a["h"] > 100 * r and a["cells"] <= a["cap"]
    for name in ("line_h", "line_v"):
        g = gi.frame_grid(fr[name].X, cell_size=r)
        assert g["grows"] >= 1 and min(g["gx"], g["gy"]) == 1
        k = gi.frame_grid(fr[name].X, 0.0, 2.0)
        assert k["branch"] == "zero_area" and k["grows"] >= 1 and min(k["gx"], k["gy"]) == 1
    assert gi.frame_grid(fr["clusters"].X, 0.0, 2.0)["grows"] >= 1
    s = gi.frame_grid(gi.thin_strip().X, 0.0, 2.0)
    assert s["branch"] == "area" and s["grows"] >= 1 and s["gy"] == 1
    assert gi.frame_grid(fr["coincident"].X, 0.0, 2.0)["branch"] == "coincident"
    assert gi.frame_grid(fr["coincident"].X, 0.0, 2.0)["h"] == 1.0
    # the hmin clamp: a strip so thin that the area rule asks for cells below 1e-6 of the extent
    assert gi.frame_grid(gi.thin_strip(width=1e-12).X, 0.0, 2.0)["branch"] == "area+hmin"
    # the bound itself: r apart is an edge, the next float is not
    assert go.radius_edges(fr["pair_at_r"].X, r).shape[0] == 2 and go.radius_edges(fr["pair_beyond_r"].X, r).shape[0] == 0
    assert (fr["negative"].X < 0).all() and fr["single"].n == 1 and fr["empty"].n == 0
    n = fr["coincident"].n
    assert go.radius_edges(fr["coincident"].X, r).shape[0] == n * (n - 1) and n - 1 > gi.RADIUS_CACHE


def test_translations_are_exact():
    base = gi.dyadic_cloud()
    assert np.array_equal(base.X * 1024.0, np.round(base.X * 1024.0)) and base.n == 3000
    for o, c in zip(gi.TRANSLATIONS, gi.translated_clouds()):
        off = np.asarray(o)
        assert np.array_equal(off * 1024.0, np.round(off * 1024.0))
        assert np.array_equal((base.X + off) - off, base.X) and np.array_equal(c.X - off, base.X)
        d = c.X[:50, None, :] - c.X[None, :50, :]
        assert np.array_equal(d, base.X[:50, None, :] - base.X[None, :50, :])       # differences, hence distances, bit for bit
    assert max(abs(v) for o in gi.TRANSLATIONS for v in o) >= 6.5e6                   # RadarScenes-like global coordinates


@pytest.mark.parametrize("k", [1, 2, 3, 32, 33, 63, 64, 65])
@pytest.mark.parametrize("biggest", [320, 321, 512, 513])
def test_knn_dispatch_frames(k, biggest):
    sizes = [f.n for f in gi.knn_dispatch_frames(k, biggest)]
    assert max(sizes) == biggest and min(sizes) == k + 1
    assert any(s % 8 == 1 for s in sizes) and any(s % 8 == 7 for s in sizes)


def test_knn_tie_frames_and_short_frames():
    f = gi.coincident_among_others()
    same = (f.X == 1.75).all(1)
    assert same.sum() == 40 and same.sum() - 1 > 10                                     # 39 candidates at distance 0 for k = 10
    lat = gi.lattice(22, 0.5)
    assert lat.n <= 512                                                                   # the brute-force kernel takes it
    d2 = go._reduced_distances(lat.X[:64], lat.X)
    d2[np.arange(64), np.arange(64)] = np.inf
    srt = np.sort(d2, 1)
    assert (srt[:, 9] == srt[:, 10]).mean() > 0.5 and (srt[:, 2] == srt[:, 3]).mean() > 0.5    # ties at the k-th place, k = 10 and 3
    assert [f.n for f in gi.short_frame_batch(6)] == [50, 6, 50, 5, 1]


@pytest.mark.parametrize("n", [4096, 4097, 16352, 16353])
def test_grid_build_thresholds(n):
    assert (n <= gi.GRID_REG_MAX_POINTS) == (n == 4096) and (n <= gi.GRID_LDS_MAX_POINTS) == (n != 16353)
    assert (gi.CELLS_PER_POINT * n + gi.CELLS_PER_FRAME <= 32 * 1024) == (n != 16353)
    f = gi.uniform_square(n)
    assert f.n == n and np.array_equal(np.round(f.X * 100.0), np.round(f.X * 100.0, 6))
    q = np.arange(0, n, max(1, n // 500))
    d2 = go._reduced_distances(f.X[q], f.X)
    mean_deg = ((d2 <= 1.0).sum() - len(q)) / len(q)
    assert 3.0 < mean_deg < 5.0
