"""Inputs that sit ON the thresholds of the neighbour search (csrc/graph.hip): pure numpy builders of ``synthetic.RadarFrame``s,
shared by tests/test_gpu_graph_edges.py (the kernels against the float64 oracle) and tests/test_graph_edge_inputs.py (proof,
from the oracle alone, that every input really hits the edge it is named for).  Needs no GPU.

All coordinates are finite.  Everything is deterministic (fixed PCG64 seeds)."""
import numpy as np

from radargnn_amd import synthetic

# thresholds of csrc/graph.hip that the builders aim at (restated: the CPU test ties the inputs to these numbers)
RADIUS_CACHE = 48          # rows up to here are copied from the count pass's cache
ROWS_LDS = 512             # k_radius_rows: dense rows up to here are ranked from LDS
ROWS_LDS_DIRECT = 128      # k_radius_rows_direct: the same split
TEAM_LANES = 16            # lanes per row of the fill pass (3 cache slots per lane)
CELLS_PER_POINT, CELLS_PER_FRAME = 2, 64
GRID_REG_MAX_POINTS = 4096                 # k_grid_frame_reg: GFR_PPT x GF_THREADS
GRID_LDS_MAX_POINTS = (32 * 1024 - 64) // 2  # k_grid_frame: 2 n + 64 <= GF_LDS_CELLS -> 16 352
STAR_DEGREES = (15, 16, 17, 47, 48, 49, 127, 128, 129, 511, 512, 513)
STAR_R = 2.0
GEOMETRY_R = 0.5
TRANSLATIONS = ((0.0, 0.0), (2.0 ** 20, -2.0 ** 20), (2.0 ** 23, 2.0 ** 23),
                (float(np.round(-6.5e6 * 1024.0) / 1024.0), float(np.round(4.1e5 * 1024.0) / 1024.0)))


def frame(X, V=None, seed=0):
    """A RadarFrame around coordinates X; V defaults to multiples of 0.5 (exact in every sum of squares used here)."""
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 2)
    n = X.shape[0]
    rng = np.random.Generator(np.random.PCG64(500 + seed))
    if V is None:
        V = rng.integers(0, 2, size=(n, 2)).astype(np.float64) * 0.5
    return synthetic.RadarFrame(X, np.ascontiguousarray(V, dtype=np.float64), rng.normal(size=(n, 1)), np.zeros((n, 1)))


def empty_frame():
    return synthetic.RadarFrame(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 1)), np.zeros((0, 1)))


def basis(f, name):
    """Distance basis of a frame: "X" [N,2], "XV" [N,4], "X8" [N,8] (X, V and four columns of small multiples of 0.25)."""
    if name == "X":
        return f.X
    if name == "XV":
        return np.concatenate((f.X, f.V), axis=1)
    if name == "X8":
        i = np.arange(f.n, dtype=np.int64)[:, None]
        W = ((i * np.array([1, 2, 3, 5])) % 3).astype(np.float64) * 0.25
        return np.concatenate((f.X, f.V, W), axis=1)
    raise ValueError(name)


def translated(f, offset):
    return synthetic.RadarFrame(f.X + np.asarray(offset, dtype=np.float64), f.V, f.rcs, f.timestamp)


# ------------------------------------------------------------------------------------------------ ties at the radius
def lattice(side=24, spacing=0.5, offset=(0.0, 0.0), seed=1):
    """side x side lattice in a shuffled row order.  spacing 0.5, r = 1: thousands of pairs at d2 == r2 exactly (and V in
    {0, 0.5}^2 keeps sums of squares exact on the XV / X8 bases); spacing 0.1, r = 0.3: exact ties and near misses by a few ulp."""
    gx, gy = np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64))
    X = np.stack([gx.ravel(), gy.ravel()], 1) * spacing
    rng = np.random.Generator(np.random.PCG64(40 + seed))
    X = X[rng.permutation(len(X))] + np.asarray(offset, dtype=np.float64)
    return frame(X, seed=seed)


def tie_counts(Xb, r, ulps=4):
    """(ordered pairs with d2 == r2 exactly, ordered pairs within `ulps` ulp of r2 on either side), oracle arithmetic."""
    from oracle import graph_oracle as go
    d2 = go._reduced_distances(Xb, Xb)
    np.fill_diagonal(d2, np.inf)
    r2 = float(r) * float(r)
    return int((d2 == r2).sum()), int((np.abs(d2 - r2) <= ulps * np.spacing(r2)).sum())


# ------------------------------------------------------------------------------------------------ row lengths
def star(d, r=STAR_R, seed=0):
    """A hub at the origin and d spokes at radii in (0.6 r, 0.95 r): the hub's row holds exactly d neighbours.
    -> (frame, row of the hub)."""
    rng = np.random.Generator(np.random.PCG64(7000 + 13 * d + seed))
    rad = rng.uniform(0.6 * r, 0.95 * r, size=d)
    ang = rng.uniform(0.0, 2.0 * np.pi, size=d)
    hub = d // 2
    X = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    X = np.concatenate([X[:hub], np.zeros((1, 2)), X[hub:]])
    return frame(np.round(X * 1024.0) / 1024.0, seed=d), hub


def star_batch(degrees=STAR_DEGREES):
    """Stars of every named degree around a clutter frame -> (frames, {d: global row of its hub})."""
    frames, hubs, off = [], {}, 0
    for j, d in enumerate(degrees):
        f, hub = star(d)
        frames.append(f)
        hubs[d] = off + hub
        off += f.n
        if j == len(degrees) // 2:
            c = synthetic.radarscenes_frame(9, n_clusters=10, pts_per_cluster=20, n_clutter=100)
            frames.append(c)
            off += c.n
    return frames, hubs


# ------------------------------------------------------------------------------------------------ grid geometry
def two_clusters(gap=1000.0, per=20, seed=2):
    rng = np.random.Generator(np.random.PCG64(60 + seed))
    a = np.round(rng.normal(size=(per, 2)) * 0.4, 3)
    b = np.round(rng.normal(size=(per, 2)) * 0.4, 3) + np.array([gap, 0.0])
    X = np.concatenate([a, b])
    return frame(X[rng.permutation(len(X))], seed=seed)


def collinear(n=200, spacing=0.25, vertical=False, seed=3):
    rng = np.random.Generator(np.random.PCG64(70 + seed))
    t = np.arange(n, dtype=np.float64)[rng.permutation(n)] * spacing
    z = np.full(n, 3.0)
    return frame(np.stack([z, t], 1) if vertical else np.stack([t, z], 1), seed=seed)


def coincident(n=60, at=(7.25, -2.5)):
    return frame(np.tile(np.asarray(at, dtype=np.float64), (n, 1)), seed=4)


def pair(distance):
    return frame(np.array([[0.0, 2.0], [distance, 2.0]]), seed=5)       # (x = 0: the difference is `distance` to the last bit)


def negative(n=80, seed=6):
    rng = np.random.Generator(np.random.PCG64(80 + seed))
    return frame(np.round(rng.uniform(-60.0, -50.0, size=(n, 2)), 2), seed=seed)


def thin_strip(n=400, length=1000.0, width=0.001, seed=7):
    rng = np.random.Generator(np.random.PCG64(90 + seed))
    X = np.stack([rng.uniform(0.0, length, size=n), rng.uniform(0.0, width, size=n)], 1)
    return frame(X, seed=seed)


def geometry_frames(r=GEOMETRY_R):
    """Item by item: (a) two far clusters, (b) a horizontal and a vertical line, (c) 60 coincident points, (d) two points r apart
    and two points nextafter(r) apart, (e) negative coordinates only, (f) one point and no point."""
    return {"clusters": two_clusters(), "line_h": collinear(), "line_v": collinear(vertical=True), "coincident": coincident(),
            "pair_at_r": pair(r), "pair_beyond_r": pair(float(np.nextafter(r, np.inf))), "negative": negative(),
            "single": frame(np.array([[4.0, 4.0]])), "empty": empty_frame()}


def frame_grid(X, cell_size=0.0, pts_per_cell=2.0):
    """frame_grid_geometry's arithmetic (csrc/graph.hip: the one function every grid build calls), step by step, in float64 -> dict(h, gx, gy, cells, cap, grows, branch)."""
    n = X.shape[0]
    cap = CELLS_PER_POINT * n + CELLS_PER_FRAME
    ex = float(X[:, 0].max() - X[:, 0].min())
    ey = float(X[:, 1].max() - X[:, 1].min())
    if cell_size > 0:
        h, branch = cell_size * (1.0 + 9.5367431640625e-07), "radius"
    else:
        area = ex * ey
        if area > 0:
            h, branch = float(np.sqrt(area * pts_per_cell / float(n))), "area"
        elif ex + ey > 0:
            h, branch = (ex + ey) * pts_per_cell / float(n), "zero_area"
        else:
            h, branch = 1.0, "coincident"
        hmin = max(ex, ey) * 1e-6
        if h < hmin:
            h, branch = hmin, branch + "+hmin"
        if not h > 0:
            h = 1.0
    grows = 0
    while True:
        gx = int(np.floor(ex / h)) + 1
        gy = int(np.floor(ey / h)) + 1
        cells = ((gx + 7) // 8) * ((gy + 7) // 8) * 64
        if cells <= cap:
            break
        h *= 1.5
        grows += 1
    return dict(h=h, gx=gx, gy=gy, cells=cells, cap=cap, grows=grows, branch=branch)


# ------------------------------------------------------------------------------------------------ translation
def dyadic_cloud(frame_idx=2):
    """An ordinary RadarScenes-shaped frame rounded to multiples of 2^-10: adding any of TRANSLATIONS is exact."""
    f = synthetic.radarscenes_frame(frame_idx)
    return synthetic.RadarFrame(np.round(f.X * 1024.0) / 1024.0, f.V, f.rcs, f.timestamp)


def translated_clouds():
    base = dyadic_cloud()
    return [translated(base, o) for o in TRANSLATIONS]


# ------------------------------------------------------------------------------------------------ kNN dispatch
def knn_dispatch_frames(k, biggest):
    """Ragged frames, all of more than k points: the biggest of `biggest` points, one of exactly k + 1, sizes = 1 and 7 (mod 8),
    and a nuScenes-shaped one (300)."""
    a = 8 * ((k + 8) // 8) + 1
    b = 8 * ((k + 8) // 8) + 7
    frames = [synthetic.small_frame(a, 21, duplicates=2), synthetic.small_frame(biggest, 22, duplicates=5),
              synthetic.small_frame(k + 1, 23, duplicates=1), synthetic.nuscenes_frame(31), synthetic.small_frame(b, 24)]
    assert all(f.n > k for f in frames) and max(f.n for f in frames) == biggest
    return frames


def coincident_among_others(n_same=40, n_other=100, seed=8):
    rng = np.random.Generator(np.random.PCG64(100 + seed))
    X = np.concatenate([np.full((n_same, 2), 1.75), np.round(rng.normal(size=(n_other, 2)) * 2.0, 2)])
    return frame(X[rng.permutation(len(X))], seed=seed)


def short_frame_batch(k=6):
    return [synthetic.small_frame(50, 41), synthetic.small_frame(k, 42), synthetic.small_frame(50, 43, duplicates=3),
            synthetic.small_frame(k - 1, 44), synthetic.small_frame(1, 45)]


# ------------------------------------------------------------------------------------------------ grid-build thresholds
def uniform_square(n, seed=9):
    """n uniform points, rounded to 0.01, in a square sized for about 4 neighbours within r = 1 (n pi / side^2 = 4)."""
    rng = np.random.Generator(np.random.PCG64(110 + seed))
    side = float(np.sqrt(n * np.pi / 4.0))
    return frame(np.round(rng.uniform(0.0, side, size=(n, 2)), 2), V=np.zeros((n, 2)), seed=seed)
