"""CPU oracle of the batched DBSCAN (ops.dbscan_labels / radargnn_amd.clustering) and the inputs of its tests.  TEST INFRASTRUCTURE ONLY:
numpy, float64, no GPU.

Neighbourhoods come from oracle/graph_oracle.py (``radius_edges``: the KD-tree arithmetic the device search is pinned to, inclusive
``d2 <= eps * eps``, self excluded by identity); the rule of include/rgnn.h ("clustering") follows in its sequential form: core
points, a union-find over the core-core edges that hooks the larger root under the smaller, clusters numbered by ascending root per
frame, border points to the smallest number among their core neighbours.

Shared by tests/test_dbscan_oracle.py (CPU, against scikit-learn) and tests/test_gpu_dbscan.py; every named case and its expected
result are computed once and are read-only."""
import functools

import numpy as np

from oracle import graph_oracle as go

CAP = 24 * 1024                 # rgnn_dbscan_max_frame_points(): tests/test_gpu_dbscan.py checks the library agrees
WINDOWED_FROM = 2048            # frames from this size: neighbour pairs through x-sorted windows (same arithmetic, not O(n^2))


def neighbour_pairs(X, eps):
    """(i, j) int64 of one frame, ascending in (i, j): j in S_i by distance alone.  Small frames: ``go.radius_edges`` as it is.  Large
    frames: the same test (``go._reduced_distances(..) <= eps * eps``) against the points whose first coordinate lies within 2 eps
    only -- a point farther than that in one coordinate alone has d2 >= (2 eps)^2 (1 - 2^-52) > eps^2, so nothing is lost."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = X.shape[0]
    if n < WINDOWED_FROM:
        E = go.radius_edges(X, eps)
        return E[:, 0].astype(np.int64), E[:, 1].astype(np.int64)
    order = np.argsort(X[:, 0], kind="stable")
    xs = X[order, 0]
    r2 = float(eps) * float(eps)
    ii, jj = [], []
    for s in range(0, n, 512):
        e = min(n, s + 512)
        lo = np.searchsorted(xs, xs[s] - 2 * eps, side="left")
        hi = np.searchsorted(xs, xs[e - 1] + 2 * eps, side="right")
        hit = go._reduced_distances(X[order[s:e]], X[order[lo:hi]]) <= r2
        a, b = np.nonzero(hit)
        a, b = order[s + a], order[lo + b]
        keep = a != b
        ii.append(a[keep])
        jj.append(b[keep])
    i, j = np.concatenate(ii), np.concatenate(jj)
    o = np.lexsort((j, i))
    return i[o].astype(np.int64), j[o].astype(np.int64)


def frame_pairs(X, eps, group=None):
    """The edges that exist in one frame: same group, group >= 0."""
    i, j = neighbour_pairs(X, eps)
    if group is not None:
        keep = (group[i] == group[j]) & (group[i] >= 0)
        i, j = i[keep], j[keep]
    return i, j


def label_frame(n, i, j, min_samples, group=None):
    """The rule on the edges (i, j) of one frame of n points -> (labels int32 [n], core bool [n], number of clusters)."""
    deg = np.bincount(i, minlength=n)
    core = deg + 1 >= min_samples
    if group is not None:
        core &= group >= 0
    parent = np.arange(n)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    both = core[i] & core[j] & (i < j)
    for a, b in zip(i[both].tolist(), j[both].tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(a) if core[a] else -1 for a in range(n)], dtype=np.int64)
    roots = np.unique(root[root >= 0])                                # ascending: the numbering
    labels = np.full(n, -1, dtype=np.int32)
    labels[core] = np.searchsorted(roots, root[core])
    border = ~core[i] & core[j]
    best = np.full(n, np.iinfo(np.int32).max, dtype=np.int64)
    np.minimum.at(best, i[border], labels[j[border]])
    hit = best < np.iinfo(np.int32).max
    labels[hit] = best[hit]
    return labels, core, len(roots)


def dbscan_batch(X, frame_ptr, eps, min_samples, group=None):
    """-> (labels int32 [N], core uint8 [N], n_clusters int32 [B]) of a batch laid back to back."""
    X = np.asarray(X, dtype=np.float64)
    labels, core, counts = np.full(X.shape[0], -1, np.int32), np.zeros(X.shape[0], np.uint8), []
    for f in range(len(frame_ptr) - 1):
        a, b = int(frame_ptr[f]), int(frame_ptr[f + 1])
        g = None if group is None else np.asarray(group[a:b])
        i, j = frame_pairs(X[a:b], eps, g)
        labels[a:b], c, k = label_frame(b - a, i, j, min_samples, g)
        core[a:b] = c
        counts.append(k)
    return labels, core, np.asarray(counts, dtype=np.int32)


def csr(X, frame_ptr, eps):
    """(rowptr int32 [N + 1], col int32 [E]) with global ids: the rows of the radius search."""
    ii, jj = [], []
    for f in range(len(frame_ptr) - 1):
        a, b = int(frame_ptr[f]), int(frame_ptr[f + 1])
        i, j = neighbour_pairs(X[a:b], eps)
        ii.append(i + a)
        jj.append(j + a)
    i, j = np.concatenate(ii), np.concatenate(jj)
    rowptr = np.concatenate(([0], np.cumsum(np.bincount(i, minlength=X.shape[0])))).astype(np.int32)
    return rowptr, j.astype(np.int32)


# ------------------------------------------------------------------------------------------------ inputs
def cloud(n, seed, quantum=None, dim=2, spread=None):
    """n points: blobs of 3..30 points plus a third of clutter over a square sized for ~1 clutter point per 9 m^2, rows shuffled.
    ``quantum``: coordinates rounded to a lattice (exact ties and coincident points).  ``dim`` > 2: further columns of small noise."""
    rng = np.random.default_rng(seed)
    if n == 0:
        return np.zeros((0, dim))
    side = spread if spread is not None else max(3.0 * np.sqrt(n), 4.0)
    pts, left = [], n - n // 3
    while left > 0:
        m = int(min(left, rng.integers(3, 31)))
        pts.append(rng.uniform(0, side, 2) + rng.normal(size=(m, 2)) * rng.uniform(0.2, 1.2))
        left -= m
    pts.append(rng.uniform(0, side, size=(n // 3, 2)))
    X = np.concatenate(pts)[:n]
    if quantum:
        X = np.round(X / quantum) * quantum
    if dim > 2:
        X = np.concatenate((X, rng.normal(size=(n, dim - 2)) * 0.3), axis=1)
    return X[rng.permutation(n)]


def batch(frames):
    ptr = np.concatenate(([0], np.cumsum([len(f) for f in frames]))).astype(np.int64)
    return np.concatenate(frames) if frames else np.zeros((0, 2)), ptr


def chain(n, eps, order="row", seed=0):
    """n points spaced exactly eps apart on a line (eps a power of two: every neighbour is a tie d2 == eps^2)."""
    x = np.arange(n, dtype=np.float64) * eps
    if order == "reversed":
        x = x[::-1]
    elif order == "shuffled":
        x = x[np.random.default_rng(seed).permutation(n)]
    return np.stack((x, np.full(n, 3.0)), axis=1)


def stars():
    """Stars of 5 leaves at 0.9 eps (eps = 1; neighbouring leaves 1.058 apart): with min_samples 5 the centre alone is core and the
    leaves are border points.  Centre first, last, in the middle; and one star of 300 leaves, all of them core."""
    out = []
    for s, at in enumerate((0, 5, 2)):
        ang = 2 * np.pi * (np.arange(5) + 0.1 * s) / 5
        leaves = 0.9 * np.stack((np.cos(ang), np.sin(ang)), axis=1)
        out.append(np.insert(leaves, at, 0.0, axis=0) + [10.0 * s, -4.0])
    ang = 2 * np.pi * np.arange(300) / 300
    out.append(np.concatenate((0.9 * np.stack((np.cos(ang), np.sin(ang)), axis=1), [[0.0, 0.0]])) + [50.0, 7.0])
    return np.concatenate(out)


def shared_border(reverse=False):
    """Two clusters (min_samples 4, eps 1) with the point at 1.5 between them: a border point with core neighbours in both."""
    X = np.array([[0, 0], [0.5, 0], [-0.5, 0], [1.5, 0], [2.5, 0], [3, 0], [3.5, 0]], dtype=np.float64)
    return X[::-1].copy() if reverse else X


def border_first():
    """A cluster whose lowest row is a border point: row 0 touches the blob's edge only."""
    return np.array([[1.9, 0.0], [1.0, 0.0], [0.5, 0.0], [0.0, 0.0], [0.5, 0.5], [0.5, -0.5], [30.0, 0.0]], dtype=np.float64)


def interleaved_classes(n=120, seed=11):
    """One blob whose points carry two classes alternately, a few rows that take no part (-1), and a far pair of class 2."""
    rng = np.random.default_rng(seed)
    X = np.concatenate((rng.normal(size=(n, 2)) * 1.5, [[40.0, 40.0], [40.3, 40.0]]))
    group = np.concatenate((np.arange(n) % 2, [2, 2])).astype(np.int32)
    group[rng.choice(n, 15, replace=False)] = -1
    return X, group


def wide_strip(n, seed):
    """n points at ~1 per m^2 in a strip 4 m wide: cheap for the windowed oracle at the cap, hundreds of clusters, border and noise."""
    rng = np.random.default_rng(seed)
    return np.stack((rng.uniform(0, n / 4.0, n), rng.uniform(0, 4.0, n)), axis=1)


def _sizes():
    return batch([cloud(n, 100 + n) for n in (0, 1, 2, 63, 64, 65, 1023, 1024, 1025)])


def _many_frames():
    rng = np.random.default_rng(5)
    sizes = [0 if f % 7 in (0, 3) else int(rng.integers(1, 120)) for f in range(70)]
    return batch([cloud(n, 200 + f, quantum=0.5 if f % 3 == 0 else None) for f, n in enumerate(sizes)])


def _grouped():
    Xa, ga = interleaved_classes()
    Xb = cloud(300, 31)
    gb = (np.arange(300) % 3 - 1).astype(np.int32)                     # -1, 0, 1 in turn
    X, ptr = batch([Xa, Xb, np.zeros((0, 2)), shared_border()])
    return X, ptr, np.concatenate((ga, gb, np.zeros(7, np.int32)))


def _case(X, ptr, eps, min_samples, group=None):
    return {"X": X, "frame_ptr": ptr, "eps": eps, "min_samples": min_samples, "group": group}


# name -> builder of {"X", "frame_ptr", "eps", "min_samples", "group"}
CASES = {
    "sizes": lambda: _case(*_sizes(), 1.0, 4),
    "chain_row": lambda: _case(*batch([chain(4096, 0.5)]), 0.5, 3),
    "chain_reversed": lambda: _case(*batch([chain(4096, 0.5, "reversed")]), 0.5, 3),
    "chain_shuffled": lambda: _case(*batch([chain(4096, 0.5, "shuffled")]), 0.5, 3),
    "chain_cap": lambda: _case(*batch([chain(CAP, 0.5)]), 0.5, 2),
    "cap": lambda: _case(*batch([cloud(300, 1), wide_strip(CAP, 2), cloud(200, 3)]), 1.0, 4),
    "stars": lambda: _case(*batch([stars()]), 1.0, 5),
    "lattice_half": lambda: _case(*batch([cloud(600, 7, quantum=0.5)]), 0.5, 3),
    "lattice_tenth": lambda: _case(*batch([cloud(500, 8, quantum=0.1, spread=12.0)]), 0.5, 3),
    "coincident": lambda: _case(*batch([np.concatenate((np.tile([[7.25, -2.5]], (40, 1)), cloud(100, 9)))]), 1.0, 5),
    "shared_border": lambda: _case(*batch([shared_border(), shared_border(True), border_first()]), 1.0, 4),
    "all_core": lambda: _case(*batch([cloud(500, 12), cloud(77, 13)]), 1.0, 1),
    "all_noise": lambda: _case(*batch([cloud(500, 12), cloud(77, 13)]), 1.0, 10 ** 6),
    "basis_4": lambda: _case(*batch([cloud(400, 14, dim=4), cloud(90, 15, dim=4)]), 1.0, 4),
    "basis_8": lambda: _case(*batch([cloud(400, 16, dim=8), cloud(90, 17, dim=8)]), 1.2, 4),
    "basis_3": lambda: _case(*batch([cloud(300, 18, dim=3)]), 1.0, 4),
    "many_frames": lambda: _case(*_many_frames(), 1.0, 3),
    "grouped": lambda: (lambda X, ptr, g: _case(X, ptr, 1.0, 4, g))(*_grouped()),
}
SKLEARN_CASES = [name for name in CASES if name not in ("chain_cap", "cap")]     # (the cap-sized ones: the windowed pairs are
#                                                                                  checked against radius_edges on a smaller strip)


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    c = case(name)
    out = dbscan_batch(c["X"], c["frame_ptr"], c["eps"], c["min_samples"], c["group"])
    for a in out:
        a.setflags(write=False)
    return out
