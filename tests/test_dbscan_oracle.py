"""The DBSCAN oracle (tests/dbscan_oracle.py) against scikit-learn, and proofs that the inputs of the GPU tests bite.  CPU only.

scikit-learn is always asked for ``algorithm="kd_tree"``: with "auto" small clouds go to the brute-force path, whose
|a|^2 - 2ab + |b|^2 arithmetic decides ties at d2 == eps^2 differently."""
import numpy as np
import pytest
import sklearn.cluster as sklearn_cluster

import dbscan_oracle as D


def sklearn_frame(X, eps, min_samples):
    n = X.shape[0]
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, bool)
    fit = sklearn_cluster.DBSCAN(eps=eps, min_samples=min_samples, algorithm="kd_tree").fit(X)
    core = np.zeros(n, bool)
    core[fit.core_sample_indices_] = True
    return fit.labels_, core


def sklearn_batch(X, frame_ptr, eps, min_samples, group):
    """scikit-learn per frame; with ``group`` per (frame, group) subset, the clusters of a frame renumbered by ascending smallest core
    row.  A border point keeps the cluster scikit-learn gave it inside its subset."""
    labels, core = np.full(X.shape[0], -1, np.int64), np.zeros(X.shape[0], bool)
    for f in range(len(frame_ptr) - 1):
        a, b = int(frame_ptr[f]), int(frame_ptr[f + 1])
        if group is None:
            labels[a:b], core[a:b] = sklearn_frame(X[a:b], eps, min_samples)
            continue
        found = []                                                     # (smallest core row, member rows) of every cluster
        for g in np.unique(group[a:b]):
            if g < 0:
                continue
            rows = a + np.nonzero(group[a:b] == g)[0]
            lab, c = sklearn_frame(X[rows], eps, min_samples)
            core[rows] = c
            for k in range(lab.max() + 1 if len(lab) else 0):
                found.append((rows[(lab == k) & c].min(), rows[lab == k]))
        for number, (_, rows) in enumerate(sorted(found, key=lambda t: t[0])):
            labels[rows] = number
    return labels, core


@pytest.mark.parametrize("name", D.SKLEARN_CASES)
def test_oracle_equals_sklearn(name):
    c = D.case(name)
    labels, core, counts = D.expected(name)
    want_labels, want_core = sklearn_batch(c["X"], c["frame_ptr"], c["eps"], c["min_samples"], c["group"])
    assert np.array_equal(labels, want_labels)
    assert np.array_equal(np.nonzero(core)[0], np.nonzero(want_core)[0])
    ptr = c["frame_ptr"]
    for f in range(len(ptr) - 1):
        seg = labels[ptr[f]:ptr[f + 1]]
        assert counts[f] == (seg.max() + 1 if len(seg) else 0)       # dense numbering from 0 in every frame


def test_oracle_equals_sklearn_on_random_clouds():
    """The sweep the rule was stated on: blobs plus clutter, a third on a 0.5 lattice, every eps / min_samples pairing."""
    for trial in range(60):
        X = D.cloud(int(20 + 7 * trial), 1000 + trial, quantum=0.5 if trial % 3 == 0 else None)
        eps, ms = [0.5, 1.0, 1.5, 2.5][trial % 4], [1, 2, 3, 5, 8][trial % 5]
        labels, core, _ = D.dbscan_batch(X, [0, len(X)], eps, ms)
        want_labels, want_core = sklearn_frame(X, eps, ms)
        assert np.array_equal(labels, want_labels) and np.array_equal(core.astype(bool), want_core), trial


def test_windowed_pairs_equal_radius_edges():
    """Frames at the cap take their neighbour pairs through x-sorted windows: the same pairs as ``radius_edges`` on a strip large
    enough for the windowed path, ties included (a 0.5 lattice)."""
    X = np.round(D.wide_strip(D.WINDOWED_FROM + 500, 4) * 2) / 2
    i, j = D.neighbour_pairs(X, 1.0)
    E = D.go.radius_edges(X, 1.0)
    assert len(E) > len(X) and np.array_equal(i, E[:, 0]) and np.array_equal(j, E[:, 1])


# ------------------------------------------------------------------------------------------------ the inputs bite
def test_lattice_half_has_exact_ties():
    c = D.case("lattice_half")
    d2 = D.go._reduced_distances(c["X"], c["X"])
    np.fill_diagonal(d2, np.inf)
    assert (d2 == c["eps"] ** 2).sum() > 100 and (d2 == 0).sum() > 0          # ties at the radius, and coincident points


def test_lattice_tenth_has_rows_on_both_sides_of_the_tie():
    """Pairs whose exact squared distance IS eps^2 (3-4-5 steps of the 0.1 lattice) land on both sides of it in float64."""
    c = D.case("lattice_tenth")
    X = c["X"]
    k = np.rint(X * 10).astype(np.int64)
    exact = ((k[:, None, :] - k[None, :, :]) ** 2).sum(axis=2) == 25
    d2 = D.go._reduced_distances(X, X)
    inside, outside = exact & (d2 <= c["eps"] ** 2), exact & (d2 > c["eps"] ** 2)
    assert inside.sum() > 0 and outside.sum() > 0, (inside.sum(), outside.sum())


def test_a_border_point_has_core_neighbours_in_two_clusters():
    c = D.case("shared_border")
    labels, core, _ = D.expected("shared_border")
    for a, b in ((0, 7), (7, 14)):                                       # both row orders
        i, j = D.frame_pairs(c["X"][a:b], c["eps"])
        lab, co = labels[a:b], core[a:b].astype(bool)
        two = [p for p in range(b - a) if not co[p] and len(set(lab[j[(i == p) & co[j]]])) == 2]
        assert two and all(lab[p] == min(lab[j[(i == p) & co[j]]]) for p in two)


def test_a_cluster_whose_first_member_is_not_its_root():
    labels, core, _ = D.expected("shared_border")
    seg, co = labels[14:], core[14:].astype(bool)                        # border_first()
    assert seg[0] == 0 and not co[0] and co[1]


def test_chains_are_one_cluster_with_border_ends():
    for name in ("chain_row", "chain_reversed", "chain_shuffled"):
        c = D.case(name)
        labels, core, counts = D.expected(name)
        ends = np.isin(c["X"][:, 0], (c["X"][:, 0].min(), c["X"][:, 0].max()))
        assert counts.tolist() == [1] and (labels == 0).all() and np.array_equal(core == 0, ends)


def test_stars_have_border_leaves():
    labels, core, counts = D.expected("stars")
    assert core[:18].sum() == 3 and (labels[:18] >= 0).all() and core[18:].all() and counts.tolist() == [4]


def test_grouped_case_separates_what_one_group_would_join():
    c = D.case("grouped")
    labels, core, counts = D.expected("grouped")
    alone = D.dbscan_batch(c["X"], c["frame_ptr"], c["eps"], c["min_samples"])
    assert (labels[c["group"] < 0] == -1).all() and not core[c["group"] < 0].any()
    assert counts[0] > alone[2][0] or not np.array_equal(labels, alone[0])
    both = [k for k in range(counts[0]) if len(set(c["group"][:122][labels[:122] == k])) > 1]
    assert not both                                                       # no cluster holds two groups
