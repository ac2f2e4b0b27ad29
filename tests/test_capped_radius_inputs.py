"""Non-vacuity of the inputs of tests/test_gpu_capped_radius.py, shown from the float64 oracle alone (tests/capped_radius_oracle.py;
no GPU): the cut of a row really falls between equal distances, the hub rows of the star batch really sit on the thresholds of
k_radius_capped_rows (csrc/graph.hip), and every (input, cap) pair has rows on both sides of the cap.  These are conditions on the
inputs, not measurements."""
import numpy as np
import pytest

import capped_radius_oracle as co
import graph_edge_inputs as gi

# thresholds of k_radius_capped_rows, restated: candidates up to RADIUS_CACHE come from the count pass's cache; a cut row beyond it
# stages up to CAPPED_LDS candidates in LDS and more in the global scratch
RADIUS_CACHE = gi.RADIUS_CACHE
CAPPED_LDS = 128


def _cut_rows(Xb, r, k):
    i, j, d2 = co.candidates(Xb, r)
    return co.cap(i, j, d2, Xb.shape[0], k)[2]


@pytest.mark.parametrize("r", [1.0, 1.5])
@pytest.mark.parametrize("k", [3, 4, 8])
@pytest.mark.parametrize("basis", ["X", "XV", "X8"])
def test_lattice_rows_are_cut_between_equal_distances(r, k, basis):
    """At least one row of the lattice is cut between two candidates of equal d2 > 0 -- on every basis the GPU test runs, with one
    exception that no lattice of this spacing can avoid: on the two-column basis at r = 1 a row holds its candidates in shells of
    4 | 4 | 4 (d2 = 0.25 | 0.5 | 1; fewer per shell at the border, never more than 8 in a row that loses a shell), so a cut
    behind the 8th candidate always falls BETWEEN two shells.  That pair is covered by the changed input: the same lattice on the
    four- and eight-column bases, whose extra columns split the shells."""
    cut = _cut_rows(gi.basis(gi.lattice(24, 0.5), basis), r, k)
    assert len(cut) and (cut[:, 1] <= cut[:, 2]).all()
    tied = (cut[:, 1] == cut[:, 2]) & (cut[:, 1] > 0)
    if (r, k, basis) == (1.0, 8, "X"):
        assert not tied.any() and set(map(tuple, cut[:, 1:])) == {(0.5, 1.0)}
    else:
        assert tied.any(), (r, k, basis, len(cut))


@pytest.mark.parametrize("k", co.CASES["coincident"][2])
def test_coincident_rows_are_cut_among_zero_distances(k):
    """The cut falls among candidates at d2 = 0: in all 60 rows of the coincident frame (59 candidates at zero: every cap here), and
    in the rows of the 40 coincident points among others for every cap below their 39."""
    r = co.CASES["coincident"][1]
    cut = _cut_rows(gi.coincident(60).X, r, k)
    assert len(cut) == 60 and (cut[:, 1:] == 0.0).all()
    if k < 39:
        cut = _cut_rows(gi.coincident_among_others().X, r, k)
        assert int(((cut[:, 1] == 0.0) & (cut[:, 2] == 0.0)).sum()) == 40


def test_star_hubs_sit_on_every_threshold_and_around_every_cap():
    frames, hubs = gi.star_batch()
    assert co.CASES["star"][1] == gi.STAR_R
    full = co.expected("star", 1)[1]
    deg = {d: int(full[row]) for d, row in hubs.items()}
    assert deg == {d: d for d in gi.STAR_DEGREES}
    for t in (RADIUS_CACHE, CAPPED_LDS, 16, 48, 128):             # the two staging thresholds, then the caps
        assert {t - 1, t, t + 1} <= set(deg.values()), t
    assert {16, 48, 128} <= set(co.CASES["star"][2])


def _classes(full, k):
    """The branch of k_radius_capped_rows a row takes: 0 empty, 1 cache uncut, 2 cache cut, 3 searched uncut, 4 cut from LDS, 5 cut
    from the global scratch."""
    cut = full > k
    return np.select([full == 0, (full <= RADIUS_CACHE) & ~cut, (full <= RADIUS_CACHE) & cut, ~cut, full <= CAPPED_LDS],
                     [0, 1, 2, 3, 4], default=5)


@pytest.mark.parametrize("name,k,basis", co.GPU_CASES)
def test_every_gpu_case_has_rows_on_both_sides_of_the_cap(name, k, basis):
    E, full, cut = co.expected(name, k, basis)
    assert (full > k).any() and ((full <= k) & (full > 0)).any(), (name, k, basis)
    assert len(cut) == int((full > k).sum())
    assert np.array_equal(np.bincount(E[:, 0], minlength=len(full)), np.minimum(full, k))


def test_the_gpu_cases_take_every_branch_of_the_fill():
    seen = set()
    for name, k, basis in co.GPU_CASES:
        seen |= set(_classes(co.expected(name, k, basis)[1], k).tolist())
    assert seen == {0, 1, 2, 3, 4, 5}
    # ... and the star batch alone takes each of them inside single blocks of the fill (16 consecutive rows per block)
    star = set()
    for k in co.CASES["star"][2]:
        cls = _classes(co.expected("star", k)[1], k)
        star |= set(cls.tolist())
        if k == 48:
            assert max(len(set(cls[b:b + 16].tolist())) for b in range(0, len(cls), 16)) >= 3
    assert {1, 2, 3, 4, 5} <= star


def test_oracle_agrees_with_the_graph_oracle_at_both_ends():
    """The capped oracle against oracle/graph_oracle.py where the two must agree: no cap in reach -> go.radius_edges; radius beyond
    the frame -> the rows of go.knn_neighbours as sets."""
    from oracle import graph_oracle as go
    f = gi.coincident_among_others()
    assert np.array_equal(co.frame_edges(f.X, 1.0, 1 << 20), go.radius_edges(f.X, 1.0))
    for k in (1, 5, 39, 40):
        E = co.frame_edges(f.X, 1e6, k)
        nbr = go.knn_neighbours(f.X, k)
        assert np.array_equal(E[:, 1].reshape(f.n, k), np.sort(nbr, axis=1))
