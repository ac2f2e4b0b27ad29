"""Batched DBSCAN on the device (csrc/cluster.hip through ops.dbscan_labels / radargnn_amd.clustering) against the numpy oracle
(tests/dbscan_oracle.py, itself checked against scikit-learn's kd_tree DBSCAN in tests/test_dbscan_oracle.py).  Labels, core flags
and cluster counts are integers: everything is compared with ``np.array_equal``, there is no tolerance anywhere."""
import numpy as np
import pytest
import torch

import dbscan_oracle as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radargnn_amd import clustering
    return clustering


def run(C, c, check=True):
    group = None if c["group"] is None else torch.tensor(c["group"])            # (copies: the cases are read-only arrays)
    return C.dbscan_frames(torch.tensor(c["X"]), torch.tensor(c["frame_ptr"]), c["eps"], c["min_samples"], group, check=check)


def host(out):
    return out.labels.cpu().numpy(), out.core.cpu().numpy(), out.num_clusters.cpu().numpy()


def assert_equal(got, want, what=""):
    for g, w, name in zip(got, want, ("labels", "core", "n_clusters")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        diff = np.nonzero(g != w)[0]
        assert np.array_equal(g, w), (what, name, len(diff), diff[:8], g[diff[:8]], w[diff[:8]])


def test_cap_is_the_oracles():
    from radargnn_amd import ops
    assert ops.dbscan_max_frame_points() == D.CAP


@pytest.mark.parametrize("name", list(D.CASES))
def test_labels_equal_the_oracle(C, name):
    """Frame sizes 0 / 1 / 2 / 63-65 / 1023-1025, a frame at the cap, chains (deepest trees) in three row orders and at the cap, stars,
    lattices with ties, coincident points, shared border points, min_samples 1 and 10^6, bases of 2 / 3 / 4 / 8 columns, 70 frames
    with empty ones, groups with -1 rows and interleaved classes."""
    out = run(C, D.case(name))
    assert int(out.status.item()) == 0
    assert_equal(host(out), D.expected(name), name)


def test_numbering_restarts_in_every_frame(C):
    c = D.case("many_frames")
    labels, _, counts = host(run(C, c))
    ptr = c["frame_ptr"]
    sizes = np.diff(ptr)
    assert (sizes == 0).sum() >= 10 and (counts[sizes == 0] == 0).all() and (counts > 1).sum() >= 10
    for f in range(len(ptr) - 1):
        seg = labels[ptr[f]:ptr[f + 1]]
        assert sorted(set(seg[seg >= 0])) == list(range(counts[f]))


def test_frame_above_the_cap_is_refused_and_the_others_are_right(C):
    from radargnn_amd import ops
    c = D.case("cap")
    ptr, X = c["frame_ptr"], c["X"]
    extra = np.array([[1e6, 1e6]])                                       # one more point in the large frame, far from everything
    X1 = np.concatenate((X[:ptr[2]], extra, X[ptr[2]:]))
    ptr1 = ptr + np.array([0, 0, 1, 1])
    c1 = dict(c, X=X1, frame_ptr=ptr1)
    with pytest.raises(ValueError, match=str(D.CAP)):
        run(C, c1)
    out = run(C, c1, check=False)
    assert int(out.status.item()) == ops.STATUS_DBSCAN_FRAME_TOO_LARGE
    with pytest.raises(ValueError, match=str(D.CAP)):
        out.check()
    labels, core, counts = host(out)
    want = D.expected("cap")
    big = slice(ptr1[1], ptr1[2])
    assert (labels[big] == -1).all() and (core[big] == 0).all() and counts[1] == 0
    for f, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        if f != 1:
            a1, b1 = ptr1[f], ptr1[f + 1]
            assert np.array_equal(labels[a1:b1], want[0][a:b]) and np.array_equal(core[a1:b1], want[1][a:b]) and counts[f] == want[2][f]


def test_same_call_twice_gives_the_same_bits(C):
    for name in ("chain_shuffled", "lattice_half", "grouped"):
        a, b = host(run(C, D.case(name))), host(run(C, D.case(name)))
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name


def _labels_from_csr(rowptr, col, ptr, min_samples):
    """ops.dbscan_labels on a hand-built CSR -> [labels, core, n_clusters, status] on the host."""
    from radargnn_amd import ops
    out = ops.dbscan_labels(torch.tensor(rowptr).cuda(), torch.tensor(col).cuda(), torch.tensor(ptr).cuda(), min_samples)
    return [t.cpu().numpy() for t in out]


def test_out_of_frame_entries_are_skipped_and_flagged(C):
    """Frame 0's first row lists a row of frame 1, frame 1's last row lists -7 and a row past the end: the status bit is raised, the
    entries are skipped (the labels are those of the rows without them) and nothing is indexed with them."""
    from radargnn_amd import ops
    c = D.case("shared_border")
    X, ptr = c["X"], c["frame_ptr"]
    rowptr, col = D.csr(X, ptr, c["eps"])
    n = len(X)
    rows = [list(col[rowptr[i]:rowptr[i + 1]]) for i in range(n)]
    rows[0] = [int(ptr[1]) + 2] + rows[0]
    rows[int(ptr[2]) - 1] = rows[int(ptr[2]) - 1] + [-7, n + 1000, 2 ** 31 - 1]
    bad_rowptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
    bad_col = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows])
    labels, core, counts, status = _labels_from_csr(bad_rowptr, bad_col, ptr, c["min_samples"])
    assert int(status[0]) == ops.STATUS_DBSCAN_BAD_ROW
    assert_equal((labels, core, counts), D.expected("shared_border"))
    clean = _labels_from_csr(rowptr, col, ptr, c["min_samples"])
    assert int(clean[3][0]) == 0
    assert_equal(clean[:3], D.expected("shared_border"))
    # a row whose offsets leave the edge list is an empty row, not a read
    broken = rowptr.copy()
    broken[3] = 10 ** 9
    labels, core, counts, status = _labels_from_csr(broken, col, ptr, c["min_samples"])
    assert int(status[0]) == ops.STATUS_DBSCAN_BAD_ROW and labels.min() >= -1 and labels.max() < n


def test_dbscan_graph_equals_dbscan_frames(C):
    """The radius graph HotPath builds for the model carries the same neighbourhoods: no second search."""
    from radargnn_amd import frames, gnn, synthetic
    fr = [synthetic.nuscenes_frame(i) for i in range(4)]
    settings = frames.GraphSettings(algorithm="radius", r=2.0, node_features=("rcs", "velocity_vector", "time_index", "degree"))
    cfg = gnn.GNNArchitectureConfig(5, 2, [64, 32], [6], [16, 5], True, True, [32, 64], [4, 8, 16], "MPNNConv", False)
    torch.manual_seed(0)
    model = gnn.DetNetBasic(cfg).cuda()
    batch = frames.FrameBatch.from_frames(fr)
    _, _, g = frames.HotPath(model, settings)(batch)
    g.check()
    got = C.dbscan_graph(g, batch.frame_ptr, 4, settings=settings)
    want = C.dbscan_frames(batch.X, batch.frame_ptr, 2.0, 4)
    assert int(want.num_clusters.sum()) > 4
    assert_equal(host(got), host(want))
    X = batch.X.cpu().numpy()
    assert_equal(host(got), D.dbscan_batch(X, batch.frame_ptr.cpu().numpy(), 2.0, 4))
    capped = frames.GraphSettings(algorithm="radius", r=2.0, max_neighbors=4)
    with pytest.raises(ValueError, match="uncapped"):
        C.dbscan_graph(frames.build_graphs(batch, capped), batch.frame_ptr, 4, settings=capped)
    knn = frames.GraphSettings(algorithm="knn", k=5)
    with pytest.raises(ValueError, match="knn"):
        C.dbscan_graph(frames.build_graphs(batch, knn), batch.frame_ptr, 4, settings=knn)


def test_sklearn_mirror(C):
    X = np.asarray(D.case("lattice_half")["X"])
    est = C.DBSCAN(eps=0.5, min_samples=3).fit(X)
    labels, core, _ = D.expected("lattice_half")
    assert est.labels_.dtype == np.int64 and np.array_equal(est.labels_, labels)
    assert np.array_equal(est.core_sample_indices_, np.nonzero(core)[0])
    assert np.array_equal(est.components_, X[core.astype(bool)])
    assert np.array_equal(C.DBSCAN(eps=0.5, min_samples=3).fit_predict(X), labels)
    empty = C.DBSCAN().fit(np.zeros((0, 2)))
    assert empty.labels_.shape == (0,) and empty.components_.shape == (0, 2)
