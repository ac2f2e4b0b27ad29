"""radargnn_amd.clustering without a device: the argument errors are raised before any device work, the scikit-learn mirror has
scikit-learn's names, and the C ABI carries the two entry points.  CPU only."""
import inspect

import numpy as np
import pytest
import torch

from radargnn_amd import clustering, ops

PTR = torch.tensor([0, 3], dtype=torch.int64)
X = np.zeros((3, 2))


@pytest.fixture(autouse=True)
def no_device_work(monkeypatch):
    """Any upload or launch fails the test: the errors below must come first."""
    def refuse(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(clustering, "_cuda", refuse)
    monkeypatch.setattr(ops, "radius_graph", refuse)
    monkeypatch.setattr(ops, "dbscan_labels", refuse)


@pytest.mark.parametrize("eps", [0, 0.0, -1.0, float("nan"), float("inf"), "1", None, True])
def test_eps_must_be_positive(eps):
    with pytest.raises(ValueError, match="eps"):
        clustering.dbscan_frames(X, PTR, eps, 3)
    with pytest.raises(ValueError, match="eps"):
        clustering.DBSCAN(eps=eps, min_samples=3).fit(X)
    with pytest.raises(ValueError, match="eps"):
        clustering.cluster_objects(X, PTR, np.zeros(3, np.int64), 5, eps, 3)


@pytest.mark.parametrize("min_samples", [0, -2, 2.0, 2.5, "3", None, True, 2 ** 31])
def test_min_samples_must_be_a_positive_integer(min_samples):
    with pytest.raises(ValueError, match="min_samples"):
        clustering.dbscan_frames(X, PTR, 1.0, min_samples)
    with pytest.raises(ValueError, match="min_samples"):
        clustering.DBSCAN(eps=1.0, min_samples=min_samples).fit_predict(X)
    with pytest.raises(ValueError, match="min_samples"):
        clustering.dbscan_graph(object(), PTR, min_samples, settings=None)


def test_numpy_integers_are_integers():
    assert clustering.check_parameters(np.float32(0.5), np.int32(4)) == (0.5, 4)


@pytest.mark.parametrize("shape", [(3, 9), (3, 0), (3,), (3, 2, 2)])
def test_basis_must_have_one_to_eight_columns(shape):
    with pytest.raises(ValueError, match="columns|2-D"):
        clustering.dbscan_frames(np.zeros(shape), PTR, 1.0, 3)
    with pytest.raises(ValueError, match="columns|2-D"):
        clustering.DBSCAN().fit(np.zeros(shape))


def test_basis_is_padded_to_the_widths_the_search_is_built_for():
    assert [clustering.check_basis_shape((5, w)) for w in range(1, 9)] == [2, 2, 4, 4, 8, 8, 8, 8]


def test_dbscan_graph_refuses_rows_that_are_no_neighbourhoods():
    from radargnn_amd.frames import GraphBatch, GraphSettings
    z = torch.zeros(1, dtype=torch.int32)

    def graph(rowptr=z):
        return GraphBatch(None, torch.zeros((2, 0), dtype=torch.int64), None, None, z, 1, rowptr=rowptr)
    with pytest.raises(ValueError, match="knn"):
        clustering.dbscan_graph(graph(None), PTR, 3, settings=GraphSettings(algorithm="knn", k=4))
    with pytest.raises(ValueError, match="knn"):
        clustering.dbscan_graph(graph(), PTR, 3, settings=GraphSettings(algorithm="knn", k=4))
    with pytest.raises(ValueError, match="uncapped"):
        clustering.dbscan_graph(graph(), PTR, 3, settings=GraphSettings(algorithm="radius", r=1.0, max_neighbors=8))
    with pytest.raises(ValueError, match="GraphSettings"):
        clustering.dbscan_graph(graph(), PTR, 3, settings=None)
    with pytest.raises(ValueError, match="rowptr"):
        clustering.dbscan_graph(graph(None), PTR, 3, settings=GraphSettings(algorithm="radius", r=1.0))
    with pytest.raises(TypeError):
        clustering.dbscan_graph(graph(), PTR, 3)


def test_dbscan_has_sklearns_names():
    import sklearn.cluster
    ours, theirs = inspect.signature(clustering.DBSCAN.__init__).parameters, inspect.signature(sklearn.cluster.DBSCAN.__init__).parameters
    assert list(ours)[:3] == list(theirs)[:3] == ["self", "eps", "min_samples"]
    assert ours["eps"].default == theirs["eps"].default == 0.5 and ours["min_samples"].default == theirs["min_samples"].default == 5
    for name in ("fit", "fit_predict"):
        assert list(inspect.signature(getattr(clustering.DBSCAN, name)).parameters)[:3] == ["self", "X", "y"]
    src = inspect.getsource(clustering.DBSCAN.fit)
    for attr in ("labels_", "core_sample_indices_", "components_"):
        assert f"self.{attr} =" in src
    est = clustering.DBSCAN(eps=2.0, min_samples=7)
    assert (est.eps, est.min_samples) == (2.0, 7) and not hasattr(est, "labels_")


def test_package_exports_the_module_and_the_abi():
    import radargnn_amd
    from radargnn_amd import _lib
    assert radargnn_amd.clustering is clustering
    assert {"rgnn_dbscan_labels", "rgnn_dbscan_max_frame_points", "rgnn_cluster_scores"} <= set(_lib.SIGNATURES)
    assert ops.dbscan_max_frame_points() == 24 * 1024
    assert (ops.STATUS_DBSCAN_FRAME_TOO_LARGE, ops.STATUS_DBSCAN_BAD_ROW) == (2048, 4096)
    header = open(__import__("os").path.join(__import__("os").path.dirname(radargnn_amd.__path__[0]), "include", "rgnn.h")).read()
    assert "#define RGNN_STATUS_DBSCAN_FRAME_TOO_LARGE 2048" in header and "#define RGNN_STATUS_DBSCAN_BAD_ROW 4096" in header


def test_ops_refuse_cpu_tensors():
    z = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cluster_scores(torch.zeros((3, 2)), torch.zeros(1, dtype=torch.int64), z, 0)
