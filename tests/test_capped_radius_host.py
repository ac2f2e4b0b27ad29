"""Host logic of the neighbour cap (no GPU): the configuration key, its way into GraphSettings, the argument check and the
refusals of the captured / streamed steps, all of which decide before anything touches the device."""
import numpy as np
import pytest


def test_configuration_key_is_max_neighbors_under_radius_only():
    from radargnn_amd.graph_constructor.configs import GraphConstructionConfiguration as Cfg
    from radargnn_amd.preprocessor import graph_settings
    feats = (["rcs", "degree"], ["relative_position"], "directed", "X")
    capped = Cfg("radius", {"k": 20, "r": 1.5, "max_neighbors": 5}, *feats)
    shipped = Cfg("radius", {"k": 20, "r": 1.5}, *feats)                  # "k" is carried under either algorithm and ignored here
    knn = Cfg("knn", {"k": 4, "r": 1.5, "max_neighbors": 2}, *feats)
    assert (capped.max_neighbors, shipped.max_neighbors, knn.max_neighbors) == (5, None, None)
    assert (capped.k, shipped.k, knn.k) == (None, None, 4)
    s = graph_settings(capped)
    assert s.capped and s.max_neighbors == 5 and s.r == 1.5
    assert not graph_settings(shipped).capped and not graph_settings(knn).capped


def test_settings_default_to_no_cap_and_ignore_it_under_knn():
    from radargnn_amd import frames as fr
    assert fr.GraphSettings().max_neighbors is None and not fr.GraphSettings(algorithm="radius").capped
    assert fr.GraphSettings(algorithm="radius", max_neighbors=8).capped
    assert not fr.GraphSettings(algorithm="knn", k=4, max_neighbors=8).capped


@pytest.mark.parametrize("k", [0, 129, -1, 2.0, "3", None, True])
def test_cap_outside_1_to_128_or_not_an_integer_raises(k):
    from radargnn_amd import ops
    with pytest.raises(ValueError, match="neighbour cap"):
        ops.check_neighbor_cap(k)


def test_cap_accepts_python_and_numpy_integers():
    from radargnn_amd import ops
    assert [ops.check_neighbor_cap(k) for k in (1, 128, np.int32(7), np.int64(16))] == [1, 128, 7, 16]


def test_captured_and_streamed_steps_refuse_a_cap_at_construction():
    from radargnn_amd import frames as fr
    cfg = fr.GraphSettings(algorithm="radius", r=1.0, max_neighbors=6)
    with pytest.raises(ValueError, match="max_neighbors"):
        fr.HotPath(object(), cfg, use_hip_graphs=True)
    hot = fr.HotPath(object(), cfg)                                       # eager: fine
    assert hot.symmetric_graph is False
    with pytest.raises(ValueError, match="max_neighbors"):
        fr.FrameStreamer(hot)
    with pytest.raises(ValueError, match="neighbour cap"):
        fr.HotPath(object(), fr.GraphSettings(algorithm="radius", max_neighbors=0))
    assert fr.HotPath(object(), fr.GraphSettings(algorithm="radius"), use_hip_graphs=True).symmetric_graph is True
