"""The reference's own tests for the graph constructor (test/test_graph_constructor.py) and its call site
(test/test_preprocessor.py:207-257), run against the HIP-backed mirror classes -- same inputs, same expected values --
plus the batched on-device pipeline (radargnn_amd.frames) against the oracle."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import gnn_oracle as G
from oracle import graph_oracle as go
from radargnn_amd import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gr():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    import gnnradarobjectdetection.graph_constructor.features as ft
    import gnnradarobjectdetection.graph_constructor.graph as g
    return g, ft


def test_point_pair_features(gr):
    _, ft = gr                                                   # test_graph_constructor.py:6-17
    p1, p2 = np.array([1, 1]).reshape(2, 1), np.array([3, 2]).reshape(2, 1)
    v1, v2 = np.array([0, 1]).reshape(2, 1), np.array([1, 0]).reshape(2, 1)
    d, a, b, c = ft.get_En_equivariant_point_pair_metrics(p1, p2, v1, v2, "directed")
    assert [round(d, 2), round(a, 2), round(b, 2), round(c, 2)] == [2.24, 90.0, 63.43, 26.57]
    v2 = np.array([0, 0]).reshape(2, 1)                          # :20-31 zero velocity -> 90 degrees
    d, a, b, c = ft.get_En_equivariant_point_pair_metrics(p1, p2, v1, v2, "directed")
    assert [round(d, 2), round(a, 2), round(b, 2), round(c, 2)] == [2.24, 90.0, 63.43, 90.0]


def test_edge_features(gr):
    g, _ = gr                                                    # test_graph_constructor.py:34-59
    graph = g.GeometricGraph()
    graph.X = np.array([[1, 1], [3, 2]])
    graph.V = np.array([[0, 1], [1, 0]])
    graph.F = {"rcs": np.array([0, 1]).reshape(2, 1)}
    graph.build(graph.X, "knn", k=1)
    graph.extract_node_pair_features(["point_pair_features", "spatial_euclidean_distance", "velocity_euclidean_distance",
                                      "relative_position", "relative_velocity"], "directed")
    assert [2.24, 90, 63.43, 26.57, 2.24, 1.41, -2, -1, -1, 1] == np.round(graph.E_feat[0, :], 2).tolist()
    assert graph.E.dtype == np.int32 and graph.E.tolist() == [[0, 1], [1, 0]]
    with pytest.raises(Exception, match="Invalid feature specified"):
        graph.extract_node_pair_features(["nope"], "directed")


def test_node_features_and_degree(gr):
    g, _ = gr                                                    # test_graph_constructor.py:62-103
    graph = g.GeometricGraph()
    graph.X = np.array([[1, 1], [3, 2]])
    graph.V = np.array([[0, 1], [1, 0]])
    graph.F = {"rcs": np.array([1.8, 2.6]).reshape(2, 1), "time_index": np.array([100, 101]).reshape(2, 1)}
    graph.build(graph.X, "knn", k=1)
    graph.extract_single_node_features(["rcs", "time_index", "degree", "velocity_vector_length", "velocity_vector",
                                        "spatial_coordinates"])
    assert [2.6, 101, 1, 1, 1, 0, 3, 2] == graph.X_feat[1, :].tolist()
    graph2 = g.GeometricGraph()
    graph2.build(np.array([[1, 1], [3, 2]]), "knn", k=1)
    graph2.add_degree_to_inv_features()
    graph2.add_degree_to_inv_features()
    assert np.sum(graph2.F.get("degree") == np.array([[1, 1], [1, 1]])) == 4
    assert graph2.A.tolist() == [[0.0, 1.0], [1.0, 0.0]]          # dense adjacency on demand


def test_add_node_feature(gr):
    g, _ = gr                                                    # test_graph_constructor.py:106-122
    rcs = np.array([-1, -2]).reshape(2, 1)
    graph = g.GeometricGraph()
    graph.X = np.array([[1, 1], [3, 2]])
    graph.F = {"rcs": rcs}
    graph.build(graph.X, "knn", k=1)
    graph.add_node_features(rcs)
    graph.extract_single_node_features(["rcs"])
    graph.add_node_features(rcs)
    assert (graph.X_feat[0, :] == [-1, -1, -1]).all()


def test_build_geometric_graph_call_site(gr):
    from radargnn_amd.graph_constructor import GraphConstructionConfiguration, build_geometric_graph, create_graph_tensors
    pc = SimpleNamespace(X_cc=np.array([[1, 1], [3, 2], [5, 8]]).reshape(3, 2), rcs=np.zeros((3, 1)),
                         timestamp=np.array([100, 101, 102]).reshape(3, 1))
    pc.V_cc_compensated = np.ones_like(pc.X_cc)                  # test_preprocessor.py:207-230
    cfg = GraphConstructionConfiguration("knn", {"k": 1, "r": 1}, ["spatial_coordinates", "time_index"],
                                         ["spatial_euclidean_distance"], "directed", "X")
    graph = build_geometric_graph(cfg, pc)
    assert (graph.E_feat[0, :] == 5 ** 0.5).all() and (graph.X_feat[1, :] == np.array([3, 2, 1])).all()
    assert (graph.E == np.array([[0, 1], [1, 0], [2, 1]])).all()
    t = create_graph_tensors(graph, pc)
    assert t["edge_index"].dtype == torch.long and t["edge_index"].shape == (2, 3) and t["x"].dtype == torch.float32
    pc2 = SimpleNamespace(X_cc=np.array([[1, 1], [2, 2], [10, 10]]).reshape(3, 2), rcs=np.zeros((3, 1)),
                          timestamp=np.zeros((3, 1)))
    pc2.V_cc_compensated = np.ones_like(pc2.X_cc)                # test_preprocessor.py:233-257
    pc2.V_cc_compensated[0, :] = 100
    e_x = build_geometric_graph(GraphConstructionConfiguration("knn", {"k": 1, "r": 1}, ["spatial_coordinates"],
                                ["spatial_euclidean_distance"], "directed", "X"), pc2).E
    e_xv = build_geometric_graph(GraphConstructionConfiguration("knn", {"k": 1, "r": 1}, ["spatial_coordinates"],
                                 ["spatial_euclidean_distance"], "directed", "XV"), pc2).E
    assert (e_x == np.array([[0, 1], [1, 0], [2, 1]])).all() and (e_xv == np.array([[0, 1], [1, 2], [2, 1]])).all()


def test_knn_with_too_many_neighbours_raises_like_sklearn(gr):
    g, _ = gr
    graph = g.GeometricGraph()
    with pytest.raises(ValueError, match="Expected n_neighbors < n_samples_fit"):
        graph.build(np.random.rand(5, 2), "knn", k=5)


@pytest.mark.parametrize("width", [1, 3, 5, 6, 8])
@pytest.mark.parametrize("routine,k,r", [("knn", 4, 1.0), ("radius", 6, 0.8)])
def test_distance_basis_of_any_width_up_to_eight(gr, width, routine, k, r):
    """graph.py:45-50,57-58: the reference measures distances over ALL columns it is handed.  Widths other than 2 / 4 / 8 run on the
    next compiled kernel behind zero columns (exact: + 0.0 per padded dimension); edges equal the KD-tree-faithful oracle's on the
    unpadded basis.  Bases wider than 8 columns are refused with a message, not searched on a prefix."""
    Graph = gr[0].Graph
    rng = np.random.default_rng(5)
    scale = 2.0 if width <= 3 else 0.6                            # (more dimensions: points move apart; keep some inside the radius)
    X = np.round(rng.normal(size=(200, width)) * scale, 2)         # (rounded: equal distances do occur)
    g = Graph()
    g.build(X, routine, k=k, r=r)
    exp = go.build_edges(np.ascontiguousarray(X, dtype=np.float64), routine, k=k, r=r)
    assert len(exp) > 0
    assert np.array_equal(go.canonical_edges(g.E), go.canonical_edges(exp))
    with pytest.raises(ValueError, match="1 to 8 columns"):
        Graph().build(rng.normal(size=(50, 9)), routine, k=k, r=r)


def test_geometric_graph_matches_reference_golden_on_3000_points(gr):
    import os
    from conftest import GOLDEN
    g, _ = gr
    d = np.load(os.path.join(GOLDEN, "rs3000_knn_k20_r1.npz"))
    graph = g.GeometricGraph()
    graph.X, graph.V = d["X"], d["V"]
    graph.F = {"rcs": d["rcs"], "time_index": d["time_index"].reshape(-1, 1)}
    graph.build(d["X"], "knn", k=20)
    graph.extract_node_pair_features(["relative_position"], "directed")
    graph.extract_single_node_features(["rcs", "velocity_vector", "time_index", "degree"])
    assert np.array_equal(graph.E, d["E"])
    assert np.array_equal(graph.X_feat.astype(np.float32), d["X_feat"])
    assert np.array_equal(graph.E_feat.astype(np.float32), d["E_feat"])


@pytest.mark.parametrize("name", ["small_n6_s0_knn_k1_r1_directed_X", "small_n40_s2_knn_k1_r1_directed_X",
                                  "small_n40_s2_knn_k1_r1_directed_XV", "small_n300_s3_knn_k1_r1_directed_X"])
def test_nearest_neighbor_points_matches_the_reference_k1_fixtures(name):
    """X[np.where(kneighbors_graph(X, 1).toarray() == 1)[1]] at dataset_creation.py:316-318 and
    postprocessing.py:233-237,469; the k = 1 fixtures were produced by the reference's own Graph.build."""
    import os
    from conftest import GOLDEN
    from radargnn_amd.graph_constructor import nearest_neighbor_index, nearest_neighbor_points
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    basis = d["X"] if name.endswith("_X") else np.concatenate((d["X"], d["V"]), axis=1)
    E = d["E"]
    assert np.array_equal(E[:, 0], np.arange(basis.shape[0]))            # one neighbour per point, rows ascending
    assert np.array_equal(nearest_neighbor_index(basis), E[:, 1])
    assert np.array_equal(nearest_neighbor_points(basis), basis[E[:, 1]])
    with pytest.raises(ValueError, match="Expected n_neighbors < n_samples_fit"):
        nearest_neighbor_index(basis[:1])


@pytest.mark.parametrize("algo", ["knn", "radius"])
def test_hot_path_batch_vs_oracle_and_hip_graph_replay(algo):
    """64-frame batch through radargnn_amd.frames: topology / features bit-exact vs the oracle's collated graphs,
    logits within 1e-5 (norm-wise) of the float64 oracle, and HIP-graph replay bit-identical to eager launches."""
    from radargnn_amd import frames as fr, gnn
    frames = [synthetic.nuscenes_frame(i) for i in range(16)] + [synthetic.radarscenes_frame(i) for i in range(2)]
    cfg = fr.GraphSettings(algorithm=algo, k=10, r=2.0)
    mcfg = gnn.GNNArchitectureConfig(5, 2, [64, 64, 32], [11], [16, 5], True, True, [32, 64], [4, 8, 16], "MPNNConv", False)
    torch.manual_seed(3)
    model = gnn.DetNetBasic(mcfg)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.cuda()
    batch = fr.FrameBatch.from_frames(frames)
    cls, bb, g = fr.HotPath(model, cfg)(batch)
    g.check()
    ref = go.collate([go.build_frame_graph(f.X, f.V, f.rcs, f.timestamp, algo, 10, 2.0, list(cfg.node_features),
                                           list(cfg.edge_features), "directed") for f in frames])
    assert np.array_equal(g.edge_index.cpu().numpy(), ref["edge_index"])
    assert np.array_equal(g.x.cpu().numpy(), ref["x"])
    np.testing.assert_allclose(g.edge_attr.cpu().numpy(), ref["edge_attr"], rtol=2e-7, atol=1e-6)
    c64, b64 = G.det_net_basic(torch.from_numpy(ref["x"]), torch.from_numpy(ref["edge_index"]),
                               torch.from_numpy(ref["edge_attr"]), sd, dtype=torch.float64)
    assert ((cls.double().cpu() - c64).abs().max() / c64.abs().max()).item() < 1e-5
    assert ((bb.double().cpu() - b64).abs().max() / b64.abs().max()).item() < 1e-5
    model.eval()                                                  # replay vs eager needs a stateless forward
    e_c, e_b, _ = fr.HotPath(model, cfg)(batch)
    hot = fr.HotPath(model, cfg, use_hip_graphs=True)
    for _ in range(4):
        r_c, r_b, r_g = hot(batch)
    torch.cuda.synchronize()
    assert torch.equal(r_c, e_c) and torch.equal(r_b, e_b) and torch.equal(r_g.edge_index, g.edge_index)


def test_hot_path_c2_bench_path_vs_oracle():
    """The exact code path bench.py times, at its own shape but on 8 frames: HotPath on RadarScenes-shaped frames, radius
    graph r = 1.0 (symmetric edge set: row-split update, source-term GEMM on the rows with edges only, edge kernel without
    the rows of isolated targets), grid-cell visiting order, the 224-wide 4-layer C2 model (LDS-DMA bf16x3 dense layers on
    row subsets) -- against the float64 oracle on the oracle's own graphs."""
    import bench
    from radargnn_amd import frames as fr
    frames = [synthetic.radarscenes_frame(i) for i in range(8)]
    cfg = bench.c2_settings()
    torch.manual_seed(0)
    model = bench.c2_model()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.cuda()
    batch = fr.FrameBatch.from_frames(frames)
    cls, bb, g = fr.HotPath(model, cfg)(batch)
    g.check()
    ref = go.collate([go.build_frame_graph(f.X, f.V, f.rcs, f.timestamp, "radius", None, 1.0, list(cfg.node_features),
                                           list(cfg.edge_features), "directed") for f in frames])
    assert np.array_equal(g.edge_index.cpu().numpy(), ref["edge_index"])
    assert np.array_equal(g.x.cpu().numpy(), ref["x"])
    deg = np.bincount(ref["edge_index"][1], minlength=ref["x"].shape[0])
    assert 0.1 < (deg == 0).mean() < 0.9                          # both row groups of the split update are exercised
    c64, b64 = G.det_net_basic(torch.from_numpy(ref["x"]), torch.from_numpy(ref["edge_index"]),
                               torch.from_numpy(ref["edge_attr"]), sd, dtype=torch.float64)
    assert ((cls.double().cpu() - c64).abs().max() / c64.abs().max()).item() < 1e-5
    assert ((bb.double().cpu() - b64).abs().max() / b64.abs().max()).item() < 1e-5


def test_c2_whole_step_hip_graph_in_training_mode_vs_oracle_and_eager():
    """What bench.py times, as it times it: the C2 model in TRAINING mode (batch statistics in every BatchNorm -- the reference
    never calls .eval(), postprocessor/inference.py:57-58) with the whole step replayed from ONE HIP graph, on 8 C2 frames:
    after >= 4 replays the logits / boxes are within 1e-5 (norm-wise) of the float64 oracle on the oracle's own graphs and
    bit-equal to the eager pass (train-mode outputs do not depend on the running statistics the replays keep updating)."""
    import bench
    from radargnn_amd import frames as fr, ops
    frames = [synthetic.radarscenes_frame(i) for i in range(8)]
    cfg = bench.c2_settings()
    model = bench.c2_model()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.cuda().train()
    batch = fr.FrameBatch.from_frames(frames)
    e_c, e_b, e_g = fr.HotPath(model, cfg)(batch)
    e_g.check()
    e_c, e_b = e_c.clone(), e_b.clone()
    hot = fr.HotPath(model, cfg, use_hip_graphs=True)
    before = ops.COUNTERS.get("f16x2", 0)
    for _ in range(6):                                          # first sight eager, then capture + 5 replays
        r_c, r_b, r_g = hot(batch)
    torch.cuda.synchronize()
    assert hot._graph is not None, "the step was not captured"
    assert ops.COUNTERS.get("f16x2", 0) > before                # the dense layers ran in the form bench.py times
    r_g.check()
    assert torch.equal(r_c, e_c) and torch.equal(r_b, e_b) and torch.equal(r_g.edge_index, e_g.edge_index)
    ref = go.collate([go.build_frame_graph(f.X, f.V, f.rcs, f.timestamp, "radius", None, 1.0, list(cfg.node_features),
                                           list(cfg.edge_features), "directed") for f in frames])
    assert np.array_equal(r_g.edge_index.cpu().numpy(), ref["edge_index"])
    c64, b64 = G.det_net_basic(torch.from_numpy(ref["x"]), torch.from_numpy(ref["edge_index"]),
                               torch.from_numpy(ref["edge_attr"]), sd, dtype=torch.float64)
    assert ((r_c.double().cpu() - c64).abs().max() / c64.abs().max()).item() < 1e-5
    assert ((r_b.double().cpu() - b64).abs().max() / b64.abs().max()).item() < 1e-5
    assert int(model.batch_norms[0].module.num_batches_tracked.item()) == 7        # one eager reference + 6 steps


def test_hip_graph_replay_follows_in_place_weight_updates():
    """A captured step bakes in the folded weights / bf16 planes cached by the eager pass; after an optimizer-style in-place
    update the graph must be re-captured, not replayed with the old folds beside the new parameters."""
    from radargnn_amd import frames as fr, gnn
    frames = [synthetic.nuscenes_frame(i) for i in range(12)]
    cfg = fr.GraphSettings(algorithm="radius", r=6.0)
    mcfg = gnn.GNNArchitectureConfig(5, 2, [96, 64], [6], [16, 5], True, True, [32, 96], [4, 8, 16], "MPNNConv", False)
    torch.manual_seed(5)
    model = gnn.DetNetBasic(mcfg).cuda().eval()
    batch = fr.FrameBatch.from_frames(frames)
    hot = fr.HotPath(model, cfg, use_hip_graphs=True)
    for _ in range(3):
        hot(batch)
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1.25).add_(0.01)
    for _ in range(2):
        r_c, r_b, _ = hot(batch)
    torch.cuda.synchronize()
    e_c, e_b, _ = fr.HotPath(model, cfg)(batch)
    assert torch.equal(r_c, e_c) and torch.equal(r_b, e_b)


@pytest.mark.parametrize("algo", ["knn", "radius"])
def test_hip_graph_replay_is_stable_over_many_steps(algo):
    """One captured graph per step (search included), replayed back to back with host reads in between: the pattern that
    faulted on this runtime when the search stage ran eagerly in front of a replayed model (frames.HotPath docstring)."""
    from radargnn_amd import frames as fr, gnn
    frames = [synthetic.radarscenes_frame(i) for i in range(2)]
    cfg = fr.GraphSettings(algorithm=algo, k=10, r=1.5)
    mcfg = gnn.GNNArchitectureConfig(5, 2, [64, 32], [6], [16, 5], True, True, [32, 64], [4, 8, 16], "MPNNConv", False)
    torch.manual_seed(8)
    model = gnn.DetNetBasic(mcfg).cuda().eval()
    batch = fr.FrameBatch.from_frames(frames)
    e_c, e_b, e_g = fr.HotPath(model, cfg)(batch)
    hot = fr.HotPath(model, cfg, use_hip_graphs=True)
    for it in range(80):
        c, b, g = hot(batch)
        if it % 9 == 0:
            g.check()                                                     # host read of the status word between replays
            assert torch.equal(c, e_c) and torch.equal(b, e_b) and torch.equal(g.edge_index, e_g.edge_index)
    torch.cuda.synchronize()


def test_hip_graph_replay_guards_the_edge_count_of_a_radius_graph():
    """The captured step of a radius graph is sized for the edge count the eager pass found.  Points modified IN PLACE so
    that the count changes: the fill (rgnn_radius_graph_rows_direct since r06: every row is compared with its committed length)
    must notice on the device and flag it -- check() raises -- instead of writing past the captured buffers; data put back, the
    replay is valid again."""
    from radargnn_amd import frames as fr, gnn, ops
    frames = [synthetic.nuscenes_frame(i) for i in range(8)]
    cfg = fr.GraphSettings(algorithm="radius", r=4.0)
    mcfg = gnn.GNNArchitectureConfig(5, 2, [64, 32], [6], [16, 5], True, True, [32, 64], [4, 8, 16], "MPNNConv", False)
    torch.manual_seed(6)
    model = gnn.DetNetBasic(mcfg).cuda().eval()
    batch = fr.FrameBatch.from_frames(frames)
    hot = fr.HotPath(model, cfg, use_hip_graphs=True)
    for _ in range(3):
        c0, b0, g0 = hot(batch)
    g0.check()
    ref_c, ref_ei = c0.clone(), g0.edge_index.clone()
    saved = batch.X.clone()
    batch.X.mul_(0.5)                                            # twice as dense: more pairs within r
    c1, _, g1 = hot(batch)
    torch.cuda.synchronize()
    assert int(g1.status.item()) & ops.STATUS_EDGE_COUNT_CHANGED
    with pytest.raises(RuntimeError, match="changed under a captured HIP graph"):
        g1.check()
    # (r06, rgnn_radius_graph_rows_direct: rows that still have their committed length are rewritten, the others keep their
    #  contents -- a flagged replay's graph arrays are a mixture, in bounds, and invalid as a whole: check() raised above)
    n_pts = batch.num_points
    assert g1.edge_index.shape == ref_ei.shape and int(g1.edge_index.min()) >= 0 and int(g1.edge_index.max()) < n_pts
    assert torch.equal(g1.edge_index[0], ref_ei[0])              # the rows themselves (committed rowptr) never move
    batch.X.copy_(saved)
    c2, _, g2 = hot(batch)
    g2.check()
    assert torch.equal(c2, ref_c) and torch.equal(g2.edge_index, ref_ei)


def test_hip_graph_replay_on_modified_points_computes_on_the_previous_rows():
    """the replayed search rewrites the rows of the static CSR; everything downstream of the checked fill (CSR by
    target, chunk table, edge kernels) is sized for the captured edge count and must not walk the new rows.  They read the rows
    of the last replay that matched (rgnn_radius_rows_commit): with three times the edges the replay stays inside its
    buffers, flags the change and leaves the graph arrays of the previous step in place -- also when the capture had no edge
    at all."""
    from radargnn_amd import frames as fr, gnn, ops
    mcfg = gnn.GNNArchitectureConfig(5, 2, [64, 32], [6], [16, 5], True, True, [32, 64], [4, 8, 16], "MPNNConv", False)
    torch.manual_seed(6)
    model = gnn.DetNetBasic(mcfg).cuda().eval()
    for r, shrink in ((4.0, 0.3), (1e-3, 1e-5)):                # (second case: no pair within 1 mm -> a capture with E = 0)
        frames = [synthetic.nuscenes_frame(i) for i in range(8)]
        batch = fr.FrameBatch.from_frames(frames)
        hot = fr.HotPath(model, fr.GraphSettings(algorithm="radius", r=r), use_hip_graphs=True)
        for _ in range(3):
            c0, b0, g0 = hot(batch)
        g0.check()
        e0 = g0.edge_index.shape[1]
        assert (e0 == 0) == (r < 1.0)
        ref_c, ref_ei, ref_rows = c0.clone(), g0.edge_index.clone(), g0.rowptr.clone()
        saved = batch.X.clone()
        batch.X.mul_(shrink)                                     # far denser: many times the pairs within r
        for _ in range(3):
            c1, _, g1 = hot(batch)
        torch.cuda.synchronize()
        assert int(g1.status.item()) & ops.STATUS_EDGE_COUNT_CHANGED
        with pytest.raises(RuntimeError, match="changed under a captured HIP graph"):
            g1.check()
        # the committed rows stay; the edge list stays inside its buffers and names existing nodes (r06: rows that kept their length
        # are rewritten by the one-launch search + fill, a flagged replay's arrays are invalid as a whole)
        assert torch.equal(g1.rowptr, ref_rows) and g1.edge_index.shape == ref_ei.shape
        if e0:
            assert int(g1.edge_index.min()) >= 0 and int(g1.edge_index.max()) < batch.num_points
            assert torch.equal(g1.edge_index[0], ref_ei[0])
        assert torch.isfinite(c1).all()
        batch.X.copy_(saved)
        c2, _, g2 = hot(batch)
        g2.check()
        assert torch.equal(c2, ref_c) and torch.equal(g2.edge_index, ref_ei)


def test_splitk_timeout_counter_is_reported_by_check():
    """A dense launch that gives up waiting for another work-group's partial tile counts it in the scratch's time-out word
    (rgnn.h RGNN_SPLITK_TIMEOUT_WORD); GraphBatch.check() reads it and raises.  Healthy runs leave it at zero."""
    from radargnn_amd import frames as fr, gnn, ops
    mcfg = gnn.GNNArchitectureConfig(5, 2, [96, 64], [6], [16, 5], True, True, [32, 96], [4, 8, 16], "MPNNConv", False)
    torch.manual_seed(2)
    model = gnn.DetNetBasic(mcfg).cuda()
    batch = fr.FrameBatch.from_frames([synthetic.radarscenes_frame(i) for i in range(2)])
    _, _, g = fr.HotPath(model, fr.GraphSettings(algorithm="knn", k=10))(batch)
    g.check()
    assert ops.splitk_timeouts("cuda") == 0 and ops._SPLITK_WS, "one-frame dense layers use the split-K scratch"
    ws = next(iter(ops._SPLITK_WS.values()))
    word = ws[ws.numel() - 4096 + 4 * ops.SPLITK_TIMEOUT_WORD:][:4].view(torch.int32)
    word.fill_(1)                                                # what linear_dma.hip does when its bounded spin runs out
    try:
        with pytest.raises(RuntimeError, match="time-out"):
            g.check()
    finally:
        word.zero_()
    g.check()


def test_hot_path_knn_frame_too_small_raises():
    from radargnn_amd import frames as fr, gnn
    batch = fr.FrameBatch.from_frames([synthetic.small_frame(6, 0), synthetic.nuscenes_frame(0)])
    with pytest.raises(ValueError, match="Expected n_neighbors < n_samples_fit"):
        fr.build_graphs(batch, fr.GraphSettings(algorithm="knn", k=10))


@pytest.mark.parametrize("pre,post,conv,aggr,bn", [(1, 1, "MPNNConv", "max", False), (2, 2, "MPNNConv", "max", False),
                                                    (2, 1, "MPNNConv", "mean", True), (1, 2, "RadarPointGNNConv", "add", True)])
def test_a_graph_without_edges_runs_through_every_layer_variant(pre, post, conv, aggr, bn):
    """Three points farther apart than the radius: E = 0.  Every architecture variant (deeper message / update MLPs go through
    rgnn_mpnn_edge_hidden + rgnn_segment_reduce, BatchNorm inside the edge MLP sees zero rows) must give what the oracle gives."""
    from radargnn_amd import frames as fr, gnn
    X = np.array([[0.0, 0.0], [10.0, 0.0], [0.0, 10.0]]); V = np.array([[1.0, 0.0], [0.0, 1.0], [0.5, 0.5]])
    frame = synthetic.RadarFrame(X, V, np.array([[1.0], [2.0], [3.0]]), np.array([[0.0], [0.0], [0.1]]))
    cfg = fr.GraphSettings(algorithm="radius", r=1.0)
    widths = [32, 32] if conv == "RadarPointGNNConv" else [48, 32]
    mcfg = gnn.GNNArchitectureConfig(5, 2, widths, [6], [16, 5], True, True, [16, 32], [4, 8], conv, bn, pre, post, False, aggr)
    torch.manual_seed(0)
    model = gnn.DetNetBasic(mcfg)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.cuda()
    cls, bb, g = fr.HotPath(model, cfg)(fr.FrameBatch.from_frames([frame]))
    g.check()
    assert g.edge_index.shape == (2, 0)
    ref = go.build_frame_graph(frame.X, frame.V, frame.rcs, frame.timestamp, "radius", None, 1.0, list(cfg.node_features),
                               list(cfg.edge_features), "directed")
    c64, b64 = G.det_net_basic(torch.from_numpy(ref["x"]), torch.from_numpy(ref["edge_index"]), torch.from_numpy(ref["edge_attr"]), sd,
                               conv_layer_type=conv, aggr=aggr, dtype=torch.float64)
    assert torch.isfinite(cls).all() and torch.isfinite(bb).all()
    assert ((cls.double().cpu() - c64).abs().max() / c64.abs().max()).item() < 1e-3      # (BatchNorm over three rows)
    assert ((bb.double().cpu() - b64).abs().max() / b64.abs().max()).item() < 1e-3


def test_whole_module_pickle_round_trip_after_inference_and_training(tmp_path):
    """gnn/trainer.py:342-354 pickles the WHOLE module (and :128-130 deep-copies it), evaluate.py:46-52 loads that pickle: a HIP
    ``DetNetBasic`` that has run inference (folded / negated / concatenated weight caches on the instances, f16 plane caches keyed on
    its parameters) and a training step (autograd nodes, updated running statistics) must come back from ``torch.save`` ->
    ``torch.load`` (and from ``copy.deepcopy``) with the same parameters and buffers, no cache in the pickle, and the same logits."""
    import copy
    from radargnn_amd import derived, frames as fr, gnn
    frames = [synthetic.radarscenes_frame(i) for i in range(3)]
    cfg = fr.GraphSettings(algorithm="radius", r=1.5)
    mcfg = gnn.GNNArchitectureConfig(5, 2, [64, 64, 32], [6], [16, 5], True, True, [32, 64, 128, 64], [4, 8, 16], "MPNNConv", False)
    torch.manual_seed(12)
    model = gnn.DetNetBasic(mcfg).cuda()
    batch = fr.FrameBatch.from_frames(frames)
    hot = fr.HotPath(model, cfg)
    for stage in ("inference", "training"):
        if stage == "training":                               # one optimizer step the way the reference's trainer drives it
            g = fr.build_graphs(batch, cfg)
            opt = torch.optim.Adam(model.parameters(), lr=1e-3)
            x = g.x.clone().requires_grad_(True)
            c, b = model(x, g.edge_index, g.edge_attr)
            (c.square().mean() + b.square().mean()).backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
        c0, b0, g0 = hot(batch)                               # leaves the caches on the instances
        g0.check()
        assert {"fold", "edge_fold", "tail"} & set(model.convs[0].__dict__[derived.HOLDER])      # its holder has the fold slots filled
        path = tmp_path / f"trained_model_{stage}.pt"
        torch.save(model, str(path))
        back = torch.load(str(path), weights_only=False)
        twin = copy.deepcopy(model)
        for m in (back, twin):
            assert isinstance(m, gnn.DetNetBasic)
            assert derived.HOLDER not in m.__dict__ and not any(derived.HOLDER in c_.__dict__ for c_ in m.convs)
            for (ka, va), (kb, vb) in zip(m.state_dict().items(), model.state_dict().items()):
                assert ka == kb and torch.equal(va, vb), ka
        assert path.stat().st_size < 1.5 * sum(v.numel() * v.element_size() for v in model.state_dict().values()) + 200_000
        # train-mode logits depend on the batch only (the running statistics each forward updates do not enter them)
        c1, b1, _ = fr.HotPath(back.cuda(), cfg)(batch)
        c2, b2, _ = fr.HotPath(twin, cfg)(batch)
        assert torch.equal(c1, c0) and torch.equal(b1, b0) and torch.equal(c2, c0) and torch.equal(b2, b0)


@pytest.mark.parametrize("edge_mode", ["directed", "undirected"])
def test_radius_hot_path_with_general_edge_features_three_ways(edge_mode, monkeypatch):
    """Radius graphs whose edge features are not just relative_position (the 100 000-point configuration's point-pair features): the
    attributes in target order computed on the reversed end points (rgnn_edge_features_reversed; eager), the same inside ONE captured
    graph whose edge side runs as a branch beside the node side, and the twin-search form they replaced -- the same bits three ways."""
    from radargnn_amd import frames as fr, gnn
    frames = [synthetic.radarscenes_frame(i, n_clusters=10, pts_per_cluster=25, n_clutter=300) for i in range(6)]
    cfg = fr.GraphSettings(algorithm="radius", r=1.5, edge_mode=edge_mode,
                           node_features=("rcs", "velocity_vector_length", "time_index", "degree"),
                           edge_features=("point_pair_features", "relative_velocity"))
    mcfg = gnn.GNNArchitectureConfig(4, 6, [64, 32], [6], [16, 5], True, False, [32, 64], [8, 16], "MPNNConv", False)
    torch.manual_seed(5)
    model = gnn.DetNetBasic(mcfg).cuda().eval()
    batch = fr.FrameBatch.from_frames(frames)
    e_c, e_b, e_g = fr.HotPath(model, cfg)(batch)
    e_g.check()
    assert e_g.edge_index.shape[1] > 2000
    hot = fr.HotPath(model, cfg, use_hip_graphs=True)
    for _ in range(4):
        r_c, r_b, r_g = hot(batch)
    torch.cuda.synchronize()
    assert hot._graph is not None
    assert torch.equal(r_c, e_c) and torch.equal(r_b, e_b) and torch.equal(r_g.edge_attr, e_g.edge_attr)
    monkeypatch.setenv("RGNN_NO_REVERSED_FEATURES", "1")
    t_c, t_b, _ = fr.HotPath(model, cfg)(batch)
    assert torch.equal(t_c, e_c) and torch.equal(t_b, e_b)


def test_side_streams_run_beside_each_other_and_the_default_stream():
    """ops.independent_stream: every stream it hands out was seen running beside the default stream and the ones before it (ROCm maps
    streams onto four hardware queues; two on one queue serialise -- tools/hw_queue_probe.py)."""
    from radargnn_amd import ops
    dev = torch.device("cuda", 0)
    # (four queues: with the side / upload / download streams of earlier tests on record no further stream can pass -- the check is
    #  made against a fresh record here and the old one put back)
    saved = ops._INDEPENDENT.pop(dev.index, None)
    try:
        a, b = ops.independent_stream(dev), ops.independent_stream(dev)
    finally:
        if saved is not None:
            ops._INDEPENDENT[dev.index] = saved + ops._INDEPENDENT.get(dev.index, [])[1:]
    assert a.cuda_stream != b.cuda_stream and 0 not in (a.cuda_stream, b.cuda_stream)
    word = torch.zeros(1, device=dev)
    for busy, cand in ((torch.cuda.default_stream(dev), a), (torch.cuda.default_stream(dev), b), (a, b), (b, a)):
        assert ops._runs_beside(busy, cand, word)
    assert ops.ctx().side(dev, "plan") is ops.ctx().side(dev, "search")          # one stream for both roles (ForwardContext.side)
    assert ops.ctx().side(dev, "upload") is not ops.ctx().side(dev, "download")


@pytest.mark.gpu
def test_unordered_csr_gives_the_same_bits_for_max_aggregation(monkeypatch):
    """r06: with max aggregation HotPath builds the CSR by target of a kNN batch without the stable order inside the segments
    (rgnn_csr_by_target with ordered = 0: a maximum does not depend on the order of a target's in-edges).  Same logits and boxes, bit for bit,
    as with the ordered build; mean / add models keep the ordered build."""
    from radargnn_amd import frames as fr, gnn
    frames = [synthetic.radarscenes_frame(i) for i in range(4)]
    batch = fr.FrameBatch.from_frames(frames)
    cfg = fr.GraphSettings(algorithm="knn", k=12)
    mcfg = gnn.GNNArchitectureConfig(5, 2, [64, 48], [6], [16, 5], True, True, [32, 64], [4, 8, 16], "MPNNConv", False)
    torch.manual_seed(9)
    model = gnn.DetNetBasic(mcfg).cuda()
    hot = fr.HotPath(model, cfg)
    assert hot._ordered_csr is False
    c0, b0, g0 = hot(batch)
    monkeypatch.setenv("RGNN_ORDERED_CSR", "1")
    hot2 = fr.HotPath(model, cfg)
    assert hot2._ordered_csr is True
    c1, b1, g1 = hot2(batch)
    g0.check(); g1.check()
    assert torch.equal(c0, c1) and torch.equal(b0, b1) and torch.equal(g0.edge_index, g1.edge_index) and torch.equal(g0.x, g1.x)
    mean_cfg = gnn.GNNArchitectureConfig(5, 2, [64], [6], [16, 5], True, True, [32, 64], [4, 8, 16], "MPNNConv", False, 1, 1, False, "mean")
    monkeypatch.delenv("RGNN_ORDERED_CSR")
    assert fr.HotPath(gnn.DetNetBasic(mean_cfg).cuda(), cfg)._ordered_csr is True
