"""The capped radius graph (ops.radius_graph_capped; csrc/graph.hip k_radius_capped_rows) and every layer above it.

Rule: row i is S_i = {j != i, same frame, d2 <= r * r} when |S_i| <= k, else the k entries of S_i smallest under (d2, j); rows are
stored with ascending neighbour ids.  Reference: tests/capped_radius_oracle.py (float64, the KD-tree's arithmetic, built from
oracle/graph_oracle.py's pieces); tests/test_capped_radius_inputs.py proves on the CPU that the inputs cut rows between equal
distances, sit on every threshold of the fill kernel and have rows on both sides of every cap.

Bar: topology has no tolerance -- rowptr, col and edge_index equal the oracle's entry for entry (np.array_equal / torch.equal).
Float features and logits: the project's parity bar, max|a - b| <= 1e-5 max|b| against the float64 oracle (tests/test_gpu_gnn.py)."""
import numpy as np
import pytest
import torch

import capped_radius_oracle as co
import graph_edge_inputs as gi
from oracle import gnn_oracle as G
from oracle import graph_oracle as go
from radargnn_amd import synthetic

pytestmark = pytest.mark.gpu
RTOL = 1e-5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    from radargnn_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()              # (a copy: the oracle's cached arrays are read-only)


def case_batch(name, basis="X"):
    frames = co.frames_of(name)
    Xb = np.ascontiguousarray(np.concatenate([gi.basis(f, basis) for f in frames], axis=0))
    return Xb, co.case_candidates(name, basis)[3]


def check_rows(rowptr, col, ei, exp, n):
    """The three outputs against an edge list int64 [E, 2] ascending in (i, j)."""
    assert rowptr.dtype == torch.int32 and col.dtype == torch.int32 and ei.dtype == torch.int64
    assert np.array_equal(rowptr.cpu().numpy(), co.rowptr_of(exp, n))
    assert np.array_equal(col.cpu().numpy(), exp[:, 1])
    assert np.array_equal(ei.cpu().numpy(), exp.T)


def normwise(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# ================================================================================================ the search against the oracle
@pytest.mark.parametrize("name,k,basis", co.GPU_CASES)
def test_capped_rows_equal_the_oracle(ops, name, k, basis):
    """Lattices (ties at the cut and at d2 == r2), coincident points, the star batch on every threshold, the grid-geometry frames,
    a thin strip, negative coordinates, translated clouds and a batch of empty / one-point / two-point frames; bases of 2, 4 and 8
    columns.  Also the properties of a row that need no oracle, and that no edge leaves its frame."""
    Xb, ptr = case_batch(name, basis)
    exp, full, _ = co.expected(name, k, basis)
    n = Xb.shape[0]
    rowptr, col, ei = ops.radius_graph_capped(dev(Xb), dev(ptr), co.CASES[name][1], k)
    check_rows(rowptr, col, ei, exp, n)
    rp, c, e = rowptr.cpu().numpy(), col.cpu().numpy().astype(np.int64), ei.cpu().numpy()
    assert np.array_equal(np.diff(rp), np.minimum(full, k))                                    # every row length is min(|S_i|, k)
    assert (e[0] != e[1]).all()                                                                # no self loops
    inside = np.ones(len(c), bool)
    inside[rp[:-1][np.diff(rp) > 0]] = False
    assert (np.diff(c)[inside[1:]] > 0).all()                                                  # ids ascending and unique per row
    frame_of = np.searchsorted(ptr, np.arange(n), side="right") - 1
    assert np.array_equal(frame_of[e[0]], frame_of[e[1]])                                      # no edge crosses a frame


def test_no_points_and_only_empty_frames(ops):
    for ptr in ([0], [0, 0, 0]):
        rowptr, col, ei = ops.radius_graph_capped(torch.zeros((0, 2), dtype=torch.float64, device="cuda"),
                                                  torch.tensor(ptr, dtype=torch.int64, device="cuda"), 1.0, 4)
        assert rowptr.tolist() == [0] and col.numel() == 0 and tuple(ei.shape) == (2, 0)
    _, _, none = ops.radius_graph_capped(dev(gi.coincident(5).X), dev(np.array([0, 5])), 1.0, 2, want_edge_index=False)
    assert none is None


# ================================================================================================ the two identities
@pytest.mark.parametrize("name,basis", [("lattice_r1", "X"), ("lattice_r1", "X8"), ("coincident", "X"), ("geometry", "X"),
                                        ("translated", "X"), ("short_frames", "X")])
def test_a_cap_out_of_reach_gives_the_radius_graph_bit_for_bit(ops, name, basis):
    """Identity (a): k = 128 where no row holds more than 128 candidates -- rowptr, col and edge_index of ops.radius_graph."""
    Xb, ptr = case_batch(name, basis)
    assert co.expected(name, 1, basis)[1].max() <= 128
    X, P, r = dev(Xb), dev(ptr), co.CASES[name][1]
    a, b = ops.radius_graph_capped(X, P, r, 128), ops.radius_graph(X, P, r)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x, y)


@pytest.mark.parametrize("k", [1, 3, 16, 39])
def test_a_radius_beyond_the_frames_gives_the_knn_rows(ops, k):
    """Identity (b): r = 1e6 -- every row, as a set, is the row of ops.knn_graph (distance asc, index asc: the same tie rule)."""
    frames = [gi.lattice(22, 0.5), gi.coincident_among_others()]
    cat, ptr = synthetic.concat_frames(frames)
    X, P = dev(cat.X), dev(ptr)
    rowptr, col, _ = ops.radius_graph_capped(X, P, 1e6, k)
    nbr, _, status = ops.knn_graph(X, P, k)
    assert status.item() == 0
    assert torch.equal(rowptr, torch.arange(0, cat.n * k + 1, k, dtype=torch.int32, device="cuda"))
    assert torch.equal(col.view(cat.n, k), nbr.sort(dim=1).values)


# ================================================================================================ determinism
def test_same_rows_on_every_call_and_in_every_point_order(ops):
    """The result is a function of the points alone: identical across two calls, and -- the points of every frame shuffled --
    identical after mapping the ids back (a tie at the cut goes to the smaller ORIGINAL index only if the ids say so: compare on the
    lattice-free star batch at k = 48, whose distances are distinct, and on the lattice through the oracle of the shuffled cloud)."""
    Xb, ptr = case_batch("star")
    r, k = gi.STAR_R, 48
    X, P = dev(Xb), dev(ptr)
    first = ops.radius_graph_capped(X, P, r, k)
    again = ops.radius_graph_capped(X, P, r, k)
    assert all(torch.equal(x, y) for x, y in zip(first, again))
    rng = np.random.Generator(np.random.PCG64(77))
    perm = np.concatenate([a + rng.permutation(b - a) for a, b in zip(ptr[:-1], ptr[1:])])      # new row p holds old point perm[p]
    _, _, ei = ops.radius_graph_capped(dev(Xb[perm]), P, r, k)
    back = perm[ei.cpu().numpy()]                                                               # edges in old ids
    exp = co.expected("star", k)[0]
    assert np.array_equal(back[:, np.lexsort((back[1], back[0]))], exp.T)
    # with ties at the cut the shuffled cloud is another input (other indices break the ties): against ITS oracle
    f = gi.lattice(24, 0.5)
    p2 = rng.permutation(f.n)
    _, _, ei2 = ops.radius_graph_capped(dev(f.X[p2]), dev(np.array([0, f.n])), 1.0, 3)
    assert np.array_equal(ei2.cpu().numpy().T, co.frame_edges(f.X[p2], 1.0, 3))


# ================================================================================================ arguments
@pytest.mark.parametrize("k", [0, 129, -1, 2.0, "3", None, True])
def test_invalid_caps_raise(ops, k):
    X, P = dev(gi.coincident(5).X), dev(np.array([0, 5]))
    with pytest.raises(ValueError, match="neighbour cap"):
        ops.radius_graph_capped(X, P, 1.0, k)


def test_c_entry_points_refuse_a_bad_cap(ops):
    import ctypes as C
    from radargnn_amd import _lib
    g = ops.GridHash(dev(gi.coincident(5).X), dev(np.array([0, 5]))).build(cell_size=1.0)
    full = torch.zeros(5, dtype=torch.int32, device="cuda")
    lens = torch.zeros(10, dtype=torch.int32, device="cuda")
    for k in (0, 129):
        assert _lib.lib.rgnn_radius_graph_capped_count(C.byref(g.desc), 1.0, k, ops._ptr(full), ops._ptr(lens), ops._stream()) == -1
        assert _lib.lib.rgnn_radius_graph_capped_rows(C.byref(g.desc), 1.0, k, ops._ptr(full), ops._ptr(lens), None, None, 0, None, 0,
                                                      ops._stream()) == -1


# ================================================================================================ graph constructor
def test_graph_build_with_a_cap(ops):
    from radargnn_amd import graph_constructor as gc
    f = gi.coincident_among_others()
    r, k = 1.5, 5
    exp = co.frame_edges(f.X, r, k)
    assert len(exp) < go.radius_edges(f.X, r).shape[0]
    for cls in (gc.Graph, gc.GeometricGraph):
        g = cls()
        g.build(f.X, "radius", r=r, max_neighbors=k)
        assert g.E.dtype == np.int32 and np.array_equal(g.E, exp)
        assert np.array_equal(np.asarray(g.get_degree()), go.undirected_degree(exp, f.n))       # asymmetric edge list
        plain, none = cls(), cls()
        plain.build(f.X, "radius", r=r)
        none.build(f.X, "radius", r=r, max_neighbors=None)
        assert np.array_equal(plain.E, go.radius_edges(f.X, r)) and np.array_equal(none.E, plain.E)
        knn = cls()
        knn.build(f.X, "knn", k=4)                                                              # (untouched by the new argument)
        assert np.array_equal(knn.E, go.knn_edges(f.X, 4))
    with pytest.raises(ValueError, match="neighbour cap"):
        gc.Graph().build(f.X, "radius", r=r, max_neighbors=0)


def test_configuration_reads_max_neighbors_and_never_k(ops):
    from radargnn_amd import graph_constructor as gc
    from radargnn_amd.graph_constructor.configs import GraphConstructionConfiguration as Cfg
    from radargnn_amd.preprocessor import graph_settings
    feats = (["rcs", "degree"], ["relative_position"], "directed", "X")
    capped = Cfg("radius", {"k": 20, "r": 1.5, "max_neighbors": 5}, *feats)
    shipped = Cfg("radius", {"k": 20, "r": 1.5}, *feats)                  # the shipped YAMLs: a "k" that a radius graph ignores
    knn = Cfg("knn", {"k": 4, "r": 1.5, "max_neighbors": 2}, *feats)      # the key means nothing to a kNN graph
    assert (capped.max_neighbors, shipped.max_neighbors, knn.max_neighbors) == (5, None, None)
    assert (capped.k, shipped.k, knn.k, knn.r) == (None, None, 4, None)
    assert graph_settings(capped).max_neighbors == 5 and graph_settings(capped).capped
    assert graph_settings(shipped).max_neighbors is None and not graph_settings(knn).capped

    class Cloud:
        pass
    f = gi.coincident_among_others()
    pc = Cloud()
    pc.X_cc, pc.V_cc_compensated, pc.rcs, pc.timestamp = f.X, f.V, f.rcs, f.timestamp
    assert np.array_equal(gc.build_geometric_graph(capped, pc).E, co.frame_edges(f.X, 1.5, 5))
    assert np.array_equal(gc.build_geometric_graph(shipped, pc).E, go.radius_edges(f.X, 1.5))
    assert np.array_equal(gc.build_geometric_graph(knn, pc).E, go.knn_edges(f.X, 4))
    g = gc.build_geometric_graph(capped, pc)
    assert np.array_equal(g.X_feat[:, 1], go.undirected_degree(co.frame_edges(f.X, 1.5, 5), f.n))


# ================================================================================================ batched pipeline
NODE_FEATURES = ("rcs", "velocity_vector", "time_index", "degree")


def small_batch():
    return [synthetic.radarscenes_frame(i, n_clusters=6, pts_per_cluster=25, n_clutter=80) for i in range(3)] + [gi.coincident_among_others()]


def oracle_graphs(frames, r, k, edge_features, edge_mode):
    """What go.build_frame_graph + go.collate give, with the capped edge list in the place of go.build_edges."""
    graphs = []
    for f in frames:
        E = co.frame_edges(f.X, r, k)
        ea = go.edge_features(f.X, f.V, E, edge_features, edge_mode)
        x = go.node_features(f.X, f.V, {"rcs": f.rcs, "time_index": go.time_index(f.timestamp)}, go.undirected_degree(E, f.n), NODE_FEATURES)
        graphs.append({"x": x.astype(np.float32), "edge_index": np.ascontiguousarray(E.T.astype(np.int64)), "edge_attr": ea.astype(np.float32),
                       "x64": x, "ea64": ea})
    out = go.collate(graphs)
    out["x64"], out["ea64"] = np.concatenate([g["x64"] for g in graphs]), np.concatenate([g["ea64"] for g in graphs])
    return out


@pytest.mark.parametrize("edge_features,edge_mode", [(("relative_position",), "directed"),
                                                     (("spatial_euclidean_distance", "relative_velocity"), "undirected")])
def test_build_graphs_with_a_cap(ops, edge_features, edge_mode):
    from radargnn_amd import frames as fr
    frames, r, k = small_batch(), 1.0, 6
    assert 300 <= sum(f.n for f in frames) <= 900
    ref = oracle_graphs(frames, r, k, list(edge_features), edge_mode)
    cfg = fr.GraphSettings(algorithm="radius", r=r, max_neighbors=k, node_features=NODE_FEATURES, edge_features=edge_features,
                           edge_mode=edge_mode)
    g = fr.build_graphs(fr.FrameBatch.from_frames(frames), cfg)
    g.check()
    n = ref["x"].shape[0]
    uncapped = fr.build_graphs(fr.FrameBatch.from_frames(frames), fr.GraphSettings(algorithm="radius", r=r, node_features=NODE_FEATURES))
    assert g.edge_index.shape[1] < uncapped.edge_index.shape[1]                       # the cap cuts rows of this batch
    assert np.array_equal(g.edge_index.cpu().numpy(), ref["edge_index"])
    assert np.array_equal(g.rowptr.cpu().numpy(), co.rowptr_of(ref["edge_index"].T, n))
    assert np.array_equal(g.degree.cpu().numpy(), ref["x64"][:, 4].astype(np.int64)) and g.split is None
    assert normwise(g.x, torch.from_numpy(ref["x64"])) <= RTOL
    assert np.array_equal(g.x[:, 4].cpu().numpy(), ref["x"][:, 4])                    # the degree column
    assert normwise(g.edge_attr, torch.from_numpy(ref["ea64"])) <= RTOL
    # the graph is not symmetric -- which is why none of the radius path's shortcuts may be taken
    e = ref["edge_index"]
    pairs = set(map(tuple, e.T.tolist()))
    assert any((b, a) not in pairs for a, b in pairs)


@pytest.mark.parametrize("aggr", ["max", "mean"])
def test_hot_path_with_a_cap_vs_oracle(ops, aggr):
    from radargnn_amd import frames as fr, gnn
    frames, r, k = small_batch(), 1.0, 6
    cfg = fr.GraphSettings(algorithm="radius", r=r, max_neighbors=k, node_features=NODE_FEATURES)
    mcfg = gnn.GNNArchitectureConfig(5, 2, [64, 64, 32], [11], [16, 5], True, True, [32, 64], [4, 8, 16], "MPNNConv", False, 1, 1, False, aggr)
    torch.manual_seed(5)
    model = gnn.DetNetBasic(mcfg)
    sd = {name: v.detach().clone() for name, v in model.state_dict().items()}
    model.cuda()
    hot = fr.HotPath(model, cfg)
    assert hot.symmetric_graph is False
    cls, bb, g = hot(fr.FrameBatch.from_frames(frames))
    g.check()
    ref = oracle_graphs(frames, r, k, ["relative_position"], "directed")
    assert np.array_equal(g.edge_index.cpu().numpy(), ref["edge_index"])
    c64, b64 = G.det_net_basic(torch.from_numpy(ref["x"]), torch.from_numpy(ref["edge_index"]), torch.from_numpy(ref["edge_attr"]), sd,
                               "MPNNConv", aggr, dtype=torch.float64)
    assert normwise(cls, c64) < RTOL and normwise(bb, b64) < RTOL


def test_captured_and_streamed_steps_refuse_a_cap(ops):
    from radargnn_amd import frames as fr, gnn
    cfg = fr.GraphSettings(algorithm="radius", r=1.0, max_neighbors=6)
    model = gnn.DetNetBasic(gnn.GNNArchitectureConfig(5, 2, [32], [6], [16, 5], True, True, [32], [4], "MPNNConv", False)).cuda()
    with pytest.raises(ValueError, match="max_neighbors"):
        fr.HotPath(model, cfg, use_hip_graphs=True)
    hot = fr.HotPath(model, cfg)
    with pytest.raises(ValueError, match="max_neighbors"):
        fr.FrameStreamer(hot)
    with pytest.raises(ValueError, match="neighbour cap"):
        fr.HotPath(model, fr.GraphSettings(algorithm="radius", r=1.0, max_neighbors=129))
    # no cap, and a cap on a kNN graph (ignored): as before
    fr.HotPath(model, fr.GraphSettings(algorithm="radius", r=1.0), use_hip_graphs=True)
    fr.HotPath(model, fr.GraphSettings(algorithm="knn", k=4, max_neighbors=6), use_hip_graphs=True)
