"""radargnn_amd.subgraph on the device (csrc/subgraph.hip) against tests/subgraph_oracle.py (itself checked against plain loops in
tests/test_subgraph_oracle.py).  Everything here is a move or an integer: results are compared EXACTLY, float tensors byte for byte so
that NaN payloads count.  The one float comparison is the model test (the project's 1e-5 bar, where equality is expected)."""
import math

import numpy as np
import pytest
import torch

import subgraph_oracle as S
from conftest import record_parity

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 4, 5, 7, 8)
NODE_FEATURES = ["rcs", "velocity_vector", "time_index", "degree"]


@pytest.fixture(scope="module")
def rg():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    import radargnn_amd
    from radargnn_amd import data, frames, gnn, graph_constructor, ops, subgraph, synthetic, transforms        # noqa: F401
    from radargnn_amd.gnn import trainer                                                                        # noqa: F401
    return radargnn_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().contiguous().numpy()


def same_bytes(got, want, what):
    got, want = host(got) if torch.is_tensor(got) else np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert got.tobytes() == want.tobytes(), (what, np.nonzero(got.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8))[0][:8])


def make_batch(rg, edge_index, batch, ptr, **attrs):
    b = rg.data.Batch()
    for k, v in attrs.items():
        setattr(b, k, v if torch.is_tensor(v) else dev(v))
    b.edge_index, b.batch, b.ptr = dev(edge_index), dev(batch), dev(ptr)
    return b


def check_part(out, want, what=""):
    same_bytes(out.edge_index, want["edge_index"], what + " edge_index")
    same_bytes(out.batch, want["batch"], what + " batch")
    same_bytes(out.ptr, want["ptr"], what + " ptr")
    same_bytes(out._edge_ptr, want["edge_ptr"], what + " _edge_ptr")
    for k, v in list(want["node_attrs"].items()) + list(want["edge_attrs"].items()):
        same_bytes(getattr(out, k), v, f"{what} {k}")


def mask(m):
    return None if m is None else dev(np.asarray(m, dtype=bool))


# ---- the hand-built batch through GraphStore.collate ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand(rg):
    """graph sizes (5, 0, 4, 1), the last without edges: x, y (NaN box rows), pos, vel per node, edge_attr per edge"""
    ei, batch, ptr = S.hand_batch()
    rng = np.random.Generator(np.random.PCG64(3))
    graphs = []
    for g in range(4):
        n0, n1 = ptr[g], ptr[g + 1]
        sel = (batch[ei[0]] == g)
        n, e = n1 - n0, int(sel.sum())
        y = rng.normal(size=(n, 6)).astype(np.float32)
        y[::2, 1:] = np.nan
        f = lambda *shape: torch.from_numpy(rng.normal(size=shape).astype(np.float32))
        graphs.append(rg.data.Data(x=f(n, 5), edge_index=torch.from_numpy(ei[:, sel] - n0), edge_attr=f(e, 2), y=torch.from_numpy(y),
                                   pos=f(n, 2), vel=f(n, 2)))
    b = rg.data.GraphStore(graphs).collate([0, 1, 2, 3])
    assert np.array_equal(host(b.edge_index), ei) and np.array_equal(host(b.ptr), ptr) and np.array_equal(host(b.batch), batch)
    arrays = {k: host(getattr(b, k)) for k in ("x", "y", "pos", "vel", "edge_attr")}
    return b, arrays


@pytest.mark.parametrize("name", list(S.MASKS))
def test_hand_batch_equals_the_oracle(rg, hand, name):
    b, arrays = hand
    kn, ke = S.MASKS[name]
    ei, batch, ptr = S.hand_batch()
    want = S.subgraph(ei, batch, ptr, kn, ke, node_attrs={k: arrays[k] for k in ("x", "y", "pos", "vel")},
                      edge_attrs={"edge_attr": arrays["edge_attr"]})
    out = rg.subgraph.subgraph(b, mask(kn), mask(ke))
    assert out.keys == b.keys and out.num_graphs == 4 and out._status == 0
    check_part(out, want, name)
    graphs = out.to_data_list()
    for got, w in zip(graphs, S.graphs_of(want)):
        same_bytes(got.edge_index, w["edge_index"], name + " graph edge_index")
        for k, v in list(w["node_attrs"].items()) + list(w["edge_attrs"].items()):
            same_bytes(getattr(got, k), v, f"{name} graph {k}")
    if name == "all":                                              # equal to the input bit for bit
        for k in b.keys:
            same_bytes(getattr(out, k), host(getattr(b, k)), "all " + k)
        same_bytes(out._edge_ptr, host(b._edge_ptr), "all _edge_ptr")
    if name == "none":
        assert host(out.ptr).tolist() == [0] * 5 and host(out._edge_ptr).tolist() == [0] * 5
        assert out.x.shape == (0, 5) and out.edge_index.shape == (2, 0) and out.edge_attr.shape == (0, 2) and out.batch.shape == (0,)


def test_uint8_masks_and_new_ids(rg, hand):
    b, _ = hand
    ei, batch, ptr = S.hand_batch()
    kn = S.MASKS["both"][0]
    want = S.subgraph(ei, batch, ptr, kn, None)
    out = rg.subgraph.subgraph(b, dev(kn.astype(np.uint8) * 7))          # any non-zero byte keeps
    check_part(out, want, "uint8")
    st = rg.ops.subgraph_structure(b.edge_index, b.batch, b.ptr, 10, rg.ops.keep_mask(mask(kn), 10, "keep"), None, want_new_id=True)
    same_bytes(st["new_id"], want["new_id"], "new_id")


# ---- scan and tile edges ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_cases():
    return {}


def random_case(rg, cache, n, epn):
    key = (n, epn)
    if key not in cache:
        c = S.random_batch(n, epn, 1 if n == 1 else 3, seed=n, widths=WIDTHS)
        wide = np.random.Generator(np.random.PCG64(n + 7)).integers(0, 2 ** 32, size=(n, 12), dtype=np.uint64).astype(np.uint32).view(np.float32)
        attrs = {f"x{w}": c[f"x{w}"] for w in WIDTHS}
        attrs["edge_attr"] = c["edge_attr"]
        b = make_batch(rg, c["edge_index"], c["batch"], c["ptr"], **attrs)
        big = dev(wide)
        b.xs = big[:, 1:5]                                          # a column slice off the 16-byte grid: the dword path, row stride 12
        b.xa = big[:, 4:8]                                          # a column slice on it: 16 bytes per lane, row stride 12
        assert n == 1 or (not b.xs.is_contiguous() and not b.xa.is_contiguous())
        c["xs"], c["xa"] = wide[:, 1:5], wide[:, 4:8]
        cache[key] = (c, b)
    return cache[key]


@pytest.mark.parametrize("share", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("n,epn", [(1, 3), (255, 3), (256, 3), (257, 3), (1023, 3), (1024, 3), (1025, 3), (70001, 3), (1025, 0)])
def test_random_batches_equal_the_oracle(rg, random_cases, n, epn, share):
    """N around the scan's 256-thread and 2048-item tiles and one batch of many tiles (the three-launch scan); rows of 1 .. 8 words:
    16 bytes per lane (4, 8), the dword path (1, 3, 5, 7); column slices; E = 0 once.  The maps against the oracle; the inputs are
    never written."""
    c, b = random_case(rg, random_cases, n, epn)
    e = c["edge_index"].shape[1]
    assert e == (0 if epn == 0 else sum(int(math.floor(s * epn)) for s in np.diff(c["ptr"])))
    rng = np.random.Generator(np.random.PCG64(int(1000 * share) + n))
    kn = rng.uniform(size=n) < share if share < 1.0 else np.ones(n, bool)
    ke = rng.uniform(size=e) < 0.5 if share == 0.5 else None
    names = [f"x{w}" for w in WIDTHS] + ["xs", "xa"]
    want = S.subgraph(c["edge_index"], c["batch"], c["ptr"], kn, ke, node_attrs={k: c[k] for k in names}, edge_attrs={"edge_attr": c["edge_attr"]})
    before = {k: getattr(b, k).clone() for k in b.keys}
    out, node_ids, edge_ids = rg.subgraph.subgraph(b, mask(kn), mask(ke), return_maps=True)
    assert out._status == 0
    check_part(out, want, f"n {n} share {share}")
    same_bytes(node_ids, want["node_ids"], "node_ids")
    same_bytes(edge_ids, want["edge_ids"], "edge_ids")
    for k, v in before.items():
        same_bytes(getattr(b, k), host(v), f"input {k} was written")
    if share == 1.0:
        same_bytes(out.edge_index, c["edge_index"], "whole edge_index")
        same_bytes(out._edge_ptr, c["edge_ptr"], "whole _edge_ptr")


def test_float64_and_int64_rows(rg):
    """8-byte elements: rows of 2 and 4 words, and an attribute with a trailing shape"""
    c = S.random_batch(300, 2, 2, seed=11)
    rng = np.random.Generator(np.random.PCG64(12))
    t64, i64, cube = rng.normal(size=300), rng.integers(-2 ** 62, 2 ** 62, size=(300, 2)), rng.normal(size=(300, 2, 3)).astype(np.float32)
    b = make_batch(rg, c["edge_index"], c["batch"], c["ptr"], t64=t64, i64=i64, cube=cube)
    kn = rng.uniform(size=300) < 0.5
    want = S.subgraph(c["edge_index"], c["batch"], c["ptr"], kn, None, node_attrs={"t64": t64, "i64": i64, "cube": cube})
    check_part(rg.subgraph.subgraph(b, mask(kn)), want, "wide rows")


# ---- unsound edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masks", ["none", "nodes", "edges"])
def test_bad_edges_are_dropped_and_reported(rg, masks):
    """an end at N, an end at -1, an edge joining two graphs and one out of graph order: refused without being used as indices"""
    ei, batch, ptr = S.bad_batch()
    e = ei.shape[1]
    rng = np.random.Generator(np.random.PCG64(8))
    x, ea = rng.normal(size=(10, 4)).astype(np.float32), rng.normal(size=(e, 2)).astype(np.float32)
    kn = np.arange(10) % 3 != 0 if masks == "nodes" else np.ones(10, bool)
    ke = np.arange(e) % 2 == 0 if masks == "edges" else None
    b = make_batch(rg, ei, batch, ptr, x=x, edge_attr=ea)
    want = S.subgraph(ei, batch, ptr, kn, ke, node_attrs={"x": x}, edge_attrs={"edge_attr": ea})
    assert want["status"] == S.BAD_ENDPOINT | S.CROSS_GRAPH | S.EDGE_ORDER
    out = rg.subgraph.subgraph(b, mask(kn), mask(ke), check=False)
    assert out._status == want["status"]
    check_part(out, want, "bad edges")
    with pytest.raises(ValueError, match="outside.*two graphs.*grouped by graph"):
        rg.subgraph.subgraph(b, mask(kn), mask(ke))
    if masks == "none":
        sound = S.subgraph(*S.hand_batch())
        same_bytes(out.edge_index, sound["edge_index"], "the sound edges")


def test_bad_graph_ids_and_offsets(rg):
    ei, batch, ptr = S.hand_batch()
    wrong = np.where(batch == 2, 7, batch)                         # the sources of graph 2's edges name a graph that does not exist
    want = S.subgraph(ei, wrong, ptr, np.ones(10, bool), None)
    out = rg.subgraph.subgraph(make_batch(rg, ei, wrong, ptr), mask(np.ones(10, bool)), check=False)
    assert out._status == want["status"] == S.BAD_GRAPH
    check_part(out, want, "bad graph id")
    bad_ptr = ptr.copy()
    bad_ptr[1], bad_ptr[4] = -3, 99
    kn = np.arange(10) % 2 == 0
    want = S.subgraph(ei, batch, bad_ptr, kn, None)
    out = rg.subgraph.subgraph(make_batch(rg, ei, batch, bad_ptr), mask(kn), check=False)
    assert out._status == want["status"] == S.BAD_GRAPH
    check_part(out, want, "bad ptr")


# ---- the degree column ------------------------------------------------------------------------------------------------------------
def test_degree_recompute(rg):
    frame = rg.synthetic.small_frame(300, seed=4)
    g = rg.graph_constructor.GeometricGraph()
    g.X = frame.X
    g.build(frame.X, "radius", r=1.0)
    ei = np.ascontiguousarray(g.E.T.astype(np.int64))
    n = 300
    assert ei.shape[1] > 1000 and np.array_equal(np.array(g.get_degree()), S.undirected_degree(ei, n))
    rng = np.random.Generator(np.random.PCG64(21))
    x = rng.normal(size=(n, 5)).astype(np.float32)
    x[:, 4] = g.get_degree()
    b = make_batch(rg, ei, np.zeros(n, np.int64), np.array([0, n]), x=x)
    kn = rng.uniform(size=n) < 0.6
    ke = rng.uniform(size=ei.shape[1]) < 0.8                       # an edge mask on top: the kept graph is no longer symmetric
    for ke_ in (None, ke):
        want = S.subgraph(ei, np.zeros(n, np.int64), np.array([0, n]), kn, ke_, node_attrs={"x": x})
        n_out = len(want["node_ids"])
        deg = S.undirected_degree(want["edge_index"], n_out)
        induced = rg.graph_constructor.Graph()
        induced.E, induced._n_nodes = np.ascontiguousarray(want["edge_index"].T.astype(np.int32)), n_out
        assert np.array_equal(np.array(induced.get_degree()), deg)
        kept = rg.subgraph.subgraph(b, mask(kn), mask(ke_))
        check_part(kept, want, "degree keep")                        # the default leaves the stored column
        out = rg.subgraph.subgraph(b, mask(kn), mask(ke_), degree="recompute", node_features=NODE_FEATURES)
        want["node_attrs"]["x"][:, 4] = deg
        check_part(out, want, "degree recompute")
    assert (deg != x[want["node_ids"], 4]).any()
    none = rg.subgraph.subgraph(b, mask(kn), mask(np.zeros(ei.shape[1], bool)), degree="recompute", node_features=NODE_FEATURES)
    assert none.edge_index.shape == (2, 0) and not host(none.x)[:, 4].any()


# ---- the pair hash -----------------------------------------------------------------------------------------------------------------
DRAWS = [(0, 0, 1, 570621), (0, 1, 0, 570621), (1, 0, 1, 15334752), (12345, 7, 191999, 5680362),
         (-1, 2147483646, 3, 16769353), (2 ** 63 - 1, 5, 5, 4786746)]


@pytest.mark.parametrize("seed,s,t,draw", DRAWS)
def test_pair_draws_through_the_device(rg, seed, s, t, draw):
    """keep = draw >= threshold: kept at threshold = draw, dropped at draw + 1 (p = threshold / 2^24 is exact in a double)"""
    ei, sd = dev(np.array([[s], [t]], dtype=np.int64)), dev(np.array([seed], dtype=np.int64))
    assert rg.ops.pair_threshold(draw / 2 ** 24) == draw and rg.ops.pair_threshold((draw + 1) / 2 ** 24) == draw + 1
    assert host(rg.ops.edge_pair_mask(ei, 2 ** 31, sd, draw / 2 ** 24)).tolist() == [True]
    assert host(rg.ops.edge_pair_mask(ei, 2 ** 31, sd, (draw + 1) / 2 ** 24)).tolist() == [False]


def test_pair_mask_on_a_symmetric_graph(rg):
    frame = rg.synthetic.small_frame(300, seed=9)
    X = dev(frame.X.astype(np.float64))
    _, _, ei = rg.ops.radius_graph(X, dev(np.array([0, 300])), 1.0)
    ei_h = host(ei)
    seed = 99
    got = host(rg.ops.edge_pair_mask(ei, 300, dev(np.array([seed])), 0.3))
    want = S.pair_mask(ei_h, 300, seed, 0.3)
    assert got.dtype == np.bool_ and np.array_equal(got, want) and 0.55 < got.mean() < 0.85
    kept = {(int(a), int(b)) for a, b in ei_h[:, got].T}
    assert kept and all((b, a) in kept for a, b in kept)
    assert host(rg.ops.edge_pair_mask(ei, 300, dev(np.array([seed])), 0.0)).all()
    assert not host(rg.ops.edge_pair_mask(ei, 300, dev(np.array([seed])), 1.0)).any()
    outside = dev(np.array([[0, -1, 5, 1], [300, 2, 0, 2]]))
    assert host(rg.ops.edge_pair_mask(outside, 300, dev(np.array([seed])), 0.0)).tolist() == [False, False, True, True]


# ---- the dropouts ------------------------------------------------------------------------------------------------------------------
def test_dropouts(rg, hand, random_cases):
    _, b = random_case(rg, random_cases, 1025, 3)
    SG = rg.subgraph
    gen = lambda: torch.Generator(device="cuda").manual_seed(77)
    for make in (lambda p, g: SG.RandomNodeDropout(p, generator=g), lambda p, g: SG.RandomEdgeDropout(p, generator=g),
                 lambda p, g: SG.RandomEdgeDropout(p, generator=g, pairs=True)):
        whole = make(0.0, gen())(b)
        for k in b.keys:
            same_bytes(getattr(whole, k), host(getattr(b, k)), "p = 0 " + k)
        first, second = make(0.4, gen())(b), make(0.4, gen())(b)
        for k in b.keys:
            same_bytes(getattr(first, k), host(getattr(second, k)), "same seed " + k)
        assert 0 < first.edge_index.shape[1] < b.edge_index.shape[1]
    empty = SG.RandomNodeDropout(1.0)(b)
    assert empty.x4.shape == (0, 4) and empty.edge_index.shape == (2, 0) and not host(empty.ptr).any() and not host(empty._edge_ptr).any()
    no_edges = SG.RandomEdgeDropout(1.0, pairs=True)(b)
    assert no_edges.edge_index.shape == (2, 0) and no_edges.x4.shape == b.x4.shape and np.array_equal(host(no_edges.ptr), host(b.ptr))
    assert SG.RandomEdgeDropout(1.0)(b).edge_attr.shape == (0, 2)
    part = SG.RandomNodeDropout(0.4, generator=gen())(b)
    assert 0.45 < part.x4.shape[0] / 1025 < 0.75


# ---- frames ---------------------------------------------------------------------------------------------------------------------
def test_drop_points(rg):
    frames = [rg.synthetic.small_frame(n, seed=30 + i) for i, n in enumerate((0, 1, 300, 1025))]
    fb = rg.frames.FrameBatch.from_frames(frames)
    n = fb.num_points
    keep = np.random.Generator(np.random.PCG64(2)).uniform(size=n) < 0.5
    keep[0] = True                                                 # the one-point frame keeps its point
    before = {k: getattr(fb, k).clone() for k in ("X", "V", "rcs", "timestamp", "frame_ptr")}
    out = rg.subgraph.drop_points(fb, mask(keep))
    ptr = host(fb.frame_ptr)
    want_ptr = np.concatenate(([0], np.cumsum(keep)))[ptr]
    same_bytes(out.frame_ptr, want_ptr.astype(np.int64), "frame_ptr")
    assert np.array_equal(out.frame_sizes, np.diff(want_ptr)) and out.num_frames == 4 and out.frame_sizes[0] == 0 and out.frame_sizes[1] == 1
    for k in ("X", "V", "rcs", "timestamp"):
        same_bytes(getattr(out, k), host(before[k])[keep], k)
        assert torch.equal(getattr(fb, k), before[k])
    none = rg.subgraph.drop_points(fb, mask(np.zeros(n, bool)))
    assert none.X.shape == (0, 2) and not none.frame_sizes.any() and not host(none.frame_ptr).any()


# ---- the model and the trainer ----------------------------------------------------------------------------------------------------
BG = 5
WEIGHTS = {"car": 1.0, "pedestrian": 2.0, "pedestrian_group": 1.5, "two_wheeler": 3.0, "large_vehicle": 0.7, "background": 0.1}


@pytest.fixture(scope="module")
def graphs(rg):
    """four graphs of 30-45 points (5 nearest neighbours, the shipped feature lists) with pos, vel and rotated boxes"""
    settings = rg.frames.GraphSettings(algorithm="knn", k=5)
    out = []
    for i, n in enumerate((30, 45, 38, 41)):
        frame = rg.synthetic.small_frame(n, seed=70 + i)
        g = rg.frames.build_graphs(rg.frames.FrameBatch.from_frames([frame]), settings)
        rng = np.random.Generator(np.random.PCG64(17 + i))
        label = np.where(rng.uniform(size=n) < 0.5, rng.integers(0, BG, size=n), BG)
        box = np.concatenate((rng.normal(0.0, 1.5, size=(n, 2)), rng.uniform(0.5, 4.0, size=(n, 2)), rng.uniform(0.0, np.pi, size=(n, 1))), axis=1)
        box[label == BG] = np.nan
        y = torch.tensor(np.concatenate((label.reshape(-1, 1), box), axis=1), dtype=torch.float32)
        out.append(rg.data.Data(x=g.x.cpu(), edge_index=g.edge_index.cpu(), edge_attr=g.edge_attr.cpu(), y=y,
                                pos=torch.tensor(frame.X, dtype=torch.float32), vel=torch.tensor(frame.V, dtype=torch.float32)))
    return out


def small_model(rg):
    arch = rg.gnn.GNNArchitectureConfig(node_feature_dimension=5, edge_feature_dimension=2, conv_layer_dimensions=[16, 8],
                                        classification_head_layer_dimensions=[6], regression_head_layer_dimensions=[8, 5],
                                        initial_node_feature_embedding=True, initial_edge_feature_embedding=True,
                                        node_feature_embedding_layer_dimensions=[8, 16],
                                        edge_feature_embedding_layer_dimensions=[4, 8], conv_layer_type="MPNNConv",
                                        batch_norm_in_mlps=False)
    torch.manual_seed(0)
    return rg.gnn.DetNetBasic(arch).cuda()


def test_model_on_a_subgraph_equals_the_model_on_the_kept_graphs(rg, graphs):
    b = rg.data.GraphStore(graphs).collate([0, 1, 2, 3])
    n = b.x.shape[0]
    kn = np.random.Generator(np.random.PCG64(5)).uniform(size=n) < 0.7
    part = rg.subgraph.subgraph(b, mask(kn))
    arrays = {k: host(getattr(b, k)) for k in ("x", "y", "pos", "vel", "edge_attr")}
    want = S.subgraph(host(b.edge_index), host(b.batch), host(b.ptr), kn, None, node_attrs={k: arrays[k] for k in ("x", "y", "pos", "vel")},
                      edge_attrs={"edge_attr": arrays["edge_attr"]})
    kept = [rg.data.Data(edge_index=torch.from_numpy(np.ascontiguousarray(g["edge_index"])), edge_attr=torch.from_numpy(g["edge_attrs"]["edge_attr"]),
                         **{k: torch.from_numpy(v) for k, v in g["node_attrs"].items()}) for g in S.graphs_of(want)]
    ref = rg.data.GraphStore(kept).collate([0, 1, 2, 3])
    model = small_model(rg)
    with torch.no_grad():
        cls_a, bb_a = model(part.x, part.edge_index, part.edge_attr)
        cls_b, bb_b = model(ref.x, ref.edge_index, ref.edge_attr)
    err = lambda a, r: float((a.double() - r.double()).abs().max() / r.double().abs().max())
    record_parity("subgraph_model", logits=err(cls_a, cls_b), boxes=err(bb_a, bb_b))
    assert err(cls_a, cls_b) <= 1e-5 and err(bb_a, bb_b) <= 1e-5
    assert cls_a.shape[0] == int(kn.sum())


def fit(rg, graph_list, transform):
    cfg = rg.gnn.TrainingConfig(dataset="radarscenes", learning_rate=5e-3, epochs=1, batch_size=2, shuffle=False, bg_index=BG,
                                class_weights=dict(WEIGHTS), val_class_weights=dict(WEIGHTS), adapt_orientation_angle=True)
    model = small_model(rg)
    train = rg.data.DataLoader(rg.data.GraphStore(graph_list), batch_size=2, shuffle=False)
    valid = rg.data.DataLoader(rg.data.GraphStore(graph_list[:2]), batch_size=2, shuffle=False)
    if transform is not None:
        train = rg.transforms.TransformedLoader(train, transform)
    t = rg.gnn.trainer.Trainer(cfg, model)
    t.fit({"train": train, "validate": valid})
    return t.train_loss, t.train_loss_cls, t.train_loss_bb, t.valid_loss


def test_trainer_through_a_dropout(rg, graphs):
    plain = fit(rg, graphs, None)
    same = fit(rg, graphs, rg.subgraph.RandomNodeDropout(0.0))
    assert same == plain                                           # p = 0 hands the trainer the input's values: equal floats
    gen = torch.Generator(device="cuda").manual_seed(5)
    dropped = fit(rg, graphs, rg.subgraph.RandomNodeDropout(0.3, generator=gen, degree="recompute", node_features=NODE_FEATURES))
    print(f"[subgraph trainer] plain {plain[0]}, p = 0.3 {dropped[0]}")
    assert all(len(l) == 1 and all(math.isfinite(v) for v in l) for l in dropped)
    assert dropped[0] != plain[0]
