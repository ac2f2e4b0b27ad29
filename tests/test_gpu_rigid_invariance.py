"""The device chain is invariant under rigid motions of the cloud: frames -> neighbour search -> features -> DetNetBasic (train
mode) on a cloud and on ``transform_frames`` of it give the same edges and, with invariant features only, the same logits and boxes.
No third-party semantics are involved: the property is the model's own (the reference's paper is about exactly this).

Input conditions, asserted on the CPU with oracle/graph_oracle.py on BOTH clouds, so that the two neighbour searches cannot
legitimately disagree: no duplicate points, no pair with |d^2 - r^2| <= 1e-9 r^2, every point's k-th and (k+1)-th neighbours apart
by more than 1e-9 relative, no status bit set on the device.

Bar: logits and boxes norm-wise (max |a - b| / max |b|) within 2e-5 = twice the project's 1e-5 parity bar (each side may be that far
from the exact value).  Should the chain be further off, the test falls back on the float64 oracle's own difference between the two
graphs (what the float32 rounding of the features alone does to the exact model) plus twice the reference-shaped float32
evaluation's error, as tests/test_gpu_aggr_ext.py computes it, and reports which bar it used.  A configuration that is NOT
invariant (``spatial_coordinates`` among the node features) must move by more than that bar: the test can fail."""
import copy
import math

import numpy as np
import pytest
import torch

from oracle import gnn_oracle, graph_oracle

pytestmark = pytest.mark.gpu

K, R = 10, 1.0
INVARIANT_NODES = ("rcs", "velocity_vector_length", "time_index", "degree")
INVARIANT_EDGES = ("point_pair_features", "spatial_euclidean_distance", "velocity_euclidean_distance")
MOVING_NODES = ("rcs", "spatial_coordinates", "time_index", "degree")
ANGLE = np.array([2.3, -0.7, math.pi])
SHIFT = np.array([[12.5, -7.25], [-3.0, 18.0], [0.0, 9.5]])


def normwise(a, b) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


@pytest.fixture(scope="module")
def clouds():
    """(original FrameBatch, moved FrameBatch): 3 synthetic frames of 300, 251 and 130 points"""
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    from radargnn_amd import frames, synthetic, transforms
    batch = frames.FrameBatch.from_frames([synthetic.small_frame(n, seed=40 + i) for i, n in enumerate((300, 251, 130))])
    moved = transforms.transform_frames(batch, transforms.RigidMotion(ANGLE, SHIFT))
    return batch, moved


def test_input_conditions(clouds):
    for name, fb in zip(("original", "moved"), clouds):
        X, ptr = fb.X.cpu().numpy(), fb.frame_ptr.cpu().numpy()
        for f in range(len(ptr) - 1):
            d2 = graph_oracle._reduced_distances(X[ptr[f]:ptr[f + 1]], X[ptr[f]:ptr[f + 1]])
            np.fill_diagonal(d2, np.inf)
            assert d2.min() > 0.0, (name, f, "duplicate points")
            assert not (np.abs(d2 - R * R) <= 1e-9 * R * R).any(), (name, f, "a pair at the radius")
            near = np.sort(d2, axis=1)
            gap = (near[:, K] - near[:, K - 1]) / near[:, K]
            assert gap.min() > 1e-9, (name, f, "k-th and (k+1)-th neighbour tie", gap.min())


def build_model(dn: int, de: int, seed: int = 5):
    import radargnn_amd.gnn as gnn
    cfg = gnn.GNNArchitectureConfig(
        node_feature_dimension=dn, edge_feature_dimension=de, conv_layer_dimensions=[24, 16],
        classification_head_layer_dimensions=[6], regression_head_layer_dimensions=[16, 5],
        initial_node_feature_embedding=True, initial_edge_feature_embedding=True,
        node_feature_embedding_layer_dimensions=[16, 24], edge_feature_embedding_layer_dimensions=[8, 8],
        conv_layer_type="MPNNConv", batch_norm_in_mlps=False, aggregation_function="max")
    torch.manual_seed(seed)
    model = gnn.DetNetBasic(cfg).cuda()
    with torch.no_grad():
        for bn in model.batch_norms:
            bn.module.weight.uniform_(0.5, 1.5)
            bn.module.bias.uniform_(-0.5, 0.5)
    return model.train()


def chain(model, settings, fb):
    from radargnn_amd import frames
    cls, bb, g = frames.HotPath(copy.deepcopy(model), settings)(fb)
    g.check()
    assert int(g.status.item()) == 0                                        # no status bit set
    return cls, bb, g


def fallback_bar(model, g_a, g_b, nm):
    """|float64 oracle on graph a - on graph b| + 2 x the reference-shaped float32 evaluation's own error (norm-wise)"""
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    run = lambda g, dt: gnn_oracle.det_net_basic(g.x.cpu(), g.edge_index.cpu(), g.edge_attr.cpu(), sd, "MPNNConv", "max", True, dt)
    i = 0 if nm == "logits" else 1
    a64, b64, b32 = run(g_a, torch.float64)[i], run(g_b, torch.float64)[i], run(g_b, torch.float32)[i]
    return normwise(a64, b64) + 2 * normwise(b32, b64)


@pytest.mark.parametrize("algorithm", ["knn", "radius"])
def test_the_chain_does_not_see_a_rigid_motion(clouds, algorithm):
    from radargnn_amd import frames
    original, moved = clouds
    settings = frames.GraphSettings(algorithm=algorithm, k=K, r=R, node_features=INVARIANT_NODES, edge_features=INVARIANT_EDGES)
    model = build_model(4, 6)
    cls_a, bb_a, g_a = chain(model, settings, original)
    cls_b, bb_b, g_b = chain(model, settings, moved)
    edges_a = graph_oracle.canonical_edges(g_a.edge_index.t().cpu().numpy())
    edges_b = graph_oracle.canonical_edges(g_b.edge_index.t().cpu().numpy())
    assert edges_a.shape[0] > 0 and np.array_equal(edges_a, edges_b)
    bars = {}
    for nm, a, b in (("logits", cls_a, cls_b), ("boxes", bb_a, bb_b)):
        err, bar = normwise(b, a), 2e-5
        if err > bar:
            bar = fallback_bar(model, g_a, g_b, nm)
        print(f"[rigid invariance] {algorithm} {nm}: moved against original {err:.2e} (bar {bar:.2e}), {edges_a.shape[0]} edges")
        assert err <= bar, (nm, err, bar)
        bars[nm] = bar

    # the same chain with coordinates among the node features is NOT invariant: it must move by more than the bar
    settings = frames.GraphSettings(algorithm=algorithm, k=K, r=R, node_features=MOVING_NODES, edge_features=INVARIANT_EDGES)
    model = build_model(5, 6)
    cls_a, bb_a, _ = chain(model, settings, original)
    cls_b, bb_b, _ = chain(model, settings, moved)
    for nm, a, b in (("logits", cls_a, cls_b), ("boxes", bb_a, bb_b)):
        err = normwise(b, a)
        print(f"[rigid invariance] {algorithm} {nm} with spatial_coordinates: moved against original {err:.2e} (must exceed {bars[nm]:.2e})")
        assert err > bars[nm]
