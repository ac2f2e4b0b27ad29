"""``radargnn_amd.inference.Predictor`` -- the reference's inference driver (postprocessor/inference.py:5-75) over steps of several
loader batches -- against what it replaces: one ``model(batch.x, batch.edge_index, batch.edge_attr)`` plus ``ops.softmax_rows``
per loader batch on a deep copy of the model, and against the float64 oracle run per loader batch.

Bars: 4e-6 norm-wise between the batched and the batch-by-batch launches and ``rtol=2e-5, atol=1e-6`` for the running statistics
(what tests/test_gpu_frame_bn.py sets for per-frame statistics in a batched launch), 1e-5 norm-wise against the float64 oracle
(the project's bar); ground truth, positions and velocities are copies: bit for bit.

Seven small graphs (2 .. 257 nodes: below, at and above the wave and the 256-row block of the epilogue kernel; the 65-node one has
a node without incoming edges), ``y`` float64 with six columns of distinct values, the small train-mode ``DetNetBasic`` of
tests/test_gpu_postprocess.py::test_pipeline_loader_model_softmax_decode_nms.  The batch-by-batch and the oracle results are
computed once per loader batch size and shared."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(2, 3), (3, 5), (64, 300), (65, 200), (130, 700), (200, 1500), (257, 900)]
NO_IN_EDGES = 3                        # graph 3 (65 nodes): its last node is no edge's target
KEYS = ("prob", "bb", "class_true", "bb_true", "pos", "vel")


def normwise(a, b) -> float:
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def make_graphs(realistic_y: bool = False):
    from radargnn_amd import data as D
    g = torch.Generator().manual_seed(5)
    graphs = []
    for i, (n, e) in enumerate(SIZES):
        ei = torch.randint(0, n, (2, e), generator=g)
        if i == NO_IN_EDGES:
            ei[1] = torch.randint(0, n - 1, (e,), generator=g)
        if realistic_y:     # labels 0 .. 5 (5 = background) and plausible boxes: what the post-processor expects
            y = torch.cat((torch.randint(0, 6, (n, 1), generator=g).double(), torch.randn(n, 5, generator=g).double()), 1)
            y[:, 3:5] = y[:, 3:5].abs() + 0.5
        else:               # every element its own value
            y = (torch.arange(n * 6, dtype=torch.float64).view(n, 6) * 0.5 + 1000.0 * i + 0.25)
        graphs.append(D.Data(x=torch.randn(n, 5, generator=g), edge_index=ei, edge_attr=torch.randn(e, 2, generator=g), y=y,
                             pos=torch.rand(n, 2, generator=g) * 40, vel=torch.randn(n, 2, generator=g) + 10.0 * i))
    return graphs


def make_model():
    from radargnn_amd import gnn
    cfg = gnn.GNNArchitectureConfig(node_feature_dimension=5, edge_feature_dimension=2, conv_layer_dimensions=[16, 8],
                                    classification_head_layer_dimensions=[6], regression_head_layer_dimensions=[8, 5],
                                    initial_node_feature_embedding=True, initial_edge_feature_embedding=True,
                                    node_feature_embedding_layer_dimensions=[8, 16], edge_feature_embedding_layer_dimensions=[4, 8],
                                    conv_layer_type="MPNNConv", batch_norm_in_mlps=False)
    torch.manual_seed(3)
    return gnn.DetNetBasic(cfg)


class World:
    """Model, graphs, and per loader batch size: the batch-by-batch device results, the model they leave behind, the oracle's."""

    def __init__(self):
        self.graphs = make_graphs()
        self.model = make_model()
        self.sd = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        self.model.cuda().train()
        self._seq = {}

    def fresh(self):
        return copy.deepcopy(self.model)

    def loader(self, batch_size, **kw):
        from radargnn_amd import data as D
        return D.DataLoader(self.graphs, batch_size=batch_size, **kw)

    def groups(self, batch_size, order=None):
        order = list(range(len(self.graphs))) if order is None else list(order)
        return [order[i:i + batch_size] for i in range(0, len(order), batch_size)]

    def sequential(self, batch_size):
        """One forward + ``ops.softmax_rows`` per loader batch on a deep copy (the loop Predictor replaces) and the oracle in
        float64 on the same concatenated graphs -> {"prob", "bb", "prob64", "bb64": lists per loader batch, "model": the copy}."""
        if batch_size not in self._seq:
            from oracle import gnn_oracle
            from radargnn_amd import ops
            model = self.fresh()
            out = {"prob": [], "bb": [], "prob64": [], "bb64": [], "model": model}
            with torch.no_grad():
                for batch in self.loader(batch_size):
                    cls, bb = model(batch.x, batch.edge_index, batch.edge_attr)
                    out["prob"].append(ops.softmax_rows(cls)); out["bb"].append(bb)
            for ids in self.groups(batch_size):
                gs = [self.graphs[i] for i in ids]
                off = np.concatenate(([0], np.cumsum([g.num_nodes for g in gs])))
                c64, b64 = gnn_oracle.det_net_basic(torch.cat([g.x for g in gs]),
                                                    torch.cat([g.edge_index + int(o) for g, o in zip(gs, off)], 1),
                                                    torch.cat([g.edge_attr for g in gs]), self.sd, dtype=torch.float64)
                out["prob64"].append(torch.softmax(c64, 1)); out["bb64"].append(b64)
            self._seq[batch_size] = out
        return self._seq[batch_size]


@pytest.fixture(scope="module")
def W():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return World()


def run(W, loader, model=None, **kw):
    from radargnn_amd.inference import Predictor
    model = W.fresh() if model is None else model
    predictions, ground_truth, pos, vel = Predictor(model, loader, verbose=kw.pop("verbose", False), **kw).predict()
    assert set(predictions) == {"bounding_box_predictions", "class_probability_prediction"}
    assert set(ground_truth) == {"bounding_box_true", "class_true"}
    res = {"prob": predictions["class_probability_prediction"], "bb": predictions["bounding_box_predictions"],
           "class_true": ground_truth["class_true"], "bb_true": ground_truth["bounding_box_true"], "pos": pos, "vel": vel}
    assert all(isinstance(res[k], list) for k in KEYS)
    return res, model


def check_against_sequential(W, res, batch_size, groups=None, seq_index=None, tag=""):
    """Logits-derived outputs against the batch-by-batch launches (4e-6) and the oracle (1e-5), entry by entry; the copies
    bit for bit against the graphs' own tensors."""
    seq = W.sequential(batch_size)
    groups = W.groups(batch_size) if groups is None else groups
    seq_index = list(range(len(groups))) if seq_index is None else seq_index
    assert all(len(res[k]) == len(groups) for k in KEYS)
    worst_hip = worst_64 = 0.0
    for e, (ids, s) in enumerate(zip(groups, seq_index)):
        n = sum(W.graphs[i].num_nodes for i in ids)
        assert res["prob"][e].shape == (n, 6) and res["bb"][e].shape == (n, 5)
        worst_hip = max(worst_hip, normwise(res["bb"][e], seq["bb"][s]), normwise(res["prob"][e], seq["prob"][s]))
        worst_64 = max(worst_64, normwise(res["bb"][e], seq["bb64"][s]), normwise(res["prob"][e], seq["prob64"][s]))
        y = torch.cat([W.graphs[i].y for i in ids])
        for key, want in (("class_true", y[:, 0]), ("bb_true", y[:, 1:]), ("pos", torch.cat([W.graphs[i].pos for i in ids])),
                          ("vel", torch.cat([W.graphs[i].vel for i in ids]))):
            got = torch.as_tensor(res[key][e]).cpu()
            assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), (tag, key, e)
    print(f"[predictor] {tag}: vs batch-by-batch {worst_hip:.2e} (bar 4e-6), vs float64 oracle {worst_64:.2e} (bar 1e-5)")
    assert worst_hip < 4e-6, (tag, worst_hip)
    assert worst_64 < 1e-5, (tag, worst_64)


def check_buffers(model, other):
    for (name, a), (_, b) in zip(model.named_buffers(), other.named_buffers()):
        if a.dtype.is_floating_point:
            np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-5, atol=1e-6, err_msg=name)
        else:
            assert torch.equal(a, b), name


def check_views(res):
    """Every list holds contiguous views of ONE buffer, laid back to back."""
    for key in KEYS:
        entries = res[key]
        base = entries[0].untyped_storage().data_ptr()
        at = entries[0].data_ptr()
        for t in entries:
            assert t.is_cuda and t.is_contiguous() and t.untyped_storage().data_ptr() == base and t.data_ptr() == at, key
            at += t.numel() * t.element_size()


@pytest.mark.parametrize("graphs_per_step", [1, 3, 100])
def test_reference_regime_one_graph_per_loader_batch(W, graphs_per_step):
    loader = W.loader(1)
    store_before = {k: v.clone() for k, v in loader.store.resident.items()}
    res, model = run(W, loader, graphs_per_step=graphs_per_step)
    check_against_sequential(W, res, 1, tag=f"batch_size=1 graphs_per_step={graphs_per_step}")
    check_buffers(model, W.sequential(1)["model"])
    check_views(res)
    assert model.training
    assert int(model.batch_norms[0].module.num_batches_tracked) == len(W.graphs)
    for k, v in loader.store.resident.items():                       # the loader's resident graphs are not written ...
        assert torch.equal(v, store_before[k]), k
    for (name, p), (_, q) in zip(model.named_parameters(), W.model.named_parameters()):     # ... nor the parameters
        assert torch.equal(p, q), name


def test_loader_batches_of_three_take_their_statistics_per_loader_batch(W):
    res, model = run(W, W.loader(3), graphs_per_step=4)              # steps: loader batches {0, 1} (6 graphs), {2} (1 graph)
    check_against_sequential(W, res, 3, tag="batch_size=3 graphs_per_step=4")
    check_buffers(model, W.sequential(3)["model"])
    check_views(res)
    assert int(model.batch_norms[0].module.num_batches_tracked) == 3
    one = W.sequential(1)
    assert normwise(torch.cat(res["bb"]), torch.cat(one["bb"])) > 1e-4        # the two scopes are different functions


def test_a_shuffling_loader_keeps_its_permutation(W):
    seed = 12
    order = torch.randperm(len(W.graphs), generator=torch.Generator().manual_seed(seed)).tolist()
    assert order != sorted(order)
    for batch_size, gps in ((1, 3), (3, 4)):
        loader = W.loader(batch_size, shuffle=True, generator=torch.Generator().manual_seed(seed))
        res, _ = run(W, loader, graphs_per_step=gps)
        groups = W.groups(batch_size, order)
        if batch_size == 1:              # train-mode outputs of a one-graph batch do not depend on what ran before it
            check_against_sequential(W, res, 1, groups=groups, seq_index=[ids[0] for ids in groups], tag="shuffled batch_size=1")
        else:                            # other groups than the unshuffled loader's: the copies and the node counts
            for e, ids in enumerate(groups):
                y = torch.cat([W.graphs[i].y for i in ids])
                assert torch.equal(res["class_true"][e].cpu(), y[:, 0]) and torch.equal(res["bb_true"][e].cpu(), y[:, 1:])
                assert torch.equal(res["pos"][e].cpu(), torch.cat([W.graphs[i].pos for i in ids]))
                assert torch.equal(res["vel"][e].cpu(), torch.cat([W.graphs[i].vel for i in ids]))
                assert res["prob"][e].shape[0] == y.shape[0] and res["bb"][e].shape[0] == y.shape[0]


def test_eval_mode_is_the_plain_batched_forward(W):
    from radargnn_amd import ops
    model = W.fresh().eval()
    before = {k: v.clone() for k, v in model.named_buffers()}
    res, model = run(W, W.loader(1), model=model, graphs_per_step=3)
    assert not model.training
    plain = W.fresh().eval()
    store = W.loader(1).store
    at = 0
    with torch.no_grad():
        for ids in ([0, 1, 2], [3, 4, 5], [6]):
            batch = store.collate(ids)
            cls, bb = plain(batch.x, batch.edge_index, batch.edge_attr)          # no frame_ptr
            prob = ops.softmax_rows(cls)
            ptr = batch.ptr.cpu().tolist()
            for j in range(len(ids)):
                assert torch.equal(res["prob"][at], prob[ptr[j]:ptr[j + 1]]) and torch.equal(res["bb"][at], bb[ptr[j]:ptr[j + 1]]), at
                at += 1
    for k, v in model.named_buffers():                               # running statistics stand still in eval mode
        assert torch.equal(v, before[k]), k


def test_a_plain_list_of_batches_gets_one_forward_per_batch(W):
    batches = list(W.loader(1))
    assert type(batches) is list
    res, model = run(W, batches, graphs_per_step=100)
    check_against_sequential(W, res, 1, tag="list of Batch")
    check_buffers(model, W.sequential(1)["model"])
    seq = W.sequential(1)
    for e in range(len(batches)):                                    # the very launches of the loop: the same bits
        assert torch.equal(res["prob"][e], seq["prob"][e]) and torch.equal(res["bb"][e], seq["bb"][e])


@pytest.mark.parametrize("resident", [True, False])
def test_to_host_gives_the_references_numpy_entries(W, resident):
    loader = W.loader(1) if resident else list(W.loader(1))
    dev, _ = run(W, loader, graphs_per_step=3)
    host, _ = run(W, W.loader(1) if resident else list(W.loader(1)), graphs_per_step=3, to_host=True)
    want = {"prob": (np.float32, (6,)), "bb": (np.float32, (5,)), "class_true": (np.float64, ()), "bb_true": (np.float64, (5,)),
            "pos": (np.float32, (2,)), "vel": (np.float32, (2,))}
    for key in KEYS:
        assert len(host[key]) == len(W.graphs)
        for e, (n, _) in enumerate(SIZES):
            a = host[key][e]
            assert isinstance(a, np.ndarray) and a.dtype == want[key][0] and a.shape == (n,) + want[key][1], (key, e)
            assert np.array_equal(a.view(np.int32 if a.dtype == np.float32 else np.int64),
                                  dev[key][e].cpu().numpy().view(np.int32 if a.dtype == np.float32 else np.int64)), (key, e)
        if resident:                                                 # views of ONE host copy per buffer
            assert all(a.base is not None for a in host[key])


def test_hand_over_to_postprocessor_and_prediction_extractor(W):
    """``Postprocessor.process`` and ``PredictionExtractor.extract`` take the returned lists as they are and give, frame for frame,
    what they give on per-frame arrays built by hand from the same values (numpy, as the reference's Predictor returns them)."""
    from radargnn_amd import data as D, postprocessor as P
    from radargnn_amd.inference import Predictor
    graphs = make_graphs(realistic_y=True)
    pred, gt, pos, vel = Predictor(W.fresh(), D.DataLoader(graphs, batch_size=1), verbose=False, graphs_per_step=3).predict()
    host = lambda lst: [t.cpu().numpy().copy() for t in lst]
    pred_h, gt_h = {k: host(v) for k, v in pred.items()}, {k: host(v) for k, v in gt.items()}
    pos_h, vel_h = host(pos), host(vel)
    cfg = P.PostProcessingConfiguration(split="t", iou_for_nms=0.1, min_object_score={c: 0.05 for c in "abcde"},
                                        max_score_for_background=0.6, bg_index=5, bb_invariance="translation")
    got = P.Postprocessor().process(cfg, pos, vel, pred, gt)
    want = P.Postprocessor().process(cfg, pos_h, vel_h, pred_h, gt_h)
    same = lambda a, b: torch.equal(torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu())
    n_boxes = 0
    for f in range(len(graphs)):
        (bp, bg_, cp, cg), (bp2, bg2, cp2, cg2) = [part[f] for part in got], [part[f] for part in want]
        assert same(bp["boxes"].corners, bp2["boxes"].corners) and same(bp["scores"], bp2["scores"]) and same(bp["labels"], bp2["labels"])
        assert same(bg_["boxes"].corners, bg2["boxes"].corners) and same(bg_["labels"], bg2["labels"])
        assert set(cp) == set(cp2) and all(same(cp[k], cp2[k]) for k in cp)
        assert set(cg) == set(cg2) and all(same(cg[k], cg2[k]) for k in cg)
        assert cp["pos"].shape == (graphs[f].num_nodes, 2)
        n_boxes += len(bp["boxes"]) + len(bg_["boxes"])
    assert n_boxes > 0
    labels, labels_h = P.PredictionExtractor().extract(pred), P.PredictionExtractor().extract(pred_h)
    assert len(labels) == len(graphs)
    for f in range(len(graphs)):
        assert labels[f].shape == (graphs[f].num_nodes, 1) and same(labels[f], labels_h[f])


@pytest.mark.parametrize("graphs_per_step", [64, 5])
def test_verbose_prints_the_references_progress_lines(W, capsys, graphs_per_step):
    from radargnn_amd import data as D
    graphs = [W.graphs[i % 3] for i in range(23)]
    capsys.readouterr()
    res, _ = run(W, D.DataLoader(graphs, batch_size=1), verbose=True, graphs_per_step=graphs_per_step)
    lines = capsys.readouterr().out.splitlines()
    assert lines == ["Device for inference: cuda"] + [f"{i}/23 inferences finished" for i in (1, 10, 20, 23)]
    assert len(res["prob"]) == 23
    run(W, D.DataLoader(graphs, batch_size=1), verbose=False)
    assert capsys.readouterr().out == ""
