"""``Trainer.fit`` on a training loader wrapped in ``TransformedLoader`` with a seeded ``RandomRigidMotion``: two epochs on four
tiny graphs, run twice.  The two runs must give the same loss lists bit for bit (the motions come from a seeded device generator,
nothing else is random), the ``GraphStore``'s resident tensors must be untouched, the transform must have seen the training
batches only (validation batches are not transformed), and it must have had an effect (the losses of a plain run differ)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BG = 5
WEIGHTS = {"car": 1.0, "pedestrian": 2.0, "pedestrian_group": 1.5, "two_wheeler": 3.0, "large_vehicle": 0.7, "background": 0.1}


@pytest.fixture(scope="module")
def rg():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    import radargnn_amd
    from radargnn_amd import data, frames, gnn, synthetic, transforms          # noqa: F401
    from radargnn_amd.gnn import trainer                                        # noqa: F401
    return radargnn_amd


@pytest.fixture(scope="module")
def graphs(rg):
    """four graphs of 30-45 points (5 nearest neighbours, the shipped feature lists) with pos, vel and rotated boxes relative to
    their points (bb_invariance "translation"); background rows carry NaN boxes"""
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
    return settings, out


class Counting:
    def __init__(self, transform):
        self.transform, self.calls, self.graphs = transform, 0, 0

    def __call__(self, batch):
        self.calls += 1
        self.graphs += batch.num_graphs
        return self.transform(batch)


def fit(rg, settings, graph_list, augment: bool):
    cfg = rg.gnn.TrainingConfig(dataset="radarscenes", learning_rate=5e-3, epochs=2, batch_size=2, shuffle=False, bg_index=BG,
                                class_weights=dict(WEIGHTS), val_class_weights=dict(WEIGHTS), adapt_orientation_angle=True)
    arch = rg.gnn.GNNArchitectureConfig(node_feature_dimension=5, edge_feature_dimension=2, conv_layer_dimensions=[16, 8],
                                        classification_head_layer_dimensions=[6], regression_head_layer_dimensions=[8, 5],
                                        initial_node_feature_embedding=True, initial_edge_feature_embedding=True,
                                        node_feature_embedding_layer_dimensions=[8, 16],
                                        edge_feature_embedding_layer_dimensions=[4, 8], conv_layer_type="MPNNConv",
                                        batch_norm_in_mlps=False)
    torch.manual_seed(0)
    model = rg.gnn.DetNetBasic(arch).cuda()
    store = rg.data.GraphStore(graph_list)
    kept = {k: v.clone() for k, v in store.resident.items()}
    train = rg.data.DataLoader(store, batch_size=2, shuffle=False)
    valid = rg.data.DataLoader(rg.data.GraphStore(graph_list[:2]), batch_size=2, shuffle=False)
    counter = None
    if augment:
        gen = torch.Generator(device="cuda").manual_seed(1234)
        counter = Counting(rg.transforms.RandomRigidMotion(settings, False, "translation", math.pi, 5.0, generator=gen))
        train = rg.transforms.TransformedLoader(train, counter)
    t = rg.gnn.trainer.Trainer(cfg, model)
    t.fit({"train": train, "validate": valid})
    for k, v in store.resident.items():                                         # the resident dataset is left alone
        assert torch.equal(v.view(torch.uint8), kept[k].view(torch.uint8)), k                # bit for bit (y holds NaN rows)
    return t, counter


def test_training_through_a_transformed_loader_is_repeatable(rg, graphs):
    settings, graph_list = graphs
    a, seen_a = fit(rg, settings, graph_list, True)
    b, seen_b = fit(rg, settings, graph_list, True)
    lists = lambda t: (t.train_loss, t.train_loss_cls, t.train_loss_bb, t.valid_loss)
    print(f"[rigid trainer] train {a.train_loss}, valid {a.valid_loss}")
    assert all(len(l) == 2 and all(math.isfinite(v) for v in l) for l in lists(a))
    assert lists(a) == lists(b)                                                  # floats compared exactly: bit-equal runs
    # 2 epochs x 2 training batches of 2 graphs; the validation loader's batches never reached the transform
    assert (seen_a.calls, seen_a.graphs) == (4, 8) and (seen_b.calls, seen_b.graphs) == (4, 8)
    plain, _ = fit(rg, settings, graph_list, False)
    assert plain.train_loss != a.train_loss                                      # the motions were seen by the model
