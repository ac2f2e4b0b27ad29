"""``radargnn_amd.gnn.trainer.Trainer`` on the device: the orientation-angle adaptation against a float64 restatement of the
reference's rule (preprocessor/bounding_box.py:536-563), ``fit`` against the training loop this repository's tests write by hand
(collate, forward, ``detection_loss``, backward, ``torch.optim.Adam``, torch's scheduler, validation in train mode under
``no_grad``), the files ``save_results`` writes, and a batch whose box loss is NaN."""
import os

import numpy as np
import pytest
import torch

from conftest import record_parity

pytestmark = pytest.mark.gpu

BG = 5
TRAIN_WEIGHTS = {"car": 1.0, "pedestrian": 2.0, "pedestrian_group": 1.5, "two_wheeler": 3.0, "large_vehicle": 0.7, "background": 0.1}
VALID_WEIGHTS = {"car": 1.0, "pedestrian": 1.0, "pedestrian_group": 1.0, "two_wheeler": 2.0, "large_vehicle": 1.0, "background": 0.3}


@pytest.fixture(scope="module")
def rg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import radargnn_amd
    from radargnn_amd import data, frames, gnn, ops, synthetic          # noqa: F401
    from radargnn_amd.gnn import trainer                                # noqa: F401
    return radargnn_amd


# ---- 1. orientation angle ------------------------------------------------------------------------------------------------------------
def adapt_reference(y: np.ndarray) -> np.ndarray:
    """the rule in float64: rows whose first box column is not NaN get sin(theta - pi if theta > pi / 2 else theta)"""
    out = y.astype(np.float64)
    for i in range(y.shape[0]):
        if not np.isnan(y[i, 1]):
            theta = np.float64(y[i, 5])
            out[i, 5] = np.sin(theta - np.pi if theta > np.pi / 2 else theta)
    return out


def angle_case(n: int) -> np.ndarray:
    rng = np.random.Generator(np.random.PCG64(100 + n))
    half = np.float32(np.pi / 2)
    special = [np.float32(0.0), half, np.nextafter(half, np.float32(0.0)), np.nextafter(half, np.float32(4.0)), np.float32(np.pi)]
    assert float(half) > np.pi / 2                                      # float32(pi / 2) lies above pi / 2: the rule flips it to -1
    y = rng.normal(0.0, 2.0, size=(n, 6)).astype(np.float32)
    y[:, 0] = rng.integers(0, 6, size=n)
    y[:, 5] = rng.uniform(0.0, np.pi, size=n).astype(np.float32)
    if n == 1:
        y[0, 5] = half
    elif n:
        y[:len(special), 5] = special
        nan_rows = np.arange(len(special), n)[rng.uniform(size=n - len(special)) < 0.4]
        y[nan_rows, 1:] = np.nan
        y[nan_rows[0], 1:].view(np.uint32)[:] = 0x7FC12345              # a NaN with a payload: copied, not recomputed
        y[nan_rows[1], 5] = 1.0                                         # no box, but a number in the angle column: left alone
    return y


@pytest.mark.parametrize("n", [0, 1, 257])
def test_orientation_angle_adaptation(rg, n):
    y = angle_case(n)
    expect = adapt_reference(y)
    src = torch.from_numpy(y).cuda()
    wide = torch.zeros(n, 9, device="cuda"); wide[:, :6] = src          # the same rows with a row stride of 9
    for given in (src, wide[:, :6]):
        kept = given.clone()
        got_dev = rg.ops.adapt_orientation_angle(given)
        assert got_dev is not given and (n == 0 or got_dev.data_ptr() != given.data_ptr())     # out of place ...
        assert torch.equal(given.view(torch.int32), kept.view(torch.int32))                    # ... and the input is left alone
        got = got_dev.cpu().numpy()
        assert got.shape == (n, 6) and got.dtype == np.float32
        box = ~np.isnan(y[:, 1])
        err = np.abs(got[box, 5].astype(np.float64) - expect[box, 5])
        print(f"n {n}: {int(box.sum())} boxes, max error {err.max() if err.size else 0.0:.3e} (bar {2.0 ** -23:.3e})")
        assert (err <= 2.0 ** -23).all()
        same = np.ones((n, 6), dtype=bool); same[box, 5] = False      # everything else: bit for bit
        assert np.array_equal(got.view(np.uint32)[same], y.view(np.uint32)[same])
    if n == 1:
        assert got[0, 5] == -1.0
    if n == 257:
        assert got[0, 5] == 0.0 and got[1, 5] == -1.0 and got[2, 5] == 1.0 and got[3, 5] == -1.0 and abs(got[4, 5]) < 1e-6


def test_orientation_angle_needs_a_rotated_box(rg):
    with pytest.raises(ValueError):
        rg.ops.adapt_orientation_angle(torch.zeros(7, 1 + 4, device="cuda"))


# ---- 2.-4. fit -----------------------------------------------------------------------------------------------------------------------
def model_config(rg):
    return rg.gnn.GNNArchitectureConfig(node_feature_dimension=5, edge_feature_dimension=2, conv_layer_dimensions=[16, 8],
                                        classification_head_layer_dimensions=[6], regression_head_layer_dimensions=[8, 5],
                                        initial_node_feature_embedding=True, initial_edge_feature_embedding=True,
                                        node_feature_embedding_layer_dimensions=[8, 16],
                                        edge_feature_embedding_layer_dimensions=[4, 8], conv_layer_type="MPNNConv",
                                        batch_norm_in_mlps=False)


def new_model(rg, seed=0):
    torch.manual_seed(seed)
    return rg.gnn.DetNetBasic(model_config(rg)).cuda()


@pytest.fixture(scope="module")
def graphs(rg):
    """six graphs of 40-70 points (synthetic frames, 5-nearest-neighbour edges) with seeded labels and boxes; graph 3 is background
    only; background rows carry NaN boxes, as in the datasets"""
    settings = rg.frames.GraphSettings(algorithm="knn", k=5)
    out = []
    for i, n in enumerate((40, 55, 70, 48, 63, 51)):
        g = rg.frames.build_graphs(rg.frames.FrameBatch.from_frames([rg.synthetic.small_frame(n, seed=i)]), settings)
        rng = np.random.Generator(np.random.PCG64(7 + i))
        label = np.where(rng.uniform(size=n) < 0.4, rng.integers(0, BG, size=n), BG) if i != 3 else np.full(n, BG)
        box = rng.normal(0.0, 1.5, size=(n, 5))
        box[:, 4] = rng.uniform(0.0, np.pi, size=n)
        box[label == BG] = np.nan
        y = torch.tensor(np.concatenate((label.reshape(-1, 1), box), axis=1), dtype=torch.float32)
        out.append(rg.data.Data(x=g.x.cpu(), edge_index=g.edge_index.cpu(), edge_attr=g.edge_attr.cpu(), y=y))
    assert sum(int((d.y[:, 0] != BG).any()) for d in out) == 5
    return out


def loaders(rg, graph_list):
    return {"train": rg.data.DataLoader(rg.data.GraphStore(graph_list), batch_size=2, shuffle=False),
            "validate": rg.data.DataLoader(rg.data.GraphStore(graph_list[:4]), batch_size=2, shuffle=False)}


def training_config(rg, **kw):
    args = dict(dataset="radarscenes", learning_rate=5e-3, epochs=3, batch_size=2, shuffle=False, bg_index=BG,
                class_weights=dict(TRAIN_WEIGHTS), val_class_weights=dict(VALID_WEIGHTS), regularization_strength=1e-4,
                exponential_lr_decay_factor=0.9, bb_loss_weight=0.8, cls_loss_weight=1.2)
    args.update(kw)
    return rg.gnn.TrainingConfig(**args)


def hand_written_loop(rg, graph_list, cfg):
    """the loop the repository's tests and tools write by hand, with torch's optimizer and three host reads per batch"""
    model = new_model(rg)
    ld = loaders(rg, graph_list)
    opt = torch.optim.Adam(model.parameters(), lr=cfg.learning_rate, weight_decay=cfg.regularization_strength)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=cfg.exponential_lr_decay_factor)
    tw, vw = list(cfg.class_weights.values()), list(cfg.val_class_weights.values())
    curves = {"train_loss": [], "train_loss_cls": [], "train_loss_bb": [], "valid_loss": []}
    for _ in range(cfg.epochs):
        total = cls_sum = bb_sum = 0.0
        for batch in ld["train"]:
            opt.zero_grad()
            c, b = model(batch.x, batch.edge_index, batch.edge_attr)
            loss, lc, lb = rg.gnn.detection_loss(c, b, batch.y, BG, tw, cfg.cls_loss_weight, cfg.bb_loss_weight)
            loss.backward()
            opt.step()
            total += loss.item(); cls_sum += lc.item(); bb_sum += lb.item()
        valid = 0.0
        with torch.no_grad():
            for batch in ld["validate"]:
                c, b = model(batch.x, batch.edge_index, batch.edge_attr)
                valid += rg.gnn.detection_loss(c, b, batch.y, BG, vw, cfg.cls_loss_weight, cfg.bb_loss_weight)[0].item()
        sched.step()
        for key, value, count in (("train_loss", total, len(ld["train"])), ("train_loss_cls", cls_sum, len(ld["train"])),
                                  ("train_loss_bb", bb_sum, len(ld["train"])), ("valid_loss", valid, len(ld["validate"]))):
            curves[key].append(value / count)
    return curves


def largest_relative_difference(a: dict, b: dict) -> float:
    return max(abs(x - y) / max(abs(y), 1e-30) for key in b for x, y in zip(a[key], b[key]))


@pytest.fixture(scope="module")
def fitted(rg, graphs):
    cfg = training_config(rg)
    trainer = rg.gnn.trainer.Trainer(cfg, new_model(rg))
    trainer.fit(loaders(rg, graphs))
    return trainer


def test_fit_equals_the_hand_written_loop(rg, graphs, fitted):
    cfg = training_config(rg)
    first, second = hand_written_loop(rg, graphs, cfg), hand_written_loop(rg, graphs, cfg)
    spread = largest_relative_difference(second, first)                 # is the hand-written loop itself reproducible?
    got = {key: getattr(fitted, key) for key in first}
    assert all(len(got[key]) == cfg.epochs for key in got)
    diff = largest_relative_difference(got, first)
    bar = max(1e-5, 4.0 * spread)
    print(f"run-to-run spread of the hand-written loop {spread:.3e}, Trainer.fit against it {diff:.3e} (bar {bar:.3e})")
    print("hand-written:", first, "\nTrainer.fit:", got)
    record_parity("trainer_fit_vs_hand_written_loop", spread=spread, difference=diff)
    assert diff <= bar
    for key in ("train_loss", "train_loss_cls", "train_loss_bb", "valid_loss"):
        assert got[key][-1] < got[key][0], (key, got[key])              # the losses fall over the three epochs
    lowest = min(fitted.valid_loss)
    assert fitted.model_lowest_valid["epoch"] == max(i + 1 for i, v in enumerate(fitted.valid_loss) if v == lowest)
    assert fitted.model.training and fitted.nan_batches == [0, 0, 0]


def test_save_results_writes_the_reference_files(rg, fitted, tmp_path):
    fitted.save_results(str(tmp_path), model_config(rg), {"DATASET": {"name": "synthetic"}})
    folder = tmp_path / "model_01"
    epoch = fitted.model_lowest_valid["epoch"]
    assert sorted(os.listdir(folder)) == sorted([
        "gnn_configs.json", "dataset_configs.json", "trained_model.pt", "trained_model_state_dict.pt",
        f"trained_model_low_val_ep{epoch}.pt", f"trained_model_low_val_ep{epoch}_state_dict.pt",
        "loss_train.npy", "loss_validation.npy", "loss_train_cls.npy", "loss_train_bb.npy", "loss_curves.png"])
    fresh = rg.gnn.DetNetBasic(model_config(rg))
    fresh.load_state_dict(torch.load(folder / "trained_model_state_dict.pt", map_location="cpu"))
    for a, b in zip(fresh.state_dict().values(), fitted.model.state_dict().values()):
        assert torch.equal(a, b.cpu())
    whole = rg.load_reference_model(str(folder / "trained_model.pt"))
    assert isinstance(whole, rg.gnn.DetNetBasic)
    for a, b in zip(whole.state_dict().values(), fitted.model.state_dict().values()):
        assert torch.equal(a.cpu(), b.cpu())
    assert np.load(folder / "loss_validation.npy").tolist() == [fitted.valid_loss]
    fitted.save_results(str(tmp_path), model_config(rg), {})
    assert (tmp_path / "model_02").is_dir()


def test_nan_batch_is_counted_and_the_store_is_left_alone(rg, graphs):
    """an object row of graph 2 (second batch) gets a NaN box target: that batch's box loss is ignored, counted once per epoch, and
    training goes on; with ``adapt_orientation_angle`` the angles are re-encoded on the collated copy, never in the store"""
    damaged = [rg.data.Data(**{k: v.clone() for k, v in d.items()}) for d in graphs]
    row = int((damaged[2].y[:, 0] != BG).nonzero()[0])
    damaged[2].y[row, 3] = float("nan")
    ld = loaders(rg, damaged)
    resident = {k: ld[k].store.resident["y"].clone() for k in ld}
    trainer = rg.gnn.trainer.Trainer(training_config(rg, epochs=2, adapt_orientation_angle=True), new_model(rg))
    trainer.fit(ld)
    assert trainer.nan_batches == [1, 1]
    for curve in (trainer.train_loss, trainer.train_loss_cls, trainer.train_loss_bb, trainer.valid_loss):
        assert len(curve) == 2 and np.isfinite(curve).all()
    assert all(torch.isfinite(p).all() for p in trainer.model.parameters())
    for k in ld:
        assert torch.equal(ld[k].store.resident["y"].view(torch.int32), resident[k].view(torch.int32))
