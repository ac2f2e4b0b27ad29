"""CPU-only checks of the training front end: ``TrainingConfig`` against the reference's field list (gnn/configs.py:33-100), the
trainer's epoch-end bookkeeping on plain floats (derived by hand from gnn/trainer.py:74-87,116-146), the numbering of result
folders (trainer.py:394-436) and the import path ``train.py`` uses."""
import dataclasses
import os

import pytest
import torch

from radargnn_amd.gnn.configs import TrainingConfig
from radargnn_amd.gnn.trainer import Trainer, get_new_result_folder_path, radar_scenes_class_weights, set_seeds

FIELDS = [("dataset", dataclasses.MISSING), ("learning_rate", dataclasses.MISSING), ("epochs", dataclasses.MISSING),
          ("batch_size", dataclasses.MISSING), ("shuffle", dataclasses.MISSING), ("bg_index", dataclasses.MISSING),
          ("deterministic", False), ("seed", 0), ("class_weights", {}), ("set_weights_according_radar_scenes_distribution", False),
          ("val_class_weights", {}), ("bb_loss_weight", 1), ("cls_loss_weight", 1), ("regularization_strength", 1e-4),
          ("reduce_lr_on_plateau_factor", 0.5), ("reduce_lr_on_plateau_patience", 0), ("exponential_lr_decay_factor", 0.0),
          ("early_stopping_patience", 10), ("adapt_orientation_angle", False)]


def config(dataset="radarscenes", **kw):
    return TrainingConfig(dataset, 1e-3, 10, 2, False, 5, **kw)


def test_training_config_fields_order_and_defaults():
    got = []
    for f in dataclasses.fields(TrainingConfig):
        default = f.default_factory() if f.default_factory is not dataclasses.MISSING else f.default
        got.append((f.name, default))
    assert got == FIELDS
    c = TrainingConfig("radarscenes", 1e-3, 10, 2, False, 5)               # the six required fields, positionally
    assert (c.learning_rate, c.epochs, c.batch_size, c.shuffle, c.bg_index) == (1e-3, 10, 2, False, 5)


def test_training_config_default_class_weights():
    c = config("radarscenes")
    assert list(c.class_weights.items()) == [("car", 1), ("pedestrian", 1), ("pedestrian_group", 1), ("two_wheeler", 1),
                                             ("large_vehicle", 1), ("background", 0.05)]
    c = config("nuscenes")
    assert list(c.class_weights.items()) == [("background", 0.05), ("barrier", 1), ("bicycle", 1), ("bus", 1), ("car", 1),
                                             ("construction", 1), ("motorcycle", 1), ("pedestrian", 1), ("trafficcone", 1),
                                             ("trailer", 1), ("truck", 1)]
    c = config("radarscenes", class_weights={"car": 3.0, "background": 0.2})   # given weights stay, in the order given
    assert c.class_weights["car"] == 3.0 and c.class_weights["background"] == 0.2 and c.class_weights["pedestrian"] == 1
    assert list(c.class_weights)[:2] == ["car", "background"] and len(c.class_weights) == 6


def test_training_config_unknown_dataset_raises():
    with pytest.raises(ValueError):
        config("kitti")


def test_training_config_validation_weights():
    c = config("radarscenes")
    assert c.val_class_weights is c.class_weights                           # empty -> the training weights
    val = {"car": 2, "pedestrian": 2, "pedestrian_group": 2, "two_wheeler": 2, "large_vehicle": 2, "background": 1}
    c = config("radarscenes", val_class_weights=dict(val))
    assert c.val_class_weights == val and c.class_weights["background"] == 0.05
    with pytest.raises(AssertionError):
        config("radarscenes", val_class_weights={"car": 1.0, "truck": 1.0})


def test_radar_scenes_distribution_weights():
    w = radar_scenes_class_weights()
    assert list(w) == ["car", "pedestrian", "pedestrian group", "two wheeler", "large vehicle", "background"]
    assert w["two wheeler"] == 1.0
    assert w["car"] == pytest.approx(2.7e5 / 2.1e6, rel=1e-12) and w["background"] == pytest.approx(2.7e5 / 1.3e8, rel=1e-12)
    t, v = Trainer(config(set_weights_according_radar_scenes_distribution=True), None).class_weight_tensors("cpu")
    assert t.dtype == torch.float32 and torch.equal(t, v) and t.tolist() == pytest.approx(list(w.values()), rel=1e-6)
    val = {"car": 2, "pedestrian": 2, "pedestrian_group": 2, "two_wheeler": 2, "large_vehicle": 2, "background": 1}
    t, v = Trainer(config(val_class_weights=val), None).class_weight_tensors("cpu")
    assert t.tolist() == pytest.approx([1, 1, 1, 1, 1, 0.05]) and v.tolist() == [2, 2, 2, 2, 2, 1]


def test_epoch_bookkeeping_lowest_validation_and_early_stopping():
    """valid = [3, 2, 2, 2.5, 2.6, 1.0], patience 2.  By hand from trainer.py:128-146: epoch 1 sets the best (3); epoch 2 lowers it
    (2); epoch 3 ties (2 <= 2: the LATER epoch is kept) and 2 > 2 is false, so the count is reset; epochs 4 and 5 are above the best:
    count 1, then 2 >= patience -> stop after epoch 5; the 1.0 of epoch 6 is never seen."""
    tr = Trainer(config(early_stopping_patience=2), None)
    valid = [3, 2, 2, 2.5, 2.6, 1.0]
    stops, triggers, lowest = [], [], []
    for epoch, v in enumerate(valid, start=1):
        stop = tr.end_epoch(epoch, 10.0 - epoch, 6.0 - epoch, 4.0, v)
        stops.append(stop); triggers.append(tr.early_stopping_triggers); lowest.append(tr.model_lowest_valid["epoch"])
        if stop:
            break
    assert stops == [False, False, False, False, True]
    assert triggers == [0, 0, 0, 1, 2]
    assert lowest == [1, 2, 3, 3, 3]
    assert tr.valid_loss == [3, 2, 2, 2.5, 2.6] and tr.train_loss == [9.0, 8.0, 7.0, 6.0, 5.0]
    assert tr.train_loss_cls == [5.0, 4.0, 3.0, 2.0, 1.0] and tr.train_loss_bb == [4.0] * 5


def test_epoch_bookkeeping_keeps_a_copy_of_the_model():
    model = torch.nn.Linear(2, 2)
    tr = Trainer(config(), model)
    tr.end_epoch(1, 1.0, 0.5, 0.5, 1.0)
    kept = tr.model_lowest_valid["model"]
    with torch.no_grad():
        model.weight.add_(1.0)
    assert kept is not model and not torch.equal(kept.weight, model.weight)


def _optimizer(lr=0.1):
    return torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)


def test_scheduler_choice_plateau_is_fed_the_validation_loss():
    tr = Trainer(config(reduce_lr_on_plateau_patience=1, reduce_lr_on_plateau_factor=0.5, exponential_lr_decay_factor=0.9), None)
    opt = _optimizer()
    sched = tr.make_scheduler(opt)
    assert isinstance(sched, torch.optim.lr_scheduler.ReduceLROnPlateau)     # the plateau patience wins over the exponential factor
    for epoch, v in enumerate([1.0, 1.0, 1.0], start=1):                    # no improvement for more than `patience` epochs
        tr.end_epoch(epoch, 0.0, 0.0, 0.0, v, sched)
    assert opt.param_groups[0]["lr"] == pytest.approx(0.05)
    assert sched.best == 1.0                                                 # it saw the validation loss, not the training loss


def test_scheduler_choice_exponential_and_constant():
    tr = Trainer(config(exponential_lr_decay_factor=0.5), None)
    opt = _optimizer()
    sched = tr.make_scheduler(opt)
    assert isinstance(sched, torch.optim.lr_scheduler.ExponentialLR)
    for epoch in (1, 2):
        tr.end_epoch(epoch, 0.0, 0.0, 0.0, 1.0 / epoch, sched)
    assert opt.param_groups[0]["lr"] == pytest.approx(0.025)
    tr = Trainer(config(), None)
    opt = _optimizer()
    sched = tr.make_scheduler(opt)
    assert isinstance(sched, torch.optim.lr_scheduler.LambdaLR)
    for epoch in (1, 2, 3):
        tr.end_epoch(epoch, 0.0, 0.0, 0.0, 1.0 / epoch, sched)
    assert opt.param_groups[0]["lr"] == 0.1


def test_result_folder_numbering(tmp_path):
    parent = str(tmp_path)
    assert get_new_result_folder_path(parent) == f"{parent}/model_01"
    os.mkdir(tmp_path / "model_09")
    assert get_new_result_folder_path(parent) == f"{parent}/model_10"
    other = tmp_path / "other"
    os.mkdir(other)
    os.mkdir(other / "model_02"); os.mkdir(other / "model_11")
    assert get_new_result_folder_path(str(other)) == f"{other}/model_12"


def test_reference_import_paths_resolve_here():
    from gnnradarobjectdetection.gnn import configs as ref_configs
    from gnnradarobjectdetection.gnn import trainer as ref_trainer
    assert ref_trainer.Trainer is Trainer and ref_trainer.set_seeds is set_seeds
    assert ref_configs.TrainingConfig is TrainingConfig


def test_set_seeds_reseeds_every_generator():
    import random
    import numpy as np
    set_seeds(7)
    a = (random.random(), float(np.random.rand()), float(torch.rand(1)))
    set_seeds(7)
    assert a == (random.random(), float(np.random.rand()), float(torch.rand(1)))


def test_fused_adam_refuses_what_it_does_not_implement():
    from radargnn_amd.optim import FusedAdam
    p = torch.nn.Parameter(torch.zeros(3))
    for flag in ("amsgrad", "maximize", "decoupled_weight_decay", "capturable", "differentiable"):
        with pytest.raises(ValueError):
            FusedAdam([p], **{flag: True})
    opt = FusedAdam([p], lr=1e-2, weight_decay=1e-4)
    assert list(opt.param_groups[0]) == list(torch.optim.Adam([p]).param_groups[0])     # torch's keys in torch's order
    p.grad = torch.ones(3)
    with pytest.raises(TypeError):                                           # a CPU parameter: refused before anything is launched
        opt.step()
    assert not opt.state[p]
