"""The reference's ``Trainer`` (gnn/trainer.py) with the whole batch loop on the device.

Same surface -- ``Trainer(config, model)``, ``fit(data_loaders)``, ``save_results(path, model_config, dataset_config_dict)``,
``show_learning_curves()``, the loss lists and ``model_lowest_valid`` -- and the same observable behaviour: optimizer
hyper-parameters and the scheduler come from the ``TrainingConfig`` (trainer.py:67-87), training and validation have their own
class weights, validation runs under ``no_grad`` with the model LEFT IN TRAIN MODE (the reference never calls ``.eval()``: BatchNorm
normalises with batch statistics and keeps updating its running statistics), the scheduler steps once per epoch, the model with the
lowest validation loss (ties go to the later epoch) is kept as a deep copy, and training stops after ``early_stopping_patience``
consecutive epochs above the best validation loss.

What differs is where the work runs.  The reference's batch loop computes the box loss with a Python loop over the nodes, reads
three scalars back per batch, re-encodes the box angle with a numpy loop on the CPU and steps ``torch.optim.Adam``.  Here a batch is

    collate (already in HBM) -> [adapt_orientation_angle] -> model -> detection loss -> backward -> FusedAdam

without a single host read: the running sums of the three losses and the number of batches whose box loss was NaN (and therefore
ignored, trainer.py:208-217) accumulate in one device tensor that is read ONCE per epoch.  The reference prints a line per
NaN batch; here the count is printed after that read."""
from __future__ import annotations

import copy
import glob
import json
import os
import random
import re
import time
from dataclasses import asdict
from typing import List

import numpy as np
import torch
from torch.optim.lr_scheduler import ExponentialLR, LambdaLR, ReduceLROnPlateau

from .. import ops
from ..data import DataLoader
from ..inference import plan_steps
from ..optim import FusedAdam
from . import autograd as AG
from .configs import GNNArchitectureConfig, TrainingConfig
from .losses import detection_loss_groups

# detections per class in RadarScenes (label order of the dataset: car, pedestrian, pedestrian group, two wheeler, large vehicle,
# background), as published with the dataset and used by the reference's ClassDistribution
RADAR_SCENES_POINTS_PER_CLASS = {"car": 2.1e6, "pedestrian": 5.1e5, "pedestrian group": 1.1e6, "two wheeler": 2.7e5,
                                 "large vehicle": 9e5, "background": 1.3e8}


def radar_scenes_class_weights() -> dict:
    """Inverse class frequency, normalised so that the rarest class (two wheeler) weighs 1 -- what
    ``set_weights_according_radar_scenes_distribution`` selects (utils/radar_scenes_properties.py:85-106)."""
    total = sum(RADAR_SCENES_POINTS_PER_CLASS.values())
    rarest = total / RADAR_SCENES_POINTS_PER_CLASS["two wheeler"]
    return {name: (total / count) / rarest for name, count in RADAR_SCENES_POINTS_PER_CLASS.items()}


class _BatchLoss(torch.autograd.Function):
    """``detection_loss``'s kernels for the trainer: also hands out the loss kernel's four sums (to count NaN box losses on the
    device) and differentiates only the total, so that ``backward()`` is one launch and never asks the device whether the
    gradients of the two reported terms are zero."""

    @staticmethod
    def forward(ctx, cls, bb, y, class_weight, bg_index, alpha, beta):
        out, sums = ops.detection_loss(cls.detach(), bb.detach(), y, class_weight, bg_index, 1.0, alpha, beta)
        ctx.save_for_backward(cls.detach(), bb.detach(), y, sums)
        ctx.class_weight = class_weight
        ctx.args = (bg_index, alpha, beta)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(out, sums)
        return out[0], out, sums

    @staticmethod
    def backward(ctx, g_loss, _g_out, _g_sums):
        if g_loss is None:
            return (None,) * 7
        cls, bb, y, sums = ctx.saved_tensors
        bg_index, alpha, beta = ctx.args
        d_cls, d_bb = ops.detection_loss_bwd(cls, bb, y, ctx.class_weight, bg_index, 1.0, alpha, beta, sums, g_loss)
        return d_cls, d_bb, None, None, None, None, None


def plan_train_steps(n_batches: int, batches_per_step: int) -> List[List[int]]:
    """Loader batches (by index, in order) grouped into training steps of ``batches_per_step`` consecutive batches; the last step
    of an epoch takes what is left."""
    k = int(batches_per_step)
    if k < 1:
        raise ValueError("train_batches_per_step must be a positive integer")
    n = int(n_batches)
    return [list(range(i, min(i + k, n))) for i in range(0, n, k)]


class _Step:
    """Several consecutive loader batches collated into one disconnected graph; ``ptr``: int64 [G + 1] on the device, the node
    offsets of the G loader batches (the segments of BatchNorm and the groups of the loss)."""
    __slots__ = ("x", "edge_index", "edge_attr", "y", "ptr", "groups")

    def __init__(self, x, edge_index, edge_attr, y, ptr, groups):
        self.x, self.edge_index, self.edge_attr, self.y, self.ptr, self.groups = x, edge_index, edge_attr, y, ptr, groups


class Trainer:
    """``Trainer(config, model)`` is the reference's trainer: one forward per loader batch, and for training one backward and one
    optimizer step per loader batch.  Two keyword arguments let a step take several loader batches through ONE launch chain; every
    train-mode BatchNorm then normalises each loader batch with its own statistics (``model(..., frame_ptr=<loader-batch borders>)``)
    and the loss is computed per loader batch (``detection_loss(..., group_ptr=...)``).

    ``valid_graphs_per_step`` > 0: validation groups whole consecutive loader batches until a step holds at least that many graphs
    (``inference.plan_steps``).  It computes THE REFERENCE'S NUMBERS: every loader batch is normalised and scored on its own, the
    running statistics are walked batch after batch, the epoch value is still the sum of the per-batch losses over ``len(loader)``.

    ``train_batches_per_step`` = k > 1: a training step takes k consecutive loader batches (the last step of an epoch what is
    left), backpropagates the MEAN of their k losses and makes one optimizer step.  This is GRADIENT ACCUMULATION: k times fewer
    optimizer steps per epoch and a trajectory that differs from the reference's (equal only in the per-batch forward and loss).
    The reported per-epoch figures stay means per loader batch."""

    def __init__(self, config: TrainingConfig, model: torch.nn.Module, *, valid_graphs_per_step: int = 0,
                 train_batches_per_step: int = 1):
        for name, value, low in (("valid_graphs_per_step", valid_graphs_per_step, 0), ("train_batches_per_step", train_batches_per_step, 1)):
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < low:
                raise ValueError(f"{name} must be an integer >= {low}, got {value!r}")
        self.valid_graphs_per_step = int(valid_graphs_per_step)
        self.train_batches_per_step = int(train_batches_per_step)
        self._mean_coef = {}                       # G -> device float [G] of 1 / G (the loss backward's per-group coefficients)
        self.config = config
        self.model = model
        self.train_loss_cls = []
        self.train_loss_bb = []
        self.train_loss = []
        self.valid_loss = []
        self.model_lowest_valid = {}
        self.early_stopping_triggers = 0
        self.nan_batches = []                      # per epoch: training batches whose box loss was NaN and ignored

    # ---- configuration -> objects ------------------------------------------------------------------------------------------------
    def make_scheduler(self, optimizer: torch.optim.Optimizer):
        """trainer.py:74-87: plateau patience first, then the exponential factor, else a constant rate."""
        cfg = self.config
        if cfg.reduce_lr_on_plateau_patience > 0:
            return ReduceLROnPlateau(optimizer, factor=cfg.reduce_lr_on_plateau_factor, patience=cfg.reduce_lr_on_plateau_patience)
        if cfg.exponential_lr_decay_factor > 0:
            return ExponentialLR(optimizer, gamma=cfg.exponential_lr_decay_factor)
        return LambdaLR(optimizer, lambda _: 1.0)

    def class_weight_tensors(self, device):
        """(training, validation) cross-entropy weights, float32 [K] on ``device``, in the order of the configuration's dicts."""
        cfg = self.config
        if cfg.set_weights_according_radar_scenes_distribution:
            train = valid = list(radar_scenes_class_weights().values())
        else:
            train, valid = list(cfg.class_weights.values()), list(cfg.val_class_weights.values())
        as_dev = lambda w: torch.tensor(w, dtype=torch.float32).to(device)
        return as_dev(train), as_dev(valid)

    # ---- epoch-end bookkeeping: plain floats in, no model and no device needed --------------------------------------------------------
    def end_epoch(self, epoch: int, loss_train: float, loss_cls: float, loss_bb: float, loss_valid: float,
                  scheduler=None) -> bool:
        """Record one epoch (trainer.py:116-146): append the losses, step the scheduler (the plateau scheduler gets the validation
        loss), keep a deep copy of the model if this validation loss is the lowest so far (``<=``: a tie goes to the later epoch),
        count consecutive epochs above the best.  -> True when training should stop."""
        self.train_loss.append(loss_train)
        self.train_loss_cls.append(loss_cls)
        self.train_loss_bb.append(loss_bb)
        self.valid_loss.append(loss_valid)
        if scheduler is not None:
            if isinstance(scheduler, ReduceLROnPlateau):
                scheduler.step(loss_valid)
            else:
                scheduler.step()
        best = min(self.valid_loss)
        if loss_valid <= best:
            self.model_lowest_valid = {"model": copy.deepcopy(self.model), "epoch": epoch}
        print(f">>> Epoch: {epoch}/{self.config.epochs}, loss_train: {round(loss_train, 5)}, loss_valid: {round(loss_valid, 5)}")
        if loss_valid > best:
            self.early_stopping_triggers += 1
            print("Trigger Times:", self.early_stopping_triggers)
            if self.early_stopping_triggers >= self.config.early_stopping_patience:
                print("Early stopping!")
                return True
        else:
            self.early_stopping_triggers = 0
        return False

    # ---- the loops ---------------------------------------------------------------------------------------------------------------
    def fit(self, data_loaders: dict) -> None:
        """Train on ``data_loaders["train"]``, validate on ``data_loaders["validate"]`` (``radargnn_amd.data.DataLoader``: the batches
        are collated in HBM; a batch of any other loader is moved with ``.to(device)``)."""
        if not torch.cuda.is_available():
            raise RuntimeError("Trainer.fit runs on the GPU (radargnn_amd has no CPU path)")
        start = time.time()
        device = torch.device("cuda", torch.cuda.current_device())
        self.model.to(device)
        cfg = self.config
        optimizer = FusedAdam(self.model.parameters(), lr=cfg.learning_rate, weight_decay=cfg.regularization_strength)
        scheduler = self.make_scheduler(optimizer)
        weights, val_weights = self.class_weight_tensors(device)
        self.early_stopping_triggers = 0
        for epoch in range(1, cfg.epochs + 1):
            loss_train, loss_cls, loss_bb, nan_batches = self._train_epoch(data_loaders.get("train"), device, optimizer, weights)
            loss_valid = self._validate_epoch(data_loaders.get("validate"), device, val_weights)
            self.nan_batches.append(nan_batches)
            if nan_batches:
                print(f">>> nan in loss_bb found and ignored in {nan_batches} batch(es) of epoch {epoch} <<<")
            if self.end_epoch(epoch, loss_train, loss_cls, loss_bb, loss_valid, scheduler):
                break
        print(f">>> Overall training duration: {round((time.time() - start) / 3600, 2)} hours")

    def _batch_loss(self, batch, device, class_weight):
        """forward + loss of one batch -> (loss, out = [loss, loss_cls, loss_bb], sums); nothing here waits for the device"""
        if getattr(batch.x, "device", device) != device:
            batch = batch.to(device)
        y = batch.y
        if self.config.adapt_orientation_angle:
            y = ops.adapt_orientation_angle(y)             # a new tensor: neither the batch nor the store it came from changes
        cls, bb = self.model(batch.x, batch.edge_index, batch.edge_attr)
        if y.dtype != torch.float32:
            y = y.float()
        return _BatchLoss.apply(cls, bb, y, class_weight, int(self.config.bg_index), float(self.config.cls_loss_weight),
                                float(self.config.bb_loss_weight))

    # ---- grouped steps: several loader batches per launch chain ------------------------------------------------------------------
    def _steps(self, loader, device, plan, full):
        """The loader's batches grouped into steps -> _Step per step (a step of one loader batch comes as the batch itself).
        A resident ``radargnn_amd.data.DataLoader`` is planned up front (``plan(batch sizes) -> lists of batch indices``) and every
        step collated ONCE from the store; any other iterable is walked, ``full(batches held, graphs held)`` closing a step, and
        its batches concatenated on the device with offset ``edge_index``."""
        if isinstance(loader, DataLoader):
            store = loader.store
            batch_ids = [np.asarray(ids, dtype=np.int64) for ids in loader.batch_ids()]     # ONE draw of a shuffling loader
            steps = plan([ids.size for ids in batch_ids])
            sizes = store.node_ptr[1:] - store.node_ptr[:-1]
            bounds = np.concatenate(([0], np.cumsum([int(sizes[ids].sum()) for ids in batch_ids], dtype=np.int64))).astype(np.int64)
            tabs = [bounds[s[0]:s[-1] + 2] - bounds[s[0]] for s in steps]                   # every step's borders in one upload
            tab_at = np.concatenate(([0], np.cumsum([t.size for t in tabs]))).astype(np.int64)
            tab_dev = torch.from_numpy(np.concatenate(tabs)).to(store.device) if tabs else None
            for k, step in enumerate(steps):
                batch = store.collate(np.concatenate([batch_ids[i] for i in step]))
                if len(step) == 1:
                    yield batch
                else:
                    yield _Step(batch.x, batch.edge_index, batch.edge_attr, batch.y, tab_dev[tab_at[k]:tab_at[k + 1]], len(step))
            return
        held, graphs = [], 0
        for batch in loader:
            if getattr(batch.x, "device", device) != device:
                batch = batch.to(device)
            held.append(batch)
            graphs += int(getattr(batch, "num_graphs", 1))
            if full(len(held), graphs):
                yield self._concatenate(held, device)
                held, graphs = [], 0
        if held:
            yield self._concatenate(held, device)

    @staticmethod
    def _concatenate(batches, device):
        if len(batches) == 1:
            return batches[0]
        offsets = np.concatenate(([0], np.cumsum([b.x.shape[0] for b in batches], dtype=np.int64))).astype(np.int64)
        return _Step(torch.cat([b.x for b in batches]),
                     torch.cat([b.edge_index + int(o) for b, o in zip(batches, offsets)], dim=1),
                     torch.cat([b.edge_attr for b in batches]), torch.cat([b.y for b in batches]),
                     torch.from_numpy(offsets).to(device), len(batches))

    def _step_loss(self, step: _Step, class_weight, record: bool):
        """forward + loss of a grouped step -> (loss [G], out [G, 3] = loss, loss_cls, loss_bb per loader batch, sums [G, 4])"""
        y = step.y
        if self.config.adapt_orientation_angle:
            y = ops.adapt_orientation_angle(y)
        if record:                                         # the differentiable segment-scoped forward, recorded once
            with AG.recording(direct=True):
                cls, bb = self.model(step.x, step.edge_index, step.edge_attr, frame_ptr=step.ptr)
        else:
            cls, bb = self.model(step.x, step.edge_index, step.edge_attr, frame_ptr=step.ptr)
        if y.dtype != torch.float32:
            y = y.float()
        loss, _, _, sums, out = detection_loss_groups(cls, bb, y, class_weight, step.ptr, int(self.config.bg_index), 1.0,
                                                      float(self.config.cls_loss_weight), float(self.config.bb_loss_weight))
        return loss, out, sums

    def _train_epoch_grouped(self, loader, device, optimizer, class_weight):
        """Gradient accumulation over ``train_batches_per_step`` loader batches: one forward, one loss launch, one backward launch of
        the loss with the coefficients 1 / G, one optimizer step."""
        acc = torch.zeros(4, dtype=torch.float64, device=device)       # sums of loss, loss_cls, loss_bb | NaN batches
        k = self.train_batches_per_step
        for step in self._steps(loader, device, lambda sizes: plan_train_steps(len(sizes), k), lambda held, _graphs: held >= k):
            optimizer.zero_grad()
            if not isinstance(step, _Step):                # one loader batch left: the step of the ungrouped loop
                loss, out, sums = self._batch_loss(step, device, class_weight)
                loss.backward()
                optimizer.step()
                acc[:3].add_(out)
                acc[3:].add_(torch.isnan(sums[2:3]))
                continue
            loss, out, sums = self._step_loss(step, class_weight, record=True)
            coef = self._mean_coef.get((device, step.groups))
            if coef is None:
                coef = self._mean_coef[(device, step.groups)] = torch.full((step.groups,), 1.0 / step.groups, dtype=torch.float32, device=device)
            torch.autograd.backward([loss], [coef])        # d (1/G) sum_g loss_g: the loss kernel takes the coefficients per group
            optimizer.step()
            acc[:3].add_(out.sum(0))
            acc[3:].add_(torch.isnan(sums[:, 2]).sum())
        total, cls_sum, bb_sum, nan_batches = acc.tolist()                 # the epoch's one host read
        n = len(loader)
        return total / n, cls_sum / n, bb_sum / n, int(nan_batches)

    def _train_epoch(self, loader, device, optimizer, class_weight):
        if self.train_batches_per_step > 1:
            return self._train_epoch_grouped(loader, device, optimizer, class_weight)
        acc = torch.zeros(4, dtype=torch.float64, device=device)       # sums of loss, loss_cls, loss_bb | NaN batches
        for batch in loader:
            optimizer.zero_grad()
            loss, out, sums = self._batch_loss(batch, device, class_weight)
            loss.backward()
            optimizer.step()
            acc[:3].add_(out)
            acc[3:].add_(torch.isnan(sums[2:3]))           # the kernel's Huber sum: NaN is what made it report loss_bb = 0
        total, cls_sum, bb_sum, nan_batches = acc.tolist()                 # the epoch's one host read
        n = len(loader)
        return total / n, cls_sum / n, bb_sum / n, int(nan_batches)

    @torch.no_grad()
    def _validate_epoch(self, loader, device, class_weight) -> float:
        acc = torch.zeros(3, dtype=torch.float64, device=device)
        if self.valid_graphs_per_step > 0:
            # whole consecutive loader batches per launch chain; each is still normalised and scored on its own (frame_ptr, group_ptr)
            per_step = self.valid_graphs_per_step
            for step in self._steps(loader, device, lambda sizes: plan_steps(sizes, per_step), lambda _held, graphs: graphs >= per_step):
                if isinstance(step, _Step):
                    acc.add_(self._step_loss(step, class_weight, record=False)[1].sum(0))
                else:
                    acc.add_(self._batch_loss(step, device, class_weight)[1])
            return acc[0].item() / len(loader)
        for batch in loader:                              # the model stays in train mode, as in the reference
            _, out, _ = self._batch_loss(batch, device, class_weight)
            acc.add_(out)
        return acc[0].item() / len(loader)

    # ---- results -----------------------------------------------------------------------------------------------------------------
    def save_results(self, path: str, model_config: GNNArchitectureConfig, dataset_config_dict: dict) -> None:
        """A new ``model_NN`` folder under ``path`` with the reference's files (trainer.py:311-376): both configurations as JSON,
        the final model and the lowest-validation model each as whole-module pickle and as state dict, the four loss curves as
        ``.npy`` and their plot."""
        folder = get_new_result_folder_path(path)
        os.mkdir(folder)
        with open(f"{folder}/gnn_configs.json", "w") as f:
            json.dump({"GNN_ARCHITECTURE_CONFIG": asdict(model_config), "TRAINING_CONFIG": asdict(self.config)}, f, indent=4)
        with open(f"{folder}/dataset_configs.json", "w") as f:
            json.dump(dataset_config_dict, f, indent=4)
        torch.save(self.model, f"{folder}/trained_model.pt")
        torch.save(self.model.state_dict(), f"{folder}/trained_model_state_dict.pt")
        best, epoch = self.model_lowest_valid.get("model"), self.model_lowest_valid.get("epoch")
        torch.save(best, f"{folder}/trained_model_low_val_ep{epoch}.pt")
        torch.save(best.state_dict(), f"{folder}/trained_model_low_val_ep{epoch}_state_dict.pt")
        for name, curve in (("loss_train", self.train_loss), ("loss_validation", self.valid_loss),
                            ("loss_train_cls", self.train_loss_cls), ("loss_train_bb", self.train_loss_bb)):
            np.save(f"{folder}/{name}.npy", np.array([curve]))
        fig, _ = self.show_learning_curves()
        fig.savefig(f"{folder}/loss_curves.png")

    def show_learning_curves(self):
        import matplotlib.pyplot as plt
        fig, ax = plt.subplots()
        for curve in (self.train_loss, self.valid_loss, self.train_loss_cls, self.train_loss_bb):
            ax.plot(range(len(curve)), curve)
        ax.legend(["Training loss", "Validation loss", "Training loss classification", "Training loss bounding box"])
        ax.set_title("Training and validation loss")
        ax.grid("minor")
        ax.set_xlabel("epoch")
        ax.set_ylabel("loss")
        return fig, ax


def get_new_result_folder_path(path: str) -> str:
    """``{path}/model_NN`` with NN one above the highest number any sub-folder's name ends in (``model_01`` in an empty parent;
    two digits below 10)."""
    numbers = []
    for folder in glob.glob(path + "/*/"):
        digits = re.search(r"(\d+)$", os.path.basename(os.path.normpath(folder)))
        if digits:
            numbers.append(int(digits.group(1)))
    return f"{path}/model_{max(numbers, default=0) + 1:02d}"


def set_seeds(seed: int) -> None:
    """Seed Python's, numpy's and torch's generators (what ``torch_geometric.seed_everything`` does; torch_geometric is not needed)."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    torch.backends.cudnn.benchmark = False
    torch.backends.cudnn.deterministic = True
