"""CPU-only checks of the grouped trainer front end: the planning of training steps (``plan_train_steps``), the planning of
validation steps the trainer borrows from the Predictor (``inference.plan_steps``) at the sizes the trainer uses, the argument
checks of ``Trainer(..., valid_graphs_per_step=, train_batches_per_step=)`` and the concatenation of loader batches that do not
come from a resident loader (offsets of ``edge_index``, borders of the groups)."""
import types

import numpy as np
import pytest
import torch

from radargnn_amd.gnn.configs import TrainingConfig
from radargnn_amd.gnn.trainer import Trainer, _Step, plan_train_steps
from radargnn_amd.inference import plan_steps


def config():
    return TrainingConfig("radarscenes", 1e-3, 10, 2, False, 5)


@pytest.mark.parametrize("n,k,want", [
    (7, 3, [[0, 1, 2], [3, 4, 5], [6]]),                      # k does not divide len(loader): the last step takes what is left
    (6, 3, [[0, 1, 2], [3, 4, 5]]),
    (4, 1, [[0], [1], [2], [3]]),                             # k = 1: the loop of today
    (2, 5, [[0, 1]]),                                         # fewer batches than k
    (0, 3, []),                                               # an empty loader
])
def test_plan_train_steps(n, k, want):
    got = plan_train_steps(n, k)
    assert got == want
    assert [i for s in got for i in s] == list(range(n))      # every batch once, in order


@pytest.mark.parametrize("k", [0, -1])
def test_plan_train_steps_refuses_non_positive_k(k):
    with pytest.raises(ValueError):
        plan_train_steps(5, k)


def test_validation_steps_hold_whole_batches():
    """6 loader batches of 2 graphs at 4 graphs per step: three steps of two batches; a short last batch joins the last step."""
    assert plan_steps([2] * 6, 4) == [[0, 1], [2, 3], [4, 5]]
    assert plan_steps([2, 2, 2, 2, 1], 4) == [[0, 1], [2, 3], [4]]
    assert plan_steps([5] * 3, 64) == [[0, 1, 2]]
    assert plan_steps([], 4) == []


def test_trainer_defaults_and_argument_checks():
    tr = Trainer(config(), None)
    assert tr.valid_graphs_per_step == 0 and tr.train_batches_per_step == 1
    tr = Trainer(config(), None, valid_graphs_per_step=64, train_batches_per_step=12)
    assert tr.valid_graphs_per_step == 64 and tr.train_batches_per_step == 12
    assert Trainer(config(), None, train_batches_per_step=np.int64(3)).train_batches_per_step == 3
    for kw in ({"valid_graphs_per_step": -1}, {"train_batches_per_step": 0}, {"train_batches_per_step": -2},
               {"valid_graphs_per_step": 2.5}, {"train_batches_per_step": "3"}, {"train_batches_per_step": True},
               {"valid_graphs_per_step": None}):
        with pytest.raises(ValueError):
            Trainer(config(), None, **kw)
    with pytest.raises(TypeError):                            # keyword-only: Trainer(config, model, 4) is not a grouped trainer
        Trainer(config(), None, 4)


def batch_of(n, e, seed):
    g = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(x=torch.randn(n, 3, generator=g), edge_index=torch.randint(0, n, (2, e), generator=g),
                                 edge_attr=torch.randn(e, 2, generator=g), y=torch.randn(n, 6, generator=g), num_graphs=2)


def test_other_iterables_are_concatenated_with_offset_edges():
    batches = [batch_of(4, 5, 1), batch_of(1, 0, 2), batch_of(6, 9, 3), batch_of(3, 2, 4), batch_of(2, 1, 5)]
    tr = Trainer(config(), None, train_batches_per_step=2)
    steps = list(tr._steps(batches, torch.device("cpu"), None, lambda held, _graphs: held >= 2))
    assert len(steps) == 3 and isinstance(steps[0], _Step) and isinstance(steps[1], _Step)
    assert steps[2] is batches[4]                             # one batch left: the batch itself
    s = steps[1]
    assert s.groups == 2 and s.ptr.dtype == torch.int64 and s.ptr.tolist() == [0, 6, 9]
    assert torch.equal(s.x, torch.cat([batches[2].x, batches[3].x])) and torch.equal(s.y, torch.cat([batches[2].y, batches[3].y]))
    assert torch.equal(s.edge_attr, torch.cat([batches[2].edge_attr, batches[3].edge_attr]))
    assert torch.equal(s.edge_index[:, :9], batches[2].edge_index) and torch.equal(s.edge_index[:, 9:], batches[3].edge_index + 6)
    assert steps[0].ptr.tolist() == [0, 4, 5]                 # a batch of one node, without edges
    # validation: steps close on the number of graphs held
    steps = list(tr._steps(batches, torch.device("cpu"), None, lambda _held, graphs: graphs >= 4))
    assert [getattr(s, "groups", 1) for s in steps] == [2, 2, 1]
