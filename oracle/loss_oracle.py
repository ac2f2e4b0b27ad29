"""CPU oracle for the trainer's loss.  TEST INFRASTRUCTURE ONLY.

Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may import this module; the
product (``radargnn_amd``) never does.

Restates src/gnnradarobjectdetection/gnn/trainer.py:181-222 with the same torch modules the reference constructs
(``torch.nn.CrossEntropyLoss(weight=...)``, ``torch.nn.HuberLoss()``, trainer.py:99,106) and the same per-node Python loop,
in float64 on the CPU; differentiable, so gradients come from torch autograd.  torch is present in this image, so this IS
the reference's arithmetic (parity pinned by executing the same library calls)."""
from __future__ import annotations

import numpy as np
import torch


def detection_loss(cls: torch.Tensor, bb: torch.Tensor, y: torch.Tensor, bg_index: int, class_weights=None,
                   cls_loss_weight: float = 1.0, bb_loss_weight: float = 1.0, delta: float = 1.0):
    weights = None if class_weights is None else torch.as_tensor(class_weights, dtype=cls.dtype)
    cross_entropy = torch.nn.CrossEntropyLoss(weight=weights)
    huber = torch.nn.HuberLoss(delta=delta)
    label_true = y[:, 0].long()
    bb_true = y[:, 1:]
    loss_cls = cross_entropy(cls, label_true)
    loss_bb = 0
    num_bb = 0
    for i, label in enumerate(label_true):
        if label != bg_index:
            num_bb += 1
            loss_bb = loss_bb + huber(bb_true[i, :], bb[i, :])
    loss_bb = loss_bb / num_bb if num_bb != 0 else 0
    try:
        if np.isnan(loss_bb.item()):
            loss_bb = 0
    except Exception:
        pass
    return cls_loss_weight * loss_cls + bb_loss_weight * loss_bb, loss_cls, loss_bb


def detection_loss_vectorised(cls: torch.Tensor, bb: torch.Tensor, y: torch.Tensor, bg_index: int, class_weights=None,
                              cls_loss_weight: float = 1.0, bb_loss_weight: float = 1.0, delta: float = 1.0):
    """``detection_loss`` without the per-node loop, in the dtype and on the device of ``cls`` (differentiable): usable at the
    10^5 rows of a training batch.  Same function term by term:

    * weighted cross-entropy, mean reduction: sum_i w[y_i] (-log softmax(cls_i)[y_i]) / sum_i w[y_i];
    * a label of -100 (``CrossEntropyLoss``'s ``ignore_index``): weight 0 in the numerator and the denominator of the cross
      entropy (no gradient to that row's logits); the row is still an object row of the box term, as in the per-node loop;
    * HuberLoss(delta) (mean over the W box components) per row whose label is not ``bg_index``, averaged over those rows;
    * no such row, or a NaN box term: the box term is 0 (and contributes no gradient)."""
    label = y[:, 0].long()
    w = torch.ones(cls.shape[1], dtype=cls.dtype, device=cls.device) if class_weights is None else \
        torch.as_tensor(class_weights, dtype=cls.dtype).to(cls.device)
    ignored = label == -100
    safe = label.masked_fill(ignored, 0)
    wi = w[safe].masked_fill(ignored, 0.0)
    nll = -torch.log_softmax(cls, dim=1).gather(1, safe.view(-1, 1)).view(-1)
    # (sum over the kept rows only: 0 * inf of an ignored row must not reach the numerator)
    loss_cls = (wi * nll)[~ignored].sum() / wi.sum()
    obj = label != bg_index
    loss_bb = torch.zeros((), dtype=cls.dtype, device=cls.device)
    if bool(obj.any()):
        r = bb[obj] - y[obj, 1:].to(bb.dtype)
        a = r.abs()
        h = torch.where(a < delta, 0.5 * r * r, delta * (a - 0.5 * delta))
        lb = h.mean(dim=1).sum() / int(obj.sum())
        if not bool(torch.isnan(lb)):
            loss_bb = lb
    return cls_loss_weight * loss_cls + bb_loss_weight * loss_bb, loss_cls, loss_bb
