"""``Predictor`` -- the inference driver of the reference (postprocessor/inference.py:5-75: ``Predictor(model, dataloader,
verbose).predict() -> predictions, ground_truth, pos, vel``) on the device.

The reference runs one forward per loader batch (evaluate.py:40 builds the loader with ``batch_size=1``), never puts the model in
eval mode, and copies six arrays per batch to the host.  Here, for a ``radargnn_amd.data.DataLoader``:

* consecutive loader batches are grouped into STEPS of at least ``graphs_per_step`` graphs (``plan_steps``).  A step is one
  ``GraphStore.collate`` and one ``model(x, edge_index, edge_attr, frame_ptr=...)`` with ``frame_ptr`` at the loader-batch
  boundaries: every train-mode BatchNorm takes its statistics per loader batch and walks its running statistics through them in
  order (gnn.linear.frame_scope) -- what one forward per loader batch computes, in one launch chain;
* the step's epilogue is one launch (``ops.predict_rows``): softmax, boxes and the two halves of ``y`` go straight to the step's
  rows of six whole-split buffers.  The returned list entries are contiguous views of those buffers, one per loader batch in
  the loader's order; ``to_host=True`` copies each buffer to the host once, after the last step, and returns numpy views.

Any other iterable of batches (a list of ``Batch``, a foreign loader) gets one forward per batch after ``.to(device)``, as the
reference does.  The forward runs under ``torch.no_grad()`` (the reference leaves autograd on and never calls backward: same
values).  The model's ``training`` flag is left as found."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .data import DataLoader


def plan_steps(batch_sizes: Sequence[int], graphs_per_step: int) -> List[List[int]]:
    """Loader batches (by index, in order) grouped into steps: a step takes whole batches until it holds at least
    ``graphs_per_step`` graphs -- a batch is never split, a batch of more graphs than that is a step of its own, the last
    step takes what is left."""
    if int(graphs_per_step) < 1:
        raise ValueError("graphs_per_step must be a positive integer")
    steps: List[List[int]] = []
    cur: List[int] = []
    held = 0
    for i, size in enumerate(batch_sizes):
        cur.append(i)
        held += int(size)
        if held >= graphs_per_step:
            steps.append(cur)
            cur, held = [], 0
    if cur:
        steps.append(cur)
    return steps


class Predictor:
    """Makes predictions for a whole split and keeps the raw results (postprocessor/inference.py:5-75).

    model: a ``DetNetBasic``; dataloader: a ``radargnn_amd.data.DataLoader`` (grouped into steps) or any iterable of batches;
    graphs_per_step: graphs per launch chain; to_host: numpy entries, as the reference returns them."""

    def __init__(self, model, dataloader, verbose: bool = True, graphs_per_step: int = 64, to_host: bool = False):
        if int(graphs_per_step) < 1:
            raise ValueError("graphs_per_step must be a positive integer")
        self.model = model
        self.dataloader = dataloader
        self.verbose = verbose
        self.graphs_per_step = int(graphs_per_step)
        self.to_host = to_host

    def predict(self) -> Tuple[Dict[str, list], Dict[str, list], list, list]:
        """-> (predictions {"bounding_box_predictions", "class_probability_prediction"}, ground_truth {"bounding_box_true",
        "class_true"}, pos, vel): lists with one entry per loader batch, in the loader's order."""
        device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')
        if self.verbose:
            print(f"Device for inference: {device}")
        self.model.to(device)
        with torch.no_grad():
            if isinstance(self.dataloader, DataLoader):
                prob, bb, class_true, bb_true, pos, vel = self._predict_resident(device)
            else:
                prob, bb, class_true, bb_true, pos, vel = self._predict_batches(device)
        predictions = {"bounding_box_predictions": bb, "class_probability_prediction": prob}
        ground_truth = {"bounding_box_true": bb_true, "class_true": class_true}
        return predictions, ground_truth, pos, vel

    def _progress(self, i: int, total: int) -> None:
        if self.verbose and ((i + 1) == 1 or (i + 1) % 10 == 0 or (i + 1) == total):
            print(f"{i+1}/{total} inferences finished")

    # ---- a resident loader: steps of several loader batches -----------------------------------------------------------------
    def _predict_resident(self, device):
        loader = self.dataloader
        store = loader.store
        for key in ("x", "edge_index", "edge_attr", "y", "pos", "vel"):
            if key not in store.resident:
                raise AttributeError(f"the graphs of the loader carry no `{key}`: Predictor needs x, edge_index, edge_attr, y, pos, vel")
        y_all = store.resident["y"]
        if y_all.dim() != 2 or y_all.shape[1] < 1 or y_all.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"`y` must be float32 or float64 [N, 1 + box columns], got {y_all.dtype} {tuple(y_all.shape)}")
        batch_ids = [np.asarray(ids, dtype=np.int64) for ids in loader.batch_ids()]     # ONE draw: a shuffling loader's permutation
        total = len(batch_ids)
        steps = plan_steps([ids.size for ids in batch_ids], self.graphs_per_step)
        # node offsets of the loader batches in the outputs (the loader's order), from the store's own table
        sizes = store.node_ptr[1:] - store.node_ptr[:-1]
        rows = [int(sizes[ids].sum()) for ids in batch_ids]
        bounds = np.concatenate(([0], np.cumsum(rows, dtype=np.int64))).astype(np.int64)
        n = int(bounds[-1])
        # per step: the offsets of its loader batches relative to its first row -- every step's table in one upload
        tabs = [bounds[s[0]:s[-1] + 2] - bounds[s[0]] for s in steps]
        tab_at = np.concatenate(([0], np.cumsum([t.size for t in tabs]))).astype(np.int64)
        tab_dev = (torch.from_numpy(np.concatenate(tabs)).to(store.device) if tabs
                   else torch.zeros(0, dtype=torch.int64, device=store.device))

        prob = bb = None                                   # (their widths are the model's: known after the first forward)
        wy = y_all.shape[1] - 1
        class_true = torch.empty((n,), dtype=y_all.dtype, device=store.device)
        bb_true = torch.empty((n, wy), dtype=y_all.dtype, device=store.device)
        for k, step in enumerate(steps):
            batch = store.collate(np.concatenate([batch_ids[i] for i in step]))
            if len(step) > 1:
                cls_s, bb_s = self.model(batch.x, batch.edge_index, batch.edge_attr, frame_ptr=tab_dev[tab_at[k]:tab_at[k + 1]])
            else:                                          # one loader batch: its forward, as it is
                cls_s, bb_s = self.model(batch.x, batch.edge_index, batch.edge_attr)
            if prob is None:
                prob = torch.empty((n, cls_s.shape[1]), dtype=torch.float32, device=store.device)
                bb = torch.empty((n, bb_s.shape[1]), dtype=torch.float32, device=store.device)
            ops.predict_rows(cls_s, bb_s, batch.y, prob, bb, class_true, bb_true, row0=int(bounds[step[0]]))
            for i in step:
                self._progress(i, total)
        if prob is None:                                   # an empty loader
            prob = torch.empty((0, 0), dtype=torch.float32, device=store.device)
            bb = torch.empty((0, 0), dtype=torch.float32, device=store.device)
        # positions and velocities never pass through the model: one segmented copy of the whole split each, in the loader's order
        order = np.concatenate(batch_ids) if batch_ids else np.zeros(0, dtype=np.int64)
        pos, vel = (self._gather_split(store, key, order, n) for key in ("pos", "vel"))
        return tuple(self._entries(buf, rows) for buf in (prob, bb, class_true, bb_true, pos, vel))

    @staticmethod
    def _gather_split(store, key: str, order: np.ndarray, n: int) -> torch.Tensor:
        res = store.resident[key]
        if store.kind[key] != "node":
            raise ValueError(f"`{key}` must hold one row per node")
        if order.size == 0:
            return res[:0].clone()
        src = store.node_ptr[order]
        dst = np.concatenate(([0], np.cumsum(store.node_ptr[order + 1] - src)))
        tab = torch.from_numpy(np.concatenate((src, dst)).astype(np.int64)).to(store.device)
        return ops.collate_rows(res, tab[:order.size], tab[order.size:], n)

    def _entries(self, buf: torch.Tensor, rows: List[int]) -> list:
        """One contiguous view of the whole-split buffer per loader batch (numpy views of ONE host copy with ``to_host``)."""
        if not rows:
            return []
        if self.to_host:
            host = buf.cpu().numpy()
            at = np.concatenate(([0], np.cumsum(rows)))
            return [host[at[i]:at[i + 1]] for i in range(len(rows))]
        return list(torch.split(buf, rows, dim=0))

    # ---- any other iterable of batches: one forward per batch, as the reference does -----------------------------------
    def _predict_batches(self, device):
        prob, bb, class_true, bb_true, pos, vel = [], [], [], [], [], []
        total = len(self.dataloader) if hasattr(self.dataloader, "__len__") else None
        for i, graph_batch in enumerate(self.dataloader):
            graph_batch.to(device)
            cls_b, bb_b = self.model(graph_batch.x, graph_batch.edge_index, graph_batch.edge_attr)
            y = graph_batch.y
            n = cls_b.shape[0]
            out = (torch.empty((n, cls_b.shape[1]), dtype=torch.float32, device=cls_b.device),
                   torch.empty((n, bb_b.shape[1]), dtype=torch.float32, device=cls_b.device),
                   torch.empty((n,), dtype=y.dtype, device=cls_b.device),
                   torch.empty((n, y.shape[1] - 1), dtype=y.dtype, device=cls_b.device))
            ops.predict_rows(cls_b, bb_b, y, *out)
            for lst, t in zip((prob, bb, class_true, bb_true, pos, vel), (*out, graph_batch.pos.detach(), graph_batch.vel.detach())):
                lst.append(t.cpu().numpy() if self.to_host else t)
            self._progress(i, -1 if total is None else total)
        return prob, bb, class_true, bb_true, pos, vel
