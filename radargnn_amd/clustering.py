"""Clustering in HBM: batched DBSCAN over the rows of the radius search, and the clusters of a segmented point cloud as boxes.

    clusters = dbscan_frames(X, frame_ptr, eps, min_samples)                  # any number of frames, one search + one launch
    clusters = dbscan_graph(graph_batch, frame_ptr, min_samples)              # from the radius graph the model already built
    labels = DBSCAN(eps=0.5, min_samples=5).fit_predict(points)               # numpy in, numpy out: scikit-learn's class
    inst = cluster_objects(pos, frame_ptr, class_of_point, bg_index, eps, min_samples, prob=class_prob)
    detections = inst.detections()                                            # postprocessor.Detections: radargnn_amd.metrics scores it

The labels equal ``sklearn.cluster.DBSCAN(eps, min_samples, algorithm="kd_tree")`` entry for entry (the rule: include/rgnn.h,
"clustering"): the neighbourhoods are the rows of ``ops.radius_graph`` at r = eps, which is pinned to the KD-tree's arithmetic
(``d2 <= eps * eps``, d2 accumulated per column in order), and clusters are numbered by their smallest row, which is the order in which
scikit-learn's sequential sweep opens them.  One work-group per frame holds the frame's union-find array in LDS
(csrc/cluster.hip): a frame of more than ``ops.dbscan_max_frame_points()`` points is refused.  There is no CPU path.
"""
from __future__ import annotations

import math
import numbers
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import ops

MAX_BASIS_COLUMNS = 8         # the neighbour search is compiled for 2, 4 and 8 columns; narrower bases are padded with zero columns


# ------------------------------------------------------------------------------------------------ argument checks (host only)
def check_parameters(eps, min_samples) -> tuple:
    """(eps as float, min_samples as int); ValueError for eps <= 0 (or not finite), a non-integer min_samples or min_samples < 1."""
    if isinstance(eps, bool) or not isinstance(eps, numbers.Real) or not math.isfinite(float(eps)) or not float(eps) > 0.0:
        raise ValueError(f"eps must be a positive finite number (got {eps!r})")
    if isinstance(min_samples, bool) or not isinstance(min_samples, numbers.Integral):
        raise ValueError(f"min_samples must be an integer (got {type(min_samples).__name__} {min_samples!r})")
    if not 1 <= int(min_samples) < 2 ** 31:
        raise ValueError(f"min_samples must be in [1, 2^31) (got {int(min_samples)})")
    return float(eps), int(min_samples)


def check_basis_shape(shape) -> int:
    """The width the distance basis is padded to (2, 4 or 8); ValueError unless it is [N, 1..8]."""
    if len(shape) != 2:
        raise ValueError(f"the distance basis must be 2-D [N, columns] (got {len(shape)}-D)")
    w = int(shape[1])
    if not 1 <= w <= MAX_BASIS_COLUMNS:
        raise ValueError(f"the neighbour search supports distance bases of 1 to {MAX_BASIS_COLUMNS} columns (got {w})")
    return 2 if w <= 2 else (4 if w <= 4 else 8)


def _cuda(x, name: str, dtype) -> torch.Tensor:
    t = torch.as_tensor(x)
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError(f"{name}: clustering runs on the GPU (no CPU fallback)")
        t = t.cuda()
    return t.contiguous()


def _basis(X) -> torch.Tensor:
    """float64 [N, 2|4|8] on the device: ``X`` padded with zero columns (exact: a zero column adds +0.0 to d2), the rule of
    ``graph_constructor.graph._distance_basis``."""
    shape = tuple(X.shape) if hasattr(X, "shape") else np.asarray(X).shape
    to = check_basis_shape(shape)
    t = _cuda(X, "X", torch.float64)
    if t.shape[1] != to:
        t = torch.cat((t, torch.zeros((t.shape[0], to - t.shape[1]), dtype=torch.float64, device=t.device)), dim=1)
    return t


# ------------------------------------------------------------------------------------------------ labels
@dataclass
class Clusters:
    """DBSCAN labels of a batch of frames, in HBM: ``labels`` int32 [N] (-1 noise; numbered from 0 in every frame by ascending
    smallest core row), ``core`` uint8 [N], ``num_clusters`` int32 [B], ``status`` int32 [1] (read by ``check``)."""
    labels: torch.Tensor
    core: torch.Tensor
    num_clusters: torch.Tensor
    status: torch.Tensor

    def check(self) -> "Clusters":
        """Synchronises (one host read); ValueError if a frame was refused or a row of the graph pointed outside its frame."""
        st = int(self.status.item())
        if st & ops.STATUS_DBSCAN_FRAME_TOO_LARGE:
            raise ValueError(f"dbscan: a frame has more than {ops.dbscan_max_frame_points()} points (the cap of the LDS-resident "
                             "union-find; its rows are labelled -1): split the frame")
        if st & ops.STATUS_DBSCAN_BAD_ROW:
            raise ValueError("dbscan: the graph holds a neighbour outside its row's frame, a row outside the edge list or a frame "
                             "outside the points (RGNN_STATUS_DBSCAN_BAD_ROW); such entries were skipped")
        return self


def _group(group, n: int) -> Optional[torch.Tensor]:
    if group is None:
        return None
    g = _cuda(group, "group", torch.int32)
    if g.shape != (n,):
        raise ValueError("group must be [N]")
    return g


def dbscan_frames(X, frame_ptr, eps: float, min_samples: int, group=None, check: bool = True) -> Clusters:
    """DBSCAN of every frame of a batch: ``X`` [N, 1..8] the distance basis (computed in float64; positions, or positions | velocities
    -- callers scale the columns themselves), ``frame_ptr`` int64 [B + 1] row offsets, ``group`` int [N] or None (a point with a
    negative group takes no part; edges between groups do not exist).  One neighbour search and one label launch; the host reads
    the search's edge count and, with ``check`` (default), the status word -- ``check=False`` leaves that read to
    ``Clusters.check()``."""
    eps, min_samples = check_parameters(eps, min_samples)
    Xb = _basis(X)
    fp = _cuda(frame_ptr, "frame_ptr", torch.int64)
    n = Xb.shape[0]
    if fp.dim() != 1 or fp.numel() < 1:
        raise ValueError("frame_ptr must be [B + 1]")
    g = _group(group, n)
    if n == 0:                                            # nothing to search: every frame is empty
        dev = Xb.device
        out = Clusters(torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.uint8, device=dev),
                       torch.zeros(fp.numel() - 1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
        return out
    rowptr, col, _ = ops.radius_graph(Xb, fp, eps, want_edge_index=False)
    out = Clusters(*ops.dbscan_labels(rowptr, col, fp, min_samples, g))
    return out.check() if check else out


def dbscan_graph(graph_batch, frame_ptr, min_samples: int, group=None, *, settings, check: bool = True) -> Clusters:
    """The labels of ``dbscan_frames`` at eps = r from the radius graph the model already built (``frames.GraphBatch``: its
    ``rowptr`` and ``edge_index[1]``) -- no second search.  ``settings``: the ``frames.GraphSettings`` the graph was built with
    (what the caller gave ``HotPath`` / ``build_graphs``; a ``GraphBatch`` does not say how it was made).  kNN graphs and capped
    radius graphs are refused: their rows are not neighbourhoods."""
    _, min_samples = check_parameters(1.0, min_samples)
    cfg = settings
    if not hasattr(cfg, "algorithm") or not hasattr(cfg, "capped"):
        raise ValueError("dbscan_graph needs `settings`, the frames.GraphSettings the graph was built with")
    if cfg.algorithm != "radius":
        raise ValueError(f"dbscan_graph needs a radius graph: the rows of a {cfg.algorithm!r} graph are not eps-neighbourhoods")
    if cfg.capped:
        raise ValueError("dbscan_graph needs an uncapped radius graph: with max_neighbors a row is not the whole eps-neighbourhood")
    if getattr(graph_batch, "rowptr", None) is None:
        raise ValueError("dbscan_graph needs the rows of the search (GraphBatch.rowptr)")
    fp = _cuda(frame_ptr, "frame_ptr", torch.int64)
    rowptr = graph_batch.rowptr
    g = _group(group, rowptr.numel() - 1)
    out = Clusters(*ops.dbscan_labels(rowptr, graph_batch.edge_index[1].to(torch.int32), fp, min_samples, g))
    return out.check() if check else out


class DBSCAN:
    """``sklearn.cluster.DBSCAN`` for one cloud, on the device: numpy in, numpy out, the same attribute names, and the labels of
    ``algorithm="kd_tree"`` (Euclidean metric, no sample weights).  ``X``: [n_samples, 1..8]."""

    def __init__(self, eps: float = 0.5, min_samples: int = 5):
        self.eps = eps
        self.min_samples = min_samples

    def fit(self, X, y=None) -> "DBSCAN":
        eps, min_samples = check_parameters(self.eps, self.min_samples)
        X = np.asarray(X, dtype=np.float64)
        check_basis_shape(X.shape)
        n = X.shape[0]
        out = dbscan_frames(X, torch.tensor([0, n], dtype=torch.int64), eps, min_samples)
        self.labels_ = out.labels.cpu().numpy().astype(np.int64)
        self.core_sample_indices_ = np.nonzero(out.core.cpu().numpy())[0].astype(np.int64)
        self.components_ = X[self.core_sample_indices_].copy()
        self.n_features_in_ = X.shape[1]
        return self

    def fit_predict(self, X, y=None) -> np.ndarray:
        return self.fit(X).labels_


# ------------------------------------------------------------------------------------------------ clusters as objects
@dataclass
class Instances:
    """The clusters of a batch of frames as objects, in HBM.  Cluster m of the batch is cluster ``m - cluster_ptr[f]`` of its frame f.
    ``instance`` int64 [N]: the cluster of every point (-1: none); ``cluster_ptr`` int64 [B + 1]; ``cls`` int32 [M]; ``score`` f64 [M];
    ``rect`` f64 [M, 5] = [x_c, y_c, l, w, theta in degrees] (aligned: [x_c, y_c, dx, dy, 0]), the float32 box target of the cluster's
    first member read back in float64 -- the numbers ``corners`` f64 [M, 4, 2] are decoded from; ``valid`` bool [M]: False for a
    cluster the box kernel refuses (two coincident points, a hull without area, more than ``ops.gt_object_cap()`` points), whose
    ``rect`` and ``corners`` are NaN; ``first`` int64 [M]: the first member row; ``obj_ptr`` / ``obj_rows``: the members
    (``ops.group_objects``); ``mean_prob`` f64 [M, K] or None."""
    instance: torch.Tensor
    cluster_ptr: torch.Tensor
    cls: torch.Tensor
    score: torch.Tensor
    rect: torch.Tensor
    corners: torch.Tensor
    valid: torch.Tensor
    first: torch.Tensor
    obj_ptr: torch.Tensor
    obj_rows: torch.Tensor
    mean_prob: Optional[torch.Tensor]
    aligned: bool
    box_status: torch.Tensor

    def __len__(self) -> int:
        return self.cls.numel()

    def detections(self):
        """The valid clusters as ``postprocessor.Detections`` (``node`` is the first member row; frame offsets on the host: one
        read), so that ``radargnn_amd.metrics`` scores a clustering detector next to the box head."""
        from .postprocessor import Detections
        keep = torch.nonzero(self.valid, as_tuple=False).view(-1)
        counts = torch.zeros(self.cluster_ptr.numel(), dtype=torch.int64, device=keep.device)
        if len(self):
            frame = torch.bucketize(keep, self.cluster_ptr[1:].contiguous(), right=True)
            counts[1:] = torch.bincount(frame, minlength=self.cluster_ptr.numel() - 1)
        ptr = torch.cumsum(counts, 0).cpu()
        out = torch.float32 if self.aligned else torch.float64            # (what Detections holds for aligned / rotated boxes)
        return Detections(self.corners.index_select(0, keep).to(out), self.score.index_select(0, keep).to(out),
                          self.cls.index_select(0, keep).to(torch.float64), self.first.index_select(0, keep), ptr, self.aligned)


def cluster_objects(pos, frame_ptr, labels, bg_index: int, eps: float, min_samples: int, prob=None, basis=None,
                    per_class: bool = True, aligned: bool = False) -> Instances:
    """Segmentation + DBSCAN as a detector: the foreground points (``labels != bg_index``; ``labels`` int [N], a class per point)
    of every frame are clustered over ``basis`` (default ``pos``) and every cluster becomes a box by the ground-truth rules
    (``ops.group_objects`` -> ``ops.create_gt_boxes``: minimum-area rectangle, or the min / max box with ``aligned``) whose corners are
    what ``ops.decode_ground_truth`` decodes from those targets.  ``per_class``: points of different classes never share a cluster
    and a cluster's class is its points'; otherwise the foreground is clustered as one group and the class is the argmax of the mean
    class probabilities (``prob`` f32 [N, K]; without it, of the members' votes).  ``score``: the mean probability of that class,
    1.0 without ``prob``."""
    check_parameters(eps, min_samples)
    pos = _cuda(pos, "pos", torch.float64)
    n = pos.shape[0]
    if pos.dim() != 2 or pos.shape[1] != 2:
        raise ValueError("pos must be [N, 2]")
    lab = _cuda(labels, "labels", None)
    if lab.shape != (n,) or lab.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError("labels must be an int tensor [N]")
    lab = lab.to(torch.int32)
    fp = _cuda(frame_ptr, "frame_ptr", torch.int64)
    fg = lab != int(bg_index)
    group = torch.where(fg, lab if per_class else torch.zeros_like(lab), torch.full_like(lab, -1))
    cl = dbscan_frames(pos if basis is None else basis, fp, eps, min_samples, group)
    obj_ptr, obj_rows = ops.group_objects(cl.labels, fp)
    m, dev = obj_ptr.numel() - 1, pos.device
    box_status = torch.zeros(1, dtype=torch.int32, device=dev)      # (our own word: a refused cluster is reported in `valid`, not raised)
    targets, _, _ = ops.create_gt_boxes(pos, obj_ptr, obj_rows, None, bool(aligned), 0, status=box_status)
    first = obj_rows.index_select(0, obj_ptr[:-1]).to(torch.int64)
    targets32, pos32 = targets.to(torch.float32), pos.to(torch.float32)
    _, corners_all = ops.decode_ground_truth(torch.where(fg, 1.0 + float(bg_index), float(bg_index)).to(torch.float32), targets32,
                                             pos32, None, int(bg_index), 0)
    t = targets32.index_select(0, first).to(torch.float64)
    valid = ~torch.isnan(t).any(dim=1)
    if aligned:
        p = pos32.index_select(0, first).to(torch.float64)
        rect = torch.cat((p + t[:, :2], t[:, 2:4], torch.zeros((m, 1), dtype=torch.float64, device=dev)), dim=1)
    else:
        rect = torch.cat((t[:, :4], t[:, 4:5] * 180 / math.pi), dim=1)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    rect = torch.where(valid.view(-1, 1), rect, nan)
    corners = torch.where(valid.view(-1, 1, 1), corners_all.index_select(0, first), nan)
    cluster_ptr = torch.cat((torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(cl.num_clusters.to(torch.int64), 0)))
    rows = torch.arange(n, dtype=torch.int64, device=dev)
    frame = torch.bucketize(rows, fp[1:].contiguous(), right=True).clamp(max=max(fp.numel() - 2, 0))
    lab64 = cl.labels.to(torch.int64)
    instance = torch.where(lab64 >= 0, cluster_ptr.index_select(0, frame) + lab64, torch.full_like(lab64, -1))
    mean_prob = None
    if prob is not None:
        prob = _cuda(prob, "prob", torch.float32)
        if prob.dim() != 2 or prob.shape[0] != n:
            raise ValueError("prob must be [N, K]")
        mean_prob, cls, score = ops.cluster_scores(prob, obj_ptr, obj_rows, int(bg_index), group, bool(per_class))
    elif per_class:
        cls = group.index_select(0, first)
        score = torch.ones(m, dtype=torch.float64, device=dev)
    else:                                                 # the members' votes: the class most of them carry, the lowest on ties
        k = max(int(lab.max().item()) + 1 if n else 1, int(bg_index) + 1, 1)
        votes = torch.nn.functional.one_hot(lab.to(torch.int64).clamp(min=0), k).to(torch.float32)
        _, cls, _ = ops.cluster_scores(votes, obj_ptr, obj_rows, int(bg_index), None, False)
        score = torch.ones(m, dtype=torch.float64, device=dev)
    return Instances(instance, cluster_ptr, cls, score, rect, corners, valid, first, obj_ptr, obj_rows, mean_prob, bool(aligned),
                     box_status)
