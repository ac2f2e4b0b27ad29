"""Ground-truth box targets in HBM: the reference's ``GroundTruthCreator`` (preprocessor/radarscenes/dataset_creation.py:232-521)
on the device -- the step that writes the box columns of ``y``, the inverse of ``postprocessor.GroundTruthExtractor``.

    boxes = GroundTruthCreator.create_2D_bounding_boxes(point_cloud, aligned, bb_invariance)      # f64 [N, 4|5], one frame
    boxes = create_2d_bounding_boxes_batched(pos, object_id, frame_ptr, aligned, bb_invariance)   # any number of frames
    y = merge_targets(label_id, boxes)                                                            # f32 [N, 1 + 4|5]

One kernel launch (csrc/groundtruth.hip: one wave per object) behind a device sort that groups the rows by (frame, object); the en
encoding adds the k = 1 search of ``ops.knn_graph``.  Two host reads per call: the number of objects and the status word.
There is no CPU path.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from .postprocessor import INVARIANCE_CODES, _nearest_in_frames

_STATUS_ERRORS = (
    (ops.STATUS_GT_OBJECT_TOO_LARGE, "RGNN_STATUS_GT_OBJECT_TOO_LARGE: an object has more than {cap} points"),
    (ops.STATUS_GT_DEGENERATE_OBJECT, "RGNN_STATUS_GT_DEGENERATE_OBJECT: an object of two coincident points, or of three or more "
                                      "points whose convex hull has no area (the reference divides by zero / raises QhullError)"),
)


def _check_status(status: torch.Tensor) -> None:
    st = int(status.item())
    fired = [msg.format(cap=ops.gt_object_cap()) for bit, msg in _STATUS_ERRORS if st & bit]
    if fired:
        raise ValueError("create_2D_bounding_boxes: " + "; ".join(fired))


def _cuda(x, name: str, dtype) -> torch.Tensor:
    t = torch.as_tensor(x)
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError(f"{name}: the ground-truth kernel needs a GPU (no CPU fallback)")
        t = t.cuda()
    return t.contiguous()


def create_2d_bounding_boxes_batched(pos, object_id, frame_ptr: Sequence[int], aligned: bool, bb_invariance: str,
                                     return_rect: bool = False):
    """Box targets of a batch of frames laid back to back, in one set of launches.
    ``pos`` [N, 2] (computed in float64); ``object_id`` int [N], negative = background, ids local to a frame and not
    necessarily dense; ``frame_ptr``: B + 1 row offsets (a host sequence; a tensor is read back once).
    -> float64 [N, 4] (aligned) or [N, 5] in HBM, NaN in the rows of background points; with ``return_rect`` also
    (rect f64 [n_obj, 5] = [x, y, l, w, theta in degrees, 0 <= theta < 180] per object, obj_ptr, obj_rows) -- the objects in
    (frame, id) order as ``ops.group_objects`` lists them.
    A refused object (more points than ``ops.gt_object_cap()``, or degenerate) raises ValueError naming the status bit."""
    if not aligned and bb_invariance not in INVARIANCE_CODES:
        raise ValueError("Wrong invariance for bounding box selection")
    inv = 0 if aligned else INVARIANCE_CODES[bb_invariance]          # (aligned boxes have one encoding)
    ptr = [int(v) for v in (frame_ptr.tolist() if isinstance(frame_ptr, torch.Tensor) else frame_ptr)]
    pos = _cuda(pos, "pos", torch.float64)
    oid = _cuda(object_id, "object_id", None)
    if oid.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64):
        raise ValueError("object_id must be an int tensor [N]")
    n = pos.shape[0]
    if pos.dim() != 2 or pos.shape[1] != 2 or oid.shape != (n,) or len(ptr) < 2 or ptr[0] != 0 or ptr[-1] != n:
        raise ValueError("shapes: pos [N, 2], object_id [N], frame_ptr from 0 to N")
    nn_index: Optional[torch.Tensor] = None
    if inv == 2 and not aligned:
        nn_index = _nearest_in_frames(pos, ptr)         # a frame of one point raises sklearn's error, as the reference does
    obj_ptr, obj_rows = ops.group_objects(oid, torch.tensor(ptr, dtype=torch.int64, device=pos.device))
    boxes, rect, status = ops.create_gt_boxes(pos, obj_ptr, obj_rows, nn_index, bool(aligned), inv, want_rect=return_rect)
    _check_status(status)
    if return_rect:
        return boxes, rect, obj_ptr, obj_rows
    return boxes


def merge_targets(label_id, boxes) -> torch.Tensor:
    """float32 [N, 1 + 4|5]: the ``y`` of create_graph_data (dataset_creation.py:800-807): class index | box."""
    boxes = _cuda(boxes, "boxes", None)
    labels = _cuda(np.asarray(label_id) if not isinstance(label_id, torch.Tensor) else label_id, "label_id", None)
    if boxes.dim() != 2 or labels.numel() != boxes.shape[0]:
        raise ValueError("one label per row of boxes")
    return torch.cat((labels.reshape(-1, 1).to(torch.float32), boxes.to(torch.float32)), dim=1)


class GroundTruthCreator:
    """dataset_creation.py:232-521 with the reference's method names.  ``point_cloud``: any object with ``X_cc`` [N, 2],
    ``track_id`` (byte strings, b'' = background) and ``label_id``."""

    @staticmethod
    def get_class_indices(point_cloud):
        return point_cloud.label_id

    @staticmethod
    def build_one_hot_vectors(point_cloud) -> np.ndarray:
        num_classes = 6
        label_id = np.asarray(point_cloud.label_id).reshape(-1)
        target = np.zeros([label_id.shape[0], num_classes])
        target[np.arange(label_id.shape[0]), label_id.astype(np.int64)] = 1
        return target

    @staticmethod
    def object_ids(point_cloud) -> np.ndarray:
        """int64 [N]: the rank of every point's track id among the frame's distinct ids, -1 for b''."""
        uniq, inverse = np.unique(np.asarray(point_cloud.track_id), return_inverse=True)
        ids = inverse.reshape(-1).astype(np.int64)
        ids[np.asarray(uniq == b"")[ids]] = -1
        return ids

    @classmethod
    def create_2D_bounding_boxes(cls, point_cloud, aligned: bool, bb_invariance: str) -> torch.Tensor:
        """-> float64 [N, 4|5] in HBM: every row the box of its point's object (NaN for background points)."""
        x_cc = np.asarray(point_cloud.X_cc)
        return create_2d_bounding_boxes_batched(x_cc, cls.object_ids(point_cloud), [0, x_cc.shape[0]], aligned, bb_invariance)
