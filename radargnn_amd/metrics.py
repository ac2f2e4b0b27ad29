"""Evaluation on the device: the step after the post-processor (the reference's ``evaluate.py:72-77``).  Mirrors of
``postprocessor/metrics.py`` (``ObjectDetectionMetrics``, ``SegmentationMetrics``), ``postprocessor/evaluation.py`` (``Evaluator``,
``get_new_evaluation_folder_path``), ``postprocessor/radarscenes/evaluation.py`` (``RadarscenesEvaluator``) and the
``evaluation_selector`` of ``postprocessor/__init__.py``, on librgnn's ``rgnn_point_iou`` / ``rgnn_box_iou`` / ``rgnn_map_match`` /
``rgnn_map_curves`` / ``rgnn_confusion_matrix``.  Inputs are what ``Postprocessor.process`` returns (tensors in HBM); lists of host
``BoundingBox`` objects and numpy arrays are uploaded once.

Differences from the reference, all deliberate:
  * only the COCO area range "all" is evaluated: the keys ``map_small`` ... ``mar_large`` are absent from the result (their pixel
    thresholds mean nothing in metres and nobody reads them);
  * every summary is a 0-dim float32 CPU tensor (the reference mixes 0-dim, [1] and an int64 ``tensor([-1])``);
  * an empty first frame does not raise; the kind of the boxes comes from ``BoundingBoxes.is_aligned``;
  * equal scores go by ascending position (the reference's ``torch.sort`` leaves ties unpinned);
  * the aligned box IoU restates ``torchvision.ops.box_iou`` and is not pinned by an executed torchvision;
  * ``"nuscenes"`` is absent from THIS ``evaluation_selector``: the nuScenes evaluator lives in ``radargnn_amd.nuscenes_eval``, whose own
    ``evaluation_selector`` holds both keys (it needs ground truth this module's callers do not have); no confusion plot is written.
"""
from __future__ import annotations

import abc
import json
import os
import re
from dataclasses import asdict
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .postprocessor import BoundingBoxes, PostProcessingConfiguration, _cuda

MAX_DETECTION_THRESHOLDS = (1, 10, 100)
# the message of the reference's exception (metrics.py:115-117), whose source line continues after 30 blanks
ROTATED_NEEDS_POINT_IOU = ("so far only Point-IOU based mAP calculation is possible for rotated bounding boxes," + " " * 30 +
                           "select 'use_point_iou = True' in configuration for rotated boxes")


def _frame_corners(boxes) -> "torch.Tensor | np.ndarray":
    if isinstance(boxes, BoundingBoxes):
        return boxes.corners.reshape(-1, 4, 2)
    return np.array([np.asarray(b.corners, dtype=np.float64) for b in boxes], dtype=np.float64).reshape(-1, 4, 2)


def _concat_cuda(parts: List, dtype: torch.dtype, tail: Sequence[int] = ()) -> torch.Tensor:
    """The per-frame arrays / tensors as ONE tensor on the device; host parts are concatenated first and uploaded once."""
    if parts and all(not isinstance(p, torch.Tensor) for p in parts):
        host = np.concatenate([np.asarray(p).reshape(-1, *tail) for p in parts])
        return _cuda(host, "evaluation input", dtype)
    if not parts:
        return _cuda(np.zeros((0, *tail)), "evaluation input", dtype)
    return torch.cat([_cuda(p, "evaluation input", dtype).reshape(-1, *tail) for p in parts])


def _boxes_are_aligned(*dict_lists) -> bool:
    for dicts in dict_lists:
        for d in dicts:
            boxes = d["boxes"]
            if isinstance(boxes, BoundingBoxes):
                return boxes.is_aligned
            if len(boxes):
                return bool(boxes[0].is_aligned)
    return True


def _box_matrices(dicts: List[Dict], aligned: bool):
    """-> (float32 [M, 4] [x_min, y_min, x_max, y_max] or [M, 5] [x, y, l, w, theta], box offsets of the frames as a list)."""
    corners = [_frame_corners(d["boxes"]) for d in dicts]
    ptr = [0]
    for c in corners:
        ptr.append(ptr[-1] + int(c.shape[0]))
    packed = _concat_cuda(corners, torch.float64, (4, 2))
    two_point, rotated = ops.box_representations(packed, two_point=aligned, rotated=not aligned)
    return (two_point if aligned else rotated).to(torch.float32), ptr


def _mean_valid(x: torch.Tensor, dims) -> torch.Tensor:
    """Mean of the entries greater than -1 over ``dims`` (float64), -1 where there is none (``_summarize``)."""
    valid = x > -1
    count = valid.sum(dim=dims)
    total = torch.where(valid, x, torch.zeros_like(x)).sum(dim=dims)
    return torch.where(count > 0, total / count.clamp(min=1), torch.full_like(total, -1.0))


class ObjectDetectionMetrics:
    """postprocessor/metrics.py:12-133."""

    @classmethod
    def get_map(cls, eval_config: PostProcessingConfiguration, bb_pred: List, bb_ground_truth: List, cls_pred: List) -> dict:
        """mAP / mAR of a list of frames at ``eval_config.iou_for_mAP`` -> dict of CPU tensors: ``map``, ``map_50``, ``map_75``,
        ``mar_1``, ``mar_10``, ``mar_100``, ``map_per_class``, ``mar_100_per_class``, plus ``classes`` (list), ``precision``
        [T, 101, K, 3] and ``recall`` [T, K, 3]."""
        return cls._get_map(eval_config, bb_pred, bb_ground_truth, cls_pred, [eval_config.iou_for_mAP])

    @classmethod
    def _get_map(cls, eval_config, bb_pred: List, bb_ground_truth: List, cls_pred: List, iou_thresholds: Sequence[float]) -> dict:
        n_frames = len(bb_pred)
        if n_frames == 0 or len(bb_ground_truth) != n_frames or len(cls_pred) != n_frames:
            raise ValueError("predictions, ground truth and positions need one entry per graph, and at least one graph")
        aligned = _boxes_are_aligned(bb_pred, bb_ground_truth)
        if not aligned and not eval_config.use_point_iou:
            raise Exception(ROTATED_NEEDS_POINT_IOU)
        boxes_pred, pred_ptr = _box_matrices(bb_pred, aligned)
        boxes_gt, gt_ptr = _box_matrices(bb_ground_truth, aligned)
        det_scores = _concat_cuda([d["scores"] for d in bb_pred], torch.float32)
        det_labels = _concat_cuda([d["labels"] for d in bb_pred], torch.float64).to(torch.int32)      # torch.long truncates too
        gt_labels = _concat_cuda([d["labels"] for d in bb_ground_truth], torch.float64).to(torch.int32)
        if det_scores.numel() != pred_ptr[-1] or det_labels.numel() != pred_ptr[-1] or gt_labels.numel() != gt_ptr[-1]:
            raise ValueError("one score and label per predicted box, one label per ground-truth box")
        if eval_config.use_point_iou:
            pos = [d["pos"] for d in cls_pred]
            frame_ptr = [0]
            for p in pos:
                frame_ptr.append(frame_ptr[-1] + int(torch.as_tensor(p).reshape(-1, 2).shape[0]))
            points = _concat_cuda(pos, torch.float32, (2,))
            iou, _ = ops.point_iou(boxes_pred, pred_ptr, boxes_gt, gt_ptr, points, frame_ptr, not aligned)
        else:
            iou, _ = ops.box_iou(boxes_pred, pred_ptr, boxes_gt, gt_ptr)
        classes = torch.unique(torch.cat((det_labels, gt_labels)))                                       # sorted (_get_classes)
        rank, matched = ops.map_match(iou, pred_ptr, gt_ptr, det_labels, det_scores, gt_labels, classes, iou_thresholds,
                                      MAX_DETECTION_THRESHOLDS[-1])
        precision, _, recall = ops.map_curves(det_labels, det_scores, rank, matched, gt_labels, classes, MAX_DETECTION_THRESHOLDS)
        return cls._summarize(precision, recall, classes, [float(t) for t in iou_thresholds])

    @staticmethod
    def _summarize(precision: torch.Tensor, recall: torch.Tensor, classes: torch.Tensor, thresholds: List[float]) -> dict:
        """``_summarize`` / ``compute`` (torchmetrics_mean_ap.py:749-794, 975-1030) on the device in float64; one copy to the host."""
        p, r = precision.to(torch.float64), recall.to(torch.float64)
        last = p[..., -1]                                                                                # [T, R, K] at max_det 100
        minus_one = torch.full((), -1.0, dtype=torch.float64, device=p.device)
        head = [_mean_valid(last, (0, 1, 2))]
        for value in (0.5, 0.75):
            head.append(_mean_valid(last[thresholds.index(value)], (0, 1)) if value in thresholds else minus_one)
        head += [_mean_valid(r[..., m], (0, 1)) for m in range(r.shape[-1])]
        k = classes.numel()
        packed = torch.cat((torch.stack(head), _mean_valid(last, (0, 1)), _mean_valid(r[..., -1], (0,)))).to(torch.float32).cpu()
        res = {name: packed[i] for i, name in enumerate(("map", "map_50", "map_75") + tuple(f"mar_{m}" for m in MAX_DETECTION_THRESHOLDS))}
        res["map_per_class"] = packed[6:6 + k]
        res[f"mar_{MAX_DETECTION_THRESHOLDS[-1]}_per_class"] = packed[6 + k:6 + 2 * k]
        res["classes"] = classes.cpu().tolist()
        res["precision"], res["recall"] = precision.cpu(), recall.cpu()
        return res


def _f1(ext: np.ndarray, average: Optional[str]):
    """sklearn's f1_score for labels = range(K) from the extended confusion matrix (row / column K = labels outside 0 .. K-1, which
    still count as false negatives / positives): 2 tp / (2 tp + fp + fn) in float64, 0 where the denominator is 0."""
    k = ext.shape[0] - 1
    tp = np.diag(ext)[:k].astype(np.float64)
    fp = ext[:, :k].sum(axis=0) - tp
    fn = ext[:k, :].sum(axis=1) - tp

    def ratio(num, den):
        num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
        return np.where(den == 0, 0.0, num / np.where(den == 0, 1.0, den))

    if average == "micro":
        return np.float64(ratio(2 * tp.sum(), 2 * tp.sum() + fp.sum() + fn.sum()))
    f = ratio(2 * tp, 2 * tp + fp + fn)
    if average is None:
        return f
    if average == "macro":
        return np.float64(f.mean()) if k else np.float64(0.0)
    if average == "weighted":
        support = tp + fn
        return np.float64((f * support).sum() / support.sum()) if support.sum() else np.float64(0.0)
    raise ValueError(f"average has to be one of (None, 'micro', 'macro', 'weighted'), got {average!r}")


class SegmentationMetrics:
    """postprocessor/metrics.py:136-196: F1 and confusion matrices of the node labels of all frames.  One launch per number of
    classes builds the [K + 1, K + 1] matrix (the extra row / column holds the labels outside 0 .. K-1, which scikit-learn leaves out
    of the confusion matrix but counts in the F1); everything else derives from it on the host in float64.  Returns numpy like
    scikit-learn.  NaN labels raise ValueError; at most 63 classes."""

    def __init__(self, cls_pred_label: List, cls_ground_truth: List):
        self.y_true = _concat_cuda([d["labels"] for d in cls_ground_truth], torch.float64).reshape(-1)
        self.y_pred = _concat_cuda(list(cls_pred_label), torch.float64).reshape(-1)
        if self.y_true.numel() != self.y_pred.numel():
            raise ValueError("Found input variables with inconsistent numbers of samples: "
                             f"[{self.y_true.numel()}, {self.y_pred.numel()}]")
        self._extended: Dict[int, np.ndarray] = {}

    def _matrix(self, num_classes: int) -> np.ndarray:
        k = int(num_classes)
        if k not in self._extended:
            def binned(y):
                t = torch.trunc(y)
                return torch.where(((t >= 0) & (t < k)) | torch.isnan(t), t, torch.full_like(t, float(k)))
            self._extended[k] = ops.confusion_matrix(binned(self.y_true), binned(self.y_pred), k + 1).cpu().numpy()
        return self._extended[k]

    def get_f1(self, num_classes: int, average: Optional[str]):
        return _f1(self._matrix(num_classes), average)

    def get_confusion_matrix(self, num_classes: int) -> np.ndarray:
        k = int(num_classes)
        return self._matrix(k)[:k, :k].copy()

    def get_confusion_matrices_per_class(self, num_classes: int) -> np.ndarray:
        ext = self._matrix(num_classes)
        k = ext.shape[0] - 1
        tp = np.diag(ext)[:k]
        fp = ext[:, :k].sum(axis=0) - tp
        fn = ext[:k, :].sum(axis=1) - tp
        tn = ext.sum() - tp - fp - fn
        return np.stack((tn, fp, fn, tp), axis=1).reshape(k, 2, 2).astype(np.int64)


class Evaluator(abc.ABC):
    """Base of the dataset evaluators (postprocessor/evaluation.py:8-20): holds the configuration and the class names, the object
    classes of ``min_object_score`` in their order with "background" at ``bg_index``."""

    def __init__(self, config: PostProcessingConfiguration, *args, **kwargs):
        object_names = list(config.min_object_score)
        self.config = config
        self.names = object_names[:config.bg_index] + ["background"] + object_names[config.bg_index:]

    @abc.abstractmethod
    def evaluate(self, predictions: Dict[str, List], ground_truth: Dict[str, Dict], num_predictions: int, pos: List) -> None:
        """Computes the metrics and keeps them on the evaluator."""

    @abc.abstractmethod
    def save_results(self, path_to_model_folder: str) -> None:
        """Writes what ``evaluate`` kept into a new evaluation folder below ``path_to_model_folder``."""


_TRAILING_NUMBER = re.compile(r"_(\d+)$")


def get_new_evaluation_folder_path(path: str) -> str:
    """``<path>/evaluation_NN`` for the next evaluation of a model (postprocessor/evaluation.py:23-61): NN is one more than the
    largest number that ends the name of a sub-folder of ``path`` after an underscore, 01 without sub-folders, two digits at least."""
    folders = [entry.name for entry in os.scandir(path) if entry.is_dir() and not entry.name.startswith(".")]
    taken = [int(found.group(1)) for found in map(_TRAILING_NUMBER.search, folders) if found]
    if folders and not taken:
        raise ValueError("max() arg is an empty sequence")          # what the reference's max() over no numbers raises
    return f"{path}/evaluation_{max(taken, default=0) + 1:02d}"


def _write_json(path: str, content: dict) -> None:
    with open(path, "w") as fh:
        json.dump(content, fh, indent=4)


class RadarscenesEvaluator(Evaluator):
    """mAP, segmentation F1 and confusion matrices of a RadarScenes evaluation run (postprocessor/radarscenes/evaluation.py:12-97,
    without the confusion plot).  Each part is switched by its flag of the configuration; a part that is off stays ``None``."""

    def __init__(self, config: PostProcessingConfiguration, *args, **kwargs):
        super().__init__(config, *args, **kwargs)
        self.mAP = self.mAP_per_class = self.f1_segmentation = None
        self.confusion_absolute = self.confusion_relative = None

    def evaluate(self, bb_pred, bb_ground_truth, cls_pred, cls_pred_label, cls_ground_truth, *args, **kwargs) -> None:
        cfg, n_classes = self.config, len(self.names)
        if cfg.get_mAP:
            detection = ObjectDetectionMetrics.get_map(cfg, bb_pred, bb_ground_truth, cls_pred)
            self.mAP = detection["map"].item()
            self.mAP_per_class = detection["map_per_class"].detach().numpy()
        segmentation = SegmentationMetrics(cls_pred_label, cls_ground_truth)
        if cfg.get_segmentation_f1:
            self.f1_segmentation = segmentation.get_f1(n_classes, cfg.f1_class_averaging)
        if cfg.get_confusion:
            counts = segmentation.get_confusion_matrix(n_classes)
            per_true_label = counts.sum(axis=1, keepdims=True).astype(np.float64)
            self.confusion_absolute = counts
            self.confusion_relative = counts / np.where(per_true_label == 0, 1e-8, per_true_label)   # empty rows divide by 1e-8

    def save_results(self, path_to_model_folder, *args, **kwargs):
        folder = get_new_evaluation_folder_path(path_to_model_folder)
        os.mkdir(folder)
        cfg = self.config
        detection = {"mAP": self.mAP, "mAP_per_class": self.mAP_per_class.tolist()} if cfg.get_mAP else {}
        f1 = self.f1_segmentation
        segmentation = {"f1": f1.tolist() if isinstance(f1, np.ndarray) else f1} if cfg.get_segmentation_f1 else {}
        _write_json(os.path.join(folder, "eval_configs.json"), {"EVALUATION_CONFIG": asdict(cfg)})
        _write_json(os.path.join(folder, "eval_results.json"),
                    {"OBJECT_DETECTION_METRICS": detection, "SEMANTIC_SEGMENTATION_METRICS": segmentation})
        if cfg.get_confusion:
            # ("convusion" is the reference's file name)
            for name, matrix in (("confusion_abs.npy", self.confusion_absolute), ("convusion_rel.npy", self.confusion_relative)):
                np.save(os.path.join(folder, name), matrix)


evaluation_selector: Dict[str, type] = {"radarscenes": RadarscenesEvaluator}
