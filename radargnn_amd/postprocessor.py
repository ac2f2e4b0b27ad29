"""Post-processor front half on the device: mirrors of the reference's
``postprocessor/configs.py::PostProcessingConfiguration`` and ``postprocessor/postprocessing.py::PredictionExtractor``
(labels, scores, background scores, score filtering, relative -> absolute box decoding) on librgnn's
``rgnn_decode_predictions``.  Inputs may be numpy arrays (as the reference passes them) or CUDA tensors (straight
from ``frames.HotPath`` / the model heads, nothing leaves the device); results stay in HBM.

The E(n)-invariant box representation needs every point's nearest neighbour: the k = 1 use of the kNN kernel
(``ops.knn_graph``) instead of sklearn + a dense N x N ``toarray()`` (postprocessing.py:233-237).

The evaluation half: ``GroundTruthExtractor`` (ground-truth decode + duplicate removal, postprocessing.py:438-575),
``Postprocessor.process`` over whole lists of frames (one decode launch per half, one duplicate-removal launch, one
segmented NMS: ``BoxSuppressor.apply_nms_frames`` -> ``Detections``) and the point IoU of ``utils/math.py:176-211`` (``point_iou``, ``point_iou_batched``) on
``rgnn_decode_ground_truth`` / ``rgnn_remove_duplicate_boxes`` / ``rgnn_point_iou``.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import ops

INVARIANCE_CODES = {"none": 0, "translation": 1, "en": 2}


@dataclass
class PostProcessingConfiguration:
    """postprocessor/configs.py:5-27 (same field names and defaults)."""
    split: str = "test"
    iou_for_nms: float = 0.3
    min_object_score: Dict[str, float] = field(default_factory=dict)
    max_score_for_background: float = 1.0
    iou_for_mAP: float = 0.3
    use_point_iou: bool = False
    bg_index: int = 5
    bb_invariance: str = "translation"
    adapt_orientation_angle: bool = False
    get_mAP: bool = True
    get_confusion: bool = True
    get_segmentation_f1: bool = True
    f1_class_averaging: Optional[str] = None


class BoundingBox:
    """One absolute box as the reference's ``preprocessor/bounding_box.py::BoundingBox``: ``corners`` [4, 2] numpy."""

    def __init__(self, corners: np.ndarray, aligned: bool):
        self.corners = corners
        self.is_aligned = aligned
        self.is_rotated = not aligned


class BoundingBoxes:
    """The decoded boxes of one graph in HBM: ``corners`` float64 [M, 4, 2].  Behaves like the list of ``BoundingBox``
    objects the reference returns (``len``, indexing, iteration copy to the host on demand)."""

    def __init__(self, corners: torch.Tensor, aligned: bool):
        self.corners = corners
        self.is_aligned = aligned
        self.is_rotated = not aligned

    def __len__(self) -> int:
        return self.corners.shape[0]

    def __getitem__(self, i) -> BoundingBox:
        return BoundingBox(self.corners[i].cpu().numpy(), self.is_aligned)

    def __iter__(self):
        host = self.corners.cpu().numpy()
        return (BoundingBox(host[i], self.is_aligned) for i in range(host.shape[0]))

    def two_point(self) -> torch.Tensor:
        """[x_min, y_min, x_max, y_max] per box (``BoundingBox.get_two_point_representations``), float64 [M, 4]."""
        return torch.cat((self.corners.min(dim=1).values, self.corners.max(dim=1).values), dim=1)


def _f32_cuda(a, name: str) -> torch.Tensor:
    t = torch.as_tensor(a)
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError(f"{name}: the post-processor kernels need a GPU (no CPU fallback)")
        t = t.cuda()
    return t.contiguous()


def decode(class_probability_prediction, bounding_box_predictions, pos, config: PostProcessingConfiguration,
           nn_index: Optional[torch.Tensor] = None, frame_ptr: Optional[torch.Tensor] = None):
    """Per-node results for a graph or a whole batch, everything on the device:
    -> (label int32 [N], score f32 [N], keep int32 [N], corners f64 [N, 4, 2]).  ``frame_ptr`` (int64 [B+1]): node offsets
    of the frames of a batch, so that nearest neighbours for the "en" representation are searched inside each frame."""
    prob = _f32_cuda(class_probability_prediction, "class_probability_prediction")
    bb = _f32_cuda(bounding_box_predictions, "bounding_box_predictions")
    p = _f32_cuda(pos, "pos")
    n, k = prob.shape
    if bb.shape[0] != n or p.shape != (n, 2) or bb.shape[1] not in (4, 5):
        raise ValueError("shapes: class probabilities [N, K], boxes [N, 4|5], pos [N, 2]")
    if config.bb_invariance not in INVARIANCE_CODES:
        raise ValueError(f"unknown bb_invariance {config.bb_invariance!r}")
    inv = INVARIANCE_CODES[config.bb_invariance]
    if inv == 2 and bb.shape[1] == 5 and n and nn_index is None:
        ptr = frame_ptr if frame_ptr is not None else torch.tensor([0, n], dtype=torch.int64, device=p.device)
        if int((ptr[1:] - ptr[:-1]).min()) <= 1:
            raise ValueError("Expected n_neighbors < n_samples_fit, but n_neighbors = 1, n_samples_fit = 1")   # sklearn's error
        nn_index, _, _ = ops.knn_graph(p.to(torch.float64), ptr, 1, want_edge_index=False)
        nn_index = nn_index.view(-1)
    return ops.decode_predictions(prob, bb, p, nn_index, config.bg_index, config.max_score_for_background,
                                  list(config.min_object_score.values()), inv, config.adapt_orientation_angle)


class PredictionExtractor:
    """postprocessor/postprocessing.py:166-319, same method names and result shapes ([N, 1] columns); tensors in HBM."""

    @staticmethod
    def _prob(class_probability_prediction) -> torch.Tensor:
        return _f32_cuda(class_probability_prediction, "class_probability_prediction")

    @classmethod
    def get_predicted_label(cls, class_probability_prediction) -> torch.Tensor:
        prob = cls._prob(class_probability_prediction)
        label, _ = ops.row_argmax(prob)
        return label.to(torch.float64).view(-1, 1)

    @classmethod
    def get_prediction_scores(cls, class_probability_prediction) -> torch.Tensor:
        prob = cls._prob(class_probability_prediction)
        _, score = ops.row_argmax(prob)
        return score.to(torch.float64).view(-1, 1)

    @classmethod
    def get_clutter_scores(cls, class_probability_prediction, bg_index: int) -> torch.Tensor:
        return cls._prob(class_probability_prediction)[:, bg_index].reshape(-1, 1)

    @classmethod
    def get_absolute_object_bounding_box_predictions(cls, class_probability_prediction, bounding_box_predictions, pos,
                                                     config: PostProcessingConfiguration
                                                     ) -> Tuple[BoundingBoxes, torch.Tensor, torch.Tensor]:
        """-> (boxes of the nodes that survive the score filters, their scores [M, 1] f64, their labels [M, 1] f64), in node
        order like the reference's ``np.delete``.  One host read (M) sizes the outputs."""
        label, score, keep, corners = decode(class_probability_prediction, bounding_box_predictions, pos, config)
        idx = torch.nonzero(keep, as_tuple=False).view(-1)
        aligned = torch.as_tensor(bounding_box_predictions).shape[1] == 4
        return (BoundingBoxes(corners.index_select(0, idx), aligned),
                score.index_select(0, idx).to(torch.float64).view(-1, 1),
                label.index_select(0, idx).to(torch.float64).view(-1, 1))

    def extract(self, predictions: Dict) -> List[torch.Tensor]:
        """postprocessing.py:321-333: the predicted label [N, 1] (float64) of every node of every graph; one launch for all."""
        frames = predictions.get("class_probability_prediction")
        prob = _concat(frames, "class_probability_prediction")
        label, _ = ops.row_argmax(prob)
        label = label.to(torch.float64).view(-1, 1)
        sizes = [int(torch.as_tensor(f).shape[0]) for f in frames]
        return list(torch.split(label, sizes)) if sizes else []

class BoxSuppressor:
    """postprocessor/postprocessing.py:336-431: non-maximum suppression of one graph's decoded boxes, rotated
    (detectron2 ``nms_rotated`` semantics) or aligned (``torchvision.ops.nms`` semantics) by the kind of the boxes."""

    @classmethod
    def apply_nms(cls, bounding_boxes: BoundingBoxes, box_scores: torch.Tensor, box_labels: torch.Tensor, iou_nms: float):
        """-> (boxes kept, their scores [M', 1], their labels [M', 1]), by descending score like the reference."""
        return cls._apply_nms_ids(bounding_boxes, box_scores, box_labels, iou_nms)[:3]

    @classmethod
    def _apply_nms_ids(cls, bounding_boxes: BoundingBoxes, box_scores: torch.Tensor, box_labels: torch.Tensor, iou_nms: float):
        """``apply_nms`` and the ids kept (int64, positions in ``bounding_boxes``)."""
        if len(bounding_boxes) == 0:
            return bounding_boxes, box_scores, box_labels, torch.empty(0, dtype=torch.int64, device=box_scores.device)
        corners = bounding_boxes.corners
        if bounding_boxes.is_rotated:
            _, mat = ops.box_representations(corners, two_point=False, rotated=True)
            lo = mat[:, :2].min()                                   # postprocessing.py:358-361: all centres made positive
            if float(lo) < 0:
                mat = mat.clone()
                mat[:, :2] += abs(float(lo)) + 100
            keep = ops.nms(mat, box_scores.reshape(-1).to(torch.float64), iou_nms, rotated=True)
            kept_boxes = BoundingBoxes(corners.index_select(0, keep), False)
            scores = box_scores.reshape(-1).to(torch.float64).index_select(0, keep).view(-1, 1)
        else:
            mat, _ = ops.box_representations(corners, two_point=True, rotated=False)
            lo = float(mat.min())                                   # postprocessing.py:391-394
            shift = abs(lo) + 100 if lo < 0 else 0.0
            mat32 = (mat + shift).to(torch.float32) if shift else mat.to(torch.float32)
            s32 = box_scores.reshape(-1).to(torch.float32)
            keep = ops.nms(mat32, s32, iou_nms, rotated=False)
            kept = mat32.index_select(0, keep)                      # the reference rebuilds the boxes from the float32 matrix
            if shift:
                kept = kept - torch.tensor(shift, dtype=torch.float32, device=kept.device)
            x0, y0, x1, y1 = kept[:, 0], kept[:, 1], kept[:, 2], kept[:, 3]
            rebuilt = torch.stack((x0, y0, x0, y1, x1, y0, x1, y1), dim=1).view(-1, 4, 2)   # corner order of :416-423
            kept_boxes = BoundingBoxes(rebuilt, True)
            scores = s32.index_select(0, keep).view(-1, 1)
        labels = box_labels.reshape(-1).index_select(0, keep).view(-1, 1)
        return kept_boxes, scores, labels, keep

    @classmethod
    def apply_nms_frames(cls, corners: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor, keep: torch.Tensor, frame_ptr,
                         iou_nms: float, aligned: bool) -> "Detections":
        """``apply_nms`` for every frame of a batch at once, on the outputs of ``decode`` (corners f64 [N, 4, 2], scores f32
        [N], labels int32 [N], keep int32 [N]) and the node offsets of the frames: the candidates of each frame (keep != 0),
        its own shift of negative coordinates, its own score order and greedy pass -- bit for bit what ``apply_nms`` returns
        for the frame alone -- in two launches and one host read per batch (``ops.nms_frames``).  A frame with more
        candidates than the kernel takes goes through ``apply_nms`` after that read and is spliced in."""
        ptr_dev = _cuda(frame_ptr, "frame_ptr", torch.int64).reshape(-1)
        node, out_labels, out_scores, out_corners, ptr, candidates = ops.nms_frames(labels, scores, keep, corners, ptr_dev,
                                                                                     iou_nms, rotated=not aligned)
        det = Detections(out_corners, out_scores, out_labels, node, ptr, aligned)
        oversize = torch.nonzero(candidates > ops.nms_frames_max_candidates()).view(-1).tolist()
        if not oversize:
            return det
        bounds = ptr_dev.cpu().tolist()
        parts, new_ptr = [], [0]
        for f in range(len(det)):
            a, b = int(ptr[f]), int(ptr[f + 1])
            part = (out_corners[a:b], out_scores[a:b], out_labels[a:b], node[a:b])
            if f in oversize:
                lo, hi = bounds[f], bounds[f + 1]
                idx = torch.nonzero(keep[lo:hi], as_tuple=False).view(-1)
                boxes, sc, lb, ids = cls._apply_nms_ids(BoundingBoxes(corners[lo:hi].index_select(0, idx), aligned),
                                                        scores[lo:hi].index_select(0, idx).to(torch.float64).view(-1, 1),
                                                        labels[lo:hi].index_select(0, idx).to(torch.float64).view(-1, 1), iou_nms)
                part = (boxes.corners, sc[:, 0], lb[:, 0], idx.index_select(0, ids) + lo)
            parts.append(part)
            new_ptr.append(new_ptr[-1] + part[0].shape[0])
        cat = [torch.cat([p[i] for p in parts]) for i in range(4)]
        return Detections(cat[0], cat[1], cat[2], cat[3], torch.tensor(new_ptr, dtype=torch.int64), aligned)


class Detections:
    """The suppressed detections of a batch of frames in HBM, packed frame after frame: ``corners`` [K, 4, 2], ``scores``
    [K] (float64 for rotated boxes; float32 for aligned ones, whose corners are the reference's float32 rebuild),
    ``labels`` float64 [K], ``node`` int64 [K] (node id in the batch) and ``ptr`` int64 [B + 1] (frame offsets in K, on
    the host).  ``len()`` is the number of frames."""

    def __init__(self, corners, scores, labels, node, ptr, aligned: bool):
        self.corners, self.scores, self.labels, self.node, self.ptr = corners, scores, labels, node, ptr
        self.is_aligned = aligned
        self._bounds = ptr.tolist()

    def __len__(self) -> int:
        return len(self._bounds) - 1

    def frame(self, f: int) -> Dict:
        """{"boxes", "scores", "labels"} of frame f as views -- the detection dict of ``Postprocessor``.  A frame without
        detections had no candidates: it gets the empty float64 tensors ``apply_nms`` hands back for an empty input."""
        a, b = self._bounds[f], self._bounds[f + 1]
        if a == b:
            dev = self.labels.device
            return {"boxes": BoundingBoxes(torch.empty((0, 4, 2), dtype=torch.float64, device=dev), self.is_aligned),
                    "scores": torch.empty(0, dtype=torch.float64, device=dev), "labels": torch.empty(0, dtype=torch.float64, device=dev)}
        return {"boxes": BoundingBoxes(self.corners[a:b], self.is_aligned), "scores": self.scores[a:b], "labels": self.labels[a:b]}


class Postprocessor:
    """postprocessor/postprocessing.py:14-163: decode + NMS + the per-node segmentation outputs of the predictions, the
    ground-truth boxes without duplicates, as the dicts the reference returns -- values are tensors in HBM instead of numpy
    arrays."""

    @staticmethod
    def process_one_raw_prediction(config: PostProcessingConfiguration, pos, raw_bb_pred, raw_cls_prob_pred):
        label, score, keep, corners = decode(raw_cls_prob_pred, raw_bb_pred, pos, config)
        return Postprocessor._finish(config, _f32_cuda(pos, "pos"), _f32_cuda(raw_cls_prob_pred, "cls"), label, score,
                                     keep, corners, torch.as_tensor(raw_bb_pred).shape[1] == 4)

    @staticmethod
    def _finish(config, pos, prob, label, score, keep, corners, aligned):
        idx = torch.nonzero(keep, as_tuple=False).view(-1)
        boxes = BoundingBoxes(corners.index_select(0, idx), aligned)
        scores = score.index_select(0, idx).to(torch.float64).view(-1, 1)
        labels = label.index_select(0, idx).to(torch.float64).view(-1, 1)
        boxes, scores, labels = BoxSuppressor.apply_nms(boxes, scores, labels, config.iou_for_nms)
        detection = {"boxes": boxes, "scores": scores[:, 0], "labels": labels[:, 0]}
        return detection, Postprocessor._segmentation(config, pos, prob, label, score)

    @staticmethod
    def process_one_ground_truth(pos, vel, raw_bb_ground_truth, raw_cls_ground_truth, bb_invariance: str, bg_index: int):
        """postprocessing.py:81-118: ground-truth boxes of one graph without duplicates, and the ground-truth segmentation."""
        boxes, labels = GroundTruthExtractor.get_absolute_object_bounding_boxes(raw_cls_ground_truth, raw_bb_ground_truth, pos,
                                                                                bb_invariance, bg_index)
        boxes, labels = GroundTruthExtractor.remove_duplicate_boxes(boxes, labels)
        objects = {"boxes": boxes, "labels": labels[:, 0]}
        segmentation = {"pos": _f32_cuda(pos, "pos"), "vel": None if vel is None else _cuda(vel, "vel", None),
                        "labels": _cuda(raw_cls_ground_truth, "class_true", None)}
        return objects, segmentation

    def process(self, config: PostProcessingConfiguration, raw_pos, raw_vel, predictions: Dict, ground_truth: Dict):
        """postprocessing.py:120-163 over lists of graphs (numpy, as ``Predictor.predict`` returns them, or CUDA tensors):
        -> (bb_pred, bb_ground_truth, cls_pred, cls_ground_truth), lists of dicts with the reference's keys.  One decode launch
        per half over all graphs, one duplicate-removal launch, one segmented NMS (``apply_nms_frames``)."""
        raw_bb_pred = predictions.get("bounding_box_predictions")
        raw_cls_prob_pred = predictions.get("class_probability_prediction")
        raw_bb_gt = ground_truth.get("bounding_box_true")
        raw_cls_gt = ground_truth.get("class_true")
        frames = [raw_pos, raw_bb_pred, raw_cls_prob_pred, raw_bb_gt, raw_cls_gt]
        n_frames = len(raw_pos)
        if any(len(f) != n_frames for f in frames) or (raw_vel is not None and len(raw_vel) != n_frames):
            raise ValueError("positions, velocities, predictions and ground truth need one entry per graph")
        if n_frames == 0:
            return [], [], [], []
        ptr = [0]
        for p in raw_pos:
            ptr.append(ptr[-1] + int(torch.as_tensor(p).shape[0]))
        pos = _concat(raw_pos, "pos")
        bb_pred, cls_prob = _concat(raw_bb_pred, "bounding_box_predictions"), _concat(raw_cls_prob_pred, "class_probability_prediction")
        bb_gt = _concat(raw_bb_gt, "bounding_box_true")
        labels_gt = _concat([_labels_column(c) for c in raw_cls_gt], "class_true", None)
        nn_index = _nearest_in_frames(pos, ptr) if config.bb_invariance == "en" else None

        # predictions: one decode launch, one segmented suppression
        label, score, keep, corners = decode(cls_prob, bb_pred, pos, config, nn_index=nn_index)
        pairs = Postprocessor._finish_frames(config, pos, cls_prob, label, score, keep, corners, bb_pred.shape[1] == 4, ptr)
        bb_out, cls_out = [p[0] for p in pairs], [p[1] for p in pairs]

        # ground truth: one decode launch, one duplicate-removal launch
        gt_corners, gt_labels, box_ptr = _ground_truth(labels_gt, bb_gt, pos, ptr, config.bb_invariance, config.bg_index, nn_index)
        bounds = box_ptr.cpu().tolist()
        aligned_gt = bb_gt.shape[1] == 4
        gt_out, gt_seg = [], []
        for f in range(n_frames):
            a, b = bounds[f], bounds[f + 1]
            gt_out.append({"boxes": BoundingBoxes(gt_corners[a:b], aligned_gt), "labels": gt_labels[a:b]})
            vel = None if raw_vel is None else _cuda(raw_vel[f], "vel", None)
            gt_seg.append({"pos": pos[ptr[f]:ptr[f + 1]], "vel": vel, "labels": labels_gt[ptr[f]:ptr[f + 1]]})
        return bb_out, gt_out, cls_out, gt_seg

    @staticmethod
    def _segmentation(config, pos, prob, label, score) -> Dict:
        return {"pos": pos, "labels": label.to(torch.float64), "scores": score.to(torch.float64),
                "clutter_scores": prob[:, config.bg_index]}

    @staticmethod
    def _finish_frames(config, pos, prob, label, score, keep, corners, aligned, bounds: List[int]):
        """``_finish`` for the frames [bounds[f], bounds[f + 1]) of one decode: list of (detection, segmentation) dicts.  More
        than one frame: one segmented suppression, the dicts are slices of its result.  A single frame stays on ``_finish``:
        ``rgnn_nms`` spreads the frame's IoUs over the whole device, the segmented kernel gives a frame one work-group
        (MEASUREMENTS.md row 3)."""
        if len(bounds) <= 2:
            return [Postprocessor._finish(config, pos[a:b], prob[a:b], label[a:b], score[a:b], keep[a:b], corners[a:b], aligned)
                    for a, b in zip(bounds[:-1], bounds[1:])]
        det = BoxSuppressor.apply_nms_frames(corners, score, label, keep, torch.tensor(bounds, dtype=torch.int64), config.iou_for_nms,
                                             aligned)
        seg = Postprocessor._segmentation(config, pos, prob, label, score)
        return [(det.frame(f), {k: v[a:b] for k, v in seg.items()}) for f, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))]

    @staticmethod
    def detect_batch(config: PostProcessingConfiguration, pos, raw_bb_pred, raw_cls_prob_pred, ptr):
        """Decode and segmented suppression of a whole batch (``Batch.ptr`` / ``FrameBatch.frame_ptr`` node offsets): three
        launches (plus the neighbour search of the "en" boxes) and one host read, whatever the number of frames.
        -> (``Detections``, the segmentation tensors of the batch: {"pos", "labels", "scores", "clutter_scores"} over all
        nodes)."""
        ptr_dev = _cuda(ptr, "ptr", torch.int64)
        label, score, keep, corners = decode(raw_cls_prob_pred, raw_bb_pred, pos, config, frame_ptr=ptr_dev)
        det = BoxSuppressor.apply_nms_frames(corners, score, label, keep, ptr_dev, config.iou_for_nms,
                                             torch.as_tensor(raw_bb_pred).shape[1] == 4)
        return det, Postprocessor._segmentation(config, _f32_cuda(pos, "pos"), _f32_cuda(raw_cls_prob_pred, "cls"), label, score)

    @staticmethod
    def process_batch(config: PostProcessingConfiguration, pos, raw_bb_pred, raw_cls_prob_pred, ptr):
        """The same for a whole batch straight from the model (``Batch.ptr`` / ``FrameBatch.frame_ptr`` node offsets): ONE
        decode launch over all nodes (nearest neighbours for the "en" boxes searched per frame), then one segmented
        suppression (postprocessing.py:150-154 for every frame at once).  -> list of (detection, segmentation) dicts."""
        ptr_dev = _cuda(ptr, "ptr", torch.int64)
        label, score, keep, corners = decode(raw_cls_prob_pred, raw_bb_pred, pos, config, frame_ptr=ptr_dev)
        pos32, prob = _f32_cuda(pos, "pos"), _f32_cuda(raw_cls_prob_pred, "cls")
        aligned = torch.as_tensor(raw_bb_pred).shape[1] == 4
        return Postprocessor._finish_frames(config, pos32, prob, label, score, keep, corners, aligned, ptr_dev.cpu().tolist())


# ---------------------------------------------------------------------------------------------------- evaluation half
def _cuda(a, name: str, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    t = torch.as_tensor(a)
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError(f"{name}: the post-processor kernels need a GPU (no CPU fallback)")
        t = t.cuda()
    return t.contiguous()


def _concat(frames, name: str, dtype: Optional[torch.dtype] = torch.float32) -> torch.Tensor:
    """One CUDA tensor of a list of per-frame arrays / tensors (rows concatenated)."""
    parts = [_cuda(f, name, dtype) for f in frames]
    return torch.cat(parts, dim=0) if len(parts) > 1 else parts[0]


def _nearest_in_frames(pos: torch.Tensor, ptr: List[int]) -> torch.Tensor:
    """int32 [N]: every point's nearest other point of its frame (kneighbors_graph(pos, 1), postprocessing.py:463-467).
    A frame of one point raises sklearn's error; empty frames are skipped, as the reference skips them."""
    sizes = [b - a for a, b in zip(ptr[:-1], ptr[1:])]
    if any(n == 1 for n in sizes):
        raise ValueError("Expected n_neighbors < n_samples_fit, but n_neighbors = 1, n_samples_fit = 1")   # sklearn's error
    if ptr[-1] == 0:
        return torch.empty(0, dtype=torch.int32, device=pos.device)
    bounds = [ptr[0]] + [b for a, b in zip(ptr[:-1], ptr[1:]) if b > a]
    nn, _, _ = ops.knn_graph(pos.to(torch.float64), torch.tensor(bounds, dtype=torch.int64, device=pos.device), 1,
                             want_edge_index=False)
    return nn.view(-1)


def _offsets(keep: torch.Tensor, ptr: torch.Tensor) -> torch.Tensor:
    """int64 [B + 1]: offsets of the kept rows of each segment (segments given by ptr, int64 on the device)."""
    csum = torch.cat((torch.zeros(1, dtype=torch.int64, device=keep.device), torch.cumsum(keep, 0, dtype=torch.int64)))
    return csum.index_select(0, ptr)


def _labels_column(class_labels) -> torch.Tensor:
    t = torch.as_tensor(class_labels)
    if t.dim() == 2 and t.shape[1] == 1:
        t = t.view(-1)
    if t.dim() != 1:
        raise ValueError("class labels must be [N] or [N, 1]")
    return _cuda(t, "class_labels", None)


def _ground_truth(labels: torch.Tensor, boxes: torch.Tensor, pos: torch.Tensor, ptr: List[int], bb_invariance: str,
                  bg_index: int, nn_index: Optional[torch.Tensor] = None, dedup: bool = True):
    """Ground truth of a batch of frames: ONE decode launch and (dedup) ONE duplicate-removal launch over all frames.
    -> (corners f64 [M, 4, 2], labels [M] in the input dtype, box offsets of the frames int64 [B + 1] on the device)."""
    if bb_invariance not in INVARIANCE_CODES:
        raise ValueError(f"unknown bb_invariance {bb_invariance!r}")
    n = pos.shape[0]
    if boxes.dim() != 2 or boxes.shape[0] != n or boxes.shape[1] not in (4, 5) or pos.shape != (n, 2) or labels.shape != (n,):
        raise ValueError("shapes: class labels [N], boxes [N, 4|5], pos [N, 2]")
    inv = INVARIANCE_CODES[bb_invariance]
    if inv == 2 and nn_index is None:
        nn_index = _nearest_in_frames(pos, ptr)            # (called for aligned boxes too: the reference searches them)
    if inv != 2 or boxes.shape[1] == 4:
        nn_index = None
    keep, corners = ops.decode_ground_truth(labels.to(torch.float32), boxes, pos, nn_index, bg_index, inv)
    ptr_dev = torch.tensor(ptr, dtype=torch.int64, device=pos.device)
    idx = torch.nonzero(keep, as_tuple=False).view(-1)
    corners, labels, box_ptr = corners.index_select(0, idx), labels.index_select(0, idx), _offsets(keep, ptr_dev)
    if dedup:
        keep = ops.remove_duplicate_boxes(corners, box_ptr)
        idx = torch.nonzero(keep, as_tuple=False).view(-1)
        corners, labels, box_ptr = corners.index_select(0, idx), labels.index_select(0, idx), _offsets(keep, box_ptr)
    return corners, labels, box_ptr


class GroundTruthExtractor:
    """postprocessor/postprocessing.py:438-575, same method names and result shapes; tensors in HBM."""

    @staticmethod
    def get_absolute_object_bounding_boxes(class_labels, bounding_boxes, pos, bb_invariance: str, bg_index: int
                                           ) -> Tuple[BoundingBoxes, torch.Tensor]:
        """-> (absolute boxes of the nodes whose label != bg_index, in node order; their labels [M, 1] in the input dtype).
        The angle is never adapted, and there is no score filter."""
        labels = _labels_column(class_labels)
        p, bb = _f32_cuda(pos, "pos"), _f32_cuda(bounding_boxes, "bounding_boxes")
        corners, labels, _ = _ground_truth(labels, bb, p, [0, p.shape[0]], bb_invariance, bg_index, dedup=False)
        return BoundingBoxes(corners, bb.shape[1] == 4), labels.view(-1, 1)

    @staticmethod
    def remove_duplicate_boxes(bounding_boxes, box_labels) -> Tuple[BoundingBoxes, torch.Tensor]:
        """Drops box j when an earlier box of the graph has the same corners or corners within an L1 distance < 0.1
        (postprocessing.py:552-575).  ``bounding_boxes``: ``BoundingBoxes`` or a list of ``BoundingBox``."""
        if isinstance(bounding_boxes, BoundingBoxes):
            corners, aligned = bounding_boxes.corners, bounding_boxes.is_aligned
        else:
            boxes = list(bounding_boxes)
            aligned = boxes[0].is_aligned if boxes else True
            corners = _cuda(np.array([np.asarray(b.corners, dtype=np.float64) for b in boxes]).reshape(-1, 4, 2), "corners",
                            torch.float64)
        corners = _cuda(corners, "corners", torch.float64)
        labels = _cuda(box_labels, "box_labels", None).reshape(-1)
        if labels.shape[0] != corners.shape[0]:
            raise ValueError("one label per box")
        keep = ops.remove_duplicate_boxes(corners, torch.tensor([0, corners.shape[0]], dtype=torch.int64, device=corners.device))
        idx = torch.nonzero(keep, as_tuple=False).view(-1)
        return BoundingBoxes(corners.index_select(0, idx), aligned), labels.index_select(0, idx).view(-1, 1)


def _boxes_f32(boxes, width: int, name: str) -> torch.Tensor:
    t = _f32_cuda(boxes, name)
    if t.numel() == 0:
        t = t.reshape(0, width)
    if t.dim() != 2 or t.shape[1] != width:
        raise ValueError(f"{name} must be [M, {width}]")
    return t


def point_iou_batched(boxes_pred: List, boxes_gt: List, points: List, box_aligned: bool) -> List[torch.Tensor]:
    """``point_iou`` for a list of graphs in ONE set of launches: boxes_pred[f] [P_f, 4|5], boxes_gt[f] [G_f, 4|5] and
    points[f] [N_f, 2] -> list of float64 [P_f, G_f] matrices (views into one packed tensor in HBM)."""
    if not (len(boxes_pred) == len(boxes_gt) == len(points)):
        raise ValueError("one entry per graph in boxes_pred, boxes_gt and points")
    if len(points) == 0:
        return []
    width = 4 if box_aligned else 5
    bp = [_boxes_f32(b, width, "boxes_pred") for b in boxes_pred]
    bg = [_boxes_f32(b, width, "boxes_gt") for b in boxes_gt]
    pts = [_f32_cuda(p, "points").reshape(-1, 2) for p in points]
    ptrs = [[0], [0], [0]]
    for lst, parts in zip(ptrs, (bp, bg, pts)):
        for t in parts:
            lst.append(lst[-1] + t.shape[0])
    iou, out = ops.point_iou(torch.cat(bp), ptrs[0], torch.cat(bg), ptrs[1], torch.cat(pts), ptrs[2], not box_aligned)
    return [iou[out[f]:out[f + 1]].view(bp[f].shape[0], bg[f].shape[0]) for f in range(len(points))]


def point_iou(boxes_pred, boxes_gt, points, box_aligned: bool) -> torch.Tensor:
    """utils/math.py:176-211: float64 [P, G] point IoU of every (predicted, ground-truth) box pair of one graph.  Boxes
    float32 [x_min, y_min, x_max, y_max] (aligned) or [x, y, l, w, theta in degrees] (rotated); points: the graph's
    coordinates [N, 2] (float32)."""
    return point_iou_batched([boxes_pred], [boxes_gt], [points], box_aligned)[0]
