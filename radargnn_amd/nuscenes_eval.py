"""The nuScenes evaluator on the device: the last stage of the nuScenes path (the reference's ``evaluate.py:72-77`` with
``dataset = "nuscenes"``).  Mirrors of ``postprocessor/nuscenes/utils.py`` (``get_submission`` and its helpers) and
``postprocessor/nuscenes/evaluation.py`` (``NuscenesEvaluator``), and this project's own statement of what the nuscenes-devkit's
``DetectionEval`` computes for the configuration ``detection_cvpr_2019`` -- NDS, mAP and the five true-positive errors -- on
librgnn's ``rgnn_nuscenes_submission`` / ``rgnn_detection_filter`` / ``rgnn_center_match`` / ``rgnn_detection_curves``.

    from radargnn_amd.nuscenes_eval import evaluation_selector          # {"radarscenes": ..., "nuscenes": NuscenesEvaluator}
    evaluator = NuscenesEvaluator(config, version, dataset_path, model_path, detection_ground_truth=gt,
                                  ego_translation=ego_t, ego_rotation=ego_r)          # or nusc=<the devkit's NuScenes object>
    evaluator.evaluate(bb_pred, bb_ground_truth, cls_pred, cls_pred_label, cls_ground_truth, vel, graph_names)
    evaluator.save_results()

or stage by stage: ``submission_boxes`` (device) -> ``get_submission`` (the reference's dict) / ``detection_eval`` (the devkit's
``metrics_summary``).  The devkit is not a dependency: nothing here imports ``nuscenes`` or ``pyquaternion``.

NOT PINNED BY AN EXECUTED DEVKIT.  Neither package exists where this is built and tested; every statement below is restated from
their published sources, and tests/nuscenes_eval_oracle.py (plain float64 numpy loops) is what the kernels are held to:
  * rotation matrix of a quaternion: normalise it, then the standard matrix of a unit quaternion (w, x, y, z) (``nuscenes.py``);
  * the ego yaw is pyquaternion's ``yaw_pitch_roll[0]``, restated as ``atan2(2 (w z - x y), 1 - 2 (y^2 + z^2))`` on the normalised
    quaternion -- restated, unpinned;
  * ``Quaternion(axis=[0, 0, 1], angle=a)`` is ``(cos(a / 2), 0, 0, sin(a / 2))``;
  * the devkit's ``quaternion_yaw`` is the atan2 of the first column of the rotation matrix;
  * ``points_in_box`` projects on the three edges that leave corner 0 and includes both ends;
  * predictions are ordered by ``sorted((score, index))[::-1]``: descending score, equal scores by DESCENDING position (not the
    ascending tie rule of this project's mAP);
  * ``np.interp`` takes the last interval whose left end is <= x.

Differences from the reference, all deliberate:
  * the ground truth comes from the caller as arrays (``DetectionGroundTruth``) or from a duck-typed ``nusc`` object; the
    reference constructs ``NuScenes(version, dataroot)`` itself and reads the split from disk;
  * ``metrics_summary`` is SET and ``nuscenes_metrics.json`` is written.  The reference leaves ``metrics_summary`` at ``None``, so
    its ``save_results`` never writes that file (the devkit writes its own ``metrics_summary.json`` instead, which is the same
    content; it is not written here);
  * no plots, no rendered curves, no ``metrics_details.json``, no ``eval_time``;
  * label 0 ('void') or a label outside the reference's list raises ``ValueError`` (the devkit refuses such a record later);
  * ``"nuscenes"`` is a key of THIS module's ``evaluation_selector``, a new dict; ``radargnn_amd.metrics.evaluation_selector`` is
    unchanged.
"""
from __future__ import annotations

import json
import os
from dataclasses import asdict, dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import metrics, ops
from ._lib import RgnnError
from .metrics import Evaluator, ObjectDetectionMetrics, SegmentationMetrics, get_new_evaluation_folder_path
from .postprocessor import PostProcessingConfiguration, _cuda

# postprocessor/nuscenes/utils.py:172-184: the label of a prediction indexes this list
LABEL_NAMES: Tuple[str, ...] = ('void', 'barrier', 'bicycle', 'bus', 'car', 'construction_vehicle', 'motorcycle', 'pedestrian',
                                'traffic_cone', 'trailer', 'truck')
NAME_CODE: Dict[str, int] = {name: code for code, name in enumerate(LABEL_NAMES)}
# the devkit's DETECTION_NAMES: the order of the classes in every table and dict of the summary
DETECTION_NAMES: Tuple[str, ...] = ('car', 'truck', 'bus', 'trailer', 'construction_vehicle', 'pedestrian', 'motorcycle', 'bicycle',
                                    'traffic_cone', 'barrier')
# utils.py:121-133
HEIGHT_MAP: Dict[str, float] = {'void': 1.029, 'barrier': 0.981, 'bicycle': 1.283, 'bus': 3.41, 'car': 1.698,
                                'construction_vehicle': 3.05, 'motorcycle': 1.471, 'pedestrian': 1.78, 'traffic_cone': 1.067,
                                'trailer': 4.04, 'truck': 2.843}
# the devkit's attributes; the code of '' is -1
ATTRIBUTE_NAMES: Tuple[str, ...] = ('cycle.with_rider', 'cycle.without_rider', 'pedestrian.moving', 'pedestrian.standing',
                                    'pedestrian.sitting_lying_down', 'vehicle.moving', 'vehicle.parked', 'vehicle.stopped')
ATTRIBUTE_CODE: Dict[str, int] = {'': -1, **{name: code for code, name in enumerate(ATTRIBUTE_NAMES)}}
# utils.py:213-224: one constant attribute per class
PREDICTED_ATTRIBUTE: Dict[str, str] = {'barrier': '', 'traffic_cone': '', 'bicycle': 'cycle.with_rider', 'motorcycle': 'cycle.with_rider',
                                       'pedestrian': 'pedestrian.moving', 'car': 'vehicle.moving', 'bus': 'vehicle.moving',
                                       'construction_vehicle': 'vehicle.moving', 'trailer': 'vehicle.moving', 'truck': 'vehicle.moving'}
TP_METRICS: Tuple[str, ...] = ('trans_err', 'scale_err', 'orient_err', 'vel_err', 'attr_err')
# the devkit's category_to_detection_name; every other category has no detection class
CATEGORY_TO_DETECTION_NAME: Dict[str, str] = {
    'movable_object.barrier': 'barrier', 'vehicle.bicycle': 'bicycle', 'vehicle.bus.bendy': 'bus', 'vehicle.bus.rigid': 'bus',
    'vehicle.car': 'car', 'vehicle.construction': 'construction_vehicle', 'vehicle.motorcycle': 'motorcycle',
    'human.pedestrian.adult': 'pedestrian', 'human.pedestrian.child': 'pedestrian', 'human.pedestrian.construction_worker': 'pedestrian',
    'human.pedestrian.police_officer': 'pedestrian', 'movable_object.trafficcone': 'traffic_cone', 'vehicle.trailer': 'trailer',
    'vehicle.truck': 'truck'}
BIKE_RACK_CATEGORY = 'vehicle.bicycle_rack'
SUBMISSION_META = {"use_camera": False, "use_lidar": False, "use_radar": True, "use_map": False, "use_external": False}   # utils.py:330-338


@dataclass()
class DetectionConfig:
    """The devkit's ``detection_cvpr_2019`` configuration, as constants."""
    class_range: Dict[str, float] = field(default_factory=lambda: {
        'car': 50, 'truck': 50, 'bus': 50, 'trailer': 50, 'construction_vehicle': 50, 'pedestrian': 40, 'motorcycle': 40, 'bicycle': 40,
        'traffic_cone': 30, 'barrier': 30})
    dist_fcn: str = 'center_distance'
    dist_ths: Tuple[float, ...] = (0.5, 1.0, 2.0, 4.0)
    dist_th_tp: float = 2.0
    min_recall: float = 0.1
    min_precision: float = 0.1
    max_boxes_per_sample: int = 500
    mean_ap_weight: int = 5

    def __post_init__(self):
        if set(self.class_range) != set(DETECTION_NAMES):
            raise ValueError("class_range needs exactly the ten detection classes")
        if self.dist_th_tp not in self.dist_ths:
            raise ValueError("dist_th_tp must be one of dist_ths")
        if self.dist_fcn != 'center_distance':
            raise ValueError("only center_distance is implemented")

    def serialize(self) -> dict:
        out = asdict(self)
        out["dist_ths"] = list(self.dist_ths)
        return out


def _host(x, dtype) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=dtype)


_NP = {torch.float64: np.float64, torch.int64: np.int64, torch.int32: np.int32}


def _up(x, name: str, dtype, tail: Tuple[int, ...] = ()) -> torch.Tensor:
    """numpy / sequence / tensor -> contiguous device tensor of ``dtype`` with trailing shape ``tail``."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(_host(x, _NP[dtype]))
    return _cuda(t, name, dtype).reshape(-1, *tail)


class DetectionGroundTruth:
    """The annotations of S samples as plain arrays, global frame, packed by ``gt_ptr`` [S + 1] -- the layout of
    ``NuScenesSamples``.  ``translation`` [G, 3], ``size`` [G, 3] (w, l, h), ``rotation`` [G, 4] (w, x, y, z), ``velocity`` [G, 2]
    (may be NaN), ``name`` int32 (a code of ``NAME_CODE``; anything below 1 has no detection class and is dropped), ``attribute``
    int32 (a code of ``ATTRIBUTE_CODE``, -1 for ''), ``num_pts`` int32 (lidar + radar), ``ego_translation`` [S, 3] of the LIDAR_TOP
    sample data.  Optional bike racks per sample: ``rack_center`` [R, 3], ``rack_size`` [R, 3], ``rack_rotation`` [R, 4],
    ``rack_ptr`` [S + 1].  ``ego_rotation`` [S, 4] is carried for the submission when ``ground_truth_from_devkit`` fills it.
    numpy arrays, sequences and tensors are taken and kept as given; they are uploaded once, on first use."""

    def __init__(self, translation, size, rotation, velocity, name, attribute, num_pts, gt_ptr, ego_translation, rack_center=None,
                 rack_size=None, rack_rotation=None, rack_ptr=None, ego_rotation=None, sample_tokens: Optional[Sequence[str]] = None):
        self.translation, self.size, self.rotation, self.velocity = translation, size, rotation, velocity
        self.name, self.attribute, self.num_pts, self.gt_ptr, self.ego_translation = name, attribute, num_pts, gt_ptr, ego_translation
        self.rack_center, self.rack_size, self.rack_rotation, self.rack_ptr = rack_center, rack_size, rack_rotation, rack_ptr
        self.ego_rotation = ego_rotation
        self.sample_tokens = None if sample_tokens is None else list(sample_tokens)
        self._dev: Optional[dict] = None

    def on_device(self) -> dict:
        if self._dev is None:
            f64, i32, i64 = torch.float64, torch.int32, torch.int64
            d = {"translation": _up(self.translation, "translation", f64, (3,)), "size": _up(self.size, "size", f64, (3,)),
                 "rotation": _up(self.rotation, "rotation", f64, (4,)), "velocity": _up(self.velocity, "velocity", f64, (2,)),
                 "name": _up(self.name, "name", i32), "attribute": _up(self.attribute, "attribute", i32),
                 "num_pts": _up(self.num_pts, "num_pts", i32), "ptr": _up(self.gt_ptr, "gt_ptr", i64),
                 "ego_translation": _up(self.ego_translation, "ego_translation", f64, (3,)), "racks": None}
            g, s = d["translation"].shape[0], d["ptr"].numel() - 1
            if any(d[k].shape[0] != g for k in ("size", "rotation", "velocity", "name", "attribute", "num_pts")):
                raise ValueError("DetectionGroundTruth: one row per box in every array")
            if s < 0 or d["ego_translation"].shape[0] != s:
                raise ValueError("DetectionGroundTruth: gt_ptr [S + 1], ego_translation [S, 3]")
            if self.rack_ptr is not None:
                d["racks"] = (_up(self.rack_center, "rack_center", f64, (3,)), _up(self.rack_size, "rack_size", f64, (3,)),
                              _up(self.rack_rotation, "rack_rotation", f64, (4,)), _up(self.rack_ptr, "rack_ptr", i64))
                if d["racks"][3].numel() != s + 1:
                    raise ValueError("DetectionGroundTruth: rack_ptr [S + 1]")
            self._dev = d
        return self._dev


def ground_truth_from_devkit(nusc, sample_tokens: Sequence[str]) -> DetectionGroundTruth:
    """What the devkit's ``load_gt`` and ``add_center_dist`` read, from a duck-typed ``nusc``: ``nusc.get(table, token)`` for the
    tables ``sample`` (``anns``, ``data['LIDAR_TOP']``), ``sample_annotation`` (``translation``, ``size``, ``rotation``,
    ``category_name``, ``attribute_tokens``, ``num_lidar_pts``, ``num_radar_pts``), ``attribute`` (``name``), ``sample_data``
    (``ego_pose_token``) and ``ego_pose`` (``translation``, ``rotation``), and ``nusc.box_velocity(annotation_token)``.  Imports
    nothing from the devkit.  Annotations without a detection class are left out; bicycle racks go to the rack arrays."""
    cols = {k: [] for k in ("translation", "size", "rotation", "velocity", "name", "attribute", "num_pts")}
    racks = {k: [] for k in ("center", "size", "rotation")}
    gt_ptr, rack_ptr, ego_t, ego_r = [0], [0], [], []
    for token in sample_tokens:
        sample = nusc.get('sample', token)
        pose = nusc.get('ego_pose', nusc.get('sample_data', sample['data']['LIDAR_TOP'])['ego_pose_token'])
        ego_t.append(list(pose['translation']))
        ego_r.append(list(pose['rotation']))
        for ann_token in sample['anns']:
            ann = nusc.get('sample_annotation', ann_token)
            if ann['category_name'] == BIKE_RACK_CATEGORY:
                racks["center"].append(list(ann['translation']))
                racks["size"].append(list(ann['size']))
                racks["rotation"].append(list(ann['rotation']))
            name = CATEGORY_TO_DETECTION_NAME.get(ann['category_name'])
            if name is None:
                continue
            attrs = ann['attribute_tokens']
            if len(attrs) > 1:
                raise Exception('Error: GT annotations must not have more than one attribute!')
            cols["translation"].append(list(ann['translation']))
            cols["size"].append(list(ann['size']))
            cols["rotation"].append(list(ann['rotation']))
            cols["velocity"].append(list(np.asarray(nusc.box_velocity(ann_token), dtype=np.float64)[:2]))
            cols["name"].append(NAME_CODE[name])
            cols["attribute"].append(ATTRIBUTE_CODE[nusc.get('attribute', attrs[0])['name']] if attrs else -1)
            cols["num_pts"].append(int(ann['num_lidar_pts']) + int(ann['num_radar_pts']))
        gt_ptr.append(len(cols["name"]))
        rack_ptr.append(len(racks["center"]))
    f = np.float64
    return DetectionGroundTruth(
        np.asarray(cols["translation"], dtype=f).reshape(-1, 3), np.asarray(cols["size"], dtype=f).reshape(-1, 3),
        np.asarray(cols["rotation"], dtype=f).reshape(-1, 4), np.asarray(cols["velocity"], dtype=f).reshape(-1, 2),
        np.asarray(cols["name"], dtype=np.int32), np.asarray(cols["attribute"], dtype=np.int32), np.asarray(cols["num_pts"], dtype=np.int32),
        np.asarray(gt_ptr, dtype=np.int64), np.asarray(ego_t, dtype=f).reshape(-1, 3),
        rack_center=np.asarray(racks["center"], dtype=f).reshape(-1, 3), rack_size=np.asarray(racks["size"], dtype=f).reshape(-1, 3),
        rack_rotation=np.asarray(racks["rotation"], dtype=f).reshape(-1, 4), rack_ptr=np.asarray(rack_ptr, dtype=np.int64),
        ego_rotation=np.asarray(ego_r, dtype=f).reshape(-1, 4), sample_tokens=sample_tokens)


@dataclass()
class DetectionBoxes:
    """The predictions of S samples on the device, global frame, packed by ``ptr`` [S + 1]: what the submission holds."""
    translation: torch.Tensor
    size: torch.Tensor
    rotation: torch.Tensor
    velocity: torch.Tensor
    name: torch.Tensor
    attribute: torch.Tensor
    score: torch.Tensor
    ptr: torch.Tensor
    yaw: Optional[torch.Tensor] = None
    packed: Optional[torch.Tensor] = None          # translation | size | rotation | yaw | label | score | status, flat float64
    host_ptr: Optional[List[int]] = None           # ptr as a list, where the builder had it on the host


def get_sample_token(graph_name: str) -> str:
    """utils.py:229-243: ``/.../..._<sample token>.pt`` -> the sample token."""
    file_name, _ = os.path.splitext(os.path.split(graph_name)[-1])
    return file_name.split('_')[-1]


def get_bounding_box_detection_name(label: int) -> str:
    """utils.py:162-185."""
    return LABEL_NAMES[int(label)]


def get_bounding_box_attribute_name(detection_name: str, velocity=None) -> str:
    """utils.py:188-226: one constant attribute per class; the velocity is not read."""
    return PREDICTED_ATTRIBUTE[detection_name]


def _table(values: Sequence, dtype, device) -> torch.Tensor:
    return torch.tensor(list(values), dtype=dtype).to(device)


def submission_boxes(bb_pred: List[Dict], ego_translation, ego_rotation) -> DetectionBoxes:
    """The predictions of a list of frames as submission arrays in HBM (``convert_results``, utils.py:246-309): the frames' boxes
    -> ``rgnn_box_representations`` -> ``rgnn_nuscenes_submission``.  ``bb_pred``: one detection dict per frame (``boxes``,
    ``labels``, ``scores``), as ``Postprocessor`` returns them; the ego pose of each frame's LIDAR_TOP sample data."""
    corners = [metrics._frame_corners(d["boxes"]) for d in bb_pred]
    ptr = [0]
    for c in corners:
        ptr.append(ptr[-1] + int(c.shape[0]))
    _, rotated = ops.box_representations(metrics._concat_cuda(corners, torch.float64, (4, 2)), two_point=False, rotated=True)
    dev = rotated.device
    labels = metrics._concat_cuda([d["labels"] for d in bb_pred], torch.float64).reshape(-1)
    scores = metrics._concat_cuda([d["scores"] for d in bb_pred], torch.float64).reshape(-1)
    m = rotated.shape[0]
    if labels.numel() != m or scores.numel() != m:
        raise ValueError("one score and label per predicted box")
    ego_t, ego_r = _up(ego_translation, "ego_translation", torch.float64, (3,)), _up(ego_rotation, "ego_rotation", torch.float64, (4,))
    if ego_t.shape[0] != len(bb_pred) or ego_r.shape[0] != len(bb_pred):
        raise ValueError("one ego pose per frame")
    name = labels.to(torch.int32)                                                       # int(label), utils.py:185
    ptr_dev = _table(ptr, torch.int64, dev)
    packed = torch.empty(13 * m + 1, dtype=torch.float64, device=dev)
    heights = _table([HEIGHT_MAP[n] for n in LABEL_NAMES], torch.float64, dev)
    translation, size, rotation, yaw, status = ops.nuscenes_submission(
        rotated, name, ptr_dev, ego_t, ego_r, heights, out=packed)
    packed[11 * m:12 * m] = name
    packed[12 * m:13 * m] = scores
    packed[13 * m:] = status
    attr_of_label = _table([-1] + [ATTRIBUTE_CODE[PREDICTED_ATTRIBUTE[n]] for n in LABEL_NAMES[1:]], torch.int32, dev)
    attribute = attr_of_label.index_select(0, name.clamp(0, len(LABEL_NAMES) - 1).to(torch.int64))
    velocity = torch.zeros((m, 2), dtype=torch.float64, device=dev)                    # get_bounding_box_velocity: always (0, 0)
    return DetectionBoxes(translation, size, rotation, velocity, name, attribute, scores, ptr_dev, yaw, packed, ptr)


def submission_records(packed: np.ndarray, ptr: Sequence[int], sample_tokens: Sequence[str]) -> Dict[str, List[dict]]:
    """The ``results`` block of the submission from the packed host copy of ``submission_boxes`` (flat float64: translation [M, 3]
    | size [M, 3] | rotation [M, 4] | yaw [M] | label [M] | score [M] | status): per sample token the list of records with the
    reference's eight keys (utils.py:298-307).  Raises ``ValueError`` if the status word flags a label without a name."""
    packed = np.asarray(packed, dtype=np.float64).reshape(-1)
    m = (packed.size - 1) // 13
    if packed.size != 13 * m + 1 or int(ptr[-1]) != m or len(ptr) != len(sample_tokens) + 1:
        raise ValueError("packed holds 13 values per box and the status word; ptr [S + 1] ends at the number of boxes")
    if int(packed[-1]) & ops.STATUS_NUSC_EVAL_BAD_LABEL:
        raise ValueError("a predicted label is 0 ('void') or outside the nuScenes detection names: no submission record exists for it")
    translation, size, rotation = packed[:3 * m].reshape(m, 3), packed[3 * m:6 * m].reshape(m, 3), packed[6 * m:10 * m].reshape(m, 4)
    label, score = packed[11 * m:12 * m], packed[12 * m:13 * m]
    results: Dict[str, List[dict]] = {}
    for s, token in enumerate(sample_tokens):
        records = []
        for i in range(int(ptr[s]), int(ptr[s + 1])):
            name = LABEL_NAMES[int(label[i])]
            records.append({"sample_token": token, "translation": tuple(translation[i].tolist()), "size": tuple(size[i].tolist()),
                            "rotation": tuple(rotation[i].tolist()), "velocity": (0.0, 0.0), "detection_name": name,
                            "detection_score": float(score[i]), "attribute_name": PREDICTED_ATTRIBUTE[name]})
        results[token] = records
    return results


def _submission_of(boxes: DetectionBoxes, graph_names: Sequence[str]) -> dict:
    tokens = [get_sample_token(g) for g in graph_names]
    host = boxes.packed.cpu().numpy()                                                   # the one copy
    ptr = boxes.host_ptr if boxes.host_ptr is not None else boxes.ptr.cpu().tolist()
    return {"meta": dict(SUBMISSION_META), "results": submission_records(host, ptr, tokens)}


def get_submission(bb_pred: List[Dict], vel, graph_names: Sequence[str], ego_translation, ego_rotation) -> dict:
    """utils.py:312-343 without the ``nusc`` argument (the ego poses come from the caller): ``{"meta": ..., "results": {token:
    [record, ...]}}``.  ``vel`` is taken and ignored, as the reference ignores it (the velocity of every record is (0, 0))."""
    if not (len(bb_pred) == len(graph_names) == len(vel)):
        raise AssertionError("predictions, velocities and graph names need one entry per graph")       # utils.py:260
    return _submission_of(submission_boxes(bb_pred, ego_translation, ego_rotation), graph_names)


# ---- the devkit's DetectionEval ------------------------------------------------------------------------------------------------
def class_score_order(score: torch.Tensor, name: torch.Tensor, keep: torch.Tensor, classes: torch.Tensor):
    """-> (order int64: the KEPT predictions class by class in the order of ``classes``, inside a class by descending score over
    all samples with equal scores by descending position; cls_ptr int64 [2, C]: where each class begins and ends in it).  Two
    passes of rgnn_sort_scores: by score on the reversed array, then a stable pass by class."""
    dev, m, c = score.device, score.numel(), classes.numel()
    class_of_name = torch.full((len(LABEL_NAMES),), c, dtype=torch.int64, device=dev)
    class_of_name[classes.to(torch.int64)] = torch.arange(c, device=dev)
    order = by = torch.empty(0, dtype=torch.int64, device=dev)
    if m:
        order = (m - 1) - ops.sort_scores(score.flip(0))
        order = order[keep.index_select(0, order).bool()]
        by = class_of_name.index_select(0, name.index_select(0, order).clamp(0, len(LABEL_NAMES) - 1).to(torch.int64))
        if order.numel():
            second = ops.sort_scores(-by.to(torch.float64))
            order, by = order.index_select(0, second), by.index_select(0, second)
    ids = torch.arange(c, device=dev)
    cls_ptr = torch.stack((torch.searchsorted(by, ids), torch.searchsorted(by, ids, right=True))).to(torch.int64).contiguous()
    return order.contiguous(), cls_ptr


def detection_tables(pred: DetectionBoxes, gt: DetectionGroundTruth, config: Optional[DetectionConfig] = None):
    """Filter, match and accumulate on the device -> (precision [C, T, 101], confidence [C, T, 101], tp_err_curve [C, 5, 101],
    float64 tensors in HBM, classes in the order of ``DETECTION_NAMES``) plus the intermediate results in a dict.  One host read:
    the status words."""
    cfg = config or DetectionConfig()
    g = gt.on_device()
    dev = pred.translation.device
    m = pred.score.numel()
    if pred.ptr.numel() != g["ptr"].numel():
        raise ValueError("predictions and ground truth need the same samples")
    class_range = _table([0.0] + [float(cfg.class_range[n]) for n in LABEL_NAMES[1:]], torch.float64, dev)
    bicycle, motorcycle, barrier = NAME_CODE['bicycle'], NAME_CODE['motorcycle'], NAME_CODE['barrier']
    score = pred.score.to(torch.float64)
    keep_p, status_p = ops.detection_filter(pred.translation, pred.name, pred.ptr, g["ego_translation"], class_range, bicycle, motorcycle,
                                            score=score, max_boxes=cfg.max_boxes_per_sample, racks=g["racks"])
    keep_g, _ = ops.detection_filter(g["translation"], g["name"], g["ptr"], g["ego_translation"], class_range, bicycle, motorcycle,
                                     num_pts=g["num_pts"], racks=g["racks"])
    classes = _table([NAME_CODE[n] for n in DETECTION_NAMES], torch.int32, dev)
    tp_index = list(cfg.dist_ths).index(cfg.dist_th_tp)
    pd = {"translation": pred.translation, "size": pred.size, "rotation": pred.rotation, "velocity": pred.velocity, "name": pred.name,
          "attribute": pred.attribute, "keep": keep_p, "ptr": pred.ptr}
    gd = {**{k: g[k] for k in ("translation", "size", "rotation", "velocity", "name", "attribute", "ptr")}, "keep": keep_g}
    order_sample = ops.sample_score_order(score, pred.ptr) if m else torch.empty(0, dtype=torch.int64, device=dev)
    match, tp_err, status_m = ops.center_match(pd, gd, order_sample, classes, cfg.dist_ths, tp_index, barrier)
    order, cls_ptr = class_score_order(score, pred.name, keep_p, classes)
    grid = torch.from_numpy(np.linspace(0, 1, 101)).to(dev)
    words = torch.cat((status_p, status_m)).cpu().tolist()                              # the one host read
    status = words[0] | words[1]
    if status & ops.STATUS_NUSC_EVAL_TOO_MANY_BOXES:
        raise ValueError(f"Error: Only <= {cfg.max_boxes_per_sample} boxes per sample allowed!")
    if status & ops.STATUS_NUSC_EVAL_NAN_SCORE:
        raise ValueError("Error: Score is NaN.")
    if status & ops.STATUS_NUSC_EVAL_BAD_LABEL:
        raise ValueError("a predicted name is no nuScenes detection class")
    if status & ops.STATUS_NUSC_EVAL_GT_OVERFLOW:
        raise RgnnError(f"rgnn_center_match: at most {ops.center_match_capacity()} ground-truth boxes of one class per sample")
    if status & ops.STATUS_NUSC_EVAL_BAD_PTR:
        raise ValueError("the box offsets of a sample do not lie inside the box lists")
    precision, confidence, tp_curve = ops.detection_curves(order, cls_ptr, score, match, tp_err, g["name"], keep_g, classes, tp_index, grid)
    parts = {"keep_pred": keep_p, "keep_gt": keep_g, "order_sample": order_sample, "order": order, "cls_ptr": cls_ptr, "match": match,
             "tp_err": tp_err}
    return precision, confidence, tp_curve, parts


def summarize(precision: np.ndarray, confidence: np.ndarray, tp_curve: np.ndarray, config: DetectionConfig) -> dict:
    """The devkit's ``calc_ap`` / ``calc_tp`` / ``DetectionMetrics.serialize`` on the [C, T, 101] tables (float64, host): the keys
    ``label_aps``, ``mean_dist_aps``, ``mean_ap``, ``label_tp_errors``, ``tp_errors``, ``tp_scores``, ``nd_score``, ``cfg``."""
    cfg = config
    first = int(round(100 * cfg.min_recall)) + 1
    tp_index = list(cfg.dist_ths).index(cfg.dist_th_tp)
    label_aps: Dict[str, Dict[float, float]] = {}
    label_tp: Dict[str, Dict[str, float]] = {}
    for ic, name in enumerate(DETECTION_NAMES):
        label_aps[name] = {}
        for it, th in enumerate(cfg.dist_ths):
            prec = np.copy(precision[ic, it, first:]) - cfg.min_precision
            prec[prec < 0] = 0
            label_aps[name][th] = float(np.mean(prec)) / (1.0 - cfg.min_precision)
        non_zero = np.nonzero(confidence[ic, tp_index])[0]
        last = 0 if len(non_zero) == 0 else int(non_zero[-1])
        label_tp[name] = {}
        for ie, metric in enumerate(TP_METRICS):
            if name == 'traffic_cone' and metric in ('attr_err', 'vel_err', 'orient_err'):
                value = float('nan')
            elif name == 'barrier' and metric in ('attr_err', 'vel_err'):
                value = float('nan')
            elif last < first:
                value = 1.0
            else:
                value = float(np.mean(tp_curve[ic, ie, first:last + 1]))
            label_tp[name][metric] = value
    mean_dist_aps = {name: float(np.mean(list(aps.values()))) for name, aps in label_aps.items()}
    mean_ap = float(np.mean(list(mean_dist_aps.values())))
    tp_errors = {metric: float(np.nanmean([label_tp[name][metric] for name in DETECTION_NAMES])) for metric in TP_METRICS}
    tp_scores = {metric: max(0.0, 1.0 - tp_errors[metric]) for metric in TP_METRICS}
    total = float(cfg.mean_ap_weight * mean_ap + np.sum(list(tp_scores.values())))
    return {"label_aps": label_aps, "mean_dist_aps": mean_dist_aps, "mean_ap": mean_ap, "label_tp_errors": label_tp,
            "tp_errors": tp_errors, "tp_scores": tp_scores, "nd_score": total / float(cfg.mean_ap_weight + len(tp_scores)),
            "cfg": cfg.serialize()}


def detection_eval(pred: DetectionBoxes, gt: DetectionGroundTruth, config: Optional[DetectionConfig] = None) -> dict:
    """The devkit's ``DetectionEval.evaluate`` + ``DetectionMetrics.serialize`` for predictions and ground truth in arrays: the
    ``metrics_summary`` dict (without ``eval_time``).  The tables are built on the device and copied to the host once."""
    cfg = config or DetectionConfig()
    precision, confidence, tp_curve, _ = detection_tables(pred, gt, cfg)
    c, t, r = precision.shape
    host = torch.cat((precision.reshape(-1), confidence.reshape(-1), tp_curve.reshape(-1))).cpu().numpy()
    return summarize(host[:c * t * r].reshape(c, t, r), host[c * t * r:2 * c * t * r].reshape(c, t, r),
                     host[2 * c * t * r:].reshape(c, 5, r), cfg)


class NuscenesEvaluator(Evaluator):
    """postprocessor/nuscenes/evaluation.py:19-141 on the device.  The reference's constructor arguments, plus the ground truth as
    keyword arguments: ``detection_ground_truth`` (a ``DetectionGroundTruth`` whose samples are in the order of the evaluated
    graphs) with ``ego_translation`` [S, 3] / ``ego_rotation`` [S, 4] of the LIDAR_TOP ego poses, or ``nusc``, a duck-typed devkit
    object handed to ``ground_truth_from_devkit`` with the sample tokens of the graph names.  Like the reference, the constructor
    creates the evaluation folder.  ``evaluate`` writes ``submission.json`` and keeps the devkit's summary in ``metrics_summary``
    (the reference leaves it ``None``); ``save_results`` therefore writes ``nuscenes_metrics.json`` too.  No plots."""

    def __init__(self, config: PostProcessingConfiguration, version: str, dataset_path: str, model_path: str, *args,
                 detection_ground_truth: Optional[DetectionGroundTruth] = None, ego_translation=None, ego_rotation=None, nusc=None,
                 detection_config: Optional[DetectionConfig] = None, **kwargs):
        self.version = version
        self.path_to_nuscenes = dataset_path
        self.path_to_model_folder = model_path
        self.evaluation_folder_path = get_new_evaluation_folder_path(self.path_to_model_folder)
        self.mAP = self.mAP_per_class = self.metrics_summary = self.f1_segmentation = None
        self.f1_class_averaging = None if config.f1_class_averaging == 'None' else config.f1_class_averaging
        self.confusion_absolute = self.confusion_relative = None
        self.detection_ground_truth, self.ego_translation, self.ego_rotation, self.nusc = detection_ground_truth, ego_translation, ego_rotation, nusc
        self.detection_config = detection_config or DetectionConfig()
        super().__init__(config, *args, **kwargs)
        os.mkdir(self.evaluation_folder_path)

    def _ground_truth(self, graph_names: Sequence[str]):
        gt = self.detection_ground_truth
        if gt is None:
            if self.nusc is None:
                raise ValueError("NuscenesEvaluator needs detection_ground_truth= (with ego_translation= and ego_rotation=) or nusc=")
            gt = ground_truth_from_devkit(self.nusc, [get_sample_token(g) for g in graph_names])
        ego_t = self.ego_translation if self.ego_translation is not None else gt.ego_translation
        ego_r = self.ego_rotation if self.ego_rotation is not None else gt.ego_rotation
        if ego_r is None:
            raise ValueError("NuscenesEvaluator needs ego_rotation= with detection_ground_truth=")
        return gt, ego_t, ego_r

    def evaluate(self, bb_pred, bb_ground_truth, cls_pred, cls_pred_label, cls_ground_truth, vel, graph_names: List[str], *args,
                 **kwargs) -> None:
        if self.version not in ("v1.0-trainval", "v1.0-mini"):
            raise ValueError("Version must be either trainval or mini!")
        if not (len(bb_pred) == len(graph_names) == len(vel)):
            raise AssertionError("predictions, velocities and graph names need one entry per graph")
        gt, ego_t, ego_r = self._ground_truth(graph_names)
        boxes = submission_boxes(bb_pred, ego_t, ego_r)
        submission = _submission_of(boxes, graph_names)
        with open(os.path.join(self.evaluation_folder_path, "submission.json"), 'w') as f:
            json.dump(submission, f, indent=4)
        self.metrics_summary = detection_eval(boxes, gt, self.detection_config)
        cfg, n_classes = self.config, len(self.names)
        if cfg.get_mAP:
            detection = ObjectDetectionMetrics.get_map(cfg, bb_pred, bb_ground_truth, cls_pred)
            self.mAP = detection["map"].item()
            self.mAP_per_class = detection["map_per_class"].detach().numpy()
        segmentation = SegmentationMetrics(cls_pred_label, cls_ground_truth)
        if cfg.get_segmentation_f1:
            self.f1_segmentation = segmentation.get_f1(n_classes, self.f1_class_averaging)
        if cfg.get_confusion:
            counts = segmentation.get_confusion_matrix(n_classes)
            per_true_label = counts.sum(axis=1, keepdims=True).astype(np.float64)
            self.confusion_absolute = counts
            self.confusion_relative = counts / np.where(per_true_label == 0, 1e-8, per_true_label)

    def save_results(self, *args, **kwargs):
        folder, cfg = self.evaluation_folder_path, self.config
        metrics._write_json(os.path.join(folder, "eval_configs.json"), {"EVALUATION_CONFIG": asdict(cfg)})
        if self.metrics_summary:
            metrics._write_json(os.path.join(folder, "nuscenes_metrics.json"), self.metrics_summary)
        detection = {"mAP": self.mAP, "mAP_per_class": self.mAP_per_class.tolist()} if cfg.get_mAP else {}
        f1 = self.f1_segmentation
        segmentation = {"f1": f1.tolist() if isinstance(f1, np.ndarray) else f1} if cfg.get_segmentation_f1 else {}
        metrics._write_json(os.path.join(folder, "eval_results.json"),
                            {"OBJECT_DETECTION_METRICS": detection, "SEMANTIC_SEGMENTATION_METRICS": segmentation})
        if cfg.get_confusion:
            for name, matrix in (("confusion_abs.npy", self.confusion_absolute), ("convusion_rel.npy", self.confusion_relative)):
                np.save(os.path.join(folder, name), matrix)


evaluation_selector: Dict[str, type] = {**metrics.evaluation_selector, "nuscenes": NuscenesEvaluator}
