"""nuScenes samples into labelled graphs, in HBM: the reference's ``process_single_sample`` from the arrays the devkit hands it on
(preprocessor/nuscenes/dataset_creation.py:121-165,189-201,241-354, conversion.py:15-67,112-187, utils.py:6-48) -- the sensor ->
vehicle transform, the two crops, ``get_labels``, ``convert_bounding_boxes`` and ``create_graph_data`` for a batch of samples.

    samples = NuScenesSamples(points, chunk_ptr, chunk_sample, chunk_rotation, chunk_translation, box_center, box_size, box_rotation,
                              box_label, box_points, box_ptr, ego_translation, ego_rotation)
    graphs = create_graph_data_from_samples(samples, graph_config, dataset_config)          # list[Data], one per sample

or stage by stage:

    batch, v_cc, src_row = sample_point_clouds(samples, dataset_config)                     # FrameBatch: vehicle frame, cropped
    boxes = prepare_boxes(samples, dataset_config)                                          # filtered, vehicle frame, cropped
    labels, targets, hit = label_points(batch.X, batch.frame_ptr, boxes, dataset_config.bb_invariance, dataset_config.wlh_offset)

Three device stages (csrc/nuscenes.hip): a masked, order-preserving compaction of the radar rows per sample (count, scan, write),
one launch that prepares the boxes, one launch that gives every point its label AND its box target -- the reference computes the
same point-in-box mask twice, once for each.  One host read in the point stage (``frame_ptr`` with the status word); the points
never return to the host.  There is no CPU path.

The nuScenes evaluator (submission records, NDS, mAP) is ``radargnn_amd.nuscenes_eval``.  Out of scope, on purpose: reading the
dataset (``NuScenes(...)``, ``from_file_multisweep``, the split lists) and the class-name -> id table (``_get_box_label`` is a
list of names; ``box_label`` comes from the caller as integers, as ``preprocessor.py`` takes ``label_map`` without a default).

Layout.  ``points`` is float64 [19, N_total], channel-major: the devkit's 18 radar channels with the timestamp row beneath, exactly
what ``get_sensor_points`` stacks (dataset_creation.py:183), in the SENSOR frame.  It is laid out in chunks, one per (sample,
sensor), back to back: ``chunk_ptr`` int64 [C + 1], ``chunk_sample`` int32 [C] non-decreasing, ``chunk_rotation`` float64 [C, 4]
(the calibrated sensor's quaternion w, x, y, z), ``chunk_translation`` float64 [C, 3].  A sample's chunks are concatenated in the
order given: THE CALLER FIXES THE SENSOR ORDER.  The reference iterates a Python ``set`` of sensor names (dataset_creation.py:325),
so its row order depends on string hashing and differs between interpreter runs.
Boxes are in the GLOBAL frame: ``box_center`` [M, 3], ``box_size`` [M, 3] (w, l, h), ``box_rotation`` [M, 4], ``box_label`` int32
[M], ``box_points`` int32 [M] (num_lidar_pts + num_radar_pts), ``box_ptr`` int64 [B + 1]; ``ego_translation`` [B, 3] and
``ego_rotation`` [B, 4] are those of the sample's LIDAR_TOP sample data (dataset_creation.py:242-243,337).

Three things the reference does that a reader may not expect, all kept:
  * the sensor order is whatever the caller gives (see above);
  * a point inside several boxes takes the LAST one in list order -- its label (``sensor_labels[mask] = box.label`` overwrites)
    and its box target (``bounding_boxes[idx] = bb_array`` overwrites);
  * ``use_z=False`` drops the z TEST, not the z TERM: the ego pose's pitch and roll give the box edges i and j a z part, and a
    point's v_z is 0 - p1_z, so the dot products have three terms.

Conventions restated from the devkit.  NOT PINNED BY AN EXECUTED DEVKIT: neither ``nuscenes`` nor ``pyquaternion`` is available
where the fixtures are generated; the fixture generator's stand-ins follow the same four statements.
  * Rotation matrix of a quaternion: normalise it, then the standard matrix of a unit quaternion (w, x, y, z).
  * A box moved to the vehicle frame: centre_v = R_e^T (centre_g - t_e), R_v = R_e^T R_box.
  * ``corners(f)`` in the box frame: x = f l / 2 [1, 1, 1, 1, -1, -1, -1, -1], y = f w / 2 [1, -1, -1, 1, 1, -1, -1, 1],
    z = f h / 2 [1, 1, -1, -1, 1, 1, -1, -1]; then R_v times that, plus the centre.
  * ``bottom_corners()``: columns [2, 3, 7, 6] of ``corners(1)``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from .frames import FrameBatch, build_graphs
from .postprocessor import INVARIANCE_CODES, _nearest_in_frames

# columns of a prepared box record (rgnn.h)
REC_RECT, REC_LABEL, REC_SRC = slice(11, 16), 16, 17


@dataclass()
class NuScenesDatasetConfiguration:
    """Field-compatible with preprocessor/nuscenes/configs.py:6-20.  ``bounding_boxes_aligned`` is carried and ignored, as the
    reference ignores it: nuScenes targets always have five columns."""
    version: str = 'v1.0-trainval'
    nsweeps: int = 1
    crop_point_cloud: bool = False
    crop_settings: dict = None
    wlh_factor: float = 1.0
    wlh_offset: float = 0.0
    bounding_boxes_aligned: bool = False
    bb_invariance: str = "translation"
    deterministic: bool = False
    seed: int = 0


def _crop(dataset_config):
    if not dataset_config.crop_point_cloud:
        return False, 0.0, 0.0
    return True, float(dataset_config.crop_settings['x']), float(dataset_config.crop_settings['y'])


def _up(x, name: str, dtype, device) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        t = x if x.dtype == dtype else x.to(dtype)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype={torch.float64: np.float64, torch.int64: np.int64,
                                                                         torch.int32: np.int32}[dtype]))
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError(f"{name}: the nuScenes kernels need a GPU (no CPU fallback)")
        t = t.to(device)
    return t.contiguous()


class NuScenesSamples:
    """Everything the devkit hands the reference for B samples, as plain arrays resident in HBM (the layout is in the module
    docstring; numpy arrays, sequences or tensors are taken).  Holds nothing of the devkit's types."""

    def __init__(self, points, chunk_ptr, chunk_sample, chunk_rotation, chunk_translation, box_center, box_size, box_rotation,
                 box_label, box_points, box_ptr, ego_translation, ego_rotation, device="cuda"):
        f64, i64, i32 = torch.float64, torch.int64, torch.int32
        self.points = _up(points, "points", f64, device)
        self.chunk_ptr = _up(chunk_ptr, "chunk_ptr", i64, device)
        self.chunk_sample = _up(chunk_sample, "chunk_sample", i32, device)
        self.chunk_rotation = _up(chunk_rotation, "chunk_rotation", f64, device).reshape(-1, 4)
        self.chunk_translation = _up(chunk_translation, "chunk_translation", f64, device).reshape(-1, 3)
        self.box_center = _up(box_center, "box_center", f64, device).reshape(-1, 3)
        self.box_size = _up(box_size, "box_size", f64, device).reshape(-1, 3)
        self.box_rotation = _up(box_rotation, "box_rotation", f64, device).reshape(-1, 4)
        self.box_label = _up(box_label, "box_label", i32, device).reshape(-1)
        self.box_points = _up(box_points, "box_points", i32, device).reshape(-1)
        self.box_ptr = _up(box_ptr, "box_ptr", i64, device).reshape(-1)
        self.ego_translation = _up(ego_translation, "ego_translation", f64, device).reshape(-1, 3)
        self.ego_rotation = _up(ego_rotation, "ego_rotation", f64, device).reshape(-1, 4)
        c, m, b = self.chunk_sample.numel(), self.box_label.numel(), self.box_ptr.numel() - 1
        if self.points.dim() != 2 or self.points.shape[0] != 19:
            raise ValueError("NuScenesSamples: points must be [19, N_total] (18 radar channels and the timestamp row)")
        if b < 0 or self.chunk_ptr.shape != (c + 1,) or self.chunk_rotation.shape[0] != c or self.chunk_translation.shape[0] != c:
            raise ValueError("NuScenesSamples: chunk_ptr [C + 1], chunk_sample [C], chunk_rotation [C, 4], chunk_translation [C, 3]")
        if any(t.shape[0] != m for t in (self.box_center, self.box_size, self.box_rotation, self.box_points)):
            raise ValueError("NuScenesSamples: box_center / box_size [M, 3], box_rotation [M, 4], box_label / box_points [M]")
        if self.ego_translation.shape[0] != b or self.ego_rotation.shape[0] != b:
            raise ValueError("NuScenesSamples: box_ptr [B + 1], ego_translation [B, 3], ego_rotation [B, 4]")

    @property
    def num_samples(self) -> int:
        return self.box_ptr.numel() - 1

    @property
    def device(self):
        return self.points.device

    @staticmethod
    def from_samples(sensor_points: Sequence[Sequence], calibrations: Sequence[Sequence], boxes: Sequence[dict], device="cuda"):
        """Host adapter.  Per sample: ``sensor_points[s]`` a list of [19, n] arrays (one per sensor, in the order the caller wants
        them concatenated), ``calibrations[s]`` the matching calibrated-sensor records (dicts with ``rotation`` and ``translation``),
        ``boxes[s]`` the dict ``from_devkit_boxes`` returns."""
        blocks = [np.asarray(p, dtype=np.float64).reshape(19, -1) for sample in sensor_points for p in sample]
        sizes = [p.shape[1] for p in blocks]
        sample_of = [s for s, sample in enumerate(sensor_points) for _ in sample]
        cal = [c for sample in calibrations for c in sample]
        if len(cal) != len(blocks):
            raise ValueError("one calibrated-sensor record per sensor point block")
        cat = lambda key, width: np.concatenate([np.asarray(b[key], dtype=np.float64).reshape(-1, width) for b in boxes]) \
            if boxes else np.zeros((0, width))
        return NuScenesSamples(
            np.concatenate(blocks, axis=1) if blocks else np.zeros((19, 0)), np.concatenate(([0], np.cumsum(sizes))).astype(np.int64),
            np.asarray(sample_of, dtype=np.int32), np.asarray([c["rotation"] for c in cal], dtype=np.float64).reshape(-1, 4),
            np.asarray([c["translation"] for c in cal], dtype=np.float64).reshape(-1, 3), cat("box_center", 3), cat("box_size", 3),
            cat("box_rotation", 4), np.concatenate([np.asarray(b["box_label"], dtype=np.int32).reshape(-1) for b in boxes]),
            np.concatenate([np.asarray(b["box_points"], dtype=np.int32).reshape(-1) for b in boxes]),
            np.concatenate(([0], np.cumsum([len(b["box_label"]) for b in boxes]))).astype(np.int64),
            np.asarray([b["ego_translation"] for b in boxes], dtype=np.float64).reshape(-1, 3),
            np.asarray([b["ego_rotation"] for b in boxes], dtype=np.float64).reshape(-1, 4), device=device)


def _quaternion_elements(q) -> np.ndarray:
    for name in ("q", "elements"):
        if hasattr(q, name):
            return np.asarray(getattr(q, name), dtype=np.float64).reshape(4)
    return np.asarray(q, dtype=np.float64).reshape(4)


def from_devkit_boxes(boxes, ego_pose: dict, annotations: Sequence[dict]) -> dict:
    """One sample's boxes as arrays.  ``boxes``: what ``nusc.get_boxes`` returns, read through duck-typed attributes only
    (``box.center``, ``box.wlh``, ``box.orientation.q`` or ``.elements``, ``box.label`` -- the integer the caller has set);
    ``ego_pose``: the LIDAR_TOP sample data's ego pose record; ``annotations``: the boxes' ``sample_annotation`` records.
    Imports neither ``nuscenes`` nor ``pyquaternion``."""
    if len(annotations) != len(boxes):
        raise ValueError("one annotation record per box")
    m = len(boxes)
    return {"box_center": np.asarray([b.center for b in boxes], dtype=np.float64).reshape(m, 3),
            "box_size": np.asarray([b.wlh for b in boxes], dtype=np.float64).reshape(m, 3),
            "box_rotation": np.asarray([_quaternion_elements(b.orientation) for b in boxes], dtype=np.float64).reshape(m, 4),
            "box_label": np.asarray([int(b.label) for b in boxes], dtype=np.int32),
            "box_points": np.asarray([int(a["num_lidar_pts"]) + int(a["num_radar_pts"]) for a in annotations], dtype=np.int32),
            "ego_translation": np.asarray(ego_pose["translation"], dtype=np.float64).reshape(3),
            "ego_rotation": _quaternion_elements(ego_pose["rotation"])}


def sensor_point_block(radar_point_cloud, timestamps) -> np.ndarray:
    """[19, n]: ``np.vstack([pc.points, timestamps])`` of what ``RadarPointCloud.from_file_multisweep`` returns
    (dataset_creation.py:180-183), read through the duck-typed ``.points``."""
    return np.vstack([np.asarray(radar_point_cloud.points, dtype=np.float64), np.asarray(timestamps, dtype=np.float64).reshape(1, -1)])


# ------------------------------------------------------------------------------------------------ stages
def _status_errors(st: int, what: str) -> None:
    fired = []
    if st & ops.STATUS_NUSC_BAD_CHUNK:
        fired.append("RGNN_STATUS_NUSC_BAD_CHUNK: chunk_sample must be non-decreasing inside [0, B) and chunk_ptr (frame_ptr) must "
                     "rise inside the rows")
    if st & ops.STATUS_NUSC_BAD_BOX_PTR:
        fired.append("RGNN_STATUS_NUSC_BAD_BOX_PTR: box_ptr must rise inside [0, M]")
    if fired:
        raise ValueError(f"{what}: " + "; ".join(fired))


def sample_point_clouds(samples: NuScenesSamples, dataset_config):
    """Stage a: -> (FrameBatch in the vehicle frame, cropped, z dropped; V_cc f64 [N, 2] = channels 6-7; src_row int32 [N] = the row
    of ``samples.points``), samples back to back, rows in the order given.  ``batch.V`` is channels 8-9 turned by the upper-left
    2 x 2 of the sensor's rotation.  A point exactly on a crop limit stays.  One host read."""
    out = ops.nusc_points(samples.points, samples.chunk_ptr, samples.chunk_sample, samples.chunk_rotation, samples.chunk_translation,
                          samples.num_samples, *_crop(dataset_config))
    frame_ptr, status = out[0], out[-1]
    head = torch.cat((frame_ptr, status.to(torch.int64))).cpu().numpy()                # the one host read
    ptr = head[:-1]
    _status_errors(int(head[-1]), "sample_point_clouds")
    n = int(ptr[-1])
    X, V, V_cc, rcs, ts, src_row = (t[:n] for t in out[1:-1])
    return FrameBatch(X, V, rcs, ts, frame_ptr, np.diff(ptr)), V_cc, src_row


@dataclass
class PreparedBoxes:
    """Stage b's result: ``records`` f64 [M, 20] (rgnn.h), sample s's survivors in list order at
    [box_ptr[s], box_ptr[s] + box_count[s])."""
    records: torch.Tensor
    box_ptr: torch.Tensor
    box_count: torch.Tensor
    status: torch.Tensor
    wlh_factor: float

    def survivors(self):
        """-> (kept int64 [K]: indices into the input list, sample by sample in list order; kept_ptr int64 [B + 1];
        rect f64 [K, 5] = x_c, y_c, l, w, theta in degrees; label int64 [K]).  Reads the counts back once."""
        _status_errors(int(self.status.item()), "prepare_boxes")
        count = self.box_count.to(torch.int64)
        m = self.records.shape[0]
        at = torch.arange(m, device=self.records.device)
        seg = torch.bucketize(at, self.box_ptr[1:].contiguous(), right=True).clamp_(max=max(count.numel() - 1, 0))
        live = at < (self.box_ptr[:-1] + count)[seg] if count.numel() else torch.zeros(0, dtype=torch.bool, device=at.device)
        rows = torch.nonzero(live).view(-1)
        rec = self.records.index_select(0, rows)
        kept_ptr = torch.cat((torch.zeros(1, dtype=torch.int64, device=at.device), torch.cumsum(count, 0)))
        return rec[:, REC_SRC].to(torch.int64), kept_ptr, rec[:, REC_RECT], rec[:, REC_LABEL].to(torch.int64)


def prepare_boxes(samples: NuScenesSamples, dataset_config, wlh_factor: Optional[float] = None) -> PreparedBoxes:
    """Stage b: drop boxes without lidar or radar points, move the rest to the vehicle frame, crop by centre (strictly inside),
    keep list order, and prepare per survivor the membership geometry and the rotated rectangle.  No host read."""
    factor = float(dataset_config.wlh_factor if wlh_factor is None else wlh_factor)
    records, count, status = ops.nusc_boxes(samples.box_center, samples.box_size, samples.box_rotation, samples.box_label,
                                            samples.box_points, samples.box_ptr, samples.ego_translation, samples.ego_rotation,
                                            *_crop(dataset_config), factor)
    return PreparedBoxes(records, samples.box_ptr, count, status, factor)


def label_points(pos: torch.Tensor, frame_ptr, boxes: PreparedBoxes, bb_invariance: str, wlh_offset: float = 0.0,
                 nn_index: Optional[torch.Tensor] = None):
    """Stage c: -> (labels int32 [N], 0 = no box; targets f64 [N, 5], NaN = no box; hit int32 [N], the winning box's index in the
    input list, -1 = none).  ``pos`` f64 [N, 2] in the vehicle frame, ``frame_ptr`` B + 1 offsets (a tensor in HBM or a host
    sequence).  A point belongs to the LAST box in list order that contains it; the test is inclusive on both sides.  The en
    encoding searches the nearest other point of the frame first (a frame of one point raises sklearn's error)."""
    if bb_invariance not in INVARIANCE_CODES:
        raise ValueError("Wrong invariance for bounding box selection")
    pos = ops._dev(pos, "pos", torch.float64).contiguous()
    if not isinstance(frame_ptr, torch.Tensor):
        frame_ptr = torch.tensor([int(v) for v in frame_ptr], dtype=torch.int64, device=pos.device)
    inv = INVARIANCE_CODES[bb_invariance]
    if inv == 2 and nn_index is None:
        nn_index = _nearest_in_frames(pos, [int(v) for v in frame_ptr.tolist()])
    labels, targets, hit, _ = ops.nusc_label_points(pos, frame_ptr, boxes.records, boxes.box_ptr, boxes.box_count,
                                                    nn_index if inv == 2 else None, inv, float(wlh_offset), status=boxes.status)
    return labels, targets, hit


# ------------------------------------------------------------------------------------------------ the reference's surface
class _OneSampleBoxes:
    """Boxes already in the vehicle frame (what ``get_labels`` returns) as a one-sample batch with a level ego pose at the origin."""

    def __init__(self, boxes, device):
        m = len(boxes)
        arr = lambda rows, width: np.asarray(rows, dtype=np.float64).reshape(m, width)
        self.box_center = _up(arr([b.center for b in boxes], 3), "box.center", torch.float64, device)
        self.box_size = _up(arr([b.wlh for b in boxes], 3), "box.wlh", torch.float64, device)
        self.box_rotation = _up(arr([_quaternion_elements(b.orientation) for b in boxes], 4), "box.orientation", torch.float64, device)
        self.box_label = _up(np.asarray([int(getattr(b, "label", 0)) for b in boxes], dtype=np.int32), "box.label", torch.int32, device)
        self.box_points = torch.ones(m, dtype=torch.int32, device=device)
        self.box_ptr = torch.tensor([0, m], dtype=torch.int64, device=device)
        self.ego_translation = torch.zeros((1, 3), dtype=torch.float64, device=device)
        self.ego_rotation = torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64, device=device)


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("radargnn_amd.nuscenes: the nuScenes kernels need a GPU (no CPU fallback)")
    return torch.device("cuda")


_NO_CROP = NuScenesDatasetConfiguration(crop_point_cloud=False)


def convert_bounding_boxes(config, point_cloud, boxes, wlh_factor: float = 1.0, wlh_offset: float = 0.0) -> torch.Tensor:
    """conversion.py:112-187 under the reference's name: ``point_cloud.X_cc`` [N, 2] and ``boxes`` in the vehicle frame (duck-typed
    ``center``, ``wlh``, ``orientation``) -> float64 [N, 5] in HBM, NaN for points of no box, in ``config.bb_invariance``."""
    dev = _device()
    pos = _up(np.asarray(point_cloud.X_cc, dtype=np.float64).reshape(-1, 2), "X_cc", torch.float64, dev)
    prepared = prepare_boxes(_OneSampleBoxes(boxes, dev), _NO_CROP, wlh_factor)
    _, targets, _ = label_points(pos, [0, pos.shape[0]], prepared, config.bb_invariance, wlh_offset)
    _status_errors(int(prepared.status.item()), "convert_bounding_boxes")
    return targets


def extended_points_in_box(box, points, wlh_factor: float = 1.0, wlh_offset: float = 0.0, use_z: bool = True) -> torch.Tensor:
    """utils.py:6-48 under the reference's name: ``points`` [3, N] -> bool [N] in HBM.  The reference only ever calls it with
    ``use_z=False`` and with z at zero (dataset_creation.py:248,272, conversion.py:141); that is the form the kernel has."""
    if use_z:
        raise NotImplementedError("extended_points_in_box: use_z=True is never used by the reference and has no kernel")
    dev = _device()
    pts = points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else np.asarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[0] != 3:
        raise ValueError("points must be [3, N]")
    if np.any(pts[2] != 0):
        raise NotImplementedError("extended_points_in_box: the kernel takes points at z = 0, as the reference passes them")
    pos = _up(np.ascontiguousarray(pts[:2].T), "points", torch.float64, dev)
    prepared = prepare_boxes(_OneSampleBoxes([box], dev), _NO_CROP, wlh_factor)
    _, _, hit = label_points(pos, [0, pos.shape[0]], prepared, "none", wlh_offset)
    return hit >= 0


class _PointCloud:
    """The attributes ``convert_point_cloud`` assigns (conversion.py:48-67), as tensors in HBM."""
    X_cc = V_cc = V_cc_compensated = rcs = timestamp = label_id = None


def convert_point_cloud(points, labels):
    """conversion.py:15-67: nuScenes rows [19, N] (vehicle frame) and labels [N] -> an object with X_cc, V_cc, V_cc_compensated
    [N, 2], rcs, timestamp, label_id [N, 1]; tensors stay where they are, arrays stay arrays."""
    pc = _PointCloud()
    if isinstance(points, torch.Tensor):
        col = lambda i: points[i].reshape(-1, 1)
        pc.X_cc, pc.V_cc, pc.V_cc_compensated = points[0:2].T, points[6:8].T, points[8:10].T
        pc.label_id = torch.as_tensor(labels).reshape(-1, 1)
    else:
        points = np.asarray(points)
        col = lambda i: np.atleast_2d(points[i]).T
        pc.X_cc, pc.V_cc, pc.V_cc_compensated = points[0:2].T, points[6:8].T, points[8:10].T
        pc.label_id = np.atleast_2d(np.asarray(labels)).T
    pc.rcs, pc.timestamp = col(5), col(18)
    return pc


def create_graph_data_from_samples(samples: NuScenesSamples, graph_config, dataset_config) -> list:
    """``process_single_sample`` (dataset_creation.py:310-354) for every sample of the batch, from the arrays on: stages a-c,
    ``build_graphs``, ``merge_targets``; -> one ``data.Data`` per sample (x, edge_index with frame-local numbering, edge_attr,
    y [N, 6] = label | box, pos, vel -- float32 / int64 as ``create_graph_data`` stores them), all in HBM.
    A sample left with fewer than two points cannot be processed by the reference either (its graph has no ``E`` and
    dataset_creation.py:298 raises): ValueError naming the samples, before any graph kernel runs."""
    from .data import Data
    from .groundtruth import merge_targets
    from .preprocessor import graph_settings
    if dataset_config.bb_invariance not in INVARIANCE_CODES:
        raise ValueError("Wrong invariance for bounding box selection")
    batch, _, _ = sample_point_clouds(samples, dataset_config)
    sizes = batch.frame_sizes
    if (sizes < 2).any():
        raise ValueError(f"create_graph_data_from_samples: samples {np.nonzero(sizes < 2)[0].tolist()} are left with fewer than two "
                         "points; the reference cannot build their graphs either")
    if len(sizes) == 0:
        return []
    ptr = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    prepared = prepare_boxes(samples, dataset_config)
    labels, boxes, _ = label_points(batch.X, ptr.tolist(), prepared, dataset_config.bb_invariance, dataset_config.wlh_offset)
    g = build_graphs(batch, graph_settings(graph_config))
    g.check()
    _status_errors(int(prepared.status.item()), "create_graph_data_from_samples")
    y = merge_targets(labels, boxes)
    pos, vel = batch.X.to(torch.float32), batch.V.to(torch.float32)
    # edges are grouped by their query in ascending order: a sample's edges are one contiguous range
    eptr = torch.searchsorted(g.edge_index[0].contiguous(), batch.frame_ptr).tolist()
    out = []
    for f in range(len(sizes)):
        a, b, ea, eb = int(ptr[f]), int(ptr[f + 1]), eptr[f], eptr[f + 1]
        out.append(Data(x=g.x[a:b], edge_index=g.edge_index[:, ea:eb] - a, edge_attr=g.edge_attr[ea:eb], y=y[a:b], pos=pos[a:b],
                        vel=vel[a:b]))
    return out
