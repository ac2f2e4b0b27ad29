"""Point-cloud frames from a RadarScenes sequence's radar scans, in HBM: the reference's ``create_point_cloud_frames``,
``concatenate_subsequent_scenes``, ``SceneCollection.process`` and ``PointCloudProcessor.transform``
(preprocessor/radarscenes/dataset_creation.py:159-184,716-783, scene_collection.py:36-156,185-230) -- the step in front of the graph
build, so that a sequence's detection table goes in once and graphs with targets come out without the points returning to the host.

    table = SequenceTable(radar_data)                                   # the columns in HBM; scenes from the timestamps
    windows = plan_windows(table.scene_timestamps, 0.5)                 # host, numpy: [first scene, last scene] per frame
    batch, label, track, src_row = accumulate_frames(table, windows, dataset_config, sensor_yaw, label_map)
    graphs = create_graph_data_from_sequence(table, graph_config, dataset_config, sensor_yaw, label_map)   # list[Data]

The host plans (which scenes make a frame: a few thousand int64 comparisons); the device does the rest in three launches
(csrc/preprocess.hip: count, scan, write -- a masked, order-preserving compaction of overlapping row ranges with one cos / sin pair
per row) straight into the layout ``frames.FrameBatch`` uses.  One host read per call: ``frame_ptr`` with the status word.
There is no CPU path for the device part.

``sensor_yaw`` and ``label_map`` have NO defaults: ``radar_scenes`` is not a dependency of this package and its values are not
restated here.  A caller with the dataset tools builds them once:

    sensor_yaw = [0.0] + [radar_scenes.sensors.get_mounting(s, json_path=None)["yaw"] for s in (1, 2, 3, 4)]   # index = sensor_id
    label_map = [None if (c := ClassificationLabel.label_to_clabel(Label(i))) is None else c.value for i in range(12)]  # index = label_id

(``radar_scenes.labels.ClassificationLabel`` / ``Label``; ``None`` or a negative entry drops the rows of that label, as the
reference's ``remove_points_without_labelID`` does.)
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .frames import FrameBatch, GraphSettings, build_graphs

# the table's columns as RadarScenes stores them (radar_data.h5) and as the kernel reads them
COLUMN_DTYPES = {"timestamp": np.int64, "sensor_id": np.uint8, "azimuth_sc": np.float32, "rcs": np.float32, "vr": np.float32,
                 "vr_compensated": np.float32, "x_cc": np.float32, "y_cc": np.float32, "label_id": np.uint8}
HOST_ONLY = ("range_sc", "x_seq", "y_seq", "uuid")          # kept on the host when present; gathered through src_row


@dataclass
class RadarScenesDatasetConfiguration:
    """Field-compatible with preprocessor/radarscenes/configs.py:5-20 (positional construction works)."""
    time_per_point_cloud_frame: float
    crop_point_cloud: bool
    crop_settings: dict
    bounding_boxes_aligned: bool
    bb_invariance: str
    create_small_subset: bool
    subset_settings: dict = None

    deterministic: bool = False
    seed: int = 0

    parallelize: bool = False


# ------------------------------------------------------------------------------------------------ host plan
def plan_windows(scene_timestamps, time_per_point_cloud_frame: float) -> np.ndarray:
    """int64 [W, 2]: first and last scene (inclusive) of every frame of a sequence whose scenes have these timestamps (int64 us,
    strictly increasing).  A window starts at scene i, takes scene i + 1 if there is one and keeps taking the next scene while
    ``(ts[last taken] - ts[i]) * 1e-6 < time_per_point_cloud_frame`` -- evaluated as the reference does (scene_collection.py:213):
    int64 difference, times the double 1e-6, against the double setting -- so it ends with the first scene at or beyond the span or
    with the last scene.  The next window starts at the scene this one ended with; the plan ends with the window that reaches the
    last scene (dataset_creation.py:747-768)."""
    ts = np.asarray(scene_timestamps)
    if ts.ndim != 1 or ts.size == 0:
        raise ValueError("plan_windows: an empty sequence (scene_timestamps must be [n_scenes], n_scenes >= 1)")
    if ts.dtype.kind not in "iu":
        raise ValueError("plan_windows: scene_timestamps must be integers (int64 microseconds)")
    ts = ts.astype(np.int64)
    if np.any(ts[1:] <= ts[:-1]):
        raise ValueError("plan_windows: scene timestamps must increase strictly")
    span = float(time_per_point_cloud_frame)
    last, out, i = ts.size - 1, [], 0
    while True:
        j = min(i + 1, last)
        while j < last and float((ts[j] - ts[i]) * 1e-6) < span:
            j += 1
        out.append((i, j))
        if j == last:
            break
        i = j
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def subset_windows(windows, num_clouds_per_sequence: int) -> np.ndarray:
    """The frames a small subset keeps (dataset_creation.py:778-781): ``floor(linspace(0, W - 1, m))`` of the window list, applied
    to the plan so that only the chosen frames are built (the reference picks from the finished list, empty frames included)."""
    windows = np.asarray(windows, dtype=np.int64).reshape(-1, 2)
    pick = np.floor(np.linspace(0, windows.shape[0] - 1, int(num_clouds_per_sequence))).astype(int)
    return windows[pick]


def scenes_from_rows(row_timestamps):
    """(scene_timestamps int64 [S], scene_ptr int64 [S + 1]) of a table sorted by time: a scene is a run of equal timestamps.
    An unsorted table is refused (its scenes would not be contiguous).  Scenes without detections cannot be seen in the rows: pass
    them to ``SequenceTable`` explicitly."""
    ts = np.asarray(row_timestamps)
    if ts.ndim != 1 or ts.dtype.kind not in "iu":
        raise ValueError("scenes_from_rows: row timestamps must be an integer array [n_rows]")
    ts = ts.astype(np.int64)
    if np.any(ts[1:] < ts[:-1]):
        raise ValueError("scenes_from_rows: the table is not sorted by timestamp")
    first = np.ones(ts.size, dtype=bool)
    first[1:] = ts[1:] != ts[:-1]
    starts = np.nonzero(first)[0].astype(np.int64)
    return ts[starts], np.concatenate((starts, np.array([ts.size], dtype=np.int64)))


# ------------------------------------------------------------------------------------------------ the table in HBM
def _exact_cast(values, dtype, name: str) -> np.ndarray:
    """``values`` in the stored dtype; refused if the cast would change a value."""
    a = np.asarray(values)
    if a.dtype == dtype:
        return np.ascontiguousarray(a)
    if a.dtype.kind not in "iufb":
        raise ValueError(f"SequenceTable: column `{name}` must be numeric, got {a.dtype}")
    if np.dtype(dtype).kind in "iu":
        info = np.iinfo(dtype)
        whole = a.dtype.kind != "f" or bool(np.isfinite(a).all() and (a == np.trunc(a)).all())
        same = a.size == 0 or (whole and info.min <= a.min() and a.max() <= info.max)
    else:
        with np.errstate(over="ignore"):
            same = np.array_equal(a.astype(dtype).astype(np.float64), a.astype(np.float64), equal_nan=True)
    if not same:
        raise ValueError(f"SequenceTable: column `{name}` ({a.dtype}) does not fit {np.dtype(dtype).name} without changing a value")
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(a.astype(dtype))


class SequenceTable:
    """The detections of one sequence (``radar_data`` of radar_scenes' Sequence) resident in HBM, with its scenes.

    ``data``: a numpy structured array or a dict of columns with RadarScenes' field names (``COLUMN_DTYPES`` plus ``track_id``;
    ``range_sc``, ``x_seq``, ``y_seq``, ``uuid`` stay on the host when present).  A column in another dtype is cast only if no value
    changes.  ``track_id`` (byte strings) is mapped once to int32: the rank among the sequence's distinct ids, ``b""`` = -1
    (``track_names[i]`` is the id of rank i).  Scenes: runs of equal timestamps of the sorted table, or ``scene_timestamps`` /
    ``scene_ptr`` given explicitly (needed only for scenes without detections)."""

    def __init__(self, data, scene_timestamps=None, scene_ptr=None, device="cuda"):
        if isinstance(data, np.ndarray) and data.dtype.names:
            get, names = (lambda k: data[k]), set(data.dtype.names)
        elif isinstance(data, dict):
            get, names = (lambda k: data[k]), set(data)
        else:
            raise ValueError("SequenceTable: a numpy structured array or a dict of columns")
        missing = [k for k in (*COLUMN_DTYPES, "track_id") if k not in names]
        if missing:
            raise ValueError(f"SequenceTable: missing columns {missing}")
        host = {k: _exact_cast(get(k), dt, k) for k, dt in COLUMN_DTYPES.items()}
        n = host["timestamp"].shape[0]
        tid = np.asarray(get("track_id"))
        if any(c.ndim != 1 or c.shape[0] != n for c in (*host.values(), tid)):
            raise ValueError("SequenceTable: every column must be [n_rows]")
        if tid.dtype.kind in "SUO":
            tid = tid.astype(np.bytes_) if tid.dtype.kind != "S" else tid
            self.track_names, inverse = np.unique(tid, return_inverse=True)
            track = inverse.reshape(-1).astype(np.int32)
            if self.track_names.size and self.track_names[0] == b"":
                track -= 1
                self.track_names = self.track_names[1:]
        else:                                                   # already numbered: negative = background
            track = _exact_cast(tid, np.int32, "track_id")
            self.track_names = None
        host["track"] = np.ascontiguousarray(track)
        if (scene_timestamps is None) != (scene_ptr is None):
            raise ValueError("SequenceTable: give scene_timestamps and scene_ptr together")
        if scene_ptr is None:
            scene_timestamps, scene_ptr = scenes_from_rows(host["timestamp"])
        self.scene_timestamps = np.asarray(scene_timestamps, dtype=np.int64).reshape(-1)
        self.scene_ptr = np.asarray(scene_ptr, dtype=np.int64).reshape(-1)
        sp = self.scene_ptr
        if sp.size != self.scene_timestamps.size + 1 or sp[0] != 0 or sp[-1] != n or np.any(sp[1:] < sp[:-1]):
            raise ValueError("SequenceTable: scene_ptr must rise from 0 to n_rows with one entry per scene plus one")
        if n and not np.array_equal(host["timestamp"], np.repeat(self.scene_timestamps, np.diff(sp))):
            raise ValueError("SequenceTable: a row's timestamp differs from its scene's")
        self.host = host
        self.host_only = {k: np.asarray(get(k)) for k in HOST_ONLY if k in names}
        self.track_id = tid
        self.num_rows = n
        if not torch.cuda.is_available():
            raise RuntimeError("SequenceTable: the pre-processor kernels need a GPU (no CPU fallback)")
        self.columns = {k: torch.from_numpy(v).to(device) for k, v in host.items()}

    @property
    def device(self):
        return self.columns["timestamp"].device

    def window_rows(self, windows) -> np.ndarray:
        """int64 [W, 2] row ranges of windows given as [first scene, last scene]."""
        w = np.asarray(windows, dtype=np.int64).reshape(-1, 2)
        s = self.scene_timestamps.size
        if w.size and (w.min() < 0 or w.max() >= s or np.any(w[:, 1] < w[:, 0])):
            raise ValueError("windows must be [first scene, last scene] pairs inside the sequence")
        return np.stack((self.scene_ptr[w[:, 0]], self.scene_ptr[w[:, 1] + 1]), axis=1)


# ------------------------------------------------------------------------------------------------ device
def _tables(sensor_yaw, label_map, device):
    if sensor_yaw is None or label_map is None:
        raise ValueError("sensor_yaw and label_map have no defaults: see the module docstring for where a caller gets them")
    yaw = torch.tensor([float(v) for v in sensor_yaw], dtype=torch.float64).to(device)
    lab = []
    for v in label_map:
        drop = v is None or (isinstance(v, float) and np.isnan(v)) or v < 0
        if not drop and int(v) != v:
            raise ValueError("label_map entries are class indices (ints), None or negative for labels to drop")
        lab.append(-1 if drop else int(v))
    return yaw, torch.tensor(lab, dtype=torch.int32).to(device)


def _crop(dataset_config):
    if not dataset_config.crop_point_cloud:
        return False, 0.0, 0.0
    return True, float(dataset_config.crop_settings.get("front")), float(dataset_config.crop_settings.get("sides"))


def _accumulate(columns, win_rows: np.ndarray, crop, sensor_yaw, label_map, device, what: str):
    yaw, lab = _tables(sensor_yaw, label_map, device)
    n_cap = int((win_rows[:, 1] - win_rows[:, 0]).sum())
    out = ops.accumulate_frames(columns, torch.from_numpy(np.ascontiguousarray(win_rows)).to(device), yaw, lab, *crop, n_cap)
    frame_ptr, status = out[0], out[-1]
    head = torch.cat((frame_ptr, status.to(torch.int64))).cpu().numpy()              # the one host read
    ptr, st = head[:-1], int(head[-1])
    if st & ops.STATUS_PREPROCESS_BAD_ROW:
        raise ValueError(f"{what}: RGNN_STATUS_PREPROCESS_BAD_ROW: a sensor_id outside sensor_yaw ({yaw.numel()} entries) or a "
                         f"label_id outside label_map ({lab.numel()} entries)")
    n = int(ptr[-1])
    return ptr, [t[:n] for t in out[1:-1]]


def accumulate_frames(table: SequenceTable, windows, dataset_config, sensor_yaw, label_map):
    """The frames of ``windows`` ([first scene, last scene] pairs, e.g. ``plan_windows``) -> (FrameBatch, label int32 [N],
    track int32 [N], src_row int32 [N]), everything in HBM, frames back to back in window order, rows in table order.
    ``label``: the reduced class of ``label_map``; ``track``: ``table``'s numbering, -1 = background -- the ``object_id`` of
    ``groundtruth.create_2d_bounding_boxes_batched``; ``src_row``: the row of the table, to gather any other column.
    Empty frames are kept (``frame_sizes`` has zeros).  An id outside its table raises ValueError."""
    win_rows = table.window_rows(windows)
    ptr, (X, V, rcs, ts, label, track, src_row) = _accumulate(table.columns, win_rows, _crop(dataset_config), sensor_yaw, label_map,
                                                             table.device, "accumulate_frames")
    batch = FrameBatch(X, V, rcs, ts, torch.from_numpy(ptr.copy()).to(table.device), np.diff(ptr))
    return batch, label, track, src_row


# ------------------------------------------------------------------------------------------------ the reference's surface
class RadarPointCloud:
    """preprocessor/radar_point_cloud.py with the reference's attribute and method names: numpy arrays, one row per point."""

    def __init__(self):
        self.X_cc = None
        self.X_seq = None
        self.V_cc = None
        self.V_cc_compensated = None
        self.range_sc = None
        self.azimuth_sc = None
        self.rcs = None
        self.vr = None
        self.vr_compensated = None
        self.timestamp = None
        self.sensor_id = None
        self.uuid = None
        self.track_id = None
        self.label_id = None

    def keep_rows(self, rows) -> None:
        for key, value in vars(self).items():
            if value is not None:
                vars(self)[key] = np.asarray(value)[rows]

    def remove_points_based_on_index(self, idx_array) -> None:
        n = next((len(v) for v in vars(self).values() if v is not None), 0)
        mask = np.ones(n, dtype=bool)
        mask[np.asarray(idx_array, dtype=np.int64)] = False
        self.keep_rows(mask)

    def remove_points_without_labelID(self) -> None:
        self.remove_points_based_on_index(np.nonzero(np.isnan(np.asarray(self.label_id, dtype=np.float64)[:, 0]))[0])

    def remove_points_without_valid_velocity(self) -> None:
        self.remove_points_based_on_index(np.nonzero(np.isnan(self.V_cc_compensated).any(axis=1))[0])

    def remove_points_out_of_range(self, x_max: float, y_max: float) -> None:
        x, y = self.X_cc[:, 0], self.X_cc[:, 1]
        with np.errstate(invalid="ignore"):
            self.remove_points_based_on_index(np.nonzero((np.abs(y) > y_max) | (x > x_max) | (x < 0))[0])


class PointCloudProcessor:
    """dataset_creation.py:159-184 for a cloud that arrives already assembled: the keep decision is the W = 1 case of the kernel
    (crop, label, compensated velocity), the cloud's arrays are then narrowed on the host."""

    @staticmethod
    def transform(dataset_config, point_cloud):
        X = np.asarray(point_cloud.X_cc, dtype=np.float64)
        n = X.shape[0]
        if n == 0:
            return point_cloud
        x32 = X.astype(np.float32)
        if not np.array_equal(x32.astype(np.float64), X, equal_nan=True):
            raise ValueError("PointCloudProcessor.transform: X_cc holds values float32 does not (RadarScenes stores float32); "
                             "the device crop would not see the same numbers")
        if not torch.cuda.is_available():
            raise RuntimeError("PointCloudProcessor.transform: the pre-processor kernels need a GPU (no CPU fallback)")
        dev = torch.device("cuda")
        bad_v = np.isnan(np.asarray(point_cloud.V_cc_compensated, dtype=np.float64)).any(axis=1)
        no_label = np.isnan(np.asarray(point_cloud.label_id, dtype=np.float64).reshape(n))
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        zeros = np.zeros(n, dtype=np.float32)
        columns = {"timestamp": up(np.zeros(n, dtype=np.int64)), "sensor_id": up(np.zeros(n, dtype=np.uint8)), "azimuth_sc": up(zeros),
                   "rcs": up(zeros), "vr_compensated": up(np.where(bad_v, np.float32("nan"), np.float32(0))),
                   "x_cc": up(x32[:, 0]), "y_cc": up(x32[:, 1]), "label_id": up((~no_label).astype(np.uint8)),
                   "track": up(np.zeros(n, dtype=np.int32))}
        _, out = _accumulate(columns, np.array([[0, n]], dtype=np.int64), _crop(dataset_config), [0.0], [None, 0], dev,
                             "PointCloudProcessor.transform")
        rows = out[-1].cpu().numpy().astype(np.int64)
        if hasattr(point_cloud, "keep_rows"):
            point_cloud.keep_rows(rows)
        else:
            for key, value in vars(point_cloud).items():
                if value is not None:
                    vars(point_cloud)[key] = np.asarray(value)[rows]
        return point_cloud


def _windows_of(table: SequenceTable, dataset_config) -> np.ndarray:
    windows = plan_windows(table.scene_timestamps, dataset_config.time_per_point_cloud_frame)
    subset = dataset_config.subset_settings or {}
    if dataset_config.create_small_subset and "num_clouds_per_sequence" in subset:
        windows = subset_windows(windows, subset.get("num_clouds_per_sequence"))
    return windows


def create_point_cloud_frames(table: SequenceTable, dataset_config, sensor_yaw, label_map) -> List[RadarPointCloud]:
    """dataset_creation.py:716-783 on a ``SequenceTable``: one ``RadarPointCloud`` per frame, empty ones included, with the
    reference's attributes as host arrays ([n, 2] / [n, 1] float64, ``label_id`` the reduced class).  The filter and the compensated
    velocity come from the device; the remaining columns are gathered through ``src_row``.  ``X_seq`` is left out (the reference
    transforms it and never reads it again)."""
    batch, label, _, src_row = accumulate_frames(table, _windows_of(table, dataset_config), dataset_config, sensor_yaw, label_map)
    ptr = np.concatenate(([0], np.cumsum(batch.frame_sizes))).astype(np.int64)
    rows = src_row.cpu().numpy().astype(np.int64)
    X, V = batch.X.cpu().numpy(), batch.V.cpu().numpy()
    rcs, ts, label = batch.rcs.cpu().numpy(), batch.timestamp.cpu().numpy(), label.cpu().numpy().astype(np.float64)
    h = table.host
    col = lambda name: h[name][rows].astype(np.float64).reshape(-1, 1)
    azimuth, vr, sensor = col("azimuth_sc"), col("vr"), h["sensor_id"][rows]
    yaw = np.asarray([float(v) for v in sensor_yaw], dtype=np.float64)[sensor].reshape(-1, 1)
    angles = azimuth + yaw
    V_cc = np.concatenate([vr * np.cos(angles), vr * np.sin(angles)], axis=1)
    clouds = []
    for a, b in zip(ptr[:-1], ptr[1:]):
        pc = RadarPointCloud()
        pc.X_cc, pc.V_cc_compensated, pc.V_cc = X[a:b], V[a:b], V_cc[a:b]
        pc.rcs, pc.timestamp, pc.label_id = rcs[a:b].reshape(-1, 1), ts[a:b].reshape(-1, 1), label[a:b].reshape(-1, 1)
        pc.azimuth_sc, pc.vr, pc.vr_compensated = azimuth[a:b], vr[a:b], col("vr_compensated")[a:b]
        pc.sensor_id = sensor[a:b].astype(np.float64).reshape(-1, 1)
        pc.track_id = table.track_id[rows[a:b]]
        if "range_sc" in table.host_only:
            pc.range_sc = table.host_only["range_sc"][rows[a:b]].astype(np.float64).reshape(-1, 1)
        if "uuid" in table.host_only:
            pc.uuid = table.host_only["uuid"][rows[a:b]]
        clouds.append(pc)
    return clouds


def graph_settings(graph_config) -> GraphSettings:
    """``GraphConstructionConfiguration`` -> the settings ``frames.build_graphs`` takes."""
    base = GraphSettings()
    return GraphSettings(algorithm=graph_config.graph_construction_algorithm, k=base.k if graph_config.k is None else int(graph_config.k),
                         r=base.r if graph_config.r is None else float(graph_config.r), node_features=tuple(graph_config.node_features),
                         edge_features=tuple(graph_config.edge_features), edge_mode=graph_config.edge_mode,
                         distance_definition=graph_config.distance_definition,
                         max_neighbors=getattr(graph_config, "max_neighbors", None))


def create_graph_data_from_sequence(table: SequenceTable, graph_config, dataset_config, sensor_yaw, label_map) -> list:
    """``create_graph_data_from_one_radar_scenes_sequence`` (dataset_creation.py:667-713) from the detection table on: plan, subset,
    accumulate, leave out frames of fewer than two points, ``build_graphs``, box targets with ``track`` as the object id,
    ``merge_targets``; -> one ``data.Data`` per remaining frame (x, edge_index with frame-local numbering, edge_attr, y, pos, vel --
    float32 / int64 as ``create_graph_data`` stores them), all in HBM.  The points never return to the host."""
    from .data import Data
    from .groundtruth import create_2d_bounding_boxes_batched, merge_targets
    batch, label, track, _ = accumulate_frames(table, _windows_of(table, dataset_config), dataset_config, sensor_yaw, label_map)
    sizes = batch.frame_sizes
    if (sizes < 2).any():                                       # dataset_creation.py:698; a dropped frame has at most one row
        kept = sizes >= 2
        row_kept = np.repeat(kept, sizes)
        if not row_kept.all():
            idx = torch.from_numpy(np.nonzero(row_kept)[0]).to(table.device)
            batch = FrameBatch(*(t.index_select(0, idx) for t in (batch.X, batch.V, batch.rcs, batch.timestamp)), None, None)
            label, track = label.index_select(0, idx), track.index_select(0, idx)
        sizes = sizes[kept]
    if len(sizes) == 0:
        return []
    ptr = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    batch = FrameBatch(batch.X, batch.V, batch.rcs, batch.timestamp, torch.from_numpy(ptr).to(table.device), sizes)
    g = build_graphs(batch, graph_settings(graph_config))
    g.check()
    boxes = create_2d_bounding_boxes_batched(batch.X, track, ptr.tolist(), dataset_config.bounding_boxes_aligned,
                                             dataset_config.bb_invariance)
    y = merge_targets(label, boxes)
    pos, vel = batch.X.to(torch.float32), batch.V.to(torch.float32)
    # edges are grouped by their query in ascending order: a frame's edges are one contiguous range
    eptr = torch.searchsorted(g.edge_index[0].contiguous(), batch.frame_ptr).tolist()
    out = []
    for f in range(len(sizes)):
        a, b, ea, eb = int(ptr[f]), int(ptr[f + 1]), eptr[f], eptr[f + 1]
        out.append(Data(x=g.x[a:b], edge_index=g.edge_index[:, ea:eb] - a, edge_attr=g.edge_attr[ea:eb], y=y[a:b], pos=pos[a:b],
                        vel=vel[a:b]))
    return out
