"""Writes tests/golden/nuscenes_*.npz: inputs and outputs of the reference's nuScenes sample stage, produced by EXECUTING the
reference's own utils.extended_points_in_box, conversion.convert_point_cloud, conversion.convert_bounding_boxes and
NuScenesGraphDataset.crop_point_cloud, crop_bounding_boxes, get_sensor_points and get_labels, loaded from /root/reference by file
path; nothing of it is restated here.  The packages that are absent (nuscenes, pyquaternion, torch_geometric) and the reference
modules out of scope are stubbed; preprocessor/bounding_box.py, radar_point_cloud.py, nuscenes/utils.py, conversion.py, configs.py
and dataset_creation.py are loaded for real.  Runs only on the build machine; the fixtures are committed.

The only stand-ins are this file's small ``Box`` and ``Quaternion`` (the devkit's conventions as radargnn_amd/nuscenes.py states
them -- NOT pinned by an executed devkit) and a mocked ``nusc`` that serves the prepared dictionaries.  The sensors are visited in
the order of the chunk list: the reference iterates a Python set there, so it has no order of its own.

Stored per fixture: the inputs (the fields of NuScenesSamples), the settings, the reference's cropped points [19, N] with z at zero,
frame_ptr, labels, the surviving boxes (index in the input list, per-sample offsets, centre and bottom corners in the vehicle frame,
the rectangle [x_c, y_c, l, w, theta in degrees] from the reference's BoundingBox), the three target matrices (boxes_none,
boxes_translation, boxes_en) and the admissibility margins (nuscenes_oracle.admissibility).  The samples are re-seeded until every
margin holds, so the tests leave out nothing.
"""
import importlib.util
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import nuscenes_oracle as O  # noqa: E402

R = "/root/reference/src/gnnradarobjectdetection"
P = "gnnradarobjectdetection"


# ------------------------------------------------------------------------------------------------ stand-ins for the devkit
class Quaternion:
    """(w, x, y, z); rotation_matrix normalises first and is the standard matrix of a unit quaternion."""

    def __init__(self, q):
        self.q = np.asarray(q, dtype=np.float64)

    @property
    def rotation_matrix(self):
        w, x, y, z = self.q / np.sqrt(np.dot(self.q, self.q))
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])

    @property
    def inverse(self):
        return Quaternion(self.q * np.array([1.0, -1.0, -1.0, -1.0]))


class Box:
    """center, wlh, a rotation matrix; translate / rotate / corners / bottom_corners as the devkit's Box has them."""

    def __init__(self, center, size, orientation, label, token):
        self.center, self.wlh, self.rot = np.array(center, dtype=np.float64), np.array(size, dtype=np.float64), orientation.rotation_matrix
        self.label, self.token, self.name = label, token, "stand-in"

    def translate(self, x):
        self.center = self.center + x

    def rotate(self, quaternion):
        self.center = np.dot(quaternion.rotation_matrix, self.center)
        self.rot = np.dot(quaternion.rotation_matrix, self.rot)

    def corners(self, wlh_factor=1.0):
        w, l, h = self.wlh * wlh_factor
        x = l / 2 * np.array([1, 1, 1, 1, -1, -1, -1, -1])
        y = w / 2 * np.array([1, -1, -1, 1, 1, -1, -1, 1])
        z = h / 2 * np.array([1, 1, -1, -1, 1, 1, -1, -1])
        c = np.dot(self.rot, np.vstack((x, y, z)))
        return c + self.center.reshape(3, 1)

    def bottom_corners(self):
        return self.corners()[:, [2, 3, 7, 6]]


class _Cloud:
    def __init__(self, points):
        self.points = points


class _DevkitRadarPointCloud:
    store = {}

    @staticmethod
    def nbr_dims():
        return 18

    @classmethod
    def from_file_multisweep(cls, nusc, sample, chan, ref_chan, nsweeps, min_distance):
        block = cls.store[sample["data"][chan]]
        return _Cloud(block[:18].copy()), block[18:19].copy()


class _Dataset:
    def __init__(self, *a, **k):
        pass


for name in (P, P + ".utils", P + ".preprocessor", P + ".preprocessor.nuscenes", P + ".graph_constructor"):
    m = types.ModuleType(name); m.__path__ = []; sys.modules[name] = m
for name in ("matplotlib", "matplotlib.pyplot", P + ".preprocessor.configs", P + ".graph_constructor.graph",
             P + ".utils.radar_scenes_properties", P + ".utils.math"):
    sys.modules[name] = MagicMock()
nusc_pkg, nusc_mod = types.ModuleType("nuscenes"), types.ModuleType("nuscenes.nuscenes")
nusc_mod.RadarPointCloud, nusc_mod.Box, nusc_mod.NuScenes = _DevkitRadarPointCloud, Box, MagicMock()
nusc_pkg.nuscenes = nusc_mod
pyq, pyq_q = types.ModuleType("pyquaternion"), types.ModuleType("pyquaternion.quaternion")
pyq_q.Quaternion = Quaternion
tg, tg_data = types.ModuleType("torch_geometric"), types.ModuleType("torch_geometric.data")
tg_data.Data, tg_data.Dataset = MagicMock(), _Dataset
for name, mod in (("nuscenes", nusc_pkg), ("nuscenes.nuscenes", nusc_mod), ("pyquaternion", pyq), ("pyquaternion.quaternion", pyq_q),
                  ("torch_geometric", tg), ("torch_geometric.data", tg_data)):
    sys.modules[name] = mod


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    return mod


BB = load(P + ".preprocessor.bounding_box", R + "/preprocessor/bounding_box.py")
load(P + ".preprocessor.radar_point_cloud", R + "/preprocessor/radar_point_cloud.py")
load(P + ".preprocessor.nuscenes.splits", R + "/preprocessor/nuscenes/splits.py")
CFG = load(P + ".preprocessor.nuscenes.configs", R + "/preprocessor/nuscenes/configs.py")
U = load(P + ".preprocessor.nuscenes.utils", R + "/preprocessor/nuscenes/utils.py")
sys.modules[P + ".preprocessor.nuscenes"].utils = U
C = load(P + ".preprocessor.nuscenes.conversion", R + "/preprocessor/nuscenes/conversion.py")
sys.modules[P + ".preprocessor.nuscenes"].conversion = C
D = load(P + ".preprocessor.nuscenes.dataset_creation", R + "/preprocessor/nuscenes/dataset_creation.py")


# ------------------------------------------------------------------------------------------------ the mocked nusc
class Nusc:
    """Serves one batch: tables keyed by the tokens this file makes up."""

    def __init__(self, inp):
        self.inp, self.tables = inp, {"sample_data": {}, "calibrated_sensor": {}, "ego_pose": {}, "sample_annotation": {}}
        for c in range(len(inp["chunk_sample"])):
            self.tables["sample_data"][f"sd{c}"] = {"calibrated_sensor_token": f"cs{c}"}
            self.tables["calibrated_sensor"][f"cs{c}"] = {"rotation": inp["chunk_rotation"][c].tolist(),
                                                          "translation": inp["chunk_translation"][c].tolist()}
            _DevkitRadarPointCloud.store[f"sd{c}"] = inp["points"][:, inp["chunk_ptr"][c]:inp["chunk_ptr"][c + 1]]
        for s in range(len(inp["box_ptr"]) - 1):
            self.tables["sample_data"][f"lidar{s}"] = {"ego_pose_token": f"ego{s}"}
            self.tables["ego_pose"][f"ego{s}"] = {"translation": inp["ego_translation"][s].tolist(), "rotation": inp["ego_rotation"][s].tolist()}
        for m in range(len(inp["box_label"])):
            n = int(inp["box_points"][m])
            self.tables["sample_annotation"][m] = {"num_lidar_pts": n // 2, "num_radar_pts": n - n // 2}

    def get(self, table, token):
        return self.tables[table][token]

    def get_boxes(self, token):
        s, inp = int(token[5:]), self.inp
        return [Box(inp["box_center"][m], inp["box_size"][m], Quaternion(inp["box_rotation"][m]), int(inp["box_label"][m]), m)
                for m in range(inp["box_ptr"][s], inp["box_ptr"][s + 1])]


def dataset(crop, xlim, ylim, factor, offset):
    """The reference's dataset object without its constructor (which reads the dataset from disk)."""
    ds = object.__new__(D.NuScenesGraphDataset)
    ds.dataset_config = CFG.NuScenesDatasetConfiguration(nsweeps=3, crop_point_cloud=crop, crop_settings={"x": xlim, "y": ylim},
                                                         wlh_factor=factor, wlh_offset=offset)
    ds.nsweeps, ds.wlh_factor, ds.wlh_offset = 3, factor, offset
    # the class-name table is out of scope: the boxes carry integer labels already
    ds.get_bounding_boxes = lambda nusc, sample, sensor: nusc.get_boxes(sample["data"][sensor])
    return ds


def case(name, seed, shapes, crop, xlim, ylim, factor, offset):
    inp, tries = O.draw_admissible(seed, shapes, crop, xlim, ylim, factor, offset)
    nusc = Nusc(inp)
    ds = dataset(crop, xlim, ylim, factor, offset)
    cropped, labels, kept, kept_ptr, center, bottom, rect, frame_ptr = [], [], [], [0], [], [], [], [0]
    targets = {mode: [] for mode in O.MODES}
    for s in range(len(inp["box_ptr"]) - 1):
        chunks = np.nonzero(inp["chunk_sample"] == s)[0]
        sample = {"data": {**{f"RADAR{c}": f"sd{c}" for c in chunks}, "LIDAR_TOP": f"lidar{s}"}}
        points = np.empty(shape=(19, 0))
        for c in chunks:                                       # dataset_creation.py:325-330, in the chunk list's order
            points = np.append(points, ds.get_sensor_points(nusc, sample, f"RADAR{c}"), axis=1)
        if crop:
            points = ds.crop_point_cloud(points)
        lab, boxes = ds.get_labels(nusc, sample, sensor="LIDAR_TOP", points=points)
        cloud = C.convert_point_cloud(points, lab)
        for mode in O.MODES:
            ds.dataset_config.bb_invariance = mode
            targets[mode].append(C.convert_bounding_boxes(ds.dataset_config, cloud, boxes, wlh_factor=factor, wlh_offset=offset))
        cropped.append(points)
        labels.append(lab)
        frame_ptr.append(frame_ptr[-1] + points.shape[1])
        kept += [b.token for b in boxes]
        kept_ptr.append(len(kept))
        for b in boxes:
            center.append(b.center)
            bottom.append(b.bottom_corners())
            rel = BB.BoundingBox(b.bottom_corners()[:2, :].T, False).get_relative_bounding_box(0.0, 0.0)
            rect.append([rel.x_center, rel.y_center, rel.l, rel.w, rel.theta])
    margins = O.admissibility(inp, crop, xlim, ylim, factor, offset)
    assert all((margins[k] >= bar).all() for k, bar in O.ADMISSIBLE.items())
    np.savez_compressed(
        os.path.join(HERE, f"nuscenes_{name}.npz"), **inp, seed=seed, crop=crop, xlim=xlim, ylim=ylim, wlh_factor=factor, wlh_offset=offset,
        threshold=np.array([O.ADMISSIBLE[k] for k in sorted(O.ADMISSIBLE)]), ref_points=np.concatenate(cropped, axis=1),
        ref_frame_ptr=np.asarray(frame_ptr, dtype=np.int64), ref_labels=np.concatenate(labels).astype(np.int64),
        ref_kept=np.asarray(kept, dtype=np.int64), ref_kept_ptr=np.asarray(kept_ptr, dtype=np.int64),
        ref_center=np.reshape(center, (-1, 3)), ref_bottom=np.reshape(bottom, (-1, 3, 4)), ref_rect=np.reshape(rect, (-1, 5)),
        **{"ref_boxes_" + mode: np.concatenate(targets[mode]) for mode in O.MODES}, **{"margin_" + k: v for k, v in margins.items()})
    lab = np.concatenate(labels)
    print(name, "seed", seed, "tries", tries, "rows", inp["points"].shape[1], "kept rows", frame_ptr, "boxes", inp["box_ptr"].tolist(),
          "kept boxes", kept_ptr, "labelled", int((lab > 0).sum()), {k: float(v.min()) for k, v in margins.items()})


def time_reference(name, n_samples=64, mode="en"):
    """Seconds the reference's own loops take for n_samples fixture-shaped samples (the fixture's three, repeated): only the part
    that runs here -- get_sensor_points, the crop, get_labels, convert_point_cloud, convert_bounding_boxes; no graph build, no
    torch_geometric Data, no file reading."""
    import time
    g = np.load(os.path.join(HERE, f"nuscenes_{name}.npz"))
    inp = O.take_samples({k: g[k] for k in O.INPUT_KEYS}, [s % 3 for s in range(n_samples)])
    nusc, factor, offset = Nusc(inp), float(g["wlh_factor"]), float(g["wlh_offset"])
    ds = dataset(bool(g["crop"]), float(g["xlim"]), float(g["ylim"]), factor, offset)
    ds.dataset_config.bb_invariance = mode
    t = time.perf_counter()
    for s in range(n_samples):
        chunks = np.nonzero(inp["chunk_sample"] == s)[0]
        sample = {"data": {**{f"RADAR{c}": f"sd{c}" for c in chunks}, "LIDAR_TOP": f"lidar{s}"}}
        points = np.empty(shape=(19, 0))
        for c in chunks:
            points = np.append(points, ds.get_sensor_points(nusc, sample, f"RADAR{c}"), axis=1)
        points = ds.crop_point_cloud(points)
        lab, boxes = ds.get_labels(nusc, sample, sensor="LIDAR_TOP", points=points)
        C.convert_bounding_boxes(ds.dataset_config, C.convert_point_cloud(points, lab), boxes, wlh_factor=factor, wlh_offset=offset)
    return time.perf_counter() - t


if __name__ == "__main__":
    if "--time" in sys.argv:
        print("reference loops, 64 samples shaped like nuscenes_inflated, en:", round(time_reference("inflated") * 1e3, 1), "ms")
        sys.exit(0)
    # three samples per file: (rows, boxes, empty chunk); the second has its FIRST chunk empty, the third no boxes at all
    shapes = [(150, 40, None), (200, 70, 0), (120, 0, 2)]
    case("plain", 21, shapes, True, 40.0, 30.0, 1.0, 0.0)
    case("inflated", 43, shapes, True, 40.0, 30.0, 1.1, 0.5)
