"""Inputs shared by tests/test_nuscenes_eval_oracle.py and tests/test_gpu_nuscenes_eval.py: box dicts in the layout of
tests/nuscenes_eval_oracle.py (numpy, host), a seeded scene generator, and the adapters to the device types."""
from __future__ import annotations

import math

import numpy as np

import nuscenes_eval_oracle as oracle

N_ATTRIBUTES = 8


def yaw_quat(yaw: float, roll: float = 0.0, pitch: float = 0.0) -> np.ndarray:
    """(w, x, y, z) of the rotation yaw (about z) after pitch (about y) after roll (about x)."""
    cy, sy, cp, sp, cr, sr = (math.cos(yaw / 2), math.sin(yaw / 2), math.cos(pitch / 2), math.sin(pitch / 2), math.cos(roll / 2),
                              math.sin(roll / 2))
    return np.array([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy])


def boxes(translation, size, rotation, velocity, name, attribute, ptr, **extra) -> dict:
    n = len(name)
    out = {"translation": np.asarray(translation, dtype=np.float64).reshape(n, 3), "size": np.asarray(size, dtype=np.float64).reshape(n, 3),
           "rotation": np.asarray(rotation, dtype=np.float64).reshape(n, 4), "velocity": np.asarray(velocity, dtype=np.float64).reshape(n, 2),
           "name": np.asarray(name, dtype=np.int32), "attribute": np.asarray(attribute, dtype=np.int32),
           "ptr": np.asarray(ptr, dtype=np.int64)}
    out.update(extra)
    return out


def simple(names, xy, ptr=None, ego=(0.0, 0.0, 0.0), score=None, yaw=None, attribute=None, num_pts=None, size=None, velocity=None) -> dict:
    """Boxes of the given class names at the given (x, y), z = 0, size (2, 4, 1.5), yaw 0, velocity 0, the class's constant
    attribute; ``score`` makes them predictions, otherwise ground truth (num_pts 1) with ``ego_translation`` per sample."""
    n = len(names)
    ptr = [0, n] if ptr is None else list(ptr)
    codes = [oracle.code(nm) if isinstance(nm, str) else int(nm) for nm in names]
    attr = [oracle.PRED_ATTRIBUTE.get(oracle.LABEL_NAMES[c], -1) if 0 <= c < 11 else -1 for c in codes] if attribute is None else attribute
    rot = [yaw_quat(0.0 if yaw is None else yaw[i]) for i in range(n)]
    out = boxes([[float(p[0]), float(p[1]), 0.0] for p in xy], [[2.0, 4.0, 1.5]] * n if size is None else size, rot,
                np.zeros((n, 2)) if velocity is None else velocity, codes, attr, ptr)
    if score is not None:
        out["score"] = np.asarray(score, dtype=np.float64)
    else:
        out["num_pts"] = np.ones(n, dtype=np.int32) if num_pts is None else np.asarray(num_pts, dtype=np.int32)
        s = len(ptr) - 1
        out["ego_translation"] = np.tile(np.asarray(ego, dtype=np.float64), (s, 1)) if np.ndim(ego) == 1 else np.asarray(ego, dtype=np.float64)
    return out


def scene(seed: int, n_samples: int = 40, max_boxes: int = 60):
    """Seeded ground truth and predictions: ten classes and some boxes without one, boxes beyond the class ranges, boxes without
    points, NaN velocities, '' attributes, bike racks, predictions near the ground truth and false positives, repeated scores."""
    rng = np.random.default_rng(seed)
    g = {k: [] for k in ("translation", "size", "rotation", "velocity", "name", "attribute", "num_pts")}
    p = {k: [] for k in ("translation", "size", "rotation", "velocity", "name", "attribute", "score")}
    racks = {"center": [], "size": [], "rotation": []}
    g_ptr, p_ptr, r_ptr, ego = [0], [0], [0], []
    for s in range(n_samples):
        e = np.array([600.0 + rng.uniform(-50, 50), 1600.0 + rng.uniform(-50, 50), rng.uniform(-1, 1)])
        ego.append(e)
        n_gt = 0 if s % 9 == 4 else int(rng.integers(1, max_boxes + 1))
        for _ in range(n_gt):
            c = int(rng.integers(1, 11)) if rng.random() > 0.05 else -1
            r, a = rng.uniform(0, 58), rng.uniform(-math.pi, math.pi)
            t = e + np.array([r * math.cos(a), r * math.sin(a), rng.uniform(0, 2)])
            size = rng.uniform(0.4, 5.0, 3)
            yaw = rng.uniform(-math.pi, math.pi)
            g["translation"].append(t)
            g["size"].append(size)
            g["rotation"].append(yaw_quat(yaw, rng.normal(0, 0.02), rng.normal(0, 0.02)) * rng.uniform(0.5, 2.0))
            g["velocity"].append([np.nan, np.nan] if rng.random() < 0.1 else rng.normal(0, 3, 2))
            g["name"].append(c)
            g["attribute"].append(-1 if rng.random() < 0.2 else int(rng.integers(0, N_ATTRIBUTES)))
            g["num_pts"].append(int(rng.integers(0, 6)))
            if c in (oracle.code('bicycle'), oracle.code('motorcycle')) and rng.random() < 0.3:
                racks["center"].append(t + np.array([rng.normal(0, 1.0), rng.normal(0, 1.0), 0.0]))
                racks["size"].append([3.0, 6.0, 8.0])
                racks["rotation"].append(yaw_quat(rng.uniform(-math.pi, math.pi)))
            if c > 0 and rng.random() < 0.7:
                pyaw = yaw + rng.normal(0, 0.4) + (math.pi if rng.random() < 0.2 else 0.0)
                p["translation"].append(t + np.array([rng.normal(0, 0.8), rng.normal(0, 0.8), 0.1]))
                p["size"].append(size * rng.uniform(0.8, 1.25, 3))
                p["rotation"].append(yaw_quat(pyaw))
                p["name"].append(c if rng.random() > 0.1 else int(rng.integers(1, 11)))
                p["score"].append(round(float(rng.uniform(0.05, 1.0)), 2) if rng.random() < 0.5 else float(rng.uniform(0.05, 1.0)))
        for _ in range(int(rng.integers(0, 8)) if s % 9 != 7 else 0):
            r, a = rng.uniform(0, 58), rng.uniform(-math.pi, math.pi)
            p["translation"].append(e + np.array([r * math.cos(a), r * math.sin(a), 1.0]))
            p["size"].append(rng.uniform(0.4, 5.0, 3))
            p["rotation"].append(yaw_quat(rng.uniform(-math.pi, math.pi)))
            p["name"].append(int(rng.integers(1, 11)))
            p["score"].append(round(float(rng.uniform(0.05, 0.6)), 2))
        g_ptr.append(len(g["name"]))
        p_ptr.append(len(p["name"]))
        r_ptr.append(len(racks["center"]))
    p["attribute"] = [oracle.PRED_ATTRIBUTE[oracle.LABEL_NAMES[c]] for c in p["name"]]
    p["velocity"] = np.zeros((len(p["name"]), 2))
    gt = boxes(g["translation"], g["size"], g["rotation"], g["velocity"], g["name"], g["attribute"], g_ptr,
               num_pts=np.asarray(g["num_pts"], dtype=np.int32), ego_translation=np.asarray(ego),
               racks=(np.asarray(racks["center"], dtype=np.float64).reshape(-1, 3), np.asarray(racks["size"], dtype=np.float64).reshape(-1, 3),
                      np.asarray(racks["rotation"], dtype=np.float64).reshape(-1, 4), np.asarray(r_ptr, dtype=np.int64)))
    pred = boxes(p["translation"], p["size"], p["rotation"], p["velocity"], p["name"], p["attribute"], p_ptr,
                 score=np.asarray(p["score"], dtype=np.float64))
    return pred, gt


def smallest_margins(pred: dict, gt: dict):
    """(smallest |centre distance - threshold| over all pairs of one sample, smallest |ego distance - class range| over all boxes)."""
    d_margin, r_margin = np.inf, np.inf
    for s in range(len(gt["ptr"]) - 1):
        e = gt["ego_translation"][s]
        pa, pb, ga, gb = int(pred["ptr"][s]), int(pred["ptr"][s + 1]), int(gt["ptr"][s]), int(gt["ptr"][s + 1])
        for b, lo, hi in ((pred, pa, pb), (gt, ga, gb)):
            for i in range(lo, hi):
                if 1 <= b["name"][i] <= 10:
                    d = math.hypot(b["translation"][i][0] - e[0], b["translation"][i][1] - e[1])
                    r_margin = min(r_margin, abs(d - oracle.CLASS_RANGE[oracle.LABEL_NAMES[int(b["name"][i])]]))
        if pb > pa and gb > ga:
            d = np.hypot(pred["translation"][pa:pb, None, 0] - gt["translation"][None, ga:gb, 0],
                         pred["translation"][pa:pb, None, 1] - gt["translation"][None, ga:gb, 1])
            for th in oracle.DIST_THS:
                d_margin = min(d_margin, float(np.abs(d - th).min()))
    return d_margin, r_margin


def device_predictions(pred: dict):
    """The oracle's prediction dict as radargnn_amd.nuscenes_eval.DetectionBoxes on the device."""
    import torch
    from radargnn_amd.nuscenes_eval import DetectionBoxes
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    return DetectionBoxes(up(pred["translation"], torch.float64), up(pred["size"], torch.float64), up(pred["rotation"], torch.float64),
                          up(pred["velocity"], torch.float64), up(pred["name"], torch.int32), up(pred["attribute"], torch.int32),
                          up(pred["score"], torch.float64), up(pred["ptr"], torch.int64))


def device_ground_truth(gt: dict):
    from radargnn_amd.nuscenes_eval import DetectionGroundTruth
    racks = gt.get("racks")
    extra = {} if racks is None else {"rack_center": racks[0], "rack_size": racks[1], "rack_rotation": racks[2], "rack_ptr": racks[3]}
    return DetectionGroundTruth(gt["translation"], gt["size"], gt["rotation"], gt["velocity"], gt["name"], gt["attribute"],
                                gt["num_pts"], gt["ptr"], gt["ego_translation"], **extra)
