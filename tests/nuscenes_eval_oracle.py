"""float64 numpy restatement of the nuScenes evaluator, written as the plain loops of the reference and of the nuscenes-devkit:
the submission records (postprocessor/nuscenes/utils.py:11-140,246-309), the devkit's ``add_center_dist`` / ``filter_eval_boxes``,
``accumulate`` with ``center_distance`` / ``scale_iou`` / ``yaw_diff`` / ``cummean``, ``calc_ap`` / ``calc_tp`` and
``DetectionMetrics.serialize`` for the configuration ``detection_cvpr_2019``.  It is the host-side baseline of
radargnn_amd.nuscenes_eval and what tests/test_gpu_nuscenes_eval.py holds the kernels to; tests/test_nuscenes_eval_oracle.py holds
IT to answers derived on paper.  ``np.interp`` and ``np.nancumsum`` are numpy's own.

NOT PINNED BY AN EXECUTED DEVKIT: neither ``nuscenes`` nor ``pyquaternion`` is available where this runs.  Restated conventions:
the rotation matrix of a quaternion is that of the normalised quaternion; pyquaternion's ``yaw_pitch_roll[0]`` is
``atan2(2 (w z - x y), 1 - 2 (y^2 + z^2))``; ``quaternion_yaw`` is the atan2 of the first column of the rotation matrix; predictions
go by ``sorted((score, index))[::-1]``.

Boxes are dicts of arrays packed by ``ptr`` [S + 1]: ``translation`` [N, 3], ``size`` [N, 3] (w, l, h), ``rotation`` [N, 4],
``velocity`` [N, 2], ``name`` (codes into LABEL_NAMES), ``attribute`` (codes, -1 for ''), predictions with ``score``, ground truth
with ``num_pts``, ``ego_translation`` [S, 3] and optionally ``racks`` = (center, size, rotation, ptr)."""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import numpy as np

LABEL_NAMES = ('void', 'barrier', 'bicycle', 'bus', 'car', 'construction_vehicle', 'motorcycle', 'pedestrian', 'traffic_cone',
               'trailer', 'truck')
DETECTION_NAMES = ('car', 'truck', 'bus', 'trailer', 'construction_vehicle', 'pedestrian', 'motorcycle', 'bicycle', 'traffic_cone',
                   'barrier')
HEIGHTS = (1.029, 0.981, 1.283, 3.41, 1.698, 3.05, 1.471, 1.78, 1.067, 4.04, 2.843)
CLASS_RANGE = {'car': 50, 'truck': 50, 'bus': 50, 'trailer': 50, 'construction_vehicle': 50, 'pedestrian': 40, 'motorcycle': 40,
               'bicycle': 40, 'traffic_cone': 30, 'barrier': 30}
DIST_THS = (0.5, 1.0, 2.0, 4.0)
DIST_TH_TP = 2.0
MIN_RECALL = 0.1
MIN_PRECISION = 0.1
MAX_BOXES = 500
MEAN_AP_WEIGHT = 5
TP_METRICS = ('trans_err', 'scale_err', 'orient_err', 'vel_err', 'attr_err')
# the constant attribute of a predicted class, as a code into radargnn_amd.nuscenes_eval.ATTRIBUTE_NAMES (-1: '')
PRED_ATTRIBUTE = {'barrier': -1, 'traffic_cone': -1, 'bicycle': 0, 'motorcycle': 0, 'pedestrian': 2, 'car': 5, 'bus': 5,
                  'construction_vehicle': 5, 'trailer': 5, 'truck': 5}


def code(name: str) -> int:
    return LABEL_NAMES.index(name)


def quat_matrix(q) -> np.ndarray:
    w, x, y, z = (float(v) for v in q)
    n = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


def ego_yaw(q) -> float:
    w, x, y, z = (float(v) for v in q)
    n = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    return math.atan2(2 * (w * z - x * y), 1 - 2 * (y * y + z * z))


def quaternion_yaw(q) -> float:
    R = quat_matrix(q)
    return math.atan2(R[1, 0], R[0, 0])


# ---- 1. submission -----------------------------------------------------------------------------------------------------------
def submission(boxes, labels, box_ptr, ego_translation, ego_rotation):
    """-> translation [M, 3], size [M, 3], rotation [M, 4], yaw [M].  ValueError for label 0 or a label outside the list."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 5)
    m = boxes.shape[0]
    translation, size, rotation, yaw = np.zeros((m, 3)), np.zeros((m, 3)), np.zeros((m, 4)), np.zeros(m)
    for s in range(len(box_ptr) - 1):
        R = quat_matrix(ego_rotation[s])
        yaw_e = ego_yaw(ego_rotation[s])
        for i in range(int(box_ptr[s]), int(box_ptr[s + 1])):
            label = int(labels[i])
            if label < 1 or label >= len(LABEL_NAMES):
                raise ValueError("no detection name")
            h = HEIGHTS[label]
            x, y, l, w, theta = (float(v) for v in boxes[i])
            for r in range(3):
                translation[i, r] = ((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * 0.0) + float(ego_translation[s][r])
            translation[i, 2] += h / 2
            size[i] = (w, l, h)
            angle = float(np.deg2rad(theta)) + yaw_e
            rotation[i] = (math.cos(angle / 2), 0.0, 0.0, math.sin(angle / 2))
            yaw[i] = angle
    return translation, size, rotation, yaw


# ---- 2. filter ---------------------------------------------------------------------------------------------------------------
def point_in_box(center, wlh, q, pt) -> bool:
    R = quat_matrix(q)
    w, l, h = (float(v) for v in wlh)
    corners = []
    for sx, sy, sz in ((1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1)):          # corners 0, 4, 1, 3
        b = (sx * (l / 2), sy * (w / 2), sz * (h / 2))
        corners.append([((R[r, 0] * b[0] + R[r, 1] * b[1]) + R[r, 2] * b[2]) + float(center[r]) for r in range(3)])
    v = [float(pt[r]) - corners[0][r] for r in range(3)]
    for a in (1, 2, 3):
        e = [corners[a][r] - corners[0][r] for r in range(3)]
        ev = (e[0] * v[0] + e[1] * v[1]) + e[2] * v[2]
        ee = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        if not (0.0 <= ev <= ee):
            return False
    return True


def filter_boxes(boxes: dict, ego_translation, class_range: Dict[str, float] = CLASS_RANGE, racks=None, is_gt: bool = False) -> np.ndarray:
    ptr = boxes["ptr"]
    n = int(ptr[-1])
    keep = np.zeros(n, dtype=bool)
    for s in range(len(ptr) - 1):
        for i in range(int(ptr[s]), int(ptr[s + 1])):
            nm = int(boxes["name"][i])
            if nm < 1 or nm >= len(LABEL_NAMES):
                continue
            dx = float(boxes["translation"][i][0]) - float(ego_translation[s][0])
            dy = float(boxes["translation"][i][1]) - float(ego_translation[s][1])
            k = math.sqrt(dx * dx + dy * dy) < class_range[LABEL_NAMES[nm]]
            if is_gt:
                k = k and int(boxes["num_pts"][i]) > 0
            if k and racks is not None and LABEL_NAMES[nm] in ('bicycle', 'motorcycle'):
                for r in range(int(racks[3][s]), int(racks[3][s + 1])):
                    if point_in_box(racks[0][r], racks[1][r], racks[2][r], boxes["translation"][i]):
                        k = False
            keep[i] = k
    return keep


def check_predictions(pred: dict, max_boxes: int = MAX_BOXES) -> None:
    ptr = pred["ptr"]
    if any(int(ptr[s + 1]) - int(ptr[s]) > max_boxes for s in range(len(ptr) - 1)):
        raise ValueError("too many boxes in a sample")
    if np.isnan(np.asarray(pred["score"], dtype=np.float64)).any():
        raise ValueError("NaN score")


# ---- 3. matching -------------------------------------------------------------------------------------------------------------
def score_order(scores, ids) -> list:
    """``ids`` by the devkit's order: sorted((score, index)) reversed."""
    return [i for (_, i) in sorted((float(scores[i]), i) for i in ids)][::-1]


def angle_diff(x: float, y: float, period: float) -> float:
    diff = (x - y + period / 2) % period - period / 2
    if diff > np.pi:
        diff = diff - (2 * np.pi)
    return diff


def match_boxes(pred: dict, gt: dict, keep_p, keep_g, dist_ths: Sequence[float] = DIST_THS, dist_th_tp: float = DIST_TH_TP):
    """-> match int32 [T, M] (ground-truth index or -1), tp_err [5, M] for dist_th_tp (NaN where unmatched)."""
    m, t_n = int(pred["ptr"][-1]), len(dist_ths)
    match = np.full((t_n, m), -1, dtype=np.int32)
    tp_err = np.full((5, m), np.nan)
    sample_of = np.zeros(m, dtype=np.int64)
    for s in range(len(pred["ptr"]) - 1):
        sample_of[int(pred["ptr"][s]):int(pred["ptr"][s + 1])] = s
    for name in DETECTION_NAMES:
        c = code(name)
        ids = [i for i in range(m) if keep_p[i] and int(pred["name"][i]) == c]
        order = score_order(pred["score"], ids)
        for it, th in enumerate(dist_ths):
            taken = set()
            for i in order:
                s = int(sample_of[i])
                min_dist, best = np.inf, None
                for g in range(int(gt["ptr"][s]), int(gt["ptr"][s + 1])):
                    if not keep_g[g] or int(gt["name"][g]) != c or g in taken:
                        continue
                    dx = float(pred["translation"][i][0]) - float(gt["translation"][g][0])
                    dy = float(pred["translation"][i][1]) - float(gt["translation"][g][1])
                    d = math.sqrt(dx * dx + dy * dy)
                    if d < min_dist:
                        min_dist, best = d, g
                if min_dist < th:
                    taken.add(best)
                    match[it, i] = best
                    if th == dist_th_tp:
                        sa, sr = np.asarray(gt["size"][best], dtype=np.float64), np.asarray(pred["size"][i], dtype=np.float64)
                        inter = np.prod(np.minimum(sa, sr))
                        iou = inter / (np.prod(sa) + np.prod(sr) - inter)
                        period = np.pi if name == 'barrier' else 2 * np.pi
                        vx = float(pred["velocity"][i][0]) - float(gt["velocity"][best][0])
                        vy = float(pred["velocity"][i][1]) - float(gt["velocity"][best][1])
                        ga = int(gt["attribute"][best])
                        tp_err[0, i] = min_dist
                        tp_err[1, i] = 1 - iou
                        tp_err[2, i] = abs(angle_diff(quaternion_yaw(gt["rotation"][best]), quaternion_yaw(pred["rotation"][i]), period))
                        tp_err[3, i] = math.sqrt(vx * vx + vy * vy)
                        tp_err[4, i] = np.nan if ga < 0 else 1.0 - float(ga == int(pred["attribute"][i]))
    return match, tp_err


# ---- 4. curves ---------------------------------------------------------------------------------------------------------------
def cummean(x: np.ndarray) -> np.ndarray:
    if sum(np.isnan(x)) == len(x):
        return np.ones(len(x))
    sum_vals = np.nancumsum(x.astype(float))
    count_vals = np.cumsum(~np.isnan(x))
    return np.divide(sum_vals, count_vals, out=np.zeros_like(sum_vals), where=count_vals != 0)


def curves(pred: dict, gt: dict, keep_p, keep_g, match, tp_err, dist_ths: Sequence[float] = DIST_THS, dist_th_tp: float = DIST_TH_TP):
    """-> precision [C, T, 101], confidence [C, T, 101], tp_err_curve [C, 5, 101], classes in the order of DETECTION_NAMES."""
    m = int(pred["ptr"][-1])
    grid = np.linspace(0, 1, 101)
    precision = np.zeros((len(DETECTION_NAMES), len(dist_ths), 101))
    confidence = np.zeros_like(precision)
    tp_curve = np.ones((len(DETECTION_NAMES), 5, 101))
    for ic, name in enumerate(DETECTION_NAMES):
        c = code(name)
        npos = sum(1 for g in range(int(gt["ptr"][-1])) if keep_g[g] and int(gt["name"][g]) == c)
        order = score_order(pred["score"], [i for i in range(m) if keep_p[i] and int(pred["name"][i]) == c])
        for it, th in enumerate(dist_ths):
            if npos == 0:
                continue
            tp, fp, conf = [], [], []
            m_conf, m_err = [], [[] for _ in range(5)]
            for i in order:
                conf.append(float(pred["score"][i]))
                if match[it, i] >= 0:
                    tp.append(1)
                    fp.append(0)
                    m_conf.append(float(pred["score"][i]))
                    for e in range(5):
                        m_err[e].append(tp_err[e, i])
                else:
                    tp.append(0)
                    fp.append(1)
            if len(m_conf) == 0:
                continue
            tp, fp, conf = np.cumsum(tp).astype(float), np.cumsum(fp).astype(float), np.array(conf)
            prec, rec = tp / (fp + tp), tp / float(npos)
            precision[ic, it] = np.interp(grid, rec, prec, right=0)
            confidence[ic, it] = np.interp(grid, rec, conf, right=0)
            if th == dist_th_tp:
                for e in range(5):
                    tmp = cummean(np.array(m_err[e], dtype=np.float64))
                    tp_curve[ic, e] = np.interp(confidence[ic, it][::-1], np.array(m_conf)[::-1], tmp[::-1])[::-1]
    return precision, confidence, tp_curve


# ---- 5. summary --------------------------------------------------------------------------------------------------------------
def calc_ap(precision: np.ndarray, min_recall: float = MIN_RECALL, min_precision: float = MIN_PRECISION) -> float:
    prec = np.copy(precision)
    prec = prec[round(100 * min_recall) + 1:]
    prec -= min_precision
    prec[prec < 0] = 0
    return float(np.mean(prec)) / (1.0 - min_precision)


def calc_tp(confidence: np.ndarray, curve: np.ndarray, min_recall: float = MIN_RECALL) -> float:
    first_ind = round(100 * min_recall) + 1
    non_zero = np.nonzero(confidence)[0]
    last_ind = 0 if len(non_zero) == 0 else non_zero[-1]
    if last_ind < first_ind:
        return 1.0
    return float(np.mean(curve[first_ind: last_ind + 1]))


def summary(precision, confidence, tp_curve, dist_ths: Sequence[float] = DIST_THS, dist_th_tp: float = DIST_TH_TP) -> dict:
    it_tp = list(dist_ths).index(dist_th_tp)
    label_aps, label_tp_errors = {}, {}
    for ic, name in enumerate(DETECTION_NAMES):
        label_aps[name] = {th: calc_ap(precision[ic, it]) for it, th in enumerate(dist_ths)}
        label_tp_errors[name] = {}
        for ie, metric in enumerate(TP_METRICS):
            if name in ['traffic_cone'] and metric in ['attr_err', 'vel_err', 'orient_err']:
                tp = np.nan
            elif name in ['barrier'] and metric in ['attr_err', 'vel_err']:
                tp = np.nan
            else:
                tp = calc_tp(confidence[ic, it_tp], tp_curve[ic, ie])
            label_tp_errors[name][metric] = float(tp)
    mean_dist_aps = {name: float(np.mean(list(d.values()))) for name, d in label_aps.items()}
    mean_ap = float(np.mean(list(mean_dist_aps.values())))
    tp_errors = {metric: float(np.nanmean([label_tp_errors[name][metric] for name in DETECTION_NAMES])) for metric in TP_METRICS}
    tp_scores = {metric: max(0.0, 1.0 - tp_errors[metric]) for metric in TP_METRICS}
    total = float(MEAN_AP_WEIGHT * mean_ap + np.sum(list(tp_scores.values())))
    total = total / float(MEAN_AP_WEIGHT + len(tp_scores.keys()))
    return {"label_aps": label_aps, "mean_dist_aps": mean_dist_aps, "mean_ap": mean_ap, "label_tp_errors": label_tp_errors,
            "tp_errors": tp_errors, "tp_scores": tp_scores, "nd_score": total}


def detection_eval(pred: dict, gt: dict, parts: Optional[dict] = None) -> dict:
    """The whole evaluation -> the summary; ``parts`` (a dict) receives every intermediate result."""
    check_predictions(pred)
    racks = gt.get("racks")
    keep_p = filter_boxes(pred, gt["ego_translation"], racks=racks)
    keep_g = filter_boxes(gt, gt["ego_translation"], racks=racks, is_gt=True)
    match, tp_err = match_boxes(pred, gt, keep_p, keep_g)
    precision, confidence, tp_curve = curves(pred, gt, keep_p, keep_g, match, tp_err)
    if parts is not None:
        parts.update(keep_pred=keep_p, keep_gt=keep_g, match=match, tp_err=tp_err, precision=precision, confidence=confidence,
                     tp_curve=tp_curve)
    return summary(precision, confidence, tp_curve)


def predictions_like(gt: dict, score: float = 0.9) -> dict:
    """Predictions equal to the ground truth: same geometry and velocity, the class's constant attribute, one score."""
    n = int(gt["ptr"][-1])
    return {"translation": np.array(gt["translation"], dtype=np.float64), "size": np.array(gt["size"], dtype=np.float64),
            "rotation": np.array(gt["rotation"], dtype=np.float64), "velocity": np.array(gt["velocity"], dtype=np.float64),
            "name": np.array(gt["name"], dtype=np.int32), "attribute": np.array(gt["attribute"], dtype=np.int32),
            "score": np.full(n, score), "ptr": np.array(gt["ptr"], dtype=np.int64)}
