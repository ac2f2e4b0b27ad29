"""numpy restatement of the reference's evaluation half, for randomized and adversarial cases the committed fixtures do not
cover: GroundTruthExtractor.get_absolute_object_bounding_boxes / remove_duplicate_boxes (postprocessor/postprocessing.py:
447-575) and point_iou (utils/math.py:61-211).  Checked against the reference-generated tests/golden/eval_*.npz by
tests/test_eval_oracle.py; the box algebra is oracle/postprocess_oracle.py's."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from oracle import postprocess_oracle as O


def ground_truth_boxes(labels: np.ndarray, bb: np.ndarray, pos: np.ndarray, bg_index: int, invariance: str,
                       nn_index: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (corners [M, 4, 2] f64, labels [M, 1] in the input dtype, kept node ids [M]) of one graph: every node whose label
    != bg_index, in node order; the angle is never adapted."""
    labels = np.asarray(labels).reshape(-1)
    kept = np.where(~(labels == bg_index))[0]
    corners = np.zeros((len(kept), 4, 2))
    for r, i in enumerate(kept):
        nn = pos[nn_index[i]] if (invariance == "en" and bb.shape[1] == 5) else None
        corners[r] = O.decode_box(bb[i], pos[i], nn, invariance, False)
    return corners, labels[kept].reshape(-1, 1), kept


def l1_sum(a: np.ndarray, b: np.ndarray) -> float:
    """np.sum(abs(a - b)) of two [4, 2] float64 corner sets, in numpy's pairwise order for 8 contiguous values."""
    d = np.abs(np.asarray(a, dtype=np.float64).reshape(8) - np.asarray(b, dtype=np.float64).reshape(8))
    return ((d[0] + d[1]) + (d[2] + d[3])) + ((d[4] + d[5]) + (d[6] + d[7]))


def boxes_match(a: np.ndarray, b: np.ndarray) -> bool:
    return bool((np.asarray(a) == np.asarray(b)).all()) or l1_sum(a, b) < 0.1


def duplicate_keep(corners: np.ndarray) -> np.ndarray:
    """bool [M]: box j is dropped iff a box i < j (dropped or not) matches it."""
    m = corners.shape[0]
    keep = np.ones(m, dtype=bool)
    for j in range(m):
        for i in range(j):
            if boxes_match(corners[i], corners[j]):
                keep[j] = False
                break
    return keep


def box_corners(box: np.ndarray) -> np.ndarray:
    """get_box_corners (utils/math.py:9-45) of [x, y, l, w, theta deg], in float64."""
    x, y, l, w, theta = (float(v) for v in np.asarray(box, dtype=np.float64))
    return O._rotated_corners(x, y, l, w, theta)


def area_slack(corners: np.ndarray, point) -> float:
    """sum of the four triangle areas - rectangle area (is_point_in_rect, utils/math.py:61-99); inside iff < 1e-6."""
    xP, yP = float(point[0]), float(point[1])
    (xA, yA), (xB, yB), (xC, yC), (xD, yD) = [(float(c[0]), float(c[1])) for c in corners]
    abcd = 0.5 * abs((yA - yC) * (xD - xB) + (yB - yD) * (xA - xC))
    abp = 0.5 * abs(xA * (yB - yP) + xB * (yP - yA) + xP * (yA - yB))
    bcp = 0.5 * abs(xB * (yC - yP) + xC * (yP - yB) + xP * (yB - yC))
    cdp = 0.5 * abs(xC * (yD - yP) + xD * (yP - yC) + xP * (yC - yD))
    dap = 0.5 * abs(xD * (yA - yP) + xA * (yP - yD) + xP * (yD - yA))
    return abp + bcp + cdp + dap - abcd


def inside(box: np.ndarray, points: np.ndarray, aligned: bool) -> np.ndarray:
    """bool [N]: the points of the graph inside one box."""
    points = np.asarray(points, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64)
    if aligned:
        return (points[:, 0] >= box[0]) & (points[:, 0] <= box[2]) & (points[:, 1] >= box[1]) & (points[:, 1] <= box[3])
    c = box_corners(box)
    return np.array([area_slack(c, p) < 1e-6 for p in points], dtype=bool)


def point_iou(boxes_pred: np.ndarray, boxes_gt: np.ndarray, points: np.ndarray, aligned: bool) -> np.ndarray:
    """float64 [P, G]: tp = distinct coordinates inside both boxes, fp / fn = points inside one box minus tp."""
    points = np.asarray(points)
    keys = [(float(x) + 0.0, float(y) + 0.0) for x, y in points]          # + 0.0: -0.0 and 0.0 are one tuple
    a_in = [inside(b, points, aligned) for b in np.asarray(boxes_pred).reshape(-1, 4 if aligned else 5)]
    b_in = [inside(b, points, aligned) for b in np.asarray(boxes_gt).reshape(-1, 4 if aligned else 5)]
    out = np.empty((len(a_in), len(b_in)))
    for i, a in enumerate(a_in):
        sa = {keys[k] for k in np.nonzero(a)[0]}
        for j, b in enumerate(b_in):
            tp = len(sa & {keys[k] for k in np.nonzero(b)[0]})
            fp, fn = int(a.sum()) - tp, int(b.sum()) - tp
            out[i, j] = tp / (tp + fp + fn) if tp + fp + fn != 0 else 0.00001
    return out


def split(packed: np.ndarray, ptr) -> List[np.ndarray]:
    return [packed[ptr[f]:ptr[f + 1]] for f in range(len(ptr) - 1)]
