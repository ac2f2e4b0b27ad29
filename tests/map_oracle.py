"""numpy restatement of the reference's evaluation metrics, for the cases the committed fixtures do not cover and as the host-side
baseline of the device path: the greedy matching and the recall / precision tables of the vendored ``MeanAveragePrecision``
(postprocessor/torchmetrics_mean_ap.py:505-551, 612-747, 898-1030; area range "all" only), ``torchvision.ops.box_iou``'s formula
(never executed against torchvision; held to a float64 evaluation of the same geometry), and the confusion matrix / F1 of
``SegmentationMetrics`` (postprocessor/metrics.py:136-196).
Checked against the reference-generated tests/golden/eval_map_*.npz and against scikit-learn by tests/test_map_oracle.py.

The reference orders equal scores with an unstable torch.sort.  This project decides: the order of scores is that of
``torch.sort(scores, descending=True, stable=True)`` -- NaN first, -0.0 and 0.0 tie, equal scores (NaNs among themselves too) by
ascending position -- here and in the kernels; tests/test_map_oracle.py holds ``order_desc`` to it."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

EPS32 = np.float32(2.220446049250313e-16)
MAX_DETS = (1, 10, 100)


def rec_thresholds() -> np.ndarray:
    """The reference's recall thresholds: torch.linspace(0.0, 1.0, 101), float32."""
    import torch
    return torch.linspace(0.0, 1.0, 101).numpy()


def order_desc(scores: np.ndarray) -> np.ndarray:
    """Positions by descending score as ``torch.sort(scores, descending=True, stable=True)`` orders them: NaN first, -0.0 and 0.0
    tie, ties (the NaNs too) by ascending position."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    nan = np.isnan(s)
    rest = np.argsort(np.where(nan, 0.0, -s), kind="stable")
    return np.concatenate((np.nonzero(nan)[0], rest[~nan[rest]]))


def box_iou(bp: np.ndarray, bg: np.ndarray) -> np.ndarray:
    """float32 [P, G] of [x_min, y_min, x_max, y_max] float32 boxes, every operation rounded to float32."""
    a, b = np.asarray(bp, dtype=np.float32).reshape(-1, 1, 4), np.asarray(bg, dtype=np.float32).reshape(1, -1, 4)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
        area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
        w = np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0])
        h = np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1])
        inter = np.maximum(w, np.float32(0)) * np.maximum(h, np.float32(0))
        return (inter / ((area_a + area_b) - inter)).astype(np.float32)


def box_iou_float64(bp: np.ndarray, bg: np.ndarray) -> np.ndarray:
    """The same geometry from the same float32 corners, every operation in float64: what ``box_iou`` is judged by."""
    a, b = np.asarray(bp, dtype=np.float64).reshape(-1, 1, 4), np.asarray(bg, dtype=np.float64).reshape(1, -1, 4)
    area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    w = np.clip(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), 0.0, None)
    h = np.clip(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), 0.0, None)
    return w * h / (area_a + area_b - w * h)


def well_conditioned_boxes(rng: np.random.Generator, n: int) -> np.ndarray:
    """float32 [n, 4] boxes with centres in [-8, 8]^2 and sides in [0.5, 10]: more than a fifth of all pairs overlap."""
    centre, side = rng.uniform(-8.0, 8.0, size=(n, 2)), rng.uniform(0.5, 10.0, size=(n, 2))
    return np.concatenate((centre - side / 2, centre + side / 2), axis=1).astype(np.float32)


def match_frame(iou: np.ndarray, det_labels, det_scores, gt_labels, classes: Sequence[int], thresholds: Sequence[float],
                max_det: int = 100):
    """One frame: iou [P, G] (float64 point IoU or float32 box IoU) -> (rank int32 [P], matched uint8 [T, P])."""
    det_labels, gt_labels = np.asarray(det_labels).reshape(-1), np.asarray(gt_labels).reshape(-1)
    det_scores = np.asarray(det_scores, dtype=np.float32).reshape(-1)
    n, t_count = len(det_labels), len(thresholds)
    rank = np.full(n, -1, dtype=np.int32)
    matched = np.zeros((t_count, n), dtype=np.uint8)
    iou = np.asarray(iou).reshape(n, len(gt_labels))
    for c in classes:
        dets = np.nonzero(det_labels == c)[0]
        if len(dets) == 0:
            continue
        dets = dets[order_desc(det_scores[dets])]
        rank[dets[:max_det]] = np.arange(min(len(dets), max_det), dtype=np.int32)
        dets = dets[:max_det]
        gts = np.nonzero(gt_labels == c)[0]
        if len(gts) == 0:
            continue
        for ti, t in enumerate(thresholds):
            thr = np.float32(t) if iou.dtype == np.float32 else float(t)
            used = np.zeros(len(gts), dtype=bool)
            for d in dets:
                row = iou[d, gts]
                vals = np.where(used, row.dtype.type(0), row)
                if np.isnan(row).any():
                    continue
                m = int(np.argmax(vals))
                if vals[m] > thr:
                    used[m] = True
                    matched[ti, d] = 1
    return rank, matched


def match(ious: List[np.ndarray], det_labels: List, det_scores: List, gt_labels: List, classes, thresholds, max_det: int = 100):
    """All frames -> (rank int32 [n_pred], matched uint8 [T, n_pred]) packed in frame order."""
    ranks, flags = [], []
    for f in range(len(det_labels)):
        r, m = match_frame(ious[f], det_labels[f], det_scores[f], gt_labels[f], classes, thresholds, max_det)
        ranks.append(r)
        flags.append(m)
    if not ranks:
        return np.zeros(0, dtype=np.int32), np.zeros((len(thresholds), 0), dtype=np.uint8)
    return np.concatenate(ranks), np.concatenate(flags, axis=1)


def envelope(pr: np.ndarray) -> np.ndarray:
    """The precision made non-increasing: the running maximum from the right."""
    return np.maximum.accumulate(pr[::-1])[::-1] if len(pr) else pr


def curves(det_labels, det_scores, rank, matched, gt_labels, classes, max_dets: Sequence[int] = MAX_DETS,
           rec: Optional[np.ndarray] = None):
    """Packed detections of all frames -> (precision f32 [T, R, K, M], scores f32 [T, R, K, M], recall f32 [T, K, M])."""
    rec = rec_thresholds() if rec is None else np.asarray(rec, dtype=np.float32)
    det_labels, gt_labels = np.asarray(det_labels).reshape(-1), np.asarray(gt_labels).reshape(-1)
    det_scores = np.asarray(det_scores, dtype=np.float32).reshape(-1)
    t_count, k_count, r_count = matched.shape[0], len(classes), len(rec)
    precision = -np.ones((t_count, r_count, k_count, len(max_dets)), dtype=np.float32)
    scores = -np.ones_like(precision)
    recall = -np.ones((t_count, k_count, len(max_dets)), dtype=np.float32)
    order = order_desc(det_scores)
    for ki, c in enumerate(classes):
        npig = int((gt_labels == c).sum())
        if npig == 0:
            continue
        for mi, max_det in enumerate(max_dets):
            sel = order[(det_labels[order] == c) & (rank[order] >= 0) & (rank[order] < max_det)]
            nd = len(sel)
            for ti in range(t_count):
                tps = matched[ti, sel].astype(bool)
                tp = np.cumsum(tps).astype(np.float32)
                fp = np.cumsum(~tps).astype(np.float32)
                rc = tp / np.float32(npig)
                pr = envelope(tp / ((fp + tp) + EPS32))
                recall[ti, ki, mi] = rc[-1] if nd else 0
                inds = np.searchsorted(rc, rec, side="left")
                ok = inds < nd
                if not ok.all():
                    ok[np.argmin(ok):] = False
                prec, score = np.zeros(r_count, dtype=np.float32), np.zeros(r_count, dtype=np.float32)
                prec[ok] = pr[inds[ok]]
                score[ok] = det_scores[sel][inds[ok]]
                precision[ti, :, ki, mi] = prec
                scores[ti, :, ki, mi] = score
    return precision, scores, recall


def _mean(a: np.ndarray) -> float:
    a = np.asarray(a, dtype=np.float64)
    a = a[a > -1]
    return float(a.mean()) if a.size else -1.0


def summarize(precision: np.ndarray, recall: np.ndarray, thresholds: Sequence[float], max_dets: Sequence[int] = MAX_DETS) -> Dict:
    """_summarize / compute (torchmetrics_mean_ap.py:749-794, 975-1030) for the area range "all", means in float64."""
    last = len(max_dets) - 1
    res = {"map": _mean(precision[:, :, :, last])}
    for name, value in (("map_50", 0.5), ("map_75", 0.75)):
        res[name] = _mean(precision[list(thresholds).index(value), :, :, last]) if value in list(thresholds) else -1.0
    for mi, m in enumerate(max_dets):
        res[f"mar_{m}"] = _mean(recall[:, :, mi])
    res["map_per_class"] = np.array([_mean(precision[:, :, k, last]) for k in range(precision.shape[2])])
    res[f"mar_{max_dets[last]}_per_class"] = np.array([_mean(recall[:, k, last]) for k in range(recall.shape[1])])
    return res


def get_classes(det_labels: List, gt_labels: List) -> List[int]:
    parts = [np.asarray(l).reshape(-1) for l in list(det_labels) + list(gt_labels)]
    return sorted(set(int(v) for v in np.concatenate(parts))) if parts else []


def mean_ap(ious: List[np.ndarray], det_labels: List, det_scores: List, gt_labels: List, thresholds: Sequence[float]) -> Dict:
    """Everything after the IoU matrices, as ``MeanAveragePrecision.compute`` returns it (plus the tables and the match flags)."""
    classes = get_classes(det_labels, gt_labels)
    rank, matched = match(ious, det_labels, det_scores, gt_labels, classes, thresholds, MAX_DETS[-1])
    cat = lambda parts, dt: np.concatenate([np.asarray(p, dtype=dt).reshape(-1) for p in parts]) if parts else np.zeros(0, dtype=dt)
    precision, scores, recall = curves(cat(det_labels, np.int64), cat(det_scores, np.float32), rank, matched, cat(gt_labels, np.int64),
                                       classes)
    res = summarize(precision, recall, thresholds)
    res.update(classes=classes, precision=precision, recall=recall, scores=scores, rank=rank, matched=matched)
    return res


# ---- segmentation: confusion matrix and F1 (sklearn's definitions for labels = range(K)) -------------------------------
SEG_CLASSES = 7


def segmentation_labels(n: int):
    """Deterministic node labels (float64) for the segmentation fixture: values -1 .. 8 for SEG_CLASSES = 7 (so some lie outside
    0 .. K-1), class 4 never occurs, predictions agree with the truth about two times in three, and every fifth prediction carries a
    fraction that astype(int) truncates."""
    i = np.arange(n, dtype=np.int64)
    y_true = (i * 7919 + i // 13) % 10 - 1
    y_pred = np.where(i % 3 != 0, y_true, (i * 104729 + i // 7) % 10 - 1)
    y_true = np.where(y_true == 4, 5, y_true).astype(np.float64)
    y_pred = np.where(y_pred == 4, 3, y_pred).astype(np.float64)
    y_pred = y_pred + np.where(i % 5 == 0, 0.25, 0.0)
    return y_true, y_pred


def extended_confusion(y_true, y_pred, k: int) -> np.ndarray:
    """int64 [K + 1, K + 1]: labels truncated like astype(int); row / column K collects the labels outside 0 .. K-1, which
    sklearn's f1_score still counts as false negatives / positives of the classes they were confused with."""
    yt, yp = np.trunc(np.asarray(y_true, dtype=np.float64).reshape(-1)), np.trunc(np.asarray(y_pred, dtype=np.float64).reshape(-1))
    if np.isnan(yt).any() or np.isnan(yp).any():
        raise ValueError("Input contains NaN.")
    yt = np.where((yt >= 0) & (yt < k), yt, k).astype(np.int64)
    yp = np.where((yp >= 0) & (yp < k), yp, k).astype(np.int64)
    cm = np.zeros((k + 1, k + 1), dtype=np.int64)
    np.add.at(cm, (yt, yp), 1)
    return cm


def confusion_matrix(y_true, y_pred, k: int) -> np.ndarray:
    return extended_confusion(y_true, y_pred, k)[:k, :k]


def _ratio(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.where(den == 0, 0.0, num / np.where(den == 0, 1.0, den))


def f1_from_confusion(ext: np.ndarray, average: Optional[str]):
    """F1 of the classes 0 .. K-1 from the extended matrix: 2 tp / (2 tp + fp + fn), 0 where that denominator is 0."""
    k = ext.shape[0] - 1
    tp = np.diag(ext)[:k].astype(np.float64)
    fp = ext[:, :k].sum(axis=0) - tp
    fn = ext[:k, :].sum(axis=1) - tp
    if average == "micro":
        return float(_ratio(2 * tp.sum(), 2 * tp.sum() + fp.sum() + fn.sum()))
    f = _ratio(2 * tp, 2 * tp + fp + fn)
    if average is None:
        return f
    if average == "macro":
        return float(f.mean()) if k else 0.0
    if average == "weighted":
        support = tp + fn
        return float((f * support).sum() / support.sum()) if support.sum() else 0.0
    raise ValueError(f"average has to be one of (None, 'micro', 'macro', 'weighted'), got {average!r}")


def matrices_per_class(ext: np.ndarray) -> np.ndarray:
    """multilabel_confusion_matrix: int64 [K, 2, 2] = [[tn, fp], [fn, tp]] per class."""
    k = ext.shape[0] - 1
    tp = np.diag(ext)[:k]
    fp = ext[:, :k].sum(axis=0) - tp
    fn = ext[:k, :].sum(axis=1) - tp
    tn = ext.sum() - tp - fp - fn
    return np.stack((tn, fp, fn, tp), axis=1).reshape(k, 2, 2).astype(np.int64)
