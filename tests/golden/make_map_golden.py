"""Writes tests/golden/eval_map_*.npz and eval_seg_confusion.npz: inputs and results of the reference's evaluation metrics, produced
by EXECUTING the reference's own code: ``MeanAveragePrecision`` (postprocessor/torchmetrics_mean_ap.py) with ``point_iou`` /
``box_area_rotated`` (utils/math.py) and the ``BoundingBox`` representations (preprocessor/bounding_box.py), loaded by file path,
and scikit-learn's ``confusion_matrix`` / ``f1_score`` / ``multilabel_confusion_matrix`` as ``SegmentationMetrics`` calls them.
Runs only in the build container; the fixtures are committed.

torchmetrics and torchvision are not installed.  This process registers stand-ins of its own: ``torchmetrics.metric.Metric`` (a
class whose ``add_state`` sets the attribute and whose ``device`` is the CPU), the two flags of ``torchmetrics.utilities.imports``,
and ``torchvision.ops.{box_area, box_convert, box_iou}`` (identity for "xyxy"; the documented formula of box_iou in float32 torch
ops).  The box IoU is therefore UNPINNED by an executed torchvision.

numpy here is 2.x: the metric hands ``point_iou`` float32 torch tensors, and the rotated path would build its corners in float32
(NEP 50), up to 0.5 away from the IoUs of the reference's numpy 1.x environment, where the same scalar expressions promote to
float64.  The name ``point_iou`` inside the loaded metric module is therefore replaced by a wrapper that casts boxes and points to
float64 before calling the reference's ``point_iou`` -- the arithmetic rgnn_point_iou is pinned to (see make_eval_golden.py).

Conditions enforced by drawing the case again with the next seed (the count is printed), so that the reference alone is unambiguous:
  - the scores of one class are pairwise distinct over the whole case (the reference's torch.sort leaves ties unpinned);
  - box-IoU cases: no IoU of a same-class pair within 1e-5 of a threshold, and the two largest candidates of a detection differ by
    more than 1e-5 unless bit-equal (float32 IoUs carry about four roundings, 2.4e-7 relative; 1e-5 is forty times that);
  - rotated point IoU: every point whose area-test slack for some box lies within 1e-9 of the 1e-6 bound is dropped;
  - on every curve the reference's iterated precision envelope is bit-equal to the running maximum from the right.

Named cases (CASES below): aligned + point IoU, rotated + point IoU, aligned + box IoU; 35 frames each, among them (SPECIAL_FRAMES)
a frame without detections, one without ground truth, one without either, one with no points, a class only among detections (7), a
class only among ground truth (8), 130 detections of one class in one frame (the max_det cut), two detections competing for one
ground-truth box, one detection with two candidates of equal IoU (copies of one box: "equal_candidates"; two DISTINCT boxes, with
a later detection that overlaps only the first of them, so that its flag tells whether the lowest or the highest position won the
tie: "tied_candidates"), and for the point-IoU cases a point IoU of exactly 3/10 (threshold
0.3) and exactly 1/2 (threshold 0.5).  Every case also runs a second threshold list with T = 3.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

R = "/root/reference/src/gnnradarobjectdetection"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import eval_oracle as E  # noqa: E402
import map_oracle as MO  # noqa: E402

for name in ("gnnradarobjectdetection", "gnnradarobjectdetection.utils", "gnnradarobjectdetection.preprocessor",
             "gnnradarobjectdetection.postprocessor", "torchmetrics", "torchmetrics.utilities", "torchvision"):
    m = types.ModuleType(name); m.__path__ = []; sys.modules[name] = m


class Metric:
    def __init__(self, **kwargs):
        self._defaults = {}
        self.device = torch.device("cpu")

    def add_state(self, name, default, dist_reduce_fx=None):
        self._defaults[name] = default
        setattr(self, name, [] if isinstance(default, list) else default)


def _box_area(b):
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def _box_iou(a, b):
    lt, rb = torch.max(a[:, None, :2], b[None, :, :2]), torch.min(a[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (_box_area(a)[:, None] + _box_area(b)[None, :] - inter)


def _box_convert(boxes, in_fmt, out_fmt):
    assert in_fmt == out_fmt == "xyxy"
    return boxes


mm = types.ModuleType("torchmetrics.metric"); mm.Metric = Metric; sys.modules["torchmetrics.metric"] = mm
mi = types.ModuleType("torchmetrics.utilities.imports"); mi._PYCOCOTOOLS_AVAILABLE = False; mi._TORCHVISION_GREATER_EQUAL_0_8 = True
sys.modules["torchmetrics.utilities.imports"] = mi
tv = types.ModuleType("torchvision.ops"); tv.box_area, tv.box_convert, tv.box_iou = _box_area, _box_convert, _box_iou
sys.modules["torchvision.ops"] = tv


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    return mod


M = load("gnnradarobjectdetection.utils.math", R + "/utils/math.py")
BB = load("gnnradarobjectdetection.preprocessor.bounding_box", R + "/preprocessor/bounding_box.py")
TM = load("gnnradarobjectdetection.postprocessor.torchmetrics_mean_ap", R + "/postprocessor/torchmetrics_mean_ap.py")


def point_iou_f64(boxes_pred, boxes_gt, points, box_aligned):
    return M.point_iou(boxes_pred.double(), boxes_gt.double(), np.asarray(points, dtype=np.float64), box_aligned)


TM.point_iou = point_iou_f64

SLACK_MARGIN = 1e-9
IOU_MARGIN = 1e-5
N_RANDOM = 22
SPECIAL_FRAMES = ("no_detections", "no_ground_truth", "neither", "no_points", "class_only_detected", "class_only_ground_truth",
                  "max_det_cut", "competing_detections", "equal_candidates", "tied_candidates", "iou_3_of_10", "iou_1_of_2", "plain")
CASES = {"aligned_point": (True, True, 21), "rotated_point": (False, True, 22), "aligned_box": (True, False, 23)}
THRESHOLDS_1 = [0.3]
THRESHOLDS_3 = [0.3, 0.5, 0.75]


def f32(v):
    return float(np.float32(v))


def make_box(aligned, cx, cy, l, w, theta):
    """-> (reference BoundingBox, its corners); aligned boxes ignore theta and have float32 coordinates."""
    if aligned:
        x0, y0, x1, y1 = f32(cx - l / 2), f32(cy - w / 2), f32(cx + l / 2), f32(cy + w / 2)
        corners = np.array([[x0, y0], [x0, y1], [x1, y0], [x1, y1]], dtype=np.float64)
        return BB.BoundingBox(corners, True)
    return BB.absolute_rotated_box_representation_to_boundingbox(cx, cy, l, w, theta)


def points_in(rng, cx, cy, l, w, theta, k, shrink=0.8):
    u = rng.uniform(-0.5, 0.5, size=(k, 2)) * [l * shrink, w * shrink]
    t = np.deg2rad(theta)
    return np.stack((cx + u[:, 0] * np.cos(t) - u[:, 1] * np.sin(t), cy + u[:, 0] * np.sin(t) + u[:, 1] * np.cos(t)), 1)


def random_objects(rng, aligned, n_obj, n_bg, n_extra):
    pts, gt, det = [], [], []
    for _ in range(n_obj):
        cx, cy = rng.uniform(-40, 80, size=2); l, w = rng.uniform(2, 8), rng.uniform(1, 4)
        theta = 0.0 if aligned else rng.uniform(0, 180)
        label = int(rng.integers(0, 5))
        pts.append(points_in(rng, cx, cy, l, w, theta, int(rng.integers(3, 20)), 1.0))
        gt.append((cx, cy, l, w, theta, label))
        for _ in range(int(rng.choice([0, 1, 1, 1, 2]))):
            det.append((cx + rng.normal(0, 0.4), cy + rng.normal(0, 0.3), l * (1 + rng.normal(0, 0.1)), w * (1 + rng.normal(0, 0.1)),
                        theta + (0 if aligned else rng.normal(0, 5)), label if rng.uniform() < 0.85 else int(rng.integers(0, 5))))
    for _ in range(n_extra):
        cx, cy = rng.uniform(-40, 80, size=2)
        det.append((cx, cy, rng.uniform(2, 8), rng.uniform(1, 4), 0.0 if aligned else rng.uniform(0, 180), int(rng.integers(0, 5))))
    pts.append(rng.uniform(-50, 100, size=(n_bg, 2)))
    return np.concatenate(pts), gt, det


def special_frame(kind, rng, aligned):
    pts, gt, det = random_objects(rng, aligned, 5, 60, 2)
    if kind == "no_detections":
        det = []
    elif kind == "no_ground_truth":
        gt = []
    elif kind == "neither":
        gt, det = [], []
    elif kind == "no_points":
        pts = np.zeros((0, 2))
    elif kind == "class_only_detected":
        det += [(10.0, 10.0, 4.0, 2.0, 0.0 if aligned else 30.0, 7), (30.0, -5.0, 5.0, 2.0, 0.0 if aligned else 100.0, 7)]
    elif kind == "class_only_ground_truth":
        gt += [(20.0, 20.0, 4.0, 2.0, 0.0 if aligned else 60.0, 8)]
    elif kind == "max_det_cut":
        for g in gt[:3]:
            gt.append(g[:5] + (0,))
        for i in range(130):
            g = gt[i % len(gt)]
            det.append((g[0] + rng.normal(0, 0.6), g[1] + rng.normal(0, 0.4), g[2] * (1 + rng.normal(0, 0.1)), g[3] * (1 + rng.normal(0, 0.1)),
                        g[4] + (0 if aligned else rng.normal(0, 5)), 0))
    elif kind == "competing_detections":
        g = gt[0]
        det += [(g[0] + 0.1, g[1], g[2], g[3], g[4], g[5]), (g[0] - 0.1, g[1] + 0.05, g[2], g[3], g[4], g[5]), (g[0], g[1] - 0.05, g[2], g[3], g[4], g[5])]
    elif kind == "equal_candidates":
        g = gt[1]
        gt += [g, g]                                              # (duplicates survive here: the metric is fed directly)
        det += [(g[0] + 0.05, g[1], g[2], g[3], g[4], g[5]), (g[0], g[1] + 0.05, g[2], g[3], g[4], g[5])]
    elif kind == "tied_candidates":
        # detection A, x in [700, 710], shares two points with each of two ground-truth boxes, x in [695, 705] and [705, 715]: IoU
        # 2 / 6 with both (box IoU 40 / 120 with both).  Detection B, x in [694, 704.5], has the lower score and overlaps the first
        # box only.  At threshold 0.3 the lowest position wins the tie: A takes the first box and B stays unmatched; had the highest
        # won, B would match.  All y in [500, 508], points on y = 504.
        xs = [696.0, 698.0, 701.0, 703.0, 707.0, 709.0, 711.0, 713.0]
        pts = np.concatenate((pts, np.stack((np.array(xs), np.full(len(xs), 504.0)), 1)))
        gt += [(700.0, 504.0, 10.0, 8.0, 0.0, 3), (710.0, 504.0, 10.0, 8.0, 0.0, 3)]
        det += [(705.0, 504.0, 10.0, 8.0, 0.0, 3), (699.25, 504.0, 10.5, 8.0, 0.0, 3)]
    elif kind in ("iou_3_of_10", "iou_1_of_2"):
        # detection x in [500, 510], ground truth x in [505, 515], both y in [500, 508]; points on the line y = 504
        tp, fp, fn = (3, 3, 4) if kind == "iou_3_of_10" else (2, 1, 1)
        label = 1 if kind == "iou_3_of_10" else 2
        xs = list(np.linspace(506, 509, tp)) + list(np.linspace(501, 504, fp)) + list(np.linspace(511, 514, fn))
        pts = np.concatenate((pts, np.stack((np.array(xs), np.full(len(xs), 504.0)), 1)))
        gt.append((510.0, 504.0, 10.0, 8.0, 0.0, label))
        det.append((505.0, 504.0, 10.0, 8.0, 0.0, label))
    return pts, gt, det


def build_case(aligned, use_point_iou, seed):
    rng = np.random.default_rng(seed)
    frames = []
    kinds = list(SPECIAL_FRAMES) + ["plain"] * N_RANDOM
    for kind in kinds:
        pts, gt, det = special_frame(kind, rng, aligned) if kind != "plain" else random_objects(
            rng, aligned, int(rng.integers(1, 9)), int(rng.integers(20, 120)), int(rng.integers(0, 4)))
        pts = pts.astype(np.float32)
        gt_boxes = [make_box(aligned, *g[:5]) for g in gt]
        det_boxes = [make_box(aligned, *d[:5]) for d in det]
        rep = BB.BoundingBox.get_two_point_representations if aligned else BB.BoundingBox.get_absolute_rotated_box_representations
        width = 4 if aligned else 5
        gt_mat = rep(gt_boxes).astype(np.float32).reshape(-1, width)
        det_mat = rep(det_boxes).astype(np.float32).reshape(-1, width)
        if not aligned and len(pts):
            bad = np.zeros(len(pts), dtype=bool)
            for b in np.concatenate((det_mat, gt_mat)):
                c = E.box_corners(b)
                bad |= np.array([abs(E.area_slack(c, p) - 1e-6) < SLACK_MARGIN for p in pts.astype(np.float64)])
            pts = pts[~bad]
        frames.append(dict(kind=kind, points=pts, gt=gt_mat, pred=det_mat,
                           gt_corners=np.array([b.corners for b in gt_boxes], dtype=np.float64).reshape(-1, 4, 2),
                           pred_corners=np.array([b.corners for b in det_boxes], dtype=np.float64).reshape(-1, 4, 2),
                           gt_labels=np.array([g[5] for g in gt], dtype=np.int64), pred_labels=np.array([d[5] for d in det], dtype=np.int64)))
    n_det = sum(len(fr["pred"]) for fr in frames)
    scores = ((rng.permutation(n_det) + 1) / (n_det + 1)).astype(np.float32)
    at = 0
    for fr in frames:
        fr["pred_scores"] = scores[at:at + len(fr["pred"])].copy()
        at += len(fr["pred"])
        if fr["kind"] == "tied_candidates" and fr["pred_scores"][-2] < fr["pred_scores"][-1]:      # A before B
            fr["pred_scores"][[-2, -1]] = fr["pred_scores"][[-1, -2]]
    return frames


def full_iou(fr, aligned, use_point_iou):
    p, g = torch.from_numpy(fr["pred"]), torch.from_numpy(fr["gt"])
    if len(p) == 0 or len(g) == 0:
        return np.zeros((len(p), len(g)), dtype=np.float64 if use_point_iou else np.float32)
    if use_point_iou:
        return point_iou_f64(p, g, fr["points"], aligned).numpy()
    return _box_iou(p, g).numpy()


def ambiguous(frames, ious, thresholds):
    """Box-IoU margins and distinct scores (see the module docstring)."""
    labels = np.concatenate([fr["pred_labels"] for fr in frames]); scores = np.concatenate([fr["pred_scores"] for fr in frames])
    for c in np.unique(labels):
        s = scores[labels == c]
        if len(np.unique(s)) != len(s):
            return "equal scores"
    for fr, iou in zip(frames, ious):
        if iou.dtype != np.float32:
            continue
        for d in range(iou.shape[0]):
            row = np.sort(iou[d, fr["gt_labels"] == fr["pred_labels"][d]].astype(np.float64))[::-1]
            if any(abs(v - t) < IOU_MARGIN for v in row for t in thresholds):
                return "IoU near a threshold"
            if len(row) > 1 and row[0] != row[1] and abs(row[0] - row[1]) < IOU_MARGIN:
                return "candidates too close"
    return None


def iterated_envelope(pr):
    """The reference's form of the envelope: add the positive forward differences until nothing changes."""
    pr = torch.from_numpy(pr.copy())
    while len(pr):
        diff = torch.clamp(torch.cat((pr[1:] - pr[:-1], torch.zeros(1))), min=0)
        if bool(torch.all(diff == 0)):
            break
        pr += diff
    return pr.numpy()


def envelopes_agree(frames, res):
    labels = np.concatenate([fr["pred_labels"] for fr in frames]); scores = np.concatenate([fr["pred_scores"] for fr in frames])
    order = MO.order_desc(scores)
    n = 0
    for c in res["classes"]:
        for max_det in MO.MAX_DETS:
            sel = order[(labels[order] == c) & (res["rank"][order] >= 0) & (res["rank"][order] < max_det)]
            for ti in range(res["matched"].shape[0]):
                tps = res["matched"][ti, sel].astype(bool)
                tp, fp = np.cumsum(tps).astype(np.float32), np.cumsum(~tps).astype(np.float32)
                pr = tp / ((fp + tp) + MO.EPS32)
                if not np.array_equal(iterated_envelope(pr), MO.envelope(pr)):
                    return False
                n += 1
    return n > 0


def run_reference(frames, aligned, use_point_iou, thresholds):
    preds = [dict(boxes=torch.from_numpy(fr["pred"]), scores=torch.from_numpy(fr["pred_scores"]), labels=torch.from_numpy(fr["pred_labels"]))
             for fr in frames]
    target = [dict(boxes=torch.from_numpy(fr["gt"]), labels=torch.from_numpy(fr["gt_labels"])) for fr in frames]
    metric = TM.MeanAveragePrecision("xyxy", "bbox", list(thresholds), class_metrics=True)
    tables = {}
    calculate = metric._calculate

    def keep_tables(class_ids):
        tables["precision"], tables["recall"] = calculate(class_ids)
        return tables["precision"], tables["recall"]

    metric._calculate = keep_tables
    if use_point_iou:
        metric.update(preds, target, True, [fr["points"] for fr in frames], aligned)
    else:
        metric.update(preds, target)
    res = metric.compute()
    out = {k: np.asarray(res[k].numpy(), dtype=np.float32).reshape(-1) for k in ("map", "map_50", "map_75", "mar_1", "mar_10", "mar_100",
                                                                                  "map_per_class", "mar_100_per_class")}
    out["classes"] = np.array(metric._get_classes(), dtype=np.int64)
    out["precision"] = tables["precision"][:, :, :, 0, :].numpy()          # area range "all"
    out["recall"] = tables["recall"][:, :, 0, :].numpy()
    return out


def check_against_restatement(frames, ious, ref, thresholds, name):
    mine = MO.mean_ap(ious, [fr["pred_labels"] for fr in frames], [fr["pred_scores"] for fr in frames], [fr["gt_labels"] for fr in frames],
                      thresholds)
    assert list(ref["classes"]) == mine["classes"], name
    assert np.array_equal(ref["precision"], mine["precision"]) and np.array_equal(ref["recall"], mine["recall"]), name
    for k in ("map", "map_50", "map_75", "mar_1", "mar_10", "mar_100", "map_per_class", "mar_100_per_class"):
        assert np.allclose(ref[k], np.asarray(mine[k]).reshape(-1), rtol=0, atol=1e-6), (name, k)
    return mine


def map_case(name):
    aligned, use_point_iou, seed = CASES[name]
    redraws = 0
    while True:
        frames = build_case(aligned, use_point_iou, seed)
        ious = [full_iou(fr, aligned, use_point_iou) for fr in frames]
        why = ambiguous(frames, ious, THRESHOLDS_3)
        if why is None:
            ref1, ref3 = run_reference(frames, aligned, use_point_iou, THRESHOLDS_1), run_reference(frames, aligned, use_point_iou, THRESHOLDS_3)
            mine1 = check_against_restatement(frames, ious, ref1, THRESHOLDS_1, name)
            mine3 = check_against_restatement(frames, ious, ref3, THRESHOLDS_3, name)
            if envelopes_agree(frames, mine1) and envelopes_agree(frames, mine3):
                break
            why = "iterated envelope differs from the running maximum"
        print(name, "drawn again:", why)
        redraws += 1
        seed += 1000
    if use_point_iou:                                                  # the exact fractions sit where the frames were built for them
        for kind, value in (("iou_3_of_10", 3 / 10), ("iou_1_of_2", 1 / 2)):
            f = [fr["kind"] for fr in frames].index(kind)
            assert ious[f][-1, -1] == value, (kind, ious[f][-1, -1])
            at = sum(len(fr["pred"]) for fr in frames[:f + 1]) - 1
            assert list(mine3["matched"][:, at]) == ([0, 0, 0] if kind == "iou_3_of_10" else [1, 0, 0]), kind
    f = [fr["kind"] for fr in frames].index("max_det_cut")
    assert (frames[f]["pred_labels"] == 0).sum() > 100
    f = [fr["kind"] for fr in frames].index("tied_candidates")          # (the tables were found equal to the reference's above)
    assert ious[f][-2, -2] == ious[f][-2, -1] > 0.3 and ious[f][-1, -2] > 0.75 and ious[f][-1, -1] < 0.3, ious[f][-2:, -2:]
    at = sum(len(fr["pred"]) for fr in frames[:f + 1])
    assert mine3["matched"][:, at - 2:at].tolist() == [[1, 0], [0, 1], [0, 1]], mine3["matched"][:, at - 2:at]
    cat = lambda key: np.concatenate([fr[key] for fr in frames])
    ptr = lambda key: np.cumsum([0] + [len(fr[key]) for fr in frames])
    out = dict(points=cat("points").reshape(-1, 2), frame_ptr=ptr("points"), pred=cat("pred"), pred_corners=cat("pred_corners"),
               pred_ptr=ptr("pred"), pred_labels=cat("pred_labels"), pred_scores=cat("pred_scores"), gt=cat("gt"), gt_corners=cat("gt_corners"),
               gt_ptr=ptr("gt"), gt_labels=cat("gt_labels"), iou=np.concatenate([i.reshape(-1) for i in ious]),
               iou_ptr=np.cumsum([0] + [i.size for i in ious]), aligned=aligned, use_point_iou=use_point_iou,
               kinds=np.array([fr["kind"] for fr in frames]), rec_thresholds=torch.linspace(0.0, 1.0, 101).numpy())
    for tag, thr, ref, mine in (("t1", THRESHOLDS_1, ref1, mine1), ("t3", THRESHOLDS_3, ref3, mine3)):
        out[f"{tag}_thresholds"] = np.array(thr, dtype=np.float64)
        for k, v in ref.items():
            out[f"{tag}_{k}"] = v
        out[f"{tag}_rank"], out[f"{tag}_matched"] = mine["rank"], mine["matched"]
    np.savez_compressed(os.path.join(HERE, f"eval_map_{name}.npz"), **out)
    print(name, "frames", len(frames), "detections", len(out["pred"]), "ground truth", len(out["gt"]), "redraws", redraws,
          "map", ref1["map"], "map(T=3)", ref3["map"], "per class", ref1["map_per_class"])


def segmentation_case():
    from sklearn.metrics import confusion_matrix, f1_score, multilabel_confusion_matrix
    out = {}
    for tag, n in (("large", 300000), ("small", 1000)):
        y_true, y_pred = MO.segmentation_labels(n)
        k = MO.SEG_CLASSES
        yt, yp = y_true.astype(int).tolist(), y_pred.astype(int).tolist()       # as SegmentationMetrics builds its vectors
        out[f"{tag}_n"] = n
        out[f"{tag}_confusion"] = confusion_matrix(yt, yp, labels=range(k))
        out[f"{tag}_per_class"] = multilabel_confusion_matrix(yt, yp, labels=range(k))
        out[f"{tag}_f1_none"] = f1_score(yt, yp, labels=range(k), average=None, zero_division=0)
        for avg in ("micro", "macro", "weighted"):
            out[f"{tag}_f1_{avg}"] = f1_score(yt, yp, labels=range(k), average=avg, zero_division=0)
        ext = MO.extended_confusion(y_true, y_pred, k)
        assert np.array_equal(ext[:k, :k], out[f"{tag}_confusion"]) and np.array_equal(MO.matrices_per_class(ext), out[f"{tag}_per_class"])
    np.savez_compressed(os.path.join(HERE, "eval_seg_confusion.npz"), **out)
    print("segmentation", {k: v for k, v in out.items() if "f1" in k and "large" in k})


if __name__ == "__main__":
    for case in CASES:
        map_case(case)
    segmentation_case()
