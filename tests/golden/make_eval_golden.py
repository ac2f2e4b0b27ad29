"""Writes tests/golden/eval_*.npz: inputs and outputs of the reference's evaluation half, produced by EXECUTING the
reference's own code: GroundTruthExtractor and Postprocessor.process_one_ground_truth (postprocessor/postprocessing.py,
loaded by file path with stub modules for torchvision / detectron2, whose names it only imports) and point_iou
(utils/math.py).  Runs only in the build container; the fixtures are committed.

numpy here is 2.x (float32 scalars stay float32 under NEP 50); the reference's environment is numpy 1.x, where the same
scalar expressions promote to float64 -- so boxes and points are cast to float64 before they enter the reference code.

Margins: device sin / cos / atan2 differ from the host's in the last ulps, so the cases avoid the two thresholds:
  - duplicate removal: every pair of ground-truth boxes of a frame whose corner-distance sum lies within 1e-7 of 0.1 makes
    the generator draw the frame again (next seed);
  - point IoU (rotated): every point whose area-test slack for some box lies within 1e-9 of the 1e-6 bound is dropped.
"""
import importlib.util
import os
import sys
import types

import numpy as np

R = "/root/reference/src/gnnradarobjectdetection"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import eval_oracle as E  # noqa: E402

for name in ("gnnradarobjectdetection", "gnnradarobjectdetection.utils", "gnnradarobjectdetection.preprocessor",
             "gnnradarobjectdetection.postprocessor"):
    m = types.ModuleType(name); m.__path__ = []; sys.modules[name] = m
sys.modules["torchvision"] = types.ModuleType("torchvision")
sys.modules["detectron2"] = types.ModuleType("detectron2")
layers = types.ModuleType("detectron2.layers"); layers.nms_rotated = None; sys.modules["detectron2.layers"] = layers


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    return mod


M = load("gnnradarobjectdetection.utils.math", R + "/utils/math.py")
load("gnnradarobjectdetection.preprocessor.bounding_box", R + "/preprocessor/bounding_box.py")
load("gnnradarobjectdetection.postprocessor.configs", R + "/postprocessor/configs.py")
PP = load("gnnradarobjectdetection.postprocessor.postprocessing", R + "/postprocessor/postprocessing.py")
BG = 5
DUP_MARGIN = 1e-7
SLACK_MARGIN = 1e-9


def synthetic_frame(rng, n_obj, n_bg, width, invariance):
    """Objects whose points all carry (float32) relative boxes of their object, plus background points with NaN boxes."""
    pos, labels, boxes = [], [], []
    for _ in range(n_obj):
        c = rng.uniform(-40, 80, size=2); l, w = rng.uniform(1.5, 6), rng.uniform(0.8, 2.5); th = rng.uniform(0, np.pi)
        k = int(rng.integers(2, 25))
        u = rng.uniform(-0.5, 0.5, size=(k, 2)) * [l, w]
        p = c + np.stack((u[:, 0] * np.cos(th) - u[:, 1] * np.sin(th), u[:, 0] * np.sin(th) + u[:, 1] * np.cos(th)), 1)
        p = p.astype(np.float32)
        pos.append(p); labels.append(np.full(k, rng.integers(0, BG), dtype=np.float32))
        b = np.zeros((k, width))
        if width == 4:
            ext = np.abs(np.cos(th)) * l + np.abs(np.sin(th)) * w, np.abs(np.sin(th)) * l + np.abs(np.cos(th)) * w
            b[:] = [0, 0, ext[0], ext[1]]
            b[:, :2] = c - p
        elif invariance == "none":
            b[:] = [c[0], c[1], l, w, th]
        else:
            b[:] = [0, 0, l, w, th]
            b[:, :2] = c - p
        boxes.append(b)
    pos.append(rng.uniform(-50, 100, size=(n_bg, 2)).astype(np.float32))
    labels.append(np.full(n_bg, BG, dtype=np.float32)); boxes.append(np.full((n_bg, width), np.nan))
    pos, labels, boxes = np.concatenate(pos), np.concatenate(labels), np.concatenate(boxes)
    perm = rng.permutation(len(pos))
    pos, labels, boxes = pos[perm], labels[perm], boxes[perm]
    if invariance == "en" and len(pos) > 1:               # the E(n)-invariant form relative to each point's nearest neighbour
        from sklearn.neighbors import kneighbors_graph
        nn = np.where(kneighbors_graph(pos.astype(np.float64), 1, mode="connectivity", include_self=False).toarray() == 1)[1]
        for i in np.where(labels != BG)[0]:
            c = pos[i].astype(np.float64) + boxes[i, :2]
            v = pos[nn[i]].astype(np.float64) - pos[i]
            th_nn = np.arctan2(v[1], v[0])
            boxes[i, 0] = np.hypot(*boxes[i, :2])
            boxes[i, 1] = np.mod(np.arctan2(c[1] - pos[i, 1], c[0] - pos[i, 0]) - th_nn, 2 * np.pi)
            boxes[i, 4] = np.mod(boxes[i, 4] - th_nn, 2 * np.pi)
    return pos, labels, boxes.astype(np.float32)


def reference_ground_truth(pos, labels, boxes, invariance):
    bbs, lab = PP.GroundTruthExtractor.get_absolute_object_bounding_boxes(labels, boxes.astype(np.float64),
                                                                          pos.astype(np.float64), invariance, BG)
    decoded = np.array([b.corners for b in bbs]).reshape(-1, 4, 2)
    objects, _ = PP.Postprocessor.process_one_ground_truth(pos.astype(np.float64), np.zeros_like(pos), boxes.astype(np.float64),
                                                           labels, invariance, BG)
    corners = np.array([b.corners for b in objects["boxes"]]).reshape(-1, 4, 2)
    return decoded, lab, corners, objects["labels"]


def near_threshold(corners):
    for j in range(len(corners)):
        for i in range(j):
            if abs(E.l1_sum(corners[i], corners[j]) - 0.1) < DUP_MARGIN:
                return True
    return False


def gt_case(name, width, invariance, seed):
    frames = []
    plan = [(6, 40), (9, 120), (0, 0), (0, 30), (14, 200)]       # (objects, background points): an empty, an all-background frame
    for f, (n_obj, n_bg) in enumerate(plan):
        s = seed * 100 + f
        while True:
            rng = np.random.default_rng(s)
            pos, labels, boxes = synthetic_frame(rng, n_obj, n_bg, width, invariance)
            decoded, dlab, corners, clab = reference_ground_truth(pos, labels, boxes, invariance)
            if not near_threshold(decoded):
                break
            s += 1000
        frames.append(dict(pos=pos, labels=labels, boxes=boxes, decoded=decoded, decoded_labels=dlab.reshape(-1),
                           corners=corners, box_labels=np.asarray(clab).reshape(-1)))
    ptr = lambda key: np.cumsum([0] + [len(fr[key]) for fr in frames])
    out = {k: np.concatenate([fr[k] for fr in frames]) for k in frames[0]}
    out["decoded"] = out["decoded"].reshape(-1, 4, 2); out["corners"] = out["corners"].reshape(-1, 4, 2)
    np.savez_compressed(os.path.join(HERE, f"eval_gt_{name}.npz"), frame_ptr=ptr("pos"), decoded_ptr=ptr("decoded"),
                        box_ptr=ptr("corners"), invariance=invariance, bg_index=BG, **out)
    print(name, "nodes", out["pos"].shape[0], "decoded", len(out["decoded"]), "kept", len(out["corners"]))


def dedup_case():
    """Hand-made corner sets through the reference's remove_duplicate_boxes: the chain, inf, NaN, sums either side of 0.1."""
    base = np.array([[1.0, 2.0], [1.0, -2.0], [-1.0, -2.0], [-1.0, 2.0]]) + [10.0, 20.0]
    boxes = [base, base + [0.02, 0.0], base + [0.04, 0.0],                        # A~B (0.08), B~C (0.08), A!~C (0.16)
             base + [5.0, 0.0], base + [5.0, 0.0],                                 # exact duplicate
             np.full((4, 2), np.inf), np.full((4, 2), np.inf),                     # equal inf: == match, sum NaN
             np.full((4, 2), np.nan), np.full((4, 2), np.nan),                     # NaN never matches
             base + [30.0, 0.0]]
    just_below = base + [30.0 + 0.0249999, 0.0]                                     # 4 x 0.0249999: just under 0.1
    just_above = base + [30.0, 0.0250001]
    boxes += [just_below, just_above]
    for k in range(-3, 4):                                                          # sums within a few ulps of 0.1
        anchor = base + [60.0 + 10 * k, 0.0]
        boxes += [anchor, anchor + [0.025 + k * 1e-17 * 2 ** 8, 0.0]]
    corners = np.array(boxes, dtype=np.float64)
    labels = np.arange(len(corners), dtype=np.float32).reshape(-1, 1)
    sums = [E.l1_sum(corners[9], corners[k]) for k in (10, 11)]
    assert sums[0] < 0.1 < sums[1], sums
    bbs = [types.SimpleNamespace(corners=c.copy()) for c in corners]
    kept_boxes, kept_labels = PP.GroundTruthExtractor.remove_duplicate_boxes(bbs, labels)
    kept = kept_labels.reshape(-1).astype(np.int64)
    np.savez_compressed(os.path.join(HERE, "eval_dedup_adversarial.npz"), corners=corners, labels=labels, kept=kept)
    print("dedup kept", kept.tolist())


def iou_case(name, aligned, seed):
    rng = np.random.default_rng(seed)
    frames = []
    for f, (n, n_pred, n_gt) in enumerate([(300, 12, 7), (150, 0, 4), (80, 5, 0), (0, 3, 2), (260, 9, 9), (2, 1, 1)]):
        pts = rng.uniform(-20, 20, size=(n, 2)).astype(np.float32)
        if n > 20:
            pts[5] = pts[4]; pts[6] = pts[4]                                          # repeated coordinates (the 1/3 case)
            pts[7] = [0.0, 3.0]; pts[8] = [-0.0, 3.0]                                 # -0.0 against 0.0
            pts[9] = [-0.0, -0.0]; pts[10] = [0.0, 0.0]
        gt, pred = [], []
        for _ in range(n_gt):
            c = rng.uniform(-15, 15, size=2); l, w = rng.uniform(2, 12), rng.uniform(1, 8); th = rng.uniform(0, 180)
            gt.append([c[0] - l / 2, c[1] - w / 2, c[0] + l / 2, c[1] + w / 2] if aligned else [c[0], c[1], l, w, th])
        for k in range(n_pred):
            if k < n_gt and k % 2 == 0:
                base = np.array(gt[k]); pred.append(base + rng.normal(0, 0.8, size=base.shape) * (base.shape[0] == 4 or [1, 1, 0.3, 0.3, 5]))
            elif k == n_pred - 1:
                pred.append([100, 100, 101, 101] if aligned else [100, 100, 1, 1, 0])      # a box with no points: 1e-5 pairs
            else:
                c = rng.uniform(-15, 15, size=2); l, w = rng.uniform(2, 12), rng.uniform(1, 8)
                pred.append([c[0] - l / 2, c[1] - w / 2, c[0] + l / 2, c[1] + w / 2] if aligned else [c[0], c[1], l, w, rng.uniform(0, 180)])
        pred = np.array(pred, dtype=np.float32).reshape(-1, 4 if aligned else 5)
        gt = np.array(gt, dtype=np.float32).reshape(-1, 4 if aligned else 5)
        if n == 2:                                                                  # two equal points inside both boxes: 1/3
            pts[:] = [1.0, 1.0]
            pred[:] = gt[:] = [0, 0, 2, 2] if aligned else [1, 1, 2, 2, 30]
        if aligned and n > 20 and len(gt):                                          # points exactly on the edges of a box
            pts[11] = [gt[0, 0], pts[11, 1]]; pts[12] = [gt[0, 2], gt[0, 3]]; pts[13] = [gt[0, 0], gt[0, 1]]
        if not aligned and n:
            bad = np.zeros(n, dtype=bool)
            for b in np.concatenate((pred, gt)):
                c = E.box_corners(b)
                bad |= np.array([abs(E.area_slack(c, p) - 1e-6) < SLACK_MARGIN for p in pts.astype(np.float64)])
            pts = pts[~bad]
        iou = M.point_iou(pred.astype(np.float64), gt.astype(np.float64), pts.astype(np.float64), aligned).numpy()
        frames.append((pts, pred, gt, iou.reshape(-1)))
    cat = lambda i, w: np.concatenate([fr[i] for fr in frames]).reshape(-1, w) if w else np.concatenate([fr[i] for fr in frames])
    ptr = lambda i: np.cumsum([0] + [len(fr[i]) for fr in frames])
    np.savez_compressed(os.path.join(HERE, f"eval_iou_{name}.npz"), points=cat(0, 2), frame_ptr=ptr(0), pred=cat(1, 4 if aligned else 5),
                        pred_ptr=ptr(1), gt=cat(2, 4 if aligned else 5), gt_ptr=ptr(2), iou=cat(3, None), iou_ptr=ptr(3), aligned=aligned)
    print(name, "points", sum(len(fr[0]) for fr in frames), "pairs", sum(len(fr[3]) for fr in frames))


if __name__ == "__main__":
    gt_case("aligned", 4, "translation", 1)
    gt_case("rot_none", 5, "none", 2)
    gt_case("rot_translation", 5, "translation", 3)
    gt_case("rot_en", 5, "en", 4)
    dedup_case()
    iou_case("aligned", True, 11)
    iou_case("rotated", False, 12)
