"""Time ``ObjectDetectionMetrics.get_map`` (point IoU, rotated boxes) on a synthetic evaluation set of RadarScenes-shaped frames
(``radargnn_amd.synthetic``), beside the numpy restatement ``tests/map_oracle.py`` on the same inputs on the same box.

    python tools/map_bench.py [--frames 2000] [--repeats 10] [--warmup 3] [--numpy-repeats 3]

The restatement covers matching, curves and summaries only (a numpy point IoU over 3000 points per frame would take hours), so it
is handed the IoU matrices the device computed; the device figure is also split into its IoU part and the rest.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def rotated_corners(c, l, w, theta):
    ox, oy = np.array([l / 2, l / 2, -l / 2, -l / 2]), np.array([w / 2, -w / 2, -w / 2, w / 2])
    return np.stack((c[0] + np.cos(theta) * ox - np.sin(theta) * oy, c[1] + np.sin(theta) * ox + np.cos(theta) * oy), 1)


def evaluation_set(n_frames: int, n_gt: int = 20, n_extra: int = 5):
    from radargnn_amd import synthetic
    from radargnn_amd.postprocessor import BoundingBoxes
    bb_pred, bb_gt, cls_pred = [], [], []
    for f in range(n_frames):
        fr = synthetic.radarscenes_frame(f)
        rng = np.random.default_rng(f)
        gt, det, gl, dl = [], [], [], []
        for i in rng.choice(fr.n, size=n_gt, replace=False):
            l, w, th, label = rng.uniform(2, 6), rng.uniform(1, 2.5), rng.uniform(0, np.pi), int(rng.integers(0, 5))
            gt.append(rotated_corners(fr.X[i], l, w, th)); gl.append(label)
            if rng.uniform() < 0.8:
                det.append(rotated_corners(fr.X[i] + rng.normal(0, 0.3, 2), l * rng.uniform(0.9, 1.1), w * rng.uniform(0.9, 1.1), th + rng.normal(0, 0.1)))
                dl.append(label if rng.uniform() < 0.9 else int(rng.integers(0, 5)))
        for i in rng.choice(fr.n, size=n_extra, replace=False):
            det.append(rotated_corners(fr.X[i], rng.uniform(2, 6), rng.uniform(1, 2.5), rng.uniform(0, np.pi))); dl.append(int(rng.integers(0, 5)))
        cuda = lambda a, dt: torch.from_numpy(np.asarray(a, dtype=dt)).cuda()
        bb_pred.append({"boxes": BoundingBoxes(cuda(det, np.float64).reshape(-1, 4, 2), False), "scores": cuda(rng.uniform(0.2, 1, len(det)), np.float64),
                        "labels": cuda(dl, np.float64)})
        bb_gt.append({"boxes": BoundingBoxes(cuda(gt, np.float64).reshape(-1, 4, 2), False), "labels": cuda(gl, np.float32)})
        cls_pred.append({"pos": cuda(fr.X, np.float32)})
    return bb_pred, bb_gt, cls_pred


def timed(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--numpy-repeats", type=int, default=3)
    args = ap.parse_args()
    import map_oracle as MO
    from radargnn_amd import metrics, ops
    from radargnn_amd.postprocessor import PostProcessingConfiguration
    config = PostProcessingConfiguration(iou_for_mAP=0.3, use_point_iou=True)
    bb_pred, bb_gt, cls_pred = evaluation_set(args.frames)
    t_all = timed(lambda: metrics.ObjectDetectionMetrics.get_map(config, bb_pred, bb_gt, cls_pred), args.repeats, args.warmup)
    res = metrics.ObjectDetectionMetrics.get_map(config, bb_pred, bb_gt, cls_pred)

    # the parts, on the packed inputs get_map builds
    boxes_pred, pred_ptr = metrics._box_matrices(bb_pred, False)
    boxes_gt, gt_ptr = metrics._box_matrices(bb_gt, False)
    points = torch.cat([c["pos"] for c in cls_pred])
    frame_ptr = np.cumsum([0] + [c["pos"].shape[0] for c in cls_pred]).tolist()
    det_scores = torch.cat([d["scores"] for d in bb_pred]).to(torch.float32)
    det_labels = torch.cat([d["labels"] for d in bb_pred]).to(torch.int32)
    gt_labels = torch.cat([d["labels"] for d in bb_gt]).to(torch.int32)
    classes = torch.unique(torch.cat((det_labels, gt_labels)))
    t_iou = timed(lambda: ops.point_iou(boxes_pred, pred_ptr, boxes_gt, gt_ptr, points, frame_ptr, True), args.repeats, args.warmup)
    iou, out_ptr = ops.point_iou(boxes_pred, pred_ptr, boxes_gt, gt_ptr, points, frame_ptr, True)

    def rest():
        rank, matched = ops.map_match(iou, pred_ptr, gt_ptr, det_labels, det_scores, gt_labels, classes, [0.3], 100)
        p, _, r = ops.map_curves(det_labels, det_scores, rank, matched, gt_labels, classes)
        return metrics.ObjectDetectionMetrics._summarize(p, r, classes, [0.3])
    t_rest = timed(rest, args.repeats, args.warmup)

    iou_h, dl, ds, gl = iou.cpu().numpy(), det_labels.cpu().numpy(), det_scores.cpu().numpy(), gt_labels.cpu().numpy()
    n = args.frames
    ious = [iou_h[out_ptr[f]:out_ptr[f + 1]].reshape(pred_ptr[f + 1] - pred_ptr[f], gt_ptr[f + 1] - gt_ptr[f]) for f in range(n)]
    split = lambda a, ptr: [a[ptr[f]:ptr[f + 1]] for f in range(n)]
    args_np = (ious, split(dl, pred_ptr), split(ds, pred_ptr), split(gl, gt_ptr), [0.3])
    times = []
    for _ in range(args.numpy_repeats):
        t0 = time.perf_counter()
        want = MO.mean_ap(*args_np)
        times.append(time.perf_counter() - t0)
    same = bool(np.array_equal(want["precision"], res["precision"].numpy()) and np.array_equal(want["recall"], res["recall"].numpy()))
    print(json.dumps({"frames": n, "detections": pred_ptr[-1], "ground_truth": gt_ptr[-1], "points": frame_ptr[-1], "iou_pairs": out_ptr[-1],
                      "get_map_ms": round(t_all * 1e3, 3), "point_iou_ms": round(t_iou * 1e3, 3),
                      "match_curves_summaries_ms": round(t_rest * 1e3, 3),
                      "numpy_match_curves_summaries_ms": round(statistics.median(times) * 1e3, 3),
                      "tables_equal_numpy": same, "map": round(float(res["map"]), 6)}))


if __name__ == "__main__":
    main()
