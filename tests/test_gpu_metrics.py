"""Evaluation metrics on the device (csrc/metrics.hip through radargnn_amd.ops and radargnn_amd.metrics) against the fixtures that the
executed reference wrote (tests/golden/make_map_golden.py): match flags, ranks, the recall / precision tables and the box IoU exact,
summaries within 1e-6 of the reference's float32 means, the confusion matrix exact and F1 within 1e-12 of scikit-learn's recorded
values.  Neither the reference nor scikit-learn is needed here."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import map_oracle as MO

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = sorted(glob.glob(os.path.join(GOLDEN, "eval_map_*.npz")))
IDS = [os.path.basename(p)[9:-4] for p in CASES]
SUMMARIES = ("map", "map_50", "map_75", "mar_1", "mar_10", "mar_100", "map_per_class", "mar_100_per_class")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radargnn_amd import ops
    return ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def device_iou(ops, g, frames=None):
    """The fixture's IoU matrices recomputed on the device, for all frames or the frames [a, b)."""
    a, b = frames if frames is not None else (0, len(g["pred_ptr"]) - 1)
    pp, gp, fp = g["pred_ptr"], g["gt_ptr"], g["frame_ptr"]
    pred, gt = dev(g["pred"][pp[a]:pp[b]]), dev(g["gt"][gp[a]:gp[b]])
    pred_ptr, gt_ptr = (pp[a:b + 1] - pp[a]).tolist(), (gp[a:b + 1] - gp[a]).tolist()
    if bool(g["use_point_iou"]):
        iou, _ = ops.point_iou(pred, pred_ptr, gt, gt_ptr, dev(g["points"][fp[a]:fp[b]]).reshape(-1, 2), (fp[a:b + 1] - fp[a]).tolist(),
                               not bool(g["aligned"]))
    else:
        iou, _ = ops.box_iou(pred, pred_ptr, gt, gt_ptr)
    return iou, pred_ptr, gt_ptr


def device_match(ops, g, tag, frames=None):
    a, b = frames if frames is not None else (0, len(g["pred_ptr"]) - 1)
    pp, gp = g["pred_ptr"], g["gt_ptr"]
    iou, pred_ptr, gt_ptr = device_iou(ops, g, frames)
    det_labels, det_scores = dev(g["pred_labels"][pp[a]:pp[b]], torch.int32), dev(g["pred_scores"][pp[a]:pp[b]])
    gt_labels, classes = dev(g["gt_labels"][gp[a]:gp[b]], torch.int32), dev(g[f"{tag}_classes"], torch.int32)
    rank, matched = ops.map_match(iou, pred_ptr, gt_ptr, det_labels, det_scores, gt_labels, classes, list(g[f"{tag}_thresholds"]), 100)
    return rank, matched, (det_labels, det_scores, gt_labels, classes)


@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_iou_recomputed_on_the_device_is_the_references(ops, path):
    g = np.load(path)
    iou, _, _ = device_iou(ops, g)
    assert iou.dtype == (torch.float64 if bool(g["use_point_iou"]) else torch.float32)
    assert np.array_equal(iou.cpu().numpy(), g["iou"])


@pytest.mark.parametrize("tag", ["t1", "t3"])
@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_match_and_curves_exact(ops, path, tag):
    g = np.load(path)
    rank, matched, (det_labels, det_scores, gt_labels, classes) = device_match(ops, g, tag)
    assert np.array_equal(rank.cpu().numpy(), g[f"{tag}_rank"])
    assert np.array_equal(matched.cpu().numpy(), g[f"{tag}_matched"])
    # the curves from the FIXTURE's flags, so that this half stands on its own
    precision, scores, recall = ops.map_curves(det_labels, det_scores, dev(g[f"{tag}_rank"]), dev(g[f"{tag}_matched"]), gt_labels, classes)
    assert precision.shape == g[f"{tag}_precision"].shape and recall.shape == g[f"{tag}_recall"].shape
    assert np.array_equal(precision.cpu().numpy(), g[f"{tag}_precision"])
    assert np.array_equal(recall.cpu().numpy(), g[f"{tag}_recall"])
    want = MO.curves(g["pred_labels"], g["pred_scores"], g[f"{tag}_rank"], g[f"{tag}_matched"], g["gt_labels"], list(g[f"{tag}_classes"]))
    assert np.array_equal(scores.cpu().numpy(), want[1])


def test_packing_does_not_leak_across_frames(ops):
    g = np.load(os.path.join(GOLDEN, "eval_map_rotated_point.npz"))
    n = len(g["pred_ptr"]) - 1
    whole_rank, whole_matched, _ = device_match(ops, g, "t3")
    cut = 9
    parts = [device_match(ops, g, "t3", (0, cut)), device_match(ops, g, "t3", (cut, n))]
    assert torch.equal(whole_rank, torch.cat([p[0] for p in parts]))
    assert torch.equal(whole_matched, torch.cat([p[1] for p in parts], dim=1))


def postprocessor_shaped(g, on_device=True):
    """The fixture as ``Postprocessor.process`` returns it (tensors in HBM) or as the reference holds it (host objects, numpy)."""
    from radargnn_amd.postprocessor import BoundingBox, BoundingBoxes
    aligned = bool(g["aligned"])
    pp, gp, fp = g["pred_ptr"], g["gt_ptr"], g["frame_ptr"]
    bb_pred, bb_gt, cls_pred = [], [], []
    for f in range(len(pp) - 1):
        pc, gc = g["pred_corners"][pp[f]:pp[f + 1]], g["gt_corners"][gp[f]:gp[f + 1]]
        scores, labels = g["pred_scores"][pp[f]:pp[f + 1]].astype(np.float64), g["pred_labels"][pp[f]:pp[f + 1]].astype(np.float64)
        gl, pos = g["gt_labels"][gp[f]:gp[f + 1]].astype(np.float32), g["points"][fp[f]:fp[f + 1]]
        if on_device:
            bb_pred.append({"boxes": BoundingBoxes(dev(pc).reshape(-1, 4, 2), aligned), "scores": dev(scores), "labels": dev(labels)})
            bb_gt.append({"boxes": BoundingBoxes(dev(gc).reshape(-1, 4, 2), aligned), "labels": dev(gl)})
            cls_pred.append({"pos": dev(pos).reshape(-1, 2)})
        else:
            bb_pred.append({"boxes": [BoundingBox(c, aligned) for c in pc], "scores": scores, "labels": labels})
            bb_gt.append({"boxes": [BoundingBox(c, aligned) for c in gc], "labels": gl})
            cls_pred.append({"pos": pos})
    return bb_pred, bb_gt, cls_pred


@pytest.mark.parametrize("on_device", [True, False], ids=["hbm", "host"])
@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_get_map_end_to_end(ops, path, on_device):
    from radargnn_amd.metrics import ObjectDetectionMetrics
    from radargnn_amd.postprocessor import PostProcessingConfiguration
    g = np.load(path)
    bb_pred, bb_gt, cls_pred = postprocessor_shaped(g, on_device)
    config = PostProcessingConfiguration(iou_for_mAP=0.3, use_point_iou=bool(g["use_point_iou"]))
    for tag, res in (("t1", ObjectDetectionMetrics.get_map(config, bb_pred, bb_gt, cls_pred)),
                     ("t3", ObjectDetectionMetrics._get_map(config, bb_pred, bb_gt, cls_pred, list(g["t3_thresholds"])))):
        assert res["classes"] == list(g[f"{tag}_classes"])
        for k in SUMMARIES:
            assert isinstance(res[k], torch.Tensor) and not res[k].is_cuda and res[k].dtype == torch.float32, k
            print(f"[map] {os.path.basename(path)} {tag} {k}: {res[k].numpy().reshape(-1)} want {g[f'{tag}_{k}']}")
            np.testing.assert_allclose(res[k].numpy().reshape(-1), g[f"{tag}_{k}"], rtol=0, atol=1e-6, err_msg=f"{tag} {k}")
        assert np.array_equal(res["precision"].numpy(), g[f"{tag}_precision"]) and np.array_equal(res["recall"].numpy(), g[f"{tag}_recall"])
        assert "map_small" not in res and "mar_large" not in res
    assert isinstance(res["map"].item(), float) and res["map_per_class"].detach().numpy().shape == (len(res["classes"]),)


def test_get_map_refusals_and_empty_frames(ops):
    from radargnn_amd import _lib
    from radargnn_amd.metrics import ObjectDetectionMetrics
    from radargnn_amd.postprocessor import BoundingBoxes, PostProcessingConfiguration
    g = np.load(os.path.join(GOLDEN, "eval_map_rotated_point.npz"))
    bb_pred, bb_gt, cls_pred = postprocessor_shaped(g)
    with pytest.raises(Exception, match="only Point-IOU based mAP calculation is possible for rotated bounding boxes"):
        ObjectDetectionMetrics.get_map(PostProcessingConfiguration(use_point_iou=False), bb_pred, bb_gt, cls_pred)
    # an empty first frame (the fixture's frame without detections or ground truth first) must not raise
    first = list(g["kinds"]).index("neither")
    order = [first] + [f for f in range(len(bb_pred)) if f != first]
    res = ObjectDetectionMetrics.get_map(PostProcessingConfiguration(use_point_iou=True), [bb_pred[f] for f in order], [bb_gt[f] for f in order],
                                         [cls_pred[f] for f in order])
    np.testing.assert_allclose(res["map"].numpy().reshape(-1), g["t1_map"], rtol=0, atol=1e-6)
    # nothing at all: every summary is -1
    empty = BoundingBoxes(torch.zeros((0, 4, 2), dtype=torch.float64, device="cuda"), True)
    none = torch.zeros(0, dtype=torch.float64, device="cuda")
    res = ObjectDetectionMetrics.get_map(PostProcessingConfiguration(use_point_iou=True), [{"boxes": empty, "scores": none, "labels": none}],
                                         [{"boxes": empty, "labels": none}], [{"pos": torch.zeros((5, 2), device="cuda")}])
    assert res["classes"] == [] and res["map"].item() == -1 and res["mar_100"].item() == -1 and res["map_per_class"].numel() == 0
    # more boxes of ONE class in one frame than the matching kernel holds: refused with a message, detections or ground truth
    cap = _lib.lib.rgnn_map_match_capacity()
    assert cap >= 1024
    n = cap + 1
    zeros = lambda m, dt=torch.int32: torch.zeros(m, dtype=dt, device="cuda")
    with pytest.raises(_lib.RgnnError, match="of one class per frame"):
        ops.map_match(zeros(n, torch.float32), [0, n], [0, 1], zeros(n), zeros(n, torch.float32), zeros(1), zeros(1), [0.5])
    with pytest.raises(_lib.RgnnError, match="of one class per frame"):
        ops.map_match(zeros(n, torch.float32), [0, 1], [0, n], zeros(1), zeros(1, torch.float32), zeros(n), zeros(1), [0.5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.map_match(torch.zeros(1), [0, 1], [0, 1], torch.zeros(1, dtype=torch.int32), torch.zeros(1), torch.zeros(1, dtype=torch.int32),
                      torch.zeros(1, dtype=torch.int32), [0.5])


def test_full_capacity_frame_matches_the_restatement(ops):
    """One frame at the kernel's capacity (2048 detections of one class, 2048 ground-truth boxes): ranks and flags against numpy."""
    from radargnn_amd import _lib
    cap = _lib.lib.rgnn_map_match_capacity()
    rng = np.random.default_rng(5)
    iou = rng.integers(0, 50, size=(cap, cap)).astype(np.float64) / 64.0            # many exact ties between candidates
    scores = (rng.permutation(cap) / cap).astype(np.float32)
    det_labels, gt_labels = np.zeros(cap, dtype=np.int64), (np.arange(cap) % 2).astype(np.int64)
    want_rank, want_matched = MO.match_frame(iou, det_labels, scores, gt_labels, [0, 1], [0.3, 0.7], 100)
    rank, matched = ops.map_match(dev(iou.reshape(-1)), [0, cap], [0, cap], dev(det_labels, torch.int32), dev(scores), dev(gt_labels, torch.int32),
                                  dev(np.array([0, 1]), torch.int32), [0.3, 0.7], 100)
    assert np.array_equal(rank.cpu().numpy(), want_rank) and np.array_equal(matched.cpu().numpy(), want_matched)


def test_frame_larger_than_the_capacity_spread_over_classes(ops):
    """The capacity is per (frame, class): a frame of 3 * 1100 detections and 3 * 1100 ground-truth boxes in three classes is
    accepted, between two small frames, and equals the numpy restatement."""
    rng = np.random.default_rng(9)
    sizes = [(5, 4), (3300, 3300), (7, 6)]
    ious, dl, ds, gl = [], [], [], []
    for p, g in sizes:
        ious.append(rng.integers(0, 40, size=(p, g)).astype(np.float32) / np.float32(64.0))
        dl.append(rng.permutation(p) % 3)
        gl.append(rng.permutation(g) % 3)
        ds.append((rng.permutation(p) / p).astype(np.float32))
    want_rank, want_matched = MO.match(ious, dl, ds, gl, [0, 1, 2], [0.3, 0.5], 100)
    ptr = lambda k: np.cumsum([0] + [s[k] for s in sizes]).tolist()
    rank, matched = ops.map_match(dev(np.concatenate([i.reshape(-1) for i in ious])), ptr(0), ptr(1), dev(np.concatenate(dl), torch.int32),
                                  dev(np.concatenate(ds)), dev(np.concatenate(gl), torch.int32), dev(np.arange(3), torch.int32), [0.3, 0.5], 100)
    assert np.array_equal(rank.cpu().numpy(), want_rank) and np.array_equal(matched.cpu().numpy(), want_matched)


def test_curves_with_classes_that_have_no_detections_or_are_not_asked_for(ops):
    """``classes`` need not cover the detections' labels and may name classes without detections: each curve reads its own class."""
    rng = np.random.default_rng(3)
    n = 6000                                                                      # more than one sort chunk
    dl, gl = rng.integers(0, 6, n), rng.integers(0, 8, 500)
    ds = (rng.permutation(n) / n).astype(np.float32)
    rank = rng.integers(-1, 100, n).astype(np.int32)
    matched = (rng.uniform(size=(2, n)) < 0.4).astype(np.uint8)
    classes = [1, 3, 4, 7]                                                        # 7: ground truth only; 0, 2, 5: not asked for
    want = MO.curves(dl, ds, rank, matched, gl, classes)
    got = ops.map_curves(dev(dl, torch.int32), dev(ds), dev(rank), dev(matched), dev(gl, torch.int32), dev(np.array(classes), torch.int32))
    for w, g in zip(want, got):
        assert np.array_equal(g.cpu().numpy(), w)


@pytest.mark.parametrize("tag", ["large", "small"])
def test_confusion_matrix_and_f1(ops, tag):
    from radargnn_amd.metrics import SegmentationMetrics
    g = np.load(os.path.join(GOLDEN, "eval_seg_confusion.npz"))
    n, k = int(g[f"{tag}_n"]), MO.SEG_CLASSES
    y_true, y_pred = MO.segmentation_labels(n)
    cm = ops.confusion_matrix(dev(y_true), dev(y_pred), k)
    assert cm.dtype == torch.int64 and np.array_equal(cm.cpu().numpy(), g[f"{tag}_confusion"])
    cut = n // 3                                                                     # two frames; predictions as [N, 1] columns
    seg = SegmentationMetrics([dev(y_pred[:cut]).view(-1, 1), dev(y_pred[cut:]).view(-1, 1)],
                              [{"labels": dev(y_true[:cut].astype(np.float32))}, {"labels": dev(y_true[cut:].astype(np.float32))}])
    assert np.array_equal(seg.get_confusion_matrix(k), g[f"{tag}_confusion"])
    assert np.array_equal(seg.get_confusion_matrices_per_class(k), g[f"{tag}_per_class"])
    for average in (None, "micro", "macro", "weighted"):
        got = seg.get_f1(k, average)
        print(f"[f1] {tag} {average}: {got}")
        np.testing.assert_allclose(got, g[f"{tag}_f1_{str(average).lower()}"], rtol=0, atol=1e-12, err_msg=str(average))
    host = SegmentationMetrics([y_pred.reshape(-1, 1)], [{"labels": y_true}])        # numpy in, uploaded once
    assert np.array_equal(host.get_confusion_matrix(k), g[f"{tag}_confusion"])


def test_confusion_matrix_edge_cases(ops):
    from radargnn_amd import _lib
    from radargnn_amd.metrics import SegmentationMetrics
    none = torch.zeros(0, dtype=torch.float64, device="cuda")
    assert not ops.confusion_matrix(none, none, 6).any() and ops.confusion_matrix(none, none, 6).shape == (6, 6)
    seg = SegmentationMetrics([], [])
    assert not seg.get_confusion_matrix(6).any() and not seg.get_f1(6, None).any() and seg.get_f1(6, "macro") == 0.0
    with pytest.raises(ValueError, match="NaN"):
        ops.confusion_matrix(torch.tensor([0.0, float("nan")], device="cuda"), torch.tensor([0.0, 1.0], device="cuda"), 6)
    with pytest.raises(_lib.RgnnError, match="at most 64 classes"):
        ops.confusion_matrix(none, none, 65)


def test_radarscenes_evaluator_writes_the_references_files(ops, tmp_path):
    from radargnn_amd.metrics import ObjectDetectionMetrics, SegmentationMetrics, evaluation_selector
    from radargnn_amd.postprocessor import PostProcessingConfiguration
    g = np.load(os.path.join(GOLDEN, "eval_map_aligned_point.npz"))
    bb_pred, bb_gt, cls_pred = postprocessor_shaped(g)
    names = {"car": 0.5, "pedestrian": 0.5, "group": 0.5, "two_wheeler": 0.5, "large_vehicle": 0.5}
    config = PostProcessingConfiguration(min_object_score=names, use_point_iou=True, bg_index=5, f1_class_averaging=None)
    fp = g["frame_ptr"]
    y_true, y_pred = MO.segmentation_labels(int(fp[-1]))
    y_true, y_pred = np.clip(y_true, 0, 5), np.clip(y_pred, 0, 5)
    cls_pred_label = [dev(y_pred[fp[f]:fp[f + 1]]).view(-1, 1) for f in range(len(fp) - 1)]
    cls_gt = [{"pos": c["pos"], "vel": None, "labels": dev(y_true[fp[f]:fp[f + 1]].astype(np.float32))} for f, c in enumerate(cls_pred)]
    ev = evaluation_selector["radarscenes"](config=config, version="v", dataset_path="d", model_path="m")
    assert ev.names == ["car", "pedestrian", "group", "two_wheeler", "large_vehicle", "background"]
    ev.evaluate(bb_pred, bb_gt, cls_pred, cls_pred_label, cls_gt, None, graph_names=["g"])
    direct = ObjectDetectionMetrics.get_map(config, bb_pred, bb_gt, cls_pred)
    seg = SegmentationMetrics(cls_pred_label, cls_gt)
    assert ev.mAP == direct["map"].item() and np.array_equal(ev.mAP_per_class, direct["map_per_class"].numpy())
    assert np.array_equal(ev.f1_segmentation, seg.get_f1(6, None)) and np.array_equal(ev.confusion_absolute, seg.get_confusion_matrix(6))
    assert np.array_equal(ev.confusion_absolute, MO.confusion_matrix(y_true, y_pred, 6))
    ev.save_results(str(tmp_path))
    ev.save_results(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["evaluation_01", "evaluation_02"]
    folder = tmp_path / "evaluation_01"
    assert sorted(os.listdir(folder)) == ["confusion_abs.npy", "convusion_rel.npy", "eval_configs.json", "eval_results.json"]
    cfg = json.load(open(folder / "eval_configs.json"))
    assert list(cfg) == ["EVALUATION_CONFIG"] and cfg["EVALUATION_CONFIG"]["iou_for_mAP"] == 0.3 and cfg["EVALUATION_CONFIG"]["use_point_iou"] is True
    out = json.load(open(folder / "eval_results.json"))
    assert list(out) == ["OBJECT_DETECTION_METRICS", "SEMANTIC_SEGMENTATION_METRICS"]
    assert out["OBJECT_DETECTION_METRICS"] == {"mAP": ev.mAP, "mAP_per_class": ev.mAP_per_class.tolist()}
    assert out["SEMANTIC_SEGMENTATION_METRICS"] == {"f1": ev.f1_segmentation.tolist()}
    absolute, relative = np.load(folder / "confusion_abs.npy"), np.load(folder / "convusion_rel.npy")
    assert np.array_equal(absolute, ev.confusion_absolute)
    sums = absolute.sum(axis=1, keepdims=True).astype(float)
    sums[sums == 0] = 1e-8
    assert np.array_equal(relative, absolute / sums)
    # averaged F1 is a plain number in the JSON; switched-off parts leave their keys out
    config2 = PostProcessingConfiguration(min_object_score=names, use_point_iou=True, get_mAP=False, get_confusion=False, f1_class_averaging="macro")
    ev2 = evaluation_selector["radarscenes"](config2)
    ev2.evaluate(bb_pred, bb_gt, cls_pred, cls_pred_label, cls_gt)
    ev2.save_results(str(tmp_path))
    out2 = json.load(open(tmp_path / "evaluation_03" / "eval_results.json"))
    assert out2 == {"OBJECT_DETECTION_METRICS": {}, "SEMANTIC_SEGMENTATION_METRICS": {"f1": float(seg.get_f1(6, "macro"))}}
    assert sorted(os.listdir(tmp_path / "evaluation_03")) == ["eval_configs.json", "eval_results.json"]
