"""Evaluation half on the device (csrc/postprocess.hip ground-truth decode, csrc/evaluate.hip duplicate removal and point
IoU, through radargnn_amd.postprocessor) against the reference-generated fixtures (tests/golden/make_eval_golden.py) and
the numpy restatement (tests/eval_oracle.py).  Labels, kept order and box counts exact; ground-truth corners within 1e-9
(device sin / cos / atan2 differ from the host's in the last ulps); duplicate removal fed the reference's corners and
every point IoU bit-exact."""
import glob
import os

import numpy as np
import pytest
import torch

import eval_oracle as E

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
GT = sorted(glob.glob(os.path.join(GOLDEN, "eval_gt_*.npz")))
IOU = sorted(glob.glob(os.path.join(GOLDEN, "eval_iou_*.npz")))
ATOL = 1e-9


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radargnn_amd import postprocessor
    return postprocessor


def frames_of(g):
    fp = g["frame_ptr"]
    return [tuple(g[k][fp[f]:fp[f + 1]] for k in ("pos", "labels", "boxes")) for f in range(len(fp) - 1)]


@pytest.mark.parametrize("path", GT, ids=[os.path.basename(p)[8:-4] for p in GT])
def test_ground_truth_matches_reference(P, path):
    g = np.load(path)
    inv, bg = str(g["invariance"]), int(g["bg_index"])
    dp, bp = g["decoded_ptr"], g["box_ptr"]
    for f, (pos, labels, boxes) in enumerate(frames_of(g)):
        bbs, lab = P.GroundTruthExtractor.get_absolute_object_bounding_boxes(labels, boxes, pos, inv, bg)
        assert len(bbs) == dp[f + 1] - dp[f] and bbs.is_aligned == (boxes.shape[1] == 4)
        assert lab.shape == (len(bbs), 1) and lab.dtype == torch.float32
        assert np.array_equal(lab.cpu().numpy().reshape(-1), g["decoded_labels"][dp[f]:dp[f + 1]])
        np.testing.assert_allclose(bbs.corners.cpu().numpy(), g["decoded"][dp[f]:dp[f + 1]], rtol=0, atol=ATOL)
        kept, klab = P.GroundTruthExtractor.remove_duplicate_boxes(bbs, lab)
        assert len(kept) == bp[f + 1] - bp[f] and klab.shape == (len(kept), 1)
        assert np.array_equal(klab.cpu().numpy().reshape(-1), g["box_labels"][bp[f]:bp[f + 1]])
        np.testing.assert_allclose(kept.corners.cpu().numpy(), g["corners"][bp[f]:bp[f + 1]], rtol=0, atol=ATOL)
        objects, seg = P.Postprocessor.process_one_ground_truth(pos, np.zeros_like(pos), boxes, labels, inv, bg)
        assert set(objects) == {"boxes", "labels"} and set(seg) == {"pos", "vel", "labels"}
        assert torch.equal(objects["boxes"].corners, kept.corners) and torch.equal(objects["labels"], klab[:, 0])
        assert np.array_equal(seg["labels"].cpu().numpy(), labels)


def test_duplicate_removal_bit_exact_on_reference_corners(P):
    """Reference corners straight in: the chain, inf, NaN, sums a few ulps either side of 0.1; then every fixture frame at
    once (one launch, frames by box offsets) against the reference's kept boxes."""
    from radargnn_amd import ops
    g = np.load(os.path.join(GOLDEN, "eval_dedup_adversarial.npz"))
    c = torch.from_numpy(g["corners"]).cuda()
    keep = ops.remove_duplicate_boxes(c, torch.tensor([0, c.shape[0]], dtype=torch.int64, device="cuda"))
    assert np.array_equal(np.nonzero(keep.cpu().numpy())[0], g["kept"])
    boxes, labels = P.GroundTruthExtractor.remove_duplicate_boxes(P.BoundingBoxes(c, True), g["labels"])
    assert np.array_equal(labels.cpu().numpy().reshape(-1).astype(np.int64), g["kept"])
    for path in GT:
        f = np.load(path)
        keep = ops.remove_duplicate_boxes(torch.from_numpy(f["decoded"]).cuda(), torch.from_numpy(f["decoded_ptr"]).cuda())
        assert np.array_equal(f["decoded"][keep.cpu().numpy().astype(bool)], f["corners"])


@pytest.mark.parametrize("seed", [0, 1])
def test_duplicate_removal_random_against_oracle(seed):
    """Frames of up to 700 boxes (several LDS tiles, blocks across frame borders) with clusters of near-duplicates at
    distances around 0.1, against the numpy restatement."""
    from radargnn_amd import ops
    rng = np.random.default_rng(seed)
    sizes = [0, 700, 1, 300, 257, 0, 40]
    frames = []
    for n in sizes:
        centres = rng.uniform(-30, 30, size=(max(n // 6, 1), 1, 2))
        c = centres[rng.integers(0, len(centres), size=n)] + rng.normal(0, 0.012, size=(n, 4, 2))
        c[rng.random(n) < 0.1] = c[0] if n else 0
        frames.append(c.reshape(n, 4, 2))
    corners = np.concatenate(frames)
    ptr = np.cumsum([0] + sizes)
    keep = ops.remove_duplicate_boxes(torch.from_numpy(corners).cuda(), torch.from_numpy(ptr).cuda()).cpu().numpy().astype(bool)
    expect = np.concatenate([E.duplicate_keep(fr) for fr in frames])
    assert np.array_equal(keep, expect)
    assert 0 < expect.sum() < len(expect)


@pytest.mark.parametrize("path", IOU, ids=[os.path.basename(p)[9:-4] for p in IOU])
def test_point_iou_matches_reference(P, path):
    g = np.load(path)
    aligned = bool(g["aligned"])
    pts, pred, gt, ious = (E.split(g[k], g[k + "_ptr"] if k != "points" else g["frame_ptr"]) for k in ("points", "pred", "gt", "iou"))
    batched = P.point_iou_batched(pred, gt, pts, aligned)
    for f in range(len(pts)):
        one = P.point_iou(pred[f], gt[f], pts[f], aligned)
        assert one.dtype == torch.float64 and one.shape == (len(pred[f]), len(gt[f]))
        assert np.array_equal(one.cpu().numpy().reshape(-1), ious[f]), f
        assert torch.equal(batched[f], one)


@pytest.mark.parametrize("aligned", [True, False])
def test_point_iou_random_against_oracle(P, aligned):
    """A 3000-point frame (sort over more points than threads, words across waves) with repeated coordinates and signed
    zeros, beside small frames, against the numpy restatement."""
    rng = np.random.default_rng(7 if aligned else 8)
    pts, pred, gt = [], [], []
    for n, np_, ng in [(3000, 16, 11), (65, 4, 3), (64, 2, 5)]:
        p = np.round(rng.uniform(-20, 20, size=(n, 2)), 1).astype(np.float32)   # a 0.1 grid: many repeated coordinates
        p[::50] = -0.0 * p[::50]
        boxes = []
        for _ in range(np_ + ng):
            c = rng.uniform(-15, 15, size=2); l, w = rng.uniform(2, 14), rng.uniform(1, 9)
            boxes.append([c[0] - l / 2, c[1] - w / 2, c[0] + l / 2, c[1] + w / 2] if aligned else [c[0], c[1], l, w, rng.uniform(0, 180)])
        boxes = np.array(boxes, dtype=np.float32)
        if not aligned:                                       # keep off the area test's threshold (see make_eval_golden.py)
            bad = np.zeros(n, dtype=bool)
            for b in boxes:
                cr = E.box_corners(b)
                bad |= np.array([abs(E.area_slack(cr, q) - 1e-6) < 1e-9 for q in p.astype(np.float64)])
            p = p[~bad]
        pts.append(p); pred.append(boxes[:np_]); gt.append(boxes[np_:])
    out = P.point_iou_batched(pred, gt, pts, aligned)
    for f in range(len(pts)):
        assert np.array_equal(out[f].cpu().numpy(), E.point_iou(pred[f], gt[f], pts[f], aligned)), f


def test_point_iou_edges_and_empty(P):
    pts = np.array([[0, 0], [2, 2], [-0.0, 1], [0.0, 1], [1, -0.0]], dtype=np.float32)
    box = np.array([[0, 0, 2, 2]], dtype=np.float32)
    assert P.point_iou(box, box, pts, True).item() == 4 / 6              # (0, 1) twice: tp 4 distinct, fp = fn = 5 - 4
    assert P.point_iou(box, np.array([[5, 5, 6, 6]], np.float32), pts, True).item() == 0.0
    assert P.point_iou(np.array([[5, 5, 6, 6]], np.float32), np.array([[7, 7, 8, 8]], np.float32), pts, True).item() == 0.00001
    assert P.point_iou(np.zeros((0, 4), np.float32), box, pts, True).shape == (0, 1)
    assert P.point_iou(box, np.zeros((0, 5), np.float32).reshape(0, 4), pts, True).shape == (1, 0)
    rot = np.array([[1, 1, 2, 2, 0]], dtype=np.float32)
    assert P.point_iou(rot, rot, np.zeros((0, 2), np.float32), False).item() == 0.00001


def synthetic_batch(rng, width, invariance, n_frames=4):
    pos, vel, bb, prob, bbt, clt = [], [], [], [], [], []
    for f in range(n_frames):
        n = [120, 0, 75, 200][f % 4]
        pos.append(rng.uniform(-30, 60, size=(n, 2)).astype(np.float32))
        vel.append(rng.normal(size=(n, 2)).astype(np.float32))
        logits = rng.normal(size=(n, 6)) * 2
        prob.append((np.exp(logits) / np.exp(logits).sum(1, keepdims=True)).astype(np.float32))
        b = rng.normal(size=(n, width)).astype(np.float32)
        b[:, 2:4] = np.abs(b[:, 2:4]) * 2 + 0.5
        bb.append(b)
        obj = rng.integers(0, 8, size=n)                     # points of one object share (almost) one absolute box
        centre = rng.uniform(-30, 60, size=(8, 2))
        t = np.zeros((n, width), dtype=np.float32)
        t[:, 2:4] = [3.0, 1.5]
        t[:, :2] = (centre[obj] - pos[-1]) if invariance != "none" else centre[obj]
        if width == 5:
            t[:, 4] = 0.3 * obj
        bbt.append(t)
        clt.append(np.where(obj < 6, obj % 5, 5).astype(np.float32))
    return pos, vel, {"bounding_box_predictions": bb, "class_probability_prediction": prob}, \
        {"bounding_box_true": bbt, "class_true": clt}


@pytest.mark.parametrize("width,inv", [(4, "translation"), (5, "translation"), (5, "none"), (5, "en")])
def test_process_matches_per_frame_calls(P, width, inv):
    rng = np.random.default_rng(width + len(inv))
    pos, vel, pred, truth = synthetic_batch(rng, width, "none" if inv == "none" else "translation")
    if inv == "en":
        pos[1] = rng.uniform(0, 5, size=(3, 2)).astype(np.float32)         # no empty frame: the en half needs neighbours
        for d, k in ((pred, "bounding_box_predictions"), (pred, "class_probability_prediction"), (truth, "bounding_box_true")):
            d[k][1] = np.abs(rng.normal(size=(3, d[k][0].shape[1]))).astype(np.float32)
        truth["class_true"][1] = np.array([0, 5, 2], dtype=np.float32)
        vel[1] = np.zeros((3, 2), np.float32)
    cfg = P.PostProcessingConfiguration(iou_for_nms=0.3, min_object_score={f"c{i}": 0.3 for i in range(5)},
                                        max_score_for_background=0.4, bg_index=5, bb_invariance=inv)
    bb_pred, bb_gt, cls_pred, cls_gt = P.Postprocessor().process(cfg, pos, vel, pred, truth)
    assert len(bb_pred) == len(bb_gt) == len(cls_pred) == len(cls_gt) == len(pos)
    for f in range(len(pos)):
        assert set(bb_pred[f]) == {"boxes", "scores", "labels"} and set(cls_pred[f]) == {"pos", "labels", "scores", "clutter_scores"}
        assert set(bb_gt[f]) == {"boxes", "labels"} and set(cls_gt[f]) == {"pos", "vel", "labels"}
        det, seg = P.Postprocessor.process_one_raw_prediction(cfg, pos[f], pred["bounding_box_predictions"][f],
                                                              pred["class_probability_prediction"][f])
        assert torch.equal(bb_pred[f]["boxes"].corners, det["boxes"].corners)
        for k in ("scores", "labels"):
            assert torch.equal(bb_pred[f][k], det[k])
        for k in seg:
            assert torch.equal(cls_pred[f][k], seg[k])
        obj, gseg = P.Postprocessor.process_one_ground_truth(pos[f], vel[f], truth["bounding_box_true"][f],
                                                             truth["class_true"][f], inv, 5)
        assert torch.equal(bb_gt[f]["boxes"].corners, obj["boxes"].corners) and bb_gt[f]["boxes"].is_aligned == (width == 4)
        assert torch.equal(bb_gt[f]["labels"], obj["labels"]) and bb_gt[f]["labels"].dtype == torch.float32
        for k in gseg:
            assert torch.equal(cls_gt[f][k], gseg[k])
        if len(pos[f]) and inv != "en":
            assert 0 < len(obj["boxes"]) <= 6                 # one box per object survives
    labels = P.PredictionExtractor().extract(pred)
    for f in range(len(pos)):
        assert torch.equal(labels[f], P.PredictionExtractor.get_predicted_label(pred["class_probability_prediction"][f]))


def test_errors_match_reference(P):
    one = np.zeros((1, 2), np.float32)
    with pytest.raises(ValueError, match="n_samples_fit"):
        P.GroundTruthExtractor.get_absolute_object_bounding_boxes(np.zeros(1, np.float32), np.ones((1, 5), np.float32), one, "en", 5)
    with pytest.raises(ValueError, match="n_samples_fit"):     # the reference searches neighbours for aligned boxes too
        P.GroundTruthExtractor.get_absolute_object_bounding_boxes(np.zeros(1, np.float32), np.ones((1, 4), np.float32), one, "en", 5)
    bbs, lab = P.GroundTruthExtractor.get_absolute_object_bounding_boxes(np.zeros(0, np.float32), np.zeros((0, 5), np.float32),
                                                                         np.zeros((0, 2), np.float32), "en", 5)
    assert len(bbs) == 0 and lab.shape == (0, 1)
    with pytest.raises(ValueError):
        P.GroundTruthExtractor.get_absolute_object_bounding_boxes(np.zeros(3, np.float32), np.ones((3, 5), np.float32),
                                                                  np.zeros((3, 2), np.float32), "bogus", 5)


def test_shim_exports_ground_truth_extractor():
    from gnnradarobjectdetection.postprocessor import postprocessing
    from radargnn_amd import postprocessor
    assert postprocessing.GroundTruthExtractor is postprocessor.GroundTruthExtractor
    assert hasattr(postprocessing.Postprocessor, "process") and hasattr(postprocessing.PredictionExtractor, "extract")
