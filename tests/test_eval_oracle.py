"""The numpy restatement of the evaluation half (tests/eval_oracle.py) against the reference-generated fixtures
(tests/golden/eval_*.npz, tests/golden/make_eval_golden.py).  CPU only."""
import glob
import os

import numpy as np
import pytest
from sklearn.neighbors import kneighbors_graph

import eval_oracle as E

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
GT = sorted(glob.glob(os.path.join(GOLDEN, "eval_gt_*.npz")))
IOU = sorted(glob.glob(os.path.join(GOLDEN, "eval_iou_*.npz")))


@pytest.mark.parametrize("path", GT, ids=[os.path.basename(p)[8:-4] for p in GT])
def test_ground_truth_oracle_matches_reference(path):
    g = np.load(path)
    inv, bg = str(g["invariance"]), int(g["bg_index"])
    fp, dp, bp = g["frame_ptr"], g["decoded_ptr"], g["box_ptr"]
    for f in range(len(fp) - 1):
        pos, labels, boxes = (g[k][fp[f]:fp[f + 1]] for k in ("pos", "labels", "boxes"))
        nn = None
        if inv == "en" and len(pos) > 1:
            nn = np.where(kneighbors_graph(pos.astype(np.float64), 1, include_self=False).toarray() == 1)[1]
        corners, lab, _ = E.ground_truth_boxes(labels, boxes, pos, bg, inv, nn)
        np.testing.assert_allclose(corners, g["decoded"][dp[f]:dp[f + 1]], rtol=0, atol=1e-12)
        assert np.array_equal(lab.reshape(-1), g["decoded_labels"][dp[f]:dp[f + 1]]) and lab.dtype == np.float32
        ref = g["decoded"][dp[f]:dp[f + 1]]
        keep = E.duplicate_keep(ref)
        assert np.array_equal(ref[keep], g["corners"][bp[f]:bp[f + 1]])
        assert np.array_equal(g["decoded_labels"][dp[f]:dp[f + 1]][keep], g["box_labels"][bp[f]:bp[f + 1]])


def test_duplicate_oracle_matches_reference_adversarial():
    g = np.load(os.path.join(GOLDEN, "eval_dedup_adversarial.npz"))
    assert np.array_equal(np.nonzero(E.duplicate_keep(g["corners"]))[0], g["kept"])
    assert not {1, 2} & set(g["kept"].tolist())            # the chain A ~ B ~ C drops B and C


@pytest.mark.parametrize("path", IOU, ids=[os.path.basename(p)[9:-4] for p in IOU])
def test_point_iou_oracle_matches_reference(path):
    g = np.load(path)
    aligned = bool(g["aligned"])
    for f, (pts, pred, gt, iou) in enumerate(zip(E.split(g["points"], g["frame_ptr"]), E.split(g["pred"], g["pred_ptr"]),
                                                 E.split(g["gt"], g["gt_ptr"]), E.split(g["iou"], g["iou_ptr"]))):
        out = E.point_iou(pred, gt, pts, aligned)
        assert np.array_equal(out.reshape(-1), iou), f
    assert g["iou"][-1] == 1 / 3                            # two equal points inside both boxes
    assert (g["iou"] == 0.00001).any()
