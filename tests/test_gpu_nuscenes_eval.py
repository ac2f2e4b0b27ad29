"""The nuScenes evaluator on the device (csrc/nuscenes_eval.hip through radargnn_amd.ops and radargnn_amd.nuscenes_eval) against
tests/nuscenes_eval_oracle.py: masks, matches and orders exact; float64 outputs within BARS.

Tolerances.  Nobody derived a bound for the device's sin / cos / atan2 / sqrt and the reassociated running sums against numpy's, so
the bars are MEASURED: the worst error of each kind of output over this file's cases on an MI355X, times 16 (the figures are in
MEASUREMENTS.md; every run prints and records its own with conftest.record_parity).  The error is |got - want| / max(|want|, 1):
relative for magnitudes above 1, absolute below (most outputs pass through 0).  A real defect -- a wrong interval, a wrong tie --
is many orders larger.  NaN must sit where the oracle has NaN."""
import json
import math
import os

import numpy as np
import pytest
import torch

import nuscenes_eval_cases as cases
import nuscenes_eval_oracle as oracle
from conftest import record_parity

pytestmark = pytest.mark.gpu

# 16 x the worst error measured on an MI355X (MEASUREMENTS.md section 8j): 1.11e-16 (the rotation's cos / sin), 1.78e-15 (orient_err:
# two atan2 and a modulo), 1.05e-15 (the resampled running means), 2.23e-16 (a mean of 90 table entries)
BARS = {"submission": 16 * 1.11e-16, "tp_err": 16 * 1.78e-15, "tables": 16 * 1.05e-15, "summary": 16 * 2.23e-16}
CHUNK = 256                                                                              # CURVE_THREADS of csrc/nuscenes_eval.hip


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radargnn_amd import ops
    return ops


@pytest.fixture(scope="module")
def ne(ops):
    from radargnn_amd import nuscenes_eval
    return nuscenes_eval


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def err_of(got, want) -> float:
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern differs"
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1.0)))


def held(name: str, kind: str, **errors) -> None:
    record_parity("nuscenes_eval " + name, **errors, bar=BARS[kind])
    assert all(e <= BARS[kind] for e in errors.values()), (name, errors, BARS[kind])


def eval_dict(b: dict, keep=None) -> dict:
    d = {"translation": dev(b["translation"]), "size": dev(b["size"]), "rotation": dev(b["rotation"]), "velocity": dev(b["velocity"]),
         "name": dev(b["name"], torch.int32), "attribute": dev(b["attribute"], torch.int32), "ptr": dev(b["ptr"], torch.int64)}
    n = len(b["name"])
    d["keep"] = dev(np.ones(n, dtype=np.uint8) if keep is None else np.asarray(keep, dtype=np.uint8))
    return d


def classes_dev():
    return dev(np.array([oracle.code(n) for n in oracle.DETECTION_NAMES], dtype=np.int32))


def device_match(ops, pred, gt, keep_p=None, keep_g=None):
    order = ops.sample_score_order(dev(pred["score"]), dev(pred["ptr"], torch.int64)) if len(pred["score"]) else \
        torch.empty(0, dtype=torch.int64, device="cuda")
    match, tp_err, status = ops.center_match(eval_dict(pred, keep_p), eval_dict(gt, keep_g), order, classes_dev(), oracle.DIST_THS, 2,
                                             oracle.code('barrier'))
    return match.cpu().numpy(), tp_err.cpu().numpy(), int(status.item()), order.cpu().numpy()


# ---- submission ------------------------------------------------------------------------------------------------------------------
POSES = [np.array([1.0, 0.0, 0.0, 0.0]), cases.yaw_quat(0.7) * 1.7, cases.yaw_quat(-2.1, 0.05, -0.03)]


@pytest.mark.parametrize("m", [0, 1, 257])
def test_submission_against_the_oracle(ops, ne, m):
    rng = np.random.default_rng(m)
    s = 7                                                                                # samples 1 and 4 are empty
    cuts = np.sort(rng.integers(0, m + 1, 4))
    ptr = np.array([0, cuts[0], cuts[0], cuts[1], cuts[2], cuts[2], cuts[3], m], dtype=np.int64)
    boxes = np.column_stack((rng.uniform(-60, 60, m), rng.uniform(-60, 60, m), rng.uniform(0.3, 12, m), rng.uniform(0.3, 3, m),
                             rng.uniform(0, 180, m)))
    boxes[:3, 4] = [0.0, 90.0, 179.999][:min(m, 3)]
    labels = rng.integers(1, 11, m).astype(np.int32)
    ego_r = np.array([POSES[i % 3] for i in range(s)])
    ego_t = np.column_stack((rng.uniform(300, 1800, s), rng.uniform(300, 1800, s), rng.uniform(-2, 2, s)))
    heights = dev(np.array(oracle.HEIGHTS))
    got = ops.nuscenes_submission(dev(boxes).reshape(-1, 5), dev(labels), dev(ptr), dev(ego_t), dev(ego_r), heights)
    assert int(got[4].item()) == 0
    want = oracle.submission(boxes, labels, ptr, ego_t, ego_r)
    errs = {k: err_of(g.cpu().numpy(), w) for k, g, w in zip(("translation", "size", "rotation", "yaw"), got[:4], want)}
    assert errs["size"] == 0.0
    held(f"submission m={m}", "submission", **errs)


def test_submission_refuses_a_label_without_a_name(ops, ne):
    from radargnn_amd.postprocessor import BoundingBoxes
    corners = dev(np.array([[[1.0, 1.0], [1.0, 3.0], [5.0, 3.0], [5.0, 1.0]]] * 2))
    ego_t, ego_r = np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0, 0.0]])
    for bad in (0.0, 11.0, -1.0):
        frame = {"boxes": BoundingBoxes(corners, False), "labels": dev(np.array([4.0, bad])), "scores": dev(np.array([0.5, 0.25]))}
        with pytest.raises(ValueError, match="void"):
            ne.get_submission([frame], [None], ["graph_tok.pt"], ego_t, ego_r)
    frame = {"boxes": BoundingBoxes(corners, False), "labels": dev(np.array([4.0, 10.0])), "scores": dev(np.array([0.5, 0.25], dtype=np.float32))}
    sub = ne.get_submission([frame], [None], ["graph_tok.pt"], ego_t, ego_r)
    assert list(sub) == ["meta", "results"] and [r["detection_name"] for r in sub["results"]["tok"]] == ["car", "truck"]
    _, rotated = ops.box_representations(corners, two_point=False, rotated=True)
    want = oracle.submission(rotated.cpu().numpy(), [4, 10], [0, 2], ego_t, ego_r)
    rec = sub["results"]["tok"][1]
    assert rec["size"] == tuple(want[1][1]) and rec["detection_score"] == 0.25 and rec["velocity"] == (0.0, 0.0)
    held("get_submission", "submission", translation=err_of(rec["translation"], want[0][1]), rotation=err_of(rec["rotation"], want[2][1]))


# ---- filter ----------------------------------------------------------------------------------------------------------------------
def device_filter(ops, b, ego, is_gt, racks=None, max_boxes=0):
    cr = dev(np.array([0.0] + [float(oracle.CLASS_RANGE[n]) for n in oracle.LABEL_NAMES[1:]]))
    r = None if racks is None else (dev(racks[0]), dev(racks[1]), dev(racks[2]), dev(racks[3], torch.int64))
    keep, status = ops.detection_filter(dev(b["translation"]), dev(b["name"], torch.int32), dev(b["ptr"], torch.int64), dev(ego), cr,
                                        oracle.code('bicycle'), oracle.code('motorcycle'),
                                        num_pts=dev(b["num_pts"], torch.int32) if is_gt else None,
                                        score=None if is_gt else dev(b["score"]), max_boxes=max_boxes, racks=r)
    return keep.cpu().numpy().astype(bool), int(status.item())


def test_filter_range_is_strict_and_points_are_needed(ops):
    ego = np.array([[600.0, 1600.0, 0.0], [0.0, 0.0, 0.0]])
    names = ['car', 'car', 'pedestrian', 'pedestrian', 'traffic_cone', 'traffic_cone', 'car', 'void', 'car']
    off = [(30, 40), (30, 39.75), (24, 32), (23.5, 32), (18, 24), (18, 23.75), (1, 1), (1, 1), (-30, -40)]      # 3-4-5 triangles: exact
    xy = [(600.0 + x, 1600.0 + y) for x, y in off[:6]] + [(1.0, 1.0), (1.0, 1.0), (-30.0, -40.0)]
    gt = cases.simple(names, xy, ptr=[0, 6, 9], ego=ego, num_pts=[1, 1, 1, 1, 1, 1, 0, 1, 1])
    gt["name"][7] = 0
    want = oracle.filter_boxes(gt, ego, is_gt=True)
    assert want.tolist() == [False, True, False, True, False, True, False, False, False]
    got, status = device_filter(ops, gt, ego, True)
    assert got.tolist() == want.tolist() and status == 0
    pred = cases.simple(names[:7], xy[:7], ptr=[0, 6, 7], score=np.linspace(0.1, 0.7, 7))
    got, status = device_filter(ops, pred, ego, False, max_boxes=500)
    assert got.tolist() == oracle.filter_boxes(pred, ego).tolist() == [False, True, False, True, False, True, True] and status == 0


def test_filter_bike_racks(ops):
    ego = np.zeros((2, 3))
    racks = (np.array([[10.0, 10.0, 0.0], [-10.0, 0.0, 0.0]]), np.array([[2.0, 4.0, 2.0], [2.0, 2.0, 2.0]]),
             np.array([[1.0, 0.0, 0.0, 0.0], cases.yaw_quat(math.pi / 4)]), np.array([0, 2, 2]))      # x 8..12, y 9..11, z -1..1
    names = ['bicycle', 'bicycle', 'bicycle', 'bicycle', 'car', 'motorcycle', 'bicycle', 'bicycle', 'bicycle']
    pts = [(10, 10, 0), (12, 10, 0), (12.5, 10, 0), (10, 10, 1.5), (10, 10, 0), (8, 9, -1), (-10, 1.25, 0), (-10, 1.5, 0), (10, 10, 0)]
    b = cases.simple(names, [(p[0], p[1]) for p in pts], ptr=[0, 8, 9], ego=ego)
    b["translation"][:, 2] = [p[2] for p in pts]
    want = oracle.filter_boxes(b, ego, racks=racks, is_gt=True)
    # inside, on the edge, outside, above, a car, a motorcycle on a corner, inside / outside the turned rack, a rack-less sample
    assert want.tolist() == [False, False, True, True, True, False, False, True, True]
    got, status = device_filter(ops, b, ego, True, racks=racks)
    assert got.tolist() == want.tolist() and status == 0
    b["score"] = np.full(9, 0.5)
    assert device_filter(ops, b, ego, False, racks=racks)[0].tolist() == want.tolist()


def test_filter_status_bits(ops, ne):
    gt = cases.simple(['car'], [(1.0, 1.0)])
    for n, bit in ((500, 0), (501, ops.STATUS_NUSC_EVAL_TOO_MANY_BOXES)):
        pred = cases.simple(['car'] * n, [(float(i % 20), float(i // 20)) for i in range(n)], score=np.linspace(0.1, 0.9, n))
        assert device_filter(ops, pred, gt["ego_translation"], False, max_boxes=500)[1] == bit
        if bit:
            with pytest.raises(ValueError, match="boxes per sample"):
                ne.detection_eval(cases.device_predictions(pred), cases.device_ground_truth(gt))
        else:
            assert 0.0 <= ne.detection_eval(cases.device_predictions(pred), cases.device_ground_truth(gt))["nd_score"] <= 1.0
    pred = cases.simple(['car', 'car'], [(1.0, 1.0), (2.0, 2.0)], score=[0.5, float("nan")])
    assert device_filter(ops, pred, gt["ego_translation"], False)[1] == ops.STATUS_NUSC_EVAL_NAN_SCORE
    with pytest.raises(ValueError, match="NaN"):
        ne.detection_eval(cases.device_predictions(pred), cases.device_ground_truth(gt))
    pred = cases.simple(['car', 'void'], [(1.0, 1.0), (2.0, 2.0)], score=[0.5, 0.25])
    keep, status = device_filter(ops, pred, gt["ego_translation"], False)
    assert keep.tolist() == [True, False] and status == ops.STATUS_NUSC_EVAL_BAD_LABEL
    with pytest.raises(ValueError, match="no nuScenes detection class"):
        ne.detection_eval(cases.device_predictions(pred), cases.device_ground_truth(gt))


# ---- match -----------------------------------------------------------------------------------------------------------------------
def sized_match_case(ng: int, n_pred: int, seed: int):
    """Sample 0: ng cars and n_pred car predictions; sample 1: empty; sample 2: a few boxes of three classes."""
    rng = np.random.default_rng(seed)
    g_xy = rng.uniform(-40, 40, (ng, 2))
    near = g_xy[rng.integers(0, ng, n_pred)] + rng.normal(0, 1.2, (n_pred, 2)) if ng else rng.uniform(-40, 40, (n_pred, 2))
    names2 = ['car', 'barrier', 'pedestrian', 'barrier', 'car']
    g2 = rng.uniform(-20, 20, (5, 2))
    p2 = g2[[1, 0, 3, 2, 4, 0]] + rng.normal(0, 0.6, (6, 2))
    rot = lambda n: [cases.yaw_quat(a) for a in rng.uniform(-math.pi, math.pi, n)]
    gt = cases.boxes(np.column_stack((np.vstack((g_xy, g2)), np.zeros(ng + 5))), rng.uniform(0.5, 5, (ng + 5, 3)), rot(ng + 5),
                     rng.normal(0, 2, (ng + 5, 2)), [oracle.code('car')] * ng + [oracle.code(n) for n in names2],
                     rng.integers(-1, 8, ng + 5), [0, ng, ng, ng + 5])
    pn = [oracle.code('car')] * n_pred + [oracle.code(n) for n in ('barrier', 'car', 'barrier', 'pedestrian', 'car', 'truck')]
    pred = cases.boxes(np.column_stack((np.vstack((near, p2)), np.zeros(n_pred + 6))), rng.uniform(0.5, 5, (n_pred + 6, 3)), rot(n_pred + 6),
                       np.zeros((n_pred + 6, 2)), pn, [oracle.PRED_ATTRIBUTE[oracle.LABEL_NAMES[c]] for c in pn],
                       [0, n_pred, n_pred, n_pred + 6], score=np.round(rng.uniform(0.05, 1.0, n_pred + 6), 2))
    return pred, gt


@pytest.mark.parametrize("ng,n_pred", [(0, 2), (1, 0), (1, 1), (63, 2), (64, 500), (65, 2), (512, 64)])
def test_match_sizes_against_the_oracle(ops, ng, n_pred):
    assert ops.center_match_capacity() == 512
    pred, gt = sized_match_case(ng, n_pred, 100 + ng)
    ones_p, ones_g = np.ones(len(pred["name"]), dtype=bool), np.ones(len(gt["name"]), dtype=bool)
    want_match, want_err = oracle.match_boxes(pred, gt, ones_p, ones_g)
    match, tp_err, status, _ = device_match(ops, pred, gt)
    assert status == 0 and np.array_equal(match, want_match)
    assert (want_match[:, n_pred:] >= 0).any()
    held(f"match ng={ng} np={n_pred}", "tp_err", **{name: err_of(tp_err[e], want_err[e]) for e, name in enumerate(oracle.TP_METRICS)})


def test_match_over_capacity_sets_the_status_bit(ops, ne):
    pred, gt = sized_match_case(513, 2, 7)
    match, _, status, _ = device_match(ops, pred, gt)
    assert status == ops.STATUS_NUSC_EVAL_GT_OVERFLOW and (match[:, :2] == -1).all() and (match[:, 2:] >= 0).any()
    keep = np.ones(518, dtype=bool)
    keep[5] = False                                                                      # 512 KEPT boxes fit
    assert device_match(ops, pred, gt, keep_g=keep)[2] == 0
    from radargnn_amd._lib import RgnnError
    gt.update(num_pts=np.ones(518, dtype=np.int32), ego_translation=np.zeros((3, 3)))
    gt["translation"], pred["translation"] = gt["translation"] * 0.5, pred["translation"] * 0.5          # all 513 inside the car range
    with pytest.raises(RgnnError, match="512"):
        ne.detection_tables(cases.device_predictions(pred), cases.device_ground_truth(gt))


def test_match_ties_thresholds_and_taken_boxes(ops):
    # sample 0: a distance exactly equal to each threshold is no match at it (and is one at the next)
    g0, p0 = [(0, 0), (10, 0), (20, 0), (30, 0)], [(0.5, 0), (11, 0), (22, 0), (34, 0)]
    # sample 1: two equidistant boxes, equal scores -- the later prediction goes first and takes the lower box
    g1, p1 = [(0, 1), (0, -1)], [(0, 0), (0, 0)]
    # sample 2: the nearest box is taken, the next nearest is used
    g2, p2 = [(0, 0), (1.5, 0)], [(0.1, 0), (0.2, 0)]
    # sample 3: at 0.5 P0 misses B (0.6) and P1 takes it; at 1.0 P0 takes B and P1 is left with A at 1.2: no match
    g3, p3 = [(0, 0), (1.3, 0)], [(0.7, 0), (1.2, 0)]
    gt = cases.simple(['car'] * 10, g0 + g1 + g2 + g3, ptr=[0, 4, 6, 8, 10], ego=np.zeros((4, 3)))
    pred = cases.simple(['car'] * 10, p0 + p1 + p2 + p3, ptr=[0, 4, 6, 8, 10], score=[0.9, 0.8, 0.7, 0.6, 0.5, 0.5, 0.9, 0.8, 0.9, 0.8])
    want, _ = oracle.match_boxes(pred, gt, np.ones(10, dtype=bool), np.ones(10, dtype=bool))
    assert want.tolist() == [[-1, -1, -1, -1, -1, -1, 6, -1, -1, 9],
                             [0, -1, -1, -1, -1, -1, 6, -1, 9, -1],
                             [0, 1, -1, -1, 5, 4, 6, 7, 9, 8],
                             [0, 1, 2, -1, 5, 4, 6, 7, 9, 8]]
    match, _, status, order = device_match(ops, pred, gt)
    assert status == 0 and match.tolist() == want.tolist()
    assert order.tolist() == [0, 1, 2, 3, 5, 4, 6, 7, 8, 9]                               # equal scores: the later position first


def test_match_tp_errors_at_the_angle_seams(ops):
    yaw_g = [3.1, -3.1, 0.1, 0.1, 1.0, -2.0, 0.0]
    yaw_p = [-3.1, 3.1, 0.1 + math.pi - 0.05, 0.1 - math.pi + 0.05, 1.0 + math.pi / 2, 2.0, math.pi]
    names = ['car', 'car', 'barrier', 'barrier', 'barrier', 'pedestrian', 'car']
    xy = [(5.0 * i, 0.0) for i in range(7)]
    gt = cases.simple(names, xy, yaw=yaw_g, attribute=[5, -1, -1, 3, -1, 2, 6], velocity=[[1, 2], [np.nan, np.nan], [0, 0], [0, 0], [0, 0], [3, -4], [0, 0]],
                      size=[[2, 4, 1.5]] * 6 + [[1, 5, 2]])
    pred = cases.simple(names, [(x + 0.25, y) for x, y in xy], yaw=yaw_p, score=np.linspace(0.9, 0.3, 7))
    want_match, want = oracle.match_boxes(pred, gt, np.ones(7, dtype=bool), np.ones(7, dtype=bool))
    assert want_match[2].tolist() == list(range(7))
    np.testing.assert_allclose(want[2], [0.083185307179586, 0.083185307179586, 0.05, 0.05, math.pi / 2, 2 * math.pi - 4.0, math.pi], atol=1e-12)
    assert np.isnan(want[4, [1, 2, 4]]).all() and want[4, [0, 3, 5, 6]].tolist() == [0.0, 1.0, 0.0, 1.0]
    assert want[3, 0] == pytest.approx(math.sqrt(5)) and np.isnan(want[3, 1]) and want[3, 5] == 5.0
    assert want[1, 6] == pytest.approx(1 - 6 / (12 + 10 - 6)) and want[1, 0] == 0.0
    match, tp_err, status, _ = device_match(ops, pred, gt)
    assert status == 0 and np.array_equal(match, want_match)
    held("match angle seams", "tp_err", **{name: err_of(tp_err[e], want[e]) for e, name in enumerate(oracle.TP_METRICS)})


# ---- curves ----------------------------------------------------------------------------------------------------------------------
def curve_case(n: int, npos: int, seed: int, p_match: float = 0.5, attr: str = "mixed"):
    """n car predictions with random match flags (plateaus of recall wherever a miss follows), npos car ground-truth boxes; 3
    pedestrian predictions without any ground truth; 2 buses in the ground truth without a prediction."""
    rng = np.random.default_rng(seed)
    m = n + 3
    names = ['car'] * n + ['pedestrian'] * 3
    pred = cases.simple(names, rng.uniform(-5, 5, (m, 2)), score=np.round(rng.uniform(0.01, 1.0, m), 2))
    gt = cases.simple(['car'] * npos + ['bus'] * 2, rng.uniform(-5, 5, (npos + 2, 2)))
    match = np.where(rng.random((4, m)) < p_match, rng.integers(0, max(npos, 1), (4, m)), -1).astype(np.int32)
    match[:, n:] = -1
    if npos == 0:
        match[:] = -1
    tp_err = np.full((5, m), np.nan)
    hit = match[2] >= 0
    tp_err[:, hit] = rng.uniform(0, 2, (5, int(hit.sum())))
    if attr == "all_nan":
        tp_err[4] = np.nan
    elif attr == "mixed":
        tp_err[4, rng.random(m) < 0.4] = np.nan
    tp_err[3, rng.random(m) < 0.1] = np.nan
    tp_err[:, ~hit] = np.nan
    return pred, gt, match, tp_err


def device_curves(ops, ne, pred, gt, match, tp_err):
    score, name = dev(pred["score"]), dev(pred["name"], torch.int32)
    keep = dev(np.ones(len(pred["name"]), dtype=np.uint8))
    order, cls_ptr = ne.class_score_order(score, name, keep, classes_dev())
    out = ops.detection_curves(order, cls_ptr, score, dev(match), dev(tp_err), dev(gt["name"], torch.int32),
                               dev(np.ones(len(gt["name"]), dtype=np.uint8)), classes_dev(), 2, dev(np.linspace(0, 1, 101)))
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("n,npos,p_match,attr", [(1, 1, 1.0, "mixed"), (2, 3, 0.7, "mixed"), (CHUNK - 1, 90, 0.5, "mixed"),
                                                 (CHUNK, 200, 0.5, "all_nan"), (CHUNK + 1, 120, 0.3, "mixed"),
                                                 (3 * CHUNK + 17, 400, 0.6, "none"), (40, 1000, 0.2, "mixed"), (12, 0, 0.5, "mixed"),
                                                 (30, 10, 0.0, "mixed"), (0, 5, 0.5, "mixed")])
def test_curves_against_the_oracle(ops, ne, n, npos, p_match, attr):
    pred, gt, match, tp_err = curve_case(n, npos, 1000 + n, p_match, attr)
    ones_p, ones_g = np.ones(len(pred["name"]), dtype=bool), np.ones(len(gt["name"]), dtype=bool)
    want = oracle.curves(pred, gt, ones_p, ones_g, match, tp_err)
    got = device_curves(ops, ne, pred, gt, match, tp_err)
    car = oracle.DETECTION_NAMES.index('car')
    if npos == 0 or p_match == 0.0 or n == 0:
        assert not want[0][car].any() and not want[1][car].any() and (want[2][car] == 1.0).all()          # no_predictions
    else:
        assert want[0][car].any()
    if attr == "all_nan":
        assert (want[2][car, 4] == 1.0).all() and not (want[2][car, 0] == 1.0).all()
    if npos == 1000:                                                                     # recall stays below 0.1: calc_tp gives 1
        assert np.nonzero(want[1][car, 2])[0][-1] < 11
    for k in (oracle.DETECTION_NAMES.index('pedestrian'), oracle.DETECTION_NAMES.index('bus')):           # no ground truth; no predictions
        for g, fill in zip(got, (0.0, 0.0, 1.0)):
            assert (g[k] == fill).all()
    held(f"curves n={n} npos={npos}", "tables", precision=err_of(got[0], want[0]), confidence=err_of(got[1], want[1]),
         tp_err_curve=err_of(got[2], want[2]))
    from radargnn_amd.nuscenes_eval import DetectionConfig, summarize
    a, b = summarize(*got, DetectionConfig()), oracle.summary(*want)
    if npos == 1000:
        assert a["label_tp_errors"]["car"]["trans_err"] == 1.0 == b["label_tp_errors"]["car"]["trans_err"]
    held(f"curves n={n} npos={npos} summary", "summary", nd_score=abs(a["nd_score"] - b["nd_score"]), mean_ap=abs(a["mean_ap"] - b["mean_ap"]))


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def flat(summary: dict) -> dict:
    out = {"mean_ap": summary["mean_ap"], "nd_score": summary["nd_score"]}
    for key in ("label_aps", "label_tp_errors"):
        for name, d in summary[key].items():
            out.update({f"{key}/{name}/{k}": v for k, v in d.items()})
    for key in ("mean_dist_aps", "tp_errors", "tp_scores"):
        out.update({f"{key}/{k}": v for k, v in summary[key].items()})
    return out


def test_end_to_end_against_the_oracle(ops, ne):
    pred, gt = cases.scene(0)                                                            # 40 samples, up to 60 boxes, 10 classes
    parts = {}
    want = oracle.detection_eval(pred, gt, parts)
    dp, dg = cases.device_predictions(pred), cases.device_ground_truth(gt)
    precision, confidence, tp_curve, got = ne.detection_tables(dp, dg)
    assert np.array_equal(got["keep_pred"].cpu().numpy().astype(bool), parts["keep_pred"])
    assert np.array_equal(got["keep_gt"].cpu().numpy().astype(bool), parts["keep_gt"])
    assert not parts["keep_gt"].all() and not parts["keep_pred"].all() and parts["keep_pred"].sum() > 500
    assert np.array_equal(got["match"].cpu().numpy(), parts["match"])
    m = len(pred["score"])
    order = got["order"].cpu().tolist()
    kept_by_class = [oracle.score_order(pred["score"], [i for i in range(m) if parts["keep_pred"][i] and pred["name"][i] == oracle.code(n)])
                     for n in oracle.DETECTION_NAMES]
    assert order == [i for ids in kept_by_class for i in ids]
    assert len(set(np.round(pred["score"], 6))) < m                                      # repeated scores are part of the scene
    held("end to end tp_err", "tp_err", **{n: err_of(got["tp_err"][e].cpu().numpy(), parts["tp_err"][e]) for e, n in enumerate(oracle.TP_METRICS)})
    held("end to end tables", "tables", precision=err_of(precision.cpu().numpy(), parts["precision"]),
         confidence=err_of(confidence.cpu().numpy(), parts["confidence"]), tp_err_curve=err_of(tp_curve.cpu().numpy(), parts["tp_curve"]))
    summary = ne.detection_eval(dp, dg)
    assert summary.pop("cfg")["dist_th_tp"] == 2.0 and list(summary) == list(want)
    a, b = flat(summary), flat(want)
    assert list(a) == list(b) and 0.05 < want["mean_ap"] < 0.95
    held("end to end summary", "summary", worst=max(err_of(a[k], b[k]) for k in a), nd_score=err_of(a["nd_score"], b["nd_score"]))


def test_evaluator_writes_the_files(ops, ne, tmp_path):
    from gnnradarobjectdetection.postprocessor.nuscenes.evaluation import NuscenesEvaluator
    from radargnn_amd.postprocessor import BoundingBoxes, PostProcessingConfiguration
    rng = np.random.default_rng(5)
    s, names = 3, {"barrier": 0.5, "bicycle": 0.5, "bus": 0.5, "car": 0.5}
    config = PostProcessingConfiguration(min_object_score=names, use_point_iou=True, bg_index=0, f1_class_averaging='None')
    ego_t = np.column_stack((rng.uniform(300, 900, s), rng.uniform(300, 900, s), np.zeros(s)))
    ego_r = np.array([cases.yaw_quat(a) for a in (0.0, 1.0, -2.0)])

    def rect(c, l, w, a):
        d = np.array([[l / 2, w / 2], [l / 2, -w / 2], [-l / 2, -w / 2], [-l / 2, w / 2]])
        return d @ np.array([[math.cos(a), math.sin(a)], [-math.sin(a), math.cos(a)]]) + c

    bb_pred, bb_gt, cls_pred, cls_label, cls_gt, g_rows, g_ptr = [], [], [], [], [], [], [0]
    for f in range(s):
        n = 4 + f
        centres, lw, ang = rng.uniform(-20, 20, (n, 2)), rng.uniform(1, 5, (n, 2)), rng.uniform(0, math.pi, n)
        labels = rng.integers(1, 5, n)
        corners = np.array([rect(centres[i], lw[i, 0], lw[i, 0] / 2, ang[i]) for i in range(n)])
        moved = np.array([rect(centres[i] + 0.3, lw[i, 0], lw[i, 0] / 2, ang[i]) for i in range(n)])
        bb_pred.append({"boxes": BoundingBoxes(dev(moved), False), "scores": dev(rng.uniform(0.3, 1, n)), "labels": dev(labels.astype(np.float64))})
        bb_gt.append({"boxes": BoundingBoxes(dev(corners), False), "labels": dev(labels.astype(np.float32))})
        pos = rng.uniform(-25, 25, (30, 2)).astype(np.float32)
        cls_pred.append({"pos": dev(pos)})
        y = rng.integers(0, 5, 30)
        cls_label.append(dev(y.astype(np.float64)).view(-1, 1))
        cls_gt.append({"pos": dev(pos), "vel": None, "labels": dev(np.where(rng.random(30) < 0.8, y, 0).astype(np.float32))})
        R = oracle.quat_matrix(ego_r[f])
        for i in range(n):                                                                # the ground truth in the global frame
            t = R @ np.array([centres[i, 0], centres[i, 1], 0.0]) + ego_t[f]
            g_rows.append((t, [lw[i, 0] / 2, lw[i, 0], 1.5], cases.yaw_quat(oracle.ego_yaw(ego_r[f]) - ang[i]), int(labels[i])))
        g_ptr.append(len(g_rows))
    gt = ne.DetectionGroundTruth([r[0] for r in g_rows], [r[1] for r in g_rows], [r[2] for r in g_rows], np.zeros((len(g_rows), 2)),
                                 [r[3] for r in g_rows], [-1] * len(g_rows), [2] * len(g_rows), g_ptr, ego_t)
    (tmp_path / "run_07").mkdir()
    ev = NuscenesEvaluator(config, "v1.0-mini", "unused", str(tmp_path), detection_ground_truth=gt, ego_translation=ego_t, ego_rotation=ego_r)
    assert ev.evaluation_folder_path == f"{tmp_path}/evaluation_08" and os.path.isdir(ev.evaluation_folder_path)
    graph_names = [f"/data/graph_{f}_token{f}.pt" for f in range(s)]
    ev.evaluate(bb_pred, bb_gt, cls_pred, cls_label, cls_gt, [None] * s, graph_names)
    ev.save_results()
    folder = tmp_path / "evaluation_08"
    assert sorted(os.listdir(folder)) == ["confusion_abs.npy", "convusion_rel.npy", "eval_configs.json", "eval_results.json",
                                          "nuscenes_metrics.json", "submission.json"]
    sub = json.load(open(folder / "submission.json"))
    assert sub["meta"]["use_radar"] is True and list(sub["results"]) == ["token0", "token1", "token2"]
    assert [len(v) for v in sub["results"].values()] == [4, 5, 6]
    assert set(sub["results"]["token1"][0]) == {"sample_token", "translation", "size", "rotation", "velocity", "detection_name",
                                                "detection_score", "attribute_name"}
    written = json.load(open(folder / "nuscenes_metrics.json"))
    assert written["nd_score"] == ev.metrics_summary["nd_score"] and list(written["label_aps"]["car"]) == ["0.5", "1.0", "2.0", "4.0"]
    # every prediction lies 0.3 * sqrt(2) m from its box: matched from 0.5 m on, with the box's own length and width
    assert ev.metrics_summary["label_aps"]["car"][0.5] > 0.5 and ev.metrics_summary["tp_errors"]["trans_err"] < 1.0
    assert ev.metrics_summary["label_tp_errors"]["car"]["trans_err"] == pytest.approx(0.3 * math.sqrt(2), abs=1e-9)
    assert ev.metrics_summary["label_tp_errors"]["car"]["scale_err"] == pytest.approx(1 - 1.5 / 1.698, abs=1e-9)
    from radargnn_amd.metrics import ObjectDetectionMetrics
    assert ev.mAP == ObjectDetectionMetrics.get_map(config, bb_pred, bb_gt, cls_pred)["map"].item()
    out = json.load(open(folder / "eval_results.json"))
    assert out["OBJECT_DETECTION_METRICS"]["mAP"] == ev.mAP and len(out["SEMANTIC_SEGMENTATION_METRICS"]["f1"]) == 5
    with pytest.raises(ValueError, match="trainval or mini"):
        NuscenesEvaluator(config, "v2", "unused", str(tmp_path), detection_ground_truth=gt, ego_translation=ego_t,
                          ego_rotation=ego_r).evaluate(bb_pred, bb_gt, cls_pred, cls_label, cls_gt, [None] * s, graph_names)
