"""CPU checks of the nuScenes evaluator: tests/nuscenes_eval_oracle.py against answers derived on paper, and the host side of
radargnn_amd.nuscenes_eval (summary, shims, selector, devkit adapter, submission records).  No GPU."""
import json
import math

import numpy as np
import pytest

import nuscenes_eval_cases as cases
import nuscenes_eval_oracle as oracle


def _one_box_per_class():
    names = list(oracle.DETECTION_NAMES)
    xy = [(2.0 * i + 1.0, -1.0 * i) for i in range(len(names))]             # all inside 30 m
    gt = cases.simple(names, xy, velocity=[[0.5 * i, -0.25 * i] for i in range(len(names))], yaw=[0.3 * i - 1.0 for i in range(len(names))])
    return gt


def test_predictions_equal_to_ground_truth_score_one():
    gt = _one_box_per_class()
    res = oracle.detection_eval(oracle.predictions_like(gt), gt)
    for name in oracle.DETECTION_NAMES:
        assert all(ap == pytest.approx(1.0, abs=1e-12) for ap in res["label_aps"][name].values()), name   # mean(0.9 ...) / 0.9
        errs = res["label_tp_errors"][name]
        nan = {'traffic_cone': {'attr_err', 'vel_err', 'orient_err'}, 'barrier': {'attr_err', 'vel_err'}}.get(name, set())
        for metric in oracle.TP_METRICS:
            assert (math.isnan(errs[metric]) if metric in nan else errs[metric] == 0.0), (name, metric, errs[metric])
    assert res["mean_ap"] == pytest.approx(1.0, abs=1e-12)
    assert all(v == 0.0 for v in res["tp_errors"].values()) and all(v == 1.0 for v in res["tp_scores"].values())
    assert res["nd_score"] == pytest.approx(1.0, abs=1e-12)                              # (5 * 1 + 5 * 1) / 10


def test_no_predictions_score_zero():
    gt = _one_box_per_class()
    pred = cases.simple([], [], ptr=[0, 0], score=[])
    res = oracle.detection_eval(pred, gt)
    assert res["mean_ap"] == 0.0 and res["nd_score"] == 0.0
    assert all(v == 1.0 for v in res["tp_errors"].values()) and all(v == 0.0 for v in res["tp_scores"].values())
    assert all(ap == 0.0 for aps in res["label_aps"].values() for ap in aps.values())


def test_three_predictions_two_boxes_by_hand():
    """Ground truth A (10, 0), B (20, 0); predictions P0 (10.3, 0) 0.9, P1 (10.1, 0) 0.8, P2 (21.5, 0) 0.7, all cars.
    At 0.5 and 1.0: P0 takes A, P1 and P2 miss: rec = (.5, .5, .5), prec = (1, 1/2, 1/3); np.interp gives 1 below 0.5, the LAST
    entry 1/3 at 0.5, 0 above: AP = (39 * 0.9 + (1/3 - 0.1)) / 90 / 0.9.
    At 2.0 and 4.0: P2 takes B: rec = (.5, .5, 1), prec = (1, 1/2, 2/3): 1 below 0.5, 1/2 at 0.5, 1/2 + (r - 1/2) / 3 above:
    AP = (39 * 0.9 + 0.4 + 50 * 0.4 + 4.25) / 90 / 0.9.
    trans_err at 2.0: matches at confidence 0.9 (0.3 m) and 0.7 (1.5 m), running mean (0.3, 0.9); the confidence table is 0.9
    below recall 0.5, 0.8 at 0.5, 0.8 - 0.2 (r - 0.5) above; resampled: 0.3, 0.6, 0.6 + 0.6 (r - 0.5): mean over recall 0.11 ..
    1.00 = (39 * 0.3 + 0.6 + 50 * 0.6 + 0.6 * 12.75) / 90 = 0.555."""
    gt = cases.simple(['car', 'car'], [(10.0, 0.0), (20.0, 0.0)])
    pred = cases.simple(['car'] * 3, [(10.3, 0.0), (10.1, 0.0), (21.5, 0.0)], score=[0.9, 0.8, 0.7])
    parts = {}
    res = oracle.detection_eval(pred, gt, parts)
    assert parts["match"].tolist() == [[0, -1, -1], [0, -1, -1], [0, -1, 1], [0, -1, 1]]
    low = (39 * 0.9 + (1 / 3 - 0.1)) / 90 / 0.9
    high = (39 * 0.9 + 0.4 + 50 * 0.4 + 4.25) / 90 / 0.9
    aps = res["label_aps"]["car"]
    assert aps[0.5] == pytest.approx(low, abs=1e-12) and aps[1.0] == pytest.approx(low, abs=1e-12)
    assert aps[2.0] == pytest.approx(high, abs=1e-12) and aps[4.0] == pytest.approx(high, abs=1e-12)
    errs = res["label_tp_errors"]["car"]
    assert errs["trans_err"] == pytest.approx(0.555, abs=1e-12)
    assert errs["scale_err"] == 0.0 and errs["orient_err"] == 0.0 and errs["vel_err"] == 0.0 and errs["attr_err"] == 0.0
    assert res["mean_ap"] == pytest.approx((low + high) / 2 / 10, abs=1e-12)
    # nine classes without ground truth have error 1; traffic_cone / barrier are left out of the means where their error is NaN
    assert res["tp_errors"]["trans_err"] == pytest.approx((0.555 + 9) / 10, abs=1e-12)
    assert res["tp_errors"]["attr_err"] == pytest.approx(7 / 8, abs=1e-12)
    nds = (5 * res["mean_ap"] + sum(max(0.0, 1 - e) for e in res["tp_errors"].values())) / 10
    assert res["nd_score"] == pytest.approx(nds, abs=1e-15)


def test_equal_scores_go_by_descending_position_and_ties_to_the_lower_box():
    gt = cases.simple(['car', 'car'], [(0.0, 1.0), (0.0, -1.0)])
    pred = cases.simple(['car', 'car'], [(0.0, 0.0), (0.0, 0.0)], score=[0.5, 0.5])
    keep = np.ones(2, dtype=bool)
    match, _ = oracle.match_boxes(pred, gt, keep, keep)
    assert oracle.score_order(pred["score"], [0, 1]) == [1, 0]
    assert match[2].tolist() == [1, 0]                       # the LATER prediction goes first and takes the LOWER of two equidistant boxes
    assert match[0].tolist() == [-1, -1] and match[1].tolist() == [-1, -1]                # distance exactly 1.0 is no match at 1.0


def test_summary_of_the_module_is_the_oracle_summary():
    from radargnn_amd.nuscenes_eval import DetectionConfig, summarize
    pred, gt = cases.scene(3, n_samples=6, max_boxes=20)
    parts = {}
    expect = oracle.detection_eval(pred, gt, parts)
    got = summarize(parts["precision"], parts["confidence"], parts["tp_curve"], DetectionConfig())
    assert got.pop("cfg") == {"class_range": oracle.CLASS_RANGE, "dist_fcn": "center_distance", "dist_ths": list(oracle.DIST_THS),
                              "dist_th_tp": 2.0, "min_recall": 0.1, "min_precision": 0.1, "max_boxes_per_sample": 500, "mean_ap_weight": 5}
    assert json.dumps(got, sort_keys=True) == json.dumps(expect, sort_keys=True)
    assert 0.0 < expect["mean_ap"] < 1.0 and 0.0 < expect["nd_score"] < 1.0


def test_detection_config_refuses_a_tp_threshold_outside_the_list():
    from radargnn_amd.nuscenes_eval import DetectionConfig
    with pytest.raises(ValueError):
        DetectionConfig(dist_th_tp=3.0)


def test_match_decisions_survive_a_perturbation_of_1e_12():
    """The seeded scene keeps every distance at least 1e-6 from the thresholds and ranges, so no decision hangs on the last bits."""
    pred, gt = cases.scene(0)
    d_margin, r_margin = cases.smallest_margins(pred, gt)
    assert d_margin >= 1e-6 and r_margin >= 1e-6, (d_margin, r_margin)
    base, moved = {}, {}
    oracle.detection_eval(pred, gt, base)
    rng = np.random.default_rng(1)
    pred2, gt2 = dict(pred), dict(gt)
    pred2["translation"] = pred["translation"] + rng.choice([-1e-12, 1e-12], pred["translation"].shape)
    gt2["translation"] = gt["translation"] + rng.choice([-1e-12, 1e-12], gt["translation"].shape)
    oracle.detection_eval(pred2, gt2, moved)
    for key in ("keep_pred", "keep_gt", "match"):
        assert np.array_equal(base[key], moved[key]), key
    assert (base["match"] >= 0).sum() > 100


def test_shims_and_selector():
    from gnnradarobjectdetection.postprocessor.nuscenes import evaluation, utils
    from gnnradarobjectdetection.postprocessor.nuscenes.evaluation import NuscenesEvaluator
    from gnnradarobjectdetection.postprocessor.nuscenes.utils import get_sample_token, get_submission
    from radargnn_amd import metrics, nuscenes_eval
    assert NuscenesEvaluator is nuscenes_eval.NuscenesEvaluator and get_submission is nuscenes_eval.get_submission
    assert evaluation.get_submission is get_submission and utils.get_bounding_box_detection_name(4) == 'car'
    assert get_sample_token("/data/graphs/graph_12_abc123.pt") == "abc123"
    assert set(nuscenes_eval.evaluation_selector) == {"radarscenes", "nuscenes"}
    assert nuscenes_eval.evaluation_selector["radarscenes"] is metrics.RadarscenesEvaluator
    assert nuscenes_eval.evaluation_selector["nuscenes"] is NuscenesEvaluator
    assert set(metrics.evaluation_selector) == {"radarscenes"}                             # the old dict is untouched
    assert issubclass(NuscenesEvaluator, metrics.Evaluator)
    assert tuple(nuscenes_eval.LABEL_NAMES) == oracle.LABEL_NAMES and tuple(nuscenes_eval.DETECTION_NAMES) == oracle.DETECTION_NAMES
    assert [nuscenes_eval.HEIGHT_MAP[n] for n in nuscenes_eval.LABEL_NAMES] == list(oracle.HEIGHTS)
    assert {n: nuscenes_eval.ATTRIBUTE_CODE[a] for n, a in nuscenes_eval.PREDICTED_ATTRIBUTE.items()} == oracle.PRED_ATTRIBUTE


class _StandInNusc:
    """The five tables and the one method ``ground_truth_from_devkit`` reads."""

    def __init__(self):
        ann = lambda cat, t, attrs=(), lidar=1, radar=0: {"category_name": cat, "translation": t, "size": [1.0, 2.0, 3.0],
                                                         "rotation": [1.0, 0.0, 0.0, 0.0], "attribute_tokens": list(attrs),
                                                         "num_lidar_pts": lidar, "num_radar_pts": radar}
        self.tables = {
            "sample": {"s0": {"anns": ["a0", "a1", "a2", "a3"], "data": {"LIDAR_TOP": "d0"}},
                       "s1": {"anns": [], "data": {"LIDAR_TOP": "d1"}},
                       "s2": {"anns": ["a4"], "data": {"LIDAR_TOP": "d2"}}},
            "sample_annotation": {"a0": ann("vehicle.car", [1.0, 2.0, 3.0], ["at_moving"], 3, 2),
                                  "a1": ann("animal", [0.0, 0.0, 0.0]),
                                  "a2": ann("vehicle.bicycle_rack", [5.0, 5.0, 0.0]),
                                  "a3": ann("movable_object.barrier", [4.0, 4.0, 0.0], [], 0, 0),
                                  "a4": ann("human.pedestrian.child", [7.0, 8.0, 9.0], ["at_standing"])},
            "attribute": {"at_moving": {"name": "vehicle.moving"}, "at_standing": {"name": "pedestrian.standing"}},
            "sample_data": {f"d{i}": {"ego_pose_token": f"e{i}"} for i in range(3)},
            "ego_pose": {f"e{i}": {"translation": [10.0 * i, 1.0, 0.0], "rotation": [1.0, 0.0, 0.0, 0.1 * i]} for i in range(3)}}

    def get(self, table, token):
        return self.tables[table][token]

    def box_velocity(self, token):
        return np.array([np.nan, np.nan, np.nan]) if token == "a3" else np.array([1.0, -1.0, 0.5])


def test_ground_truth_from_devkit_on_stand_in_objects():
    from radargnn_amd.nuscenes_eval import ATTRIBUTE_CODE, NAME_CODE, ground_truth_from_devkit
    gt = ground_truth_from_devkit(_StandInNusc(), ["s0", "s1", "s2"])
    assert gt.gt_ptr.tolist() == [0, 2, 2, 3] and gt.rack_ptr.tolist() == [0, 1, 1, 1]
    assert gt.name.tolist() == [NAME_CODE['car'], NAME_CODE['barrier'], NAME_CODE['pedestrian']]
    assert gt.attribute.tolist() == [ATTRIBUTE_CODE['vehicle.moving'], -1, ATTRIBUTE_CODE['pedestrian.standing']]
    assert gt.num_pts.tolist() == [5, 0, 1]
    assert gt.translation.tolist() == [[1.0, 2.0, 3.0], [4.0, 4.0, 0.0], [7.0, 8.0, 9.0]]
    assert gt.velocity[0].tolist() == [1.0, -1.0] and np.isnan(gt.velocity[1]).all()
    assert gt.rack_center.tolist() == [[5.0, 5.0, 0.0]] and gt.rack_size.tolist() == [[1.0, 2.0, 3.0]]
    assert gt.ego_translation.tolist() == [[0.0, 1.0, 0.0], [10.0, 1.0, 0.0], [20.0, 1.0, 0.0]]
    assert gt.ego_rotation[2].tolist() == [1.0, 0.0, 0.0, 0.2] and gt.sample_tokens == ["s0", "s1", "s2"]
    nusc = _StandInNusc()
    nusc.tables["sample_annotation"]["a0"]["attribute_tokens"] = ["at_moving", "at_standing"]
    with pytest.raises(Exception, match="more than one attribute"):
        ground_truth_from_devkit(nusc, ["s0"])


def test_submission_records_have_the_reference_shape():
    from radargnn_amd.nuscenes_eval import SUBMISSION_META, submission_records
    boxes = np.array([[1.0, 2.0, 4.0, 2.0, 30.0], [0.0, -3.0, 1.0, 0.5, 90.0], [5.0, 5.0, 2.0, 2.0, 0.0]])
    labels, scores, ptr = [4, 7, 1], [0.75, 0.5, 0.25], [0, 2, 2, 3]
    ego_t, ego_r = np.array([[100.0, 200.0, 1.0]] * 3), np.array([cases.yaw_quat(0.5)] * 3)
    translation, size, rotation, yaw = oracle.submission(boxes, labels, ptr, ego_t, ego_r)
    packed = np.concatenate([translation.ravel(), size.ravel(), rotation.ravel(), yaw, labels, scores, [0.0]])
    results = submission_records(packed, ptr, ["tok0", "tok1", "tok2"])
    assert list(results) == ["tok0", "tok1", "tok2"] and [len(v) for v in results.values()] == [2, 0, 1]
    rec = results["tok0"][0]
    assert list(rec) == ["sample_token", "translation", "size", "rotation", "velocity", "detection_name", "detection_score", "attribute_name"]
    assert rec["sample_token"] == "tok0" and rec["detection_name"] == "car" and rec["attribute_name"] == "vehicle.moving"
    assert rec["size"] == (2.0, 4.0, 1.698) and rec["velocity"] == (0.0, 0.0) and rec["detection_score"] == 0.75
    assert rec["translation"][2] == 1.0 + 1.698 / 2 and rec["rotation"][1:3] == (0.0, 0.0)
    assert rec["rotation"][0] == pytest.approx(math.cos((math.radians(30.0) + 0.5) / 2), abs=1e-15)
    assert results["tok2"][0]["detection_name"] == "barrier" and results["tok2"][0]["attribute_name"] == ""
    json.dumps({"meta": SUBMISSION_META, "results": results})                             # serialisable as it stands
    assert SUBMISSION_META == {"use_camera": False, "use_lidar": False, "use_radar": True, "use_map": False, "use_external": False}
    packed[-1] = 1.0
    with pytest.raises(ValueError):
        submission_records(packed, ptr, ["tok0", "tok1", "tok2"])
    with pytest.raises(ValueError):
        oracle.submission(boxes, [4, 0, 1], ptr, ego_t, ego_r)


def test_c_abi_refuses_bad_arguments_without_gpu():
    from radargnn_amd import _lib
    cap = _lib.lib.rgnn_center_match_capacity()
    assert cap >= 256 and cap & (cap - 1) == 0                                          # a power of two
    assert _lib.lib.rgnn_detection_curves_tmp_bytes(10, 4) == 10 * 4 * 4 + 10 * 6 * 8
    assert _lib.lib.rgnn_detection_curves_tmp_bytes(-1, 4) == -1
    rc = _lib.lib.rgnn_center_match(None, None, 1, None, None, 0, None, 0, 0, 1, None, None, None, None)
    assert rc == -1 and b"null box lists" in _lib.lib.rgnn_last_error()
    rc = _lib.lib.rgnn_detection_curves(None, None, None, None, None, 0, None, None, 0, None, 1, 4, 7, None, 101, None, None, None, None, None)
    assert rc == -1 and b"tp_index" in _lib.lib.rgnn_last_error()
