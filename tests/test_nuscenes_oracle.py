"""The numpy oracle of the nuScenes sample stage (tests/nuscenes_oracle.py) against the reference-generated fixtures
(tests/golden/nuscenes_*.npz, tests/golden/make_nuscenes_golden.py).  CPU only.

Kept rows and their order, frame_ptr, labels, the surviving boxes and the NaN pattern of the targets must agree exactly.  For the
float columns ``oracle_differences`` measures the worst absolute difference per stage and mode; that figure is the unit of the GPU
test's bar (tests/test_gpu_nuscenes.py allows the device 10 x it, with a floor of 8 ulp of the column's largest magnitude).  The
ceiling asserted here is reasoned, not measured: the global coordinates reach ~2e3 and are differenced to vehicle coordinates of
~5e1, so one rounding of the difference is 2.3e-13 and the rotation carries it through a few more at that size -> below 1e-11 for
the positions (the sibling oracle tests use 1e-12 at coordinates of 1e2); lengths and angles inherit it through a sqrt / atan2
of well-conditioned arguments (sides >= 0.5 m)."""
import glob
import os

import numpy as np
import pytest

import nuscenes_oracle as O
from conftest import record_parity

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "nuscenes_*.npz")))
IDS = [os.path.basename(p)[9:-4] for p in FIXTURES]
EN_QUANTUM = 1e-5 * np.pi / 180          # the reference rounds the en angles to 5 decimals in degrees
STAGES = ("points", "velocity", "centre", "rect", "none", "translation", "en")


def settings(g):
    return bool(g["crop"]), float(g["xlim"]), float(g["ylim"]), float(g["wlh_factor"]), float(g["wlh_offset"])


def inputs(g):
    return {k: g[k] for k in O.INPUT_KEYS}


def oracle_differences(g):
    """{stage or mode: (worst |oracle - reference| over positions, lengths and unrounded angles, worst over the two rounded en
    angles)}.  Everything discrete must agree exactly."""
    o = O.create(inputs(g), *settings(g))
    ref = g["ref_points"]
    assert np.array_equal(o["frame_ptr"], g["ref_frame_ptr"])
    assert np.array_equal(g["points"][3:8, o["src_row"]], ref[3:8]) and np.array_equal(g["points"][10:, o["src_row"]], ref[10:])
    assert np.array_equal(o["rcs"], ref[5]) and np.array_equal(o["timestamp"], ref[18]) and np.array_equal(o["V_cc"], ref[6:8].T)
    assert (ref[2] == 0).all()
    assert np.array_equal(o["kept"], g["ref_kept"]) and np.array_equal(o["kept_ptr"], g["ref_kept_ptr"])
    assert np.array_equal(o["labels"], g["ref_labels"])
    out = {"points": (np.abs(o["X"] - ref[:2].T).max(), 0.0), "velocity": (np.abs(o["V"] - ref[8:10].T).max(), 0.0),
           "centre": (np.abs(o["center"] - g["ref_center"]).max(), 0.0), "rect": (np.abs(o["rect"] - g["ref_rect"]).max(), 0.0)}
    for mode in O.MODES:
        got, want = o["boxes_" + mode], g["ref_boxes_" + mode]
        assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), mode
        assert np.array_equal(np.isnan(want).all(1), o["hit"] < 0), mode
        d = np.abs(np.nan_to_num(got - want))
        out[mode] = (d[:, [0, 2, 3]].max(), d[:, [1, 4]].max()) if mode == "en" else (d.max(), 0.0)
    return out


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_oracle_matches_reference(path):
    g = np.load(path)
    diff = oracle_differences(g)
    record_parity("nuscenes_oracle_vs_reference_" + os.path.basename(path)[9:-4], **{k: v[0] for k, v in diff.items()},
                  en_angles=diff["en"][1])
    for key, (plain, angles) in diff.items():
        assert plain <= 1e-11, (key, plain)
        assert angles <= 1e-11 + EN_QUANTUM, (key, angles)


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_fixture_is_admissible_and_covers_the_cases(path):
    g = np.load(path)
    inp, (crop, xlim, ylim, factor, offset) = inputs(g), settings(g)
    assert O.is_admissible(inp, crop, xlim, ylim, factor, offset)
    margins = O.admissibility(inp, crop, xlim, ylim, factor, offset)
    for k, v in margins.items():
        assert np.array_equal(v, g["margin_" + k]), k
    assert np.array_equal(g["threshold"], [O.ADMISSIBLE[k] for k in sorted(O.ADMISSIBLE)])
    for k in ("points", "chunk_rotation", "chunk_translation", "box_center", "box_size", "box_rotation", "ego_translation", "ego_rotation"):
        assert g[k].dtype == np.float64 and np.array_equal(g[k], g[k].astype(np.float32).astype(np.float64)), k
    o = O.create(inp, crop, xlim, ylim, factor, offset)
    n_rows, n_boxes = np.diff(g["chunk_ptr"][[0, 5, 10, 15]]), np.diff(g["box_ptr"])
    assert len(n_boxes) == 3 and (n_rows <= 200).all() and (n_boxes <= 70).all() and n_boxes[2] == 0 and n_boxes[1] > 64
    assert g["chunk_ptr"][5] == g["chunk_ptr"][6]                                   # the second sample's first chunk is empty
    assert (np.diff(o["frame_ptr"]) < n_rows).all() and (np.diff(o["frame_ptr"]) >= 2).all()          # the crop drops rows everywhere
    dropped = np.setdiff1d(np.arange(len(g["box_label"])), o["kept"])
    assert (g["box_points"][dropped] == 0).any() and (g["box_points"][dropped] > 0).any()           # no points / beyond the crop
    assert (o["wlh"][:, 0] > o["wlh"][:, 1]).any()                                  # wider than long
    # a point in two boxes with different labels, and the later one wins
    in_two = 0
    for s in range(2):
        a, b, ka, kb = o["frame_ptr"][s], o["frame_ptr"][s + 1], o["kept_ptr"][s], o["kept_ptr"][s + 1]
        inside, _ = O.membership(o["X"][a:b], o["center"][ka:kb], o["R"][ka:kb], o["wlh"][ka:kb], factor, offset)
        for p in np.nonzero(inside.sum(0) >= 2)[0]:
            ks = np.nonzero(inside[:, p])[0]
            if len(set(o["label"][ka + ks].tolist())) > 1:
                in_two += 1
                assert g["ref_labels"][a + p] == o["label"][ka + ks[-1]]
    assert in_two >= 1
    ego = O.rotation_matrices(g["ego_rotation"])
    tilt = np.degrees(np.arccos(ego[:, 2, 2]))
    assert (tilt > 0.5).all() and (tilt < 8).all()                                  # a few degrees of pitch and roll
    ts = g["points"][18]
    assert len(np.unique(ts)) == 3                                                  # nsweeps-like repeated timestamps
    assert (g["ref_labels"] > 0).sum() >= 30 and (g["ref_labels"][g["ref_frame_ptr"][2]:] == 0).all()


def test_fixtures_cover_both_inflations():
    pairs = {(float(np.load(p)["wlh_factor"]), float(np.load(p)["wlh_offset"])) for p in FIXTURES}
    assert {(1.0, 0.0), (1.1, 0.5)} <= {(round(f, 6), round(o, 6)) for f, o in pairs}


def test_oracle_hand_vectors():
    # an axis-aligned 4 x 2 box at (3, 1): level ego pose at the origin, identity rotations
    one = lambda **k: {**dict(points=np.zeros((19, 0)), chunk_ptr=np.zeros(1, dtype=np.int64), chunk_sample=np.zeros(0, dtype=np.int32),
                              chunk_rotation=np.zeros((0, 4)), chunk_translation=np.zeros((0, 3)), box_center=np.array([[3.0, 1.0, 0.5]]),
                              box_size=np.array([[2.0, 4.0, 1.0]]), box_rotation=np.array([[1.0, 0, 0, 0]]),
                              box_label=np.array([4], dtype=np.int32), box_points=np.array([1], dtype=np.int32),
                              box_ptr=np.array([0, 1]), ego_translation=np.zeros((1, 3)), ego_rotation=np.array([[1.0, 0, 0, 0]])), **k}
    b = O.vehicle_boxes(one(), False, 0, 0)
    rect, d = O.rectangles(b["center"], b["R"], b["wlh"])
    assert np.array_equal(rect, [[3.0, 1.0, 4.0, 2.0, 0.0]]) and np.array_equal(d, [[2.0, np.sqrt(20.0), 4.0]])
    pos = np.array([[5.0, 2.0], [5.5, 2.0], [1.0, 0.0], [0.5, 0.0]])
    inside, _ = O.membership(pos, b["center"], b["R"], b["wlh"], 1.0, 0.0)
    assert inside.tolist() == [[True, False, True, False]]
    inside, _ = O.membership(pos, b["center"], b["R"], b["wlh"], 1.0, 0.5)
    assert inside.all()
    b = O.vehicle_boxes(one(box_size=np.array([[4.0, 2.0, 1.0]])), False, 0, 0)          # wider than long: l and w swap, theta turns
    rect, _ = O.rectangles(b["center"], b["R"], b["wlh"])
    assert np.array_equal(rect, [[3.0, 1.0, 4.0, 2.0, 90.0]])
