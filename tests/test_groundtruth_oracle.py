"""The numpy oracle of the ground-truth box targets (tests/groundtruth_oracle.py) against the reference-generated fixtures
(tests/golden/groundtruth_*.npz, tests/golden/make_groundtruth_golden.py).  CPU only.

The oracle forms the rectangle from the hull projections directly; the reference goes through atan2 / cos / sin
(rotate_points, utils/math.py:356-371) and the mean of four corners.  The difference measured here (absolute, per mode, worst
over all columns but the two rounded en angles) is the unit of the GPU test's bar: tests/test_gpu_groundtruth.py allows the device
10 x this.  Its own ceiling below is reasoned, not measured: coordinates reach ~1e2, float64 eps is 2.2e-16, and the reference's
detour is a chain of some ten roundings at that magnitude -> a few 1e-13; 1e-12 is the bar of the sibling oracle tests."""
import glob
import os

import numpy as np
import pytest

import groundtruth_oracle as O
from conftest import record_parity

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "groundtruth_*.npz")))
MODES = (("aligned", True, "translation"), ("none", False, "none"), ("translation", False, "translation"), ("en", False, "en"))
EN_QUANTUM = 1e-5 * np.pi / 180          # the reference rounds the en angles to 5 decimals in degrees


def oracle_differences(g):
    """{mode: (worst |oracle - reference| over positions, lengths and unrounded angles, worst over the two rounded en angles)},
    plus "rect".  NaN patterns (background rows) must agree exactly."""
    out = {}
    pos, oid, ptr = g["pos"], g["object_id"], g["frame_ptr"]
    for key, aligned, inv in MODES:
        boxes, rect = O.create_boxes(pos, oid, ptr, aligned, inv)
        ref = g["boxes_" + key]
        assert boxes.shape == ref.shape and np.array_equal(np.isnan(boxes), np.isnan(ref)), key
        assert np.array_equal(np.isnan(ref).all(1), oid < 0) and np.array_equal(np.isnan(ref).any(1), oid < 0), key
        d = np.abs(np.nan_to_num(boxes - ref))
        if key == "en":
            out[key] = (d[:, [0, 2, 3]].max(), d[:, [1, 4]].max())
        else:
            out[key] = (d.max(), 0.0)
        if key == "none":
            out["rect"] = (np.abs(rect - g["rect"]).max(), 0.0)
    return out


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[12:-4] for p in FIXTURES])
def test_oracle_matches_reference(path):
    g = np.load(path)
    diff = oracle_differences(g)
    record_parity("groundtruth_oracle_vs_reference_" + os.path.basename(path)[12:-4],
                  **{k: v[0] for k, v in diff.items()}, en_angles=diff["en"][1])
    for key, (plain, angles) in diff.items():
        assert plain <= 1e-12, (key, plain)
        assert angles <= 1e-12 + EN_QUANTUM, (key, angles)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[12:-4] for p in FIXTURES])
def test_fixture_is_admissible_and_covers_the_sizes(path):
    g = np.load(path)
    pos, oid, ptr = g["pos"], g["object_id"], g["frame_ptr"]
    assert O.is_admissible(pos, oid, ptr)
    margins = O.admissibility(pos, oid, ptr)
    for k, v in margins.items():
        assert np.array_equal(v, g["margin_" + k]), k
    sizes = {len(rows) for rows in O.objects(oid, ptr)}
    assert {1, 2, 3, 4, 5, 17, 35, 63, 64, 65} <= sizes
    assert np.array_equal(pos, pos.astype(np.float32).astype(np.float64))
    per_frame = [set(oid[a:b][oid[a:b] >= 0].tolist()) for a, b in zip(ptr[:-1], ptr[1:])]
    assert per_frame[0] & per_frame[1] & per_frame[2]                       # ids reused across frames
    assert max(per_frame[0]) > len(per_frame[0])                            # and not dense
    assert all((oid[a:b] < 0).sum() >= 50 for a, b in zip(ptr[:-1], ptr[1:]))


def test_oracle_refuses_degenerate_objects():
    ptr = np.array([0, 3])
    with pytest.raises(O.DegenerateObject):
        O.create_boxes(np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]]), np.zeros(3, dtype=np.int64), ptr, False, "none")
    with pytest.raises(O.DegenerateObject):
        O.create_boxes(np.array([[1.0, 2.0], [1.0, 2.0], [5.0, 5.0]]), np.array([0, 0, -1]), ptr, False, "none")


def test_oracle_hand_vectors():
    # an exact 3-4-5 right triangle: the rectangle flush with either leg is 4 x 3 (area 12); flush with the hypotenuse 5 x 2.4
    pos = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 3.0]])
    _, rect = O.create_boxes(pos, np.zeros(3, dtype=np.int64), np.array([0, 3]), False, "none")
    assert np.allclose(rect[0], [2.0, 1.5, 4.0, 3.0, 0.0], rtol=0, atol=1e-15)
