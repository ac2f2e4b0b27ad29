"""Ground-truth box targets on the device (csrc/groundtruth.hip through radargnn_amd.groundtruth / ops) against the
reference-generated fixtures (tests/golden/groundtruth_*.npz), the numpy oracle (tests/groundtruth_oracle.py) and hand vectors.

Bars.  Positions, lengths and the unrounded angle are compared with the REFERENCE's values at 10 x the difference between the
oracle and the reference on the same fixture and mode (measured here by test_groundtruth_oracle.oracle_differences: float64
trigonometry in the reference's rotate_points; the factor covers the device's atan2 / sincos).  Measured: oracle 2.1e-14 (none,
translation), 2.4e-14 (en), 0 (aligned: min / max and four exact operations, so the device must match bit for bit); bars
2.1e-13 / 2.4e-13 / 0 (MEASUREMENTS.md).  The two en angles get the reference's rounding quantum (1e-5 degrees in radians) on top.
Against the oracle (fuzz, where no reference ran) the bar is the same quantity: 10 x the worst fixture difference of the mode.
"""
import glob
import os

import numpy as np
import pytest
import torch

import groundtruth_oracle as O
from conftest import record_parity
from test_groundtruth_oracle import EN_QUANTUM, FIXTURES, MODES, oracle_differences

pytestmark = pytest.mark.gpu
IDS = [os.path.basename(p)[12:-4] for p in FIXTURES]
_BARS = {}


def bars(path=None):
    """{mode: 10 x |oracle - reference|} of one fixture (or the worst over all fixtures), computed once."""
    for p in FIXTURES:
        if p not in _BARS:
            _BARS[p] = {k: 10 * v[0] for k, v in oracle_differences(np.load(p)).items()}
    if path is not None:
        return _BARS[path]
    return {k: max(b[k] for b in _BARS.values()) for k in next(iter(_BARS.values()))}


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radargnn_amd import groundtruth
    return groundtruth


def track_ids(object_id):
    return np.array([b"" if i < 0 else str(int(i)).encode() for i in object_id])


def check_boxes(got, ref, key, bar, what):
    """got / ref [N, 4|5]: same NaN rows (all columns), plain columns within `bar`, the en angles within bar + quantum."""
    assert got.shape == ref.shape and got.dtype == np.float64, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    d = np.abs(np.nan_to_num(got - ref))
    plain, angles = (d[:, [0, 2, 3]], d[:, [1, 4]]) if key == "en" else (d, np.zeros((1, 1)))
    print(f"[groundtruth] {what} {key}: plain {plain.max():.2e} (bar {bar:.2e}), en angles {angles.max():.2e}")
    assert plain.max() <= bar, (what, key, plain.max(), bar)
    assert angles.max() <= bar + EN_QUANTUM, (what, key, angles.max())
    return plain.max(), angles.max()


# ---------------------------------------------------------------------------------------------- 1. fixtures
@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_matches_reference_fixtures(G, path):
    g = np.load(path)
    pos, oid, ptr = g["pos"], g["object_id"], g["frame_ptr"]
    bar = bars(path)
    worst = {}
    for key, aligned, inv in MODES:
        ref = g["boxes_" + key]
        assert np.array_equal(np.isnan(ref).all(1), oid < 0)                       # background rows: NaN in every column
        batched, rect, obj_ptr, _ = G.create_2d_bounding_boxes_batched(pos, oid, ptr.tolist(), aligned, inv, return_rect=True)
        assert batched.is_cuda and batched.dtype == torch.float64
        worst[key], worst[key + "_angles"] = check_boxes(batched.cpu().numpy(), ref, key, bar[key], "batched")
        for a, b in zip(ptr[:-1], ptr[1:]):
            cloud = type("Cloud", (), dict(X_cc=pos[a:b], track_id=track_ids(oid[a:b]), label_id=np.zeros(b - a)))()
            single = G.GroundTruthCreator.create_2D_bounding_boxes(cloud, aligned, inv)
            check_boxes(single.cpu().numpy(), ref[a:b], key, bar[key], f"frame {a}:{b}")
        if not aligned:
            d = np.abs(rect.cpu().numpy() - g["rect"])
            d[:, 4] = np.abs((d[:, 4] + 90) % 180 - 90)
            assert d.max() <= bar["rect"], (key, d.max())
            worst["rect"] = d.max()
        assert obj_ptr.numel() - 1 == len(g["rect"])
    record_parity("groundtruth_gpu_vs_reference_" + os.path.basename(path)[12:-4], **worst)


# ---------------------------------------------------------------------------------------------- 2. round trip
def _angle_diff(a, b, period):
    return np.abs((a - b + period / 2) % period - period / 2)


@pytest.mark.parametrize("key,aligned,inv", MODES, ids=[m[0] for m in MODES])
def test_round_trip_through_the_decoder(G, key, aligned, inv):
    from radargnn_amd import ops
    from radargnn_amd.postprocessor import GroundTruthExtractor
    g = np.load(FIXTURES[0])
    a, b = g["frame_ptr"][0], g["frame_ptr"][1]                                     # the frame with the 1- and 2-point objects
    pos, oid = g["pos"][a:b], g["object_id"][a:b]
    boxes, rect, obj_ptr, obj_rows = G.create_2d_bounding_boxes_batched(pos, oid, [0, b - a], aligned, inv, return_rect=True)
    bg = 5
    labels = np.where(oid >= 0, 1.0, float(bg))
    y = G.merge_targets(labels, boxes)
    assert y.dtype == torch.float32 and y.shape == (b - a, 1 + boxes.shape[1])
    pos32 = torch.from_numpy(pos.astype(np.float32)).cuda()
    decoded, kept_labels = GroundTruthExtractor.get_absolute_object_bounding_boxes(y[:, 0], y[:, 1:], pos32, inv, bg)
    kept = np.nonzero(oid >= 0)[0]
    assert len(decoded) == len(kept) and (kept_labels.cpu().numpy() == 1).all()
    two_point, rotated = ops.box_representations(decoded.corners)
    two_point, rotated = two_point.cpu().numpy(), rotated.cpu().numpy()
    rect, obj_ptr, obj_rows = rect.cpu().numpy(), obj_ptr.cpu().numpy(), obj_rows.cpu().numpy()
    want = np.full((b - a, 5), np.nan)
    for o in range(len(obj_ptr) - 1):
        want[obj_rows[obj_ptr[o]:obj_ptr[o + 1]]] = rect[o]
    want = want[kept]
    assert not np.isnan(want).any()
    if aligned:
        ref = np.stack([want[:, 0] - want[:, 2] / 2, want[:, 1] - want[:, 3] / 2, want[:, 0] + want[:, 2] / 2,
                        want[:, 1] + want[:, 3] / 2], axis=1)
        err = np.abs(two_point - ref).max() / np.abs(ref).max()
        record_parity(f"groundtruth_round_trip_{key}", boxes=err)
        assert err <= 1e-5
        return
    err_c = np.abs(rotated[:, :2] - want[:, :2]).max() / np.abs(want[:, :2]).max()
    err_s = np.abs(rotated[:, 2:4] - want[:, 2:4]).max() / np.abs(want[:, 2:4]).max()
    square = want[:, 2] == want[:, 3]                                              # single points: 0.5 x 0.5, any multiple of 90
    assert square.any() and not square.all()
    if key == "en":
        # a single point's en row is [0, 0, 0.5, 0.5, 0] (dataset_creation.py:323-343): angle 0 RELATIVE to the nearest neighbour, so
        # the decoder turns that square to the neighbour's direction -- the reference's own round trip; expect exactly that
        nn = O.nearest_in_frames(pos, np.array([0, b - a]))[0][kept[square]]
        v = pos[nn] - pos[kept[square]]
        want[square, 4] = np.degrees(np.arctan2(v[:, 1], v[:, 0])) % 180
    err_t = max(_angle_diff(rotated[~square, 4], want[~square, 4], 180).max(),
                _angle_diff(rotated[square, 4], want[square, 4], 90).max()) / 180
    record_parity(f"groundtruth_round_trip_{key}", centre=err_c, size=err_s, theta=err_t)
    assert err_c <= 1e-5 and err_s <= 1e-5 and err_t <= 1e-5


# ---------------------------------------------------------------------------------------------- 3. hand vectors
def _one(G, pos, oid, aligned, inv, ptr=None):
    pos = np.asarray(pos, dtype=np.float64)
    out = G.create_2d_bounding_boxes_batched(pos, np.asarray(oid, dtype=np.int64), ptr or [0, len(pos)], aligned, inv,
                                             return_rect=True)
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def test_hand_right_triangle(G):
    # 3-4-5: flush with a leg the rectangle is 4 x 3 (area exactly 12); flush with the hypotenuse 5 x 2.4 = 12.000000000000002 in
    # float64 without FMA.  The leg at the lowest hull position wins: centre (2, 1.5), l 4, w 3, theta 0.
    pos = [[0.0, 0.0], [4.0, 0.0], [0.0, 3.0]]
    boxes, rect = _one(G, pos, [0, 0, 0], False, "none")
    assert np.array_equal(rect, [[2.0, 1.5, 4.0, 3.0, 0.0]])
    assert np.array_equal(boxes, np.tile([2.0, 1.5, 4.0, 3.0, 0.0], (3, 1)))
    boxes, _ = _one(G, pos, [0, 0, 0], False, "translation")
    assert np.array_equal(boxes, [[2.0, 1.5, 4.0, 3.0, 0.0], [-2.0, 1.5, 4.0, 3.0, 0.0], [2.0, -1.5, 4.0, 3.0, 0.0]])
    boxes, rect = _one(G, pos, [0, 0, 0], True, "none")
    assert np.array_equal(boxes, [[2.0, 1.5, 4.0, 3.0], [-2.0, 1.5, 4.0, 3.0], [2.0, -1.5, 4.0, 3.0]])
    assert np.array_equal(rect, [[2.0, 1.5, 4.0, 3.0, 0.0]])


def test_hand_unit_square_with_interior_point(G):
    pos = [[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.25, 0.5]]
    boxes, rect = _one(G, pos, [4, 4, 4, 4, 4], False, "translation")
    assert np.array_equal(rect[0, :4], [0.5, 0.5, 1.0, 1.0]) and rect[0, 4] % 90 == 0 and 0 <= rect[0, 4] < 180
    assert np.array_equal(boxes[:, :4], [[0.5, 0.5, 1, 1], [-0.5, 0.5, 1, 1], [-0.5, -0.5, 1, 1], [0.5, -0.5, 1, 1], [0.25, 0.0, 1, 1]])
    assert np.allclose(np.degrees(boxes[:, 4]) % 90, 0, rtol=0, atol=1e-12)


def test_hand_two_points_and_single_point(G):
    pos = [[1.0, 1.0], [9.0, 9.0], [4.0, 5.0], [7.0, 7.0]]                       # object 2: rows 0 and 2 (p1 = row 0); 6: row 3
    oid = [2, -1, 2, 6]
    boxes, rect = _one(G, pos, oid, False, "none")
    theta = np.arctan2(4.0 / 5.0, 3.0 / 5.0)
    assert np.array_equal(rect[0, :4], [2.5, 3.0, 5.0, 0.5]) and abs(rect[0, 4] - np.degrees(theta)) <= 1e-13
    assert np.array_equal(rect[1], [7.0, 7.0, 0.5, 0.5, 0.0])
    assert np.array_equal(boxes[[0, 2], :4], [[2.5, 3.0, 5.0, 0.5]] * 2) and np.abs(boxes[[0, 2], 4] - theta).max() <= 2e-15   # 16 ulp of 0.93
    assert np.isnan(boxes[1]).all() and np.array_equal(boxes[3], [7.0, 7.0, 0.5, 0.5, 0.0])
    boxes, _ = _one(G, pos, oid, False, "translation")
    assert np.array_equal(boxes[[0, 2], :2], [[1.5, 2.0], [-1.5, -2.0]]) and np.array_equal(boxes[3], [0, 0, 0.5, 0.5, 0])
    boxes, _ = _one(G, pos, oid, False, "en")
    assert np.array_equal(boxes[3], [0, 0, 0.5, 0.5, 0]) and np.isnan(boxes[1]).all()
    # row 0: nearest other point is row 2, which is also where the centre and the long side point: both angles 0, d = 2.5
    assert np.array_equal(boxes[0], [2.5, 0.0, 5.0, 0.5, 0.0])
    boxes, rect = _one(G, pos, oid, True, "none")
    assert np.array_equal(boxes[[0, 2, 3]], [[1.5, 2.0, 3.0, 4.0], [-1.5, -2.0, 3.0, 4.0], [0, 0, 0.5, 0.5]])
    pos_left = [[5.0, 2.0], [1.0, 2.0]]                                          # p2 - p1 = (-4, 0): 180 folds to 0
    _, rect = _one(G, pos_left, [0, 0], False, "none")
    assert np.array_equal(rect, [[3.0, 2.0, 4.0, 0.5, 0.0]])


def test_hand_background_only_and_empty_frames(G):
    rng = np.random.default_rng(5)
    pos = rng.uniform(-10, 10, size=(7, 2))
    for key, aligned, inv in MODES:
        boxes, rect = _one(G, pos, [-1] * 7, aligned, inv)
        assert boxes.shape == (7, 4 if aligned else 5) and np.isnan(boxes).all() and rect.shape == (0, 5)
    g = np.load(FIXTURES[0])
    a, b, c = g["frame_ptr"][0], g["frame_ptr"][1], g["frame_ptr"][2]
    pos, oid = g["pos"][a:c], g["object_id"][a:c]
    for key, aligned, inv in MODES:
        boxes, _ = _one(G, pos, oid, aligned, inv, ptr=[0, b - a, b - a, c - a])   # an empty frame between two full ones
        plain, _ = _one(G, pos, oid, aligned, inv, ptr=[0, b - a, c - a])
        assert np.array_equal(boxes, plain, equal_nan=True)
    empty = G.create_2d_bounding_boxes_batched(np.zeros((0, 2)), np.zeros(0, dtype=np.int64), [0, 0], False, "none")
    assert empty.shape == (0, 5)


def test_en_needs_two_points_in_the_frame(G):
    with pytest.raises(ValueError, match="n_neighbors"):
        G.create_2d_bounding_boxes_batched(np.array([[1.0, 2.0]]), np.array([0]), [0, 1], False, "en")


# ---------------------------------------------------------------------------------------------- 4. batch == frames, repeatable
@pytest.mark.parametrize("key,aligned,inv", MODES, ids=[m[0] for m in MODES])
def test_batch_equals_frames_bitwise(G, key, aligned, inv):
    g = np.load(FIXTURES[0])
    pos, oid, ptr = g["pos"], g["object_id"], g["frame_ptr"].tolist()
    batched = G.create_2d_bounding_boxes_batched(pos, oid, ptr, aligned, inv).cpu().numpy()
    again = G.create_2d_bounding_boxes_batched(pos, oid, ptr, aligned, inv).cpu().numpy()
    assert np.array_equal(batched.view(np.int64), again.view(np.int64))
    for a, b in zip(ptr[:-1], ptr[1:]):
        single = G.create_2d_bounding_boxes_batched(pos[a:b], oid[a:b], [0, b - a], aligned, inv).cpu().numpy()
        assert np.array_equal(single.view(np.int64), batched[a:b].view(np.int64))


# ---------------------------------------------------------------------------------------------- 5. row order
@pytest.mark.parametrize("key,aligned,inv", MODES, ids=[m[0] for m in MODES])
def test_row_order_does_not_matter(G, key, aligned, inv):
    g = np.load(FIXTURES[0])
    a, b = g["frame_ptr"][0], g["frame_ptr"][1]
    pos, oid = g["pos"][a:b], g["object_id"][a:b]
    perm = np.random.default_rng(3).permutation(b - a)
    base = G.create_2d_bounding_boxes_batched(pos, oid, [0, b - a], aligned, inv).cpu().numpy()
    moved = G.create_2d_bounding_boxes_batched(pos[perm], oid[perm], [0, b - a], aligned, inv).cpu().numpy()
    sizes = {i: (oid == i).sum() for i in np.unique(oid[oid >= 0])}
    two = np.array([i >= 0 and sizes[i] == 2 for i in oid])
    assert two.sum() == 2
    assert np.array_equal(moved[~two[perm]].view(np.int64), base[perm][~two[perm]].view(np.int64))
    if aligned:
        assert np.array_equal(moved.view(np.int64), base[perm].view(np.int64))
        return
    # two points: p1 is the lower row, so a swap turns p2 - p1 round; centre, l, w and the folded theta stay (to rounding: the
    # direction is normalised before atan2)
    _, rect_a = _one(G, pos, oid, False, "none")
    _, rect_b = _one(G, pos[perm], oid[perm], False, "none")
    assert np.array_equal(rect_a[:, :4], rect_b[:, :4])
    assert _angle_diff(rect_a[:, 4], rect_b[:, 4], 180).max() <= 1e-12


# ---------------------------------------------------------------------------------------------- 6. refusals
def _with_valid_object(bad_pos, rng):
    """bad object (id 0) + a valid 5-point object (id 1) + 3 background points; -> pos, oid."""
    good = (rng.normal(size=(5, 2)) * [3.0, 0.7] + [20.0, -5.0]).astype(np.float32).astype(np.float64)
    bgp = rng.uniform(-40, 40, size=(3, 2))
    pos = np.concatenate((bad_pos, good, bgp))
    oid = np.concatenate((np.zeros(len(bad_pos)), np.ones(5), -np.ones(3))).astype(np.int64)
    return pos, oid


def _refused(G, pos, oid, bit_name, aligned=False):
    from radargnn_amd import ops
    with pytest.raises(ValueError, match=bit_name):
        G.create_2d_bounding_boxes_batched(pos, oid, [0, len(pos)], aligned, "translation")
    p = torch.from_numpy(pos).cuda()
    obj_ptr, obj_rows = ops.group_objects(torch.from_numpy(oid).cuda(), torch.tensor([0, len(pos)], device="cuda"))
    boxes, rect, status = ops.create_gt_boxes(p, obj_ptr, obj_rows, None, aligned, 1, want_rect=True)
    torch.cuda.synchronize()                                           # the kernel returned normally
    assert status.item() == getattr(ops, "STATUS_" + bit_name)
    boxes = boxes.cpu().numpy()
    assert np.isnan(boxes[oid == 0]).all() and np.isnan(boxes[oid < 0]).all() and np.isnan(rect[0].cpu().numpy()).all()
    keep = oid == 1
    want, _ = O.create_boxes(pos[keep], oid[keep], np.array([0, keep.sum()]), aligned, "translation")
    assert np.abs(boxes[keep] - want).max() <= bars()["aligned" if aligned else "translation"]
    return boxes


def test_object_over_the_cap_is_refused_and_the_cap_itself_works(G):
    from radargnn_amd import ops
    cap = ops.gt_object_cap()
    assert cap >= 1024
    rng = np.random.default_rng(8)
    big = (rng.normal(size=(cap + 1, 2)) * [4.0, 1.0]).astype(np.float32).astype(np.float64)
    pos, oid = _with_valid_object(big, rng)
    _refused(G, pos, oid, "GT_OBJECT_TOO_LARGE")
    _refused(G, pos, oid, "GT_OBJECT_TOO_LARGE", aligned=True)
    pos, oid = _with_valid_object(big[:cap], rng)
    assert O.is_admissible(pos, oid, np.array([0, len(pos)]))
    for key, aligned, inv in MODES:
        got = G.create_2d_bounding_boxes_batched(pos, oid, [0, len(pos)], aligned, inv).cpu().numpy()
        want, _ = O.create_boxes(pos, oid, np.array([0, len(pos)]), aligned, inv)
        check_boxes(got, want, key, bars()[key], "cap")


def test_degenerate_objects_are_refused(G):
    rng = np.random.default_rng(9)
    pos, oid = _with_valid_object(np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]]), rng)           # three collinear points
    _refused(G, pos, oid, "GT_DEGENERATE_OBJECT")
    pos, oid = _with_valid_object(np.array([[3.0, -2.0], [3.0, -2.0]]), rng)                      # two coincident points
    _refused(G, pos, oid, "GT_DEGENERATE_OBJECT")
    pos, oid = _with_valid_object(np.array([[3.0, -2.0]] * 4), rng)                               # four points in one place
    _refused(G, pos, oid, "GT_DEGENERATE_OBJECT")


# ---------------------------------------------------------------------------------------------- 7. fuzz
@pytest.fixture(scope="module")
def fuzz_clouds():
    clouds = []
    for seed in range(20):
        rng = np.random.default_rng(1000 + seed)
        frames = []
        for _ in range(int(rng.integers(1, 4))):
            sizes, left = [], int(rng.integers(40, 90))
            while left > 0 and len(sizes) < 6:
                sizes.append(int(min(rng.integers(1, 81), left)))
                left -= sizes[-1]
            frames.append(sizes)
        clouds.append(O.draw_admissible(5000 + seed, frames, int(rng.integers(2, 10))))
    return clouds


def test_fuzz_against_the_oracle(G, fuzz_clouds):
    worst = {}
    for cloud, (pos, oid, ptr, _) in enumerate(fuzz_clouds):
        assert len(pos) <= 300 and O.is_admissible(pos, oid, ptr)                  # the same filter as the fixture maker
        for key, aligned, inv in MODES:
            got = G.create_2d_bounding_boxes_batched(pos, oid, ptr.tolist(), aligned, inv).cpu().numpy()
            want, _ = O.create_boxes(pos, oid, ptr, aligned, inv)
            p, a = check_boxes(got, want, key, bars()[key], f"cloud {cloud}")
            worst[key] = max(worst.get(key, 0.0), p)
            worst[key + "_angles"] = max(worst.get(key + "_angles", 0.0), a)
    record_parity("groundtruth_gpu_vs_oracle_fuzz", **worst)
