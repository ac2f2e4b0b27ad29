"""nuScenes samples on the device (csrc/nuscenes.hip through radargnn_amd.nuscenes / ops) against the reference-generated
fixtures (tests/golden/nuscenes_*.npz), hand vectors and the numpy oracle (tests/nuscenes_oracle.py).

Bars.  Everything discrete -- kept rows and their order, frame_ptr, labels, surviving boxes, NaN rows -- is compared exactly.  A
float column is compared with the REFERENCE's value at 10 x the difference between the oracle and the reference on the same
fixture, stage and mode (test_nuscenes_oracle.oracle_differences), with a floor of 8 ulp of the column's largest magnitude: oracle
and reference can agree to the bit on a column where the device's atan2, sincos or association does not.  The two en angles get
the reference's rounding quantum (1e-5 degrees in radians) on top.  Against the oracle (fuzz, where no reference ran) the bar is
the same quantity taken from the worst fixture.  Values cast to float32 (pos, vel, y of the final Data) get one float32 spacing
of the column's largest magnitude on top: a float64 difference inside the bar can sit on a float32 rounding boundary.
Measured figures: MEASUREMENTS.md "nuScenes samples".
"""
import os

import numpy as np
import pytest
import torch

import nuscenes_oracle as O
from conftest import record_parity
from test_nuscenes_oracle import EN_QUANTUM, FIXTURES, IDS, inputs, oracle_differences, settings

pytestmark = pytest.mark.gpu
_DIFF = {}


def diffs(path=None):
    """{stage or mode: |oracle - reference|} of one fixture (or the worst over all fixtures), computed once."""
    for p in FIXTURES:
        if p not in _DIFF:
            _DIFF[p] = {k: v[0] for k, v in oracle_differences(np.load(p)).items()}
    if path is not None:
        return _DIFF[path]
    return {k: max(d[k] for d in _DIFF.values()) for k in next(iter(_DIFF.values()))}


def check_columns(got, ref, diff, what, angles=(), extra=None):
    """got / ref [N, C]: same NaN pattern; column c within max(10 x diff, 8 ulp of max |ref[:, c]|) (+ the rounding quantum for the
    columns in `angles`, + `extra[c]`).  -> the worst difference and the widest bar."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    worst, widest = 0.0, 0.0
    for c in range(ref.shape[1] if ref.size else 0):
        col = ref[:, c][~np.isnan(ref[:, c])]
        if col.size == 0:
            continue
        bar = max(10 * diff, 8 * np.spacing(np.abs(col).max())) + (EN_QUANTUM if c in angles else 0.0) + (0.0 if extra is None else extra[c])
        d = np.abs(np.nan_to_num(got[:, c] - ref[:, c])).max()
        print(f"[nuscenes] {what} column {c}: {d:.2e} (bar {bar:.2e})")
        assert d <= bar, (what, c, d, bar)
        worst, widest = max(worst, d), max(widest, bar)
    return worst, widest


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radargnn_amd import nuscenes
    return nuscenes


def config(N, crop, xlim, ylim, factor, offset, inv="translation"):
    return N.NuScenesDatasetConfiguration(nsweeps=3, crop_point_cloud=crop, crop_settings={"x": xlim, "y": ylim}, wlh_factor=factor,
                                          wlh_offset=offset, bb_invariance=inv)


def run_stages(N, inp, cfg, modes=O.MODES):
    """All stages on the device -> dict of numpy arrays with the oracle's keys."""
    samples = N.NuScenesSamples(**inp)
    batch, v_cc, src_row = N.sample_point_clouds(samples, cfg)
    boxes = N.prepare_boxes(samples, cfg)
    kept, kept_ptr, rect, label = boxes.survivors()
    out = {"frame_ptr": batch.frame_ptr.cpu().numpy(), "X": batch.X.cpu().numpy(), "V": batch.V.cpu().numpy(), "V_cc": v_cc.cpu().numpy(),
           "rcs": batch.rcs.cpu().numpy(), "timestamp": batch.timestamp.cpu().numpy(), "src_row": src_row.cpu().numpy(),
           "kept": kept.cpu().numpy(), "kept_ptr": kept_ptr.cpu().numpy(), "rect": rect.cpu().numpy(), "label": label.cpu().numpy()}
    assert np.array_equal(out["frame_ptr"], np.concatenate(([0], np.cumsum(batch.frame_sizes))))
    for mode in modes:
        labels, targets, hit = N.label_points(batch.X, batch.frame_ptr, boxes, mode, cfg.wlh_offset)
        assert labels.dtype == torch.int32 and targets.dtype == torch.float64 and targets.is_cuda
        out["labels_" + mode], out["boxes_" + mode], out["hit_" + mode] = labels.cpu().numpy(), targets.cpu().numpy(), hit.cpu().numpy()
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------- 1. fixtures
@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_stages_match_reference_fixtures(N, path):
    g = np.load(path)
    crop, xlim, ylim, factor, offset = settings(g)
    diff, ref, worst = diffs(path), g["ref_points"], {}
    got = run_stages(N, inputs(g), config(N, crop, xlim, ylim, factor, offset))
    assert np.array_equal(got["frame_ptr"], g["ref_frame_ptr"])
    rows = got["src_row"]
    assert np.array_equal(g["points"][3:8, rows], ref[3:8]) and np.array_equal(g["points"][10:, rows], ref[10:])   # kept rows, in order
    assert same_bits(got["rcs"], ref[5]) and same_bits(got["timestamp"], ref[18]) and same_bits(got["V_cc"], np.ascontiguousarray(ref[6:8].T))
    worst["points"], worst["points_bar"] = check_columns(got["X"], ref[:2].T, diff["points"], "points")
    worst["velocity"], worst["velocity_bar"] = check_columns(got["V"], ref[8:10].T, diff["velocity"], "velocity")
    assert np.array_equal(got["kept"], g["ref_kept"]) and np.array_equal(got["kept_ptr"], g["ref_kept_ptr"])
    assert np.array_equal(got["label"], g["box_label"][g["ref_kept"]])
    worst["rect"], worst["rect_bar"] = check_columns(got["rect"], g["ref_rect"], diff["rect"], "rect")
    for mode in O.MODES:
        assert np.array_equal(got["labels_" + mode], g["ref_labels"]), mode
        want = g["ref_boxes_" + mode]
        assert np.array_equal(got["hit_" + mode] < 0, np.isnan(want).all(1)) and np.array_equal(np.isnan(want).all(1), np.isnan(want).any(1))
        worst[mode], worst[mode + "_bar"] = check_columns(got["boxes_" + mode], want, diff[mode], mode, angles=(1, 4) if mode == "en" else ())
    record_parity("nuscenes_gpu_vs_reference_" + os.path.basename(path)[9:-4], **worst)


@pytest.mark.parametrize("path,mode", [(p, m) for p in FIXTURES for m in O.MODES], ids=[f"{i}-{m}" for i in IDS for m in O.MODES])
def test_graph_data_matches_reference_and_the_per_frame_path(N, path, mode):
    from radargnn_amd.data import GraphStore, create_graph_data
    from radargnn_amd.graph_constructor.configs import GraphConstructionConfiguration
    from radargnn_amd.graph_constructor.graph import build_geometric_graph
    g = np.load(path)
    crop, xlim, ylim, factor, offset = settings(g)
    cfg = config(N, crop, xlim, ylim, factor, offset, mode)
    graph_config = GraphConstructionConfiguration("knn", {"k": 5, "r": 6.0}, ["rcs", "velocity_vector", "time_index", "degree"],
                                                  ["relative_position"], "directed", "X")
    samples = N.NuScenesSamples(**inputs(g))
    graphs = N.create_graph_data_from_samples(samples, graph_config, cfg)
    stages = run_stages(N, inputs(g), cfg, modes=(mode,))
    ptr, ref, diff = g["ref_frame_ptr"], g["ref_points"], diffs(path)
    assert len(graphs) == len(ptr) - 1
    y_ref = np.concatenate((g["ref_labels"].reshape(-1, 1).astype(np.float64), g["ref_boxes_" + mode]), axis=1)
    for s, d in enumerate(graphs):
        a, b = ptr[s], ptr[s + 1]
        assert all(getattr(d, k).is_cuda for k in d.keys)
        assert d.y.dtype == torch.float32 and d.y.shape == (b - a, 6) and d.edge_index.dtype == torch.int64
        assert same_bits(d.y[:, 0].cpu().numpy().astype(np.int64), g["ref_labels"][a:b])
        one = lambda ref_cols: np.array([np.spacing(np.float32(np.nanmax(np.abs(c), initial=0.0))) for c in ref_cols.T], dtype=np.float64)
        check_columns(d.pos.cpu().numpy(), ref[:2, a:b].T.astype(np.float32), diff["points"], f"pos {s}", extra=one(ref[:2, a:b].T))
        check_columns(d.vel.cpu().numpy(), ref[8:10, a:b].T.astype(np.float32), diff["velocity"], f"vel {s}", extra=one(ref[8:10, a:b].T))
        check_columns(d.y.cpu().numpy(), y_ref[a:b].astype(np.float32), diff[mode], f"y {s}", angles=(2, 5) if mode == "en" else (),
                      extra=one(y_ref[a:b]))
        # the per-frame path on the device's own stage outputs: bit for bit
        cloud = type("Cloud", (), dict(X_cc=stages["X"][a:b], V_cc_compensated=stages["V"][a:b], rcs=stages["rcs"][a:b].reshape(-1, 1),
                                       timestamp=stages["timestamp"][a:b].reshape(-1, 1), label_id=stages["labels_" + mode][a:b].reshape(-1, 1)))()
        want = create_graph_data(build_geometric_graph(graph_config, cloud), cloud.label_id, stages["boxes_" + mode][a:b], cloud)
        assert d.keys == want.keys
        for k in want.keys:
            u, v = getattr(d, k), getattr(want, k)
            assert u.dtype == v.dtype and u.shape == v.shape, (k, u.shape, v.shape)
            assert u.cpu().contiguous().numpy().tobytes() == v.cpu().contiguous().numpy().tobytes(), (k, s)
    batch = GraphStore(graphs).collate(list(range(len(graphs))))
    assert batch.num_graphs == len(graphs) and batch.y.shape == (ptr[-1], 6) and batch.x.shape[0] == ptr[-1]


# ---------------------------------------------------------------------------------------------- 2. hand vectors
IDENT = [1.0, 0.0, 0.0, 0.0]
HALF_TURN = [0.0, 0.0, 0.0, 1.0]                  # a yaw of exactly 180 degrees: R = diag(-1, -1, 1) without rounding


def hand(samples):
    """A batch from per-sample (chunks, boxes): chunks = list of (xy [n, 2], rotation, translation), boxes = list of
    (centre xyz, (w, l, h), rotation, label, points).  Channel 5 carries the row number, channels 6-9 simple velocities."""
    parts = []
    for chunks, boxes in samples:
        n = sum(len(c[0]) for c in chunks)
        pts = np.zeros((19, n))
        at, ptr = 0, [0]
        for xy, _, _ in chunks:
            xy = np.reshape(np.asarray(xy, dtype=np.float64), (-1, 2))
            pts[:2, at:at + len(xy)] = xy.T
            at += len(xy)
            ptr.append(at)
        pts[5], pts[6], pts[7], pts[8], pts[9], pts[18] = np.arange(n), 1.0, 2.0, 3.0, -4.0, 0.5
        parts.append({"points": pts, "chunk_ptr": np.asarray(ptr, dtype=np.int64),
                      "chunk_rotation": np.reshape([c[1] for c in chunks], (-1, 4)).astype(np.float64),
                      "chunk_translation": np.reshape([c[2] for c in chunks], (-1, 3)).astype(np.float64),
                      "box_center": np.reshape([b[0] for b in boxes], (-1, 3)).astype(np.float64),
                      "box_size": np.reshape([b[1] for b in boxes], (-1, 3)).astype(np.float64),
                      "box_rotation": np.reshape([b[2] for b in boxes], (-1, 4)).astype(np.float64),
                      "box_label": np.asarray([b[3] for b in boxes], dtype=np.int32), "box_points": np.asarray([b[4] for b in boxes], dtype=np.int32),
                      "ego_translation": np.zeros(3), "ego_rotation": np.asarray(IDENT)})
    return O.concat_samples(parts)


def run_hand(N, inp, crop=None, factor=1.0, offset=0.0, mode="translation"):
    cfg = config(N, crop is not None, *(crop or (0.0, 0.0)), factor, offset)
    return run_stages(N, inp, cfg, modes=(mode,))


def plain(xy):
    return [(xy, IDENT, [0.0, 0.0, 0.0])]


BOX = ([3.0, 1.0, 0.5], (2.0, 4.0, 1.0), IDENT, 4, 1)           # x in [1, 5], y in [0, 2]
NAN5 = [np.nan] * 5


def test_hand_faces_and_offset(N):
    xy = [[5.0, 2.0], [5.5, 2.0], [1.0, 0.0], [0.5, 0.0], [3.0, 2.5], [6.0, 1.0]]
    got = run_hand(N, hand([(plain(xy), [BOX])]), mode="none")
    assert np.array_equal(got["labels_none"], [4, 0, 4, 0, 0, 0])                      # exactly on a face is inside
    assert np.array_equal(got["rect"], [[3.0, 1.0, 4.0, 2.0, 0.0]])
    assert np.array_equal(got["boxes_none"], [[3.0, 1.0, 4.0, 2.0, 0.0], NAN5, [3.0, 1.0, 4.0, 2.0, 0.0], NAN5, NAN5, NAN5], equal_nan=True)
    got = run_hand(N, hand([(plain(xy), [BOX])]), offset=0.5)
    assert np.array_equal(got["labels_translation"], [4, 4, 4, 4, 4, 0])               # one offset outside is inside with that offset
    assert np.array_equal(got["boxes_translation"][:5], [[-2.0, -1.0, 4.0, 2.0, 0.0], [-2.5, -1.0, 4.0, 2.0, 0.0], [2.0, 1.0, 4.0, 2.0, 0.0],
                                                         [2.5, 1.0, 4.0, 2.0, 0.0], [0.0, -1.5, 4.0, 2.0, 0.0]])
    got = run_hand(N, hand([(plain(xy), [BOX])]), factor=1.5)                          # x in [0, 6], y in [-0.5, 2.5]; the target is not inflated
    assert np.array_equal(got["labels_translation"], [4, 4, 4, 4, 4, 4]) and np.array_equal(got["boxes_translation"][5], [-3.0, 0.0, 4.0, 2.0, 0.0])


def test_hand_crop_limits(N):
    xy = [[10.0, 0.0], [10.5, 0.0], [-10.0, -8.0], [0.0, 8.5], [0.0, -8.0], [-10.5, 0.0], [2.0, 3.0]]
    boxes = [([10.0, 0.0, 0.5], (2.0, 4.0, 1.0), IDENT, 1, 1), ([9.5, 0.0, 0.5], (2.0, 4.0, 1.0), IDENT, 2, 1),
             ([0.0, -8.0, 0.5], (2.0, 4.0, 1.0), IDENT, 3, 1), ([0.0, 7.5, 0.5], (2.0, 4.0, 1.0), IDENT, 4, 1),
             ([-10.0, 0.0, 0.5], (2.0, 4.0, 1.0), IDENT, 5, 1)]
    got = run_hand(N, hand([(plain(xy), boxes)]), crop=(10.0, 8.0))
    assert np.array_equal(got["src_row"], [0, 2, 4, 6]) and np.array_equal(got["frame_ptr"], [0, 4])     # on the limit: stays
    assert np.array_equal(got["X"], [[10.0, 0.0], [-10.0, -8.0], [0.0, -8.0], [2.0, 3.0]])
    assert np.array_equal(got["kept"], [1, 3]) and np.array_equal(got["kept_ptr"], [0, 2])             # a centre on the limit: goes
    assert np.array_equal(got["labels_translation"], [2, 0, 0, 0])
    got = run_hand(N, hand([(plain(xy), boxes)]))                                      # crop_point_cloud = False: nothing goes
    assert np.array_equal(got["src_row"], np.arange(7)) and np.array_equal(got["kept"], np.arange(5))


def test_hand_last_box_wins_and_swapping_swaps(N):
    a = ([3.0, 1.0, 0.5], (2.0, 4.0, 1.0), IDENT, 4, 1)
    b = ([4.0, 1.0, 0.5], (2.0, 6.0, 1.0), IDENT, 7, 1)                           # x in [1, 7]
    xy = [[2.0, 1.0], [6.0, 1.0], [0.0, 0.0]]
    got = run_hand(N, hand([(plain(xy), [a, b])]))
    assert np.array_equal(got["labels_translation"], [7, 7, 0]) and np.array_equal(got["hit_translation"], [1, 1, -1])
    assert np.array_equal(got["boxes_translation"][:2], [[2.0, 0.0, 6.0, 2.0, 0.0], [-2.0, 0.0, 6.0, 2.0, 0.0]])   # its label AND its box
    got = run_hand(N, hand([(plain(xy), [b, a])]))
    assert np.array_equal(got["labels_translation"], [4, 7, 0]) and np.array_equal(got["hit_translation"], [1, 0, -1])
    assert np.array_equal(got["boxes_translation"][:2], [[1.0, 0.0, 4.0, 2.0, 0.0], [-2.0, 0.0, 6.0, 2.0, 0.0]])
    got = run_hand(N, hand([(plain(xy), [a, ([4.0, 1.0, 0.5], (2.0, 6.0, 1.0), IDENT, 7, 0)])]))      # the later box has no points: dropped
    assert np.array_equal(got["labels_translation"], [4, 0, 0]) and np.array_equal(got["kept"], [0])


def test_hand_square_wide_and_half_turn(N):
    square = ([3.0, 1.0, 0.5], (2.0, 2.0, 1.0), IDENT, 1, 1)
    wide = ([3.0, 1.0, 0.5], (4.0, 2.0, 1.0), IDENT, 2, 1)                          # w > l: y in [-1, 3], x in [2, 4]
    turned = ([3.0, 1.0, 0.5], (2.0, 4.0, 1.0), HALF_TURN, 3, 1)
    flat = ([3.0, 1.0, 0.5], (2.0, 0.0, 1.0), IDENT, 5, 1)                          # zero length: 0 / 0, contains nothing
    xy = [[3.0, 1.0], [3.0, 3.0], [5.0, 1.0]]
    got = run_hand(N, hand([(plain(xy), [square]), (plain(xy), [wide]), (plain(xy), [turned]), (plain(xy), [flat])]))
    # a square takes p1 - p2 (90 degrees at yaw 0); a box wider than long swaps l and w; a half turn keeps theta = 180
    assert np.array_equal(got["rect"][:3], [[3.0, 1.0, 2.0, 2.0, 90.0], [3.0, 1.0, 4.0, 2.0, 90.0], [3.0, 1.0, 4.0, 2.0, 180.0]])
    assert np.array_equal(got["rect"][3, :4], [3.0, 1.0, 2.0, 0.0])
    assert np.array_equal(got["labels_translation"], [1, 0, 0, 2, 2, 0, 3, 0, 3, 0, 0, 0])
    assert np.array_equal(got["boxes_translation"][[0, 3, 4, 6, 8]],
                          [[0.0, 0.0, 2.0, 2.0, (90.0 * np.pi) / 180], [0.0, 0.0, 4.0, 2.0, (90.0 * np.pi) / 180],
                           [0.0, -2.0, 4.0, 2.0, (90.0 * np.pi) / 180], [0.0, 0.0, 4.0, 2.0, np.pi], [-2.0, 0.0, 4.0, 2.0, np.pi]])
    assert np.isnan(got["boxes_translation"][9:]).all()


def _grid(n_boxes, n_points):
    """Boxes 2 long and 1 wide at (4 k, 0), labels k + 1; point j sits at (0.5, 0.25) from the centre of box j mod n_boxes."""
    boxes = [([4.0 * k, 0.0, 0.5], (1.0, 2.0, 1.0), IDENT, k + 1, 1) for k in range(n_boxes)]
    xy = [[4.0 * (j % max(n_boxes, 1)) + 0.5, 0.25] for j in range(n_points)]
    return xy, boxes


def test_hand_box_and_point_counts_around_a_stage_and_a_wave(N):
    shapes = [(0, 2), (1, 63), (64, 64), (65, 65), (130, 257)]
    got = run_hand(N, hand([(plain(_grid(k, p)[0]), _grid(k, p)[1]) for k, p in shapes]))
    assert np.array_equal(got["frame_ptr"], np.cumsum([0] + [p for _, p in shapes]))
    assert np.array_equal(got["kept_ptr"], np.cumsum([0] + [k for k, _ in shapes]))
    want_label = np.concatenate([np.zeros(p, dtype=np.int64) if k == 0 else np.arange(p) % k + 1 for k, p in shapes])
    assert np.array_equal(got["labels_translation"], want_label)
    assert np.isnan(got["boxes_translation"][:2]).all()
    assert np.array_equal(got["boxes_translation"][2:], np.tile([-0.5, -0.25, 2.0, 1.0, 0.0], (len(want_label) - 2, 1)))
    assert np.array_equal(got["rect"][:, 0], np.concatenate([4.0 * np.arange(k) for k, _ in shapes]))


def test_hand_chunks_empty_first_and_turned(N):
    xy = np.array([[1.0, 2.0], [3.0, -4.0], [0.5, 0.25]])
    none = np.zeros((0, 2))
    turned = (xy, HALF_TURN, [1.0, 2.0, 0.0])                                     # x' = 1 - x, y' = 2 - y, v' = -v
    inp = hand([([(none, IDENT, [9.0, 9.0, 9.0]), turned], []), ([(xy, IDENT, [0.5, 0.0, 7.0]), (none, IDENT, [0.0, 0.0, 0.0])], []),
                ([(none, IDENT, [0.0, 0.0, 0.0])], [])])
    got = run_hand(N, inp)
    assert np.array_equal(got["frame_ptr"], [0, 3, 6, 6]) and np.array_equal(got["src_row"], np.arange(6))
    assert np.array_equal(got["X"], [[0.0, 0.0], [-2.0, 6.0], [0.5, 1.75], [1.5, 2.0], [3.5, -4.0], [1.0, 0.25]])
    assert np.array_equal(got["V"], [[-3.0, 4.0]] * 3 + [[3.0, -4.0]] * 3)        # channels 8-9 turned ...
    assert np.array_equal(got["V_cc"], [[1.0, 2.0]] * 6)                          # ... channels 6-7 as they are
    assert np.array_equal(got["rcs"], [0, 1, 2, 0, 1, 2]) and np.array_equal(got["timestamp"], [0.5] * 6)
    assert np.array_equal(got["labels_translation"], np.zeros(6)) and np.isnan(got["boxes_translation"]).all()


# ---------------------------------------------------------------------------------------------- 3. invariants
@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_batched_equals_single_samples_and_repeats_bitwise(N, path):
    g = np.load(path)
    cfg = config(N, *settings(g))
    inp = inputs(g)
    whole, again = run_stages(N, inp, cfg), run_stages(N, inp, cfg)
    for k in whole:
        assert same_bits(whole[k], again[k]), k
    fp, kp = whole["frame_ptr"], whole["kept_ptr"]
    for s in range(3):
        one = run_stages(N, O.take_samples(inp, [s]), cfg)
        for k in ("X", "V", "V_cc", "rcs", "timestamp") + tuple(f"{n}_{m}" for n in ("labels", "boxes") for m in O.MODES):
            assert same_bits(one[k], whole[k][fp[s]:fp[s + 1]]), (k, s)
        for k in ("rect", "label"):
            assert same_bits(one[k], whole[k][kp[s]:kp[s + 1]]), (k, s)
        assert np.array_equal(one["kept"] + inp["box_ptr"][s], whole["kept"][kp[s]:kp[s + 1]])
    for mode in O.MODES:       # the membership used for the labels is the one of the targets
        assert np.array_equal(whole["labels_" + mode] > 0, ~np.isnan(whole["boxes_" + mode]).any(1))
        assert np.array_equal(whole["hit_" + mode] >= 0, ~np.isnan(whole["boxes_" + mode]).all(1))


def test_permuting_boxes_that_do_not_overlap_changes_nothing(N):
    xy, boxes = _grid(65, 65)
    base = run_hand(N, hand([(plain(xy), boxes)]), mode="en")
    perm = np.random.default_rng(4).permutation(65)
    moved = run_hand(N, hand([(plain(xy), [boxes[i] for i in perm])]), mode="en")
    assert same_bits(base["labels_en"], moved["labels_en"]) and same_bits(base["boxes_en"], moved["boxes_en"])
    assert np.array_equal(perm[moved["hit_en"]], base["hit_en"])


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_a_sample_cropped_to_one_point_is_named(N):
    from radargnn_amd.graph_constructor.configs import GraphConstructionConfiguration
    graph_config = GraphConstructionConfiguration("knn", {"k": 1, "r": 6.0}, ["rcs"], ["relative_position"], "directed", "X")
    xy = [[1.0, 1.0], [2.0, 2.0], [3.0, 1.0]]
    inp = hand([(plain(xy), [BOX]), (plain([[1.0, 1.0], [50.0, 0.0], [60.0, 0.0]]), [BOX]), (plain(xy), [])])
    with pytest.raises(ValueError, match=r"samples \[1\]"):
        N.create_graph_data_from_samples(N.NuScenesSamples(**inp), graph_config, config(N, True, 10.0, 10.0, 1.0, 0.0))
    graphs = N.create_graph_data_from_samples(N.NuScenesSamples(**O.take_samples(inp, [0, 2])), graph_config, config(N, True, 10.0, 10.0, 1.0, 0.0))
    assert [d.y.shape for d in graphs] == [(3, 6), (3, 6)] and np.array_equal(graphs[0].y[:, 0].cpu().numpy(), [4, 4, 4])


def test_cpu_tensors_are_refused(N):
    from radargnn_amd import ops
    inp = hand([(plain([[1.0, 1.0], [2.0, 2.0]]), [BOX])])
    s = N.NuScenesSamples(**inp)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nusc_points(s.points.cpu(), s.chunk_ptr, s.chunk_sample, s.chunk_rotation, s.chunk_translation, 1, False, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nusc_boxes(s.box_center, s.box_size.cpu(), s.box_rotation, s.box_label, s.box_points, s.box_ptr, s.ego_translation,
                       s.ego_rotation, False, 0.0, 0.0, 1.0)
    boxes = N.prepare_boxes(s, config(N, False, 0.0, 0.0, 1.0, 0.0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        N.label_points(torch.zeros((2, 2), dtype=torch.float64), [0, 2], boxes, "none")


def test_bad_lists_set_their_status_bit_and_write_nothing_out_of_range(N):
    from radargnn_amd import ops
    xy = [[1.0, 1.0], [2.0, 2.0], [3.0, 1.0]]
    inp = hand([([(xy, IDENT, [0.0, 0.0, 0.0]), (xy, IDENT, [0.0, 0.0, 0.0])], [BOX, BOX]), (plain(xy), [BOX, BOX])])
    cfg = config(N, False, 0.0, 0.0, 1.0, 0.0)
    for bad in ([1, 0, 0], [0, 0, 2], [0, -1, 1]):                                 # decreasing; beyond the samples; negative
        s = N.NuScenesSamples(**{**inp, "chunk_sample": np.asarray(bad, dtype=np.int32)})
        out = ops.nusc_points(s.points, s.chunk_ptr, s.chunk_sample, s.chunk_rotation, s.chunk_translation, 2, False, 0.0, 0.0)
        torch.cuda.synchronize()                                                   # the kernels returned normally
        assert int(out[-1].item()) == ops.STATUS_NUSC_BAD_CHUNK
        ptr = out[0].cpu().numpy()
        assert ptr.shape == (3,) and ptr[0] == 0 and (np.diff(ptr) >= 0).all() and ptr[-1] <= 9 and out[1].shape == (9, 2)     # a chunk is read once
        with pytest.raises(ValueError, match="NUSC_BAD_CHUNK"):
            N.sample_point_clouds(s, cfg)
    for bad in ([0, 3, 12, 9], [0, 6, 3, 9]):                                      # beyond the rows; falling
        s = N.NuScenesSamples(**{**inp, "chunk_ptr": np.asarray(bad, dtype=np.int64)})
        out = ops.nusc_points(s.points, s.chunk_ptr, s.chunk_sample, s.chunk_rotation, s.chunk_translation, 2, False, 0.0, 0.0)
        torch.cuda.synchronize()
        assert int(out[-1].item()) == ops.STATUS_NUSC_BAD_CHUNK and out[0].shape == (3,) and out[1].shape == (9, 2) and out[6].shape == (9,)
    for bad in ([0, 5, 4], [0, 3, 2], [-1, 2, 4]):                                 # beyond the list; falling; negative
        s = N.NuScenesSamples(**{**inp, "box_ptr": np.asarray(bad, dtype=np.int64)})
        boxes = N.prepare_boxes(s, cfg)
        torch.cuda.synchronize()
        assert int(boxes.status.item()) == ops.STATUS_NUSC_BAD_BOX_PTR
        count = boxes.box_count.cpu().numpy()
        assert count.shape == (2,) and (count >= 0).all() and count.sum() <= 4 and boxes.records.shape == (4, 20)
        with pytest.raises(ValueError, match="NUSC_BAD_BOX_PTR"):
            boxes.survivors()
        labels, targets, hit = N.label_points(torch.tensor([[2.0, 1.0]] * 6, dtype=torch.float64, device="cuda"), [0, 3, 6], boxes, "none")
        torch.cuda.synchronize()
        assert labels.shape == (6,) and targets.shape == (6, 5)
    good = N.prepare_boxes(N.NuScenesSamples(**inp), cfg)
    labels, targets, hit, status = ops.nusc_label_points(torch.zeros((6, 2), dtype=torch.float64, device="cuda"),
                                                         torch.tensor([0, 7, 6], device="cuda"), good.records, good.box_ptr, good.box_count,
                                                         None, 0, 0.0)
    torch.cuda.synchronize()
    assert int(status.item()) == ops.STATUS_NUSC_BAD_CHUNK and (labels == 0).all() and torch.isnan(targets).all()


def test_reference_names_and_use_z(N):
    import gnnradarobjectdetection.preprocessor.nuscenes.configs as shim_configs
    import gnnradarobjectdetection.preprocessor.nuscenes.conversion as shim_conversion
    import gnnradarobjectdetection.preprocessor.nuscenes.utils as shim_utils
    assert shim_configs.NuScenesDatasetConfiguration is N.NuScenesDatasetConfiguration
    box = type("Box", (), dict(center=np.array([3.0, 1.0, 0.5]), wlh=np.array([2.0, 4.0, 1.0]),
                               orientation=type("Q", (), dict(q=np.array(IDENT)))(), label=4))()
    pts = np.array([[5.0, 5.5, 1.0, 0.5], [2.0, 2.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    assert shim_utils.extended_points_in_box(box, pts, use_z=False).cpu().tolist() == [True, False, True, False]
    assert shim_utils.extended_points_in_box(box, pts, wlh_offset=0.5, use_z=False).cpu().tolist() == [True] * 4
    with pytest.raises(NotImplementedError):
        shim_utils.extended_points_in_box(box, pts)
    cloud = shim_conversion.convert_point_cloud(np.vstack((pts[:2], np.zeros((17, 4)))), np.zeros(4))
    out = shim_conversion.convert_bounding_boxes(N.NuScenesDatasetConfiguration(bb_invariance="none"), cloud, [box])
    assert np.array_equal(out.cpu().numpy(), [[3.0, 1.0, 4.0, 2.0, 0.0], NAN5, [3.0, 1.0, 4.0, 2.0, 0.0], NAN5], equal_nan=True)
    with pytest.raises(ValueError, match="Wrong invariance"):
        shim_conversion.convert_bounding_boxes(N.NuScenesDatasetConfiguration(bb_invariance="polar"), cloud, [box])


def test_graphs_collate_and_a_model_trains_on_them(N):
    from radargnn_amd import gnn
    from radargnn_amd.data import GraphStore
    from radargnn_amd.gnn.losses import detection_loss
    from radargnn_amd.graph_constructor.configs import GraphConstructionConfiguration
    g = np.load(FIXTURES[0])
    graph_config = GraphConstructionConfiguration("knn", {"k": 5, "r": 6.0}, ["rcs", "velocity_vector", "time_index", "degree"],
                                                  ["relative_position"], "directed", "X")
    graphs = N.create_graph_data_from_samples(N.NuScenesSamples(**inputs(g)), graph_config, config(N, *settings(g)))
    batch = GraphStore(graphs).collate([0, 1, 2])
    assert batch.num_graphs == 3 and batch.y.shape == (g["ref_frame_ptr"][-1], 6)
    torch.manual_seed(0)
    model = gnn.DetNetBasic(gnn.GNNArchitectureConfig(5, 2, [64, 32], [11], [16, 5], True, True, [32, 64], [4, 8, 16], "MPNNConv", False)).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    before = [p.detach().clone() for p in model.parameters()]
    x, ea = batch.x.clone().requires_grad_(), batch.edge_attr.clone().requires_grad_()
    cls, bb = model(x, batch.edge_index, ea)
    assert cls.shape == (batch.y.shape[0], 11) and bb.shape == (batch.y.shape[0], 5)
    loss, loss_cls, loss_bb = detection_loss(cls, bb, batch.y, 0)                   # 0: the label of a point in no box
    loss.backward()
    opt.step()
    assert np.isfinite(float(loss.item())) and float(loss_bb.item()) > 0
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))


# ---------------------------------------------------------------------------------------------- 5. fuzz
@pytest.fixture(scope="module")
def fuzz_batches():
    out = []
    for seed in range(20):
        rng = np.random.default_rng(2000 + seed)
        shapes = [(int(rng.integers(8, 201)), int(rng.integers(0, 71)), None if rng.random() < 0.5 else int(rng.integers(0, 4)))
                  for _ in range(3)]
        factor, offset = ((1.0, 0.0), (1.1, 0.5), (1.0, 0.5), (0.9, 0.0))[seed % 4]
        crop = seed % 5 != 0
        inp, _ = O.draw_admissible(7000 + 10 * seed, shapes, crop, 40.0, 30.0, factor, offset)
        out.append((inp, crop, factor, offset))
    return out


def test_fuzz_against_the_oracle(N, fuzz_batches):
    diff, worst = diffs(), {}
    for batch, (inp, crop, factor, offset) in enumerate(fuzz_batches):
        assert O.is_admissible(inp, crop, 40.0, 30.0, factor, offset)              # the same filter as the fixture maker
        want = O.create(inp, crop, 40.0, 30.0, factor, offset)
        got = run_stages(N, inp, config(N, crop, 40.0, 30.0, factor, offset))
        assert np.array_equal(got["frame_ptr"], want["frame_ptr"]) and np.array_equal(got["src_row"], want["src_row"])
        assert np.array_equal(got["kept"], want["kept"]) and np.array_equal(got["kept_ptr"], want["kept_ptr"])
        assert same_bits(got["rcs"], want["rcs"]) and same_bits(got["V_cc"], np.ascontiguousarray(want["V_cc"]))
        pairs = [("points", got["X"], want["X"], ()), ("velocity", got["V"], want["V"], ()), ("rect", got["rect"], want["rect"], ())]
        for mode in O.MODES:
            assert np.array_equal(got["labels_" + mode], want["labels"]) and np.array_equal(got["hit_" + mode], want["hit"]), (batch, mode)
            pairs.append((mode, got["boxes_" + mode], want["boxes_" + mode], (1, 4) if mode == "en" else ()))
        for key, a, b, angles in pairs:
            worst[key] = max(worst.get(key, 0.0), check_columns(a, b, diff[key], f"batch {batch} {key}", angles=angles)[0])
    record_parity("nuscenes_gpu_vs_oracle_fuzz", **worst)
