"""The evaluation kernels (csrc/metrics.hip through radargnn_amd.ops) where a wave-level argmax, a ballot compaction or a chunked scan
goes subtly wrong, and where this project decides what the reference leaves open: equal, NaN and signed-zero scores, IoUs equal to a
threshold and the float32 rounding of that threshold, NaN IoUs, ``max_det`` from 1 to more than a class holds, class segments at the
chunk edges of the curves kernel, arbitrary recall thresholds, degenerate boxes, empty frames in the middle of a frame list, labels at
the truncation edges of the confusion matrix.  Everything is compared exactly with the numpy restatement tests/map_oracle.py, which
tests/test_map_oracle.py holds to torch's stable sort, to a float64 box IoU and to scikit-learn.  Every case comes from a seeded
generator and is built once; the generators run without a GPU."""
import functools
import os

import numpy as np
import pytest
import torch

import map_oracle as MO

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radargnn_amd import ops
    return ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def ptr_of(sizes):
    return np.cumsum([0] + [int(s) for s in sizes]).tolist()


def same_bits(got: np.ndarray, want: np.ndarray) -> bool:
    """Equal NaN positions, every other value bit for bit (so -0.0 is not 0.0)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    bits = np.uint32 if want.dtype == np.float32 else np.uint64
    return np.array_equal(got.view(bits)[ok], want.view(bits)[ok])


# ---- matcher ------------------------------------------------------------------------------------------------------------------------
# (detections, ground truth) across the 64-lane edge, with frames without detections, without ground truth and without either between
MATCH_SIZES = [(63, 65), (0, 7), (64, 64), (5, 0), (65, 63), (0, 0), (129, 130), (1, 1)]
NAN_FRAME = 6                                     # the frame whose classes 0 and 1 get a NaN IoU next to an IoU of 1
LABELS = [0, 1, 2, 4]                             # three classes, and 4: present but not asked for
ASKED = [0, 1, 2, 3]                              # 3: asked for but absent
THRESHOLDS = [0.25, 0.5, 0.75]                    # each equals some k/8 exactly: equality must not match
MAX_DETS = [1, 3, 100, 1000]
SCORE_LEVELS = np.array([0.9, 0.7, 0.5, 0.3, 0.1], dtype=np.float32)
SIDE = (6, 5)                                     # boxes of each other label in a frame of the "one_class" layout
# expected own-class candidates with a non-zero IoU per detection.  k/8 IoUs in every pair match nearly every detection (0.96 of them
# at (129, 130)), which would hide a wrong flag; these densities put the share matched at the middle threshold inside 5 % .. 95 % for
# every case, and the test asserts that on the restatement's output before it looks at the device
CANDIDATES = {"spread": 1.2, "one_class": 1.6}


def labels_of(layout, rng, f, count, side):
    """"spread": the frame holds exactly ``count`` boxes, their labels drawn from LABELS.  "one_class": ONE class holds exactly ``count``
    boxes of the frame (so that its ranks and its argmax straddle lanes 63 / 64 and 127 / 128) beside ``side`` boxes of every other label."""
    if count == 0:
        return np.zeros(0, dtype=np.int64)
    if count == 1:
        return np.array([f % 3], dtype=np.int64)
    if layout == "spread":
        return rng.choice(LABELS, size=count).astype(np.int64)
    main = LABELS[f % 3]
    return rng.permutation(np.concatenate([np.full(count if c == main else side, c) for c in LABELS])).astype(np.int64)


@functools.lru_cache(maxsize=None)
def match_case(layout: str, dtype_name: str):
    dtype = np.dtype(dtype_name).type
    rng = np.random.default_rng({"spread": 101, "one_class": 202}[layout] + (dtype_name == "float32"))
    ious, dl, ds, gl, nan_dets = [], [], [], [], []
    for f, (p, g) in enumerate(MATCH_SIZES):
        d_lab, g_lab = labels_of(layout, rng, f, p, SIDE[0]), labels_of(layout, rng, f, g, SIDE[1])
        p, g = len(d_lab), len(g_lab)
        scores = SCORE_LEVELS[rng.integers(0, len(SCORE_LEVELS), p)].copy()
        u = rng.uniform(size=p)
        for lo, value in ((0.00, -0.0), (0.08, 0.0), (0.16, np.nan), (0.24, 1e-40), (0.27, -1e-40)):      # through every class
            scores[(u >= lo) & (u < lo + (0.08 if lo < 0.24 else 0.03))] = value
        own = np.array([(g_lab == c).sum() for c in d_lab], dtype=np.float64).reshape(p, 1)           # ground truth of the row's class
        density = np.minimum(1.0, CANDIDATES[layout] / np.maximum(own, 1.0))
        iou = np.where(rng.uniform(size=(p, g)) < density, rng.integers(1, 9, size=(p, g)) / 8.0, 0.0).astype(dtype)
        if p == 1 and g == 1:
            iou[0, 0] = 0.625
        if f == NAN_FRAME:
            for c in (0, 1):
                d, gts = int(np.nonzero(d_lab == c)[0][0]), np.nonzero(g_lab == c)[0]
                assert len(gts) >= 2
                iou[:, gts[-1]] = 0                                       # nobody else takes the box that would match
                iou[d, gts[-1]], iou[d, gts[0]] = 1.0, np.nan
                scores[d] = np.nan                                        # first of its class by position and NaN: rank 0
                nan_dets.append((c, sum(len(x) for x in dl) + d))                 # its position in the packed list
        ious.append(iou)
        dl.append(d_lab), ds.append(scores), gl.append(g_lab)
    return {"ious": ious, "dl": dl, "ds": ds, "gl": gl, "nan_dets": nan_dets}


@functools.lru_cache(maxsize=None)
def match_want(layout: str, dtype_name: str, max_det: int):
    c = match_case(layout, dtype_name)
    return MO.match(c["ious"], c["dl"], c["ds"], c["gl"], ASKED, THRESHOLDS, max_det)


def check_match_case_can_fail(layout, dtype_name, max_det):
    """What the generated case holds, asserted on the restatement alone."""
    c = match_case(layout, dtype_name)
    rank, matched = match_want(layout, dtype_name, max_det)
    det_labels, det_scores = np.concatenate(c["dl"]), np.concatenate(c["ds"])
    selected = rank >= 0
    share = float(matched[1, selected].mean())
    print(f"[match] {layout} {dtype_name} max_det {max_det}: {int(selected.sum())} of {len(rank)} selected, matched at "
          f"{THRESHOLDS[1]}: {share:.3f}; per threshold {matched[:, selected].mean(axis=1).round(3).tolist()}")
    assert 0.05 <= share <= 0.95
    assert not selected[(det_labels == 4)].any() and (det_labels == 4).any() and not (det_labels == 3).any()
    for f, (iou, d_lab, g_lab) in enumerate(zip(c["ious"], c["dl"], c["gl"])):
        assert iou.dtype == np.dtype(dtype_name) and iou.shape == (len(d_lab), len(g_lab))
    counts = {(len(d), len(g)) for d, g in zip(c["dl"], c["gl"])} if layout == "spread" else \
        {(int((d == LABELS[f % 3]).sum()), int((g == LABELS[f % 3]).sum())) for f, (d, g) in enumerate(zip(c["dl"], c["gl"]))}
    assert counts == set(MATCH_SIZES)
    for cls in (0, 1, 2):                                                 # equal keys of every kind in every class
        s = det_scores[det_labels == cls]
        assert np.isnan(s).sum() >= 2 and ((s == 0) & np.signbit(s)).sum() >= 2 and ((s == 0) & ~np.signbit(s)).sum() >= 2
        assert len(np.unique(s[~np.isnan(s) & (np.abs(s) > 1e-30)])) == len(SCORE_LEVELS)
    # an IoU equal to a threshold is a candidate somewhere, and rows hold exact ties
    flat = np.concatenate([i.reshape(-1) for i in c["ious"]])
    assert all((flat == np.dtype(dtype_name).type(t)).sum() > 20 for t in THRESHOLDS)
    assert len(c["nan_dets"]) == 2
    for cls, d in c["nan_dets"]:                                          # selected first, a 1.0 in its row, and still unmatched
        assert det_labels[d] == cls and rank[d] == 0 and not matched[:, d].any()
    return rank, matched


@pytest.mark.parametrize("max_det", MAX_DETS)
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("layout", ["spread", "one_class"])
def test_match_ties_nans_thresholds_and_max_det(ops, layout, dtype_name, max_det):
    want_rank, want_matched = check_match_case_can_fail(layout, dtype_name, max_det)
    c = match_case(layout, dtype_name)
    iou = np.concatenate([i.reshape(-1) for i in c["ious"]])
    rank, matched = ops.map_match(dev(iou), ptr_of(len(d) for d in c["dl"]), ptr_of(len(g) for g in c["gl"]), dev(np.concatenate(c["dl"]), torch.int32),
                                  dev(np.concatenate(c["ds"])), dev(np.concatenate(c["gl"]), torch.int32), dev(np.array(ASKED), torch.int32),
                                  THRESHOLDS, max_det)
    assert rank.dtype == torch.int32 and matched.dtype == torch.uint8
    assert np.array_equal(rank.cpu().numpy(), want_rank)
    assert np.array_equal(matched.cpu().numpy(), want_matched)


def test_match_threshold_is_strict_and_rounded_like_the_iou(ops):
    """``best > thr`` with ``thr`` rounded to float32 for a float32 IoU and left as it is for a float64 IoU: threshold 0.3, one frame
    of one detection and one ground-truth box per value."""
    f32_03 = np.float32(0.3)
    assert float(f32_03) > 0.3                                            # float32(0.3) = 0.300000011920929 lies above the double 0.3
    cases = {np.float32: ([f32_03, np.nextafter(f32_03, np.float32(1))], [0, 1]),
             # the last value tells the two paths apart: against a threshold rounded to float32 it would be equal, so unmatched
             np.float64: ([0.3, np.nextafter(0.3, 1.0), float(f32_03)], [0, 1, 1])}
    for dtype, (values, want) in cases.items():
        iou = np.array(values, dtype=dtype)
        n = len(values)
        zeros = np.zeros(n, dtype=np.int64)
        rank, matched = ops.map_match(dev(iou), list(range(n + 1)), list(range(n + 1)), dev(zeros, torch.int32), dev(np.full(n, 0.5, dtype=np.float32)),
                                      dev(zeros, torch.int32), dev(np.array([0]), torch.int32), [0.3], 100)
        ref_rank, ref_matched = MO.match([iou[i].reshape(1, 1) for i in range(n)], [[0]] * n, [[0.5]] * n, [[0]] * n, [0], [0.3], 100)
        assert ref_matched.tolist() == [want] and ref_rank.tolist() == [0] * n
        assert matched.cpu().numpy().tolist() == [want], dtype.__name__
        assert rank.cpu().numpy().tolist() == [0] * n


# ---- curves -------------------------------------------------------------------------------------------------------------------------
CURVE_CLASSES = [1, 3, 6, 8]                      # 3 holds the segment under test, between two others; 8 has detections but no ground truth
CURVE_MAX_DETS = (1, 2, 1000)
CURVE_LEVELS = np.array([0.8, 0.6, 0.4, 0.2, 0.0, -0.0], dtype=np.float32)
NPIG = 256                                        # ground truth of class 3: recalls are c / 256, so some thresholds below are hit exactly
NPIG_DISTINCT = 1024                              # ... of the "distinct" case: recalls are exactly the 1024 thresholds k / 1024
REC7 = np.array([0.0, 0.0625, 0.125, 0.3, 0.5, 0.7, 1.0], dtype=np.float32)
REC_VARIANTS = {
    "one": np.array([0.5], dtype=np.float32),
    "repeated": np.array([0.0, 0.0, 0.25, 0.25, 0.25, 0.5, 1.0, 1.0], dtype=np.float32),
    "above_one": np.array([0.5, 1.0, 1.5, 2.0, np.inf], dtype=np.float32),        # above every reachable recall: precision and score 0
    "limit_1024": (np.arange(1, 1025) / 1024.0).astype(np.float32),
}


@functools.lru_cache(maxsize=None)
def curve_case(n: int, kind: str):
    """Class 3 has exactly ``n`` detections; classes 1 (77), 6 (31), 8 (20, no ground truth) and 9 (10, not asked for) surround it."""
    rng = np.random.default_rng(1000 + n + 7 * len(kind))
    dl = rng.permutation(np.concatenate([np.full(m, c) for c, m in ((1, 77), (3, n), (6, 31), (8, 20), (9, 10))])).astype(np.int64)
    npig = NPIG_DISTINCT if kind == "distinct" else NPIG
    gl = rng.permutation(np.concatenate([np.full(m, c) for c, m in ((1, 40), (3, npig), (6, 16), (5, 7))])).astype(np.int64)
    total = len(dl)
    ds = CURVE_LEVELS[rng.integers(0, len(CURVE_LEVELS), total)].copy()
    rank = rng.integers(-1, 4, total).astype(np.int32)                   # max_det 1, 2, 1000 select a fifth, two fifths, four fifths
    matched = (rng.uniform(size=(2, total)) < 0.4).astype(np.uint8)
    seg = dl == 3
    if kind == "none_selected":
        rank[seg] = -1
    elif kind == "none_matched":
        matched[:, seg] = 0
    elif kind == "all_matched":
        matched[:, seg] = 1
    elif kind == "rising":                                                # precision grows towards the END of the order: the envelope of
        matched[0] = ds <= 0.4                                            # every chunk is the maximum of the chunks right of it
        matched[1] = ds <= 0.2
    elif kind == "distinct":                                              # every detection selected, matched and alone with its score
        ds = (rng.permutation(total) / total).astype(np.float32)
        rank[:] = 0
        matched[:] = 1
    else:
        assert kind == "random"
    return {"dl": dl, "ds": ds, "rank": rank, "matched": matched, "gl": gl}


@functools.lru_cache(maxsize=None)
def curve_want(n: int, kind: str, rec_name: str):
    c = curve_case(n, kind)
    rec = REC7 if rec_name == "rec7" else REC_VARIANTS[rec_name]
    return MO.curves(c["dl"], c["ds"], c["rank"], c["matched"], c["gl"], CURVE_CLASSES, CURVE_MAX_DETS, rec)


def device_curves(ops, c, rec, classes=CURVE_CLASSES, max_dets=CURVE_MAX_DETS):
    return ops.map_curves(dev(c["dl"], torch.int32), dev(c["ds"]), dev(c["rank"]), dev(c["matched"]), dev(c["gl"], torch.int32),
                          dev(np.array(classes), torch.int32), max_dets, None if rec is None else torch.from_numpy(rec))


def assert_tables_equal(got, want):
    for name, g, w in zip(("precision", "scores", "recall"), got, want):
        g = g.cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype == np.float32, name
        assert same_bits(g, w), f"{name}: {int((g != w).sum())} of {w.size} entries differ"


CURVE_CASES = [(n, "random") for n in (255, 256, 257, 512, 513, 1100)] + \
              [(513, k) for k in ("none_selected", "none_matched", "all_matched", "rising")] + [(1100, "rising")]


@pytest.mark.parametrize("n,kind", CURVE_CASES, ids=[f"{k}_{n}" for n, k in CURVE_CASES])
def test_curves_at_the_chunk_edges(ops, n, kind):
    c = curve_case(n, kind)
    want = curve_want(n, kind, "rec7")
    precision, scores, recall = want
    # what the case holds, on the restatement alone
    assert int((c["dl"] == 3).sum()) == n and precision.shape == (2, 7, 4, 3)
    ki = CURVE_CLASSES.index(3)
    assert (precision[:, :, CURVE_CLASSES.index(8)] == -1).all() and (recall[:, CURVE_CLASSES.index(8)] == -1).all()
    assert (precision[:, :, [0, 1, 2]] >= 0).all()
    if kind == "none_selected":
        assert not precision[:, :, ki].any() and not recall[:, ki].any() and not scores[:, :, ki].any()
    elif kind == "none_matched":
        assert not precision[:, :, ki].any() and not recall[:, ki].any()
    elif kind == "all_matched":
        assert (precision[:, 0, ki] == 1).all() and (recall[:, ki] > 0).all()
    elif kind == "random":
        assert (precision[:, 0, ki] > 0).all() and (recall[:, ki, 2] > 0.25).all()
        assert len(np.unique(precision[:, :, ki, 2])) > 3 and len(np.unique(scores[:, :, ki, 2])) >= 2     # several thresholds served
    if kind == "rising":                                                  # the first detection's envelope is the LAST chunk's maximum
        sel = MO.order_desc(c["ds"])
        sel = sel[(c["dl"][sel] == 3) & (c["rank"][sel] >= 0)]
        tps = c["matched"][0, sel].astype(bool)
        pr = np.cumsum(tps) / np.arange(1, len(sel) + 1)
        assert not tps[0] and len(sel) > 256 and pr[-(len(sel) // 4):].max() > pr[:-(len(sel) // 4)].max()
    assert_tables_equal(device_curves(ops, c, REC7), want)


@pytest.mark.parametrize("rec_name", list(REC_VARIANTS))
def test_curves_recall_threshold_variants(ops, rec_name):
    n, kind = (1100, "distinct") if rec_name == "limit_1024" else (513, "random")
    want = curve_want(n, kind, rec_name)
    rec = REC_VARIANTS[rec_name]
    ki = CURVE_CLASSES.index(3)
    assert want[0].shape == (2, len(rec), 4, 3)
    if rec_name == "above_one":
        assert (want[0][:, 0, ki, 2] > 0).all() and not want[0][:, 2:, :3].any() and not want[1][:, 2:, :3].any()
    if rec_name == "repeated":
        assert np.array_equal(want[0][:, 2], want[0][:, 3]) and np.array_equal(want[1][:, 3], want[1][:, 4]) and want[0][:, 2, ki].any()
    if rec_name == "limit_1024":                                          # every detection serves its own threshold with its own score
        assert len(np.unique(want[1][0, :, ki, 2])) == 1024
    assert_tables_equal(device_curves(ops, curve_case(n, kind), rec), want)


def test_curves_refusals(ops):
    from radargnn_amd import _lib
    c = curve_case(255, "random")
    with pytest.raises(_lib.RgnnError, match="at most 1024 recall thresholds"):
        device_curves(ops, c, (np.arange(1025) / 1024.0).astype(np.float32))
    with pytest.raises(ValueError, match="rec_thresholds must be a non-empty ascending vector"):
        device_curves(ops, c, np.array([0.0, 0.5, 0.25], dtype=np.float32))
    with pytest.raises(ValueError, match="rec_thresholds must be a non-empty ascending vector"):
        device_curves(ops, c, np.zeros(0, dtype=np.float32))
    for classes in ([3, 1], [1, 3, 3]):
        with pytest.raises(ValueError, match="classes must be strictly ascending"):
            device_curves(ops, c, REC7, classes=classes)


def test_curves_default_thresholds_at_a_chunk_edge(ops):
    """The 101 default thresholds and the default ``max_dets`` on the 513 segment (tied scores, unlike the 6000-detection test)."""
    c = curve_case(513, "random")
    want = MO.curves(c["dl"], c["ds"], c["rank"], c["matched"], c["gl"], CURVE_CLASSES)
    assert_tables_equal(device_curves(ops, c, None, max_dets=(1, 10, 100)), want)


# ---- box IoU ------------------------------------------------------------------------------------------------------------------------
HAND_BOXES = np.array([
    [0, 0, 2, 2],              # 0  a plain box
    [0, 0, 2, 2],              # 1  identical to 0
    [2, 0, 4, 2],              # 2  touches 0 along an edge
    [2, 2, 3, 3],              # 3  touches 0 at a corner
    [0.5, 0.5, 1.5, 1.5],      # 4  nested in 0
    [1, 1, 1, 1],              # 5  a point inside 0: zero area
    [1, 0, 1, 2],              # 6  a line inside 0: zero width
    [9, 9, 9, 9],              # 7  a point away from everything
    [3, 3, 1, 1],              # 8  inverted in both axes
    [3, 0, 1, 2],              # 9  inverted in x only: negative area
    [-1e20, -1e20, 1e20, 1e20],  # 10 its area overflows float32
    [0, 0, np.inf, 1],         # 11 one infinite corner
    [-3, -3, -1, -1],          # 12 disjoint from 0
], dtype=np.float32)


def test_box_iou_degenerate_boxes(ops):
    want = MO.box_iou(HAND_BOXES, HAND_BOXES)
    n = len(HAND_BOXES)
    # the restatement says what the comments above say
    assert want[0, 1] == 1.0 and want[0, 0] == 1.0 and want[4, 4] == 1.0
    assert want[0, 2] == 0.0 and want[0, 3] == 0.0 and want[0, 12] == 0.0
    assert want[0, 4] == np.float32(0.25) and want[4, 0] == np.float32(0.25)
    assert np.isnan(want[5, 5]) and np.isnan(want[6, 6]) and np.isnan(want[7, 7]) and want[7, 0] == 0.0 and want[12, 6] == 0.0
    assert want[8, 8] == 0.0 and want[0, 8] == 0.0
    assert np.isnan(want[10, 10]) and np.isnan(want[11, 11]) and want[10, 0] == 0.0 and want[11, 0] == 0.0
    got, out = ops.box_iou(dev(HAND_BOXES), [0, n], dev(HAND_BOXES), [0, n])
    assert out == [0, n * n] and got.dtype == torch.float32
    assert same_bits(got.cpu().numpy().reshape(n, n), want)


BOX_FRAMES = [(0, 3), (5, 0), (0, 0), (70, 9), (1, 1), (300, 2)]              # empty frames first and in the middle


def test_box_iou_frames_with_empty_ones_between(ops):
    rng = np.random.default_rng(11)
    pp, gp = ptr_of(p for p, _ in BOX_FRAMES), ptr_of(g for _, g in BOX_FRAMES)
    pred, gt = MO.well_conditioned_boxes(rng, pp[-1]), MO.well_conditioned_boxes(rng, gp[-1])
    want = [MO.box_iou(pred[pp[f]:pp[f + 1]], gt[gp[f]:gp[f + 1]]) for f in range(len(BOX_FRAMES))]
    flat = np.concatenate([w.reshape(-1) for w in want])
    assert float((flat > 0).mean()) >= 0.2 and np.isfinite(flat).all()
    whole, out = ops.box_iou(dev(pred), pp, dev(gt), gp)
    assert out == ptr_of(p * g for p, g in BOX_FRAMES) and whole.shape == (out[-1],)
    assert same_bits(whole.cpu().numpy(), flat)
    parts = []
    for f in range(len(BOX_FRAMES)):
        part, part_out = ops.box_iou(dev(pred[pp[f]:pp[f + 1]]), [0, pp[f + 1] - pp[f]], dev(gt[gp[f]:gp[f + 1]]), [0, gp[f + 1] - gp[f]])
        assert part_out == [0, want[f].size] and part.shape == (want[f].size,)
        parts.append(part)
    assert torch.equal(whole, torch.cat(parts))


# ---- confusion matrix ---------------------------------------------------------------------------------------------------------------
def special_labels(k: int) -> np.ndarray:
    return np.array([-1.0, -0.5, -0.0, 0.0, np.nextafter(1.0, 0.0), 1.0, k - 1.0, np.nextafter(float(k), 0.0), float(k), k + 0.5, 2.0 ** 31,
                     -2.0 ** 31 - 1, 2.0 ** 40, 1e300, -1e300, np.inf, -np.inf, 5e-324, -5e-324], dtype=np.float64)


@pytest.mark.parametrize("k", [1, 6, 64])
def test_confusion_matrix_labels_at_the_edges(ops, k):
    """The reference is ``np.trunc`` in float64 followed by the range test 0 <= label < K.  For finite labels inside the int64 range
    that is ``astype(np.int64)`` (asserted here).  What ``astype(int)`` makes of +-inf and of values beyond int64 is undefined; the
    kernel's documented choice is to leave such nodes out, as it does every label outside 0 .. K-1."""
    rng = np.random.default_rng(k)
    special = special_labels(k)
    a, b = np.meshgrid(special, special, indexing="ij")                   # every special label on either side of the pair
    some = rng.integers(-2, k + 2, 5000) + rng.choice([0.0, 0.25, 0.999], 5000)
    y_true = np.concatenate((a.reshape(-1), some, rng.integers(0, k, 3000).astype(np.float64)))
    y_pred = np.concatenate((b.reshape(-1), rng.integers(-2, k + 2, 5000) + rng.choice([0.0, 0.5], 5000), some[:3000]))
    want = MO.confusion_matrix(y_true, y_pred, k)
    inside = lambda y: np.isfinite(y) & (np.abs(y) < 2.0 ** 62)
    both = inside(y_true) & inside(y_pred)
    ti, pi = y_true[both].astype(np.int64), y_pred[both].astype(np.int64)
    assert np.array_equal(ti, np.trunc(y_true[both])) and np.array_equal(pi, np.trunc(y_pred[both]))
    keep = (ti >= 0) & (ti < k) & (pi >= 0) & (pi < k)
    by_astype = np.zeros((k, k), dtype=np.int64)
    np.add.at(by_astype, (ti[keep], pi[keep]), 1)
    assert np.array_equal(by_astype, want)                                # nothing outside int64's range lands in the matrix
    # -0.5, -0.0, 0.999... and 5e-324 are class 0; K - 1 + 0.999... is class K - 1; K is out
    assert MO.confusion_matrix(np.array([-0.5, -0.0, np.nextafter(1.0, 0.0), -5e-324]), np.zeros(4), k)[0, 0] == 4
    assert MO.confusion_matrix(np.array([np.nextafter(float(k), 0.0), float(k)]), np.array([k - 1.0, k - 1.0]), k)[k - 1, k - 1] == 1
    assert want.sum() > 500 and (k > 6 or (want > 0).all())
    got = ops.confusion_matrix(dev(y_true), dev(y_pred), k)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    swapped = ops.confusion_matrix(dev(y_pred), dev(y_true), k)
    assert np.array_equal(swapped.cpu().numpy(), want.T)


def test_confusion_matrix_grid_stride_tail_is_already_covered():
    """The kernel launches at most 1024 work-groups of 256 lanes; a second trip of its grid-stride loop needs more than 262144 nodes.
    tests/test_gpu_metrics.py::test_confusion_matrix_and_f1[large] runs 300000, beyond the 1024 * 256 + 257 asked for, so no further
    case is added here; this holds the fixture to that size."""
    assert int(np.load(os.path.join(GOLDEN, "eval_seg_confusion.npz"))["large_n"]) >= 1024 * 256 + 257
