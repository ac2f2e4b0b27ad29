"""Segmented suppression (rgnn_nms_frames through ops.nms_frames, BoxSuppressor.apply_nms_frames, Postprocessor.detect_batch /
process / process_batch) against the single-frame device path (BoxSuppressor.apply_nms, ops.nms on each frame's slice) and the
oracle.  Every comparison is exact: the segmented kernels call the same device functions in the same operand order as the
single-frame kernels, so ids, counts, labels, scores and corners must agree bit for bit."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import postprocess_oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "postprocess_*.npz")))


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radargnn_amd import postprocessor
    assert hasattr(postprocessor, "Detections") and hasattr(postprocessor.BoxSuppressor, "apply_nms_frames")
    return postprocessor


# ---- inputs ----------------------------------------------------------------------------------------------------------
def rotated_corners(b):
    """[M, 5] [x, y, l, w, theta deg] -> corners [M, 4, 2] in the corner order of the decode kernel."""
    b = np.asarray(b, dtype=np.float64).reshape(-1, 5)
    t = np.deg2rad(b[:, 4])
    c, s, hl, hw = np.cos(t)[:, None], np.sin(t)[:, None], b[:, 2] / 2, b[:, 3] / 2
    ox, oy = np.stack((hl, hl, -hl, -hl), 1), np.stack((hw, -hw, -hw, hw), 1)
    return np.stack((c * ox - s * oy + b[:, 0:1], s * ox + c * oy + b[:, 1:2]), axis=2)


def aligned_corners(tp):
    """[M, 4] [x0, y0, x1, y1] -> corners [M, 4, 2]."""
    tp = np.asarray(tp, dtype=np.float64).reshape(-1, 4)
    x0, y0, x1, y1 = tp[:, 0], tp[:, 1], tp[:, 2], tp[:, 3]
    return np.stack((np.stack((x1, y1), 1), np.stack((x1, y0), 1), np.stack((x0, y0), 1), np.stack((x0, y1), 1)), axis=1)


def random_boxes(rng, m, extent, aligned, lo=None):
    lo = -extent if lo is None else lo
    if aligned:
        p = rng.uniform(lo, extent, (m, 2))
        return aligned_corners(np.concatenate((p, p + rng.uniform(0.5, 5, (m, 2))), axis=1))
    return rotated_corners(np.stack((rng.uniform(lo, extent, m), rng.uniform(lo, extent, m), rng.uniform(1, 6, m),
                                     rng.uniform(0.5, 3, m), rng.uniform(0, 180, m)), axis=1))


def tied_scores(rng, m):
    s = rng.uniform(0, 1, m)
    s[m // 2:] = np.round(s[m // 2:], 1)                       # ties: the order must be the stable descending sort
    return s.astype(np.float32)


class Batch:
    """Decode-shaped inputs of a batch: the candidates of every frame (corners, scores) scattered among ``extra`` nodes with
    keep == 0, in node order."""

    def __init__(self, rng, frames, extra):
        cs, ss, ks, ptr = [], [], [], [0]
        for (c, s), e in zip(frames, extra):
            m = len(s)
            n = m + e
            slots = np.sort(rng.choice(n, m, replace=False))
            cf, sf, kf = rng.uniform(-50, 50, (n, 4, 2)), rng.uniform(0, 1, n).astype(np.float32), np.zeros(n, dtype=np.int32)
            cf[slots], sf[slots], kf[slots] = c, s, 1
            cs.append(cf), ss.append(sf), ks.append(kf), ptr.append(ptr[-1] + n)
        n = ptr[-1]
        self.corners = torch.from_numpy(np.concatenate(cs).reshape(n, 4, 2) if cs else np.zeros((0, 4, 2))).cuda()
        self.score = torch.from_numpy(np.concatenate(ss) if ss else np.zeros(0, dtype=np.float32)).cuda()
        self.keep = torch.from_numpy(np.concatenate(ks) if ks else np.zeros(0, dtype=np.int32)).cuda()
        self.label = torch.from_numpy(rng.integers(0, 5, n).astype(np.int32)).cuda()
        self.bounds = ptr
        self.ptr = torch.tensor(ptr, dtype=torch.int64).cuda()

    def run(self, P, thr, aligned):
        return P.BoxSuppressor.apply_nms_frames(self.corners, self.score, self.label, self.keep, self.ptr, thr, aligned)


# ---- the single-frame device path ------------------------------------------------------------------------------------
def nms_matrix(corners, aligned):
    """The matrix BoxSuppressor.apply_nms hands to ops.nms (postprocessing.py:356-361, 389-394)."""
    from radargnn_amd import ops
    if aligned:
        mat, _ = ops.box_representations(corners, two_point=True, rotated=False)
        lo = float(mat.min())
        shift = abs(lo) + 100 if lo < 0 else 0.0
        return (mat + shift).to(torch.float32) if shift else mat.to(torch.float32)
    _, mat = ops.box_representations(corners, two_point=False, rotated=True)
    lo = float(mat[:, :2].min())
    if lo < 0:
        mat = mat.clone()
        mat[:, :2] += abs(lo) + 100
    return mat


def single_frame(P, batch, f, thr, aligned):
    """Frame f alone: apply_nms on the frame's candidates, and the node ids ops.nms keeps on the same matrix."""
    from radargnn_amd import ops
    lo, hi = batch.bounds[f], batch.bounds[f + 1]
    idx = torch.nonzero(batch.keep[lo:hi], as_tuple=False).view(-1)
    c = batch.corners[lo:hi].index_select(0, idx)
    s = batch.score[lo:hi].index_select(0, idx).to(torch.float64).view(-1, 1)
    lb = batch.label[lo:hi].index_select(0, idx).to(torch.float64).view(-1, 1)
    boxes, ks, kl = P.BoxSuppressor.apply_nms(P.BoundingBoxes(c, aligned), s, lb, thr)
    out = {"corners": boxes.corners, "scores": ks[:, 0], "labels": kl[:, 0], "cand": idx + lo, "mat": None, "s": None}
    if len(idx):
        out["mat"] = nms_matrix(c, aligned)
        out["s"] = s.view(-1).to(torch.float32) if aligned else s.view(-1)
        out["node"] = out["cand"].index_select(0, ops.nms(out["mat"], out["s"], thr, rotated=not aligned))
    else:
        out["node"] = idx
    return out


def same_bits(a, b):
    """torch.equal that also accepts NaN at the same places."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) \
        and torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))


def check_frames(P, det, batch, thr, aligned, oracle_upto=0, frames=None, equal=torch.equal):
    assert len(det) == len(batch.bounds) - 1 and det.ptr.dtype == torch.int64 and int(det.ptr[0]) == 0
    assert det.node.dtype == torch.int64 and det.labels.dtype == torch.float64
    assert det.corners.dtype == det.scores.dtype == (torch.float32 if aligned else torch.float64)
    assert det.corners.shape == (int(det.ptr[-1]), 4, 2) and det.scores.shape == det.labels.shape == det.node.shape == (int(det.ptr[-1]),)
    for f in (range(len(det)) if frames is None else frames):
        ref = single_frame(P, batch, f, thr, aligned)
        a, b = int(det.ptr[f]), int(det.ptr[f + 1])
        assert b - a == ref["node"].numel(), f
        got = det.frame(f)
        if a == b:                                            # no candidates: the empty float64 tensors of apply_nms
            assert ref["cand"].numel() == 0
            assert got["boxes"].corners.shape == (0, 4, 2) and got["boxes"].corners.dtype == torch.float64
            assert got["scores"].shape == (0,) and got["scores"].dtype == torch.float64 and got["labels"].dtype == torch.float64
            continue
        assert torch.equal(det.node[a:b], ref["node"]), f
        assert det.corners[a:b].dtype == ref["corners"].dtype and equal(det.corners[a:b], ref["corners"]), f
        assert det.scores[a:b].dtype == ref["scores"].dtype and equal(det.scores[a:b], ref["scores"]), f
        assert torch.equal(det.labels[a:b], ref["labels"]), f
        assert equal(got["boxes"].corners, ref["corners"]) and equal(got["scores"], ref["scores"]) and got["boxes"].is_aligned == aligned
        if ref["cand"].numel() <= oracle_upto:
            nms = O.nms_aligned if aligned else O.nms_rotated
            keep = nms(ref["mat"].cpu().numpy(), ref["s"].cpu().numpy(), thr)
            assert det.node[a:b].tolist() == ref["cand"].cpu().numpy()[keep].tolist(), f


# ---- 1: edge sizes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [False, True], ids=["rotated", "aligned"])
def test_edge_sizes_match_single_frame_path_and_oracle(P, aligned):
    rng = np.random.default_rng(11 + aligned)
    counts = [0, 1, 2, 63, 0, 64, 65, 129, 300, 0]
    extra = [3, 0, 4, 20, 0, 1, 7, 40, 100, 0]                 # nodes with keep == 0 in between; two frames without any node
    frames = [(random_boxes(rng, m, 4 + m / 20, aligned), tied_scores(rng, m)) for m in counts]
    batch = Batch(rng, frames, extra)
    thr = 0.3
    det = batch.run(P, thr, aligned)
    check_frames(P, det, batch, thr, aligned, oracle_upto=150)
    kept = (det.ptr[1:] - det.ptr[:-1]).tolist()
    assert [k > 0 for k in kept] == [m > 0 for m in counts] and kept[8] < 300      # something was suppressed


# ---- 2: degenerate batches -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [False, True], ids=["rotated", "aligned"])
def test_degenerate_batches(P, aligned):
    rng = np.random.default_rng(2)
    one = Batch(rng, [(random_boxes(rng, 30, 4, aligned), tied_scores(rng, 30))], [5])
    check_frames(P, one.run(P, 0.3, aligned), one, 0.3, aligned, oracle_upto=150)
    empty = Batch(rng, [(np.zeros((0, 4, 2)), np.zeros(0, dtype=np.float32))] * 3, [4, 0, 2])
    det = empty.run(P, 0.3, aligned)
    assert det.ptr.tolist() == [0, 0, 0, 0]
    check_frames(P, det, empty, 0.3, aligned)
    none = Batch(rng, [], [])
    det = none.run(P, 0.3, aligned)
    assert len(det) == 0 and det.ptr.tolist() == [0] and det.corners.shape == (0, 4, 2) and det.node.shape == (0,)
    assert det.node.dtype == torch.int64 and det.labels.dtype == torch.float64
    no_nodes = Batch(rng, [(np.zeros((0, 4, 2)), np.zeros(0, dtype=np.float32))] * 2, [0, 0])      # N = 0, B = 2
    assert no_nodes.run(P, 0.3, aligned).ptr.tolist() == [0, 0, 0]


# ---- 3: frames do not see each other ---------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [False, True], ids=["rotated", "aligned"])
def test_frames_do_not_see_each_other(P, aligned):
    rng = np.random.default_rng(3)
    boxes, scores = random_boxes(rng, 40, 5, aligned), (tied_scores(rng, 40) * 0.5).astype(np.float32)
    on_top = (boxes.copy(), (scores + np.float32(0.5)).astype(np.float32))                   # same places, higher scores
    batch = Batch(np.random.default_rng(0), [(boxes, scores), on_top, (boxes, scores)], [0, 0, 0])
    batch.label[80:] = batch.label[:40]
    det = batch.run(P, 0.3, aligned)
    check_frames(P, det, batch, 0.3, aligned, oracle_upto=150)
    f0, f2 = det.frame(0), det.frame(2)
    assert 0 < len(f0["boxes"]) < 40
    assert torch.equal(f0["boxes"].corners, f2["boxes"].corners) and torch.equal(f0["scores"], f2["scores"])
    assert torch.equal(f0["labels"], f2["labels"])
    assert torch.equal(det.node[int(det.ptr[0]):int(det.ptr[1])] + 80, det.node[int(det.ptr[2]):int(det.ptr[3])])
    alone = P.BoxSuppressor.apply_nms_frames(batch.corners[:40], batch.score[:40], batch.label[:40], batch.keep[:40],
                                             batch.ptr[:2], 0.3, aligned)
    assert torch.equal(alone.corners, f0["boxes"].corners) and torch.equal(alone.scores, f0["scores"])
    assert torch.equal(alone.labels, f0["labels"]) and torch.equal(alone.node, det.node[:int(det.ptr[1])])


# ---- 4: the shift is the frame's own ---------------------------------------------------------------------------------
def test_shift_is_per_frame_aligned(P):
    rng = np.random.default_rng(4)
    neg = random_boxes(rng, 50, 20, True)                                        # frame 0: negative coordinates
    pos = random_boxes(rng, 50, 20, True, lo=0.001)                              # frame 1: all positive, float64 noise below float32
    assert neg.min() < 0 < pos.min()
    batch = Batch(rng, [(neg, tied_scores(rng, 50)), (pos, tied_scores(rng, 50))], [3, 3])
    det = batch.run(P, 0.3, True)
    check_frames(P, det, batch, 0.3, True, oracle_upto=150)
    a, b = int(det.ptr[1]), int(det.ptr[2])
    tp = torch.from_numpy(O.two_point(batch.corners[det.node[a:b]].cpu().numpy())).to(torch.float32).cuda()      # no shift at all
    x0, y0, x1, y1 = tp[:, 0], tp[:, 1], tp[:, 2], tp[:, 3]
    unshifted = torch.stack((x0, y0, x0, y1, x1, y0, x1, y1), dim=1).view(-1, 4, 2)
    assert torch.equal(det.corners[a:b], unshifted)
    shifted = (tp.double() + (abs(float(neg.min())) + 100)).float() - torch.tensor(abs(float(neg.min())) + 100).float().cuda()
    assert not torch.equal(shifted, tp)                                          # a batch-wide shift would have changed the bits


def iou_of_pair_on_device(ops, mat):
    """The float64 IoU rgnn_nms computes for rows 0 (higher score) and 1 of ``mat``: the largest threshold at which
    row 1 is still suppressed (the test is >=), found by bisection over the float64 numbers."""
    scores = torch.tensor([0.9, 0.1], dtype=torch.float64).cuda()
    lo, hi = 0.0, 1.0
    while True:
        mid = (lo + hi) / 2
        if mid == lo or mid == hi:
            return lo
        if ops.nms(mat, scores, mid, rotated=True).numel() == 1:
            lo = mid
        else:
            hi = mid


def test_shift_is_per_frame_rotated(P):
    """Rotated boxes: frame 0 has negative centres, frame 1 is a pair of overlapping boxes with positive centres.  The
    threshold is the pair's own IoU as the single-frame path computes it WITHOUT a shift, so the >= decision sits on the last
    bit: centres moved by another frame's minimum round differently."""
    from radargnn_amd import ops
    rng = np.random.default_rng(5)
    neg = random_boxes(rng, 30, 20, False)
    for case in range(4):
        pair = np.array([[10.1 + case * 3.3, 7.7, 4.2, 2.1, 31.0 + 17 * case], [10.9 + case * 3.3, 8.3, 3.7, 1.9, 52.0 + 11 * case]])
        corners = rotated_corners(pair)
        batch = Batch(rng, [(neg, tied_scores(rng, 30)), (corners, np.array([0.9, 0.1], dtype=np.float32))], [2, 0])
        thr = iou_of_pair_on_device(ops, nms_matrix(batch.corners[batch.bounds[1]:], False))
        assert 0.05 < thr < 0.95
        for t, kept in ((thr, 1), (float(np.nextafter(thr, 1.0)), 2)):
            det = batch.run(P, t, False)
            assert int(det.ptr[2] - det.ptr[1]) == kept
            check_frames(P, det, batch, t, False)


# ---- 5: threshold semantics ------------------------------------------------------------------------------------------
def test_threshold_semantics(P):
    rng = np.random.default_rng(6)
    sc = np.array([0.8, 0.6], dtype=np.float32)
    al = Batch(rng, [(aligned_corners([[0, 0, 2, 1], [1, 0, 3, 1]]), sc)], [0])
    det = al.run(P, 1 / 3, True)                                                 # IoU == 1/3 and the test is >
    assert det.node.tolist() == [0, 1]
    check_frames(P, det, al, 1 / 3, True, oracle_upto=150)
    assert al.run(P, 0.33, True).node.tolist() == [0]
    ro = Batch(rng, [(rotated_corners([[1, .5, 2, 1, 0], [2, .5, 2, 1, 0]]), sc)], [0])
    check_frames(P, ro.run(P, 1 / 3, False), ro, 1 / 3, False)                   # whatever ops.nms decides for the pair


@pytest.mark.parametrize("side,expected", [(-0.01, [1]), (+0.01, [1, 0])])
def test_reference_known_answer_as_frame_2_of_3(P, side, expected):
    """test/test_postprocessor.py:8-35 of the reference (tests/test_gpu_postprocess.py:121-128), between other frames."""
    rng = np.random.default_rng(7)
    known = (rotated_corners([[1, 2, 1, 1, 90], [1, 2.9, 1, 1, 90]]), np.array([0.2, 0.7], dtype=np.float32))
    other = [(random_boxes(rng, 20, 5, False), tied_scores(rng, 20)) for _ in range(2)]
    batch = Batch(rng, [other[0], other[1], known], [2, 2, 0])
    thr = 0.1 / (2 - 0.1) + side
    det = batch.run(P, thr, False)
    assert (det.node[int(det.ptr[2]):] - batch.bounds[2]).tolist() == expected
    check_frames(P, det, batch, thr, False, oracle_upto=150)


# ---- 6: non-finite input ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [False, True], ids=["rotated", "aligned"])
def test_non_finite_input(P, aligned):
    rng = np.random.default_rng(8)
    frames = [(random_boxes(rng, 70, 5, aligned), tied_scores(rng, 70)) for _ in range(3)]
    frames[1][1][5] = np.nan                                   # a NaN score sorts first
    frames[1][0][9] = np.nan                                   # a box of NaN (rotated: the reference's default box)
    frames[1][0][12, 3] = np.nan                               # one NaN corner: NaN centre, the frame's minimum is NaN -> no shift
    batch = Batch(rng, frames, [0, 0, 0])
    det = batch.run(P, 0.3, aligned)
    check_frames(P, det, batch, 0.3, aligned, equal=same_bits)
    assert torch.isnan(det.scores[int(det.ptr[1])]) and int(det.node[int(det.ptr[1])]) == batch.bounds[1] + 5


# ---- 7: a frame beyond the kernel's capacity --------------------------------------------------------------------------
def test_oversize_frame_goes_through_the_single_frame_path(P):
    from radargnn_amd import ops
    rng = np.random.default_rng(9)
    m = ops.nms_frames_max_candidates() + 1
    assert m == 4097
    frames = [(random_boxes(rng, 30, 5, True), tied_scores(rng, 30)), (random_boxes(rng, m, 60, True), tied_scores(rng, m)),
              (random_boxes(rng, 45, 5, True), tied_scores(rng, 45))]
    batch = Batch(rng, frames, [3, 10, 3])
    raw = ops.nms_frames(batch.label, batch.score, batch.keep, batch.corners, batch.ptr, 0.3, rotated=False)
    assert raw[5].tolist() == [30, m, 45] and int(raw[4][2] - raw[4][1]) == 0      # left empty by the kernels, and reported
    det = batch.run(P, 0.3, True)
    check_frames(P, det, batch, 0.3, True)
    assert 45 < int(det.ptr[2] - det.ptr[1]) < m
    exact = Batch(rng, [(random_boxes(rng, m - 1, 60, True), tied_scores(rng, m - 1))] + frames[:1], [1, 0])    # 4096: in the kernel
    assert ops.nms_frames(exact.label, exact.score, exact.keep, exact.corners, exact.ptr, 0.3, rotated=False)[4][1] > 0
    check_frames(P, exact.run(P, 0.3, True), exact, 0.3, True)


@pytest.mark.parametrize("thr", [0.3, 1e-12, 0.0])
def test_rotated_frames_from_dense_to_sparse(P, thr):
    """Rotated pairs too far apart to touch are decided without their IoU when the threshold allows it: the decisions stay
    those of the single-frame path where nearly all pairs overlap, where nearly none do, and at thresholds at which a zero
    IoU still suppresses (0) or is the only thing that does not (1e-12)."""
    rng = np.random.default_rng(10)
    batch = Batch(rng, [(random_boxes(rng, 400, e, False), tied_scores(rng, 400)) for e in (5, 40, 400)], [5, 5, 5])
    det = batch.run(P, thr, False)
    check_frames(P, det, batch, thr, False)
    kept = (det.ptr[1:] - det.ptr[:-1]).tolist()
    assert kept == [1, 1, 1] if thr == 0.0 else kept[0] < kept[1] < kept[2] <= 400


# ---- 8: reference vectors through process_batch ----------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[12:-4] for p in GOLDEN])
def test_reference_vectors_through_process_batch(P, path):
    """Frame 0 of [fixture, a frame without candidates, fixture moved by 300] against the oracle flow of
    tests/test_gpu_postprocess.py::test_box_suppressor_flow, with its tolerances.  (The middle frame holds two background
    nodes: the en representation needs a neighbour in every frame.)"""
    g = np.load(path)
    cfg = P.PostProcessingConfiguration(split="test", iou_for_nms=0.2, min_object_score={f"c{i}": float(v) for i, v in enumerate(g["min_scores"])},
                                        max_score_for_background=float(g["max_bg"]), bg_index=int(g["bg_index"]),
                                        bb_invariance=str(g["invariance"]), adapt_orientation_angle=bool(g["adapt"]))
    n, k = g["prob"].shape
    bg = np.zeros((2, k), dtype=np.float32)
    bg[:, cfg.bg_index] = 1.0
    prob = np.concatenate((g["prob"], bg, g["prob"]))
    bb = np.concatenate((g["bb"], np.ones((2, g["bb"].shape[1]), dtype=np.float32), g["bb"]))
    pos = np.concatenate((g["pos"], np.array([[1.0, 2.0], [3.0, 5.0]], dtype=g["pos"].dtype), g["pos"] + 300))
    results = P.Postprocessor.process_batch(cfg, pos, bb, prob, [0, n, n + 2, 2 * n + 2])
    assert len(results) == 3 and len(results[1][0]["boxes"]) == 0 and results[1][0]["scores"].dtype == torch.float64
    assert len(results[2][0]["boxes"]) > 0 and results[2][1]["pos"].shape == (n, 2)
    det = results[0][0]
    corners, sc, lb = g["corners"], g["scores"][g["kept"]], g["labels"][g["kept"]]
    if g["bb"].shape[1] == 5:
        mat = O.rotated_representation(corners)
        if mat[:, :2].min() < 0:
            mat[:, :2] += abs(mat[:, :2].min()) + 100
        keep = O.nms_rotated(mat, sc[:, 0], 0.2)
        np.testing.assert_allclose(det["boxes"].corners.cpu().numpy(), corners[keep], rtol=0, atol=1e-9)
        assert np.array_equal(det["scores"].cpu().numpy(), sc[keep][:, 0])
    else:
        mat = O.two_point(corners)
        shift = abs(mat.min()) + 100 if mat.min() < 0 else 0
        m32 = (mat + shift).astype(np.float32)
        keep = O.nms_aligned(m32, sc[:, 0].astype(np.float32), 0.2)
        back = m32[keep] - np.float32(shift)
        exp = np.stack((back[:, [0, 1]], back[:, [0, 3]], back[:, [2, 1]], back[:, [2, 3]]), axis=1)
        np.testing.assert_allclose(det["boxes"].corners.cpu().numpy(), exp, rtol=0, atol=1e-4)
        assert np.array_equal(det["scores"].cpu().numpy(), sc[keep][:, 0].astype(np.float32))
    assert np.array_equal(det["labels"].cpu().numpy(), lb[keep][:, 0]) and 0 < len(keep) <= len(corners)
    d, seg = P.Postprocessor.detect_batch(cfg, pos, bb, prob, [0, n, n + 2, 2 * n + 2])
    assert len(d) == 3 and torch.equal(d.frame(0)["boxes"].corners, det["boxes"].corners) and seg["labels"].shape == (2 * n + 2,)
    assert torch.equal(seg["clutter_scores"][:n], results[0][1]["clutter_scores"])


# ---- 9: routing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,inv", [(4, "translation"), (5, "translation"), (4, "en"), (5, "en")])
def test_process_and_process_batch_equal_the_single_frame_path(P, width, inv):
    rng = np.random.default_rng(width * 3 + len(inv))
    sizes = [int(s) for s in rng.integers(20, 201, 5)]
    pos, prob, bb, cls_gt, bb_gt = [], [], [], [], []
    for n in sizes:
        logits = rng.normal(size=(n, 6)) * 2
        prob.append((np.exp(logits) / np.exp(logits).sum(1, keepdims=True)).astype(np.float32))
        pos.append(rng.uniform(-10, 30, (n, 2)).astype(np.float32))
        b = rng.normal(size=(n, width)).astype(np.float32)
        b[:, 2:4] = np.abs(b[:, 2:4]) + 0.5
        if width == 5:
            b[:, 4] = rng.uniform(0, np.pi, n)
        bb.append(b)
        cls_gt.append(rng.integers(0, 6, n).astype(np.float32))
        bb_gt.append(b + np.float32(0.25))
    cfg = P.PostProcessingConfiguration(split="t", iou_for_nms=0.3, min_object_score={c: 0.2 for c in "abcde"},
                                        max_score_for_background=0.5, bg_index=5, bb_invariance=inv)
    single = [P.Postprocessor.process_one_raw_prediction(cfg, pos[f], bb[f], prob[f]) for f in range(5)]
    assert sum(len(d["boxes"]) for d, _ in single) > 5
    bounds = np.concatenate(([0], np.cumsum(sizes)))
    batch = P.Postprocessor.process_batch(cfg, torch.from_numpy(np.concatenate(pos)).cuda(), torch.from_numpy(np.concatenate(bb)).cuda(),
                                          torch.from_numpy(np.concatenate(prob)).cuda(), torch.from_numpy(bounds).cuda())
    bb_out, _, cls_out, _ = P.Postprocessor().process(cfg, pos, None, {"bounding_box_predictions": bb, "class_probability_prediction": prob},
                                                      {"bounding_box_true": bb_gt, "class_true": cls_gt})
    for f, (det, seg) in enumerate(single):
        for got_det, got_seg in (batch[f], (bb_out[f], cls_out[f])):
            assert got_det["boxes"].corners.dtype == det["boxes"].corners.dtype and got_det["boxes"].is_aligned == (width == 4)
            assert torch.equal(got_det["boxes"].corners, det["boxes"].corners)
            assert got_det["scores"].dtype == det["scores"].dtype and torch.equal(got_det["scores"], det["scores"])
            assert got_det["labels"].dtype == det["labels"].dtype and torch.equal(got_det["labels"], det["labels"])
            assert sorted(got_seg) == sorted(seg)
            for key in seg:
                assert got_seg[key].dtype == seg[key].dtype and torch.equal(got_seg[key], seg[key]), key
