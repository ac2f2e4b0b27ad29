"""Segmentation + DBSCAN as a detector (radargnn_amd.clustering.cluster_objects, rgnn_cluster_scores): a scene of planted objects
comes back as those objects, with the boxes of the ground-truth chain run on the planted ids, class scores that are float64 means,
and detections the metrics module takes.

Bars.  Instances and corners: exact (the same kernels on the same point sets).  Round trip corners -> box_representations -> rect:
1e-9 absolute (metres / degrees; the orientation modulo 180: theta and theta + 180 are one rectangle).  Class means: 1e-12 against
a float64 numpy mean -- at most 1 024 addends in [0, 1], so a different summation order moves the sum by at most
(n - 1) 2^-53 sum(x) ~ 1.1e-13 relative."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BG, K = 5, 6
EPS, MIN_SAMPLES = 1.0, 4


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radargnn_amd import clustering
    return clustering


def blob(rng, centre, size, angle, spacing=0.4):
    """A jittered grid inside a rotated rectangle: every point has neighbours well inside EPS, so the blob is one cluster of core points."""
    gx, gy = np.meshgrid(np.arange(0, size[0], spacing), np.arange(0, size[1], spacing))
    p = np.stack((gx.ravel(), gy.ravel()), axis=1) + rng.uniform(-0.1, 0.1, size=(gx.size, 2)) - np.asarray(size) / 2
    c, s = np.cos(angle), np.sin(angle)
    return p @ np.array([[c, s], [-s, c]]) + centre


def build_scene():
    """Three frames.  Frames 0 and 1: two separated blobs each; frame 2: two blobs of classes 1 and 2 that TOUCH (gap 0.3 < EPS:
    separate objects per class, one cluster without classes).  Every frame: background clutter (also on top of the blobs) and three
    isolated foreground points (noise).  Rows shuffled.  -> pos f64 [N, 2], frame_ptr, class [N], planted object id [N] (numbered by
    ascending smallest row, -1 none)."""
    rng = np.random.default_rng(42)
    plans = [[((10.0, 5.0), (4.0, 2.0), 0.3, 0), ((40.0, -12.0), (3.0, 1.6), 1.2, 3)],
             [((-20.0, 8.0), (5.0, 1.6), 2.0, 1), ((15.0, 30.0), (3.0, 1.6), 0.7, 4)],
             [((0.0, 0.0), (3.0, 2.0), 0.0, 1), ((3.3, 0.0), (3.0, 2.0), 0.0, 2)]]
    pos, cls, oid, ptr = [], [], [], [0]
    for plan in plans:
        p, c, o = [], [], []
        for k, (centre, size, angle, klass) in enumerate(plan):
            b = blob(rng, centre, size, angle)
            if klass == 2:
                b[:, 0] += 0.3 - (b[:, 0].min() - p[-1][:, 0].max())          # exactly 0.3 between the two touching blobs
            p.append(b); c.append(np.full(len(b), klass)); o.append(np.full(len(b), k))
        clutter = np.concatenate((rng.uniform(-50, 50, size=(60, 2)), p[0][:5] + 0.05))
        p.append(clutter); c.append(np.full(len(clutter), BG)); o.append(np.full(len(clutter), -1))
        lone = np.array([[80.0, 80.0], [-80.0, 80.0], [80.0, -80.0]])
        p.append(lone); c.append(np.array([0, 1, 2])); o.append(np.full(3, -1))
        p, c, o = np.concatenate(p), np.concatenate(c), np.concatenate(o)
        perm = rng.permutation(len(p))
        p, c, o = p[perm], c[perm], o[perm]
        firsts = sorted((np.nonzero(o == k)[0].min(), k) for k in range(len(plan)))
        renumber = {k: new for new, (_, k) in enumerate(firsts)}
        o = np.array([renumber.get(int(v), -1) for v in o])
        pos.append(p); cls.append(c); oid.append(o); ptr.append(ptr[-1] + len(p))
    return np.concatenate(pos), np.asarray(ptr, np.int64), np.concatenate(cls).astype(np.int64), np.concatenate(oid).astype(np.int64)


@pytest.fixture(scope="module")
def scene():
    pos, ptr, cls, oid = build_scene()
    rng = np.random.default_rng(43)
    prob = rng.dirichlet(np.ones(K), size=len(pos)).astype(np.float32)
    return {"pos": pos, "ptr": ptr, "cls": cls, "oid": oid, "prob": prob}


@pytest.fixture(scope="module")
def inst(C, scene):
    return C.cluster_objects(scene["pos"], torch.from_numpy(scene["ptr"]), scene["cls"], BG, EPS, MIN_SAMPLES, prob=scene["prob"])


def ground_truth_chain(scene, aligned=False):
    """The ground-truth kernels on the planted ids: targets -> float32 -> decoder; -> (corners of every object [M, 4, 2], first rows)."""
    from radargnn_amd import ops
    pos = torch.from_numpy(scene["pos"]).cuda()
    fp = torch.from_numpy(scene["ptr"]).cuda()
    obj_ptr, obj_rows = ops.group_objects(torch.from_numpy(scene["oid"]).cuda(), fp)
    targets, _, status = ops.create_gt_boxes(pos, obj_ptr, obj_rows, None, aligned, 0)
    assert int(status.item()) == 0
    labels = torch.from_numpy(np.where(scene["oid"] >= 0, 1.0, float(BG)).astype(np.float32)).cuda()
    _, corners = ops.decode_ground_truth(labels, targets.float(), pos.float(), None, BG, 0)
    first = obj_rows[obj_ptr[:-1]].long()
    return corners[first].cpu().numpy(), first.cpu().numpy()


def test_instances_are_the_planted_objects(inst, scene):
    ptr, oid = scene["ptr"], scene["oid"]
    assert len(inst) == 6 and inst.cluster_ptr.tolist() == [0, 2, 4, 6] and inst.valid.all()
    want = np.where(oid >= 0, oid + 2 * (np.searchsorted(ptr, np.arange(len(oid)), side="right") - 1), -1)
    assert np.array_equal(inst.instance.cpu().numpy(), want)
    assert (want[scene["cls"] == BG] == -1).all() and (want == -1).sum() > 3 * 65          # clutter and the lone points belong to nobody
    first = np.array([np.nonzero(want == m)[0].min() for m in range(6)])
    assert np.array_equal(inst.first.cpu().numpy(), first)
    assert np.array_equal(inst.cls.cpu().numpy(), scene["cls"][first])                         # per_class: the members' class


@pytest.mark.parametrize("aligned", [False, True], ids=["rotated", "aligned"])
def test_corners_are_the_ground_truth_chains(C, scene, aligned):
    from radargnn_amd import ops
    got = C.cluster_objects(scene["pos"], torch.from_numpy(scene["ptr"]), scene["cls"], BG, EPS, MIN_SAMPLES, aligned=aligned)
    corners, first = ground_truth_chain(scene, aligned)
    assert got.corners.dtype == torch.float64 and np.array_equal(got.corners.cpu().numpy(), corners)
    assert np.array_equal(got.first.cpu().numpy(), first) and (got.score == 1.0).all() and got.mean_prob is None
    # round trip: the corners give back `rect`
    two_point, rotated = ops.box_representations(got.corners)
    rect = got.rect.cpu().numpy()
    if aligned:
        tp = two_point.cpu().numpy()
        back = np.stack(((tp[:, 0] + tp[:, 2]) / 2, (tp[:, 1] + tp[:, 3]) / 2, tp[:, 2] - tp[:, 0], tp[:, 3] - tp[:, 1]), axis=1)
        err = np.abs(back - rect[:, :4]).max()
        assert (rect[:, 4] == 0).all()
    else:
        rot = rotated.cpu().numpy()
        d_theta = np.abs((rot[:, 4] - rect[:, 4] + 90) % 180 - 90)
        err = max(np.abs(rot[:, :4] - rect[:, :4]).max(), d_theta.max())
        assert (rect[:, 2] > rect[:, 3] + 0.2).all()                       # no squares: the orientation is defined
    print(f"[cluster_objects] round trip {'aligned' if aligned else 'rotated'}: {err:.2e} (bar 1e-9)")
    assert err <= 1e-9
    # and the boxes are the blobs': every member lies inside its rectangle's corners' bounding box
    tp = two_point.cpu().numpy()
    inst_of = got.instance.cpu().numpy()
    for m in range(len(got)):
        p = scene["pos"][inst_of == m].astype(np.float32)
        assert (p[:, 0] >= tp[m, 0] - 1e-4).all() and (p[:, 0] <= tp[m, 2] + 1e-4).all()
        assert (p[:, 1] >= tp[m, 1] - 1e-4).all() and (p[:, 1] <= tp[m, 3] + 1e-4).all()


def test_class_means_are_float64_means(inst, scene):
    inst_of = inst.instance.cpu().numpy()
    want = np.stack([scene["prob"][inst_of == m].astype(np.float64).mean(axis=0) for m in range(6)])
    assert max((inst_of == m).sum() for m in range(6)) <= 1024
    err = np.abs(inst.mean_prob.cpu().numpy() - want).max()
    print(f"[cluster_objects] class means: {err:.2e} (bar 1e-12)")
    assert err <= 1e-12
    cls = inst.cls.cpu().numpy()
    assert np.array_equal(inst.score.cpu().numpy(), inst.mean_prob.cpu().numpy()[np.arange(6), cls])


def test_without_classes_touching_blobs_merge_and_ties_go_to_the_lowest_class(C, scene):
    """per_class = False: one foreground group.  The touching blobs of frame 2 are one cluster; the class is the argmax of the mean
    probabilities over k != BG, the lowest k on a tie -- and the background column never wins, however large."""
    prob = scene["prob"].copy()
    oid, ptr = scene["oid"], scene["ptr"]
    frame = np.searchsorted(ptr, np.arange(len(oid)), side="right") - 1
    prob[(frame == 0) & (oid == 0)] = np.float32([0.3, 0.3, 0.05, 0.05, 0.1, 0.2])            # columns 0 and 1 tie exactly -> 0
    prob[(frame == 0) & (oid == 1)] = np.float32([0.05, 0.1, 0.25, 0.25, 0.05, 0.3])          # 2 and 3 tie, BG larger -> 2
    prob[(frame == 1) & (oid == 0)] = np.float32([0.0, 0.0, 0.0, 0.0, 0.0, 1.0])              # all zero but BG -> 0
    got = C.cluster_objects(scene["pos"], torch.from_numpy(ptr), scene["cls"], BG, EPS, MIN_SAMPLES, prob=prob, per_class=False)
    assert len(got) == 5 and got.cluster_ptr.tolist() == [0, 2, 4, 5] and got.valid.all()
    inst_of = got.instance.cpu().numpy()
    assert set(scene["cls"][inst_of == 4]) == {1, 2}
    cls, score, mean = got.cls.cpu().numpy(), got.score.cpu().numpy(), got.mean_prob.cpu().numpy()
    assert cls[:3].tolist() == [0, 2, 0]
    assert mean[0, 0] == mean[0, 1] and mean[1, 2] == mean[1, 3] and mean[1, BG] > mean[1, 2] and score[2] == 0.0
    want = np.stack([prob[inst_of == m].astype(np.float64).mean(axis=0) for m in range(5)])
    assert np.abs(mean - want).max() <= 1e-12
    best = np.argmax(want[:, :BG], axis=1)
    assert np.array_equal(cls[3:], best[3:]) and np.array_equal(score, mean[np.arange(5), cls])
    # without probabilities: the members' votes, score 1
    votes = C.cluster_objects(scene["pos"], torch.from_numpy(ptr), scene["cls"], BG, EPS, MIN_SAMPLES, per_class=False)
    v = votes.cls.cpu().numpy()
    n1, n2 = (scene["cls"][inst_of == 4] == 1).sum(), (scene["cls"][inst_of == 4] == 2).sum()
    assert np.array_equal(v[:4], scene["cls"][votes.first.cpu().numpy()[:4]])
    assert v[4] == (1 if n1 >= n2 else 2) and (votes.score == 1.0).all()


def test_refused_clusters_are_invalid_not_errors(C):
    """min_samples = 1: a lone point is a cluster (a 0.5 x 0.5 box); three points on a line and two coincident points are clusters the
    box kernel refuses: valid = False, NaN boxes, no exception, and they are left out of the detections."""
    from radargnn_amd import ops
    pos = np.array([[0.0, 0.0], [10.0, 0.0], [10.5, 0.0], [11.0, 0.0], [20.0, 5.0], [20.0, 5.0], [30.0, 0.0], [30.5, 0.0], [30.0, 0.5]])
    cls = np.zeros(len(pos), np.int64)
    got = C.cluster_objects(pos, torch.tensor([0, len(pos)]), cls, BG, 0.6, 1)
    assert got.instance.tolist() == [0, 1, 1, 1, 2, 2, 3, 3, 3]
    assert got.valid.tolist() == [True, False, False, True]
    assert int(got.box_status.item()) == ops.STATUS_GT_DEGENERATE_OBJECT
    rect, corners = got.rect.cpu().numpy(), got.corners.cpu().numpy()
    assert np.isnan(rect[1:3]).all() and np.isnan(corners[1:3]).all() and not np.isnan(rect[[0, 3]]).any()
    assert rect[0].tolist()[:4] == [0.0, 0.0, 0.5, 0.5]
    det = got.detections()
    assert len(det) == 1 and det.ptr.tolist() == [0, 2] and det.node.tolist() == [0, 6]


def test_detections_feed_the_metrics(inst, scene):
    from radargnn_amd.metrics import ObjectDetectionMetrics
    from radargnn_amd.postprocessor import BoundingBoxes, Detections, PostProcessingConfiguration
    det = inst.detections()
    assert isinstance(det, Detections) and len(det) == 3 and det.ptr.tolist() == [0, 2, 4, 6] and not det.is_aligned
    assert np.array_equal(det.node.cpu().numpy(), inst.first.cpu().numpy()) and det.scores.dtype == torch.float64
    bb_pred = [det.frame(f) for f in range(3)]
    bb_gt = [{"boxes": BoundingBoxes(inst.corners[2 * f:2 * f + 2], False), "labels": inst.cls[2 * f:2 * f + 2].double()} for f in range(3)]
    ptr = scene["ptr"]
    cls_pred = [{"pos": torch.from_numpy(scene["pos"][ptr[f]:ptr[f + 1]].astype(np.float32)).cuda()} for f in range(3)]
    res = ObjectDetectionMetrics.get_map(PostProcessingConfiguration(iou_for_mAP=0.3, use_point_iou=True, bg_index=BG), bb_pred, bb_gt, cls_pred)
    print(f"[cluster_objects] mAP of the clustering detector against its own boxes: {res['map'].item():.4f}")
    assert res["map"].item() >= 0.99
