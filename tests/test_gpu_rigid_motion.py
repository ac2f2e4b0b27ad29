"""Rigid motions on the device (csrc/transform.hip through radargnn_amd.transforms) against the float64 oracle
(tests/rigid_motion_oracle.py), against existing code that is not under test (``ops.decode_ground_truth``,
``create_2d_bounding_boxes_batched``), and against their own input where nothing may change.

Bars.
* identity motion, columns that are "not written", frames whose angle (and shift) is exactly 0: bit-equal.
* float32 outputs: within 1 ulp32 of the oracle.  Both sides evaluate the same float64 expression from the same stored operands and
  round once; only the device's sin / cos differ from numpy's, by U ulp64, which can move a float64 result across one float32
  rounding boundary and no further.
* float64 outputs of ``transform_frames``: |x' - oracle| <= (3 + U) eps64 (|c x| + |s y| + |t|), eps64 = 2^-52: the two products and
  the two sums are rounded on each side (4 x 2^-53 per side on the terms they touch, 3 eps64 together with margin), and the device's
  c and s differ from numpy's by at most U ulp64.  U = 1, measured: the ROCm math documentation is not installed with this
  toolchain, so the test measures the device's double sin and cos (``torch.sin`` / ``torch.cos`` of a float64 device tensor: the
  same two library functions the kernels call, and not code under test) against numpy over its own angles and asserts that the
  difference stays <= U.  On the MI355X: 1 ulp64 on the random angles of B3 and B70, 0 on the special ones (0, pi, 1e-9, pi / 2).
* rigid-body property: the corners ``ops.decode_ground_truth`` gives on the moved batch against ``R corners + t`` of its corners on
  the original batch: <= 4 ulp32(M) per coordinate, M the largest coordinate magnitude of the frame (points, centres and corners,
  before and after).  The decode of the original is exact in the stored operands (float64 noise); the moved batch stores rounded
  values: the centre (``none``: 1/2 ulp32(M); ``translation``: point + offset, 1/2 + 1/2) and theta' (1/2 ulp32(pi) = 2^-23 rad,
  which moves a corner by at most r 2^-23, r the half diagonal; some corner coordinate of the box is at least r / sqrt 2, so
  r <= sqrt 2 M and r 2^-23 <= 2 sqrt 2 M 2^-24 <= 2.83 ulp32(M)): 1 + 2.83 < 4.
* objects of >= 3 points with l != w of tests/golden/groundtruth_mixed.npz: the moved boxes against the boxes created from the moved
  points, the same bar.
"""
import math
import os

import numpy as np
import pytest
import torch

import rigid_motion_oracle as O
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

U = 1                                                  # ulp64 between the device's and numpy's sin / cos (see the docstring)
EPS64 = 2.0 ** -52
NODE_ORDERS = (["rcs", "velocity_vector", "time_index", "degree", "spatial_coordinates", "velocity_vector_length"],
               ["velocity_vector_length", "spatial_coordinates", "degree", "time_index", "velocity_vector", "rcs"])
EDGE_ORDERS = (["relative_position", "point_pair_features", "relative_velocity", "spatial_euclidean_distance", "velocity_euclidean_distance"],
               ["velocity_euclidean_distance", "spatial_euclidean_distance", "relative_velocity", "point_pair_features", "relative_position"])
BOX_MODES = (("none", False, "none"), ("translation", False, "translation"), ("en", False, "en"), ("aligned", True, "none"))
SEVEN = (0, 1, 2, 63, 64, 65, 257)
# name -> (rows per graph, edges per graph): B = 1, 3, 70; an empty graph, graphs of 1 ... 257 rows; a graph without edges, one with
# 257, and edge counts that cross the 256 boundary of a block (300 in one graph; 256 + 1 over two graphs; 4 061 over seventy)
SHAPES = {"B1": ([257], [257]), "B3": ([64, 0, 65], [300, 0, 0]), "B3b": ([2, 63, 1], [0, 256, 1]),
          "B70": (list(SEVEN) * 10, [0 if s == 0 else (0, 5, 257, 9)[k % 4] for k, s in enumerate(list(SEVEN) * 10)])}


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    from radargnn_amd import transforms
    return transforms


def motions(b: int, kind: str, seed: int = 0):
    """angle [b], shift [b, 2] on the host.  ``mixed``: exactly 0, pi, 1e-9, -1e-9 and random angles in turn; shifts with exact zeros
    (whole rows and single components) among random ones; frame 0 is the identity where b allows it."""
    rng = np.random.default_rng(100 + seed + b)
    if kind == "zero":
        angle = np.zeros(b)
    elif kind == "pi":
        angle = np.full(b, math.pi)
    elif kind == "tiny":
        angle = np.full(b, 1e-9)
    elif kind == "random":
        angle = rng.uniform(-2 * math.pi, 2 * math.pi, size=b)
    else:
        special = [0.0, math.pi, 1e-9, -1e-9, 0.0, -math.pi / 2]
        angle = np.array([special[k % 12] if k % 12 < len(special) else rng.uniform(-7.0, 7.0) for k in range(b)])
    shift = rng.uniform(-20.0, 20.0, size=(b, 2))
    if kind == "mixed":
        shift[0::4] = 0.0                               # with angle 0 at k = 0, 12, ...: the identity for that frame
        shift[1::8, 0] = 0.0
        shift[3::8, 1] = 0.0
    return angle, shift


_DATA = {}


def graph_data(shape: str, order: int, edge_mode: str, box: str):
    """A collated batch as numpy arrays (float32 where the device holds float32), made once per combination and never changed:
    real coordinates where they matter, sentinels (arbitrary bit patterns, a NaN with a payload among them) everywhere else."""
    key = (shape, order, edge_mode, box)
    if key in _DATA:
        return _DATA[key]
    sizes, edges = SHAPES[shape]
    rng = np.random.default_rng([len(sizes), order, edge_mode == "directed", sum(sizes)])
    n, ptr = sum(sizes), np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    batch = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    pos = rng.uniform(-50, 50, size=(n, 2)).astype(np.float32)
    vel = rng.normal(0, 3, size=(n, 2)).astype(np.float32)
    vel[rng.uniform(size=n) < 0.3] = 0.0
    sentinel = lambda *s: rng.integers(0x3A000000, 0x46000000, size=s, dtype=np.uint32).view(np.float32)
    nf, ef = NODE_ORDERS[order], EDGE_ORDERS[order]
    x = sentinel(n, sum(O.NODE_WIDTH[k] for k in nf))
    for nm, w in O.columns(nf, O.NODE_WIDTH)[0]:
        if nm == "spatial_coordinates":
            x[:, w:w + 2] = pos
        elif nm == "velocity_vector":
            x[:, w:w + 2] = vel
    if n:                                                                # a NaN with a payload in a column that never moves
        x.view(np.uint32)[n // 2, dict(O.columns(nf, O.NODE_WIDTH)[0])["rcs"]] = 0x7FC54321
    ei = np.concatenate([rng.integers(ptr[g], ptr[g + 1], size=(2, e)) if e else np.zeros((2, 0), dtype=np.int64)
                         for g, e in enumerate(edges)], axis=1).astype(np.int64)
    ea = sentinel(ei.shape[1], sum(O.EDGE_WIDTH[k] for k in ef))
    for nm, w in O.columns(ef, O.EDGE_WIDTH)[0]:
        if nm in ("relative_position", "relative_velocity"):
            q = (pos if nm == "relative_position" else vel).astype(np.float64)
            d = q[ei[0]] - q[ei[1]]
            ea[:, w:w + 2] = (np.abs(d) if edge_mode == "undirected" else d).astype(np.float32)
    _, aligned, inv = next(m for m in BOX_MODES if m[0] == box)
    y = sentinel(n, 1 + (4 if aligned else 5))
    y[:, 0] = rng.integers(0, 6, size=n)
    if not aligned and inv != "en":
        centre = pos + rng.normal(0, 2, size=(n, 2)).astype(np.float32)
        y[:, 1:3] = centre if inv == "none" else centre - pos
        y[:, 3:5] = rng.uniform(0.5, 12, size=(n, 2))
        y[:, 5] = rng.uniform(0, np.pi, size=n).astype(np.float32)
        y[y[:, 5] >= np.float32(np.pi), 5] = 0.0
        special = [0.0, np.nextafter(np.float32(np.pi), np.float32(0)), np.float32(np.pi / 2), np.float32(1e-9)]
        y[:min(n, len(special)), 5] = special[:min(n, len(special))]
    bg = rng.uniform(size=n) < 0.35
    if n > 8:
        bg[:4] = False
    y[bg, 1:] = np.nan
    if bg.any():
        y.view(np.uint32)[np.nonzero(bg)[0][0], 1:] = 0x7FC12345        # a NaN with a payload: kept, not recomputed
    _DATA[key] = dict(pos=pos, vel=vel, x=x, edge_index=ei, edge_attr=ea, y=y, batch=batch, ptr=ptr, node_features=nf,
                      edge_features=ef, edge_mode=edge_mode, aligned=aligned, inv=inv)
    return _DATA[key]


def to_batch(d):
    from radargnn_amd.data import Batch
    b = Batch(**{k: torch.from_numpy(d[k]).cuda() for k in ("x", "edge_index", "edge_attr", "y", "pos", "vel")})
    b.batch, b.ptr = torch.from_numpy(d["batch"]).cuda(), torch.from_numpy(d["ptr"]).cuda()
    return b


TENSORS = ("x", "edge_index", "edge_attr", "y", "pos", "vel", "batch", "ptr")


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def run(T, d, angle, shift, rotates=None):
    b = to_batch(d)
    before = {k: getattr(b, k).clone() for k in TENSORS}
    m = T.RigidMotion(angle, shift, rotates=rotates)
    assert m.angle.is_cuda and m.rotates == (bool(np.any(angle != 0)) if rotates is None else rotates)
    out = T.transform_graphs(b, m, d["node_features"], d["edge_features"], d["edge_mode"], d["aligned"], d["inv"])
    for k in TENSORS:                                                       # the input batch is left alone
        assert np.array_equal(bits(getattr(b, k)), bits(before[k])), k
    assert out is not b and out.keys == b.keys and out.num_graphs == b.num_graphs
    for k in ("edge_index", "batch", "ptr"):
        assert getattr(out, k) is getattr(b, k)                             # untouched tensors are shared
    return b, out


def moving_masks(d):
    """boolean column masks of x, edge_attr and y: True where a motion may write"""
    mx = np.zeros(d["x"].shape[1], dtype=bool)
    for nm, w in O.columns(d["node_features"], O.NODE_WIDTH)[0]:
        if nm in ("spatial_coordinates", "velocity_vector"):
            mx[w:w + 2] = True
    me = np.zeros(d["edge_attr"].shape[1], dtype=bool)
    for nm, w in O.columns(d["edge_features"], O.EDGE_WIDTH)[0]:
        if nm in ("relative_position", "relative_velocity"):
            me[w:w + 2] = True
    my = np.zeros(d["y"].shape[1], dtype=bool)
    if not d["aligned"] and d["inv"] != "en":
        my[[1, 2, 5]] = True
    return mx, me, my


def within_one_ulp(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float32 and want.dtype == np.float32, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64)) / O.ulp32(want[ok])
    worst = err.max() if err.size else 0.0
    assert worst <= 1.0, f"{what}: {worst} ulp32"
    return worst


def check_against_oracle(T, d, angle, shift, what):
    b, out = run(T, d, angle, shift)
    want = O.graph_nodes(d["pos"], d["vel"], d["x"], d["y"], d["batch"], angle, shift, d["node_features"], d["aligned"], d["inv"])
    want["edge_attr"] = O.graph_edges(d["edge_attr"], d["edge_features"], d["edge_mode"], d["edge_index"], d["batch"], angle,
                                      d["pos"], d["vel"])
    got = {k: getattr(out, k).cpu().numpy() for k in ("pos", "vel", "x", "y", "edge_attr")}
    worst = {k: within_one_ulp(got[k], want[k], f"{what} {k}") for k in got}
    mx, me, my = moving_masks(d)
    assert np.array_equal(bits(got["x"])[:, ~mx], bits(d["x"])[:, ~mx]), what             # not written: the sentinels, bit for bit
    assert np.array_equal(bits(got["edge_attr"])[:, ~me], bits(d["edge_attr"])[:, ~me]), what
    assert np.array_equal(bits(got["y"])[:, ~my], bits(d["y"])[:, ~my]), what
    nan_rows = np.isnan(d["y"][:, 1])
    assert np.array_equal(bits(got["y"])[nan_rows], bits(d["y"])[nan_rows]), what          # NaN box rows stay, payload included
    if my.any():
        theta = got["y"][~nan_rows, 5]
        assert bool((theta >= 0).all()) and bool((theta.astype(np.float64) < math.pi).all()), what
    # the exact-zero rule, frame by frame
    still = (angle == 0.0)[d["batch"]]
    fixed = still & (shift[d["batch"]] == 0.0).all(axis=1)
    estill = (angle == 0.0)[d["batch"][d["edge_index"][0]]]
    assert np.array_equal(bits(got["vel"])[still], bits(d["vel"])[still]), what
    assert np.array_equal(bits(got["edge_attr"])[estill], bits(d["edge_attr"])[estill]), what
    assert np.array_equal(bits(got["y"])[still][:, [5] if my.any() else []], bits(d["y"])[still][:, [5] if my.any() else []]), what
    for nm, w in O.columns(d["node_features"], O.NODE_WIDTH)[0]:
        if nm == "velocity_vector":
            assert np.array_equal(bits(got["x"])[still, w:w + 2], bits(d["x"])[still, w:w + 2]), what
    for k in ("pos", "vel", "x", "y"):
        assert np.array_equal(bits(got[k])[fixed], bits(d[k])[fixed]), (what, k)
    return b, out, worst


# ---------------------------------------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("shape", list(SHAPES))
def test_identity_motion_returns_the_input_bits(T, shape):
    for order in (0, 1):
        for edge_mode in ("directed", "undirected"):
            for box, _, _ in BOX_MODES:
                d = graph_data(shape, order, edge_mode, box)
                b = to_batch(d)
                out = T.transform_graphs(b, T.RigidMotion.identity(len(SHAPES[shape][0])), d["node_features"], d["edge_features"],
                                         edge_mode, d["aligned"], d["inv"])
                for k in TENSORS:
                    assert np.array_equal(bits(getattr(out, k)), bits(d[k])), (shape, order, edge_mode, box, k)
                # zeros whose rotates flag says True take the kernels' own zero branches
                bz, outz = run(T, d, np.zeros(len(SHAPES[shape][0])), np.zeros((len(SHAPES[shape][0]), 2)), rotates=not d["aligned"])
                for k in TENSORS:
                    assert np.array_equal(bits(getattr(outz, k)), bits(d[k])), (shape, order, edge_mode, box, k)


# ---------------------------------------------------------------------------------------------- 2. against the oracle
CASES = [("B1", "zero"), ("B1", "pi"), ("B1", "tiny"), ("B1", "random"), ("B3", "mixed"), ("B3", "random"), ("B3b", "mixed"),
         ("B70", "mixed"), ("B70", "random")]


@pytest.mark.parametrize("box", [m[0] for m in BOX_MODES])
@pytest.mark.parametrize("shape,kind", CASES, ids=[f"{s}-{k}" for s, k in CASES])
def test_graphs_match_the_oracle(T, shape, kind, box):
    worst = {}
    for order in (0, 1):
        for edge_mode in ("directed", "undirected"):
            d = graph_data(shape, order, edge_mode, box)
            angle, shift = motions(len(SHAPES[shape][0]), kind, seed=order)
            if d["aligned"]:
                angle = np.zeros_like(angle)                                # aligned boxes: a pure shift
            _, out, w = check_against_oracle(T, d, angle, shift, f"{shape} {kind} {box} order {order} {edge_mode}")
            for k, v in w.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(f"[rigid] {shape} {kind} {box}: worst ulp32 " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


def test_sharing_follows_what_moves(T):
    d = graph_data("B3", 0, "directed", "en")
    b = to_batch(d)
    shift_only = T.RigidMotion(np.zeros(3), np.ones((3, 2)))
    out = T.transform_graphs(b, shift_only, d["node_features"], d["edge_features"], "directed", False, "en")
    assert out.vel is b.vel and out.edge_attr is b.edge_attr and out.y is b.y and out.x is not b.x and out.pos is not b.pos
    out = T.transform_graphs(b, shift_only, ["rcs", "degree"], ["point_pair_features"], "directed", False, "translation")
    assert out.x is b.x and out.y is b.y and out.edge_attr is b.edge_attr
    turn = T.RigidMotion(np.ones(3), np.zeros((3, 2)))
    out = T.transform_graphs(b, turn, ["rcs", "degree"], ["point_pair_features"], "directed", False, "en")
    assert out.x is b.x and out.y is b.y and out.edge_attr is b.edge_attr and out.vel is not b.vel
    with pytest.raises(ValueError, match="aligned"):
        T.transform_graphs(b, turn, d["node_features"], d["edge_features"], "directed", True, "none")
    with pytest.raises(ValueError, match="frames"):
        T.transform_graphs(b, T.RigidMotion.identity(2), d["node_features"], d["edge_features"], "directed", False, "en")


def test_rows_wider_than_their_feature_list(T):
    """x as a view of a wider tensor (row stride 11): the leading dimension is honoured and the input view is left alone"""
    d = graph_data("B3", 1, "directed", "none")
    b = to_batch(d)
    wide = torch.full((d["x"].shape[0], 11), 7.0, device="cuda")
    wide[:, :d["x"].shape[1]] = b.x
    b.x = wide[:, :d["x"].shape[1]]
    angle, shift = motions(3, "random")
    out = T.transform_graphs(b, T.RigidMotion(angle, shift), d["node_features"], d["edge_features"], "directed", False, "none")
    want = O.graph_nodes(None, None, d["x"], None, d["batch"], angle, shift, d["node_features"], False, "none")["x"]
    within_one_ulp(out.x.cpu().numpy(), want, "strided x")
    assert bool((wide[:, d["x"].shape[1]:] == 7.0).all()) and np.array_equal(bits(b.x), bits(d["x"]))


# ---------------------------------------------------------------------------------------------- 3. frames (float64)
def device_trig_ulps(angle):
    """ulp64 between the device's double sin / cos (torch on the device: not the code under test) and numpy's"""
    a = torch.from_numpy(angle).cuda()
    worst = 0.0
    for dev, ref in ((torch.sin(a).cpu().numpy(), np.sin(angle)), (torch.cos(a).cpu().numpy(), np.cos(angle))):
        worst = max(worst, float((np.abs(dev - ref) / np.spacing(np.abs(ref))).max()))
    return worst


@pytest.mark.parametrize("shape,kind", CASES, ids=[f"{s}-{k}" for s, k in CASES])
def test_frames_match_the_oracle(T, shape, kind):
    from radargnn_amd.frames import FrameBatch
    sizes = SHAPES[shape][0]
    rng = np.random.default_rng(len(sizes))
    n, ptr = sum(sizes), np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    X, V = rng.uniform(-100, 100, size=(n, 2)), rng.normal(0, 5, size=(n, 2))
    V[rng.uniform(size=n) < 0.3] = 0.0
    if n > 2:
        X[1] = [-0.0, 0.0]
        V[2] = [0.0, -0.0]
    angle, shift = motions(len(sizes), kind)
    measured = device_trig_ulps(angle)
    print(f"[rigid] {shape} {kind}: device sin / cos against numpy over these angles: {measured:.2f} ulp64 (U = {U})")
    assert measured <= U
    up = lambda a: torch.from_numpy(a).cuda()
    fb = FrameBatch(up(X), up(V), up(rng.normal(size=n)), up(rng.normal(size=n)), up(ptr), np.diff(ptr))
    out = T.transform_frames(fb, T.RigidMotion(angle, shift))
    assert out.rcs is fb.rcs and out.timestamp is fb.timestamp and out.frame_ptr is fb.frame_ptr and out.frame_sizes is fb.frame_sizes
    assert np.array_equal(bits(fb.X), bits(X)) and np.array_equal(bits(fb.V), bits(V))      # the input is left alone
    gx, gv = out.X.cpu().numpy(), out.V.cpu().numpy()
    wx, wv = O.rigid_points(X, V, ptr, angle, shift)
    f = O.frame_of_rows(ptr, n)
    c, s, t = np.abs(np.cos(angle))[f], np.abs(np.sin(angle))[f], np.abs(shift)[f]
    for got, want, q, tt, nm in ((gx, wx, X, t, "X"), (gv, wv, V, 0 * t, "V")):
        bar = (3 + U) * EPS64 * np.stack([c * np.abs(q[:, 0]) + s * np.abs(q[:, 1]) + tt[:, 0],
                                          s * np.abs(q[:, 0]) + c * np.abs(q[:, 1]) + tt[:, 1]], axis=1)
        err = np.abs(got - want)
        ratio = float((err / np.maximum(bar, 1e-300)).max()) if n else 0.0
        print(f"[rigid] {shape} {kind} {nm}: worst error / bar {ratio:.3f}")
        assert bool((err <= bar).all()), (nm, ratio)
    still = (angle == 0.0)[f]
    fixed = still & (shift[f] == 0.0).all(axis=1)
    assert np.array_equal(bits(gv)[still], bits(V)[still]) and np.array_equal(bits(gx)[fixed], bits(X)[fixed])
    ident = T.transform_frames(fb, T.RigidMotion.identity(len(sizes)))
    assert np.array_equal(bits(ident.X), bits(X)) and np.array_equal(bits(ident.V), bits(V))
    with pytest.raises(ValueError, match="frames"):
        T.transform_frames(fb, T.RigidMotion.identity(len(sizes) + 1))


# ---------------------------------------------------------------------------------------------- 4. rigid bodies
def same_rectangles(got, want):
    """per row: max |got - want| over the corners, where a theta' folded by pi lists the SAME rectangle from the opposite corner"""
    d0 = np.abs(got - want).max(axis=(1, 2))
    d2 = np.abs(got - np.roll(want, 2, axis=1)).max(axis=(1, 2))
    return np.minimum(d0, d2)


def frame_magnitude(batch, num, *arrays):
    """per frame: the largest |coordinate| over the given [rows, ...] arrays (rows listed by ``batch``)"""
    m = np.zeros(num)
    for a in arrays:
        flat = np.abs(a.reshape(a.shape[0], -1)).max(axis=1) if a.shape[0] else np.zeros(0)
        np.maximum.at(m, batch, flat)
    return m


def decode(ops, y, pos, inv):
    keep, corners = ops.decode_ground_truth(y[:, 0], y[:, 1:], pos, None, 5, O.INVARIANCE[inv])
    return corners.cpu().numpy()


@pytest.mark.parametrize("inv", ["none", "translation"])
@pytest.mark.parametrize("shape,kind", [("B3", "mixed"), ("B70", "mixed"), ("B70", "random")])
def test_decoded_boxes_move_as_rigid_bodies(T, shape, kind, inv):
    from radargnn_amd import ops
    d = graph_data(shape, 0, "directed", inv)
    angle, shift = motions(len(SHAPES[shape][0]), kind)
    b, out = run(T, d, angle, shift)
    box = ~np.isnan(d["y"][:, 1])
    rows = d["batch"][box]
    before = decode(ops, b.y, b.pos, inv)[box]
    after = decode(ops, out.y, out.pos, inv)[box]
    want = O.move_corners(before, angle[rows], shift[rows])
    m = frame_magnitude(rows, len(angle), before, want, after, d["pos"][box].astype(np.float64), out.pos.cpu().numpy()[box].astype(np.float64))
    err = same_rectangles(after, want) / O.ulp32(m[rows])
    print(f"[rigid] {shape} {kind} {inv}: {int(box.sum())} boxes, worst corner error {err.max():.2f} ulp32 of the frame's largest "
          f"coordinate (bar 4)")
    assert err.max() <= 4.0


@pytest.mark.parametrize("inv", ["none", "translation"])
def test_moved_boxes_agree_with_boxes_created_from_moved_points(T, inv):
    from radargnn_amd import groundtruth, ops
    from radargnn_amd.data import Batch
    g = np.load(os.path.join(GOLDEN, "groundtruth_mixed.npz"))
    pos64, oid, ptr = g["pos"], g["object_id"], g["frame_ptr"].astype(np.int64)
    pos32 = pos64.astype(np.float32)
    frames = len(ptr) - 1
    batch = np.repeat(np.arange(frames), np.diff(ptr)).astype(np.int64)
    # the boxes of the float32 points (what a stored graph holds), as targets
    boxes = groundtruth.create_2d_bounding_boxes_batched(pos32.astype(np.float64), oid, ptr.tolist(), False, inv)
    y = groundtruth.merge_targets(np.where(oid >= 0, 1.0, 5.0), boxes)
    b = Batch(y=y, pos=torch.from_numpy(pos32).cuda())
    b.batch, b.ptr = torch.from_numpy(batch).cuda(), torch.from_numpy(ptr).cuda()
    angle, shift = motions(frames, "random", seed=5)
    out = T.transform_graphs(b, T.RigidMotion(angle, shift), [], [], "directed", False, inv)
    moved_pos = out.pos.cpu().numpy()
    created = groundtruth.create_2d_bounding_boxes_batched(moved_pos.astype(np.float64), oid, ptr.tolist(), False, inv).cpu().numpy()
    # objects of at least three points with l != w
    key = batch * (int(oid.max()) + 2) + oid
    count = {k: int(c) for k, c in zip(*np.unique(key[oid >= 0], return_counts=True))}
    rows = np.array([o >= 0 and count[k] >= 3 for o, k in zip(oid, key)])
    rows &= ~np.isnan(created[:, 0]) & (boxes.cpu().numpy()[:, 2] != boxes.cpu().numpy()[:, 3])
    assert rows.sum() >= 20
    after = decode(ops, out.y, out.pos, inv)[rows]
    want = O.box_corners(created[rows], moved_pos[rows], inv)
    m = frame_magnitude(batch[rows], frames, after, want, moved_pos[rows].astype(np.float64), pos64[rows])
    err = same_rectangles(after, want) / O.ulp32(m[batch[rows]])
    print(f"[rigid] golden {inv}: {int(rows.sum())} rows of objects with >= 3 points, moved boxes against boxes created from the moved "
          f"points: worst corner difference {err.max():.2f} ulp32 of the frame's largest coordinate (bar 4)")
    assert err.max() <= 4.0
