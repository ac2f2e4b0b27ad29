"""Rigid motions in numpy float64 -- the formulas of radargnn_amd.transforms (include/rgnn.h, "rigid motions") applied to the same
stored operands and rounded once to the output dtype.  Test infrastructure: nothing here is imported by the package.

    p' = R(a_f) p + t_f,  v' = R(a_f) v,  R = [[c, -s], [s, c]],  a_f in radians, counter-clockwise

Every product and sum is a separate float64 operation in the order ``c x - s y`` / ``s x + c y``, then ``+ t``.  An angle of exactly
0 leaves rotated quantities as they are, a shift component of exactly 0 is not added.  ``theta' = fmod(theta + a, pi)`` folded into
[0, pi); a value that rounds to float32(pi) becomes 0."""
import numpy as np

NODE_WIDTH = {"rcs": 1, "time_index": 1, "degree": 1, "velocity_vector_length": 1, "velocity_vector": 2, "spatial_coordinates": 2}
EDGE_WIDTH = {"point_pair_features": 4, "spatial_euclidean_distance": 1, "velocity_euclidean_distance": 1, "relative_position": 2,
              "relative_velocity": 2}
INVARIANCE = {"none": 0, "translation": 1, "en": 2}
PI = 3.141592653589793


def columns(names, widths):
    """{name: first column} of a feature list (a name met twice keeps every position: -> list of (name, column))"""
    out, w = [], 0
    for nm in names:
        out.append((nm, w))
        w += widths[nm]
    return out, w


def rotate(angle, x, y):
    """R(angle) (x, y) per row, float64; rows whose angle is exactly 0 come back untouched"""
    angle, x, y = (np.asarray(v, dtype=np.float64) for v in (angle, x, y))
    c, s = np.cos(angle), np.sin(angle)
    rot = angle != 0.0
    with np.errstate(invalid="ignore"):
        return np.where(rot, c * x - s * y, x), np.where(rot, s * x + c * y, y)


def move(angle, shift, x, y):
    """R(angle) (x, y) + shift per row; a shift component of exactly 0 is not added"""
    rx, ry = rotate(angle, x, y)
    shift = np.asarray(shift, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(shift[:, 0] != 0.0, rx + shift[:, 0], rx), np.where(shift[:, 1] != 0.0, ry + shift[:, 1], ry)


def wrap(theta, angle, dtype=np.float32):
    """theta + angle folded into [0, pi), rounded once to ``dtype``; float32: what rounds to float32(pi) is 0.  Rows whose angle is
    exactly 0 keep theta."""
    theta64, angle = np.asarray(theta, dtype=np.float64), np.asarray(angle, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        t = np.fmod(theta64 + angle, PI)
        t = np.where(t < 0.0, t + PI, t)
        t = np.where(t >= PI, t - PI, t)
        r = t.astype(dtype)
        if dtype == np.float32:
            r = np.where(r >= np.float32(PI), np.float32(0.0), r)
    return np.where(angle != 0.0, r, np.asarray(theta).astype(dtype))


def frame_of_rows(frame_ptr, n):
    """the frame of every row: the last f with frame_ptr[f] <= i (empty frames are stepped over)"""
    return np.searchsorted(np.asarray(frame_ptr)[1:], np.arange(n), side="right")


def rigid_points(X, V, frame_ptr, angle, shift):
    """-> X', V' float64 [N, 2]"""
    f = frame_of_rows(frame_ptr, len(X))
    a, t = np.asarray(angle, dtype=np.float64)[f], np.asarray(shift, dtype=np.float64).reshape(-1, 2)[f]
    return np.stack(move(a, t, X[:, 0], X[:, 1]), axis=1), np.stack(rotate(a, V[:, 0], V[:, 1]), axis=1)


def graph_nodes(pos, vel, x, y, batch, angle, shift, node_features, aligned, bb_invariance, dtype=np.float32):
    """-> dict(pos, vel, x, y) in ``dtype``; any input may be None.  Columns that do not move are copied bit for bit."""
    batch = np.asarray(batch)
    a, t = np.asarray(angle, dtype=np.float64)[batch], np.asarray(shift, dtype=np.float64).reshape(-1, 2)[batch]
    out = {"pos": None, "vel": None, "x": None, "y": None}
    if pos is not None:
        out["pos"] = np.stack(move(a, t, pos[:, 0], pos[:, 1]), axis=1).astype(dtype)
    if vel is not None:
        out["vel"] = np.stack(rotate(a, vel[:, 0], vel[:, 1]), axis=1).astype(dtype)
    if x is not None:
        xo = np.array(x, dtype=dtype, copy=True)
        for nm, w in columns(node_features, NODE_WIDTH)[0]:
            if nm == "spatial_coordinates":
                rx, ry = move(a, t, x[:, w], x[:, w + 1])
            elif nm == "velocity_vector":
                rx, ry = rotate(a, x[:, w], x[:, w + 1])
            else:
                continue
            xo[:, w], xo[:, w + 1] = rx.astype(dtype), ry.astype(dtype)
        out["x"] = xo
    if y is not None:
        yo = np.array(y, dtype=dtype, copy=True)
        inv = INVARIANCE[bb_invariance]
        if not aligned and inv != 2:
            box = ~np.isnan(y[:, 1])
            rx, ry = move(a, t, y[:, 1], y[:, 2]) if inv == 0 else rotate(a, y[:, 1], y[:, 2])
            yo[box, 1], yo[box, 2] = rx.astype(dtype)[box], ry.astype(dtype)[box]
            yo[box, 5] = wrap(y[:, 5], a, dtype)[box]
        out["y"] = yo
    return out


def graph_edges(edge_attr, edge_features, edge_mode, edge_index, batch, angle, pos, vel, dtype=np.float32):
    """-> edge_attr' in ``dtype``; the frame of edge e is batch[edge_index[0, e]]"""
    out = np.array(edge_attr, dtype=dtype, copy=True)
    i, j = np.asarray(edge_index)[0], np.asarray(edge_index)[1]
    a = np.asarray(angle, dtype=np.float64)[np.asarray(batch)[i]]
    rot = a != 0.0
    for nm, w in columns(edge_features, EDGE_WIDTH)[0]:
        if nm not in ("relative_position", "relative_velocity"):
            continue
        if edge_mode == "directed":
            rx, ry = rotate(a, edge_attr[:, w], edge_attr[:, w + 1])
        else:
            q = np.asarray(pos if nm == "relative_position" else vel, dtype=np.float64)
            rx, ry = rotate(a, q[i, 0] - q[j, 0], q[i, 1] - q[j, 1])
            rx, ry = np.abs(rx), np.abs(ry)
        out[rot, w], out[rot, w + 1] = rx.astype(dtype)[rot], ry.astype(dtype)[rot]
    return out


def box_corners(boxes, pos, bb_invariance):
    """Corners c1..c4 [N, 4, 2] float64 of rotated boxes [c0, c1, l, w, theta]: the corner decode of the post-processor restated
    (half sizes (+, +), (+, -), (-, -), (-, +) turned by theta about the centre; ``translation``: the centre is pos + (c0, c1))."""
    boxes, pos = np.asarray(boxes, dtype=np.float64), np.asarray(pos, dtype=np.float64)
    inv = INVARIANCE[bb_invariance]
    assert inv != 2
    cx = boxes[:, 0] + (pos[:, 0] if inv == 1 else 0.0)
    cy = boxes[:, 1] + (pos[:, 1] if inv == 1 else 0.0)
    hl, hw, th = boxes[:, 2] / 2, boxes[:, 3] / 2, boxes[:, 4]
    c, s = np.cos(th), np.sin(th)
    ox = np.stack([hl, hl, -hl, -hl], axis=1)
    oy = np.stack([hw, -hw, -hw, hw], axis=1)
    return np.stack([c[:, None] * ox - s[:, None] * oy + cx[:, None], s[:, None] * ox + c[:, None] * oy + cy[:, None]], axis=2)


def move_corners(corners, angle, shift):
    """R corners + t per row of [N, 4, 2] (float64, plain formula: the yardstick of the rigid-body property)"""
    c, s = np.cos(angle)[:, None], np.sin(angle)[:, None]
    shift = np.asarray(shift, dtype=np.float64)
    return np.stack([c * corners[:, :, 0] - s * corners[:, :, 1] + shift[:, :1], s * corners[:, :, 0] + c * corners[:, :, 1] + shift[:, 1:]],
                    axis=2)


def ulp32(v):
    """the spacing of float32 at |v| (of the smallest normal below it)"""
    return np.spacing(np.maximum(np.abs(np.asarray(v, dtype=np.float32)), np.float32(2.0 ** -126))).astype(np.float64)
