"""Float64 numpy oracle of the nuScenes sample stage (radargnn_amd/nuscenes.py, csrc/nuscenes.hip), written from the description
of the reference's preprocessor/nuscenes (get_sensor_points, the two crops, get_labels, extended_points_in_box,
convert_bounding_boxes), not from its code and not from the device code: everything is vectorised over rows, boxes and
(box, point) pairs with einsum, where the reference loops and the device walks.  Pinned to reference-generated fixtures by
tests/test_nuscenes_oracle.py; the GPU tests compare against it where no fixture exists (fuzz).

Also the admissibility filter shared by the fixture maker and the fuzz test: inputs on which two implementations may
legitimately disagree (a point within rounding of a box face or a crop limit, a box centre within rounding of a crop limit, two
sides of a rectangle of nearly equal length, an angle on a wrap point, two nearest neighbours at nearly the same distance) are
rejected when the samples are DRAWN, so the tests compare every row they hold.

Inputs are a dict of arrays with the field names of ``radargnn_amd.nuscenes.NuScenesSamples``.
"""
import numpy as np

INVARIANCE_CODES = {"none": 0, "translation": 1, "en": 2}
MODES = ("none", "translation", "en")
INPUT_KEYS = ("points", "chunk_ptr", "chunk_sample", "chunk_rotation", "chunk_translation", "box_center", "box_size", "box_rotation",
              "box_label", "box_points", "box_ptr", "ego_translation", "ego_rotation")
# the devkit's corner order (Box.corners): x along the length, y along the width, z up
CORNER_SIGNS = np.array([[1, 1, 1, 1, -1, -1, -1, -1], [1, -1, -1, 1, 1, -1, -1, 1], [1, 1, -1, -1, 1, 1, -1, -1]], dtype=np.float64)


def rotation_matrices(q):
    """[..., 4] quaternions (w, x, y, z), normalised here -> [..., 3, 3]."""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    rows = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    return np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)


# ---------------------------------------------------------------------------------------------------- points
def sample_point_clouds(inp, crop, xlim, ylim):
    """-> dict: frame_ptr, X, V, V_cc [N, 2], rcs, timestamp [N], src_row, and for the margins xy_all [N_total, 2]."""
    pts = np.asarray(inp["points"], dtype=np.float64)
    cptr, csample = np.asarray(inp["chunk_ptr"]), np.asarray(inp["chunk_sample"])
    n_samples = len(inp["box_ptr"]) - 1
    chunk_of_row = np.repeat(np.arange(len(csample)), np.diff(cptr))
    R = rotation_matrices(inp["chunk_rotation"])[chunk_of_row]
    xyz = np.einsum("nij,jn->ni", R, pts[:3]) + np.asarray(inp["chunk_translation"], dtype=np.float64)[chunk_of_row]
    v = np.einsum("nij,jn->ni", R[:, :2, :2], pts[8:10])
    keep = np.ones(pts.shape[1], dtype=bool)
    if crop:
        keep = ~((xyz[:, 0] > xlim) | (xyz[:, 0] < -xlim) | (xyz[:, 1] > ylim) | (xyz[:, 1] < -ylim))
    rows = np.nonzero(keep)[0]
    counts = np.bincount(csample[chunk_of_row][rows], minlength=n_samples)
    return {"frame_ptr": np.concatenate(([0], np.cumsum(counts))).astype(np.int64), "X": xyz[rows, :2], "V": v[rows],
            "V_cc": pts[6:8, rows].T, "rcs": pts[5, rows], "timestamp": pts[18, rows], "src_row": rows.astype(np.int32),
            "xy_all": xyz[:, :2]}


# ---------------------------------------------------------------------------------------------------- boxes
def vehicle_boxes(inp, crop, xlim, ylim):
    """-> dict: kept (indices into the input list, list order), kept_ptr [B + 1], center [K, 3], R [K, 3, 3], wlh [K, 3],
    label [K], and for the margins center_all [M, 3]."""
    bptr = np.asarray(inp["box_ptr"])
    sample_of_box = np.repeat(np.arange(len(bptr) - 1), np.diff(bptr))
    Re = rotation_matrices(inp["ego_rotation"])[sample_of_box]
    d = np.asarray(inp["box_center"], dtype=np.float64) - np.asarray(inp["ego_translation"], dtype=np.float64)[sample_of_box]
    c = np.einsum("mji,mj->mi", Re, d)
    Rv = np.einsum("mji,mjk->mik", Re, rotation_matrices(inp["box_rotation"]))
    keep = np.asarray(inp["box_points"]) > 0
    if crop:
        keep &= (-xlim < c[:, 0]) & (c[:, 0] < xlim) & (-ylim < c[:, 1]) & (c[:, 1] < ylim)
    kept = np.nonzero(keep)[0]
    counts = np.bincount(sample_of_box[kept], minlength=len(bptr) - 1)
    return {"kept": kept, "kept_ptr": np.concatenate(([0], np.cumsum(counts))).astype(np.int64), "center": c[kept], "R": Rv[kept],
            "wlh": np.asarray(inp["box_size"], dtype=np.float64)[kept], "label": np.asarray(inp["box_label"])[kept],
            "center_all": c}


def corners(center, R, wlh, factor):
    """[K, 3, 8]: the devkit's Box.corners(wlh_factor)."""
    s = wlh * factor
    local = np.stack([s[:, 1] / 2, s[:, 0] / 2, s[:, 2] / 2], axis=1)[:, :, None] * CORNER_SIGNS[None]
    return np.einsum("kij,kjc->kic", R, local) + center[:, :, None]


def rectangles(center, R, wlh):
    """-> (rect [K, 5] = x_c, y_c, l, w, theta in degrees (0 <= theta <= 180), d [K, 3] the three distances from the first bottom
    corner) of the bottom corners [2, 3, 7, 6] of corners(1), x and y only."""
    p = corners(center, R, wlh, 1.0)[:, :2, :][:, :, [2, 3, 7, 6]]
    if len(p) == 0:
        return np.zeros((0, 5)), np.zeros((0, 3))
    diff = p[:, :, :1] - p[:, :, 1:]                                   # p1 - p2, p1 - p3, p1 - p4
    d = np.sqrt((diff * diff).sum(1))
    k = np.arange(len(p))
    wi = d.argmin(1)                                                   # the first smallest is the width
    rest = d.copy()
    rest[k, wi] = np.inf
    l = rest.min(1)
    li = (d == l[:, None]).argmax(1)                                   # the first side equal to the length gives the direction
    v = diff[k, :, li]
    v = v / np.sqrt((v * v).sum(1, keepdims=True))
    theta = np.degrees(np.arctan2(v[:, 1], v[:, 0]))
    theta = np.where(theta < 0, 180 + theta, theta)
    c = (((p[:, :, 0] + p[:, :, 1]) + p[:, :, 2]) + p[:, :, 3]) / 4
    return np.stack([c[:, 0], c[:, 1], l, d[k, wi], theta], axis=1), d


def membership(pos, center, R, wlh, factor, offset):
    """(inside bool [K, P], margin [K, P]: the least distance of i.v / |i|, j.v / |j| from their four bounds; inf for a box with a
    zero side, which contains nothing)."""
    cor = corners(center, R, wlh, factor)
    p1, i, j = cor[:, :, 0], cor[:, :, 4] - cor[:, :, 0], cor[:, :, 1] - cor[:, :, 0]
    ni, nj = np.sqrt((i * i).sum(1)), np.sqrt((j * j).sum(1))
    v = np.concatenate((pos, np.zeros((len(pos), 1))), axis=1)[None] - p1[:, None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        iv = np.einsum("kd,kpd->kp", i, v) / ni[:, None]
        jv = np.einsum("kd,kpd->kp", j, v) / nj[:, None]
        inside = (-offset <= iv) & (iv <= ni[:, None] + offset) & (-offset <= jv) & (jv <= nj[:, None] + offset)
        margin = np.minimum(np.minimum(np.abs(iv + offset), np.abs(ni[:, None] + offset - iv)),
                            np.minimum(np.abs(jv + offset), np.abs(nj[:, None] + offset - jv)))
    return inside, np.where(np.isnan(margin), np.inf, margin)


def nearest_in_frames(pos, frame_ptr):
    """(index of the nearest other point of the frame, relative gap between the nearest and the second nearest distance)."""
    nn, gap = np.full(len(pos), -1, dtype=np.int64), np.full(len(pos), np.inf)
    for a, b in zip(frame_ptr[:-1], frame_ptr[1:]):
        if b - a < 2:
            continue
        p = pos[a:b]
        d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(2)
        np.fill_diagonal(d2, np.inf)
        nn[a:b] = a + d2.argmin(1)
        if b - a > 2:
            s = np.sqrt(np.sort(d2, axis=1)[:, :2])
            with np.errstate(invalid="ignore", divide="ignore"):
                gap[a:b] = np.where(s[:, 1] > 0, (s[:, 1] - s[:, 0]) / s[:, 1], 0.0)
    return nn, gap


def _en(p, q, rect):
    """The en columns of points p with neighbours q and rectangles rect: (d, b, a in degrees, and both angles before rounding and
    wrapping; the centre angle is NaN where the point is the centre)."""
    v = q - p
    v = v / np.sqrt((v * v).sum(1, keepdims=True))
    th_nn = np.degrees(np.arctan2(v[:, 1], v[:, 0]))
    xr, yr = rect[:, 0] - p[:, 0], rect[:, 1] - p[:, 1]
    t = np.tan(rect[:, 4] * np.pi / 180)
    dn = np.sqrt(1.0 + t * t)
    raw_a = np.degrees(np.arctan2(t / dn, 1.0 / dn)) - th_nn
    a = np.round(raw_a, 5)
    a = np.where(a < 0, 360 + a, a)
    a = np.where(a >= 180, a - 180, a)
    d = np.sqrt(xr * xr + yr * yr)
    with np.errstate(invalid="ignore", divide="ignore"):
        raw_b = np.degrees(np.arctan2(yr / d, xr / d)) - th_nn
    b = np.round(raw_b, 5)
    b = np.where(b < 0, 360 + b, b)
    b = np.where(d != 0, b, 0.0)
    return d, b, a, np.where(d != 0, raw_b, np.nan), raw_a


def create(inp, crop, xlim, ylim, factor, offset, modes=MODES):
    """Everything the stage produces: the dicts of ``sample_point_clouds`` and ``vehicle_boxes`` merged, plus rect [K, 5], labels
    int [N], hit int [N] (index of the winning box in the INPUT list, -1), boxes_<mode> [N, 5] and the margins' raw material."""
    out = sample_point_clouds(inp, crop, xlim, ylim)
    out.update(vehicle_boxes(inp, crop, xlim, ylim))
    rect, dist = rectangles(out["center"], out["R"], out["wlh"])
    pos, fptr, kptr = out["X"], out["frame_ptr"], out["kept_ptr"]
    win = np.full(len(pos), -1, dtype=np.int64)                        # index into the kept list
    face = np.full(len(pos), np.inf)
    for s in range(len(fptr) - 1):
        a, b, ka, kb = fptr[s], fptr[s + 1], kptr[s], kptr[s + 1]
        if a == b or ka == kb:
            continue
        inside, margin = membership(pos[a:b], out["center"][ka:kb], out["R"][ka:kb], out["wlh"][ka:kb], factor, offset)
        last = (kb - ka - 1) - inside[::-1].argmax(0)                  # the last box in list order that contains the point
        win[a:b] = np.where(inside.any(0), ka + last, -1)
        face[a:b] = margin.min(0)
    has = win >= 0
    hit, labels = np.full(len(pos), -1, dtype=np.int64), np.zeros(len(pos), dtype=np.int64)
    hit[has], labels[has] = out["kept"][win[has]], out["label"][win[has]]
    out.update(rect=rect, side_distances=dist, face_margin=face, win=win, hit=hit, labels=labels)
    nn, gap = nearest_in_frames(pos, fptr)
    out.update(nn=nn, nn_gap=gap)
    rows = np.nonzero(has)[0]
    r, p = rect[win[rows]], pos[rows]
    for mode in modes:
        boxes = np.full((len(pos), 5), np.nan)
        if mode == "none":
            boxes[rows] = np.stack([p[:, 0] + (r[:, 0] - p[:, 0]), p[:, 1] + (r[:, 1] - p[:, 1]), r[:, 2], r[:, 3], (r[:, 4] * np.pi) / 180], 1)
        elif mode == "translation":
            boxes[rows] = np.stack([r[:, 0] - p[:, 0], r[:, 1] - p[:, 1], r[:, 2], r[:, 3], (r[:, 4] * np.pi) / 180], 1)
        elif mode == "en":
            if (np.diff(fptr) == 1).any():
                raise ValueError("Expected n_neighbors < n_samples_fit, but n_neighbors = 1, n_samples_fit = 1")
            if len(rows):
                d, b, a, raw_b, raw_a = _en(p, pos[nn[rows]], r)
                boxes[rows] = np.stack([d, (b * np.pi) / 180, r[:, 2], r[:, 3], (a * np.pi) / 180], 1)
                out["en_raw"] = (raw_b, raw_a)
        else:
            raise ValueError("Wrong invariance for bounding box selection")
        out["boxes_" + mode] = boxes
    return out


# ---------------------------------------------------------------------------------------------------- admissibility
def _wrap_distance(x, period):
    r = np.mod(x, period)
    return np.minimum(r, period - r)


def admissibility(inp, crop, xlim, ylim, factor, offset):
    """The margins of a batch of samples: dict of arrays (inf where a margin does not apply):
      face       per kept point: the least distance (m) of i.v / |i|, j.v / |j| from their bounds, over the sample's boxes
      point_crop per input row: the distance (m) of x, y from the crop limits
      box_crop   per input box with points: the distance (m) of the centre's x, y from the crop limits
      sides      per kept box: the least gap (m) between the three distances d1, d2, d3
      theta      per kept box: degrees from theta to 0 / 180
      nn         per kept point: relative gap between nearest and second-nearest neighbour distance
      en         per point with a box: degrees from either en angle (before rounding) to its wrap point."""
    o = create(inp, crop, xlim, ylim, factor, offset, modes=("en",))
    m = {"face": o["face_margin"], "nn": o["nn_gap"]}
    if crop:
        xy = o["xy_all"]
        m["point_crop"] = np.minimum(np.abs(np.abs(xy[:, 0]) - xlim), np.abs(np.abs(xy[:, 1]) - ylim))
        c = o["center_all"][np.asarray(inp["box_points"]) > 0]
        m["box_crop"] = np.minimum(np.abs(np.abs(c[:, 0]) - xlim), np.abs(np.abs(c[:, 1]) - ylim))
    else:
        m["point_crop"], m["box_crop"] = np.full(1, np.inf), np.full(1, np.inf)
    d = o["side_distances"]
    m["sides"] = np.minimum(np.minimum(np.abs(d[:, 0] - d[:, 1]), np.abs(d[:, 0] - d[:, 2])), np.abs(d[:, 1] - d[:, 2]))
    m["theta"] = np.minimum(o["rect"][:, 4], 180 - o["rect"][:, 4])
    if "en_raw" in o:
        raw_b, raw_a = o["en_raw"]
        m["en"] = np.minimum(_wrap_distance(raw_a, 180), np.where(np.isnan(raw_b), np.inf, _wrap_distance(raw_b, 360)))
    else:
        m["en"] = np.full(1, np.inf)
    return {k: (v if len(v) else np.full(1, np.inf)) for k, v in m.items()}


ADMISSIBLE = {"face": 1e-6, "point_crop": 1e-6, "box_crop": 1e-6, "sides": 1e-3, "theta": 1e-3, "nn": 1e-6, "en": 1e-3}


def is_admissible(inp, crop, xlim, ylim, factor, offset):
    try:
        margins = admissibility(inp, crop, xlim, ylim, factor, offset)
    except ValueError:                                              # a sample cropped to one point: the en encoding has no neighbour
        return False
    return all((margins[k] >= bar).all() for k, bar in ADMISSIBLE.items())


# ---------------------------------------------------------------------------------------------------- samples
def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _yaw_quat(yaw, pitch=0.0, roll=0.0):
    cy, sy, cp, sp, cr, sr = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2), np.sin(roll / 2)
    return np.array([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy])


def _quat_mul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


SENSOR_YAWS = (0.0, 1.55, -1.56, 3.1, -3.05)           # roughly the five radars of the car: front, the two sides, the two rear corners
SENSOR_OFFSETS = ((3.4, 0.0, 0.5), (2.4, 0.8, 0.5), (2.4, -0.8, 0.5), (-0.56, 0.63, 0.5), (-0.56, -0.63, 0.5))


def draw_sample(rng, n_points, n_boxes, xlim=40.0, ylim=30.0, empty_chunk=None):
    """One sample in the layout of the module docstring (one sample's share of every array): an ego pose with a few degrees of
    pitch and roll, boxes drawn in the vehicle frame and moved to the global one (overlapping pairs with different labels, boxes
    wider than long, boxes without points, boxes beyond the crop), five sensor chunks whose rows are drawn in the vehicle frame
    (half of them inside boxes) and moved to the sensor's, three repeated timestamps per chunk.  Every value is a float64 that
    float32 holds exactly."""
    ego_q = _f32(_yaw_quat(rng.uniform(-np.pi, np.pi), np.radians(rng.uniform(-4, 4)), np.radians(rng.uniform(-4, 4))))
    ego_t = _f32([rng.uniform(300, 1800), rng.uniform(300, 1800), rng.uniform(-1, 1)])
    Re = rotation_matrices(ego_q)
    centers, sizes, quats, labels, npts = [], [], [], [], []
    for k in range(n_boxes):
        overlap = k % 7 == 3                                        # overlaps the box before it, another label
        if overlap:
            c = centers[-1] + np.array([rng.uniform(-0.6, 0.6), rng.uniform(-0.6, 0.6), 0.0])
        else:
            c = np.array([rng.uniform(-xlim - 12, xlim + 12), rng.uniform(-ylim - 10, ylim + 10), rng.uniform(0.3, 1.5)])
        l, w = rng.uniform(1.5, 9.0), rng.uniform(0.5, 2.6)
        if abs(l - w) < 0.1:
            l += 0.5
        if k % 5 == 1:                                              # a barrier: wider than long
            l, w = w, l
        centers.append(c)
        sizes.append([w, l, rng.uniform(0.8, 3.0)])
        quats.append(_yaw_quat(rng.uniform(-np.pi, np.pi), np.radians(rng.uniform(-1, 1)), np.radians(rng.uniform(-1, 1))))
        labels.append(int(labels[-1] % 10 + 1) if overlap else int(rng.integers(1, 11)))
        npts.append(0 if k % 6 == 2 else int(rng.integers(1, 40)))
    centers, quats = np.reshape(centers, (-1, 3)), np.reshape(quats, (-1, 4))
    box_center = _f32(centers @ Re.T + ego_t)
    box_rotation = _f32(np.array([_quat_mul(ego_q / np.linalg.norm(ego_q), q) for q in quats]).reshape(-1, 4))
    # rows in the vehicle frame: every other one inside a box with points
    pv = np.stack([rng.uniform(-xlim - 8, xlim + 8, n_points), rng.uniform(-ylim - 8, ylim + 8, n_points), rng.uniform(-0.3, 1.2, n_points)], 1)
    if n_boxes:
        for r in range(0, n_points, 2):
            k = int(rng.integers(0, n_boxes))
            u = np.array([rng.uniform(-0.55, 0.55) * sizes[k][1], rng.uniform(-0.55, 0.55) * sizes[k][0], 0.0])
            pv[r] = centers[k] + rotation_matrices(quats[k]) @ u
            pv[r, 2] = rng.uniform(-0.3, 1.2)
    cuts = np.sort(rng.integers(0, n_points + 1, size=4))
    ptr = np.concatenate(([0], cuts, [n_points]))
    if empty_chunk is not None:                                     # one of the first four chunks: the next one takes its rows
        ptr[empty_chunk + 1] = ptr[empty_chunk]
    points = np.zeros((19, n_points))
    rot, trans = [], []
    stamps = _f32([0.0, 0.0769, 0.1538])
    for c in range(5):
        q = _f32(_yaw_quat(SENSOR_YAWS[c] + rng.uniform(-0.02, 0.02), rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01)))
        t = _f32(np.array(SENSOR_OFFSETS[c]) + rng.uniform(-0.05, 0.05, 3))
        rot.append(q)
        trans.append(t)
        a, b = ptr[c], ptr[c + 1]
        points[:3, a:b] = (rotation_matrices(q).T @ (pv[a:b] - t).T)
        points[18, a:b] = stamps[rng.integers(0, 3, b - a)]
    points[3] = rng.integers(0, 8, n_points)
    points[4] = rng.integers(0, 200, n_points)
    points[5] = rng.uniform(-5, 30, n_points)
    points[6:10] = rng.uniform(-12, 12, (4, n_points))
    points[10:18] = rng.integers(0, 20, (8, n_points))
    return {"points": _f32(points), "chunk_ptr": ptr.astype(np.int64), "chunk_rotation": np.reshape(rot, (5, 4)),
            "chunk_translation": np.reshape(trans, (5, 3)), "box_center": box_center.reshape(-1, 3),
            "box_size": _f32(np.reshape(sizes, (-1, 3))), "box_rotation": box_rotation, "box_label": np.asarray(labels, dtype=np.int32),
            "box_points": np.asarray(npts, dtype=np.int32), "ego_translation": ego_t, "ego_rotation": ego_q}


def concat_samples(parts):
    """A batch from a list of one-sample dicts (``draw_sample``)."""
    out = {k: np.concatenate([p[k] for p in parts], axis=1 if k == "points" else 0)
           for k in ("points", "chunk_rotation", "chunk_translation", "box_center", "box_size", "box_rotation", "box_label", "box_points")}
    rows = np.cumsum([0] + [p["points"].shape[1] for p in parts])
    out["chunk_ptr"] = np.concatenate([p["chunk_ptr"][:-1] + r for p, r in zip(parts, rows)] + [rows[-1:]]).astype(np.int64)
    out["chunk_sample"] = np.concatenate([np.full(len(p["chunk_ptr"]) - 1, s) for s, p in enumerate(parts)]).astype(np.int32)
    out["box_ptr"] = np.cumsum([0] + [len(p["box_label"]) for p in parts]).astype(np.int64)
    out["ego_translation"] = np.stack([p["ego_translation"] for p in parts])
    out["ego_rotation"] = np.stack([p["ego_rotation"] for p in parts])
    return out


def take_samples(inp, samples):
    """The batch made of the given samples of ``inp``, in that order."""
    parts = []
    for s in samples:
        chunks = np.nonzero(np.asarray(inp["chunk_sample"]) == s)[0]
        a, b = inp["chunk_ptr"][chunks[0]], inp["chunk_ptr"][chunks[-1] + 1]
        ka, kb = inp["box_ptr"][s], inp["box_ptr"][s + 1]
        parts.append({"points": inp["points"][:, a:b], "chunk_ptr": inp["chunk_ptr"][chunks[0]:chunks[-1] + 2] - a,
                      "chunk_rotation": inp["chunk_rotation"][chunks], "chunk_translation": inp["chunk_translation"][chunks],
                      "box_center": inp["box_center"][ka:kb], "box_size": inp["box_size"][ka:kb], "box_rotation": inp["box_rotation"][ka:kb],
                      "box_label": inp["box_label"][ka:kb], "box_points": inp["box_points"][ka:kb],
                      "ego_translation": inp["ego_translation"][s], "ego_rotation": inp["ego_rotation"][s]})
    return concat_samples(parts)


def draw_admissible(seed, shapes, crop, xlim, ylim, factor, offset):
    """A batch whose every sample is admissible: sample s is drawn from generator seed + s, then seed + s + 1000, ... until it
    passes (samples do not interact).  ``shapes``: (n_points, n_boxes, empty_chunk) per sample.  -> (inputs, tries)."""
    parts, tries = [], 0
    for s, (n_points, n_boxes, empty_chunk) in enumerate(shapes):
        g = seed + s
        while True:
            tries += 1
            part = draw_sample(np.random.default_rng(g), n_points, n_boxes, xlim, ylim, empty_chunk)
            if is_admissible(concat_samples([part]), crop, xlim, ylim, factor, offset):
                break
            g += 1000
        parts.append(part)
    return concat_samples(parts), tries
