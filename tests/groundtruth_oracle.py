"""Float64 numpy oracle of the ground-truth box targets (radargnn_amd/groundtruth.py, csrc/groundtruth.hip), written from the
description of the reference's GroundTruthCreator.create_2D_bounding_boxes, not from its code: its own monotone-chain hull, the
rectangle from the projections directly (no trigonometric detour), one loop per object.  Pinned to reference-generated fixtures
by tests/test_groundtruth_oracle.py; the GPU tests compare against it where no fixture exists (fuzz, hand vectors).

Also the admissibility filter shared by the fixture maker and the fuzz test: inputs on which two implementations may
legitimately disagree (two rectangles of nearly equal area, l ~ w, an angle on a wrap point, two nearest neighbours at nearly the
same distance) are rejected when the clouds are DRAWN, so the tests compare every case they hold.
"""
import numpy as np

INVARIANCE_CODES = {"none": 0, "translation": 1, "en": 2}


class DegenerateObject(ValueError):
    pass


def monotone_chain(pts):
    """Indices of the strictly convex hull, counter-clockwise from the lowest (x, y) point (Andrew's monotone chain)."""
    order = sorted(range(len(pts)), key=lambda i: (pts[i][0], pts[i][1], i))
    uniq = [order[0]]
    for i in order[1:]:
        if pts[i][0] != pts[uniq[-1]][0] or pts[i][1] != pts[uniq[-1]][1]:
            uniq.append(i)
    if len(uniq) < 3:
        return uniq

    def cross(o, a, b):
        return (pts[a][0] - pts[o][0]) * (pts[b][1] - pts[o][1]) - (pts[a][1] - pts[o][1]) * (pts[b][0] - pts[o][0])

    def half(seq):
        out = []
        for i in seq:
            while len(out) >= 2 and cross(out[-2], out[-1], i) <= 0:
                out.pop()
            out.append(i)
        return out

    lower, upper = half(uniq), half(uniq[::-1])
    return lower[:-1] + upper[:-1]


def edge_rectangles(pts, hull):
    """Per hull edge k: (area, ux, uy, min_p, len_p, min_o, len_o) of the rectangle flush with it."""
    h = pts[hull]
    out = []
    for k in range(len(hull)):
        p0, p1 = h[k], h[(k + 1) % len(hull)]
        dis = np.sqrt((p0[0] - p1[0]) ** 2 + (p0[1] - p1[1]) ** 2)
        ux, uy = (p1[0] - p0[0]) / dis, (p1[1] - p0[1]) / dis
        dp = ux * h[:, 0] + uy * h[:, 1]
        do = -uy * h[:, 0] + ux * h[:, 1]
        len_p, len_o = dp.max() - dp.min(), do.max() - do.min()
        out.append((len_p * len_o, ux, uy, dp.min(), len_p, do.min(), len_o))
    return out


def _fold(theta):
    if theta < 0:
        theta = 180 + theta
    if theta >= 180:
        theta = theta - 180
    return theta


def object_rect(pts, aligned):
    """[cx, cy, l, w, theta in degrees 0..180) of one object's points (rows ascending)."""
    m = len(pts)
    if aligned:
        if m == 1:
            return np.array([pts[0, 0], pts[0, 1], 0.5, 0.5, 0.0])
        x0, x1, y0, y1 = pts[:, 0].min(), pts[:, 0].max(), pts[:, 1].min(), pts[:, 1].max()
        return np.array([(((x0 + x0) + x1) + x1) / 4, (((y0 + y1) + y0) + y1) / 4, abs(x0 - x1), abs(y0 - y1), 0.0])
    if m == 1:
        return np.array([pts[0, 0], pts[0, 1], 0.5, 0.5, 0.0])
    if m == 2:
        v = pts[1] - pts[0]
        nrm = np.sqrt(v[0] * v[0] + v[1] * v[1])
        if not nrm > 0:
            raise DegenerateObject("two coincident points")
        c = (pts[0] + pts[1]) / 2
        return np.array([c[0], c[1], nrm, 0.5, _fold(np.arctan2(v[1] / nrm, v[0] / nrm) * 180 / np.pi)])
    hull = monotone_chain(pts)
    if len(hull) < 3:
        raise DegenerateObject("hull without area")
    rects = edge_rectangles(pts, hull)
    area, ux, uy, min_p, len_p, min_o, len_o = min(rects, key=lambda r: r[0])      # the first minimum: lowest hull position
    if not area > 0:
        raise DegenerateObject("hull without area")
    cp, co = min_p + len_p / 2, min_o + len_o / 2
    cx, cy = cp * ux + co * (-uy), cp * uy + co * ux
    if len_p >= len_o:
        l, w, theta = len_p, len_o, np.arctan2(uy, ux)
    else:
        l, w, theta = len_o, len_p, np.arctan2(ux, -uy)
    return np.array([cx, cy, l, w, _fold(theta * 180 / np.pi)])


def _round5(x):
    return np.round(x, 5)


def en_angles(p, q, xr, yr, theta):
    """(d, angle nn -> centre in degrees, angle nn -> long side in degrees [0, 180), and both before wrapping)."""
    v = q - p
    vn = np.sqrt(v[0] * v[0] + v[1] * v[1])
    th_nn = np.arctan2(v[1] / vn, v[0] / vn) * 180 / np.pi
    t = np.tan((theta * np.pi) / 180)
    dn = np.sqrt(1.0 + t * t)
    raw_a = np.arctan2(t / dn, 1.0 / dn) * 180 / np.pi - th_nn
    a = _round5(raw_a)
    if a < 0:
        a = 360 + a
    if a >= 180:
        a = a - 180
    d = np.sqrt(xr * xr + yr * yr)
    b, raw_b = 0.0, None
    if d != 0:
        raw_b = np.arctan2(yr / d, xr / d) * 180 / np.pi - th_nn
        b = _round5(raw_b)
        if b < 0:
            b = 360 + b
    return d, b, a, raw_b, raw_a


def nearest_in_frames(pos, frame_ptr):
    """(index of the nearest other point of the frame, relative gap between the nearest and the second nearest distance)."""
    n = len(pos)
    nn, gap = np.full(n, -1, dtype=np.int64), np.full(n, np.inf)
    for a, b in zip(frame_ptr[:-1], frame_ptr[1:]):
        if b - a < 2:
            continue
        p = pos[a:b]
        d2 = (p[:, None, 0] - p[None, :, 0]) ** 2 + (p[:, None, 1] - p[None, :, 1]) ** 2
        np.fill_diagonal(d2, np.inf)
        nn[a:b] = a + d2.argmin(1)
        if b - a > 2:
            s = np.sqrt(np.sort(d2, axis=1)[:, :2])
            gap[a:b] = (s[:, 1] - s[:, 0]) / s[:, 1]
    return nn, gap


def objects(object_id, frame_ptr):
    """The objects in (frame, id) order: a list of ascending row arrays."""
    out = []
    for a, b in zip(frame_ptr[:-1], frame_ptr[1:]):
        ids = object_id[a:b]
        for i in np.unique(ids[ids >= 0]):
            out.append(a + np.nonzero(ids == i)[0])
    return out


def create_boxes(pos, object_id, frame_ptr, aligned, invariance):
    """-> (boxes float64 [N, 4|5] with NaN background rows, rect float64 [n_obj, 5]).  Raises DegenerateObject."""
    pos = np.asarray(pos, dtype=np.float64)
    inv = INVARIANCE_CODES[invariance] if not aligned else 0
    out = np.full((len(pos), 4 if aligned else 5), np.nan)
    objs = objects(np.asarray(object_id), frame_ptr)
    rects = np.full((len(objs), 5), np.nan)
    nn = nearest_in_frames(pos, frame_ptr)[0] if inv == 2 else None
    for o, rows in enumerate(objs):
        pts = pos[rows]
        m = len(rows)
        cx, cy, l, w, theta = rects[o] = object_rect(pts, aligned)
        for r in rows:
            px, py = pos[r]
            if aligned:
                out[r] = [0.0, 0.0, l, w] if m == 1 else [cx - px, cy - py, l, w]
            elif m == 1:
                out[r] = [px, py, 0.5, 0.5, 0.0] if inv == 0 else [0.0, 0.0, 0.5, 0.5, 0.0]
            else:
                xr, yr = cx - px, cy - py
                if inv == 0:
                    out[r] = [cx, cy, l, w, (theta * np.pi) / 180] if m == 2 else [px + xr, py + yr, l, w, (theta * np.pi) / 180]
                elif inv == 1:
                    out[r] = [xr, yr, l, w, (theta * np.pi) / 180]
                else:
                    d, b, a, _, _ = en_angles(pos[r], pos[nn[r]], xr, yr, theta)
                    out[r] = [d, (b * np.pi) / 180, l, w, (a * np.pi) / 180]
    return out, rects


# ---------------------------------------------------------------------------------------------------- admissibility
def _wrap_distance(x, period):
    """Distance of x (degrees) to the nearest multiple of `period`."""
    r = np.mod(x, period)
    return min(r, period - r)


def admissibility(pos, object_id, frame_ptr):
    """The margins of a cloud, per object: dict of arrays [n_obj] (inf where a margin does not apply):
      area   relative excess area of the best rectangle of ANOTHER orientation (direction differs by > 1e-6 rad modulo 90 deg)
      lw     (l - w) / l
      theta  degrees from theta to 0 / 180
      en     degrees from either en angle (before rounding) to its wrap point (multiples of 360; 180 for the direction angle)
      nn     relative gap between nearest and second-nearest neighbour distance, over the object's points."""
    pos = np.asarray(pos, dtype=np.float64)
    objs = objects(np.asarray(object_id), frame_ptr)
    nn, gap = nearest_in_frames(pos, frame_ptr)
    out = {k: np.full(len(objs), np.inf) for k in ("area", "lw", "theta", "en", "nn")}
    for o, rows in enumerate(objs):
        pts = pos[rows]
        if len(rows) >= 2:
            out["nn"][o] = gap[rows].min()
        if len(rows) < 2:
            continue
        cx, cy, l, w, theta = object_rect(pts, False)
        out["theta"][o] = min(theta, 180 - theta)
        if len(rows) >= 3:
            out["lw"][o] = (l - w) / l
            rects = edge_rectangles(pts, monotone_chain(pts))
            best = min(rects, key=lambda r: r[0])
            ang = np.arctan2(best[2], best[1])
            for r in rects:
                d = np.mod(np.arctan2(r[2], r[1]) - ang, np.pi / 2)
                if min(d, np.pi / 2 - d) > 1e-6:
                    out["area"][o] = min(out["area"][o], (r[0] - best[0]) / best[0])
        for r in rows:
            if nn[r] < 0:
                continue
            _, _, _, raw_b, raw_a = en_angles(pos[r], pos[nn[r]], cx - pos[r, 0], cy - pos[r, 1], theta)
            m = _wrap_distance(raw_a, 180)
            if raw_b is not None:
                m = min(m, _wrap_distance(raw_b, 360))
            out["en"][o] = min(out["en"][o], m)
    return out


ADMISSIBLE = {"area": 1e-6, "lw": 1e-3, "theta": 1e-3, "en": 1e-3, "nn": 1e-6}


def is_admissible(pos, object_id, frame_ptr):
    try:
        margins = admissibility(pos, object_id, frame_ptr)
    except DegenerateObject:
        return False
    return all((margins[k] >= bar).all() for k, bar in ADMISSIBLE.items())


# ---------------------------------------------------------------------------------------------------- clouds
def draw_cloud(rng, sizes, n_background, extent=60.0, labels=None):
    """One frame: objects of the given sizes (elongated, randomly turned blobs), background points, rows shuffled, non-dense ids.
    Coordinates are float64 values that float32 holds exactly (RadarScenes stores float32).  -> (pos [n, 2], object_id [n])."""
    pts, ids = [], []
    if labels is None:
        labels = rng.choice(np.arange(1, 4 * len(sizes) + 4), size=len(sizes), replace=False)
    for size, label in zip(sizes, labels):
        c = rng.uniform(-extent, extent, size=2)
        ang = rng.uniform(0, np.pi)
        rot = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        local = rng.normal(size=(size, 2)) * np.array([rng.uniform(1.5, 4.0), rng.uniform(0.3, 1.0)])
        pts.append(local @ rot.T + c)
        ids.append(np.full(size, label))
    pts.append(rng.uniform(-extent - 20, extent + 20, size=(n_background, 2)))
    ids.append(np.full(n_background, -1))
    pos, ids = np.concatenate(pts), np.concatenate(ids)
    perm = rng.permutation(len(pos))
    return pos[perm].astype(np.float32).astype(np.float64), ids[perm].astype(np.int64)


def draw_admissible(seed, frames, n_background, labels=None):
    """A batch whose every frame is admissible: frame f is drawn from generator seed + f, then seed + f + 1000, ... until it
    passes (frames do not interact: neighbours are searched inside a frame).  `frames`: a list of object-size lists; `labels`: the
    object ids per frame (default: drawn, non-dense).  -> (pos, object_id, frame_ptr, tries)."""
    parts, tries = [], 0
    for f, sizes in enumerate(frames):
        s = seed + f
        while True:
            tries += 1
            pos, oid = draw_cloud(np.random.default_rng(s), sizes, n_background, labels=None if labels is None else labels[f])
            if is_admissible(pos, oid, np.array([0, len(pos)])):
                break
            s += 1000
        parts.append((pos, oid))
    ptr = np.concatenate(([0], np.cumsum([len(p) for p, _ in parts]))).astype(np.int64)
    return np.concatenate([p for p, _ in parts]), np.concatenate([i for _, i in parts]), ptr, tries
