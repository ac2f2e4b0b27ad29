"""numpy restatement of the reference's frame accumulation -- create_point_cloud_frames, concatenate_subsequent_scenes,
SceneCollection.process, PointCloudProcessor.transform (preprocessor/radarscenes/dataset_creation.py:159-184,716-783,
scene_collection.py:36-156,185-230) -- vectorised over the rows of all windows at once (no per-point loop), float64 like the
reference.  Pinned against fixtures produced by running the reference (tests/golden/make_preprocess_golden.py) in
tests/test_preprocess_oracle.py; shares no code with radargnn_amd.preprocessor.

A table is a dict of the RadarScenes columns (timestamp int64, sensor_id / label_id uint8, azimuth_sc, rcs, vr, vr_compensated,
x_cc, y_cc float32, track int32 with -1 = background); ``label_values``: float64 per label_id, NaN = no reduced class.
"""
import numpy as np


def plan_windows(ts, span):
    """[first scene, last scene] per frame: from scene i the frame runs to the first later scene j with
    (ts[j] - ts[i]) * 1e-6 >= span (float64, as scene_collection.py:213 evaluates it), at least to i + 1, at most to the end."""
    ts = np.asarray(ts, dtype=np.int64)
    out, i, last = [], 0, len(ts) - 1
    while True:
        beyond = np.nonzero(~((ts[i + 1:] - ts[i]) * 1e-6 < span))[0]
        j = min(i + 1 + int(beyond[0]), last) if len(beyond) else last
        out.append((i, j))
        if j == last:
            return np.array(out, dtype=np.int64).reshape(-1, 2)
        i = j


def subset(windows, m):
    return windows[np.floor(np.linspace(0, len(windows) - 1, m)).astype(int)]


def window_rows(scene_ptr, windows):
    scene_ptr = np.asarray(scene_ptr, dtype=np.int64)
    return np.stack((scene_ptr[windows[:, 0]], scene_ptr[windows[:, 1] + 1]), axis=1)


def gather(win_rows):
    """(table row of every row of every window, in window order; window of each)."""
    sizes = win_rows[:, 1] - win_rows[:, 0]
    window = np.repeat(np.arange(len(win_rows)), sizes)
    starts = np.concatenate(([0], np.cumsum(sizes)))[:-1]
    rows = np.arange(sizes.sum()) - np.repeat(starts, sizes) + np.repeat(win_rows[:, 0], sizes)
    return rows.astype(np.int64), window


def evaluate(table, rows, yaw, label_values, crop, front, sides):
    """Per gathered row: the widened values, both velocities and the keep decision in the reference's order of tests."""
    f64 = lambda name: table[name][rows].astype(np.float64)
    x, y = f64("x_cc"), f64("y_cc")
    angle = f64("azimuth_sc") + np.asarray(yaw, dtype=np.float64)[table["sensor_id"][rows]]
    with np.errstate(invalid="ignore"):
        c, s = np.cos(angle), np.sin(angle)
        vr, vc = f64("vr"), f64("vr_compensated")
        V_cc = np.stack((vr * c, vr * s), axis=1)
        V = np.stack((vc * c, vc * s), axis=1)
        label = np.asarray(label_values, dtype=np.float64)[table["label_id"][rows]]
        keep = np.ones(len(rows), dtype=bool)
        if crop:
            keep &= ~((np.abs(y) > sides) | (x > front) | (x < 0))
    keep &= ~np.isnan(label)
    keep &= ~(np.isnan(V[:, 0]) | np.isnan(V[:, 1]))
    return dict(X=np.stack((x, y), axis=1), V=V, V_cc=V_cc, rcs=f64("rcs"), timestamp=f64("timestamp"), label=label,
                track=table["track"][rows], keep=keep)


def accumulate(table, win_rows, yaw, label_values, crop, front, sides):
    """-> dict: frame_ptr int64 [W + 1]; X, V (compensated), V_cc f64 [N, 2]; rcs, timestamp f64 [N]; label, track, src_row int32."""
    rows, window = gather(np.asarray(win_rows, dtype=np.int64))
    e = evaluate(table, rows, yaw, label_values, crop, front, sides)
    k = e.pop("keep")
    out = {name: v[k] for name, v in e.items()}
    out["label"] = out["label"].astype(np.int32)
    out["src_row"] = rows[k].astype(np.int32)
    out["frame_ptr"] = np.concatenate(([0], np.cumsum(np.bincount(window[k], minlength=len(win_rows))))).astype(np.int64)
    return out


def label_values(label_map):
    """int table with -1 = drop -> the float64 values the reference stores (NaN for a label without reduced class)."""
    m = np.asarray(label_map, dtype=np.float64)
    return np.where(m < 0, np.nan, m)


def load_table(g):
    """The table of a fixture: columns in their stored dtypes + ``track`` (rank of the track id among the distinct ids, b'' = -1)."""
    names = ("timestamp", "sensor_id", "azimuth_sc", "rcs", "vr", "vr_compensated", "x_cc", "y_cc", "label_id")
    table = {k: g[k] for k in names}
    uniq, inv = np.unique(g["track_id"], return_inverse=True)
    track = inv.reshape(-1).astype(np.int32)
    if len(uniq) and uniq[0] == b"":
        track -= 1
    table["track"] = track
    return table
