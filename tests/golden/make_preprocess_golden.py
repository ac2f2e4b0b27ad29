"""Writes tests/golden/preprocess_*.npz: detection tables and the frames the reference makes of them, produced by EXECUTING the
reference's own create_point_cloud_frames (preprocessor/radarscenes/dataset_creation.py:716-783) with its
concatenate_subsequent_scenes, SceneCollection.process (scene_collection.py) and PointCloudProcessor.transform, loaded from
/root/reference by file path; nothing of it is restated here.  The packages that are absent (ray, torch_geometric, radar_scenes,
matplotlib) and the reference modules out of scope are stubbed with MagicMock; radar_point_cloud.py, scene_collection.py and
dataset_creation.py are loaded for real.  Stand-ins supplied here: a Sequence (timestamps, get_scene, next_scene_after,
next_timestamp_after; Sequence.from_json patched to return it), scenes holding structured ``radar_data``, and get_mounting /
label_to_clabel built from ARBITRARY test tables (YAW, LABELS below -- not RadarScenes' values).  Runs only on the build machine; the
fixtures are committed.

Stored per fixture: the table's columns, track_id, scene_timestamps, scene_ptr, the test tables, span / front / sides; per run
(crop off / on, with and without num_clouds_per_sequence): the windows ([first scene, last scene], recorded from the scene lists the
reference collected), frame_ptr, and every frame's X_cc, V_cc_compensated, V_cc, rcs, timestamp, label_id, track_id back to back, plus
the source rows, carried through the spare column range_sc.
"""
import importlib.util
import os
import sys
import types
from types import SimpleNamespace
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import groundtruth_oracle as GO  # noqa: E402
import preprocess_oracle as PO  # noqa: E402

R = "/root/reference/src/gnnradarobjectdetection"
P = "gnnradarobjectdetection"
for name in (P, P + ".utils", P + ".preprocessor", P + ".preprocessor.radarscenes", P + ".graph_constructor"):
    m = types.ModuleType(name); m.__path__ = []; sys.modules[name] = m
for name in ("ray", "torch_geometric", "torch_geometric.data", "radar_scenes", "radar_scenes.sequence", "radar_scenes.sensors",
             "radar_scenes.coordinate_transformation", "radar_scenes.labels", "matplotlib", "matplotlib.pyplot",
             P + ".utils.radar_scenes_properties", P + ".utils.math", P + ".preprocessor.configs", P + ".preprocessor.bounding_box",
             P + ".preprocessor.radarscenes.configs", P + ".graph_constructor.graph"):
    sys.modules[name] = MagicMock()


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    return mod


load(P + ".preprocessor.radar_point_cloud", R + "/preprocessor/radar_point_cloud.py")
S = load(P + ".preprocessor.radarscenes.scene_collection", R + "/preprocessor/radarscenes/scene_collection.py")
D = load(P + ".preprocessor.radarscenes.dataset_creation", R + "/preprocessor/radarscenes/dataset_creation.py")

# arbitrary test tables: yaw per sensor id (0..4), reduced class per label id (0..11), -1 = no reduced class
YAW = np.array([0.0, -1.4835298641951802, -0.4363323129985824, 0.4363323129985824, 1.4835298641951802])
LABELS = np.array([0, 0, 1, 1, 2, -1, 3, 4, 4, -1, -1, 5], dtype=np.int32)
FRONT, SIDES = 100.0, 50.0

S.get_mounting = lambda s_id, json_path=None: {"yaw": float(YAW[int(s_id)])}
S.transform_detections_sequence_to_car = lambda x, y, odometry: (x, y)
S.ClassificationLabel = SimpleNamespace(
    label_to_clabel=lambda l: None if LABELS[int(l)] < 0 else SimpleNamespace(value=int(LABELS[int(l)])))

DTYPE = np.dtype([("timestamp", np.int64), ("sensor_id", np.uint8), ("range_sc", np.float32), ("azimuth_sc", np.float32),
                  ("rcs", np.float32), ("vr", np.float32), ("vr_compensated", np.float32), ("x_cc", np.float32), ("y_cc", np.float32),
                  ("x_seq", np.float32), ("y_seq", np.float32), ("uuid", "S8"), ("track_id", "S8"), ("label_id", np.uint8)])


class StandInSequence:
    def __init__(self, data, scene_ts, scene_ptr):
        self.timestamps = np.asarray(scene_ts, dtype=np.int64)
        self.scenes = [SimpleNamespace(timestamp=int(t), radar_data=data[a:b], odometry_data=None, index=i)
                       for i, (t, a, b) in enumerate(zip(scene_ts, scene_ptr[:-1], scene_ptr[1:]))]
        self.by_ts = {s.timestamp: s for s in self.scenes}

    def get_scene(self, t):
        return self.by_ts[int(t)]

    def next_timestamp_after(self, t):
        i = self.by_ts[int(t)].index + 1
        return None if i >= len(self.scenes) else self.scenes[i].timestamp

    def next_scene_after(self, t):
        i = self.by_ts[int(t)].index + 1
        return None if i >= len(self.scenes) else self.scenes[i]


def run_reference(data, scene_ts, scene_ptr, span, crop, m=None):
    seq = StandInSequence(data, scene_ts, scene_ptr)
    D.Sequence.from_json = lambda path: seq
    windows, made = [], []
    collect, transform = S.concatenate_subsequent_scenes, D.PointCloudProcessor.transform

    def collect_and_record(*a, **k):
        c = collect(*a, **k)
        windows.append((c.scenes[0].index, c.scenes[-1].index))
        return c

    def transform_and_record(cfg, pc):
        out = transform(cfg, pc)
        made.append(out)
        return out

    D.concatenate_subsequent_scenes = collect_and_record
    D.PointCloudProcessor.transform = staticmethod(transform_and_record)
    try:
        cfg = SimpleNamespace(time_per_point_cloud_frame=span, crop_point_cloud=crop, crop_settings={"front": FRONT, "sides": SIDES},
                              create_small_subset=m is not None, subset_settings={} if m is None else {"num_clouds_per_sequence": m})
        clouds = D.create_point_cloud_frames("unused", "unused", cfg)
    finally:
        D.concatenate_subsequent_scenes = collect
        D.PointCloudProcessor.transform = staticmethod(transform)
    picked = [next(i for i, c in enumerate(made) if c is pc) for pc in clouds]
    windows = np.array(windows, dtype=np.int64).reshape(-1, 2)[picked]
    cat = lambda name, width: np.concatenate([np.asarray(getattr(pc, name), dtype=np.float64).reshape(-1, width) for pc in clouds])
    rows = cat("range_sc", 1).reshape(-1)
    assert np.array_equal(rows, np.round(rows))
    return dict(windows=windows, frame_ptr=np.concatenate(([0], np.cumsum([len(pc.X_cc) for pc in clouds]))).astype(np.int64),
                X=cat("X_cc", 2), V=cat("V_cc_compensated", 2), V_cc=cat("V_cc", 2), rcs=cat("rcs", 1).reshape(-1),
                timestamp=cat("timestamp", 1).reshape(-1), label=cat("label_id", 1).reshape(-1),
                track_id=np.concatenate([np.asarray(pc.track_id, dtype="S8").reshape(-1) for pc in clouds]),
                src_row=rows.astype(np.int32))


def save(name, data, scene_ts, scene_ptr, span, subset=None):
    data = data.copy()
    data["range_sc"] = np.arange(len(data), dtype=np.float32)                  # the spare column carries the row number
    assert len(data) < 2 ** 24
    out = {k: data[k] for k in DTYPE.names if k not in ("x_seq", "y_seq", "uuid", "range_sc")}
    runs = [("crop0", False, None), ("crop1", True, None)]
    if subset is not None:
        runs += [("crop0_sub", False, subset), ("crop1_sub", True, subset)]
    for key, crop, m in runs:
        for k, v in run_reference(data, scene_ts, scene_ptr, span, crop, m).items():
            out[f"{key}_{k}"] = v
    np.savez_compressed(os.path.join(HERE, f"preprocess_{name}.npz"), scene_timestamps=np.asarray(scene_ts, dtype=np.int64),
                        scene_ptr=np.asarray(scene_ptr, dtype=np.int64), yaw=YAW, label_map=LABELS, front=FRONT, sides=SIDES, span=span,
                        subset=-1 if subset is None else subset, **out)
    print(name, "rows", len(data), "scenes", len(scene_ts), {k: len(out[k + "_windows"]) for k, _, _ in runs},
          {k: int(out[k + "_frame_ptr"][-1]) for k, _, _ in runs})
    return out


def random_rows(rng, n, ts):
    d = np.zeros(n, dtype=DTYPE)
    d["timestamp"] = ts
    d["sensor_id"] = rng.integers(1, 5, n)
    d["azimuth_sc"] = rng.uniform(-1.0, 1.0, n)
    d["rcs"] = rng.normal(-5, 10, n)
    d["vr"] = rng.normal(0, 5, n)
    d["vr_compensated"] = rng.normal(0, 5, n)
    d["x_cc"] = rng.uniform(-10, 120, n)
    d["y_cc"] = rng.uniform(-70, 70, n)
    d["label_id"] = rng.integers(0, 12, n)
    d["uuid"] = [b"u%06d" % i for i in rng.integers(0, 10 ** 6, n)]
    return d


def product_sides():
    """(span below, span at-or-above): two settings s with an exact microsecond count d = s * 1e6 whose float64 product d * 1e-6
    falls below s for the one and not below it for the other -- the comparison of scene_collection.py:213 on both sides."""
    below = above = None
    for tenth_ms in range(1000, 9999):
        s = tenth_ms / 10000
        d = np.int64(tenth_ms * 100)
        if float(repr(s)) * 1e6 != float(d):
            continue
        if d * 1e-6 < s and below is None:
            below = (s, int(d))
        if not d * 1e-6 < s and above is None:                   # (the double 1e-6 lies below 1e-6: the product never exceeds s)
            above = (s, int(d))
    return below, above


def sequence_case(name, seed, span, d_exact):
    """~200 scenes, ~5000 rows: tracked objects as moving blobs (so that the frames' objects pass groundtruth_oracle.is_admissible)
    plus background; in the first window a scene exactly d_exact us after the window's start; two gaps longer than the span in a row
    (a two-scene window); scenes without rows; a frame of one survivor."""
    for attempt in range(400):
        rng = np.random.default_rng(seed + 1000 * attempt)
        gaps = rng.integers(int(span * 1e6 / 18), int(span * 1e6 / 14), 199)        # ~16 scenes per window
        ts = np.concatenate(([1_600_000_000_000_000], 1_600_000_000_000_000 + np.cumsum(gaps))).astype(np.int64)
        k = int(np.searchsorted(ts - ts[0], d_exact))             # the scene nearest the span takes the exact place
        ts[k] = ts[0] + d_exact
        assert ts[k - 1] < ts[k] < ts[k + 1]
        big = 120                                                  # scenes big, big + 1, big + 2: gaps longer than the span
        ts[big + 1:] += int(span * 1e6) + 40000
        ts[big + 2:] += int(span * 1e6) + 90000
        windows = PO.plan_windows(ts, span)
        ends = set(windows[:, 1].tolist()) | set(windows[:, 0].tolist())
        assert (big + 1, big + 2) in [tuple(w) for w in windows.tolist()]
        empty = [s for s in (17, 18, 60, 150) if s not in ends]
        n_tracks = 6
        centre = np.stack((rng.uniform(15, 85, n_tracks), rng.uniform(-35, 35, n_tracks)), axis=1)
        drift = rng.normal(0, 0.002, (n_tracks, 2))
        turn = rng.uniform(0, np.pi, n_tracks)
        t_label = rng.choice([0, 2, 4, 6, 7, 11], n_tracks)
        parts = []
        for s, t in enumerate(ts):
            if s in empty:
                parts.append(np.zeros(0, dtype=DTYPE)); continue
            if s == big + 2:                                       # rows that all go: with scene big + 1 a frame of ONE survivor
                d = random_rows(rng, 9, t); d["label_id"] = 5; d["track_id"] = b""
                parts.append(d); continue
            if s == big + 1:
                d = random_rows(rng, 7, t); d["label_id"] = 9; d["track_id"] = b""
                d["label_id"][3] = 2; d["x_cc"][3] = 40.0; d["y_cc"][3] = -3.0
                parts.append(d); continue
            n_bg = int(rng.integers(14, 24))
            d = random_rows(rng, n_bg, t)
            d["track_id"] = b""
            obj = []
            for o in range(n_tracks):
                m = int(rng.integers(0, 3))
                if m == 0:
                    continue
                local = rng.normal(0, 1, (m, 2)) * [2.2, 0.6]
                rot = np.array([[np.cos(turn[o]), -np.sin(turn[o])], [np.sin(turn[o]), np.cos(turn[o])]])
                p = centre[o] + drift[o] * (s * 65.0) + local @ rot.T   # (drift per scene)
                e = random_rows(rng, m, t)
                e["x_cc"], e["y_cc"], e["label_id"], e["track_id"] = p[:, 0], p[:, 1], t_label[o], b"trk%d" % (7 * o + 3)
                obj.append(e)
            d = np.concatenate([d] + obj)
            parts.append(d[rng.permutation(len(d))])
        data = np.concatenate(parts)
        scene_ptr = np.concatenate(([0], np.cumsum([len(p) for p in parts]))).astype(np.int64)
        # a few invalid velocities in the random part
        bad = rng.choice(len(data), 40, replace=False)
        data["vr_compensated"][bad[:20]] = np.nan
        data["vr"][bad[20:]] = np.nan
        data["vr_compensated"][scene_ptr[big + 1] + 3] = 1.5      # (the one survivor stays one)
        shared = windows[1:, 0]
        if not (np.diff(scene_ptr)[shared] > 0).all():
            continue
        # admissible objects in every frame of two or more points, both crops (tests/groundtruth_oracle.py)
        table = {k: data[k] for k in DTYPE.names}
        uniq, inv = np.unique(data["track_id"], return_inverse=True)
        table["track"] = inv.astype(np.int32) - 1
        ok = True
        for crop in (False, True):
            acc = PO.accumulate(table, PO.window_rows(scene_ptr, windows), YAW, PO.label_values(LABELS), crop, FRONT, SIDES)
            sizes = np.diff(acc["frame_ptr"])
            keep = np.repeat(sizes >= 2, sizes)
            ptr = np.concatenate(([0], np.cumsum(sizes[sizes >= 2])))
            ok = ok and GO.is_admissible(acc["X"][keep], acc["track"][keep].astype(np.int64), ptr)
        if ok:
            print(name, "attempt", attempt, "windows", len(windows))
            return save(name, data, ts, scene_ptr, span, subset=5)
    raise RuntimeError("no admissible draw")


def rowcount_case():
    """Every scene more than the span after the one before: window k is scenes (k, k + 1).  Rows per window 0, 1, 63, 64, 65, 255,
    256, 257, 1000, then a window from which nothing survives and one with exactly one survivor."""
    rng = np.random.default_rng(77)
    sizes = [0, 0, 1, 62, 2, 63, 192, 64, 193, 807, 40, 30, 25]
    ts = 1_000_000 + 900_000 * np.arange(len(sizes), dtype=np.int64)
    parts = []
    for s, (n, t) in enumerate(zip(sizes, ts)):
        d = random_rows(rng, n, t)
        d["x_cc"] = rng.uniform(1, 99, n); d["y_cc"] = rng.uniform(-49, 49, n)
        d["label_id"] = rng.choice([0, 1, 2, 3, 4, 6, 7, 8, 11], n)
        d["track_id"] = [b"" if v else b"t%d" % rng.integers(0, 9) for v in rng.integers(0, 2, n)]
        if s >= 10:
            d["label_id"] = 10                                     # no reduced class: the whole scene goes
        if s == 11:
            d["vr_compensated"][::2] = np.nan                      # ... half of it for two reasons
        if s == 12:
            d["label_id"][11] = 4                                  # the one survivor of the last window
        parts.append(d)
    data = np.concatenate(parts)
    return save("rowcounts", data, ts, np.concatenate(([0], np.cumsum(sizes))), 0.5)


def filter_case():
    rng = np.random.default_rng(78)
    f32 = np.float32
    up = lambda v: np.nextafter(f32(v), f32(np.inf))
    dn = lambda v: np.nextafter(f32(v), f32(-np.inf))
    nan, inf = f32("nan"), f32("inf")
    # (x, y, azimuth, vr, vr_compensated, label, sensor)
    special = [(FRONT, 1, .1, 1, 1, 0, 1), (0.0, 1, .1, 1, 1, 0, 2), (-0.0, 1, .1, 1, 1, 0, 3), (5, SIDES, .1, 1, 1, 0, 4),
               (5, -SIDES, .1, 1, 1, 0, 0), (up(FRONT), 1, .1, 1, 1, 0, 1), (dn(0.0), 1, .1, 1, 1, 0, 1), (5, up(SIDES), .1, 1, 1, 0, 1),
               (5, dn(-SIDES), .1, 1, 1, 0, 1), (nan, 1, .1, 1, 1, 0, 1), (5, nan, .1, 1, 1, 0, 1), (5, 1, .1, 1, nan, 0, 1),
               (5, 1, nan, 1, 1, 0, 1), (5, 1, inf, 1, 1, 0, 2), (5, 1, -inf, 1, 1, 0, 3), (5, 1, .1, nan, 1, 0, 1),
               (5, 1, .1, 1, 1, 5, 1), (5, 1, .1, 1, 1, 9, 1), (5, 1, .1, 1, 1, 10, 1), (up(FRONT), 1, .1, 1, 1, 5, 1),
               (5, up(SIDES), .1, 1, nan, 0, 1), (dn(0.0), 1, nan, 1, 1, 9, 1), (5, 1, 0.0, 1, inf, 0, 0), (5, 1, 0.0, 1, -inf, 0, 0),
               (5, 1, .1, inf, 1, 0, 1), (inf, 1, .1, 1, 1, 0, 1), (-inf, 1, .1, 1, 1, 0, 1), (5, 1, .1, 1, 0.0, 0, 1)]
    n = 300
    sizes = [60, 100, 140]
    ts = np.repeat(np.array([5_000_000, 5_100_000, 5_200_000], dtype=np.int64), sizes)
    d = random_rows(rng, n, ts)
    d["sensor_id"] = rng.integers(0, 5, n)
    d["track_id"] = b""
    place = rng.choice(n, len(special), replace=False)
    for r, (x, y, az, vr, vc, lab, sen) in zip(place, special):
        d["x_cc"][r], d["y_cc"][r], d["azimuth_sc"][r], d["vr"][r], d["vr_compensated"][r] = x, y, az, vr, vc
        d["label_id"][r], d["sensor_id"][r] = lab, sen
    return save("filter", d, np.array([5_000_000, 5_100_000, 5_200_000]), np.concatenate(([0], np.cumsum(sizes))), 0.5)


def one_scene_case():
    rng = np.random.default_rng(79)
    d = random_rows(rng, 20, 42_000_000)
    d["track_id"] = b""
    return save("one_scene", d, np.array([42_000_000]), np.array([0, 20]), 0.5, subset=3)


if __name__ == "__main__":
    below, above = product_sides()
    print("span whose exact gap's product falls below it:", below, "; not below:", above)
    assert below is not None and above is not None
    sequence_case("seq_below", 11, *below)
    sequence_case("seq_above", 12, *above)
    rowcount_case()
    filter_case()
    one_scene_case()
