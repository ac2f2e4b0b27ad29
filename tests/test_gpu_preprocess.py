"""Frames from a sequence's detection table on the device (csrc/preprocess.hip through radargnn_amd.preprocessor / ops) against the
fixtures made by running the reference (tests/golden/preprocess_*.npz) and the numpy oracle (tests/preprocess_oracle.py).

Bars.  frame_ptr, X, rcs, timestamp, label, track, src_row and the keep decision are copies and comparisons: bit-exact.  The
compensated velocity is compared with the REFERENCE's values at |difference| <= 8 * 2^-52 * |vr_compensated| per component: the
device library's documented 4 ulp for double sin / cos plus 1 ulp for the host libm is <= 5 * 2^-52 (an ulp of a value <= 1 is at
most 2^-52), the two multiply roundings add <= 2^-52, the angle's add is the same IEEE operation on both sides; |cos|, |sin| <= 1
turns that into the bound relative to |v|.  Reasoned, not tuned; the worst measured ratio to the bar is recorded (MEASUREMENTS.md).
"""
import numpy as np
import pytest
import torch

import groundtruth_oracle as GO
import preprocess_oracle as O
from conftest import record_parity
from test_preprocess_oracle import FIXTURES, IDS, bits, fixture, kept_frames, oracle_run, runs

pytestmark = pytest.mark.gpu
V_BAR = 8 * 2.0 ** -52


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radargnn_amd import preprocessor
    return preprocessor


_TABLES = {}


def table_of(P, path):
    """(fixture, SequenceTable) -- uploaded once per fixture."""
    if path not in _TABLES:
        g = np.load(path)
        data = {k: g[k] for k in (*P.COLUMN_DTYPES, "track_id")}
        _TABLES[path] = (g, P.SequenceTable(data, g["scene_timestamps"], g["scene_ptr"]))
    return _TABLES[path]


def config(P, g, crop, m=None, **kw):
    return P.RadarScenesDatasetConfiguration(float(g["span"]), crop, {"front": float(g["front"]), "sides": float(g["sides"])},
                                             kw.get("aligned", False), kw.get("inv", "translation"), m is not None,
                                             None if m is None else {"num_clouds_per_sequence": m})


def tables(g):
    return g["yaw"].tolist(), g["label_map"].tolist()


def device_run(P, path, key, crop):
    g, table = table_of(P, path)
    batch, label, track, src_row = P.accumulate_frames(table, g[key + "_windows"], config(P, g, crop), *tables(g))
    cpu = lambda t: t.cpu().numpy()
    return dict(frame_ptr=cpu(batch.frame_ptr), sizes=batch.frame_sizes, X=cpu(batch.X), V=cpu(batch.V), rcs=cpu(batch.rcs),
                timestamp=cpu(batch.timestamp), label=cpu(label), track=cpu(track), src_row=cpu(src_row))


def v_ratio(got_v, ref_v, vc):
    """Worst |difference| / (bar * |vr_compensated|) over both components (0 where both are exactly equal)."""
    d = np.abs(got_v - ref_v)
    scale = V_BAR * np.abs(vc).reshape(-1, 1)
    return float(np.max(np.where(d == 0, 0.0, d / np.where(scale > 0, scale, np.finfo(np.float64).tiny)), initial=0.0))


# ---------------------------------------------------------------------------------------------- 1. fixtures and oracle
@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_matches_reference_fixtures(P, path):
    g, table = table_of(P, path)
    worst = 0.0
    for key, crop, _ in runs(g):
        got, ora = device_run(P, path, key, crop), oracle_run(g, key, crop)
        assert got["X"].dtype == np.float64 and got["label"].dtype == np.int32 and got["src_row"].dtype == np.int32
        assert np.array_equal(got["frame_ptr"], g[key + "_frame_ptr"]) and np.array_equal(got["sizes"], np.diff(g[key + "_frame_ptr"]))
        assert np.array_equal(got["src_row"], g[key + "_src_row"]), key              # the keep decision, NaN tests included
        for name in ("X", "rcs", "timestamp"):
            assert np.array_equal(bits(got[name]), bits(g[f"{key}_{name}"])), (key, name)
        assert np.array_equal(got["label"], g[key + "_label"].astype(np.int32))
        assert np.array_equal(got["track"], ora["track"]) and np.array_equal(got["track"], table.host["track"][got["src_row"]])
        if table.track_names is not None and len(table.track_names):
            names = np.where(got["track"] < 0, b"", table.track_names[np.maximum(got["track"], 0)])
            assert np.array_equal(names, g[key + "_track_id"])
        assert not np.isnan(got["V"]).any()
        vc = g["vr_compensated"][got["src_row"]].astype(np.float64)
        ratio = v_ratio(got["V"], g[key + "_V"], vc)
        print(f"[preprocess] {IDS[FIXTURES.index(path)]} {key}: V worst |d| / (8 * 2^-52 |v|) = {ratio:.3f}")
        worst = max(worst, ratio)
        assert ratio <= 1.0, (key, ratio)
    record_parity("preprocess_V_vs_reference_" + IDS[FIXTURES.index(path)], ratio_to_bar=worst)


# ---------------------------------------------------------------------------------------------- 2. repeatable, order of windows
def test_run_to_run_bits_and_permuted_windows(P):
    path = FIXTURES[IDS.index("seq_below")]
    g, table = table_of(P, path)
    cfg = config(P, g, True)
    windows = g["crop1_windows"]

    def run(w):
        batch, label, track, src = P.accumulate_frames(table, w, cfg, *tables(g))
        return [t.cpu().numpy() for t in (batch.frame_ptr, batch.X, batch.V, batch.rcs, batch.timestamp, label, track, src)]

    a, b = run(windows), run(windows)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    perm = np.random.default_rng(4).permutation(len(windows))
    c = run(windows[perm])
    ptr, ptr_c = a[0], c[0]
    assert np.array_equal(np.diff(ptr_c), np.diff(ptr)[perm])
    for u, v in zip(a[1:], c[1:]):
        want = np.concatenate([u[ptr[w]:ptr[w + 1]] for w in perm])
        assert want.tobytes() == v.tobytes()


# ---------------------------------------------------------------------------------------------- 3. an assembled cloud
@pytest.mark.parametrize("crop", [False, True])
def test_transform_of_an_assembled_cloud_equals_the_one_window_slice(P, crop):
    g = fixture("filter")
    key = "crop1" if crop else "crop0"
    table = O.load_table(g)
    rows, _ = O.gather(O.window_rows(g["scene_ptr"], g[key + "_windows"]))
    e = O.evaluate(table, rows, g["yaw"], O.label_values(g["label_map"]), crop, float(g["front"]), float(g["sides"]))
    pc = P.RadarPointCloud()
    pc.X_cc, pc.V_cc_compensated, pc.V_cc = e["X"], e["V"], e["V_cc"]
    pc.rcs, pc.timestamp, pc.label_id = e["rcs"].reshape(-1, 1), e["timestamp"].reshape(-1, 1), e["label"].reshape(-1, 1)
    pc.track_id = g["track_id"][rows]
    out = P.PointCloudProcessor.transform(config(P, g, crop), pc)
    assert out is pc
    for name, attr in (("X", "X_cc"), ("V", "V_cc_compensated"), ("V_cc", "V_cc"), ("rcs", "rcs"), ("timestamp", "timestamp"),
                       ("label", "label_id")):
        assert np.array_equal(bits(np.asarray(getattr(pc, attr)).reshape(g[f"{key}_{name}"].shape)), bits(g[f"{key}_{name}"])), name
    assert np.array_equal(pc.track_id, g[key + "_track_id"])
    with pytest.raises(ValueError, match="float32"):
        bad = P.RadarPointCloud()
        bad.X_cc, bad.V_cc_compensated, bad.label_id = np.array([[0.1, 0.2]]), np.zeros((1, 2)), np.zeros((1, 1))
        P.PointCloudProcessor.transform(config(P, g, crop), bad)


def test_create_point_cloud_frames_returns_every_frame(P):
    path = FIXTURES[IDS.index("seq_above")]
    g, table = table_of(P, path)
    for key, crop, m in runs(g):
        clouds = P.create_point_cloud_frames(table, config(P, g, crop, m), *tables(g))
        ptr = g[key + "_frame_ptr"]
        assert [len(c.X_cc) for c in clouds] == np.diff(ptr).tolist() and (np.diff(ptr) == 0).any() == any(len(c.X_cc) == 0 for c in clouds)
        cat = lambda attr, width: np.concatenate([np.asarray(getattr(c, attr), dtype=np.float64).reshape(-1, width) for c in clouds])
        assert np.array_equal(bits(cat("X_cc", 2)), bits(g[key + "_X"])) and np.array_equal(bits(cat("rcs", 1)[:, 0]), bits(g[key + "_rcs"]))
        assert np.array_equal(bits(cat("V_cc", 2)), bits(g[key + "_V_cc"]))          # gathered and computed on the host: numpy's
        assert np.array_equal(cat("label_id", 1)[:, 0], g[key + "_label"])
        assert np.array_equal(np.concatenate([c.track_id for c in clouds]), g[key + "_track_id"])
        assert clouds[0].X_seq is None and clouds[0].V_cc_compensated.shape == clouds[0].X_cc.shape


# ---------------------------------------------------------------------------------------------- 4. ids outside their tables
@pytest.mark.parametrize("which", ["sensor_id", "label_id"])
def test_id_outside_its_table_sets_the_status_bit_and_drops_only_that_row(P, which):
    from radargnn_amd import ops
    path = FIXTURES[IDS.index("rowcounts")]
    g, table = table_of(P, path)
    yaw, label_map = tables(g)
    n_table = len(yaw) if which == "sensor_id" else len(label_map)
    good = g["crop1_src_row"]
    victim = int(good[len(good) // 2])                                         # a row that survives, in a window of many rows
    data = {k: g[k].copy() for k in (*P.COLUMN_DTYPES, "track_id")}
    data[which][victim] = n_table                                              # the first id beyond the table
    broken = P.SequenceTable(data, g["scene_timestamps"], g["scene_ptr"])
    with pytest.raises(ValueError, match="RGNN_STATUS_PREPROCESS_BAD_ROW"):
        P.accumulate_frames(broken, g["crop1_windows"], config(P, g, True), yaw, label_map)
    win_rows = torch.from_numpy(broken.window_rows(g["crop1_windows"])).cuda()
    n_cap = int((win_rows[:, 1] - win_rows[:, 0]).sum())
    out = ops.accumulate_frames(broken.columns, win_rows, torch.tensor(yaw, dtype=torch.float64).cuda(),
                                torch.tensor(label_map, dtype=torch.int32).cuda(), True, float(g["front"]), float(g["sides"]), n_cap)
    torch.cuda.synchronize()
    assert int(out[-1].item()) == ops.STATUS_PREPROCESS_BAD_ROW
    n = int(out[0][-1].item())
    want = good[good != victim]                                                # every other row is written as usual
    assert n == len(want) and np.array_equal(out[7][:n].cpu().numpy(), want)
    keep = good != victim
    assert np.array_equal(bits(out[1][:n].cpu().numpy()), bits(g["crop1_X"][keep]))
    assert np.array_equal(bits(out[3][:n].cpu().numpy()), bits(g["crop1_rcs"][keep]))


# ---------------------------------------------------------------------------------------------- 5. table to graphs
@pytest.mark.parametrize("name,algo,aligned,inv,crop,m", [("seq_below", "knn", False, "translation", True, None),
                                                          ("seq_above", "radius", True, "none", False, 5)])
def test_graph_data_from_sequence_equals_the_per_frame_path(P, name, algo, aligned, inv, crop, m):
    from radargnn_amd.data import create_graph_data
    from radargnn_amd.graph_constructor.configs import GraphConstructionConfiguration
    from radargnn_amd.graph_constructor.graph import build_geometric_graph
    from radargnn_amd.groundtruth import GroundTruthCreator
    path = FIXTURES[IDS.index(name)]
    g, table = table_of(P, path)
    key = ("crop1" if crop else "crop0") + ("" if m is None else "_sub")
    graph_config = GraphConstructionConfiguration(algo, {"k": 5, "r": 6.0}, ["rcs", "velocity_vector", "time_index", "degree"],
                                                  ["relative_position"], "directed", "X")
    got = P.create_graph_data_from_sequence(table, graph_config, config(P, g, crop, m, aligned=aligned, inv=inv), *tables(g))
    ptr = g[key + "_frame_ptr"]
    frames = [(a, b) for a, b in zip(ptr[:-1], ptr[1:]) if b - a >= 2]
    assert len(frames) < len(ptr) - 1 or m is not None                        # the full run holds a frame of fewer than two points ...
    assert len(got) == len(frames)                                             # ... and it is absent
    keep, kept_ptr = kept_frames(g, key)
    ora = oracle_run(g, key, crop)
    assert GO.is_admissible(ora["X"][keep], ora["track"][keep].astype(np.int64), kept_ptr)
    for d, (a, b) in zip(got, frames):
        cloud = type("Cloud", (), dict(X_cc=g[key + "_X"][a:b], V_cc_compensated=g[key + "_V"][a:b], rcs=g[key + "_rcs"][a:b].reshape(-1, 1),
                                       timestamp=g[key + "_timestamp"][a:b].reshape(-1, 1), track_id=g[key + "_track_id"][a:b],
                                       label_id=g[key + "_label"][a:b].reshape(-1, 1)))()
        graph = build_geometric_graph(graph_config, cloud)
        boxes = GroundTruthCreator.create_2D_bounding_boxes(cloud, aligned, inv).cpu().numpy()
        want = create_graph_data(graph, GroundTruthCreator.get_class_indices(cloud), boxes, cloud)
        assert d.keys == want.keys
        for k in want.keys:
            u, v = getattr(d, k), getattr(want, k)
            assert u.is_cuda and u.dtype == v.dtype and u.shape == v.shape, (k, u.shape, v.shape)
            assert u.cpu().contiguous().numpy().tobytes() == v.contiguous().numpy().tobytes(), (k, a, b)
