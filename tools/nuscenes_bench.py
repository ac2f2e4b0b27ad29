"""Wall time of the nuScenes sample stage for 64 fixture-shaped samples (the three samples of tests/golden/nuscenes_inflated.npz
repeated): ``create_graph_data_from_samples`` with and without the graph build, and the numpy oracle on the same input on the same
machine.  Prints one JSON line.  A record, not a pass mark (MEASUREMENTS.md "nuScenes samples").

    python tools/nuscenes_bench.py [--samples 64] [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import nuscenes_oracle as O  # noqa: E402
from radargnn_amd import nuscenes as N  # noqa: E402
from radargnn_amd.graph_constructor.configs import GraphConstructionConfiguration  # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return statistics.median(out) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mode", default="en")
    a = ap.parse_args()
    g = np.load(os.path.join(REPO, "tests", "golden", "nuscenes_inflated.npz"))
    inp = O.take_samples({k: g[k] for k in O.INPUT_KEYS}, [s % 3 for s in range(a.samples)])
    crop, xlim, ylim, factor, offset = bool(g["crop"]), float(g["xlim"]), float(g["ylim"]), float(g["wlh_factor"]), float(g["wlh_offset"])
    cfg = N.NuScenesDatasetConfiguration(crop_point_cloud=crop, crop_settings={"x": xlim, "y": ylim}, wlh_factor=factor, wlh_offset=offset,
                                         bb_invariance=a.mode)
    graph_config = GraphConstructionConfiguration("knn", {"k": 5, "r": 6.0}, ["rcs", "velocity_vector", "time_index", "degree"],
                                                  ["relative_position"], "directed", "X")
    samples = N.NuScenesSamples(**inp)

    def stages():
        batch, _, _ = N.sample_point_clouds(samples, cfg)
        boxes = N.prepare_boxes(samples, cfg)
        return N.label_points(batch.X, batch.frame_ptr, boxes, a.mode, offset)

    full = lambda: N.create_graph_data_from_samples(samples, graph_config, cfg)
    full(), stages()                                             # first calls: library load, allocator
    t = time.perf_counter()
    O.create(inp, crop, xlim, ylim, factor, offset, modes=(a.mode,))
    oracle_ms = (time.perf_counter() - t) * 1e3
    print(json.dumps({"samples": a.samples, "rows": int(inp["points"].shape[1]), "boxes": int(len(inp["box_label"])), "mode": a.mode,
                      "graph_data_ms": round(timed(full, a.reps), 3), "stages_only_ms": round(timed(stages, a.reps), 3),
                      "numpy_oracle_ms": round(oracle_ms, 3), "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
