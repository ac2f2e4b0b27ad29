"""Batched DBSCAN on the C2 cloud (64 RadarScenes-shaped frames x 3000 points, eps = 1, min_samples = 4) beside the radius search it
follows and beside scikit-learn on the host:
  (a) the label launch alone (ops.dbscan_labels on a resident CSR), with the search (ops.radius_graph at r = eps, its host read
      included) as its yardstick: the labels stage moves 4 (N + E) bytes once, so it should not cost more than the search;
  (b) clustering.dbscan_frames end to end (search + labels + the status read);
  (c) sklearn.cluster.DBSCAN(algorithm="kd_tree") frame by frame on the host (wall clock, one pass), labels compared entry for entry.
Also a chain of 24 576 points at min_samples = 2 (one frame at the cap, one cluster: the deepest union-find trees) as the label
launch's worst case.
Device events around `reps` calls, median of 5 windows (min .. max), every shape warmed up first.  Tools only.
    python tools/dbscan_bench.py [--reps 50] [--json out.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from radargnn_amd import clustering, frames as fr, ops, synthetic

EPS, MIN_SAMPLES = 1.0, 4


def time_us(f, reps):
    f(); f(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(5):
        e0.record()
        for _ in range(reps):
            f()
        e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1) / reps)
    ts.sort()
    return ts[2] * 1e3, ts[0] * 1e3, ts[4] * 1e3


def measure(name, X, P, reps, min_samples=MIN_SAMPLES):
    rowptr, col, _ = ops.radius_graph(X, P, EPS, want_edge_index=False)
    n, e = X.shape[0], col.numel()
    out = {"case": name, "points": n, "frames": P.numel() - 1, "edges": e, "eps": EPS, "min_samples": min_samples}
    status = torch.zeros(1, dtype=torch.int32, device=X.device)
    for key, f in (("search_us", lambda: ops.radius_graph(X, P, EPS, want_edge_index=False)),
                   ("labels_us", lambda: ops.dbscan_labels(rowptr, col, P, min_samples, status=status)),
                   ("dbscan_frames_us", lambda: clustering.dbscan_frames(X, P, EPS, min_samples))):
        med, lo, hi = time_us(f, reps)
        out[key], out[key + "_min_max"] = med, [lo, hi]
        print(f"{name:6s} {key:18s} {med:9.1f} us ({lo:.1f} .. {hi:.1f})", flush=True)
    out["labels_over_search"] = out["labels_us"] / out["search_us"]
    out["labels_bytes"] = 4 * (n + 1 + e) + 5 * n
    out["labels_gb_per_s"] = out["labels_bytes"] / out["labels_us"] * 1e-3
    got = clustering.dbscan_frames(X, P, EPS, min_samples)
    out["clusters"] = int(got.num_clusters.sum().item())
    print(f"{name:6s} N = {n}, E = {e}, clusters = {out['clusters']}; labels / search = {out['labels_over_search']:.3f}; "
          f"labels stage {out['labels_gb_per_s']:.1f} GB/s of its {out['labels_bytes']} compulsory bytes", flush=True)
    from sklearn.cluster import DBSCAN
    Xh, Ph, lab = X.cpu().numpy(), P.cpu().numpy(), got.labels.cpu().numpy()
    t0 = time.perf_counter()
    want = [DBSCAN(eps=EPS, min_samples=min_samples, algorithm="kd_tree").fit(Xh[a:b]).labels_ for a, b in zip(Ph[:-1], Ph[1:])]
    out["sklearn_kd_tree_us"] = (time.perf_counter() - t0) * 1e6
    out["labels_equal_sklearn"] = bool(np.array_equal(np.concatenate(want), lab))
    out["sklearn_over_dbscan_frames"] = out["sklearn_kd_tree_us"] / out["dbscan_frames_us"]
    print(f"{name:6s} sklearn kd_tree on the host, frame by frame: {out['sklearn_kd_tree_us']:.0f} us "
          f"({out['sklearn_over_dbscan_frames']:.0f} x dbscan_frames); labels equal: {out['labels_equal_sklearn']}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dbscan_bench: no GPU visible (there is no CPU timing of a HIP path)")
    batch = fr.FrameBatch.from_frames([synthetic.radarscenes_frame(i) for i in range(bench.FRAMES_PER_GPU)])
    res = [measure("C2", batch.X, batch.frame_ptr, args.reps)]
    cap = ops.dbscan_max_frame_points()
    chain = torch.stack((torch.arange(cap, dtype=torch.float64) * EPS, torch.zeros(cap, dtype=torch.float64)), dim=1).cuda()
    # min_samples 2: every point of the chain is core and the whole frame is one cluster (one tree over 24 576 rows)
    res.append(measure("chain", chain, torch.tensor([0, cap], dtype=torch.int64).cuda(), args.reps, min_samples=2))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
