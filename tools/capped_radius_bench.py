"""ops.radius_graph_capped beside ops.radius_graph and ops.knn_graph on the same resident batches: the C2 batch (64 RadarScenes-shaped
frames x 3000 points, r = 1) and the most crowded configuration bench.py --full builds (C5: one 100 000-point cloud, r = 1), at
k = 8, 16 and 32 -- and at k = 128 >= the longest row where the batch has no longer one, where the capped search does the radius
search's work and the ratio of the two is the price of its protocol.  Per graph: the search time (grid build to finished rows,
one host read each for the radius forms), the edge count, and the time of one eager model forward on that graph (graph side
included: CSR by target, edge attributes in target order, the model).  Device events around `reps` calls, median of 5 windows,
every shape warmed up first.  Tools only.
    python tools/capped_radius_bench.py [--reps 50] [--json out.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from radargnn_amd import frames as fr, ops, synthetic

CAPS = (8, 16, 32)


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


def forward_us(model, settings, batch, reps):
    """One eager forward of the model on the graph `settings` builds from `batch` (HotPath's model half) -> (E, median, min, max)."""
    hot = fr.HotPath(model, settings)
    _, _, g = hot(batch)
    g.check()
    return (int(g.edge_index.shape[1]),) + time_us(lambda: hot._model(g), reps)


def config(name, model, base, frames, reps):
    batch = fr.FrameBatch.from_frames(frames)
    basis = batch.X if base.distance_definition == "X" else torch.cat((batch.X, batch.V), dim=1)
    P, r, biggest = batch.frame_ptr, base.r, int(batch.frame_sizes.max())
    rowptr, _, _ = ops.radius_graph(basis, P, r)
    longest = int((rowptr[1:] - rowptr[:-1]).max().item())
    out = {"config": name, "points": batch.num_points, "frames": batch.num_frames, "r": r, "longest_row": longest, "rows": []}
    feats = dict(node_features=base.node_features, edge_features=base.edge_features, edge_mode=base.edge_mode,
                 distance_definition=base.distance_definition)

    def row(graph, k, search, settings):
        e, fwd, lo, hi = forward_us(model, settings, batch, max(reps // 2, 2))
        s, slo, shi = time_us(search, reps)
        out["rows"].append({"graph": graph, "k": k, "edges": e, "search_us": s, "search_us_min_max": [slo, shi], "forward_us": fwd,
                            "forward_us_min_max": [lo, hi]})
        print(f"{name:4s} {graph:14s} k={str(k):>4s}  E={e:9d}  search {s:9.1f} us ({slo:.1f} .. {shi:.1f})  forward {fwd:9.1f} us ({lo:.1f} .. {hi:.1f})",
              flush=True)

    row("radius", None, lambda: ops.radius_graph(basis, P, r), fr.GraphSettings(algorithm="radius", r=r, **feats))
    for k in CAPS + ((ops.RADIUS_CAP_MAX,) if longest <= ops.RADIUS_CAP_MAX else ()):
        row("radius_capped", k, lambda: ops.radius_graph_capped(basis, P, r, k, max_frame_points=0),
            fr.GraphSettings(algorithm="radius", r=r, max_neighbors=k, **feats))
    for k in CAPS:
        row("knn", k, lambda: ops.knn_graph(basis, P, k, max_frame_points=biggest), fr.GraphSettings(algorithm="knn", k=k, **feats))
    by = {(x["graph"], x["k"]): x for x in out["rows"]}
    if ("radius_capped", ops.RADIUS_CAP_MAX) in by:
        a, b = by[("radius_capped", ops.RADIUS_CAP_MAX)], by[("radius", None)]
        assert a["edges"] == b["edges"]
        out["capped_over_radius_at_k_beyond_longest_row"] = a["search_us"] / b["search_us"]
        print(f"{name}: capped / radius search at k = {ops.RADIUS_CAP_MAX} >= longest row {longest}: {a['search_us'] / b['search_us']:.3f}", flush=True)
    else:
        out["capped_over_radius_at_k_beyond_longest_row"] = None
        print(f"{name}: longest row {longest} > {ops.RADIUS_CAP_MAX}: no cap reaches it, the equal-work ratio is not measured here", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", choices=["C2", "C5"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("capped_radius_bench: no GPU visible (there is no CPU timing of a HIP path)")
    res = []
    if args.only in (None, "C2"):
        res.append(config("C2", bench.c2_model().cuda(), bench.c2_settings(),
                          [synthetic.radarscenes_frame(i) for i in range(bench.FRAMES_PER_GPU)], args.reps))
    if args.only in (None, "C5"):
        c5 = fr.GraphSettings(algorithm="radius", r=1.0, node_features=("rcs", "velocity_vector_length", "time_index", "degree"),
                              edge_features=("point_pair_features",))
        res.append(config("C5", bench.shipped_model([224, 224, 224, 128, 64, 32], 6, node_dim=4, edge_dim=4).cuda(), c5,
                          [synthetic.stress_cloud()], args.reps))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
