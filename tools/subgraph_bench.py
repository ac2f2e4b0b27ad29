"""``subgraph`` (csrc/subgraph.hip) on the C2 batch -- 64 RadarScenes-shaped frames x 3000 points, the radius graph r = 1 with the
shipped feature lists (x: rcs, velocity_vector, time_index, degree; edge_attr: relative_position), y, pos and vel -- with a node
mask that keeps 0.8 of the points, beside the composition of torch ops that does the same: boolean indexing of every attribute, a
``cumsum`` relabelling of edge_index, ``bincount`` / ``cumsum`` for the offsets.  Both forms size their result on the device and
read it back (the new call 16 bytes once; the torch form inside every boolean indexing).
Per form: device events around `reps` calls, median (min .. max) of 5 windows, every shape warmed up first; the bytes the algorithm
needs (computed from the shapes, every value read once and every kept value written once) over the median, against the 8 TB/s of
the MI355X's HBM.  The two outputs are compared for equality before anything is timed.  Tools only.
    python tools/subgraph_bench.py [--reps 20] [--json out.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from radargnn_amd import frames as fr, synthetic
from radargnn_amd.data import Batch
from radargnn_amd.subgraph import subgraph

HBM_BYTES_PER_S = 8.0e12
NODE_KEYS, EDGE_KEYS = ("x", "y", "pos", "vel"), ("edge_attr",)


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


def c2_batch():
    settings = bench.c2_settings()
    frames = fr.FrameBatch.from_frames([synthetic.radarscenes_frame(i) for i in range(bench.FRAMES_PER_GPU)])
    g = fr.build_graphs(frames, settings)
    g.check()
    n = g.x.shape[0]
    gen = torch.Generator(device="cuda").manual_seed(0)
    y = torch.randn(n, 6, device="cuda", generator=gen)
    y[torch.rand(n, device="cuda", generator=gen) < 0.7, 1:] = float("nan")
    b = Batch(x=g.x, edge_index=g.edge_index, edge_attr=g.edge_attr, y=y, pos=frames.X.float(), vel=frames.V.float())
    b.ptr = frames.frame_ptr
    b.batch = torch.repeat_interleave(torch.arange(frames.num_frames, device="cuda"), frames.frame_ptr[1:] - frames.frame_ptr[:-1])
    return b


def torch_subgraph(b, keep):
    """the same part as torch ops (PyG's ``subgraph`` with relabelling, plus the offsets of a Batch)"""
    nb = b.ptr.numel() - 1
    s, t = b.edge_index
    keep_e = keep[s] & keep[t]
    new_id = torch.cumsum(keep, 0) - 1
    out = {"edge_index": new_id[b.edge_index[:, keep_e]], "batch": b.batch[keep]}
    for k in NODE_KEYS:
        out[k] = getattr(b, k)[keep]
    for k in EDGE_KEYS:
        out[k] = getattr(b, k)[keep_e]
    zero = torch.zeros(1, dtype=torch.int64, device=keep.device)
    out["ptr"] = torch.cat((zero, torch.cumsum(torch.bincount(out["batch"], minlength=nb), 0)))
    out["_edge_ptr"] = torch.cat((zero, torch.cumsum(torch.bincount(b.batch[s[keep_e]], minlength=nb), 0)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("subgraph_bench: no GPU visible (there is no CPU timing of a HIP path)")
    b = c2_batch()
    n, e, nb = b.x.shape[0], b.edge_index.shape[1], b.num_graphs
    keep = torch.rand(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) < 0.8

    # ---- the two forms agree before they are timed
    got, ref = subgraph(b, keep), torch_subgraph(b, keep)
    for k, r in ref.items():
        g = getattr(got, k)
        assert g.dtype == r.dtype and g.shape == r.shape, (k, g.dtype, g.shape, r.dtype, r.shape)
        assert torch.equal(g.contiguous().view(torch.uint8), r.contiguous().view(torch.uint8)), k
    n_out, e_out = got.x.shape[0], got.edge_index.shape[1]
    print(f"agreement: {len(ref)} tensors equal byte for byte; kept {n_out} of {n} nodes, {e_out} of {e} edges", flush=True)

    row_bytes = lambda keys: sum(getattr(b, k).shape[1] * getattr(b, k).element_size() for k in keys)
    # mask 1 B and batch 8 B per node, edge_index 16 B per edge, in; per kept node its rows in and out and batch out, per kept edge
    # its rows in and out and edge_index out; the offsets are noise
    nbytes = n * (1 + 8) + e * 16 + n_out * (2 * row_bytes(NODE_KEYS) + 8) + e_out * (2 * row_bytes(EDGE_KEYS) + 16)
    rows = []

    def row(name, f, reps):
        med, lo, hi = time_us(f, reps)
        rate = nbytes / (med * 1e-6)
        rows.append({"name": name, "us": med, "us_min_max": [lo, hi], "bytes": nbytes, "bytes_per_s": rate,
                     "share_of_hbm_peak": rate / HBM_BYTES_PER_S})
        print(f"{name:34s} {med:9.1f} us ({lo:.1f} .. {hi:.1f})  {nbytes / 1e6:8.1f} MB  {rate / 1e12:6.3f} TB/s = "
              f"{100 * rate / HBM_BYTES_PER_S:5.1f} % of 8 TB/s", flush=True)

    row("subgraph(batch, keep)", lambda: subgraph(b, keep), args.reps)
    row("torch composition", lambda: torch_subgraph(b, keep), args.reps)
    verdict = "below" if rows[0]["us"] < rows[1]["us"] else "NOT below"
    print(f"the new call's median is {verdict} the composition's ({rows[0]['us']:.1f} vs {rows[1]['us']:.1f} us)", flush=True)
    res = {"config": f"C2 batch: {nb} frames, {n} nodes, {e} edges; kept {n_out} nodes, {e_out} edges", "rows": rows}
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
