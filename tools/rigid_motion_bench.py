"""The rigid-motion launches (csrc/transform.hip) on the C2 batch -- 64 RadarScenes-shaped frames x 3000 points, the radius graph
r = 1 with the shipped feature lists (x: rcs, velocity_vector, time_index, degree; edge_attr: relative_position), rotated boxes
with bb_invariance "none" -- beside a composition of torch ops that does the same float64 arithmetic:
    nodes   rgnn_rigid_graph_nodes alone (outputs allocated and copied beforehand), and its torch composition
    edges   rgnn_rigid_graph_edges alone, and its torch composition
    call    transforms.transform_graphs as a user calls it (the copies of x, y and edge_attr included)
    frames  transforms.transform_frames (float64 X and V)
Per launch: device events around `reps` calls, median (min .. max) of 5 windows, every shape warmed up first; the bytes the
algorithm needs (computed from the shapes below, every moving value read once and written once) over the median, against the
8 TB/s of the MI355X's HBM.  The outputs of the two forms are compared (1 ulp32) before anything is timed.  Tools only.
    python tools/rigid_motion_bench.py [--reps 50] [--json out.json]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from radargnn_amd import frames as fr, ops, synthetic, transforms as T
from radargnn_amd.data import Batch

HBM_BYTES_PER_S = 8.0e12


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
    pos = frames.X.float()
    box = torch.cat((pos + torch.randn(n, 2, device="cuda", generator=gen), torch.rand(n, 2, device="cuda", generator=gen) * 5 + 0.5,
                     torch.rand(n, 1, device="cuda", generator=gen) * 3.14), dim=1)
    box[torch.rand(n, device="cuda", generator=gen) < 0.7] = float("nan")
    y = torch.cat((torch.randint(0, 6, (n, 1), device="cuda", generator=gen).float(), box), dim=1)
    b = Batch(x=g.x, edge_index=g.edge_index, edge_attr=g.edge_attr, y=y, pos=pos, vel=frames.V.float())
    b.ptr = frames.frame_ptr
    b.batch = torch.repeat_interleave(torch.arange(frames.num_frames, device="cuda"), frames.frame_ptr[1:] - frames.frame_ptr[:-1])
    return settings, frames, b


def torch_nodes(b, m, vcol):
    """the node launch as torch ops: float64 from the stored float32, one rounding at the end"""
    a = m.angle[b.batch]
    c, s, t = torch.cos(a), torch.sin(a), m.shift[b.batch]
    rot = lambda q: torch.stack((c * q[:, 0] - s * q[:, 1], s * q[:, 0] + c * q[:, 1]), dim=1)
    pos = (rot(b.pos.double()) + t).float()
    vel = rot(b.vel.double()).float()
    x = b.x.clone()
    x[:, vcol:vcol + 2] = rot(b.x[:, vcol:vcol + 2].double()).float()
    y = b.y.clone()
    y[:, 1:3] = (rot(b.y[:, 1:3].double()) + t).float()
    th = torch.fmod(b.y[:, 5].double() + a, math.pi)
    th = torch.where(th < 0, th + math.pi, th)
    y[:, 5] = th.float()
    return pos, vel, x, y


def torch_edges(b, m):
    a = m.angle[b.batch[b.edge_index[0]]]
    c, s = torch.cos(a), torch.sin(a)
    q = b.edge_attr.double()
    return torch.stack((c * q[:, 0] - s * q[:, 1], s * q[:, 0] + c * q[:, 1]), dim=1).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rigid_motion_bench: no GPU visible (there is no CPU timing of a HIP path)")
    settings, frames, b = c2_batch()
    n, e, nb = b.x.shape[0], b.edge_index.shape[1], b.num_graphs
    m = T.RigidMotion.random(nb, math.pi, 10.0, generator=torch.Generator(device="cuda").manual_seed(1))
    plan = dict(node_features=list(settings.node_features), edge_features=list(settings.edge_features), edge_mode=settings.edge_mode,
                aligned=False, bb_invariance="none")
    vcol = list(settings.node_features).index("velocity_vector")
    assert list(settings.node_features)[:vcol] == ["rcs"] and list(settings.edge_features) == ["relative_position"]

    # ---- the two forms agree before they are timed
    out = T.transform_graphs(b, m, **plan)
    ref = dict(zip(("pos", "vel", "x", "y"), torch_nodes(b, m, vcol)), edge_attr=torch_edges(b, m))
    for k, r in ref.items():
        got = getattr(out, k)
        assert bool((torch.isnan(got) == torch.isnan(r)).all()), k
        d = torch.nan_to_num(got.double() - r.double()).abs()
        if k == "y":                       # theta is an angle mod pi (the torch form leaves out the float32(pi) -> 0 rule)
            d[:, 5] = torch.minimum(d[:, 5], (math.pi - d[:, 5]).abs())
        ulp = (torch.nextafter(r.abs(), torch.full_like(r, float("inf"))) - r.abs()).double()
        worst = float(torch.nan_to_num(d / ulp).max())
        print(f"agreement {k}: worst {worst:.2f} ulp32", flush=True)
        assert worst <= 1.0 or (k == "y" and float(d[:, 5].max()) <= 1e-6), k

    # ---- the launches alone
    arr_n, n_n = ops._codes(plan["node_features"], ops.NODE_FEATURE_CODES, "node ")
    arr_e, n_e = ops._codes(plan["edge_features"], ops.EDGE_FEATURE_CODES, "")
    P, S, lib = ops._ptr, ops._stream, ops.lib
    pos_o, vel_o, x_o, y_o, ea_o = torch.empty_like(b.pos), torch.empty_like(b.vel), b.x.clone(), b.y.clone(), b.edge_attr.clone()

    def nodes():
        ops.check(lib.rgnn_rigid_graph_nodes(P(b.pos), P(b.vel), P(b.x), b.x.shape[1], arr_n, n_n, P(b.y), 6, 5, 0, P(b.batch), n, nb,
                                             P(m.angle), P(m.shift), P(pos_o), P(vel_o), P(x_o), b.x.shape[1], P(y_o), 6, S()))

    def edges():
        ops.check(lib.rgnn_rigid_graph_edges(P(b.edge_attr), 2, arr_e, n_e, 0, P(b.edge_index), e, P(b.batch), n, nb, P(m.angle),
                                             P(b.pos), P(b.vel), P(ea_o), 2, S()))

    boxes = int((~torch.isnan(b.y[:, 1])).sum())
    # batch 8; pos, vel, x.velocity_vector: 8 in + 8 out each; y: the first box column of every row (4), of box rows c0 c1 theta in + out
    node_bytes = n * (8 + 3 * 16 + 4) + boxes * (8 + 12)
    # edge_index both rows 16, batch[i] 8, the 2-vector 8 in + 8 out
    edge_bytes = e * (16 + 8 + 16)
    frame_bytes = frames.num_points * 64
    rows = []

    def row(name, f, nbytes, reps):
        med, lo, hi = time_us(f, reps)
        rate = None if nbytes is None else nbytes / (med * 1e-6)
        rows.append({"name": name, "us": med, "us_min_max": [lo, hi], "bytes": nbytes, "bytes_per_s": rate,
                     "share_of_hbm_peak": None if rate is None else rate / HBM_BYTES_PER_S})
        tail = "" if rate is None else f"  {nbytes / 1e6:8.1f} MB  {rate / 1e12:6.3f} TB/s = {100 * rate / HBM_BYTES_PER_S:5.1f} % of 8 TB/s"
        print(f"{name:34s} {med:9.1f} us ({lo:.1f} .. {hi:.1f}){tail}", flush=True)

    row("nodes: rgnn_rigid_graph_nodes", nodes, node_bytes, args.reps)
    row("nodes: torch composition", lambda: torch_nodes(b, m, vcol), node_bytes, max(args.reps // 5, 2))
    row("edges: rgnn_rigid_graph_edges", edges, edge_bytes, args.reps)
    row("edges: torch composition", lambda: torch_edges(b, m), edge_bytes, max(args.reps // 5, 2))
    row("call: transform_graphs", lambda: T.transform_graphs(b, m, **plan), None, args.reps)
    mf = T.RigidMotion(m.angle, m.shift, rotates=True)
    row("frames: transform_frames", lambda: T.transform_frames(frames, mf), frame_bytes, args.reps)
    res = {"config": f"C2 batch: {nb} frames, {n} nodes, {e} edges, {boxes} box rows", "rows": rows}
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
