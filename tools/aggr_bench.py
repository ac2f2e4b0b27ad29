"""Forward and backward launches of the fused aggregation M[t] = aggr_e(Q[s_e] + W_e a_e) per aggregation on the C2 graph
(tools only; MEASUREMENTS.md section 4.2).

    python tools/aggr_bench.py [-r rounds] [-d 224] mean min var std

64 RadarScenes-shaped frames of 3000 points, radius 1 m, grid-cell visiting order, the chunk table the layers use; Q, W_e [d, 8], the
edge attributes and dM are random.  Per aggregation: median and extremes over the rounds of the mean of 5 back-to-back calls of
ops.mpnn_aggregate (forward) and of ops.mpnn_aggregate_bwd (backward: all its launches), device events.  RGNN_LIB=path selects
another build of the library (the parent's, for the yardstick `mean`)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from radargnn_amd import frames as fr, ops, synthetic
from radargnn_amd.gnn.mpnn_layers import TargetCSR


def main():
    argv = sys.argv[1:]
    rounds, d, names = 9, 224, []
    while argv:
        a = argv.pop(0)
        if a == "-r":
            rounds = int(argv.pop(0))
        elif a == "-d":
            d = int(argv.pop(0))
        else:
            names.append(a)
    frames = [synthetic.radarscenes_frame(i) for i in range(64)]
    g = fr.build_graphs(fr.FrameBatch.from_frames(frames), fr.GraphSettings(algorithm="radius", r=1.0))
    csr = TargetCSR(g.edge_index, g.x.shape[0], order=g.cell_order, symmetric=True)
    n, e = g.x.shape[0], csr.num_edges
    torch.manual_seed(0)
    Q = torch.randn(n, d, device="cuda")
    We = torch.randn(d, 8, device="cuda") * 0.3
    ea = torch.randn(e, 8, device="cuda").relu_()
    dM = torch.randn(n, d, device="cuda")
    scale = (1.0 / csr.in_degree().clamp(min=1.0)).view(-1).contiguous()
    source_csr, chunks = csr.source_csr(), csr.chunks

    def fwd(aggr):
        return ops.mpnn_aggregate(None, None, Q, We, ea, csr.rowptr, csr.src, aggr, node_order=csr.order, chunks=chunks)

    def bwd(aggr):
        return ops.mpnn_aggregate_bwd(dM, Q, We, ea, csr.rowptr, csr.src, aggr, source_csr, node_order=csr.order,
                                      target_scale=scale if aggr == "mean" else None)

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {(a, w): [] for a in names for w in ("fwd", "bwd")}
    for a in names:                                          # every shape once before any timed window
        fwd(a), bwd(a)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for a in names:                                      # the aggregations alternate inside a round
            for w, fn in (("fwd", fwd), ("bwd", bwd)):
                fn(a)
                e0.record()
                for _ in range(5):
                    fn(a)
                e1.record()
                torch.cuda.synchronize()
                times[(a, w)].append(e0.elapsed_time(e1) / 5)
    print(f"aggr_bench: lib={os.environ.get('RGNN_LIB', 'in-tree')} N={n} E={e} D={d} rounds={rounds}  gather volume {4 * e * d / 1e9:.2f} GB")
    for a in names:
        for w in ("fwd", "bwd"):
            t = sorted(times[(a, w)])
            print(f"    {a:5s} {w}: median {t[len(t) // 2] * 1e3:8.1f} us   min {t[0] * 1e3:8.1f}   max {t[-1] * 1e3:8.1f}")


if __name__ == "__main__":
    main()
