"""Frames per second of ``radargnn_amd.inference.Predictor`` against the hand loop it replaces (one
``model(batch.x, batch.edge_index, batch.edge_attr)`` plus ``ops.softmax_rows`` per loader batch), on the same loader in the same
process.

    python tools/predict_bench.py [--frames 512] [--repeats 7] [--out FILE.json]

Data: ``--frames`` graphs of ``synthetic.radarscenes_frame`` (3000 points each) through the graph build of C2 (radius graph,
r = 1 m; bench.c2_settings / bench.c2_model, train mode as the reference leaves it), stored as ``Data`` in a ``DataLoader`` with
``batch_size=1`` (evaluate.py:40).  Variants, each a whole pass over the loader ending in a device synchronise:

    hand loop, device      model + softmax_rows per batch, the six outputs kept as device tensors
    hand loop, host        the same with ``.cpu().numpy()`` per output and batch (the reference's, and INTEGRATION.md's, loop)
    Predictor g = 1, 8, 64 ``Predictor(model, loader, verbose=False, graphs_per_step=g).predict()``
    Predictor g = 64, host the same with ``to_host=True``

One warm-up pass per variant, then ``--repeats`` rounds that run the variants one after the other (alternating, so drift of
the shared host hits all alike); median and min .. max of the rounds, in frames per second.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def build_loader(n_frames: int):
    import bench
    from radargnn_amd import data as D, frames as fr, synthetic
    settings = bench.c2_settings()
    graphs = []
    for i in range(n_frames):
        frame = synthetic.radarscenes_frame(i)
        g = fr.build_graphs(fr.FrameBatch.from_frames([frame]), settings)
        n = g.x.shape[0]
        gen = torch.Generator().manual_seed(i)
        y = torch.cat((torch.randint(0, 6, (n, 1), generator=gen).float(), torch.randn(n, 5, generator=gen)), 1)
        graphs.append(D.Data(x=g.x.cpu(), edge_index=g.edge_index.cpu(), edge_attr=g.edge_attr.cpu(), y=y,
                             pos=torch.as_tensor(frame.X, dtype=torch.float32), vel=torch.as_tensor(frame.V, dtype=torch.float32)))
    loader = D.DataLoader(graphs, batch_size=1)
    loader.store                                        # the split goes to HBM once, outside every timed pass
    return loader, sum(g.num_nodes for g in graphs), sum(g.num_edges for g in graphs)


def hand_loop(model, loader, to_host: bool):
    from radargnn_amd import ops
    out = [[] for _ in range(6)]
    keep = (lambda t: t.cpu().numpy()) if to_host else (lambda t: t)
    with torch.no_grad():
        for batch in loader:
            cls, bb = model(batch.x, batch.edge_index, batch.edge_attr)
            prob = ops.softmax_rows(cls)
            for lst, t in zip(out, (prob, bb, batch.y[:, 0], batch.y[:, 1:], batch.pos, batch.vel)):
                lst.append(keep(t))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predict_bench needs the GPU: a host run measures nothing")
    import bench
    from radargnn_amd.inference import Predictor
    loader, nodes, edges = build_loader(args.frames)
    model = bench.c2_model().cuda()                     # train mode: the reference never calls .eval()

    def predictor(g, to_host=False):
        return lambda: Predictor(model, loader, verbose=False, graphs_per_step=g, to_host=to_host).predict()

    variants = [("hand loop, device", lambda: hand_loop(model, loader, False)),
                ("hand loop, host", lambda: hand_loop(model, loader, True)),
                ("Predictor graphs_per_step=1", predictor(1)),
                ("Predictor graphs_per_step=8", predictor(8)),
                ("Predictor graphs_per_step=64", predictor(64)),
                ("Predictor graphs_per_step=64, to_host", predictor(64, True))]
    for _, fn in variants:                              # every shape of the timed passes has run once
        fn()
    torch.cuda.synchronize()
    rates = {name: [] for name, _ in variants}
    for _ in range(args.repeats):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            rates[name].append(args.frames / (time.perf_counter() - t0))
    result = {"tool": "predict_bench", "frames": args.frames, "nodes": nodes, "edges": edges, "repeats": args.repeats,
              "device": torch.cuda.get_device_name(0), "frames_per_s": {}}
    for name, r in rates.items():
        result["frames_per_s"][name] = {"median": round(statistics.median(r), 1), "min": round(min(r), 1), "max": round(max(r), 1)}
    med = lambda name: result["frames_per_s"][name]["median"]
    result["ratio_to_hand_loop_device"] = {f"g={g}": round(med(f"Predictor graphs_per_step={g}") / med("hand loop, device"), 2)
                                           for g in (1, 8, 64)}
    result["ratio_host_g64_to_hand_loop_host"] = round(med("Predictor graphs_per_step=64, to_host") / med("hand loop, host"), 2)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
