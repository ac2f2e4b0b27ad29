"""Time the trainer's two loops with and without grouped steps (gnn/trainer.py: ``valid_graphs_per_step``,
``train_batches_per_step``) on a synthetic resident dataset at the reference's loader batch size.  A measurement for
MEASUREMENTS.md, not the headline metric (that is bench.py).

    python tools/trainer_group_bench.py [--graphs 60] [--epochs 5] [--ungrouped-only]

Dataset: ``--graphs`` RadarScenes-shaped frames from ``radargnn_amd.synthetic`` as radius graphs (bench.py's C2 settings), once
with about 500 and once with about 3000 points per frame; loader ``batch_size = 5``; the shipped model widths (bench.c2_model).
Per size: one validation epoch at ``valid_graphs_per_step`` 0 and 64 and one training epoch at ``train_batches_per_step`` 1 and
12, each 3 warm-up epochs and then the median of ``--epochs`` (at least 5) timed ones.  ``--ungrouped-only`` times the two ungrouped
rows through ``Trainer(config, model)`` alone, so the same file also runs on a commit whose Trainer has no grouped steps: the
package and ``bench`` are imported from the working directory first, then from this file's repository.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from radargnn_amd import data, frames as fr, synthetic
from radargnn_amd.gnn.configs import TrainingConfig
from radargnn_amd.gnn.trainer import Trainer
from radargnn_amd.optim import FusedAdam

SIZES = {"500": dict(n_clusters=6, pts_per_cluster=35, n_clutter=290), "3000": dict(n_clusters=40, pts_per_cluster=35, n_clutter=1600)}
WARMUP, BATCH_SIZE = 3, 5


def dataset(n_graphs, shape):
    settings = bench.c2_settings()
    gen = torch.Generator().manual_seed(0)
    graphs = []
    for i in range(n_graphs):
        g = fr.build_graphs(fr.FrameBatch.from_frames([synthetic.radarscenes_frame(i, **shape)]), settings)
        n = g.x.shape[0]
        label = torch.randint(0, 6, (n, 1), generator=gen).float()
        y = torch.cat((label, torch.randn(n, 5, generator=gen)), 1)               # graph_batch.y: label | box
        graphs.append(data.Data(x=g.x.cpu(), edge_index=g.edge_index.cpu(), edge_attr=g.edge_attr.cpu(), y=y))
    return graphs


def median_epoch_ms(run, epochs):
    for _ in range(WARMUP):
        run()
    times = []
    for _ in range(epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=60)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--ungrouped-only", action="store_true")
    args = ap.parse_args()
    epochs = max(5, args.epochs)
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = TrainingConfig("radarscenes", 1e-4, 1, BATCH_SIZE, False, 5)
    result = {"tool": "trainer_group_bench", "graphs": args.graphs, "batch_size": BATCH_SIZE, "warmup_epochs": WARMUP,
              "timed_epochs": epochs, "unit": "ms per epoch (median)", "rows": {}}
    rows = [("valid", 0), ("train", 1)] if args.ungrouped_only else [("valid", 0), ("valid", 64), ("train", 1), ("train", 12)]
    for size, shape in SIZES.items():
        graphs = dataset(args.graphs, shape)
        loader = data.DataLoader(graphs, batch_size=BATCH_SIZE, shuffle=False, device="cuda")
        points = sum(g.x.shape[0] for g in graphs) / len(graphs)
        for loop, group in rows:
            torch.manual_seed(0)
            model = bench.c2_model().cuda().train()
            kw = {} if args.ungrouped_only else ({"valid_graphs_per_step": group} if loop == "valid" else {"train_batches_per_step": group})
            trainer = Trainer(cfg, model, **kw)
            w_train, w_valid = trainer.class_weight_tensors(dev)
            if loop == "valid":
                run = lambda: trainer._validate_epoch(loader, dev, w_valid)
            else:
                opt = FusedAdam(model.parameters(), lr=cfg.learning_rate, weight_decay=cfg.regularization_strength)
                run = lambda: trainer._train_epoch(loader, dev, opt, w_train)
            ms = median_epoch_ms(run, epochs)
            result["rows"][f"{loop}_{size}pts_group{group}"] = {"ms_per_epoch": round(ms, 3), "loader_batches": len(loader),
                                                                "points_per_frame": round(points),
                                                                "frames_per_s": round(args.graphs / ms * 1e3, 1)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
