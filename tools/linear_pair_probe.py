"""Gate for ops.linear_pair: a conv layer's source term and isolated-row update as ONE grid against the two launches, on the shapes of
the C2 step's second conv layer (K = 224; 133 516 listed rows at N = 464; 58 484 listed rows at N = 224 with bias and column
statistics; the BatchNorm-apply table + ReLU on the A1 operand of both), in one process, interleaved blocks.
    python tools/linear_pair_probe.py [--blocks 7] [--reps 20] [--layer 2|3|4] [--out file.json]
Every variant is captured once as a HIP graph of `reps` repetitions (no host time between the launches, as in the captured step)
and a block is one replay of it; the blocks of the variants alternate.  Variants: `two` = the two launches (isolated rows first:
the layer's order), `pair` = ops.linear_pair, `q` / `iso` = either launch alone.  Prints every block and the medians, and
compares the outputs of `pair` and `two` bit for bit."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from radargnn_amd import ops

LAYERS = {2: (224, 464, 224), 3: (224, 464, 128), 4: (128, 272, 64)}          # K, N of the source term, N of the update


def main():
    argv = sys.argv[1:]
    blocks, reps, layer, out_path = 7, 20, 2, None
    while argv:
        a = argv.pop(0)
        if a == "--blocks": blocks = int(argv.pop(0))
        elif a == "--reps": reps = int(argv.pop(0))
        elif a == "--layer": layer = int(argv.pop(0))
        elif a == "--out": out_path = argv.pop(0)
    k, n_q, n_iso = LAYERS[layer]
    rows, with_edges = 192000, 133516
    dev = "cuda"
    torch.manual_seed(0)
    x = torch.rand(rows, k, device=dev) * 4 - 2
    w_q, w_iso, b_iso = (torch.rand(n_q, k, device=dev) - 0.5) * 0.2, (torch.rand(n_iso, k, device=dev) - 0.5) * 0.2, torch.rand(n_iso, device=dev) - 0.5
    table = torch.stack([torch.rand(k, device=dev) - 0.5, torch.rand(k, device=dev) + 0.5, torch.rand(k, device=dev) - 0.5])
    perm = torch.randperm(rows, device=dev)
    lists = []
    for ids in (perm[:with_edges], perm[with_edges:]):                          # ascending, in buffers of `rows` entries: the layers' lists
        buf = torch.zeros(rows, dtype=torch.int32, device=dev)
        buf[:ids.numel()] = ids.sort().values.int()
        lists.append((buf, torch.tensor([ids.numel()], dtype=torch.int64, device=dev)))
    outs = {v: (ops.padded_rows(rows, n_q, dev), torch.empty(rows, n_iso, device=dev),
                torch.empty(ops.stat_panels(rows), ops.STAT_ROWS, n_iso, device=dev)) for v in ("two", "pair", "q", "iso")}

    def calls(v):
        q_out, h, stats = outs[v]
        first = dict(a1=x, w1=w_q, row_index=lists[0][0], m_dev=lists[0][1], a1_affine=table, out=q_out)
        second = dict(a1=x, w1=w_iso, bias1=b_iso, out=h, row_index=lists[1][0], m_dev=lists[1][1], stats_out=stats, a1_affine=table)
        return first, second

    def issue(v):
        first, second = calls(v)
        if v == "pair":
            ops.linear_pair(first, second)
        else:
            if v in ("two", "iso"):
                ops.linear(**second)
            if v in ("two", "q"):
                ops.linear(**first)

    variants = ["two", "pair", "q", "iso"]
    graphs = {}
    with ops.bound_tracking(dev):
        ops.set_bound(table, ops.make_bound(torch.tensor(8.0, device=dev)))
        for v in variants:
            for t in outs[v]:
                t.zero_()
            issue(v)                                                            # eager: weight planes, split-K scratch, LDS attributes
        torch.cuda.synchronize()
        fused = ops.linear_pair_fuses(*calls("pair"))
        same = all(torch.equal(a, b) for a, b in zip(outs["two"], outs["pair"]))
        for v in variants:
            graphs[v] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[v]):
                for _ in range(reps):
                    issue(v)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {v: [] for v in variants}
    for v in variants:
        graphs[v].replay()                                                      # warm-up
    for _ in range(blocks):
        for v in variants:
            e0.record()
            graphs[v].replay()
            e1.record()
            e1.synchronize()
            times[v].append(round(e0.elapsed_time(e1) / reps * 1e3, 2))          # us per repetition
    res = {"layer": layer, "k": k, "n_q": n_q, "n_iso": n_iso, "rows_q": with_edges, "rows_iso": rows - with_edges, "reps": reps,
           "pair_runs_as_one_grid": fused, "pair_equals_two_launches": same, "blocks_us": times,
           "median_us": {v: statistics.median(t) for v, t in times.items()}, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
