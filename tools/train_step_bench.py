"""Time one training step (trainer.py:175-231 shape: forward, cross-entropy + Huber, backward, Adam) of the C2 workload
on the HIP path.  Not the headline metric (that is bench.py, inference); a measurement for MEASUREMENTS.md section 8.

    python tools/train_step_bench.py [steps] [adam|fused|ab]

adam (default): torch.optim.Adam; fused: radargnn_amd.optim.FusedAdam (one launch per step); ab: both on the same model and batch,
in alternating rounds of `steps` steps after a warm-up of each, one line per round -- the rounds show the run-to-run spread."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from radargnn_amd import frames as fr, synthetic
from radargnn_amd.gnn.mpnn_layers import TargetCSR

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
model = bench.c2_model().cuda()
settings = fr.GraphSettings(algorithm="radius", k=0, r=1.0)
batch = fr.FrameBatch.from_frames([synthetic.radarscenes_frame(i) for i in range(64)])
g = fr.build_graphs(batch, settings)
n = g.x.shape[0]
label = torch.randint(0, 6, (n,), device="cuda")
box = torch.randn(n, 5, device="cuda")
y = torch.cat((label.float().view(-1, 1), box), 1)              # graph_batch.y: label | box (trainer.py:185-186)
from radargnn_amd.gnn.losses import detection_loss
which = sys.argv[2] if len(sys.argv) > 2 else "adam"
if which not in ("adam", "fused", "ab"):
    sys.exit(f"unknown optimizer {which!r}: adam, fused or ab")


def make_optimizer(name):
    if name == "fused":
        from radargnn_amd.optim import FusedAdam
        return FusedAdam(model.parameters(), lr=1e-3)
    return torch.optim.Adam(model.parameters(), lr=1e-3)


opt = make_optimizer("adam" if which == "ab" else which)
x, ei, ea = g.x, g.edge_index, g.edge_attr


def step():
    opt.zero_grad()
    x.requires_grad_(); ea.requires_grad_()
    c, bb = model(x, ei, ea)
    loss, _, _ = detection_loss(c, bb, y, 5, [1.0, 1.0, 1.0, 1.0, 1.0, 0.3])   # trainer.py:181-222 on the device
    loss.backward()
    opt.step()
    return loss


def timed_round():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


if which == "ab":
    optimizers = {"adam": opt, "fused": make_optimizer("fused")}
    for opt in optimizers.values():
        for _ in range(3):
            step()
    rounds = {name: [] for name in optimizers}
    for r in range(6):
        for name in (("adam", "fused") if r % 2 == 0 else ("fused", "adam")):
            opt = optimizers[name]
            rounds[name].append(timed_round())
    for name, ms in rounds.items():
        print(f"{name:5s} train step ms per round: " + " ".join(f"{v:.3f}" for v in ms) +
              f" | median {sorted(ms)[len(ms) // 2]:.3f} min {min(ms):.3f} max {max(ms):.3f}")
    sys.exit(0)

for _ in range(2):
    step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    l = step()
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / steps
with torch.no_grad():
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps):
        model(x, ei, ea)
    torch.cuda.synchronize()
    df = (time.perf_counter() - t0) / steps
print(f"train step {dt*1e3:.2f} ms ({64/dt:.0f} frames/s), forward only {df*1e3:.2f} ms, loss {l.item():.4f}, N={n}, E={ei.shape[1]}")
