"""The backward pass against float64 AT THE SIZE bench.py TRAINS (``training_step``: the C2 workload, 64 frames x 3000 points,
192 000 nodes, 799 078 radius edges, ``c2_model()``, the detection loss).  tests/test_gpu_backward.py stops at 2 000 nodes; here:

1. per kernel family, strict (norm-wise per tensor against float64, ``GTOL`` = 2e-5 unless stated):
   * ``ops.mpnn_aggregate_bwd``, max, on the real C2 graph and on a C4-shaped kNN k = 20 batch (3.84 M edges): the generic kernel
     (``edge_maps=None``) and the lane-local one (de = 8, ``edge_maps``) with and without the forward's recorded winners.  The
     winners the launch used are read back (``arg_out``): each one attains the float64 maximum to within
     delta = 1e-6 max|v64|, and equals the float64 first-id winner wherever best and runner-up are further apart than delta; the
     forward's recorded winners and the backward's recomputed ones obey the same two conditions between each other.  dQ,
     d_edge_attr and dW_e against float64 routed through the kernel's own winners;
   * mean and add through the same entry point;
   * ``ops.linear_wgrad`` at M = 192 000 and M = 799 078 rows at the step's widths, bf16x3 and f16x2 forms, all rows and a row list;
   * the BatchNorm backward chain (``rgnn_bn_bwd_stats`` / ``_coef`` / ``_apply``, mask from the apply table and from y) at 192 000 rows;
   * the detection loss and its backward at n = 192 000 (loss 2e-6, gradients 2e-5 against oracle/loss_oracle.py).
2. end to end: one C2 training step's backward (and a 24-frame step of a RadarPointGNNConv model with BatchNorm inside its MLPs)
   against autograd of the differentiable hoisted float64 oracle (oracle/gnn_hoisted.py), pinned in the same test against the
   faithful per-edge oracle.  Parameter gradients, dX and dEA within max(GTOL, 4 err32), err32 being the error of the same oracle
   evaluated in fp32 (TF32 off) -- at 10^8 activations a few ReLU inputs within rounding of zero flip their mask in ANY fp32
   evaluation (the convention of tools/fuzz_backward.py).  Every bar and measured error is recorded (conftest.record_parity).
   LOOSE BARS: at this size that convention gives bars above 1e-3 to dX, dEA and most first-layer / conv weight gradients (C2:
   17 of 46 tensors, up to ~0.2 for dEA; near-tie winners and ReLU masks flip between any two fp32 evaluations).  Their kernels
   are held strictly by section 1: test_max_aggregation_backward_at_full_size and test_exact_ties_in_the_backward_kernels (edge
   stage: dQ, d_edge_attr, dW_e), test_weight_gradient_at_the_step_sizes (every dW), test_batchnorm_backward_chain_at_192000_rows
   and test_detection_loss_and_backward_at_192000_rows.
   What the C2 step runs (pinned by the test): the lane-local max backward with the forward's recorded winners (the edge
   embedding's last Linear is folded into W_e, so the edge stage is 8 wide), BatchNorm backward with the mask from the apply table.
3. edges: a hub target with 65 535 / 65 536 / 65 537 in-edges on either side of the uint16 winner limit (TargetCSR.edge_maps());
   exact ties (duplicate points, duplicate edges) through ``model(x, ei, ea)`` on both backward kernels, which must follow the
   first-id rule; HotPath under autograd builds the ordered CSR (bit-equal gradients to the ordered build)."""
import time

import pytest
import torch

from conftest import record_parity
from oracle import gnn_hoisted as GH
from oracle import gnn_oracle as G
from oracle import loss_oracle as L
from radargnn_amd import synthetic

pytestmark = pytest.mark.gpu
GTOL = 2e-5
WEIGHTS = [1.0, 1.0, 1.0, 1.0, 1.0, 0.3]
F64 = torch.float64


@pytest.fixture(scope="module")
def rg():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    from radargnn_amd import frames, gnn, ops
    from radargnn_amd.gnn.mpnn_layers import TargetCSR
    return frames, gnn, ops, TargetCSR


def normwise(a, b) -> float:
    a, b = a.detach().to(F64), b.detach().to(F64).to(a.device)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.fixture(scope="module")
def c2(rg):
    """bench.training_step's graph: C2 settings over radarscenes frames 0..63, keyed by target as the model's forward keys it."""
    import bench
    fr, gnn, ops, TargetCSR = rg
    batch = fr.FrameBatch.from_frames([synthetic.radarscenes_frame(i) for i in range(64)])
    g = fr.build_graphs(batch, bench.c2_settings())
    g.check()
    assert g.edge_index.shape[1] == 799078 and g.x.shape[0] == 192000
    return g, TargetCSR(g.edge_index, g.x.shape[0])


@pytest.fixture(scope="module")
def c4(rg):
    fr, gnn, ops, TargetCSR = rg
    batch = fr.FrameBatch.from_frames([synthetic.radarscenes_frame(100 + i) for i in range(64)])
    g = fr.build_graphs(batch, fr.GraphSettings(algorithm="knn", k=20))
    g.check()
    assert g.edge_index.shape[1] == 3840000
    return g, TargetCSR(g.edge_index, g.x.shape[0])


# ---- 1. per-kernel parity ------------------------------------------------------------------------------------------------
def _sorted_edges(graph):
    tgt = graph.edge_index[1][graph.perm.long()].long()          # target of every row of the target-sorted edge list
    return graph.src.long(), tgt


def _runner_up(Q64, We64, ea64, src, tgt, n, win, chunk=1 << 18):
    """-> (second largest message per (target, channel) once the first-id winner is taken out: -inf for a single edge,
    max |v| over all messages)."""
    d = Q64.shape[1]
    R = torch.full((n, d), float("-inf"), dtype=F64, device=Q64.device)
    vmax = 0.0
    for a in range(0, src.numel(), chunk):
        s, t = src[a:a + chunk], tgt[a:a + chunk]
        v = Q64[s] + ea64[a:a + chunk] @ We64.t()
        vmax = max(vmax, float(v.abs().max()))
        pos = torch.arange(a, a + s.numel(), device=v.device).view(-1, 1)
        v = torch.where(win[t] == pos, torch.full_like(v, float("-inf")), v)
        R.scatter_reduce_(0, t.view(-1, 1).expand(-1, d), v, "amax")
    return R, vmax


def _value_at(Q64, We64, ea64, src, pos, rows=8192):
    """v64[pos[t, c], c] = Q64[src[pos], c] + ea64[pos] . We64[c] for every (t, c) with pos >= 0 (else -inf)."""
    n, d = pos.shape
    out = torch.full((n, d), float("-inf"), dtype=F64, device=Q64.device)
    ch = torch.arange(d, device=Q64.device).view(1, -1)
    for a in range(0, n, rows):
        p = pos[a:a + rows]
        ok = p >= 0
        pc = p.clamp(min=0)
        v = Q64[src[pc], ch.expand_as(pc)] + (ea64[pc] * We64.unsqueeze(0)).sum(-1)
        out[a:a + rows] = torch.where(ok, v, out[a:a + rows])
    return out


def _winner_positions(arg, graph, kind):
    """The kernel's winners as positions in the target-sorted edge list (-1 on targets without edges)."""
    deg = (graph.rowptr[1:] - graph.rowptr[:-1]).long().view(-1, 1)
    if kind == "int32":
        pos = arg.long()
    else:                                                       # uint16 in-segment index
        pos = graph.rowptr[:-1].long().view(-1, 1) + (arg.long() & 0xFFFF)
    return torch.where(deg > 0, pos, torch.full_like(pos, -1))


def _check_winners(name, kern, ref, M64, gap, delta, valid, v_at):
    """kern / ref: winner positions.  Every kernel winner attains the float64 maximum to within delta; where best and runner-up
    are further apart than delta it is ``ref``.  -> number of near-ties."""
    vk = v_at(kern)
    assert bool((kern[valid] >= 0).all()), name
    short = (vk < M64 - delta) & valid
    assert not bool(short.any()), f"{name}: {int(short.sum())} winners more than delta below the float64 maximum"
    clear = valid & (gap > delta)
    bad = clear & (kern != ref)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} winners differ where the float64 gap exceeds delta"
    return int((valid & (gap <= delta)).sum())


def check_max_backward(rg, name, graph, d, de, path, seed, canon=None):
    """One max-aggregation backward launch against float64; path: 'generic' | 'local' (recomputed winners) | 'local+fwd'
    (the forward's recorded winners).  ``canon`` (node -> the node it duplicates): equal rows of Q for duplicates and edge
    attributes that are a function of (canon[source], target), so messages of duplicate points and duplicate edges tie EXACTLY
    -- in fp32 as in float64 -- and the first-id rule alone decides: the kernel's winner must be the float64 first-id winner there.
    Returns the number of near-ties."""
    fr, gnn, ops, _ = rg
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(seed)
    n, E = graph.num_nodes, graph.num_edges
    Q = torch.randn(n, d, device=dev, generator=gen)
    We = torch.randn(d, de, device=dev, generator=gen) * 0.5
    ea = torch.randn(E, de, device=dev, generator=gen)
    if canon is not None:
        Q = Q[canon].contiguous()
        ei = graph.edge_index[:, graph.perm.long()].long()                       # sorted order
        key = (canon[ei[0]] * 1.37 + ei[1] * 0.61).double().view(-1, 1) + torch.arange(de, device=dev).view(1, -1) * 2.3
        ea = torch.sin(key).float().contiguous()
    dM = torch.randn(n, d, device=dev, generator=gen)
    src, tgt = _sorted_edges(graph)
    Q64, We64, ea64 = Q.to(F64), We.to(F64), ea.to(F64)
    M64, win64 = GH.edge_max(Q64, We64, ea64, src, tgt, n)
    R64, vmax = _runner_up(Q64, We64, ea64, src, tgt, n, win64)
    delta = 1e-6 * vmax
    valid = win64 >= 0
    gap = M64 - R64
    v_at = lambda p: _value_at(Q64, We64, ea64, src, p)
    maps = None if path == "generic" else graph.edge_maps()
    if path != "generic":
        assert maps is not None and ops.lib.rgnn_mpnn_max_bwd_supported(d, de)
    fwd_arg = None
    if path == "local+fwd":
        M, fwd_arg = ops.mpnn_aggregate_max_arg(None, Q, We, ea, graph.rowptr, graph.src, chunks=graph.chunks)
        assert fwd_arg is not None
        assert normwise(M[valid.any(1)], M64[valid.any(1)]) < 1e-6
    out = torch.empty((n, d), dtype=torch.int32 if path == "generic" else torch.int16, device=dev)
    dQ, dea, dWe = ops.mpnn_aggregate_bwd(dM, Q, We, ea, graph.rowptr, graph.src, "max", graph.source_csr(), edge_maps=maps,
                                          arg=fwd_arg, arg_out=None if fwd_arg is not None else out)
    torch.cuda.synchronize()
    used = fwd_arg if fwd_arg is not None else out
    kern = _winner_positions(used, graph, "int32" if path == "generic" else "uint16")
    near = _check_winners(name, kern, win64, M64, gap, delta, valid, v_at)
    if canon is not None:
        exact = valid & (gap == 0)
        assert int(exact.sum()) > 1000, int(exact.sum())
        wrong = exact & (kern != win64)
        assert not bool(wrong.any()), f"{name}: {int(wrong.sum())} of {int(exact.sum())} exact ties not won by the first edge"
        print(f"[max bwd] {name}: {int(exact.sum())} exact ties, all won by the first edge")
    if fwd_arg is not None:                                       # the backward's own recomputation next to the forward's record
        ops.mpnn_aggregate_bwd(dM, Q, We, ea, graph.rowptr, graph.src, "max", graph.source_csr(), edge_maps=maps, arg_out=out)
        bwd = _winner_positions(out, graph, "uint16")
        _check_winners(name + " [recomputed]", bwd, win64, M64, gap, delta, valid, v_at)
        differ = valid & (bwd != kern)
        assert not bool((differ & (gap > delta)).any())
        print(f"[max bwd] {name}: forward and backward winners differ on {int(differ.sum())} near-ties")
    eQ, eA, eW = GH.edge_max_backward(dM.to(F64), We64, ea64, src, tgt, n, kern)
    errs = {"dQ": normwise(dQ, eQ), "d_edge_attr": normwise(dea, eA), "dW_e": normwise(dWe, eW)}
    print(f"[max bwd] {name}: {int(valid.sum())} (target, channel) maxima, {near} near-ties (gap <= {delta:.2e})")
    record_parity(f"backward {name} [near-ties {near}]", **errs)
    assert all(v < GTOL for v in errs.values()), errs
    return near


MAX_CASES = [("c2", 224, 16, "generic"), ("c2", 224, 8, "generic"), ("c2", 224, 8, "local"), ("c2", 224, 8, "local+fwd"),
             ("c2", 128, 8, "local+fwd"), ("c2", 64, 16, "generic"), ("c4", 224, 16, "generic"), ("c4", 128, 8, "local"),
             ("c4", 64, 8, "local+fwd")]


@pytest.mark.parametrize("which,d,de,path", MAX_CASES, ids=lambda c: str(c))
def test_max_aggregation_backward_at_full_size(rg, request, which, d, de, path):
    graph = request.getfixturevalue(which)[1]
    check_max_backward(rg, f"max {which.upper()} ({graph.num_edges} edges) d={d} de={de} {path}", graph, d, de, path, seed=d + de)


@pytest.mark.parametrize("which,aggr,d,de", [("c2", "mean", 128, 16), ("c2", "add", 224, 8), ("c4", "mean", 64, 16),
                                             ("c4", "add", 64, 8)])
def test_mean_and_add_backward_at_full_size(rg, request, which, aggr, d, de):
    fr, gnn, ops, _ = rg
    graph = request.getfixturevalue(which)[1]
    gen = torch.Generator(device="cuda").manual_seed(d)
    n, E = graph.num_nodes, graph.num_edges
    Q = torch.randn(n, d, device="cuda", generator=gen)
    We = torch.randn(d, de, device="cuda", generator=gen) * 0.5
    ea = torch.randn(E, de, device="cuda", generator=gen)
    dM = torch.randn(n, d, device="cuda", generator=gen)
    deg = graph.in_degree().view(-1)
    scale = (1.0 / deg.clamp(min=1.0)).contiguous() if aggr == "mean" else None
    dQ, dea, dWe = ops.mpnn_aggregate_bwd(dM, Q, We, ea, graph.rowptr, graph.src, aggr, graph.source_csr(), target_scale=scale)
    src, tgt = _sorted_edges(graph)
    g64 = dM.to(F64)
    if aggr == "mean":
        g64 = g64 / deg.to(F64).clamp(min=1.0).view(-1, 1)
    eQ = torch.zeros((n, d), dtype=F64, device="cuda")
    eA = torch.empty((E, de), dtype=F64, device="cuda")
    eW = torch.zeros((d, de), dtype=F64, device="cuda")
    for a in range(0, E, 1 << 18):
        rows = g64[tgt[a:a + (1 << 18)]]
        eQ.index_add_(0, src[a:a + (1 << 18)], rows)
        eA[a:a + (1 << 18)] = rows @ We.to(F64)
        eW += rows.t() @ ea[a:a + (1 << 18)].to(F64)
    errs = {"dQ": normwise(dQ, eQ), "d_edge_attr": normwise(dea, eA), "dW_e": normwise(dWe, eW)}
    record_parity(f"backward {aggr} {which.upper()} ({E} edges) d={d} de={de}", **errs)
    assert all(v < GTOL for v in errs.values()), errs


# the step's weight-gradient shapes: node embedding (5 -> 32 -> 64 -> 128 -> 224), conv update [x | M] and source term, both at
# 192 000 rows; the edge embedding (2 -> 4 -> 8 -> 16) at 799 078 rows (k_wgrad_narrow)
WGRAD = [(192000, 5, 0, 32), (192000, 64, 0, 128), (192000, 128, 0, 224), (192000, 224, 464, 224), (192000, 128, 272, 64),
         (192000, 224, 0, 464), (799078, 2, 0, 4), (799078, 4, 0, 8), (799078, 8, 0, 16)]


@pytest.mark.parametrize("m,k1,k2,n", WGRAD)
def test_weight_gradient_at_the_step_sizes(rg, m, k1, k2, n):
    """Both forms of rgnn_wgrad over long slabs: bf16x3 at the bars of test_weight_gradient_kernel_matches_float64 (4 x the fp32-MFMA
    kernel's error + 2e-7 where that kernel applies, else 2e-6), f16x2 with bounds at those of
    test_weight_gradient_in_the_f16x2_form_matches_float64 (2e-5 per column block, 4 x the bf16x3 error + 2e-6 overall); all rows
    and a row list of half of them."""
    fr, gnn, ops, _ = rg
    gen = torch.Generator(device="cuda").manual_seed(m + n + k1)
    Gd = torch.randn(m, n, device="cuda", generator=gen)
    A1 = torch.randn(m, k1, device="cuda", generator=gen)
    A2 = torch.randn(m, k2, device="cuda", generator=gen) * 0.5 if k2 else None
    full = torch.cat([A1.to(F64)] + ([A2.to(F64)] if k2 else []) + [torch.ones(m, 1, dtype=F64, device="cuda")], 1)
    exp = Gd.to(F64).t() @ full
    slabs = int(ops.lib.rgnn_wgrad_slabs(m, n, k1, k2, 1))
    got = ops.linear_wgrad(Gd, A1, A2, with_bias=True)
    err = normwise(got, exp)
    if n % 4 == 0 and k1 % 4 == 0 and k2 % 4 == 0:
        e32 = normwise(ops.linear_wgrad_fp32(Gd, A1, A2), exp[:, :-1])
        bar = 4 * e32 + 2e-7
        assert normwise(got[:, :-1], exp[:, :-1]) < bar
    else:
        e32, bar = float("nan"), 2e-6
    assert err < max(bar, 2e-6), (err, bar)
    rows = torch.randperm(m, generator=torch.Generator().manual_seed(m))[: m // 2 + 1].cuda()
    lst = torch.full((m,), -7, dtype=torch.int32, device="cuda")
    lst[:rows.numel()] = rows.int()
    cnt = torch.tensor([rows.numel()], dtype=torch.int64, device="cuda")
    part_exp = Gd[rows].to(F64).t() @ full[rows]
    part = ops.linear_wgrad(Gd, A1, A2, with_bias=True, row_index=lst, m_dev=cnt)
    err_rows = normwise(part, part_exp)
    assert err_rows < max(bar, 2e-6), err_rows
    before = ops.COUNTERS.get("wgrad_f16x2", 0)
    with ops.using_bounds(ops.BoundPool("cuda")):
        bounds = (ops.make_bound(Gd.abs().max()), ops.make_bound(A1.abs().max()), None if A2 is None else ops.make_bound(A2.abs().max()))
        f16 = ops.linear_wgrad(Gd, A1, A2, with_bias=True, bounds=bounds)
        f16_rows = ops.linear_wgrad(Gd, A1, A2, with_bias=True, row_index=lst, m_dev=cnt, bounds=bounds)
    assert ops.COUNTERS.get("wgrad_f16x2", 0) - before == 2
    worst16 = 0.0
    for got_, e_ in ((f16, exp), (f16_rows, part_exp)):
        for lo, hi in ((0, k1), (k1, k1 + k2), (k1 + k2, k1 + k2 + 1)):
            if hi > lo:
                e = normwise(got_[:, lo:hi], e_[:, lo:hi])
                worst16 = max(worst16, e)
                assert e < 2e-5, (lo, hi, e)
    assert normwise(f16, exp) < 4 * err + 2e-6
    record_parity(f"wgrad M={m} k1={k1} k2={k2} n={n} ({slabs} slabs)", bf16x3=err, bf16x3_rows=err_rows, fp32_mfma=e32,
                  f16x2_worst_block=worst16)


@pytest.mark.parametrize("c", [224, 128, 64])
@pytest.mark.parametrize("relu,from_table", [(True, True), (True, False), (False, False)])
def test_batchnorm_backward_chain_at_192000_rows(rg, monkeypatch, c, relu, from_table):
    """AG.batch_norm_act's backward (rgnn_bn_bwd_stats -> rgnn_bn_bwd_coef -> rgnn_bn_bwd_apply) against the float64
    formula dh = gamma rstd (g - mean g - xhat mean(g xhat)), g = relu'(y) dy with the mask taken from the DEVICE's y (torch's ReLU
    backward), dgamma = sum g xhat, dbeta = sum g."""
    fr, gnn, ops, _ = rg
    from radargnn_amd.gnn import autograd as AG
    monkeypatch.setattr(ops, "BN_BWD_MASK_FROM_TABLE", from_table)
    m = 192000
    gen = torch.Generator(device="cuda").manual_seed(c + relu)
    h = (torch.randn(m, c, device="cuda", generator=gen) * 3 + torch.randn(1, c, device="cuda", generator=gen)).requires_grad_(True)
    dy = torch.randn(m, c, device="cuda", generator=gen)
    bn = gnn.BatchNorm(c).cuda().train()
    with torch.no_grad():
        bn.module.weight.uniform_(0.5, 1.5)
        bn.module.bias.uniform_(-0.5, 0.5)
    y = AG.batch_norm_act(h, bn, relu=relu)
    y.backward(dy)
    h64, dy64 = h.detach().to(F64), dy.to(F64)
    mean = h64.mean(0)
    rstd = 1.0 / torch.sqrt(h64.var(0, unbiased=False) + bn.module.eps)
    xhat = (h64 - mean) * rstd
    gam = bn.module.weight.detach().to(F64)
    y64 = gam * xhat + bn.module.bias.detach().to(F64)
    assert normwise(y, torch.relu(y64) if relu else y64) < 1e-5
    g = torch.where(y.detach() > 0, dy64, torch.zeros_like(dy64)) if relu else dy64
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    dh = gam * rstd * (g - g.mean(0) - xhat * (g * xhat).mean(0))
    errs = {"dh": normwise(h.grad, dh), "dgamma": normwise(bn.module.weight.grad, dgamma), "dbeta": normwise(bn.module.bias.grad, dbeta)}
    record_parity(f"BatchNorm backward 192000 x {c} (relu {relu}, mask from {'table' if from_table else 'y'})", **errs)
    assert all(v < GTOL for v in errs.values()), errs


def step_targets(n):
    """``y`` as bench.training_step makes it (labels 0..5 | 5 box values, one CUDA generator seeded 0)."""
    gen = torch.Generator(device="cuda").manual_seed(0)
    return torch.cat((torch.randint(0, 6, (n, 1), device="cuda", generator=gen).float(), torch.randn(n, 5, device="cuda", generator=gen)), 1)


def test_detection_loss_and_backward_at_192000_rows(rg):
    fr, gnn, ops, _ = rg
    n = 192000
    assert int(ops.lib.rgnn_detection_loss_blocks(n)) > 1
    y = step_targets(n)
    gen = torch.Generator(device="cuda").manual_seed(5)
    cls = (torch.randn(n, 6, device="cuda", generator=gen) * 2).requires_grad_(True)
    bb = torch.randn(n, 5, device="cuda", generator=gen).requires_grad_(True)
    loss, lc, lb = gnn.detection_loss(cls, bb, y, 5, WEIGHTS)
    loss.backward()
    c64, b64 = cls.detach().to(F64).requires_grad_(True), bb.detach().to(F64).requires_grad_(True)
    l64, lc64, lb64 = L.detection_loss_vectorised(c64, b64, y.to(F64), 5, WEIGHTS)
    l64.backward()
    errs = {"loss": abs(float(loss) - float(l64)) / abs(float(l64)), "loss_cls": abs(float(lc) - float(lc64)) / abs(float(lc64)),
            "loss_bb": abs(float(lb) - float(lb64)) / abs(float(lb64))}
    assert all(v < 2e-6 for v in errs.values()), errs
    gerr = {"d_cls": normwise(cls.grad, c64.grad), "d_boxes": normwise(bb.grad, b64.grad)}
    record_parity("detection loss n=192000 (bench.training_step's y, weights [1,1,1,1,1,0.3])", **errs, **gerr)
    assert all(v < GTOL for v in gerr.values()), gerr


# ---- 2. end to end -------------------------------------------------------------------------------------------------------
def _leaves(sd, dtype):
    return {k: (v.detach().to("cuda", dtype).requires_grad_("running" not in k) if v.is_floating_point() else v.detach().cuda())
            for k, v in sd.items()}


def oracle_step(x, ei, ea, sd, y, conv_type, dtype):
    """Autograd of the hoisted oracle + the vectorised loss in ``dtype`` on the GPU -> (loss, logits, boxes, grads by name, dX, dEA)."""
    sd_ = _leaves(sd, dtype)
    x_ = x.detach().to(dtype).requires_grad_(True)
    ea_ = ea.detach().to(dtype).requires_grad_(True)
    c, b = GH.det_net_basic_hoisted_grad(x_, ei, ea_, sd_, conv_layer_type=conv_type)
    loss = L.detection_loss_vectorised(c, b, y.to(dtype), 5, WEIGHTS)[0]
    loss.backward()
    return (loss.detach(), c.detach(), b.detach(), {k: v.grad for k, v in sd_.items() if v.requires_grad and v.grad is not None},
            x_.grad, ea_.grad)


def pin_hoisted_grad(x, ei, ea, sd, conv_type, name):
    """The differentiable hoisted evaluation against autograd of the faithful per-edge oracle (CPU, float64), small batch."""
    rc, rb = torch.randn(x.shape[0], 6, dtype=F64), torch.randn(x.shape[0], 5, dtype=F64)
    res = []
    for fn in (lambda x_, ea_, s: G.det_net_basic(x_, ei.cpu(), ea_, s, conv_type, dtype=F64),
               lambda x_, ea_, s: [t.cpu() for t in GH.det_net_basic_hoisted_grad(
                   x_.cuda(), ei.cuda(), ea_.cuda(), {k: v.cuda() for k, v in s.items()}, conv_type)]):
        s = {k: v.detach().cpu().to(F64).requires_grad_("running" not in k) if v.is_floating_point() else v.cpu() for k, v in sd.items()}
        x_ = x.detach().cpu().to(F64).requires_grad_(True)
        ea_ = ea.detach().cpu().to(F64).requires_grad_(True)
        c, b = fn(x_, ea_, s)
        ((c * rc).sum() + (b * rb).sum()).backward()
        res.append((c.detach(), b.detach(), x_.grad, ea_.grad, {k: v.grad for k, v in s.items() if v.requires_grad}))
    (c0, b0, dx0, da0, g0), (c1, b1, dx1, da1, g1) = res
    largest = max(float(v.abs().max()) for v in g0.values())
    # (an exactly-zero gradient -- a bias in front of a train-mode BatchNorm -- against the largest one)
    worst = max(max(float((g1[k] - g0[k]).abs().max()) / (largest if float(g0[k].abs().max()) < 1e-9 * largest else float(g0[k].abs().max()))
                    for k in g0),
                normwise(dx1, dx0), normwise(da1, da0))
    errs = {"logits": normwise(c1, c0), "boxes": normwise(b1, b0), "worst_gradient": worst}
    record_parity(name + " [hoisted grad f64 vs faithful f64]", **errs)
    assert errs["logits"] < 1e-10 and errs["boxes"] < 1e-10 and worst < 1e-9, errs


def _spy(monkeypatch, ops):
    """Which backward entry points run: mpnn_aggregate_bwd (lane-local or generic form), bn_bwd_stats (mask from the table / y / none)."""
    seen = {}
    real_bwd, real_stats = ops.mpnn_aggregate_bwd, ops.bn_bwd_stats

    def bwd(dM, Q, We, ea, *a, **k):
        de = 0 if ea is None else ea.shape[1]
        local = (a[2] == "max" and k.get("edge_maps") is not None and bool(ops.lib.rgnn_mpnn_max_bwd_supported(Q.shape[1], de)))
        key = f"mpnn_bwd {a[2]} {'lane-local' if local else 'generic'} de={de}" + (" fwd-arg" if k.get("arg") is not None else "")
        seen[key] = seen.get(key, 0) + 1
        return real_bwd(dM, Q, We, ea, *a, **k)

    def stats(dy, y, h, table=None):
        key = "bn_bwd_stats " + ("table" if table is not None else ("y" if y is not None else "no mask"))
        seen[key] = seen.get(key, 0) + 1
        return real_stats(dy, y, h, table=table)

    monkeypatch.setattr(ops, "mpnn_aggregate_bwd", bwd)
    monkeypatch.setattr(ops, "bn_bwd_stats", stats)
    return seen


def end_to_end(rg, monkeypatch, name, model, g, conv_type, pin_graph):
    fr, gnn, ops, _ = rg
    t0 = time.perf_counter()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    pin_hoisted_grad(*pin_graph, sd, conv_type, name)
    model.cuda().train()
    n = g.x.shape[0]
    y = step_targets(n)
    seen = _spy(monkeypatch, ops)
    w0 = (ops.COUNTERS.get("wgrad_f16x2", 0), ops.COUNTERS.get("wgrad_other", 0))
    x = g.x.clone().requires_grad_(True)
    ea = g.edge_attr.clone().requires_grad_(True)
    c, bb = model(x, g.edge_index, ea)
    loss = gnn.detection_loss(c, bb, y, 5, WEIGHTS)[0]
    loss.backward()
    torch.cuda.synchronize()
    wg = (ops.COUNTERS.get("wgrad_f16x2", 0) - w0[0], ops.COUNTERS.get("wgrad_other", 0) - w0[1])
    print(f"[e2e] {name}: entry points {seen}, wgrad launches (f16x2, bf16x3) {wg}")
    ei = g.edge_index
    l64, c64, b64, g64, dx64, dea64 = oracle_step(x, ei, ea, sd, y, conv_type, F64)
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    l32, c32, b32, g32, dx32, dea32 = oracle_step(x, ei, ea, sd, y, conv_type, torch.float32)
    lerr = abs(float(loss) - float(l64)) / abs(float(l64))
    errs = {"loss": lerr, "logits": normwise(c, c64), "boxes": normwise(bb, b64)}
    assert lerr < 2e-6 and errs["logits"] < 1e-5 and errs["boxes"] < 1e-5, errs
    largest = max(float(v.abs().max()) for v in g64.values())

    def rel_err(got, ref):
        # (a bias in front of a train-mode BatchNorm has the exact gradient 0: against the largest gradient; everything else against
        #  its own magnitude floored at 5 % of the largest -- test_det_net_backward_matches_float64_autograd)
        r = float(ref.abs().max())
        return float((got.detach().to(F64) - ref.to(F64)).abs().max()) / (largest if r < 1e-9 * largest else max(r, 5e-2 * largest))

    table, bad = {}, {}
    pairs = [(nm, p.grad, g64[nm], g32[nm]) for nm, p in model.named_parameters()] + [("dX", x.grad, dx64, dx32),
                                                                                        ("dEA", ea.grad, dea64, dea32)]
    for nm, got, ref, r32 in pairs:
        assert got is not None, nm
        e = normwise(got, ref) if nm in ("dX", "dEA") else rel_err(got, ref)
        e32 = normwise(r32, ref) if nm in ("dX", "dEA") else rel_err(r32, ref)
        bar = max(GTOL, 4 * e32)
        table[nm], table[nm + " (fp32 oracle)"] = e, e32
        if not e < bar:
            bad[nm] = (e, bar)
    record_parity(name + f" [{time.perf_counter() - t0:.0f} s]", **errs, **table)
    assert not bad, bad
    return seen, wg


def test_c2_training_step_backward_vs_float64(rg, c2, monkeypatch):
    """bench.training_step's step, once: c2_model(), the C2 graph, the detection loss; requires_grad_ on x and ea."""
    import bench
    fr, gnn, ops, _ = rg
    g, _ = c2
    one = fr.build_graphs(fr.FrameBatch.from_frames([synthetic.radarscenes_frame(0)]), bench.c2_settings())
    seen, wg = end_to_end(rg, monkeypatch, "C2 training step (192000 nodes, 799078 edges)", bench.c2_model(), g, "MPNNConv",
                          (one.x, one.edge_index, one.edge_attr))
    # what ran (measured, then pinned): the edge embedding's last Linear is folded into W_e, so the edge stage is 8 wide and the max
    # backward is the LANE-LOCAL kernel with the winners the forward recorded -- not the generic one; the BatchNorm backward reads
    # its ReLU mask from the apply table; the weight gradients take both forms
    assert seen == {"mpnn_bwd max lane-local de=8 fwd-arg": 4, "bn_bwd_stats table": 4}, seen
    assert wg[0] > 0 and wg[1] > 0, wg


def test_radar_point_conv_with_batchnorm_in_mlps_backward_vs_float64(rg, monkeypatch):
    """24 frames of the C2 workload (> 10^4 rows), RadarPointGNNConv with one pre-layer (hoistable), BatchNorm inside the embedding
    and head MLPs: the other conv type and the BatchNorm-in-MLP backward at the bars of the C2 step."""
    import bench
    fr, gnn, ops, _ = rg
    g = fr.build_graphs(fr.FrameBatch.from_frames([synthetic.radarscenes_frame(i) for i in range(24)]), bench.c2_settings())
    torch.manual_seed(3)
    model = gnn.DetNetBasic(gnn.GNNArchitectureConfig(5, 2, [64, 64, 64], [6], [16, 5], True, True, [32, 64], [4, 8, 16],
                                                      "RadarPointGNNConv", True))
    one = fr.build_graphs(fr.FrameBatch.from_frames([synthetic.radarscenes_frame(0)]), bench.c2_settings())
    seen, wg = end_to_end(rg, monkeypatch, f"RadarPointGNNConv, BatchNorm in MLPs, 24 frames ({g.x.shape[0]} nodes)", model, g,
                          "RadarPointGNNConv", (one.x, one.edge_index, one.edge_attr))
    # (RadarPointGNNConv goes through AggregateFn: lane-local kernel, winners recomputed; 7 BatchNorms: 3 convs', 1 in the node
    #  embedding, 2 in the edge embedding, 1 in the regression head)
    assert seen == {"mpnn_bwd max lane-local de=8": 3, "bn_bwd_stats table": 7}, seen


# ---- 3. edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hub", [65535, 65536, 65537])
def test_in_degree_limit_of_the_lane_local_winners(rg, hub):
    """One target with ``hub`` in-edges (winners stored as uint16 indices inside the segment): TargetCSR.edge_maps() follows its
    guard (present up to 65 535, None above), and the backward is right on both sides -- the lane-local kernel (recomputed and
    forward-recorded winners) where the maps exist, the generic kernel otherwise."""
    fr, gnn, ops, TargetCSR = rg
    n = hub + 1 + 2000
    g = torch.Generator().manual_seed(hub)
    hub_src = torch.randperm(n - 1, generator=g)[:hub] + 1                     # distinct sources, node 0 is the hub
    other = torch.stack([torch.randint(0, n, (20000,), generator=g), torch.randint(1, n, (20000,), generator=g)])
    ei = torch.cat([torch.stack([hub_src, torch.zeros_like(hub_src)]), other], 1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)].contiguous().cuda()
    graph = TargetCSR(ei, n)
    maps = graph.edge_maps()
    assert (maps is not None) == (hub <= 65535)
    check_max_backward(rg, f"hub of {hub} in-edges d=8 de=2 generic", graph, 8, 2, "generic", seed=hub)
    if maps is not None:
        check_max_backward(rg, f"hub of {hub} in-edges d=8 de=2 local", graph, 8, 2, "local", seed=hub)
        check_max_backward(rg, f"hub of {hub} in-edges d=8 de=2 local+fwd", graph, 8, 2, "local+fwd", seed=hub)
    else:                                                                     # what the layers then launch: the generic kernel
        torch.manual_seed(0)
        conv = gnn.MPNNConv(8, 8, 2, aggr="max").cuda()
        x = torch.randn(n, 8, device="cuda", requires_grad=True)
        ea = torch.randn(ei.shape[1], 2, device="cuda", requires_grad=True)
        sd = {k: v.detach().to(F64).requires_grad_(True) for k, v in conv.state_dict().items()}
        r = torch.randn(n, 8, device="cuda")
        (conv(x, ei, ea) * r).sum().backward()
        x64, ea64 = x.detach().to(F64).requires_grad_(True), ea.detach().to(F64).requires_grad_(True)
        W = sd["pre_mlp.0.weight"]
        M, _ = GH._EdgeMax.apply(x64 @ W[:, 8:16].t(), W[:, 16:], ea64, ei[0], ei[1], n, 1 << 18, None)
        deg = torch.bincount(ei[1], minlength=n).view(-1, 1)
        m = torch.where(deg > 0, M + torch.nn.functional.linear(x64, W[:, :8], sd["pre_mlp.0.bias"]), torch.zeros((), dtype=F64, device="cuda"))
        out = torch.nn.functional.linear(torch.cat([x64, m], 1), sd["post_mlp.0.weight"], sd["post_mlp.0.bias"])
        (out * r.to(F64)).sum().backward()
        errs = {"dX": normwise(x.grad, x64.grad), "dEA": normwise(ea.grad, ea64.grad)}
        errs.update({k: normwise(p.grad, sd[k].grad) for k, p in conv.named_parameters()})
        record_parity(f"MPNNConv over a hub of {hub} in-edges (no edge maps)", **errs)
        assert all(v < GTOL for v in errs.values()), errs


def duplicate_point_batch(fr, n_frames=8, k=12):
    """RadarScenes-shaped frames in which every 10th point repeats the point before it exactly (position, velocity, RCS, time):
    messages from a point and its twin to a common target tie exactly."""
    frames = []
    for i in range(n_frames):
        f = synthetic.radarscenes_frame(200 + i)
        X, V, rcs, ts = f.X.copy(), f.V.copy(), f.rcs.copy(), f.timestamp.copy()
        X[1::10], V[1::10], rcs[1::10], ts[1::10] = X[0::10][:len(X[1::10])], V[0::10][:len(V[1::10])], rcs[0::10][:len(rcs[1::10])], \
            ts[0::10][:len(ts[1::10])]
        frames.append(synthetic.RadarFrame(X, V, rcs, ts))
    return fr.FrameBatch.from_frames(frames), fr.GraphSettings(algorithm="knn", k=k)


@pytest.mark.parametrize("d,de,path", [(224, 16, "generic"), (64, 16, "generic"), (224, 8, "generic"), (224, 8, "local"),
                                        (128, 8, "local+fwd")])
def test_exact_ties_in_the_backward_kernels(rg, d, de, path):
    """Exact ties on the duplicate-point kNN batch (+ duplicate edges) at kernel level: generic kernel (k_mpnn_bwd_arg),
    lane-local kernel with recomputed winners, and the winners the forward kernel records -- all follow the first-id rule."""
    fr, gnn, ops, TargetCSR = rg
    batch, cfg = duplicate_point_batch(fr)
    g = fr.build_graphs(batch, cfg)
    ei = torch.cat([g.edge_index, g.edge_index[:, ::997]], 1).contiguous()        # duplicate edges, listed after their originals
    n = g.x.shape[0]
    canon = torch.arange(n, device="cuda")
    ptr = batch.frame_ptr.tolist()
    for a, b in zip(ptr[:-1], ptr[1:]):
        dup = torch.arange(a + 1, b, 10, device="cuda")
        canon[dup] = dup - 1
    check_max_backward(rg, f"exact ties kNN ({ei.shape[1]} edges) d={d} de={de} {path}", TargetCSR(ei, n), d, de, path, seed=d,
                       canon=canon)


@pytest.mark.parametrize("edge_emb", [[4, 8, 16], [4, 8]], ids=["emb16", "emb8"])
def test_exact_ties_follow_the_first_id_rule(rg, monkeypatch, edge_emb):
    """Duplicate points and a few duplicate edges (kNN batch): exact ties at the max aggregation.  The gradient of a tied maximum
    goes to the FIRST of the tied edges -- the oracle's rule -- through ``model(x, ei, ea)`` on both backward kernels."""
    fr, gnn, ops, _ = rg
    batch, cfg = duplicate_point_batch(fr)
    g = fr.build_graphs(batch, cfg)
    ei = torch.cat([g.edge_index, g.edge_index[:, ::5000]], 1).contiguous()      # duplicate edges, listed after their originals
    ea = torch.cat([g.edge_attr, g.edge_attr[::5000]], 0).contiguous()
    torch.manual_seed(2)
    model = gnn.DetNetBasic(gnn.GNNArchitectureConfig(5, 2, [64, 48], [6], [16, 5], True, True, [32, 64], edge_emb, "MPNNConv", False))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    found = []
    with torch.no_grad():
        GH.det_net_basic_hoisted_grad(g.x.to(F64), ei, ea.to(F64), _leaves(sd, F64), winners_out=found)
    src = ei[0].long()
    # exact ties: a winner's message equals that of a later in-edge of the same target -- counted on the first layer
    x64 = G.run_sequential(g.x.to(F64), _leaves(sd, F64), "node_emb_mlp.")
    e64 = G.run_sequential(ea.to(F64), _leaves(sd, F64), "edge_emb_mlp.")
    W = sd["convs.0.pre_mlp.0.weight"].cuda().to(F64)
    c = x64.shape[1]
    v = x64[src] @ W[:, c:2 * c].t() + e64 @ W[:, 2 * c:].t()
    win = found[0]
    vw = v.gather(0, win.clamp(min=0)[ei[1].long()])                           # winner's value at every edge's target
    tied_later = (v == vw) & (torch.arange(ei.shape[1], device="cuda").view(-1, 1) > win[ei[1].long()])
    seg_ties = int(tied_later.sum())
    assert seg_ties > 100, seg_ties
    # (the pin against the faithful oracle needs a batch WITHOUT ties: torch's amax splits a tied gradient -- one original frame)
    one = fr.build_graphs(fr.FrameBatch.from_frames([synthetic.radarscenes_frame(200)]), cfg)
    pin_graph = (one.x, one.edge_index, one.edge_attr)
    seen, _ = end_to_end(rg, monkeypatch, f"exact ties ({seg_ties} tied (edge, channel) pairs in layer 0), edge embedding {edge_emb}",
                         model, type("Gr", (), {"x": g.x, "edge_index": ei, "edge_attr": ea})(), "MPNNConv",
                         pin_graph)
    # (the embedding's last Linear is folded into W_e: the edge stage reads its 8- / 4-wide input -- the lane-local kernel with the
    #  forward's recorded winners; the generic kernel's tie rule is held by test_exact_ties_in_the_backward_kernels)
    assert {k for k in seen if k.startswith("mpnn_bwd max")} == {f"mpnn_bwd max lane-local de={edge_emb[-2]} fwd-arg"}, seen


def test_hot_path_under_autograd_builds_the_ordered_csr(rg, monkeypatch):
    """HotPath builds the CSR of a kNN batch without the stable in-segment order for a max-aggregation model -- for inference.  A
    step run under autograd's recording (the model's differentiable form) must not: under exact ties the gradient goes to the
    first in-edge, so the unordered build would make it depend on the order of the build's atomics.  Gradients through HotPath are
    bit-equal to those through the ordered build (RGNN_ORDERED_CSR) on a batch with duplicate points."""
    fr, gnn, ops, _ = rg
    from radargnn_amd.gnn import autograd as AG
    batch, cfg = duplicate_point_batch(fr, n_frames=4)
    torch.manual_seed(4)
    model = gnn.DetNetBasic(gnn.GNNArchitectureConfig(5, 2, [64, 48], [6], [16, 5], True, True, [32, 64], [4, 8, 16], "MPNNConv", False)).cuda()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    grads = []
    for ordered_env in (False, True):
        if ordered_env:
            monkeypatch.setenv("RGNN_ORDERED_CSR", "1")
        hot = fr.HotPath(model, cfg)
        assert hot._ordered_csr is ordered_env                    # inference: as before
        model.load_state_dict(sd)
        model.zero_grad()
        with torch.enable_grad(), AG.recording(direct=True):
            assert hot._ordered_csr is True
            c, bb, g = hot(batch)
        assert c.requires_grad
        y = step_targets(c.shape[0])
        gnn.detection_loss(c, bb, y, 5, WEIGHTS)[0].backward()
        grads.append([p.grad.clone() for p in model.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
