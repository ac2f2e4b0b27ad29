"""Pins of the oracle pieces the full-size backward tests (tests/test_gpu_backward_timed_sizes.py) stand on, CPU only:
* the differentiable hoisted evaluation (oracle/gnn_hoisted.py ``det_net_basic_hoisted_grad``) against autograd of the faithful
  per-edge oracle (oracle/gnn_oracle.py) on small tie-free batches: outputs and every gradient to 1e-10;
* its tie rule on a hand-built graph -- duplicate points and a duplicate edge: the whole gradient of a tied maximum goes to the
  lowest edge id (torch-scatter's rule, csrc/backward.hip), checked against a hand count;
* the vectorised float64 loss (oracle/loss_oracle.py ``detection_loss_vectorised``) against the per-node restatement of the
  trainer's loss: value and gradients to 1e-12, NaN-box and background-only batches included; Huber deltas other than 1,
  ``ignore_index`` (-100) labels and fractional labels (tests/test_gpu_loss_edges.py uses it above a few hundred rows)."""
import pytest
import torch

from oracle import gnn_hoisted as GH
from oracle import gnn_oracle as G
from oracle import loss_oracle as L


def rel(a, b) -> float:
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def random_sd(conv_type, aggr, enc, seed, bn_mlps=False):
    """A reference-keyed state_dict: node / edge embeddings, two conv layers, both heads (the shapes of DetNetBasic)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def lin(key, o, i):
        sd[key + ".weight"] = torch.randn(o, i, generator=g, dtype=torch.float64) / i ** 0.5
        sd[key + ".bias"] = torch.randn(o, generator=g, dtype=torch.float64) * 0.3

    def bn(key, c):
        sd[key + ".module.weight"] = 0.5 + torch.rand(c, generator=g, dtype=torch.float64)
        sd[key + ".module.bias"] = torch.rand(c, generator=g, dtype=torch.float64) - 0.5
        sd[key + ".module.running_mean"] = torch.zeros(c, dtype=torch.float64)
        sd[key + ".module.running_var"] = torch.ones(c, dtype=torch.float64)

    dn, de, c = 5, 2, 12
    lin("node_emb_mlp.0", 8, dn)
    if bn_mlps:
        bn("node_emb_mlp.1", 8)
    lin("node_emb_mlp.3" if bn_mlps else "node_emb_mlp.2", c, 8)
    lin("edge_emb_mlp.0", 4, de)
    lin("edge_emb_mlp.2", 6, 4)
    dims = [c, 10, 10] if conv_type == "MPNNConv" else [c, c, c]
    for l in range(2):
        ci, co = dims[l], dims[l + 1]
        e_in = 6
        if conv_type == "MPNNConv":
            if enc:
                lin(f"convs.{l}.edge_encoder", ci, e_in)
                e_in = ci
            msg = 2 * ci + e_in
        else:
            msg = ci + e_in
        lin(f"convs.{l}.pre_mlp.0", msg if conv_type == "MPNNConv" else ci, msg)
        lin(f"convs.{l}.post_mlp.0", co, ci + (msg if conv_type == "MPNNConv" else ci))
        bn(f"batch_norms.{l}", co)
    lin("classification_head.0", 6, dims[2])
    lin("regression_head.0", 7, dims[2])
    lin("regression_head.2", 5, 7)
    return sd


def random_graph(n, e, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (3 * e,), generator=g)
    dst = torch.randint(0, n - 3, (3 * e,), generator=g)          # (the last 3 nodes receive nothing)
    keep = src != dst
    pairs = torch.unique(torch.stack([src[keep], dst[keep]]), dim=1)
    return pairs[:, torch.randperm(pairs.shape[1], generator=g)[:e]].contiguous()


def grads_of(fn, x, ea, sd, rc, rb):
    sd = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in sd.items()}
    x, ea = x.clone().requires_grad_(True), ea.clone().requires_grad_(True)
    c, b = fn(x, ea, sd)
    ((c * rc).sum() + (b * rb).sum()).backward()
    return c.detach(), b.detach(), x.grad, ea.grad, {k: v.grad for k, v in sd.items() if v.requires_grad}


@pytest.mark.parametrize("conv,aggr,enc,bn_mlps", [("MPNNConv", "max", False, False), ("MPNNConv", "max", True, True),
                                                   ("MPNNConv", "mean", False, False), ("MPNNConv", "add", True, False),
                                                   ("RadarPointGNNConv", "max", False, True), ("RadarPointGNNConv", "add", False, False)])
@pytest.mark.parametrize("chunk", [1 << 18, 97])
def test_hoisted_gradients_equal_the_faithful_oracle(conv, aggr, enc, bn_mlps, chunk):
    torch.manual_seed(3)
    n, e = 60, 400
    sd = random_sd(conv, aggr, enc, seed=7, bn_mlps=bn_mlps)
    ei = random_graph(n, e, seed=5)
    x = torch.randn(n, 5, dtype=torch.float64)
    ea = torch.randn(ei.shape[1], 2, dtype=torch.float64)
    rc, rb = torch.randn(n, 6, dtype=torch.float64), torch.randn(n, 5, dtype=torch.float64)
    c0, b0, dx0, dea0, g0 = grads_of(lambda x_, ea_, sd_: G.det_net_basic(x_, ei, ea_, sd_, conv, aggr, dtype=torch.float64),
                                     x, ea, sd, rc, rb)
    c1, b1, dx1, dea1, g1 = grads_of(lambda x_, ea_, sd_: GH.det_net_basic_hoisted_grad(x_, ei, ea_, sd_, conv, aggr, chunk=chunk),
                                     x, ea, sd, rc, rb)
    assert rel(c1, c0) < 1e-12 and rel(b1, b0) < 1e-12
    assert rel(dx1, dx0) < 1e-10 and rel(dea1, dea0) < 1e-10
    assert g0.keys() == g1.keys()
    largest = max(float(v.abs().max()) for v in g0.values())
    for k in g0:
        # (a bias in front of a train-mode BatchNorm has the exact gradient 0: measured against the largest gradient)
        ref = float(g0[k].abs().max())
        assert float((g1[k] - g0[k]).abs().max()) < 1e-10 * (largest if ref < 1e-9 * largest else ref), k


def test_hoisted_winners_can_be_given_and_are_reported():
    """``winners=`` routes through the given edges; ``winners_out`` reports the first-id winners the oracle found."""
    n, e = 40, 240
    sd = random_sd("MPNNConv", "max", False, seed=2)
    ei = random_graph(n, e, seed=4)
    x, ea = torch.randn(n, 5, dtype=torch.float64), torch.randn(ei.shape[1], 2, dtype=torch.float64)
    rc, rb = torch.randn(n, 6, dtype=torch.float64), torch.randn(n, 5, dtype=torch.float64)
    found = []
    ref = grads_of(lambda x_, ea_, sd_: GH.det_net_basic_hoisted_grad(x_, ei, ea_, sd_, winners_out=found), x, ea, sd, rc, rb)
    assert len(found) == 2 and [tuple(w.shape) for w in found] == [(n, 30), (n, 26)]
    deg = torch.bincount(ei[1], minlength=n)
    assert bool((found[0][deg == 0] == -1).all()) and bool((found[0][deg > 0] >= 0).all())
    assert bool((ei[1][found[0][deg > 0]] == torch.nonzero(deg > 0).view(-1, 1)).all())        # a winner is an in-edge of its target
    same = grads_of(lambda x_, ea_, sd_: GH.det_net_basic_hoisted_grad(x_, ei, ea_, sd_, winners=found), x, ea, sd, rc, rb)
    assert torch.equal(same[2], ref[2]) and torch.equal(same[3], ref[3])
    other = [w.clone() for w in found]
    t = int(torch.nonzero(deg >= 2)[0])
    other[0][t, 0] = int(torch.nonzero(ei[1] == t)[-1]) if int(found[0][t, 0]) != int(torch.nonzero(ei[1] == t)[-1]) else \
        int(torch.nonzero(ei[1] == t)[0])
    moved = grads_of(lambda x_, ea_, sd_: GH.det_net_basic_hoisted_grad(x_, ei, ea_, sd_, winners=other), x, ea, sd, rc, rb)
    assert not torch.equal(moved[3], ref[3])                        # another winner: another edge receives the gradient


def test_max_tie_rule_on_a_hand_built_graph():
    """Nodes 0 and 1 are the same point (equal rows of Q), node 2 another; edges, in id order:
         e0: 1 -> 3,  e1: 0 -> 3  (duplicate points: an exact tie at target 3, every channel)
         e2: 2 -> 4,  e3: 2 -> 4  (a duplicate edge with equal attributes: an exact tie at target 4)
         e4: 0 -> 4               (smaller on every channel)
       With dM = 1 everywhere the first-id rule gives, by hand: e0 and e2 receive every channel (D each), e1, e3, e4 nothing;
       dQ[1] = dQ[2] = 1 per channel, dQ[0] = 0; d_edge_attr = 1^T W_e on e0 and e2; dW_e = 1 (a_e0 + a_e2)^T.  torch's amax
       splits the ties in halves instead -- the rule this oracle exists to replace."""
    d, de = 3, 2
    Q = torch.tensor([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.5, -1.0, 4.0], [0, 0, 0], [0, 0, 0]], dtype=torch.float64)
    We = torch.tensor([[1.0, 0.5], [-0.25, 1.0], [0.75, -0.5]], dtype=torch.float64)
    ea = torch.tensor([[0.1, 0.2], [0.1, 0.2], [0.3, -0.1], [0.3, -0.1], [-5.0, -5.0]], dtype=torch.float64)
    src = torch.tensor([1, 0, 2, 2, 0])
    dst = torch.tensor([3, 3, 4, 4, 4])
    for chunk in (1, 2, 3, 1 << 18):                              # ties inside a chunk and across chunk boundaries
        M, win = GH.edge_max(Q, We, ea, src, dst, 5, chunk)
        assert win.tolist() == [[-1] * d] * 3 + [[0] * d, [2] * d]
        assert torch.equal(M[3], Q[1] + We @ ea[0]) and torch.equal(M[4], Q[2] + We @ ea[2])
        dM = torch.ones(5, d, dtype=torch.float64)
        dQ, dea, dWe = GH.edge_max_backward(dM, We, ea, src, dst, 5, win, chunk)
        routed = torch.zeros(5)
        for e in win[3:].reshape(-1).tolist():
            routed[e] += 1
        assert routed.tolist() == [d, 0, d, 0, 0]
        assert dQ.tolist() == [[0.0] * d, [1.0] * d, [1.0] * d, [0.0] * d, [0.0] * d]
        exp_dea = torch.zeros(5, de, dtype=torch.float64)
        exp_dea[0] = exp_dea[2] = We.sum(0)
        assert torch.equal(dea, exp_dea)
        assert torch.allclose(dWe, (ea[0] + ea[2]).expand(d, -1), rtol=0, atol=1e-15)
    # through autograd (the Function the hoisted model uses) and against torch's even split
    Qg, Weg, eag = Q.clone().requires_grad_(True), We.clone().requires_grad_(True), ea.clone().requires_grad_(True)
    M, _ = GH._EdgeMax.apply(Qg, Weg, eag, src, dst, 5, 2, None)
    M[3:].sum().backward()
    assert Qg.grad.tolist() == [[0.0] * d, [1.0] * d, [1.0] * d, [0.0] * d, [0.0] * d]
    Qs = Q.clone().requires_grad_(True)
    amax = torch.full((5, d), float("-inf"), dtype=torch.float64).scatter_reduce(0, dst.view(-1, 1).expand(-1, d),
                                                                                    Qs[src] + ea @ We.t(), "amax")
    amax[3:].sum().backward()
    assert Qs.grad[0].tolist() == [0.5] * d                          # (torch splits: the reason for the oracle above)


def test_tie_rule_through_the_hoisted_model():
    """A whole model on a graph with duplicate points and a duplicate edge: the oracle's gradients equal those of the same
    float64 evaluation with the winners chosen by hand (lowest id among the exact maxima, found element by element)."""
    n = 30
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n, 5, generator=g, dtype=torch.float64)
    x[1] = x[0]; x[7] = x[0]; x[12] = x[5]                         # duplicate points
    ei = random_graph(n, 150, seed=3)
    ei = torch.cat([ei, ei[:, :4]], 1)                             # duplicate edges (ids at the end: the originals come first)
    ea = torch.zeros(ei.shape[1], 2, dtype=torch.float64)          # attributes of the duplicates equal: exact ties
    ea[:, 0] = (x[ei[0], 0] - x[ei[1], 0]).abs()
    sd = random_sd("MPNNConv", "max", False, seed=9)
    found = []
    with torch.no_grad():
        GH.det_net_basic_hoisted_grad(x, ei, ea, sd, winners_out=found)
    # hand: per layer, recompute the messages, take the lowest id among the exact maxima
    xx = G.run_sequential(x, sd, "node_emb_mlp.")
    e_ = G.run_sequential(ea, sd, "edge_emb_mlp.")
    W = sd["convs.0.pre_mlp.0.weight"]
    c = xx.shape[1]
    v = xx[ei[0]] @ W[:, c:2 * c].t() + e_ @ W[:, 2 * c:].t()
    ties = 0
    for t in range(n):
        es = torch.nonzero(ei[1] == t).view(-1)
        if es.numel() == 0:
            continue
        for ch in range(v.shape[1]):
            col = v[es, ch]
            best = torch.nonzero(col == col.max()).view(-1)
            ties += int(best.numel() > 1)
            assert int(found[0][t, ch]) == int(es[best[0]])
    assert ties > 0


@pytest.mark.parametrize("n", [1, 257, 2000])
@pytest.mark.parametrize("kind", ["mixed", "background_only", "nan_box"])
def test_vectorised_loss_equals_the_per_node_oracle(n, kind):
    g = torch.Generator().manual_seed(n + len(kind))
    cls = torch.randn(n, 6, generator=g, dtype=torch.float64) * 2
    bb = torch.randn(n, 5, generator=g, dtype=torch.float64) * 2
    label = torch.randint(0, 6, (n, 1), generator=g).double()
    if kind == "background_only":
        label[:] = 5
    y = torch.cat([label, torch.randn(n, 5, generator=g, dtype=torch.float64) * 2], 1)
    if kind == "nan_box":
        label[0] = 1
        y[0, 0] = 1
        y[0, 3] = float("nan")
    for weights in (None, [1.0, 1.0, 1.0, 1.0, 1.0, 0.3]):
        got, exp = [], []
        for fn, out in ((L.detection_loss_vectorised, got), (L.detection_loss, exp)):
            c_, b_ = cls.clone().requires_grad_(True), bb.clone().requires_grad_(True)
            loss, lc, lb = fn(c_, b_, y, 5, weights, 1.0, 0.5)
            loss.backward()
            out += [loss.detach(), torch.as_tensor(lc).detach(), torch.as_tensor(lb, dtype=torch.float64).detach(), c_.grad,
                    torch.zeros_like(bb) if b_.grad is None else b_.grad]
        for a, b in zip(got, exp):
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), (kind, weights)
        if kind in ("background_only", "nan_box"):
            assert float(got[2]) == 0.0 and float(got[4].abs().max()) == 0.0


@pytest.mark.parametrize("delta", [0.25, 1.0, 3.0])
@pytest.mark.parametrize("weights", [None, [0.5, 2.0, 1.0, 3.0, 0.7, 0.1]])
def test_vectorised_loss_follows_ignore_index_fractional_labels_and_delta(delta, weights):
    """n = 300 with -100 labels (CrossEntropyLoss's ignore_index: out of the cross entropy's numerator and denominator, still an
    object row of the box term), labels with a fraction (``.long()`` truncates toward zero: 2.7 -> 2, -0.5 -> 0, 5.999 -> 5 =
    background) and residuals on both sides of every delta: values and gradients of the two oracles agree to 1e-12 relative."""
    n, k, w, bg = 300, 6, 5, 5
    g = torch.Generator().manual_seed(11)
    cls = torch.randn(n, k, generator=g, dtype=torch.float64) * 3
    bb = torch.randn(n, w, generator=g, dtype=torch.float64) * 2
    label = torch.randint(0, k, (n,), generator=g).double()
    label[::7] = -100.0
    label[1::7] = 2.7
    label[2::7] = -0.5
    label[3::7] = k - 1 + 0.999
    label[4::7] += 0.25
    y = torch.cat([label.view(-1, 1), torch.randn(n, w, generator=g, dtype=torch.float64) * 2], 1)
    a = (bb - y[:, 1:]).abs()
    assert bool((a < 0.25).any()) and bool((a > 3.0).any()) and int((label == -100).sum()) > 40
    got, exp = [], []
    for fn, out in ((L.detection_loss_vectorised, got), (L.detection_loss, exp)):
        c_, b_ = cls.clone().requires_grad_(True), bb.clone().requires_grad_(True)
        loss, lc, lb = fn(c_, b_, y, bg, weights, 0.75, 2.5, delta)
        loss.backward()
        out += [loss.detach(), lc.detach(), lb.detach(), c_.grad, b_.grad]
    for name, a_, b_ in zip(("loss", "loss_cls", "loss_bb", "d cls", "d bb"), got, exp):
        assert float((a_ - b_).abs().max()) <= 1e-12 * float(b_.abs().max()), (name, delta, weights)
    ignored = label == -100
    assert float(exp[3][ignored].abs().max()) == 0.0 and float(got[3][ignored].abs().max()) == 0.0      # no gradient to their logits
    assert bool((got[4][ignored].abs().sum(1) > 0).all())                                               # but they are object rows
    background = label.long() == bg
    assert float(got[4][background].abs().max()) == 0.0 and bool(background[3::7].all())
    if delta != 1.0:                                                # delta reaches both oracles (it is not the default's value)
        assert abs(float(exp[2]) - float(L.detection_loss(cls, bb, y, bg, weights, 0.75, 2.5)[2])) > 1e-3


def test_vectorised_loss_when_every_label_is_ignored():
    """Every label -100: 0 / 0 = NaN cross entropy in both oracles (torch's weighted mean over no row), a finite box term."""
    g = torch.Generator().manual_seed(12)
    cls, bb = torch.randn(40, 6, generator=g, dtype=torch.float64), torch.randn(40, 5, generator=g, dtype=torch.float64)
    y = torch.cat([torch.full((40, 1), -100.0, dtype=torch.float64), torch.randn(40, 5, generator=g, dtype=torch.float64)], 1)
    for weights in (None, [1.0, 1.0, 1.0, 1.0, 1.0, 0.3]):
        a = L.detection_loss_vectorised(cls, bb, y, 5, weights)
        b = L.detection_loss(cls, bb, y, 5, weights)
        assert bool(torch.isnan(a[1])) and bool(torch.isnan(b[1]))
        assert abs(float(a[2]) - float(b[2])) <= 1e-12 * float(b[2]) and float(b[2]) > 0
