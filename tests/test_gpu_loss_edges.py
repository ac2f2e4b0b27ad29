"""The detection loss (csrc/loss.hip: k_loss_partial, k_loss_finish, k_loss_bwd; radargnn_amd/gnn/losses.py) and the row softmax
(csrc/norm.hip: k_softmax_rows) at the edges tests/test_gpu_loss.py does not reach: block and grid edges with the grid-stride
loop taken, logits at +-88, +-1e4 and -inf, labels that are ignored / fractional / weighted 0, the Huber seam for three deltas,
strided views, gradients arriving through ``loss_cls`` and ``loss_bb``, the empty batch and run-to-run bits.

Reference: the float64 evaluation of the same float32 inputs -- ``oracle.loss_oracle.detection_loss`` (the per-node restatement
with torch's own modules) up to a few hundred rows, ``detection_loss_vectorised`` (held to it in tests/test_oracle_backward.py)
above; ``torch.softmax(x.double(), 1)`` for the softmax.  Strided calls are held bit for bit to the same call on contiguous
copies.  ``alpha``, ``beta``, ``delta`` and the class weights used here are float32 numbers, so both sides see the same inputs.

Bars, from the arithmetic (eps32 = 2^-24, the relative error of one correctly rounded float32 operation):

* values: every float32 operation of ``m + logf(se) - c[label]`` rounds a number of size at most L = max|finite logit| + ln K;
  the sums run in double and a weighted mean cannot exceed the per-node bound: |loss_cls - ref| <= 8 eps32 L;
  |loss_bb - ref| <= 8 eps32 max(1, ref); loss: alpha and beta times those.
* d cls: D_max = max|c - lse| over the batch's finite entries; expf(c - lse) is off by at most eps32 (|c - lse| + 4) relative,
  so an entry is within sc eps32 (D_max + 8) with sc = that row's alpha w / sum w (exactly 0 where sc is 0).
* d bb: 4 eps32 relative (exactly 0 where the reference is 0: background rows, zero residuals).
* softmax: |y - ref| <= eps32 (|x - max| + n + 4) ref + 2^-126; a row sums to 1 within (n + 4) eps32.

Each test prints its largest error-to-bar ratio (``[loss-edges] ...``; MEASUREMENTS section 7, the trainer's loss, is where they are kept)."""
import math

import pytest
import torch

from oracle import loss_oracle

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
INF = float("inf")
ALPHA, BETA = 0.75, 2.5                                   # float32 numbers
WEIGHTS6 = [0.5, 2.0, 1.0, 3.0, 7.0, 0.125]              # float32 numbers; class 4's weight belongs to no other class
GRID_CAP_ROWS = 1024 * 256                                # k_loss_partial loops above this many rows
PER_NODE_ROWS = 300                                       # the per-node oracle up to here, the vectorised one above


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radargnn_amd.gnn import losses
    return losses


@pytest.fixture(scope="module")
def ops(L):
    from radargnn_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------------------- helpers
def make(n, k, w, bg, seed, scale=2.0, obj_frac=0.4):
    g = torch.Generator().manual_seed(seed)
    cls = torch.randn(n, k, generator=g) * scale
    bb = torch.randn(n, w, generator=g) * 1.5
    label = torch.where(torch.rand(n, generator=g) < obj_frac, torch.randint(0, k, (n,), generator=g), torch.full((n,), bg))
    y = torch.cat((label.float().view(-1, 1), torch.randn(n, w, generator=g) * 1.5), 1)
    return cls, bb, y


def combine_loss(outs):
    return outs[0]


def reference(cls, bb, y, bg, weights=None, alpha=1.0, beta=1.0, delta=1.0, combine=combine_loss):
    """float64 values and gradients of ``combine((loss, loss_cls, loss_bb))`` for the float32 inputs."""
    fn = loss_oracle.detection_loss if cls.shape[0] <= PER_NODE_ROWS else loss_oracle.detection_loss_vectorised
    c64, b64 = cls.double().requires_grad_(True), bb.double().requires_grad_(True)
    outs = fn(c64, b64, y.double(), bg, weights, alpha, beta, delta)
    outs = tuple(torch.as_tensor(o, dtype=torch.float64) for o in outs)
    total = combine(outs)
    if total.requires_grad:
        total.backward()
    zero = torch.zeros_like
    return {"loss": float(outs[0].detach()), "lc": float(outs[1].detach()), "lb": float(outs[2].detach()),
            "dc": zero(c64) if c64.grad is None else c64.grad, "db": zero(b64) if b64.grad is None else b64.grad}


def device(L, cls, bb, y, bg, weights=None, alpha=1.0, beta=1.0, delta=1.0, combine=combine_loss):
    c, b = cls.cuda().requires_grad_(True), bb.cuda().requires_grad_(True)
    outs = L.detection_loss(c, b, y.cuda(), bg, weights, alpha, beta, delta)
    assert all(o.dtype == torch.float32 and o.dim() == 0 for o in outs)
    combine(outs).backward()
    assert c.grad.shape == cls.shape and b.grad.shape == bb.shape
    return {"loss": float(outs[0].detach()), "lc": float(outs[1].detach()), "lb": float(outs[2].detach()), "dc": c.grad.cpu(),
            "db": b.grad.cpu()}


def row_scale(cls, y, weights, alpha):
    """sc of the d cls bar: alpha w / sum w per row (w = 0 for a label outside [0, K), as CrossEntropyLoss ignores -100)."""
    k = cls.shape[1]
    label = y[:, 0].double().long()                               # truncation toward zero, as the reference's .long()
    ok = (label >= 0) & (label < k)
    w = torch.ones(k, dtype=torch.float64) if weights is None else torch.tensor(weights, dtype=torch.float64)
    wi = torch.where(ok, w[label.clamp(0, k - 1)], torch.zeros((), dtype=torch.float64))
    return alpha * wi / wi.sum()


def logit_sizes(cls):
    """L and D_max of the bars."""
    c = cls.double()
    finite = torch.isfinite(c)
    size = float(c[finite].abs().max()) + math.log(cls.shape[1])
    d = (c - torch.logsumexp(c, 1, keepdim=True)).abs()
    return size, float(d[finite & torch.isfinite(d)].max())


def same_special(got, ref):
    """A non-finite reference value is met exactly (NaN by NaN, an infinity by the same infinity)."""
    return math.isnan(got) if math.isnan(ref) else got == ref


def check(name, got, ref, cls, y, weights, alpha, beta, cls_scale=None):
    """Values and both gradients of one call against the reference, at the bars of the module docstring.  ``cls_scale``: the
    per-row factor of d cls where the differentiated expression is not ``loss`` alone."""
    size, d_max = logit_sizes(cls)
    ratios = {}
    bar_c = 8 * EPS32 * size
    bar_b = 8 * EPS32 * max(1.0, ref["lb"]) if math.isfinite(ref["lb"]) else 0.0
    for key, bar in (("lc", bar_c), ("lb", bar_b), ("loss", alpha * bar_c + beta * bar_b)):
        if math.isfinite(ref[key]):
            ratios[key] = abs(got[key] - ref[key]) / bar
        else:
            assert same_special(got[key], ref[key]), (name, key, got[key], ref[key])
    sc = (row_scale(cls, y, weights, alpha) if cls_scale is None else cls_scale).view(-1, 1)
    known = torch.isfinite(ref["dc"]) & torch.isfinite(sc)
    err = (got["dc"].double() - ref["dc"]).abs()
    bar = (sc * EPS32 * (d_max + 8)).expand_as(err)
    assert bool(torch.isfinite(got["dc"][known]).all()), name
    assert bool((err[known & (bar == 0)] == 0).all()), name                       # weight 0 / ignored rows: exactly 0
    live = known & (bar > 0)
    ratios["dc"] = float((err[live] / bar[live]).max()) if bool(live.any()) else 0.0
    known = torch.isfinite(ref["db"])
    err = (got["db"].double() - ref["db"]).abs()
    assert bool(torch.isfinite(got["db"][known]).all()), name
    assert bool((got["db"][known & (ref["db"] == 0)] == 0).all()), name           # background rows, zero residuals: exactly 0
    live = known & (ref["db"] != 0)
    ratios["db"] = float((err[live] / (4 * EPS32 * ref["db"][live].abs())).max()) if bool(live.any()) else 0.0
    print(f"[loss-edges] {name}: error / bar " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for key, r in ratios.items():
        assert r <= 1.0, (name, key, r)                                            # (a NaN ratio fails too)
    return ratios


# --------------------------------------------------------------------------------------------- 1. block and grid edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_block_edges(L, n):
    cls, bb, y = make(n, 6, 5, 5, 100 + n)
    if n > 1:
        y[-1, 0] = 4.0                                            # the last row is an object of its own class
    args = (cls, bb, y, 5, WEIGHTS6, ALPHA, BETA)
    got, ref = device(L, *args), reference(*args)
    check(f"block edges n={n}", got, ref, cls, y, WEIGHTS6, ALPHA, BETA)
    if n > 1:
        assert float(got["db"][-1].abs().min()) > 0 and float(got["dc"][-1].abs().min()) > 0


@pytest.fixture(scope="module")
def beyond_the_grid_cap(L):
    """n = 1024 * 256 + 257: the grid is capped, k_loss_partial takes its loop.  The only object rows are the last 257 and the
    last row alone has label 4 (weight 7): a dropped tail shows as loss_bb = 0, a wrong sum w and zero gradient rows at the end.
    Inputs, the float64 reference and one device call, computed once for the tests below."""
    n, tail = GRID_CAP_ROWS + 257, 257
    g = torch.Generator().manual_seed(7)
    cls = torch.randn(n, 6, generator=g) * 2
    bb = torch.randn(n, 5, generator=g) * 1.5
    label = torch.full((n,), 5)
    label[-tail:] = torch.randint(0, 4, (tail,), generator=g)
    label[-1] = 4
    y = torch.cat((label.float().view(-1, 1), torch.randn(n, 5, generator=g) * 1.5), 1)
    args = (cls, bb, y, 5, WEIGHTS6, ALPHA, BETA)
    return args, reference(*args), device(L, *args)


def test_grid_stride_loop_and_its_tail(L, ops, beyond_the_grid_cap):
    (cls, bb, y, *_), ref, got = beyond_the_grid_cap
    n = cls.shape[0]
    assert int(ops.lib.rgnn_detection_loss_blocks(n)) == 1024 and n > 1024 * 256          # the loop is taken
    assert int(ops.lib.rgnn_detection_loss_blocks(GRID_CAP_ROWS)) == 1024 and int(ops.lib.rgnn_detection_loss_blocks(257)) == 2
    check(f"grid-stride loop n={n}", got, ref, cls, y, WEIGHTS6, ALPHA, BETA)
    assert got["lb"] > 0.1 and ref["lb"] > 0.1
    assert bool((got["db"][-257:].abs().sum(1) > 0).all()) and float(got["db"][:-257].abs().max()) == 0.0
    assert float(got["dc"][-1].abs().min()) > 0 and bool((got["dc"].abs().sum(1) > 0).all())


# --------------------------------------------------------------------------------------------------- 2. extreme logits
def planted_logits(k, g):
    """Rows (and their labels) at which a log-sum-exp goes wrong; ``k`` >= 2."""
    rows, labels = [], []
    r = torch.zeros(k); r[0], r[1] = 88.0, -88.0
    rows += [r, r.clone()]; labels += [0, 1]                                    # nll 0 and 176
    r = torch.zeros(k); r[0], r[1] = 1e4, -1e4
    rows += [r, r.clone()]; labels += [0, 1]                                    # nll 0 and 2e4: expf(c - lse) underflows
    rows += [torch.zeros(k), torch.full((k,), -1e4)]; labels += [k - 1, 0]      # all equal: nll = ln K at any offset
    r = torch.randn(k, generator=g) * 30; r[1] = -INF
    rows.append(r); labels.append(0)                                            # -inf beside the label column
    r = torch.randn(k, generator=g) * 30; r[0] = float(r.min()) - 200.0
    rows.append(r); labels.append(0)                                            # the label column 200 below the rest
    return torch.stack(rows), torch.tensor(labels)


@pytest.mark.parametrize("k", [2, 6, 11])
def test_extreme_logits(L, k):
    n, w, bg = 257, 4, k - 1
    cls, bb, y = make(n, k, w, bg, 200 + k, scale=30.0)
    rows, labels = planted_logits(k, torch.Generator().manual_seed(k))
    at = torch.arange(rows.shape[0]) * 31 + 3                                    # spread over the blocks and waves
    cls[at] = rows
    y[at, 0] = labels.float()
    weights = [0.25 + 0.125 * i for i in range(k)]
    args = (cls, bb, y, bg, weights, ALPHA, BETA)
    got, ref = device(L, *args), reference(*args)
    assert math.isfinite(ref["lc"]) and bool(torch.isfinite(ref["dc"]).all()) and ref["lc"] > 2e4 * 0.25 / (1.75 * n)
    check(f"extreme logits K={k}", got, ref, cls, y, weights, ALPHA, BETA)
    assert math.isfinite(got["loss"]) and bool(torch.isfinite(got["dc"]).all())
    hole = torch.isneginf(cls)
    assert int(hole.sum()) == 1 and float(got["dc"][hole].abs().max()) == 0.0 and float(ref["dc"][hole].abs().max()) == 0.0


def test_minus_infinity_in_the_label_column(L):
    cls, bb, y = make(257, 6, 4, 5, 9, scale=30.0)
    y[100, 0] = 2.0
    cls[100, 2] = -INF
    loss, lc, lb = L.detection_loss(cls.cuda(), bb.cuda(), y.cuda(), 5, WEIGHTS6, ALPHA, BETA)
    ref = loss_oracle.detection_loss(cls.double(), bb.double(), y.double(), 5, WEIGHTS6, ALPHA, BETA)
    assert float(ref[1]) == INF and float(ref[0]) == INF
    assert float(lc) == INF and float(loss) == INF
    assert abs(float(lb) - float(ref[2])) <= 8 * EPS32 * max(1.0, float(ref[2]))


# ------------------------------------------------------------------------------------------------------------ 3. labels
def test_ignored_and_fractional_labels(L):
    n, k, w, bg = 64, 6, 5, 5
    cls, bb, y = make(n, k, w, bg, 31)
    planted = {0: -100.0, 1: 2.7, 2: -0.5, 3: k - 1 + 0.999, 17: -100.0, 40: 2.7, 63: -100.0}
    for r, v in planted.items():
        y[r, 0] = v
    args = (cls, bb, y, bg, WEIGHTS6, ALPHA, BETA)
    got, ref = device(L, *args), reference(*args)
    check("labels -100 / 2.7 / -0.5 / K-1+0.999", got, ref, cls, y, WEIGHTS6, ALPHA, BETA)
    for r, v in planted.items():
        if v == -100.0:                       # out of the cross entropy, still an object of the box term
            assert float(got["dc"][r].abs().max()) == 0.0 and float(ref["dc"][r].abs().max()) == 0.0
            assert float(got["db"][r].abs().min()) > 0 and float(ref["db"][r].abs().min()) > 0
    # .long() truncates toward zero: the rows equal those of the integer labels 2, 0 and K - 1 (= background: no box gradient)
    y_int = y.clone()
    y_int[:, 0] = torch.where(y[:, 0] == -100.0, y[:, 0], y[:, 0].double().long().float())
    assert y_int[1, 0] == 2 and y_int[2, 0] == 0 and y_int[3, 0] == k - 1
    twin = device(L, cls, bb, y_int, bg, WEIGHTS6, ALPHA, BETA)
    for key in ("loss", "lc", "lb"):
        assert twin[key] == got[key]
    assert torch.equal(twin["dc"], got["dc"]) and torch.equal(twin["db"], got["db"])
    assert float(got["db"][3].abs().max()) == 0.0 and float(got["dc"][1, 2]) < 0 and float(got["dc"][2, 0]) < 0


def test_every_label_ignored(L):
    cls, bb, y = make(64, 6, 5, 5, 32)
    y[:, 0] = -100.0
    args = (cls, bb, y, 5, WEIGHTS6, ALPHA, BETA)
    got, ref = device(L, *args), reference(*args)
    assert math.isnan(ref["lc"]) and math.isnan(ref["loss"]) and math.isfinite(ref["lb"]) and ref["lb"] > 0
    assert math.isnan(got["lc"]) and math.isnan(got["loss"])
    assert abs(got["lb"] - ref["lb"]) <= 8 * EPS32 * max(1.0, ref["lb"])
    err = (got["db"].double() - ref["db"]).abs()
    assert bool((ref["db"] != 0).all()) and bool((err <= 4 * EPS32 * ref["db"].abs()).all())


def test_zero_class_weights(L):
    n, k, bg = 64, 6, 5
    cls, bb, y = make(n, k, 5, bg, 33, obj_frac=0.6)
    weights = [0.5, 2.0, 0.0, 3.0, 7.0, 0.125]
    rows = y[:, 0] == 2
    assert int(rows.sum()) >= 3
    args = (cls, bb, y, bg, weights, ALPHA, BETA)
    got, ref = device(L, *args), reference(*args)
    check("class weight 0 on a present class", got, ref, cls, y, weights, ALPHA, BETA)
    assert float(got["dc"][rows].abs().max()) == 0.0 and float(got["db"][rows].abs().min()) > 0
    args = (cls, bb, y, bg, [0.0] * k, ALPHA, BETA)
    got, ref = device(L, *args), reference(*args)
    assert math.isnan(ref["lc"]) and math.isnan(got["lc"]) and math.isnan(got["loss"])            # 0 / 0, like torch
    assert abs(got["lb"] - ref["lb"]) <= 8 * EPS32 * max(1.0, ref["lb"])


# -------------------------------------------------------------------------------------------------------- 4. Huber seam
def seam_residuals(delta, big):
    d = torch.tensor(delta, dtype=torch.float32)
    zero, inf = torch.tensor(0.0), torch.tensor(INF)
    vals = [zero, d, -d, torch.nextafter(d, zero), torch.nextafter(-d, zero), torch.nextafter(d, inf), torch.nextafter(-d, -inf)]
    if big:
        vals += [torch.tensor(1e30), torch.tensor(-1e30)]
    return torch.stack(vals)


@pytest.mark.parametrize("w", [1, 4, 5])
@pytest.mark.parametrize("delta", [0.25, 1.0, 3.0])
def test_huber_seam(L, delta, w):
    """Residuals set exactly (the box targets are 0): 0, +-delta, one ulp inside and outside, +-1e30.  The forward takes the
    quadratic branch at |r| <= delta, the backward clamps: value and derivative are continuous there, so both must agree with
    torch's HuberLoss(delta) in float64.  Once without the +-1e30 entries, whose size would hide the seam in the value."""
    n, k, bg = 65, 6, 5
    for big in (False, True):
        cls, bb, y = make(n, k, w, bg, 400 + w, obj_frac=0.8)
        y[:, 1:] = 0.0
        vals = seam_residuals(delta, big)
        bb = vals[(torch.arange(n * w) * 5) % vals.numel()].view(n, w).clone()          # 5 is coprime to 7 and 9
        obj = y[:, 0] != bg
        assert all(bool((bb[obj] == v).any()) for v in vals) and bool((~obj).any())
        args = (cls, bb, y, bg, WEIGHTS6, ALPHA, BETA, delta)
        got, ref = device(L, *args), reference(*args)
        check(f"huber seam delta={delta} W={w} big={big}", got, ref, cls, y, WEIGHTS6, ALPHA, BETA)
        sb = BETA / (int(obj.sum()) * w)
        at = obj.view(-1, 1) & (bb.abs() >= delta)                  # at and beyond the seam: +-sb delta
        assert bool(((got["db"][at].double().abs() - sb * delta).abs() <= 4 * EPS32 * sb * delta).all())
        assert bool((got["db"][bb == 0] == 0).all())


@pytest.mark.parametrize("delta", [0.25, 1.0, 3.0])
def test_huber_infinite_residual(L, delta):
    n, k, w, bg = 65, 6, 5, 5
    cls, bb, y = make(n, k, w, bg, 41)
    y[:, 1:] = 0.0
    y[7, 0] = 1.0
    bb[7, 2] = INF
    obj = y[:, 0] != bg
    args = (cls, bb, y, bg, WEIGHTS6, ALPHA, BETA, delta)
    got, ref = device(L, *args), reference(*args)
    assert ref["lb"] == INF and got["lb"] == INF and got["loss"] == INF            # inf, not 0: only a NaN box term is dropped
    sb = BETA / (int(obj.sum()) * w)
    assert abs(float(got["db"][7, 2]) - sb * delta) <= 4 * EPS32 * sb * delta
    assert bool(torch.isfinite(got["db"]).all()) and bool(torch.isfinite(ref["db"]).all())
    check(f"huber +inf residual delta={delta}", got, ref, cls, y, WEIGHTS6, ALPHA, BETA)


# ----------------------------------------------------------------------------------------------------------- 5. strides
def call_with_grads(L, cls, bb, y, bg, weights, delta=1.0):
    """One call on (views of) device tensors; gradients with respect to ``cls`` and ``bb`` as given."""
    loss, lc, lb = L.detection_loss(cls, bb, y, bg, weights, ALPHA, BETA, delta)
    dc, db = torch.autograd.grad(loss, [cls, bb])
    return [loss.detach().cpu(), lc.detach().cpu(), lb.detach().cpu(), dc.cpu(), db.cpu()]


def bitwise(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n,w", [(65, 5), (257, 4), (1, 5), (65, 1)])
def test_strided_views_equal_contiguous_copies(L, n, w):
    k, bg = 6, 5
    g = torch.Generator().manual_seed(50 + n + w)
    Z = torch.randn(n, 16, generator=g) * 2
    Y = torch.randn(n, w + 4, generator=g) * 1.5
    Y[:, 1] = torch.randint(0, k, (n,), generator=g).float()
    Y[0, 1] = 2.0
    weights = WEIGHTS6
    cls_c, bb_c, y_c = Z[:, :k].contiguous(), Z[:, k:k + w].contiguous(), Y[:, 1:2 + w].contiguous()
    ref = reference(cls_c, bb_c, y_c, bg, weights, ALPHA, BETA)
    base = call_with_grads(L, cls_c.cuda().requires_grad_(True), bb_c.cuda().requires_grad_(True), y_c.cuda(), bg, weights)
    got = dict(zip(("loss", "lc", "lb"), (float(v) for v in base[:3])), dc=base[3], db=base[4])
    check(f"contiguous twin n={n} W={w}", got, ref, cls_c, y_c, weights, ALPHA, BETA)

    Zd = Z.cuda().requires_grad_(True)
    Yd = Y.cuda()
    cls_v, bb_v, y_v = Zd[:, :k], Zd[:, k:k + w], Yd[:, 1:2 + w]
    assert cls_v.stride() == (16, 1) and bb_v.stride(0) == 16 and y_v.stride(0) == w + 4
    if n > 1:
        assert not cls_v.is_contiguous() and not bb_v.is_contiguous() and not y_v.is_contiguous()
    views = call_with_grads(L, cls_v, bb_v, y_v, bg, weights)
    assert views[3].shape == (n, k) and views[4].shape == (n, w)
    assert bitwise(views, base)

    cm = lambda t: t.t().contiguous().t()                       # column-major: stride(1) != 1, copied by ops._rowmajor
    cls_m, bb_m, y_m = cm(cls_c.cuda()).requires_grad_(True), cm(bb_c.cuda()).requires_grad_(True), cm(y_c.cuda())
    if n > 1:
        assert cls_m.stride(1) != 1 and y_m.stride(1) != 1
    col = call_with_grads(L, cls_m, bb_m, y_m, bg, weights)
    assert col[3].shape == (n, k) and col[4].shape == (n, w)
    assert bitwise(col, base)


def test_integer_and_double_targets(L):
    """``losses.detection_loss`` converts ``y``: int64 and float64 targets give the bits of the float32 ones."""
    n, k, w, bg = 65, 6, 5, 5
    g = torch.Generator().manual_seed(61)
    cls, bb = torch.randn(n, k, generator=g) * 2, torch.randn(n, w, generator=g) * 3
    y_int = torch.cat((torch.randint(0, k, (n, 1), generator=g), torch.randint(-3, 4, (n, w), generator=g)), 1)
    assert y_int.dtype == torch.int64
    _, _, y32 = make(n, k, w, bg, 62)
    for other, plain in ((y_int, y_int.float()), (y32.double(), y32)):
        a = call_with_grads(L, cls.cuda().requires_grad_(True), bb.cuda().requires_grad_(True), other.cuda(), bg, WEIGHTS6)
        b = call_with_grads(L, cls.cuda().requires_grad_(True), bb.cuda().requires_grad_(True), plain.cuda(), bg, WEIGHTS6)
        assert bitwise(a, b)
        ref = reference(cls, bb, plain, bg, WEIGHTS6, ALPHA, BETA)
        got = dict(zip(("loss", "lc", "lb"), (float(v) for v in a[:3])), dc=a[3], db=a[4])
        check(f"targets as {other.dtype}", got, ref, cls, plain, WEIGHTS6, ALPHA, BETA)


# -------------------------------------------------------------------------------------- 6. other outputs and empty input
@pytest.mark.parametrize("g_loss,g_cls,g_bb", [(0.0, 2.0, 3.0), (1.0, 0.5, 0.0)])
def test_gradients_through_loss_cls_and_loss_bb(L, g_loss, g_cls, g_bb):
    """``g_loss * loss + g_cls * loss_cls + g_bb * loss_bb`` through autograd on both sides.  The device adds one launch per
    output with a gradient: the bars are those of the launches plus one rounding of their sum (d cls: sc of a launch is
    g * (alpha, 1 or 0) * w / sum w; d bb: one launch alone is non-zero in both cases, so 4 eps32 stands)."""
    n, k, w, bg = 65, 6, 5, 5
    cls, bb, y = make(n, k, w, bg, 71)

    def combine(outs):
        total = 0
        for gq, o in zip((g_loss, g_cls, g_bb), outs):
            if gq != 0:
                total = total + gq * o
        return total

    args = (cls, bb, y, bg, WEIGHTS6, ALPHA, BETA, 1.0, combine)
    got, ref = device(L, *args), reference(*args)
    _, d_max = logit_sizes(cls)
    scale = row_scale(cls, y, WEIGHTS6, 1.0) * (g_loss * ALPHA + g_cls)
    scale = scale + ref["dc"].abs().max(1).values / (d_max + 8)          # + eps32 |d cls|: one rounding of the launches' sum
    check(f"outputs weighted {g_loss}, {g_cls}, {g_bb}", got, ref, cls, y, WEIGHTS6, ALPHA, BETA, cls_scale=scale)
    assert float(ref["db"].abs().max()) > 0 and float(ref["dc"].abs().max()) > 0


def test_empty_batch(L):
    k, w = 6, 5
    empty = lambda cols: torch.zeros(0, cols)
    ref = loss_oracle.detection_loss(empty(k).double(), empty(w).double(), empty(1 + w).double(), 5, WEIGHTS6)
    assert math.isnan(float(ref[0])) and math.isnan(float(ref[1])) and float(ref[2]) == 0.0
    c, b = empty(k).cuda().requires_grad_(True), empty(w).cuda().requires_grad_(True)
    loss, lc, lb = L.detection_loss(c, b, empty(1 + w).cuda(), 5, WEIGHTS6, ALPHA, BETA)
    assert math.isnan(float(loss.detach())) and math.isnan(float(lc.detach())) and float(lb.detach()) == 0.0
    loss.backward()
    assert c.grad is None or c.grad.shape == (0, k)
    assert b.grad is None or b.grad.shape == (0, w)
    c2, b2 = empty(k).cuda().requires_grad_(True), empty(w).cuda().requires_grad_(True)
    outs = L.detection_loss(c2, b2, empty(1 + w).cuda(), 5)
    (2 * outs[1] + 3 * outs[2]).backward()
    assert c2.grad is None or c2.grad.shape == (0, k)
    assert b2.grad is None or b2.grad.shape == (0, w)


# ------------------------------------------------------------------------------------------------------- 7. determinism
def test_two_calls_give_the_same_bits(L, beyond_the_grid_cap):
    """No atomics, a fixed order of the partial sums: bit-identical values and gradients, the loop of the capped grid included."""
    args, _, first = beyond_the_grid_cap
    second = device(L, *args)
    for key in ("loss", "lc", "lb"):
        assert second[key] == first[key], key
    assert torch.equal(second["dc"], first["dc"]) and torch.equal(second["db"], first["db"])


# ------------------------------------------------------------------------------------------------------------- softmax
def softmax_rows_under_test(m, n):
    """[m, n]: rows at randn * 30 with, from the top, the planted rows of the loss tests, exact ties at the maximum, a near tie
    and an all -inf row (the first ``m`` rows of a 257-row matrix; with m = 1 the callers take the rows one by one)."""
    g = torch.Generator().manual_seed(1000 + n)
    x = torch.randn(257, n, generator=g) * 30
    rows = []
    if n >= 2:
        rows += [r for r in planted_logits(n, g)[0]]
        r = torch.randn(n, generator=g) * 30; r[0] = r[n - 1] = float(r.max()) + 1.0
        rows.append(r)                                                            # two maxima
        r = torch.randn(n, generator=g) * 30; r[n // 2:] = float(r.max()) + 0.5
        rows.append(r)                                                            # every column of the upper half
        r = torch.randn(n, generator=g) * 30; r[1] = 40.0; r[0] = float(torch.nextafter(torch.tensor(40.0), torch.tensor(0.0)))
        rows.append(r)                                                            # one ulp below the maximum, in front of it
    else:
        rows += [torch.tensor([88.0]), torch.tensor([-1e4]), torch.tensor([0.0]), torch.tensor([1e4])]
    rows.append(torch.full((n,), -INF))
    planted = torch.stack(rows)
    x[:planted.shape[0]] = planted
    return x[:m].clone() if m > 1 else x[:planted.shape[0] + 2].clone()


def check_softmax(name, x, got):
    m, n = x.shape
    assert got.shape == x.shape and got.dtype == torch.float32
    x64 = x.double()
    ref = torch.softmax(x64, 1)
    dead = torch.isneginf(x).all(1)
    assert bool(torch.isnan(got[dead]).all()) and bool(torch.isnan(ref[dead]).all())               # like torch
    xs, g, r = x64[~dead], got[~dead], ref[~dead]
    hole = torch.isneginf(xs)
    mx = xs.max(1, keepdim=True).values
    dist = torch.where(hole, torch.zeros_like(xs), (xs - mx).abs())
    bar = EPS32 * (dist + n + 4) * r + 2.0 ** -126
    err = (g.double() - r).abs()
    assert bool(torch.isfinite(g).all()), name
    ratio = float((err / bar).max()) if g.numel() else 0.0
    sums = float((g.double().sum(1) - 1).abs().max() / ((n + 4) * EPS32)) if g.numel() else 0.0
    print(f"[loss-edges] {name}: error / bar entries {ratio:.3f}, row sums {sums:.3f}")
    assert ratio <= 1.0 and sums <= 1.0, (name, ratio, sums)
    assert torch.equal(g.argmax(1), xs.argmax(1)), name                                            # the first maximal column
    top = g.max(1, keepdim=True).values
    assert bool((g[xs == mx] == top.expand_as(g)[xs == mx]).all()), name                           # tied maxima: the same bits
    assert bool((g[hole] == 0).all()), name


@pytest.mark.parametrize("n", [1, 2, 6, 11, 33])
@pytest.mark.parametrize("m", [1, 255, 256, 257])
def test_softmax_rows_edges(ops, m, n):
    x = softmax_rows_under_test(m, n)
    if m > 1:
        got = ops.softmax_rows(x.cuda()).cpu()
        if n >= 2:
            assert int(torch.isneginf(x).all(1).sum()) == 1 and int(((x == x.max(1, keepdim=True).values).sum(1) > 1).sum()) >= 4
    else:                                                        # every planted row as a one-row call
        got = torch.cat([ops.softmax_rows(x[i:i + 1].cuda()).cpu() for i in range(x.shape[0])])
    check_softmax(f"softmax m={m} n={n}", x, got)
    # views: columns 3 .. 3 + n of a wider matrix (m = 1: a row stride larger than the width), and column-major
    wide = torch.full((x.shape[0], n + 7), 5e4)
    wide[:, 3:3 + n] = x
    wide = wide.cuda()
    step = x.shape[0] if m > 1 else 1
    for i in range(0, x.shape[0], step):
        rows = slice(i, i + step)
        view = wide[rows, 3:3 + n]
        assert view.stride(0) == n + 7 and view.data_ptr() != wide.data_ptr()
        out = ops.softmax_rows(view)
        assert out.is_contiguous() and out.shape == view.shape
        assert torch.equal(out.cpu().view(torch.int32), got[rows].view(torch.int32))                # NaN rows too: the bits
        col = x[rows].cuda().t().contiguous().t()
        assert torch.equal(ops.softmax_rows(col).cpu().view(torch.int32), got[rows].view(torch.int32))
