"""Backward of BatchNorm with statistics per segment of rows (csrc/norm.hip: k_bn_seg_bwd<4>, k_bn_seg_bwd<1>, k_bn_seg_bwd_params;
``ops.batchnorm_segments_bwd``) behind the forward ``ops.batchnorm_act_segments(..., return_stats=True)``.

Reference: float64 torch autograd over a Python loop of per-segment ``F.batch_norm(training=True)`` (+ ``relu``).  Segments of one
row are left out of it (torch refuses them) and held to the exact values of the header: ``dh = 0``, their ``g`` goes to ``dbeta``,
nothing to ``dgamma``.

Bar: the one tests/test_gpu_bn_bwd_edges.py states for the whole-batch kernels -- norm-wise 4 x the error of float32 autograd on the
CPU + 2e-7 -- applied to ``dh`` per segment (m = the segment's rows) and to ``dgamma`` / ``dbeta`` over the call."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
EPS, MOM = 1e-5, 0.1
LENGTHS = [2, 3, 63, 64, 65, 127, 128, 129, 257, 1]
WIDTHS = [1, 5, 33, 64, 65, 224]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    from radargnn_amd import ops as o
    return o


def norm(a, b) -> float:
    return float((a.double().cpu() - b).abs().max() / b.abs().max())


def bits_equal(a, b) -> bool:
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


class Case:
    """Inputs of one call and its references (float64 and float32 autograd on the CPU), computed once."""

    def __init__(self, sizes, n, relu, seed, zero_gamma=True, constant=None, tensors=None):
        self.sizes, self.n, self.relu = list(sizes), n, relu
        self.seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        m = int(self.seg[-1])
        g = torch.Generator().manual_seed(seed)
        self.h = torch.randn(m, n, generator=g) * (torch.rand(n, generator=g) * 4 + 0.25) + torch.randn(n, generator=g) * 3
        if constant is not None:                               # a column that is constant inside one segment: var = 0
            s, c = constant
            self.h[int(self.seg[s]):int(self.seg[s + 1]), c] = 1.5
        self.dy = torch.randn(m, n, generator=g)
        self.gamma = torch.randn(n, generator=g) + 0.5
        if zero_gamma and n >= 5:
            self.gamma[n // 2] = 0.0                           # an exact 0: the statistics must not come from table / gamma
        self.beta = torch.randn(n, generator=g)
        if n < 5:
            self.gamma[0], self.beta[0] = 1.25, 0.1            # (a single column must not sit wholly on one side of the ReLU)
        if tensors is not None:
            self.h, self.dy, self.gamma, self.beta = tensors
        self.refs = {dt: self._autograd(dt) for dt in (torch.float64, torch.float32)}

    def _autograd(self, dt):
        h, gm, bt = (t.detach().clone().to(dt).requires_grad_(True) for t in (self.h, self.gamma, self.beta))
        outs, margin = [], float("inf")
        for a, b in zip(self.seg[:-1], self.seg[1:]):
            if b - a < 2:
                outs.append(None)
                continue
            z = F.batch_norm(h[a:b], None, None, gm, bt, True, MOM, EPS)
            margin = min(margin, float(z.detach().abs().min()))
            outs.append(torch.relu(z) if self.relu else z)
        live = [(o, a, b) for o, a, b in zip(outs, self.seg[:-1], self.seg[1:]) if o is not None]
        if live:
            torch.autograd.backward([o for o, _, _ in live], [self.dy[a:b].to(dt) for _, a, b in live])
        zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
        return {"dh": zero(h), "dgamma": zero(gm), "dbeta": zero(bt), "margin": margin}


def device_run(ops, case, wrap=lambda t: t, pool=False):
    h, dy = wrap(case.h.cuda()), wrap(case.dy.cuda())
    seg, gamma, beta = torch.from_numpy(case.seg).cuda(), case.gamma.cuda(), case.beta.cuda()
    y, stats = ops.batchnorm_act_segments(h, seg, gamma, beta, None, None, None, MOM, EPS, case.relu, return_stats=True)
    assert stats.shape == (len(case.sizes), 2, case.n) and stats.dtype == torch.float64
    dh, dgamma, dbeta = ops.batchnorm_segments_bwd(dy, y if case.relu else None, h, seg, stats, gamma, EPS)
    return y, dh, dgamma, dbeta


def check(case, y, dh, dgamma, dbeta, what):
    e64, e32 = case.refs[torch.float64], case.refs[torch.float32]
    if case.relu:
        assert e64["margin"] > 1e-6, (what, e64["margin"])     # no activation close enough to 0 for the mask to differ
    worst = 0.0
    extra_beta = torch.zeros(case.n, dtype=torch.float64)
    for s, (a, b) in enumerate(zip(case.seg[:-1], case.seg[1:])):
        a, b = int(a), int(b)
        if b - a == 0:
            continue
        if b - a == 1:                                         # the header's exact values
            assert bool((dh[a:b] == 0).all()), (what, s)
            g = case.dy[a:b].double()
            if case.relu:
                g = torch.where(y[a:b].cpu() > 0, g, torch.zeros_like(g))
            extra_beta += g[0]
            continue
        ref = e64["dh"][a:b]
        err, bar = norm(dh[a:b], ref), 4 * norm(e32["dh"][a:b], ref) + 2e-7
        worst = max(worst, err / bar)
        assert err < bar, (what, "dh", s, b - a, err, bar)
    if float(e64["dgamma"].abs().max()) > 0:
        for name, got, extra in (("dgamma", dgamma, 0.0), ("dbeta", dbeta, extra_beta)):
            ref = e64[name] + extra
            err, bar = norm(got, ref), 4 * norm(e32[name] + (extra if name == "dbeta" else 0.0), ref) + 2e-7
            worst = max(worst, err / bar)
            assert err < bar, (what, name, err, bar)
    else:                                                       # nothing but one-row and empty segments
        assert bool((dgamma == 0).all()) and norm(dbeta, extra_beta) < 2e-7
    print(f"[bn-seg-bwd] {what}: worst error / bar {worst:.3f}")


def padded(t):
    """``t`` as columns [3 : 3 + n] of a matrix 7 columns wider: a row stride above the width, NaN around, off the 16-byte grid."""
    w = torch.full((t.shape[0], t.shape[1] + 7), float("nan"), device=t.device)
    w[:, 3:3 + t.shape[1]] = t
    return w[:, 3:3 + t.shape[1]]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("n", WIDTHS)
def test_every_segment_length_at_every_width(ops, n, relu):
    """Lengths 2 ... 257 and 1 in one call: both sides of the 16- and 64-row-group seams; widths on both sides of the 64-channel
    slab and of the 16-byte form; gamma with an exact 0; a column that is constant inside one segment; contiguous operands and
    views with a row stride above the width."""
    case = Case(LENGTHS, n, relu, seed=100 + n, constant=(3, 0))
    y, dh, dgamma, dbeta = device_run(ops, case)
    check(case, y, dh, dgamma, dbeta, f"n {n} relu {relu}")
    y, dh, dgamma, dbeta = device_run(ops, case, wrap=padded)
    assert dh.is_contiguous() and dh.shape == case.h.shape
    check(case, y, dh, dgamma, dbeta, f"n {n} relu {relu} strided views")


MIXES = {"empty first, middle, last": [0, 5, 0, 70, 0], "300 segments of 2 rows": [2] * 300, "one segment": [500],
         "two equal segments": [130, 130], "only one-row and empty segments": [1, 0, 1]}


@pytest.mark.parametrize("mix", list(MIXES))
@pytest.mark.parametrize("n", [33, 64])
def test_segment_mixes(ops, mix, n):
    case = Case(MIXES[mix], n, True, seed=37 + n)
    check(case, *device_run(ops, case), f"{mix} n {n}")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("m,n", [(129, 65), (257, 64)])
def test_one_segment_equals_the_whole_batch_path(ops, m, n, relu):
    """One segment covering all rows against ``AG.batch_norm_act`` (rgnn_bn_bwd_stats / _coef / _apply) at the same bar, on the data
    tests/test_gpu_bn_bwd_edges.py holds that chain to the bar with (the integer matrices of tests/dense_bwd_cases.py, its seeds)."""
    import dense_bwd_cases as dc
    from radargnn_amd import gnn
    from radargnn_amd.gnn import autograd as AG
    c = dc.BnCase(m, n, "none")
    gen = torch.Generator().manual_seed(m + n)
    gamma, beta = torch.randn(n, generator=gen) + 0.5, torch.randn(n, generator=gen)
    tensors = (torch.from_numpy(c.h.astype(np.float32)), torch.from_numpy(c.dy.astype(np.float32)), gamma, beta)
    case = Case([m], n, relu, seed=0, tensors=tensors)
    y, dh, dgamma, dbeta = device_run(ops, case)
    check(case, y, dh, dgamma, dbeta, f"one segment m {m} n {n} relu {relu}")
    bn = gnn.BatchNorm(n).cuda().train()
    with torch.no_grad():
        bn.module.weight.copy_(case.gamma.cuda()); bn.module.bias.copy_(case.beta.cuda())
    h = case.h.cuda().requires_grad_(True)
    AG.batch_norm_act(h, bn, relu=relu).backward(case.dy.cuda())
    e64, e32 = case.refs[torch.float64], case.refs[torch.float32]
    for name, seg_form, whole in (("dh", dh, h.grad), ("dgamma", dgamma, bn.module.weight.grad), ("dbeta", dbeta, bn.module.bias.grad)):
        err, bar = norm(seg_form, whole.double().cpu()), 4 * norm(e32[name], e64[name]) + 2e-7
        print(f"[bn-seg-bwd] one segment against the whole-batch path, m {m} n {n} relu {relu} {name}: {err:.2e} (bar {bar:.2e})")
        assert err < bar, (name, err, bar)


def test_two_calls_give_the_same_bits(ops):
    case = Case(LENGTHS + [0, 300], 224, True, seed=9)
    first, second = device_run(ops, case), device_run(ops, case)
    for a, b in zip(first, second):
        assert bits_equal(a, b)
    first, second = device_run(ops, case, wrap=padded), device_run(ops, case, wrap=padded)     # the scalar form
    for a, b in zip(first, second):
        assert bits_equal(a, b)


@pytest.mark.parametrize("n,wrap", [(64, None), (33, None), (64, padded)])
def test_the_bound_is_the_exact_maximum(ops, n, wrap):
    """Inside a bound pool ``dh`` carries a bound whose maximum over the slots is ``dh.abs().max()`` bit for bit."""
    case = Case([5, 0, 300, 1, 64], n, True, seed=21)
    with ops.using_bounds(ops.BoundPool("cuda", 4)):
        _, dh, _, _ = device_run(ops, case, wrap=wrap or (lambda t: t))
        word = ops.bound_of(dh)
    assert word is not None and word.numel() == ops.BOUND_SLOTS
    assert bits_equal(word.max().reshape(1), dh.abs().max().reshape(1)) and float(word.max()) > 0
    assert ops.bound_of(device_run(ops, case)[1]) is None     # outside a pool: no bound


def test_shape_checks(ops):
    case = Case([4, 4], 8, False, seed=1)
    y, dh, _, _ = device_run(ops, case)
    h, dy, seg = case.h.cuda(), case.dy.cuda(), torch.from_numpy(case.seg).cuda()
    stats = torch.zeros(2, 2, 8, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        ops.batchnorm_segments_bwd(dy[:, :4], None, h, seg, stats, None, EPS)
    with pytest.raises(ValueError):
        ops.batchnorm_segments_bwd(dy, None, h, seg, stats[:1], None, EPS)
    with pytest.raises(TypeError):
        ops.batchnorm_segments_bwd(dy, None, h, seg, stats.float(), None, EPS)
