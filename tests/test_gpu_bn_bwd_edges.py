"""The ReLU / BatchNorm backward kernels (csrc/backward.hip: k_relu_bwd, k_bn_bwd_stats, k_bn_bwd_apply<VEC>; csrc/norm.hip:
k_bn_bwd_coef, k_bn_bwd_coef4) on the hand-built cases of tests/dense_bwd_cases.py: integer data on which the partial sums and
dx = A g + B h + C are exact, so the kernels must return the int64 reference BIT FOR BIT at every mask (none, y with +0 / -0 / NaN /
a denormal, an apply table that lands on exactly 0), on both sides of the 32-row, 128-row and 64-column seams, of the VEC / scalar
switch and of the two coefficient kernels; the coefficients against the header's formula in float64."""
import numpy as np
import pytest
import torch

import dense_bwd_cases as dc

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    from radargnn_amd import ops as o
    return o


def cuda(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(dtype))).cuda()


def bits_equal(got, want):
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    return got.shape == want.shape and bool((got.view(torch.int32) == want.view(torch.int32)).all())


def assert_bits(got, want, what):
    if not bits_equal(got, want):
        g, w = got.detach().cpu(), want.detach().cpu()
        bad = g.contiguous().view(torch.int32) != w.contiguous().view(torch.int32)
        idx = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} differ, first at {idx}: {g[idx].item()!r} != {w[idx].item()!r}")


def off_grid(t, flat=False):
    """The same values at an address 4 bytes off the 16-byte grid: a matrix as columns [1 : 1 + n] of one 4 columns wider (the row
    stride stays a multiple of 4 floats where n is); ``flat`` (coef, table) or 1-D: behind one float of a flat buffer."""
    if t.dim() == 2 and not flat:
        w = torch.full((t.shape[0], t.shape[1] + 4), float("nan"), dtype=t.dtype, device=t.device)
        w[:, 1:1 + t.shape[1]] = t
        v = w[:, 1:1 + t.shape[1]]
    else:
        w = torch.full((t.numel() + 1,), float("nan"), dtype=t.dtype, device=t.device)
        w[1:] = t.reshape(-1)
        v = w[1:].view(t.shape)
    assert v.data_ptr() % 16 == 4 and bits_equal(v, t)
    return v


def in_wider(t, poison):
    """``t`` as columns [2 : 2 + n] of a matrix 5 columns wider: stride above the width; the other columns hold 3 or NaN."""
    w = torch.full((t.shape[0], t.shape[1] + 5), float("nan") if poison else 3.0, dtype=t.dtype, device=t.device)
    w[:, 2:2 + t.shape[1]] = t
    return w[:, 2:2 + t.shape[1]]


class DevBn:
    def __init__(self, c):
        self.c = c
        self.dy, self.h = cuda(c.dy), cuda(c.h)
        self.y = None if c.y is None else cuda(c.y)
        self.table = None if c.table is None else cuda(c.table)
        self.coef = cuda(c.coef)
        self.stats = torch.from_numpy(c.stats_reference().astype(np.float32))
        self.dx = torch.from_numpy(c.dx_reference().astype(np.float32))


# ------------------------------------------------------------------------------------------------ relu_bwd
@pytest.mark.parametrize("count", dc.RELU_COUNTS)
def test_relu_bwd_masks_and_tail(ops, count):
    """dx = where(y > 0, dy, +0) bit for bit at +0, -0, NaN and the smallest denormal of y, on both sides of the 4-wide groups and
    of a 256-thread block; the zero has a clear sign bit whatever dy holds."""
    rng = np.random.default_rng(count)
    y, keep = dc.special_y(rng, (count,))
    dy = rng.choice(np.array([1.0, -5.0, 3.0, np.nan, np.inf, -np.inf, -0.0], dtype=np.float32), size=count)
    want = np.where(keep, dy, np.float32(0.0)).astype(np.float32)
    got = ops.relu_bwd(cuda(dy), cuda(y))
    assert_bits(got, torch.from_numpy(want), f"count {count}")
    assert not np.signbit(got.cpu().numpy()[~keep]).any()


def test_relu_bwd_refuses_operands_off_the_16_byte_grid(ops):
    from radargnn_amd._lib import RgnnError
    dy, y = torch.ones(64, device="cuda"), torch.ones(64, device="cuda")
    for a, b in ((off_grid(dy), y), (dy, off_grid(y))):
        with pytest.raises(RgnnError, match="16-byte"):
            ops.relu_bwd(a, b)
    assert bits_equal(ops.relu_bwd(dy, y), dy)


# ------------------------------------------------------------------------------------------------ bn_bwd_stats
def run_stats(ops, d, wrap=lambda t: t):
    return ops.bn_bwd_stats(wrap(d.dy), None if d.y is None else wrap(d.y), wrap(d.h), table=d.table)


@pytest.mark.parametrize("m", dc.BN_M)
def test_bn_bwd_stats_is_exact(ops, m):
    """Every (m, n, mask): the [panels, 2, n] partials bit for bit -- also on column views with a stride above the width, and with
    NaN in the columns outside the views."""
    for n in dc.BN_N:
        for mask in dc.BN_MASKS:
            d = DevBn(dc.BnCase(m, n, mask))
            assert_bits(run_stats(ops, d), d.stats, f"m {m} n {n} {mask}")
            assert_bits(run_stats(ops, d, lambda t: in_wider(t, False)), d.stats, f"m {m} n {n} {mask} views")
            assert_bits(run_stats(ops, d, lambda t: in_wider(t, True)), d.stats, f"m {m} n {n} {mask} views in NaN")


@pytest.mark.parametrize("m,n", [(33, 3), (129, 65), (257, 64)])
def test_bn_bwd_stats_table_mask_equals_y_mask_for_a_real_forward(ops, m, n):
    c = dc.BnCase(m, n, "none")
    h, dy = cuda(c.h), cuda(c.dy)
    gen = torch.Generator().manual_seed(m)
    gamma, beta = (torch.randn(n, generator=gen) + 0.5).cuda(), torch.randn(n, generator=gen).cuda()
    table = ops.batchnorm_finalize(ops.column_stats(h), m, n, gamma, beta, None, None, None, True, 0.1, 1e-5)
    y = ops.apply_table_reference(h, table).to(F32)
    assert bool((y > 0).any()) and bool((y < 0).any())
    assert bits_equal(ops.bn_bwd_stats(dy, None, h, table=table), ops.bn_bwd_stats(dy, y, h))
    assert not bits_equal(ops.bn_bwd_stats(dy, None, h), ops.bn_bwd_stats(dy, y, h))


# ------------------------------------------------------------------------------------------------ bn_bwd_apply
def run_apply(ops, d, **moved):
    g = lambda k: moved.get(k, getattr(d, k))
    return ops.bn_bwd_apply(g("dy"), g("y"), g("h"), g("coef"), table=g("table"))


@pytest.mark.parametrize("m", dc.BN_M)
def test_bn_bwd_apply_is_exact(ops, m):
    for n in dc.BN_N:
        for mask in dc.BN_MASKS:
            d = DevBn(dc.BnCase(m, n, mask))
            assert_bits(run_apply(ops, d), d.dx, f"m {m} n {n} {mask}")


@pytest.mark.parametrize("m,n", [(33, 4), (257, 64), (129, 128), (97, 65)])
def test_bn_bwd_apply_vec_and_scalar_forms_agree_on_integers(ops, m, n):
    """One operand moved off the 16-byte grid (dy, h, y, coef, table in turn) takes the scalar form: equal bits, and no refusal."""
    for mask in dc.BN_MASKS:
        d = DevBn(dc.BnCase(m, n, mask))
        aligned = run_apply(ops, d)
        assert_bits(aligned, d.dx, f"{mask} aligned")
        for k in ("dy", "h", "y", "coef", "table"):
            if getattr(d, k) is None:
                continue
            assert_bits(run_apply(ops, d, **{k: off_grid(getattr(d, k), flat=k in ("coef", "table"))}), d.dx, f"m {m} n {n} {mask}: {k} off the grid")


@pytest.mark.parametrize("m,n", [(257, 64), (130, 128)])
def test_bn_bwd_apply_on_gaussian_data_stays_within_three_roundings(ops, m, n):
    """Both forms within 4 * 2^-24 * (|A g| + |B h| + |C|) per element of float64 (three roundings and a product, with or without
    contraction); whether their bits agree is printed, not asserted."""
    gen = torch.Generator().manual_seed(n)
    dy, h, y = (torch.randn(m, n, generator=gen).cuda() for _ in range(3))
    coef = torch.randn(3, n, generator=gen).cuda()
    g = torch.where(y > 0, dy, torch.zeros_like(dy)).double()
    A, B, C = coef.double()
    exp = A * g + B * h.double() + C
    bar = 4 * 2.0 ** -24 * ((A * g).abs() + (B * h.double()).abs() + C.abs())
    vec = ops.bn_bwd_apply(dy, y, h, coef)
    scalar = ops.bn_bwd_apply(off_grid(dy), y, h, coef)
    for name, got in (("VEC", vec), ("scalar", scalar)):
        excess = ((got.double() - exp).abs() - bar).max().item()
        assert excess <= 0, (name, excess)
    print(f"[bn_bwd_apply] m {m} n {n}: VEC and scalar bits agree on Gaussian data: {bits_equal(vec, scalar)}; "
          f"worst |err| / bar {(((vec.double() - exp).abs() / bar).max().item()):.3f}")


@pytest.mark.parametrize("m,n,waves", [(3, 4, 1), (300, 256, 300), (257, 65, None)])
def test_bn_bwd_apply_bound_is_the_exact_maximum(ops, m, n, waves):
    """Inside a bound pool the maximum over the 256 slots of the attached bound is dx.abs().max() bit for bit: one wave writes one
    slot (the rest stay 0); more than 256 waves wrap around the slots."""
    d = DevBn(dc.BnCase(m, n, "y"))
    with ops.using_bounds(ops.BoundPool("cuda", 2)):
        dx = run_apply(ops, d)
        word = ops.bound_of(dx)
    assert word is not None and word.numel() == dc.BOUND_SLOTS
    assert_bits(dx, d.dx, "dx")
    assert bits_equal(word.max().reshape(1), dx.abs().max().reshape(1)) and float(word.max()) > 0
    if waves == 1:
        assert int((word != 0).sum()) == 1 and float(word[0]) > 0
    elif waves is not None:
        blocks = dc.ceil_div(m * (n // 4), 256)
        assert blocks > 64 and blocks * 4 > dc.BOUND_SLOTS and blocks <= dc.APPLY_MAX_BLOCKS


# ------------------------------------------------------------------------------------------------ bn_bwd_coef
@pytest.mark.parametrize("n", dc.COEF_N)
def test_bn_bwd_coef_matches_the_formula(ops, n):
    """coef, dgamma, dbeta against the header's formula in float64: one float32 ulp of the reference plus 2^-40 of the absolute terms
    of its expression per value; in eval mode B = C = 0 bit for bit."""
    worst = 0.0
    for panels in dc.COEF_PANELS:
        for with_gamma in (True, False):
            for train in (True, False):
                c = dc.CoefCase(n, panels, with_gamma, train)
                gamma = None if c.gamma is None else cuda(c.gamma)
                coef, dgamma, dbeta = ops.bn_bwd_coef(cuda(c.fwd_stats) if train else None, None if train else cuda(c.running_mean),
                                                      None if train else cuda(c.running_var), cuda(c.bwd_part), c.m, gamma,
                                                      dc.COEF_EPS, train)
                got = {"A": coef[0], "B": coef[1], "C": coef[2], "dgamma": dgamma, "dbeta": dbeta}
                for name, (val, terms) in c.reference().items():
                    err = np.abs(got[name].double().cpu().numpy() - val)
                    bar = dc.coef_bar(val, terms)
                    worst = max(worst, float((err / bar).max()))
                    assert (err <= bar).all(), (n, panels, with_gamma, train, name, float((err / bar).max()))
                if not train:
                    zero = torch.zeros(n)
                    assert bits_equal(coef[1], zero) and bits_equal(coef[2], zero)
    print(f"[bn_bwd_coef] n {n}: worst error / bar {worst:.3f}")


# ------------------------------------------------------------------------------------------------ the chain
@pytest.mark.parametrize("m,n", [(129, 65), (257, 64)])
def test_bn_backward_chain_on_integers_matches_float64_autograd(ops, m, n):
    """bn_bwd_stats -> bn_bwd_coef -> bn_bwd_apply against float64 autograd of relu(batch_norm(h)), under the existing norm-wise bar:
    4 x the error of float32 autograd on the CPU + 2e-7."""
    c = dc.BnCase(m, n, "none")
    gen = torch.Generator().manual_seed(m + n)
    gamma, beta = torch.randn(n, generator=gen) + 0.5, torch.randn(n, generator=gen)
    h0, dy0 = torch.from_numpy(c.h.astype(np.float32)), torch.from_numpy(c.dy.astype(np.float32))

    def autograd(dt):
        h, g, b = (t.to(dt).requires_grad_(True) for t in (h0, gamma, beta))
        z = torch.nn.functional.batch_norm(h, None, None, g, b, True, 0.1, 1e-5)
        torch.relu(z).backward(dy0.to(dt))
        return z.detach(), h.grad, g.grad, b.grad

    z64, *exp = autograd(torch.float64)
    assert float(z64.abs().min()) > 1e-6                             # (no activation close enough to 0 for the mask to differ)
    _, *g32 = autograd(torch.float32)
    hd, dyd, gd, bd = h0.cuda(), dy0.cuda(), gamma.cuda(), beta.cuda()
    stats = ops.column_stats(hd)
    table = ops.batchnorm_finalize(stats, m, n, gd, bd, None, None, None, True, 0.1, 1e-5)
    part = ops.bn_bwd_stats(dyd, None, hd, table=table)
    coef, dgamma, dbeta = ops.bn_bwd_coef(stats, None, None, part, m, gd, 1e-5, True)
    dx = ops.bn_bwd_apply(dyd, None, hd, coef, table=table)
    norm = lambda a, b: float((a.double().cpu() - b).abs().max() / b.abs().max())
    for name, got, e64, e32 in zip(("dx", "dgamma", "dbeta"), (dx, dgamma, dbeta), exp, g32):
        err, bar = norm(got, e64), 4 * norm(e32, e64) + 2e-7
        print(f"[bn chain] m {m} n {n} {name}: {err:.2e} (bar {bar:.2e})")
        assert err < bar, (name, err, bar)
