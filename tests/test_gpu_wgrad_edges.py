"""The weight-gradient kernels (csrc/wgrad.hip: k_wgrad_x3 in the bf16x3 and the f16x2 form, the three k_wgrad_narrow instances,
k_wg_reduce) on the hand-built operands of tests/dense_bwd_cases.py: every output is a sum of integers below 2^24 in its sum of
|terms|, so the kernels must return the int64 reference BIT FOR BIT -- a dropped split product, a lost column, a stray read, a slab
or block that does not write its tile each fail an equality.  tests/test_dense_bwd_cases.py proves on the CPU that the cases are
what they say.  One float net at the end (Gaussian data, per-output error against float64) makes no new accuracy claim."""
import functools

import numpy as np
import pytest
import torch

import dense_bwd_cases as dc
from conftest import record_parity

pytestmark = pytest.mark.gpu
IDS = lambda c: c.name


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    from radargnn_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def operands(name, layout, a1_scale=1):
    return dc.Operands(dc.by_name(name), layout, a1_scale)


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


class Dev:
    """The operands of one launch on the device, as views into their wider matrices."""

    def __init__(self, op, poison=False, identity=False):
        c = op.case
        self.op = op
        self.wide = {k: cuda(op.wide(k, poison)) for k in ("g", "a1", "a2")}
        rows = op.rows_alloc if c.row_list is not None else c.m
        view = lambda k, w: self.wide[k][:rows, op.off[k][0]:op.off[k][0] + w]
        self.g, self.a1, self.a2 = view("g", c.n), view("a1", c.k1), (view("a2", c.k2) if c.k2 else None)
        lst = op.row_index_for(poison)
        self.row_index = None if lst is None else cuda(lst)
        self.m_dev = None if op.count is None else torch.tensor([op.count], dtype=torch.int64, device="cuda")
        if identity:
            assert lst is None
            self.row_index = torch.arange(c.m, dtype=torch.int32, device="cuda")


def wgrad(ops, d, ones, bounds=None):
    return ops.linear_wgrad(d.g, d.a1, d.a2, with_bias=ones, row_index=d.row_index, m_dev=d.m_dev, bounds=bounds)


def raw_wgrad(ops, d, ones, part_fill=None, bounds=(None, None, None)):
    """lib.rgnn_wgrad itself, with a partial buffer the caller may pre-fill."""
    from radargnn_amd._lib import lib
    c = d.op.case
    kt = c.k1 + c.k2 + (1 if ones else 0)
    slabs = int(lib.rgnn_wgrad_slabs(c.m, c.n, c.k1, c.k2, 1 if ones else 0))
    part = torch.full((slabs, c.n, kt), float("nan") if part_fill is None else part_fill, dtype=torch.float32, device="cuda")
    dw = torch.full((c.n, kt), 7.0, dtype=torch.float32, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()
    ld = lambda t: 0 if t is None else ops._ld(t)
    rc = lib.rgnn_wgrad(p(d.g), ld(d.g), c.n, p(d.a1) if c.k1 else None, ld(d.a1) if c.k1 else 0, c.k1, p(d.a2), ld(d.a2), c.k2,
                        1 if ones else 0, c.m, p(d.row_index), p(d.m_dev), p(bounds[0]), p(bounds[1]), p(bounds[2]), p(part), p(dw),
                        ops._stream())
    assert rc == 0, lib.rgnn_last_error().decode()
    return dw


def ref32(op, ones):
    ref = op.reference(ones)[0].astype(np.float64)
    r32 = ref.astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), ref)
    return torch.from_numpy(r32)


def assert_bits(got, want, what):
    got = got.detach().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(torch.int32) != want.contiguous().view(torch.int32)
    if bool(bad.any()):
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outputs differ, first at {idx}: "
                             f"{got[tuple(idx)].item()!r} != {want[tuple(idx)].item()!r}")


# ------------------------------------------------------------------------------------------------ exact, bf16x3 and narrow
@pytest.mark.parametrize("case", dc.GEOMETRY_CASES + dc.NARROW_CASES, ids=IDS)
def test_weight_gradient_is_exact(ops, case):
    """Every case in its layouts, with and without the bias column: the int64 reference bit for bit; the result without the bias
    column is the leading columns of the one with it; a repeat call returns the same bits."""
    for lay in case.layouts:
        op = operands(case.name, lay)
        d = Dev(op)
        with_b, without = wgrad(ops, d, True), wgrad(ops, d, False)
        assert_bits(with_b, ref32(op, True), f"{case.name}/{lay}/bias")
        assert_bits(without, ref32(op, False), f"{case.name}/{lay}")
        assert torch.equal(without, with_b[:, :-1])
        assert_bits(wgrad(ops, d, True), with_b.cpu(), f"{case.name}/{lay}/repeat")


@pytest.mark.parametrize("case", dc.K2_ONLY_CASES, ids=IDS)
def test_weight_gradient_without_a_first_block(ops, case):
    """k1 = 0 with A1 null, through the entry point itself."""
    for lay in case.layouts:
        op = operands(case.name, lay)
        d = Dev(op)
        for ones in (True, False):
            assert_bits(raw_wgrad(ops, d, ones), ref32(op, ones), f"{case.name}/{lay}/{ones}")


@pytest.mark.parametrize("case", dc.NARROW_CASES, ids=IDS)
def test_narrow_kernels_equal_the_mfma_kernel(ops, case):
    """An identity row list forces k_wgrad_x3: on integer data the two kernels return equal bits."""
    for lay in case.layouts:
        op = operands(case.name, lay)
        for ones in (False, True):
            direct = wgrad(ops, Dev(op), ones)
            forced = wgrad(ops, Dev(op, identity=True), ones)
            assert_bits(forced, direct.cpu(), f"{case.name}/{lay}/{ones}")
            assert_bits(forced, ref32(op, ones), f"{case.name}/{lay}/{ones}/reference")


# ------------------------------------------------------------------------------------------------ exact, f16x2
def f16_layouts(case):
    return ("small",) if len(case.layouts) == 1 else dc.LAYOUTS_F16


def make_bounds(ops, op, loose=1.0, slot=0, values=None):
    def one(v, present):
        if not present:
            return None
        b = torch.zeros(ops.BOUND_SLOTS, dtype=torch.float32, device="cuda")
        b[slot] = v * loose
        return b
    bg, b1, b2 = values if values is not None else op.bounds()
    if slot == 0 and loose == 1.0:                                  # (the library's own constructor where it applies)
        mk = lambda v, present: ops.make_bound(torch.tensor(v, dtype=torch.float32, device="cuda")) if present else None
        return mk(bg, True), mk(b1, op.case.k1 > 0), mk(b2, op.case.k2 > 0)
    return one(bg, True), one(b1, op.case.k1 > 0), one(b2, op.case.k2 > 0)


def wgrad_f16(ops, d, ones, bounds):
    before = ops.COUNTERS.get("wgrad_f16x2", 0)
    with ops.using_bounds(ops.BoundPool("cuda", 4)):
        out = wgrad(ops, d, ones, bounds=bounds)
    assert ops.COUNTERS.get("wgrad_f16x2", 0) - before == 1, "the launch did not take the f16x2 form"
    return out


@pytest.mark.parametrize("case", dc.GEOMETRY_CASES, ids=IDS)
def test_weight_gradient_f16x2_is_exact(ops, case):
    """The same geometry in the f16x2 form, bounds at the exact maxima: bit-exact, and the counter proves the path."""
    for lay in f16_layouts(case):
        op = operands(case.name, lay)
        d = Dev(op)
        bounds = make_bounds(ops, op)
        for ones in (True, False):
            assert_bits(wgrad_f16(ops, d, ones, bounds), ref32(op, ones), f"{case.name}/{lay}/{ones}")


BOUND_CASES = ("k64+63", "m129", "n65", "rows_short")


@pytest.mark.parametrize("name", BOUND_CASES)
def test_f16x2_bounds_loose_and_in_other_slots(ops, name):
    """A bound loose by 2 and by 2^8 only moves the pre-scale (still exact); the bound may sit in any of the 256 slots."""
    for lay in dc.LAYOUTS_F16:
        op = operands(name, lay)
        d = Dev(op)
        want = ref32(op, True)
        for loose in (2.0, 256.0):
            assert_bits(wgrad_f16(ops, d, True, make_bounds(ops, op, loose=loose)), want, f"{name}/{lay}/loose {loose}")
        for slot in (63, 64, 200, 255):
            assert_bits(wgrad_f16(ops, d, True, make_bounds(ops, op, slot=slot)), want, f"{name}/{lay}/slot {slot}")


def test_f16x2_zero_bound_on_a_zero_operand_gives_zero(ops):
    """Bound 0 (largest pre-scale) on an all-zero operand: 0, not NaN."""
    op = operands("k64+63", "small")
    bg, b1, b2 = op.bounds()
    d = Dev(op)
    d.wide["g"].zero_()
    out = wgrad_f16(ops, d, True, make_bounds(ops, op, values=(0.0, b1, b2)))
    assert_bits(out, torch.zeros_like(out).cpu(), "G = 0")
    d = Dev(op)
    d.wide["a1"].zero_(); d.wide["a2"].zero_()
    out = wgrad_f16(ops, d, True, make_bounds(ops, op, values=(bg, 0.0, 0.0)))
    want = ref32(op, True).clone()
    want[:, :-1] = 0.0                                               # (the bias column is the column sum of G, whatever A holds)
    assert_bits(out, want, "A = 0")


def test_f16x2_blocks_whose_bounds_are_2_10_apart(ops):
    for lay in ("small", "low_g16"):
        op = operands("k64+63", lay, 1024)
        for ones in (True, False):
            assert_bits(wgrad_f16(ops, Dev(op), ones, make_bounds(ops, op)), ref32(op, ones), f"{lay}/{ones}")


# ------------------------------------------------------------------------------------------------ containment
POISON_CASES = [c for c in dc.GEOMETRY_CASES + dc.NARROW_CASES if c.m <= 5000]


@pytest.mark.parametrize("case", POISON_CASES, ids=IDS)
def test_nothing_outside_the_operands_is_read(ops, case):
    """NaN in every row the launch does not select (the unused tail of a row list names such a row), in every column of the wider
    matrices outside the views, in the rows between M and the next multiple of 16: the result does not move."""
    for lay in [l for l in ("small", "low_g") if l in case.layouts]:
        op = operands(case.name, lay)
        d = Dev(op, poison=True)
        if case.row_list is not None or case.views or case.m % dc.STEP:
            assert any(bool(torch.isnan(w).any()) for w in d.wide.values())
        for ones in (True, False):
            clean = wgrad(ops, Dev(op), ones)
            assert_bits(wgrad(ops, d, ones), clean.cpu(), f"{case.name}/{lay}/{ones}/poison")
            assert_bits(clean, ref32(op, ones), f"{case.name}/{lay}/{ones}")


@pytest.mark.parametrize("name", ["m1", "m33", "m257", "m385", "m2049_n129", "rows_sparse", "rows_count0", "rows_count17", "k192+64",
                                  "narrow_m1", "narrow_m1025", "narrow_m16385", "narrow_m32769", "class_n32_kt6", "width65"])
def test_every_slab_and_block_writes_its_whole_tile(ops, name):
    """``partial`` pre-filled with NaN: dW is still exact, so every slab (the empty ones included) and every block of the narrow
    launch writes all of its tile before k_wg_reduce reads it."""
    op = operands(name, "small")
    d = Dev(op)
    for ones in (True, False):
        assert_bits(raw_wgrad(ops, d, ones, part_fill=float("nan")), ref32(op, ones), f"{name}/{ones}")
    if op.case.row_list is None and op.case.kernel(True) == "x3":
        bounds = make_bounds(ops, op)
        assert_bits(raw_wgrad(ops, d, True, part_fill=float("nan"), bounds=bounds), ref32(op, True), f"{name}/f16x2")


# ------------------------------------------------------------------------------------------------ non-finite operands
@pytest.mark.parametrize("name", ["k64+63", "rows_short", "class_n16_kt9", "class_n8_kt17"])
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_a_non_finite_operand_stays_in_its_row_or_column(ops, name, bad):
    op = operands(name, "small")
    c = op.case
    ones = c.ones                                                   # (the stated form: the narrow cases stay narrow)
    want = ref32(op, ones)
    r = int(op.eff[len(op.eff) // 2])                               # a row the launch reads
    j, col = c.n - 1, (c.k1 - 1 if c.k2 == 0 else c.k1)             # (the first column of A2 where there is one)
    d = Dev(op)
    d.g[r, j] = bad
    out = wgrad(ops, d, ones).cpu()
    assert not torch.isfinite(out[j]).any(), "row j of dW must be non-finite throughout"
    keep = torch.ones(c.n, dtype=torch.bool); keep[j] = False
    assert_bits(out[keep], want[keep], f"{name}: G[{r}, {j}] = {bad}")
    d = Dev(op)
    (d.a1 if col < c.k1 else d.a2)[r, col if col < c.k1 else col - c.k1] = bad
    out = wgrad(ops, d, ones).cpu()
    assert not torch.isfinite(out[:, col]).any(), "column c of dW must be non-finite throughout"
    keep = torch.ones(want.shape[1], dtype=torch.bool); keep[col] = False
    assert_bits(out[:, keep], want[:, keep], f"{name}: A[{r}, {col}] = {bad}")


# ------------------------------------------------------------------------------------------------ refusals and empties
def test_refusals_and_empties(ops):
    from radargnn_amd._lib import lib
    n, k1 = 6, 8
    G = torch.ones((4, n), device="cuda"); A = torch.ones((4, k1), device="cuda")
    part = torch.empty((512, n, k1 + 1), device="cuda")
    lst = torch.arange(4, dtype=torch.int32, device="cuda")
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    p = lambda t: t.data_ptr()

    def call(ldg=n, nn=n, kk=k1, ones=1, m=4, rows=None, m_dev=None):
        dW = torch.full((n, k1 + 1), 7.0, device="cuda")
        rc = lib.rgnn_wgrad(p(G), ldg, nn, p(A), k1, kk, None, 0, 0, ones, m, rows, m_dev, None, None, None, p(part), p(dW), None)
        torch.cuda.synchronize()
        return rc, dW

    rc, dW = call(m=0)
    assert rc == 0 and float(dW.abs().max()) == 0.0                               # m = 0: the sum over nothing
    rc, dW = call(rows=p(lst), m_dev=p(zero))
    assert rc == 0 and float(dW.abs().max()) == 0.0                               # m_dev = 0: likewise, by the kernels
    assert torch.equal(ops.linear_wgrad(G[:0], A[:0], with_bias=True), torch.zeros((n, k1 + 1), device="cuda"))
    assert torch.equal(ops.linear_wgrad(G, A, with_bias=True, row_index=lst, m_dev=zero), torch.zeros((n, k1 + 1), device="cuda"))
    rc, dW = call(nn=0)
    assert rc == 0 and bool((dW == 7.0).all())                                    # n = 0: OK, nothing written
    rc, dW = call(kk=0, ones=0)
    assert rc == 0 and bool((dW == 7.0).all())                                    # Kt = 0: likewise
    rc, dW = call(m_dev=p(zero))
    assert rc != 0 and b"m_dev" in lib.rgnn_last_error() and bool((dW == 7.0).all())     # m_dev without row_index: refused
    from radargnn_amd._lib import RgnnError
    with pytest.raises(RgnnError):
        ops.linear_wgrad(G, A, with_bias=True, m_dev=zero)
    # a row stride of 2^29 floats (2 GiB): refused before anything is launched -- but behind the m = 0 early return, which wins
    rc, dW = call(ldg=1 << 29)
    assert rc != 0 and b"stride" in lib.rgnn_last_error() and bool((dW == 7.0).all())
    rc, dW = call(ldg=1 << 29, m=0)
    assert rc == 0 and float(dW.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ one float net
@pytest.mark.parametrize("label,m,n,k1,k2,ones", [("k64+63 with bias", 1000, 40, 64, 63, True), ("n129", 1000, 129, 40, 0, True),
                                                  ("narrow 16 x 9", 1000, 16, 9, 0, False)])
def test_gaussian_outputs_stay_within_the_float32_rule(ops, label, m, n, k1, k2, ones):
    """No new accuracy claim: each output's error against float64 over ITS OWN sum |G||A|, worst output, under the project's rule --
    4 x the same ratio of a float32 product computed by torch on the CPU, plus 2e-7."""
    gen = torch.Generator().manual_seed(n + k1)
    G = torch.randn(m, n, generator=gen)
    A = torch.randn(m, k1 + k2, generator=gen)
    full = torch.cat([A] + ([torch.ones(m, 1)] if ones else []), 1)
    exp = G.double().t() @ full.double()
    mass = G.double().abs().t() @ full.double().abs()
    ratio = lambda got: float(((got.double() - exp).abs() / mass).max())
    r32 = ratio(G.t() @ full)
    bar = 4 * r32 + 2e-7
    Gd, Ad = G.cuda(), A.cuda()
    got = ops.linear_wgrad(Gd, Ad[:, :k1], Ad[:, k1:] if k2 else None, with_bias=ones).cpu()
    r = ratio(got)
    record_parity(f"wgrad edges, gaussian {label}", kernel=r, torch_fp32=r32, bar=bar)
    assert r < bar, (r, bar)
