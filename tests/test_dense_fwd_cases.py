"""Proof, on the CPU alone, that the cases of tests/dense_fwd_cases.py are what they say: the exactness budget holds on every
reference, the statistics cases keep their panel sums exact about any pivot, the split forms add up to the integer reference
(and every product of pieces carries the result somewhere), the poison is where it should be -- and every case reaches the
planned instance it claims: rgnn_linear_fwd_plan is asked on made-up 16-byte-aligned addresses (it reads nothing behind a
pointer) under the switches the GPU test will set, and the claimed rows cover the instance list."""
import ctypes as C
import functools

import numpy as np
import pytest

import dense_fwd_cases as fc
from dense_bwd_cases import BF16X3_OMITTED, BF16X3_PRODUCTS, EXACT_LIMIT, F16X2_OMITTED, F16X2_PRODUCTS

IDS = lambda c: c.name
GROUPS = {"tiny": fc.TINY_CASES, "fp32": fc.FP32_CASES, "x3": fc.X3_CASES, "dma": fc.DMA_CASES, "schedule": fc.SCHEDULE_CASES}


@functools.lru_cache(maxsize=None)
def operands(name):
    return fc.Operands(fc.by_name(name))


def reference(c):
    op = operands(c.name)
    if c.affine == "segments":
        lst, _ = fc.pad_list_emulated(c)
        return op, op.reference(lst, len(lst)), lst
    return op, op.reference(), op.list


def test_the_case_lists_have_the_expected_size_and_unique_names():
    names = [c.name for c in fc.ALL_CASES]
    assert len(set(names)) == len(names)
    assert 150 <= len(names) <= 300
    for c in fc.ALL_CASES:
        assert set(c.env) <= set(fc.SWITCHES), c.name               # only the switches the suite may set
        assert c.expect and len(c.expect) == 8, c.name


# ------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("group", list(GROUPS))
def test_every_reference_keeps_the_exactness_budget(group):
    """sum |terms| + |bias| + |residual| (+ |previous out|) < 2^24 on every output, the reference itself is a float32 integer,
    and only the result's rows and columns differ from the sentinel."""
    for c in GROUPS[group]:
        op, ref, _ = reference(c)
        assert ref["budget"] < EXACT_LIMIT, (c.name, ref["budget"])
        out = ref["out"]
        assert np.array_equal(out, np.rint(out)) and np.array_equal(out.astype(np.float32).astype(np.float64), out), c.name
        before = op.out_alloc().astype(np.float64)
        assert np.array_equal(out[~ref["touched"]], before[~ref["touched"]]), c.name
        off = c.view("out")[0]
        assert not ref["touched"][:, :off].any() and not ref["touched"][:, off + c.n:].any() and not ref["touched"][c.m:].any(), c.name
        if c.rc == 0 and ref["M"] > 0 and c.rows is None:
            assert ref["touched"][:c.m, off:off + c.n].all(), c.name


def test_statistics_cases_are_exact_about_any_pivot():
    """128 (2 max |v|)^2 < 2^24 with max |v| over the stored values AND what an absent row's lanes compute (the epilogue takes
    a lane's first value as its pivot, stored or not): s1, s2 and every merge of two partial results are exact."""
    seen = 0
    for c in fc.ALL_CASES:
        if not c.stats:
            continue
        _, ref, _ = reference(c)
        v = max(ref["absmax"], ref["phantom"])
        assert fc.BM * (2 * v) ** 2 < EXACT_LIMIT, (c.name, v)
        assert ref["stats"].shape[0] == fc.ceil_div(ref["M"], fc.BM)
        seen += 1
    assert seen >= 40


LAYOUT_CASES = [c for c in fc.ALL_CASES if c.layout != "small"]


@pytest.mark.parametrize("c", LAYOUT_CASES, ids=IDS)
def test_split_forms_add_up_to_the_integer_reference(c):
    """The products the kernel keeps sum to the reference exactly, their |terms| stay below 2^24 (in units of the pre-scale),
    and the products it omits are all zero."""
    op = operands(c.name)
    rows = op.named_rows()
    want, _ = op.product(rows)
    got, abs_terms = op.emulate(rows=rows)
    assert np.array_equal(got, want)
    assert abs_terms.max() + 14 < EXACT_LIMIT
    omitted, _ = op.emulate(BF16X3_OMITTED if c.form == "bf16x3" else F16X2_OMITTED, rows=rows)
    assert not omitted.any()


def test_every_split_product_carries_the_result_in_some_case():
    """Dropping any ONE product of pieces changes the result of some layout, in the register-staged kernel's cases, in the
    LDS-DMA kernel's direct cases and in its subset cases alike."""
    pools = {"x3": [c for c in fc.X3_CASES if c.layout != "small"],
             "dma direct": [c for c in fc.DMA_CASES if c.layout != "small" and c.form == "bf16x3" and c.rows is None],
             "dma subset": [c for c in fc.DMA_CASES if c.layout != "small" and c.form == "bf16x3" and c.rows is not None],
             "f16 direct": [c for c in fc.DMA_CASES if c.layout != "small" and c.form == "f16x2" and c.rows is None],
             "f16 subset": [c for c in fc.DMA_CASES if c.layout != "small" and c.form == "f16x2" and c.rows is not None]}
    for pool, cases in pools.items():
        products = F16X2_PRODUCTS if pool.startswith("f16") else BF16X3_PRODUCTS
        for drop in products:
            if drop == ("h", "h"):
                continue                                                  # (every case)
            kept = tuple(p for p in products if p != drop)
            hit = [c.name for c in cases
                   if not np.array_equal(operands(c.name).emulate(kept, operands(c.name).named_rows())[0],
                                         operands(c.name).product(operands(c.name).named_rows())[0])]
            assert hit, (pool, drop)


def test_values_depend_on_row_column_and_k_without_a_power_of_two_period():
    op = operands("sched_psk8_bf16")                                       # 257 rows, 72 columns, K = 512
    A = np.concatenate([op.A1, op.A2], axis=1)
    for x in (A, op.W):
        for period in (16, 32, 64, 128, 256):
            assert not np.array_equal(x[:, period:], x[:, :-period])
            if x.shape[0] > period:
                assert not np.array_equal(x[period:], x[:-period])
    b = operands("dma_f16x2_tn8_n256").bias1
    assert (b[1:] != b[:-1]).all()
    for period in (16, 32, 64, 128):
        assert not np.array_equal(b[period:], b[:-period])


def test_poison_sits_around_every_operand():
    op = operands("dma_bf16x3_rows_holes513")
    c = op.c
    for which, width in (("a1", c.k1), ("a2", c.k2), ("w", c.k)):
        w = op.wide(which)
        off = c.view(which)[0]
        assert off > 0 and np.isnan(w[:, :off]).all() and np.isnan(w[:, off + width:]).all() and w.shape[1] > off + width
    named = op.named_rows()
    unnamed = np.setdiff1d(np.arange(c.m), named)
    assert unnamed.size and np.isnan(op.wide("a1")[unnamed]).all() and not np.isnan(op.wide("a1")[named, c.view("a1")[0]]).any()
    assert (op.list[c.subset_count:] == fc.LIST_TAIL).all() and len(op.list) > c.subset_count
    assert (op.list[[0, 1, 2, 127, 128, 129, 253, 254, 255]] == -1).all() and (op.list[[3, 126, 130, 252, 256]] >= 0).all()
    tile = operands("dma_bf16x3_rows_tile-1700").list
    assert (tile[256:512] == -1).all() and (tile[:256] >= 0).all() and (tile[512:700] >= 0).all()
    long_ = operands("dma_bf16x3_rows_long600")
    assert long_.c.subset_count > long_.c.m and len(long_.named_rows()) == long_.c.m
    assert np.isnan(operands("fp32_fast_on").bias_alloc("b1")[-4:]).all()
    assert (op.out_alloc() == fc.SENTINEL).all() and op.out_alloc().shape[0] > c.m and c.ld("out") > c.n


def test_tables_keep_the_operand_integer():
    for name in ("dma_bf16x3_affine_relu0", "dma_f16x2_segments_k512", "fp32_affine_relu1"):
        op = operands(name)
        t = op.table
        assert set(np.unique(t[:, 1])) <= {0.5, 1.0, 2.0} and np.array_equal(t[:, 0], np.rint(t[:, 0])) and np.array_equal(t[:, 2], np.rint(t[:, 2]))
        a = op.a1_eff(np.arange(op.c.m))
        assert np.array_equal(a, np.rint(a)) and (a != op.A1).any()
    assert set(np.unique(operands("dma_f16x2_segments_k512").table[:, 1])) == {0.5, 1.0, 2.0}


# ------------------------------------------------------------------------------------------------ the plan
def plan_of(c, monkeypatch):
    from radargnn_amd import _lib, ops
    for name in fc.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name in c.env:
        monkeypatch.setenv(name, "1")
    ops.reload_env()                                                      # (undone after the test: monkeypatch, then conftest's reload)
    f = fc.fields(c, fc.MADE_UP, int(_lib.lib.rgnn_linear_planes_kp(c.k)), int(_lib.lib.rgnn_linear_splitk_ws_bytes()))
    args, out = _lib.RgnnLinearArgs(), (C.c_int32 * 8)()
    for k, v in f.items():
        setattr(args, k, v)
    _lib.lib.rgnn_linear_fwd_plan(C.byref(args), C.byref(out))
    return tuple(out), f, args


@pytest.mark.parametrize("group", list(GROUPS))
def test_every_case_reaches_the_plan_row_it_claims(group, monkeypatch):
    from radargnn_amd import _lib
    for c in GROUPS[group]:
        row, f, args = plan_of(c, monkeypatch)
        assert row == c.expect, (c.name, row, c.expect)
        rules = fc.restated(c, f)
        assert bool(row[5]) == rules["bufl"], (c.name, "bufl")
        for claim in ("vec", "fast", "direct"):
            if getattr(c, claim) is not None:
                assert rules[claim] == getattr(c, claim), (c.name, claim)
        fuses = _lib.lib.rgnn_linear_fwd_fuses_a1_affine(C.byref(args))
        if c.affine:
            assert bool(fuses) == (c.rc == 0), c.name
        if c.rc != 0:                                                     # refused before any launch: no GPU needed to see it
            assert _lib.lib.rgnn_linear_fwd(C.byref(args), None) == c.rc == fc.ERR_UNSUPPORTED, c.name
        # the tile the restated ladders give
        fam, _, tile, nt = row[:4]
        if fam == fc.FP32:
            assert tile == fc.fp32_tile(c.n, c.k, rules["bufl"], c.rows is not None), c.name
        elif fam == fc.X3:
            assert tile == fc.x3_tile(c.n) and (c.n <= 32 or c.k % 16 or c.k1 % 16 or "RGNN_X3_NODMA" in c.env), c.name
        elif fam == fc.DMA:
            form = "f16x2" if row[1] == 2 else "bf16x3"
            assert tile == 32 * fc.dma_pick_tn(c.n, c.m, form, c.no_small_m()) and c.n > 32 and c.k % 16 == 0 and c.k1 % 16 == 0, c.name
        if fam != fc.TINY:
            assert nt == fc.ceil_div(c.n, tile), c.name
        else:
            assert c.m >= 4096 and c.k1 <= 8 and c.k2 == 0 and c.n <= 64, c.name


def test_the_claimed_rows_cover_the_instance_list():
    got = {(c.expect[0], c.expect[1], c.expect[2], c.expect[4]) for c in fc.ALL_CASES if c.rc == 0}
    missing = [r for r in fc.REQUIRED_INSTANCES if r not in got]
    assert not missing, missing
    assert {c.expect[5] for c in fc.FP32_CASES} == {0, 1}                                       # with and without buffer descriptors
    for fam, tiles in ((fc.FP32, (32, 64, 128)),):                                            # the ladder tiles on every loader
        for t in tiles:
            assert {c.expect[5] for c in fc.FP32_CASES if c.expect[2] == t} == {0, 1}, t
    assert any(c.vec is False for c in fc.FP32_CASES) and any(c.vec and not c.expect[5] for c in fc.FP32_CASES)
    assert {c.fast for c in fc.FP32_CASES if c.direct is False} >= {True, False}
    for form in (1, 2):                                                                       # fused tables, both kinds, both forms
        assert any(c.affine == "batch" and c.expect[1] == form and c.rc == 0 for c in fc.DMA_CASES)
        assert any(c.affine == "segments" and c.expect[1] == form and c.rc == 0 for c in fc.DMA_CASES)
    assert any(c.expect[7] for c in fc.SCHEDULE_CASES)
    # no forbidden switch, no instance forced
    assert not any(e in ("RGNN_DMA_WAVES", "RGNN_DMA_TN") for c in fc.ALL_CASES for e in c.env)
    assert len(fc.UNREACHABLE) == 2


def test_claimed_schedules_agree_with_the_restated_conditions(monkeypatch):
    seen = set()
    for c in fc.DMA_CASES + fc.SCHEDULE_CASES:
        if c.rc != 0:
            continue
        row, _, _ = plan_of(c, monkeypatch)
        form = "f16x2" if row[1] == 2 else "bf16x3"
        count = len(fc.pad_list_emulated(c)[0]) if c.affine == "segments" else c.subset_count
        got = fc.dma_schedule(count, c.n, c.k, row[2] // 32, form, c.m, bool(row[7]), "RGNN_DMA_NOPSK" in c.env)
        assert got == set(c.schedule) or (count == 0 and not got), (c.name, got, c.schedule)
        seen |= got
    assert {("static", 1), ("streamk", 1), ("psk", 2), ("psk", 8)} <= seen
    # the one large case is as small as the kernel's own condition allows: one row less and no XCD hands a tile over
    big = fc.by_name("sched_streamk_f16x2")
    assert 30000 < big.m < 100000
    assert ("streamk", 1) not in fc.dma_schedule(big.m - 1, big.n, big.k, 2, "f16x2", big.m - 1, True, False)


def test_the_largest_fused_table_sits_on_the_lds_limit():
    for form, tn in (("bf16x3", 7), ("f16x2", 8)):
        fits = next(c for c in fc.DMA_CASES if c.name.startswith(f"dma_{form}_affine_fits"))
        past = next(c for c in fc.DMA_CASES if c.name.startswith(f"dma_{form}_affine_too_wide"))
        lds = fc.dma_lds_bytes(tn, form)
        assert lds + fc.AFFINE_ROWS * 4 * fits.k1 <= fc.LDS_BYTES < lds + fc.AFFINE_ROWS * 4 * past.k1 and past.k1 == fits.k1 + 16
        assert past.rc == fc.ERR_UNSUPPORTED and past.expect[6] == 0 and fits.expect[6] == 1
