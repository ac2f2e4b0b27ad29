"""Proof, on the CPU alone, that the cases of tests/dense_bwd_cases.py are what they say: every exact output stays below 2^24 in its
sum of |terms|, the int64 references agree with float64 (and a per-row loop), every split product a layout claims to pin is load
bearing on that layout's data, and every geometry situation the GPU tests rely on -- steps per slab, empty slabs, narrow class,
16-byte or scalar path, blocks of the narrow launch, tails of the reduce, the live column groups, k tiles -- follows from the
kernel constants restated there and does occur."""
import numpy as np
import pytest

import dense_bwd_cases as dc

ALL_WGRAD = dc.GEOMETRY_CASES + dc.NARROW_CASES + dc.K2_ONLY_CASES
BIG = 20000                                   # rows above which a case is only checked in its first layout here (seconds, not minutes)


def _ops(case, layouts=None):
    for lay in (layouts or case.layouts):
        yield lay, dc.Operands(case, lay)


def test_case_names_are_unique_and_every_sweep_value_is_a_case():
    names = [c.name for c in ALL_WGRAD]
    assert len(set(names)) == len(names)
    for n in dc.N_SWEEP:
        assert dc.by_name(f"n{n}").n == n
    for k1 in dc.K1_SWEEP:
        assert dc.by_name(f"k{k1}").k1 == k1 and dc.by_name(f"k{k1}").k2 == 0
    for k1, k2 in dc.K12_SWEEP:
        c = dc.by_name(f"k{k1}+{k2}")
        assert (c.k1, c.k2) == (k1, k2)
    for m in dc.M_SWEEP:
        assert dc.by_name(f"m{m}").m == m
    assert [(c.k1, c.k2) for c in dc.K2_ONLY_CASES] == [(0, 5), (0, 64)]


@pytest.mark.parametrize("case", ALL_WGRAD, ids=lambda c: c.name)
def test_wgrad_outputs_are_exact_sums(case):
    """Sum of |terms| below 2^24 -- of the plain products and of the products of the bf16 pieces the kernel really sums -- and the
    emulated six-product sum IS the reference; int64 equals float64."""
    for lay, op in _ops(case, case.layouts[:1] if case.m > BIG else None):
        for ones in (False, True):
            ref, mass = op.reference(ones)
            assert mass.max(initial=0) < dc.EXACT_LIMIT, (lay, ones, mass.max())
            G, A = op.operand(ones)
            assert np.array_equal(G.astype(np.float64).T @ A.astype(np.float64), ref.astype(np.float64))
            if case.m <= BIG:
                emu, emass = dc.emulate_bf16x3(G.astype(np.float32), A.astype(np.float32))
                assert emass.max(initial=0) < dc.EXACT_LIMIT, (lay, ones, emass.max())
                assert np.array_equal(emu, ref.astype(np.float64)), (lay, ones)
        if lay == "small":
            G, A = op.operand(True)
            assert (G != 0).all() and np.abs(G).max(initial=0) <= 7 and np.abs(A).max(initial=0) <= 7
        else:
            capped = op.G if lay in ("mid", "low_g") else np.concatenate([op.A1, op.A2], axis=1)
            assert (np.abs(capped).sum(1) > 0).sum() <= (dc.MID_ROWS if lay == "mid" else dc.LOW_ROWS)
            assert (capped[capped != 0] % 2 == 1).all()


def test_reference_equals_a_per_row_loop_on_the_smallest_cases():
    for name in ("m1", "m17", "k1+1", "rows_count17", "rows_repeat", "class_n1_kt1", "view_a1"):
        case = dc.by_name(name)
        for lay, op in _ops(case):
            G, A = op.operand(True)
            want = np.zeros((case.n, A.shape[1]), dtype=np.int64)
            for r in range(G.shape[0]):
                want += np.outer(G[r], A[r])
            assert np.array_equal(op.reference(True)[0], want)
            assert np.array_equal(op.reference(False)[0], want[:, :-1])


def test_active_rows_sit_on_the_edges():
    for case in dc.GEOMETRY_CASES:
        op = dc.Operands(case, "low_g")
        m = len(op.eff)
        pos = set(op.active_pos.tolist())
        per = dc.slab_steps(m, case.slabs(True))[2] * dc.STEP
        last0 = (dc.ceil_div(m, dc.STEP) - 1) * dc.STEP if m else 0
        want = [p for p in (0, m - 1, dc.STEP - 1, dc.STEP, last0 - 1, last0, per - 1, per) if 0 <= p < m]
        want = list(dict.fromkeys(want))[:dc.LOW_ROWS]
        assert set(want) <= pos, (case.name, want, pos)
        assert (np.abs(op.G[op.eff[op.active_pos]]).sum(1) > 0).all()


# ------------------------------------------------------------------------------------------------ load-bearing products
def _drop(products, one):
    return tuple(p for p in products if p != one)


@pytest.mark.parametrize("layout,claims", [("small", [("h", "h")]),
                                           ("mid", [("h", "h"), ("h", "m"), ("m", "h"), ("m", "m")]),
                                           ("low_g", [("l", "h"), ("m", "h"), ("h", "h")]),
                                           ("low_a", [("h", "l"), ("h", "m"), ("h", "h")])])
def test_bf16x3_products_are_load_bearing(layout, claims):
    for name in ("k64+63", "m129", "n65"):
        op = dc.Operands(dc.by_name(name), layout)
        G, A = (x.astype(np.float32) for x in op.operand(True))
        ref = op.reference(True)[0].astype(np.float64)
        assert np.array_equal(dc.emulate_bf16x3(G, A)[0], ref)
        for prod in claims:
            assert not np.array_equal(dc.emulate_bf16x3(G, A, _drop(dc.BF16X3_PRODUCTS, prod))[0], ref), (name, prod)
        for prod in dc.BF16X3_OMITTED:                    # what the kernel leaves out is identically zero on the data
            assert not dc.emulate_bf16x3(G, A, (prod,))[1].any(), (name, prod)


@pytest.mark.parametrize("layout,claims", [("small", [("h", "h")]), ("low_g16", [("l", "h"), ("h", "h")]),
                                           ("low_a16", [("h", "l"), ("h", "h")])])
@pytest.mark.parametrize("loose", [1.0, 2.0, 256.0])
def test_f16x2_products_are_load_bearing(layout, claims, loose):
    for name in ("k64+63", "m129", "n65"):
        op = dc.Operands(dc.by_name(name), layout)
        G, A = op.operand(False)
        bg, b1, b2 = op.bounds()
        ref = op.reference(True)[0].astype(np.float64)
        emu, mass = dc.emulate_f16x2(G, A, bg * loose, max(b1, b2) * loose, True)
        assert np.array_equal(emu, ref), (name, loose)
        assert mass.max() < dc.EXACT_LIMIT, (name, mass.max())        # in units of the smallest product of split pieces
        for prod in claims:
            assert not np.array_equal(dc.emulate_f16x2(G, A, bg * loose, max(b1, b2) * loose, True, _drop(dc.F16X2_PRODUCTS, prod))[0],
                                      ref), (name, prod)
        assert not dc.emulate_f16x2(G, A, bg * loose, max(b1, b2) * loose, True, dc.F16X2_OMITTED)[0].any()


def test_f16x2_geometry_cases_are_exact_at_the_exact_bound():
    for case in dc.GEOMETRY_CASES:
        if case.m > 500 or "small" not in case.layouts or len(case.layouts) == 1:
            continue
        for lay in dc.LAYOUTS_F16:
            op = dc.Operands(case, lay)
            if not len(op.eff):
                continue
            G, A = op.operand(False)
            bg, b1, b2 = op.bounds()
            emu, mass = dc.emulate_f16x2(G, A, bg, max(b1, b2), True)
            assert np.array_equal(emu, op.reference(True)[0].astype(np.float64)), (case.name, lay)
            assert mass.max() < dc.EXACT_LIMIT


def test_f16x2_blocks_with_bounds_2_10_apart_stay_exact():
    for lay in ("small", "low_g16"):
        op = dc.Operands(dc.by_name("k64+63"), lay, a1_scale=1024)
        G, A = op.operand(False)
        bg, b1, b2 = op.bounds()
        assert b1 == 1024 * b2 or lay == "small" and b1 >= 512 * b2
        emu, mass = dc.emulate_f16x2(G, A, bg, max(b1, b2), True)
        assert np.array_equal(emu, op.reference(True)[0].astype(np.float64)) and mass.max() < dc.EXACT_LIMIT
        if lay == "small":                                # (low_g16: below 2^24 in units of 2^10 only, which is what `mass` counts)
            assert op.reference(True)[1].max() < dc.EXACT_LIMIT


# ------------------------------------------------------------------------------------------------ geometry situations
def test_geometry_cases_take_the_mfma_kernel_and_narrow_cases_what_they_state():
    for c in dc.GEOMETRY_CASES + dc.K2_ONLY_CASES:
        assert c.kernel(False) == "x3" and c.kernel(True) == "x3", c.name
    for c in dc.NARROW_CASES:
        assert c.kernel(c.ones) == c.expect, c.name
    seen = {c.expect for c in dc.NARROW_CASES}
    assert seen == {"x3", "narrow1", "narrow2", "narrow3"}
    # both sides of every class boundary
    cls = lambda n, kt: dc.narrow_class(n, kt, 0, 0)
    assert (cls(16, 9), cls(16, 10), cls(17, 9)) == (1, 0, 0)
    assert (cls(8, 17), cls(8, 18), cls(9, 17)) == (2, 0, 0)
    assert (cls(32, 6), cls(32, 7), cls(33, 6), cls(17, 6), cls(1, 1)) == (3, 0, 0, 3, 1)


def test_slab_situations_occur():
    counts, past_seen, short_last = set(), False, False
    for m in dc.M_SWEEP:
        c = dc.by_name(f"m{m}")
        assert c.slabs(True) == 8 and c.slabs(False) == 8
        steps, past, per = dc.slab_steps(m, 8)
        assert sum(steps) == dc.ceil_div(m, dc.STEP)
        counts |= set(steps)
        past_seen |= any(past)
        live = [s for s in steps if s]
        short_last |= len(live) > 1 and live[-1] < per
    assert {0, 1, 2, 3} <= counts and past_seen and short_last
    c = dc.by_name("m2049_n129")
    assert c.slabs(True) == 16 and dc.tiles(c.n, c.k1, c.k2, True) == (2, 1)
    c = dc.by_name("rows_sparse")
    steps, past, _ = dc.slab_steps(c.m_eff, c.slabs(True))
    assert sum(1 for s in steps if s == 0) > len(steps) // 2                 # most slabs are empty
    assert dc.by_name("rows_count0").m_eff == 0 and dc.by_name("rows_short").m_eff < dc.by_name("rows_short").m
    op = dc.Operands(dc.by_name("rows_short"), "small")
    assert (op.row_index[op.case.m_eff:] == -7).all() and (op.row_index[:op.case.m_eff] >= 0).all()
    op = dc.Operands(dc.by_name("rows_repeat"), "small")
    assert len(np.unique(op.eff)) < len(op.eff)
    op = dc.Operands(dc.by_name("rows_reversed"), "small")
    assert (np.diff(op.eff) < 0).all()


def test_k_axis_situations_occur():
    # the bias column fits the padding at k1 = 63, opens a new 64-column group at k1 = 64; with k1 = 32 group 1 is live for it alone
    assert dc.virtual_k(63, 0, True) == (64, 64) and dc.virtual_columns(63, 0, True)[-1] == 63
    assert dc.virtual_k(64, 0, True) == (128, 128) and dc.virtual_k(64, 0, False) == (64, 64)
    assert dc.a_live(32, 0, True)[:3] == [True, True, False] and dc.a_live(32, 0, False)[:2] == [True, False]
    assert dc.tiles(40, 192, 64, True)[1] == 2 and dc.tiles(40, 192, 64, False)[1] == 1
    assert dc.tiles(40, 257, 0, False)[1] == 2 and dc.tiles(40, 256, 0, True)[1] == 2 and dc.tiles(40, 255, 0, True)[1] == 1
    assert dc.tiles(160, 40, 0, True)[0] == 2
    patterns = set()
    for c in dc.GEOMETRY_CASES + dc.K2_ONLY_CASES:
        for ones in (False, True):
            live = dc.a_live(c.k1, c.k2, ones)
            cols = dc.virtual_columns(c.k1, c.k2, ones)
            assert len(cols) == c.k1 + c.k2 + ones and len(set(cols)) == len(cols)
            assert {v // dc.LIVE for v in cols} == {i for i, l in enumerate(live) if l}, (c.name, ones)   # live <=> holds a column
            k1p, kv = dc.virtual_k(c.k1, c.k2, ones)
            assert all(v < kv for v in cols) and k1p % dc.WAVE_COLS == 0 and kv % dc.WAVE_COLS == 0
            patterns.add(tuple(live))
    assert len(patterns) >= 10
    assert any(list(p).index(False) < max(i for i, l in enumerate(p) if l) for p in patterns)     # a dead group in FRONT of a live one
    assert dc.a_live(0, 5, True)[0] and dc.virtual_k(0, 5, True) == (0, 64)                       # (k1 = 0: A2 starts at virtual column 0)


def test_narrow_and_reduce_situations_occur():
    blocks = {m: dc.narrow_blocks(m) for m in (1, 255, 256, 257, 1024, 1025, 16385, 32769, 262145)}
    assert blocks == {1: 1, 255: 1, 256: 1, 257: 1, 1024: 1, 1025: 2, 16385: 17, 32769: 33, 262145: 256}
    assert dc.narrow_trips(262144) == 4 and dc.narrow_trips(262145) == 5 and dc.narrow_trips(1025) == 3
    assert dc.by_name("narrow_m262145").m * 49 < dc.EXACT_LIMIT
    assert dc.reduce_paths(1) == (False, False, True)
    assert dc.reduce_paths(17) == (True, False, True)          # group 0 pairs slabs 0 and 16, the other groups take the tail alone
    assert dc.reduce_paths(33) == (True, True, False)          # group 0 takes the tail (slab 32) behind the loop
    assert dc.reduce_paths(8)[2] and dc.reduce_paths(512)[0] and dc.reduce_paths(256) == (True, False, False)
    widths = {c.n * c.k1 for c in dc.NARROW_CASES if c.name.startswith("width")}
    assert widths == {1, dc.RED_COLS - 1, dc.RED_COLS, dc.RED_COLS + 1}
    paths = set()
    for c in dc.NARROW_CASES:
        if not c.name.startswith("vec_"):
            continue
        go, ge = c.views.get("g", (0, 0))
        ao, ae = c.views.get("a1", (0, 0))
        gv, av = dc.vec_path(c.n, go + c.n + ge, go), dc.vec_path(c.k1, ao + c.k1 + ae, ao)
        assert gv == av == c.name.endswith("aligned"), c.name
        paths.add((c.name.rsplit("_", 1)[1], gv))
    assert paths == {("aligned", True), ("offgrid", False), ("oddstride", False)}
    for nm in ("view_a1", "view_g", "view_a2"):
        c = dc.by_name(nm)
        (key, (off, extra)), = c.views.items()
        width = {"g": c.n, "a1": c.k1, "a2": c.k2}[key]
        assert off % 4 != 0 or (off + width + extra) % 4 != 0


def test_library_host_functions_agree_with_the_restated_rules():
    """rgnn_wgrad_slabs and rgnn_linear_stat_panels are host-only: callable here."""
    from radargnn_amd import ops
    from radargnn_amd._lib import lib
    for c in ALL_WGRAD:
        for ones in (0, 1):
            assert int(lib.rgnn_wgrad_slabs(c.m, c.n, c.k1, c.k2, ones)) == dc.slabs(c.m, c.n, c.k1, c.k2, ones), (c.name, ones)
    for m in list(dc.BN_M) + [0, 255, 256, 4100]:
        assert ops.stat_panels(m) == dc.ceil_div(m, dc.PANEL) == dc.stat_panels(m)
    assert ops.BOUND_SLOTS == dc.BOUND_SLOTS


# ------------------------------------------------------------------------------------------------ BatchNorm / ReLU
def test_bn_cases():
    kinds = set()
    for m in dc.BN_M:
        for n in dc.BN_N:
            for mask in dc.BN_MASKS:
                c = dc.BnCase(m, n, mask)
                assert np.abs(c.dy).max() <= 4 and np.abs(c.h).max() <= 8
                ref = c.stats_reference()
                assert ref.shape == (dc.stat_panels(m), 2, n)
                assert np.array_equal(ref.sum(0)[0], c.g.sum(0)) and np.array_equal(ref.sum(0)[1], (c.g * c.h).sum(0))
                assert np.abs(c.g * c.h).sum(0).max() < dc.EXACT_LIMIT
                dx = c.dx_reference()
                assert np.array_equal(dx.astype(np.float32).astype(np.float64), dx)
                want = c.coef[0].astype(np.float64) * c.g + c.coef[1].astype(np.float64) * c.h + c.coef[2].astype(np.float64)
                assert np.array_equal(dx, want)
                if mask == "table":
                    assert (c.y_table == 0).any(axis=0).all()                     # an exact zero in every column
                    assert np.array_equal(c.table.astype(np.int64).astype(np.float32), c.table)
                    if m >= 32 and n >= 3:
                        assert (c.y_table > 0).any() and (c.y_table < 0).any()
                    assert not c.keep[c.y_table == 0].any()
                if mask == "y":
                    y = c.y.reshape(-1)
                    kinds |= {("nan" if np.isnan(v) else "-0" if (v == 0 and np.signbit(v)) else "+0" if v == 0 else
                               "den" if 0 < v < 1e-40 else "pos" if v > 0 else "neg") for v in y[:6]}
                    assert np.array_equal(c.keep, np.nan_to_num(c.y, nan=-1.0) > 0)
    assert kinds == {"nan", "-0", "+0", "den", "pos", "neg"}
    # the seams: 32-row groups and 128-row panels of the stats kernel, its 64 columns, the VEC switch of the apply
    assert {31, 32, 33} <= set(dc.BN_M) and {127, 128, 129} <= set(dc.BN_M) and dc.PANEL_GROUP == 32 and dc.PANEL == 128
    assert {dc.STATS_COLS - 1, dc.STATS_COLS, dc.STATS_COLS + 1} <= set(dc.BN_N)
    assert {n % 4 == 0 for n in dc.BN_N} == {True, False}


def test_coef_cases():
    assert {n % 4 == 0 for n in dc.COEF_N} == {True, False}
    scalar = [n for n in dc.COEF_N if n % 4]
    assert min(scalar) < dc.COEF_CH < max(scalar)
    for g in dc.COEF_GROUPS:
        assert {g - 1, g, g + 1} <= set(dc.COEF_PANELS)
    for n in (1, 4, 17):
        for panels in (1, 3, 65):
            c = dc.CoefCase(n, panels, True, True)
            cnt, piv, s1, s2 = (c.fwd_stats[:, i].astype(np.float64) for i in range(4))
            live = cnt > 0
            assert np.allclose(np.where(live, s1 + cnt * piv, 0).sum(0), c.v.sum(0), rtol=0, atol=0)
            assert np.array_equal(np.where(live, s2 + 2 * piv * s1 + cnt * piv * piv, 0).sum(0), (c.v ** 2).sum(0))
            assert int(cnt[:, 0].sum()) == c.m
            if panels >= 3:
                assert not live[1].any()
            ref = c.reference()
            assert set(ref) == {"A", "B", "C", "dgamma", "dbeta"}
            ec = dc.CoefCase(n, panels, False, False)
            e = ec.reference()
            assert not e["B"][0].any() and not e["C"][0].any()
            assert np.array_equal(e["A"][0], 1.0 / np.sqrt(ec.running_var.astype(np.float64) + np.float64(np.float32(dc.COEF_EPS))))
