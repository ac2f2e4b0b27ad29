"""Every input of tests/feature_edge_cases.py stands on the edge it is named for -- shown on the CPU, from numpy and the oracle
alone, so that a later simplification of a builder fails here and not silently on the device.  No GPU, no torch."""
from fractions import Fraction

import numpy as np

import feature_edge_cases as fc
from oracle import graph_oracle as go


def frames_of(ts, ptr):
    return [ts[int(ptr[f]):int(ptr[f + 1])] for f in range(len(ptr) - 1)]


# ================================================================================================ time index
def test_time_index_frame_sizes_stand_on_the_round_edges():
    sizes = list(fc.TI_FRAME_SIZES)
    T, R = fc.TI_THREADS, fc.TI_ROUND
    assert (T, R, fc.TI_CAP) == (1024, 4096, 4096)
    assert {1, T - 1, T, T + 1, R - 1, R, R + 1, 2 * R + 1} <= set(sizes)
    assert sizes[:2] == [0, 0] and sizes[-1] == 0 and 0 in sizes[2:-1]           # empties: doubled in front, inside, at the back
    ts, ptr = fc.ti_size_batch()
    assert np.array_equal(np.diff(ptr), sizes) and len(ts) == sum(sizes) and np.isfinite(ts).all()
    exp = fc.ti_expected(ts, ptr)
    for f, v in enumerate(frames_of(ts, ptr)):
        if len(v) == 0:
            continue
        d = len(np.unique(v))
        assert d <= 2049 < fc.TI_MAX_UNIQUE
        assert (v[:-1] < v[-1]).all()                                            # the last point's value is its own and the largest
        assert exp[int(ptr[f + 1]) - 1] == d - 1 and (d == 1) == (len(v) == 1)
        if len(v) > 1:
            assert d >= min(len(v), 2048) - 1


def test_time_index_value_kinds_are_what_they_are_named():
    ts, ptr = fc.ti_value_batch()
    fr = frames_of(ts, ptr)
    assert [len(v) for v in fr] == [301, 0] * len(fc.TI_VALUE_KINDS)
    v = dict(zip(fc.TI_VALUE_KINDS, fr[::2]))
    assert not np.isnan(ts).any()
    assert len(np.unique(v["equal"])) == 1
    assert (np.diff(v["descending"]) < 0).all()
    z = v["zeros"]
    assert ((z == 0) & np.signbit(z)).any() and ((z == 0) & ~np.signbit(z)).any() and len(np.unique(z)) == 3
    inf = v["infinities"]
    assert (inf == np.inf).any() and (inf == -np.inf).any() and len(np.unique(inf)) == 5
    t = v["tiniest"]
    assert (t == 5e-324).any() and (t == -5e-324).any() and ((t == 0) & np.signbit(t)).any() and len(np.unique(t)) == 5
    nb = v["neighbours"]
    assert np.array_equal(nb[1::2], np.nextafter(nb[0:-1:2], np.inf)) and len(np.unique(nb)) == 10
    assert (v["negatives"] < 0).all() and len(np.unique(v["negatives"])) > 100
    us = v["microseconds"]
    assert (us == np.round(us)).all() and (np.abs(us - 1.5e15) < 1e4).all() and len(np.unique(us)) > 10
    # 0.0 and -0.0 get ONE rank, the neighbours one ulp apart get two
    ez = fc.ti_expected(z, fc.ptr_of([len(z)]))
    assert len(set(ez[z == 0].tolist())) == 1
    en = fc.ti_expected(nb, fc.ptr_of([len(nb)]))
    assert (en[1::2] == en[0:-1:2] + 1).all()


def test_time_index_distinct_counts_stand_on_the_limit():
    assert fc.TI_MAX_UNIQUE == 3072
    ts, ptr = fc.ti_distinct_batch()
    per = fc.ti_distinct_per_frame(ts, ptr)
    assert per == [1, 2, 3071, 3072, 3072] and set(fc.TI_DISTINCT_COUNTS) == set(per)
    sizes = np.diff(ptr).tolist()
    assert sizes[3] > 3072 and sizes[4] == 3072                                  # at the limit with repeats, and without
    ts, ptr = fc.ti_overflow_batch()
    assert fc.ti_distinct_per_frame(ts, ptr) == [3, 3073, 2]


def slot_restated(t):
    """(bits * 0x9E3779B97F4A7C15 mod 2^64) >> 52 in Python integers."""
    t = 0.0 if t == 0.0 else float(t)
    key = int(np.array([t], dtype=np.float64).view(np.uint64)[0])
    return ((key * 0x9E3779B97F4A7C15) % (1 << 64)) >> 52


def probe_places(values):
    """Linear probing with wrap-around in a table of 4 096 slots, keys entered in order -> {value: (home, place)}."""
    table, where = {}, {}
    for t in values:
        t = 0.0 if t == 0.0 else float(t)
        if t in where:
            continue
        home = h = slot_restated(t)
        while h in table:
            h = (h + 1) % 4096
        table[h] = t
        where[t] = (home, h)
    return where


def test_time_index_probe_chain_crosses_the_table_end():
    hot = fc.ti_last_slot_values()
    assert len(hot) == 62 and len(np.unique(hot)) == 62
    assert all(slot_restated(t) == 4095 for t in hot)
    assert np.array_equal(fc.ti_slot(hot), np.full(62, 4095))
    ts, ptr = fc.ti_wrap_batch()
    fr = frames_of(ts, ptr)
    for v in fr[1:]:
        mine = np.unique(v[np.isin(v, hot)])
        assert len(mine) == 62 >= 40
        assert len(np.unique(v)) <= fc.TI_MAX_UNIQUE
        where = probe_places(v)                                                   # (any insertion order gives the same set of places)
        wrapped = [t for t, (home, place) in where.items() if place < home]
        assert len(wrapped) >= 40 and all(where[t][0] == 4095 or where[t][1] <= 80 for t in wrapped)
        assert (np.bincount(np.searchsorted(mine, v[np.isin(v, hot)]))[:62] >= 2).all()     # repeats: look-ups walk the chain too
    assert len(np.unique(fr[1])) > 500                                           # ordinary values in the mix


def test_time_index_many_frames_exceed_the_spread_out_limit():
    ts, ptr = fc.ti_many_frames()
    sizes = np.diff(ptr)
    assert len(sizes) == 1025 == fc.TI_SPREAD_MAX_FRAMES + 1 and fc.TI_SPREAD_HINT > 16384
    assert sizes.min() == 0 and sizes.max() == 3 and sizes[0] == 0 and len(ts) == sizes.sum()
    assert ((ts == 0) & np.signbit(ts)).any() and fc.ti_expected(ts, ptr).max() >= 2


# ================================================================================================ edge features
def pair_columns(X, V, E, mode):
    return go.edge_features(X, V, E, ["point_pair_features"], mode)


def test_lattice_rows_are_nan_where_the_self_dot_product_rounds_above_one():
    c = fc.lattice_vectors()
    assert c.shape == (168, 2) and np.abs(c).max() == 6 and (c == np.round(c)).all() and (c != 0).any(axis=1).all()
    uu = fc.unit_self_dots()
    over, one, under = int((uu > 1).sum()), int((uu == 1).sum()), int((uu < 1).sum())
    assert over >= 20 and one >= 60 and under >= 60 and over + one + under == 168          # measured: 24, 80, 64
    nan_rows = {}
    for variant in fc.LATTICE_VARIANTS:
        X, V, E = fc.lattice_case(variant)
        assert E.shape == (336, 2) and np.array_equal(E[:168], E[168:, ::-1])               # both ways
        und, dire = pair_columns(X, V, E, "undirected"), pair_columns(X, V, E, "directed")
        assert not np.isnan(dire).any()
        assert not np.isnan(und[:, :2]).any()                                                # distance and the clamped angle
        assert np.array_equal(np.isnan(und[:, 2]), np.isnan(und[:, 3]))
        nan_rows[variant] = np.isnan(und[:, 2])
        if "_" not in variant:
            assert np.array_equal(nan_rows[variant][:168], nan_rows[variant][168:])
    for variant in ("parallel", "antiparallel"):
        assert int(nan_rows[variant][:168].sum()) >= 20
        assert np.array_equal(nan_rows[variant][:168], uu > 1)                              # exactly the rows with u . u > 1
    assert not nan_rows["perpendicular"].any()
    # one end parallel (NaN where u . u > 1), the other perpendicular (90 degrees): Python's min / max keep or drop the NaN by
    # the ORDER of their arguments, so these rows tell `t2 < t1 ? t2 : t1` from fmin
    X, V, E = fc.lattice_case("parallel_perpendicular")
    und = pair_columns(X, V, E, "undirected")
    assert np.isnan(und[:, 2:]).any() and np.isfinite(und[:, 2:]).any()
    assert not np.array_equal(np.isnan(und[:168, 2]), np.isnan(und[168:, 2]))                # ... and (i, j) differs from (j, i)
    # directed: the clamp turns the same rows into exactly 0 and 180 degrees
    X, V, E = fc.lattice_case("parallel")
    dire = pair_columns(X, V, E, "directed")
    assert (dire[:168][uu > 1][:, 2] == 0.0).all() and (dire[168:][uu > 1][:, 2] == 180.0).all()


def test_degenerate_rows_give_ninety_degrees_where_a_unit_vector_is_zero():
    X, V, E, rows = fc.degenerate_case()
    assert set(rows) == set(fc.DEGENERATE_ROWS) and sorted(sum(rows.values(), [])) == list(range(len(E)))
    for mode in ("directed", "undirected"):
        f = pair_columns(X, V, E, mode)
        assert not np.isnan(f).any()
        for name in ("coincident", "self_loop"):                                  # no connection vector: both of its angles are 90
            assert (f[rows[name], 0] == 0).all() and (f[rows[name], 2:] == 90.0).all()
        assert (f[rows["zero_velocity_both"], 1:] == 90.0).all()
        for name in ("zero_velocity_first", "zero_velocity_second"):
            assert (f[rows[name], 1] == 90.0).all() and (f[rows[name], 2:] == 90.0).any()
    e = E[rows["coincident"][0]]
    assert e[0] != e[1] and np.array_equal(X[e[0]], X[e[1]])
    e = E[rows["self_loop"][0]]
    assert e[0] == e[1]
    assert (V[E[rows["zero_velocity_first"][0]][0]] == 0).all() and (V[E[rows["zero_velocity_first"][0]][1]] != 0).any()
    assert (V[E[rows["zero_velocity_second"][0]][1]] == 0).all() and (V[E[rows["zero_velocity_second"][0]][0]] != 0).any()
    nz = E[rows["negative_zero"]].reshape(-1)
    assert (np.signbit(X[nz]) & (X[nz] == 0)).any() and (np.signbit(V[nz]) & (V[nz] == 0)).any()
    rel = go.edge_features(X, V, E, ["relative_position", "relative_velocity"], "directed")
    assert (np.signbit(rel) & (rel == 0)).any() and (~np.signbit(rel) & (rel == 0)).any()     # both zeros among the differences


def test_float_extremes_overflow_and_underflow_in_float32_only():
    X, V, E = fc.extreme_case()
    for mode in ("directed", "undirected"):
        f = go.edge_features(X, V, E, list(fc.EDGE_NAMES), mode)
        exact, angle = fc.edge_columns(fc.EDGE_NAMES)
        assert np.isfinite(f[:, exact]).all() and (mode == "undirected" or np.isfinite(f).all())
        with np.errstate(over="ignore"):
            f32 = f.astype(np.float32)
        assert np.isinf(f32[:, exact]).any() and ((f32[:, exact] == 0) & (f[:, exact] != 0)).any()
        tiny = np.float32(1.4e-45)
        assert (np.abs(f32[:, exact]) == tiny).any()                                  # and a float32 subnormal
    assert (np.abs(X) == 1e39).any() and (np.abs(V) == 1e39).any()
    d = np.abs(X[E[:, 0]] - X[E[:, 1]])
    assert np.isin(d, [1e-46]).any() and np.isin(d, [1e-45]).any()


def test_edge_feature_lists_and_sizes():
    lists = fc.edge_lists()
    assert [l for l in lists if len(l) == 1] == [[nm] for nm in fc.EDGE_NAMES]
    assert sorted(map(tuple, fc.rotations(fc.EDGE_NAMES))) == sorted({tuple(l) for l in lists if len(l) == 5}) and len(fc.rotations(fc.EDGE_NAMES)) == 5
    assert {l[0] for l in fc.rotations(fc.EDGE_NAMES)} == set(fc.EDGE_NAMES)
    sixteen = [l for l in lists if len(l) == fc.MAX_FEATURE_CODES]
    assert len(sixteen) == 2 and fc.MAX_FEATURE_CODES == 16
    assert sum(go.EDGE_FEATURE_WIDTH[nm] for nm in sixteen[0]) == 64 and set(sixteen[1]) == set(fc.EDGE_NAMES)
    exact, angle = fc.edge_columns(fc.EDGE_NAMES)
    assert angle.tolist() == [1, 2, 3] and exact.tolist() == [0, 4, 5, 6, 7, 8, 9]
    assert {255, 256, 257, 0, 1, 513} == set(fc.EDGE_SIZES)                            # around one and two blocks of 256 threads
    X, V, pool = fc.edge_pool()
    assert len(pool) == 6 * 336 + 9 + 22 + 128 == 2175 and pool.max() == len(X) - 1 == len(V) - 1
    for n in fc.EDGE_SIZES:
        _, _, E = fc.sized_edges(n)
        assert E.shape == (n, 2)
    _, _, E = fc.sized_edges(513)
    und = go.edge_features(X, V, E, ["point_pair_features"], "undirected")
    assert np.isnan(und).any() and (und[:, 2:] == 90.0).any()                         # NaN rows and degenerate rows in the sample
    assert (np.abs(X[E]) == 1e39).any()


def test_reversed_lists():
    n = 513
    lists = fc.reversed_lists(n)
    sub = lists["permuted_subset"]
    assert len(np.unique(sub)) == len(sub) == n // 2 and (np.diff(sub) < 0).any()
    rep = lists["repeats"]
    assert len(np.unique(rep)) < len(rep) and rep.max() < n
    assert [len(lists[k]) for k in ("rows_0", "rows_1", "rows_257")] == [0, 1, 257]
    assert all(len(v) != n and v.dtype == np.int32 and (len(v) == 0 or (0 <= v.min() and v.max() < n)) for v in lists.values())


def fused(a, b, c):
    """fma(a, b, c): a b + c rounded once."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def test_inputs_tell_a_fused_multiply_add_from_a_multiply_and_an_add():
    """What the device would compute if -ffp-contract=off were lost for csrc/features.hip, simulated in exact arithmetic: the NaN
    rows of the lattice move, and distances of the generic ring and velocity lengths of the node case change bits."""
    u = go._unit_or_zero(fc.lattice_vectors())
    plain = go._dot2(u, u)
    for a, b in ((0, 1), (1, 0)):                                                # either product may be the fused one
        contracted = np.array([fused(r[a], r[a], r[b] * r[b]) for r in u])
        assert int(((contracted > 1) != (plain > 1)).sum()) >= 10                # measured: 12
    X, V, E = fc.generic_case()
    d = X[E[:, 0]] - X[E[:, 1]]
    plain = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    assert np.array_equal(plain, go.edge_features(X, V, E, ["spatial_euclidean_distance"], "directed")[:, 0])
    for a, b in ((0, 1), (1, 0)):
        assert int((np.sqrt(np.array([fused(r[a], r[a], r[b] * r[b]) for r in d])) != plain).sum()) >= 6
    V = fc.node_case(257)["V"]
    plain = np.sqrt(V[:, 0] * V[:, 0] + V[:, 1] * V[:, 1])
    for a, b in ((0, 1), (1, 0)):
        assert int((np.sqrt(np.array([fused(r[a], r[a], r[b] * r[b]) for r in V])) != plain).sum()) >= 2


# ================================================================================================ node features
def test_node_cases_hold_their_special_values():
    assert set(fc.NODE_SIZES) == {0, 1, 255, 256, 257}
    assert fc.node_case(0)["X"].shape == (0, 2) and fc.node_case(0)["frame_ptr"].tolist() == [0, 0, 0, 0]
    c = fc.node_case(257)
    deg = c["degree"]
    assert deg.dtype == np.int32 and set(fc.DEGREE_EDGES) <= set(deg.tolist())
    as32 = deg.astype(np.float64).astype(np.float32).astype(np.float64)
    assert (as32[deg == 2 ** 24 + 1] == 2 ** 24).all() and (as32[deg == 2 ** 31 - 1] == 2 ** 31).all()    # the cast rounds
    rcs = c["rcs"]
    assert np.isnan(rcs).any() and (rcs == np.inf).any() and (rcs == -np.inf).any() and ((rcs == 0) & np.signbit(rcs)).any()
    assert (np.abs(c["X"]) == 1e39).any() and (np.abs(c["V"]) == 1e39).any() and (c["V"] == 1e-46).any()
    ptr = c["frame_ptr"]
    assert ptr[1] == ptr[2] and 0 < ptr[1] < ptr[3] == 257
    ti = fc.ti_expected(c["timestamp"], ptr)
    assert ti.max() == 4 and not np.array_equal(ti, c["time_index"])
    one = fc.node_case(1)
    assert one["degree"][0] == 0 and np.signbit(one["rcs"][0])
    lists = fc.node_lists()
    assert [l for l in lists if len(l) == 1] == [[nm] for nm in fc.NODE_NAMES]
    assert len([l for l in lists if len(l) == 6]) == 6 and {l[0] for l in lists if len(l) == 6} == set(fc.NODE_NAMES)
    assert [len(l) for l in lists][-1] == 16 and set(lists[-1]) == set(fc.NODE_NAMES)
    exp = fc.node_expected(c, list(fc.NODE_NAMES), ti)
    assert exp.shape == (257, 8) and np.array_equal(fc.bits(exp[:, 0]), fc.bits(rcs))


# ================================================================================================ frame split
def test_split_frames_stand_on_the_strip_edges():
    S = fc.SPLIT_STRIP
    assert S == 1024 and {0, 1, S - 1, S, S + 1, 2 * S + 1} <= set(fc.SPLIT_FRAME_SIZES)
    sizes = list(fc.SPLIT_FRAME_SIZES)
    assert sizes[0] == 0 and any(a == b == 0 for a, b in zip(sizes, sizes[1:]))
    many = fc.split_many_frame_sizes()
    assert len(many) == 1030 > S and many.min() == 0 and many.max() == 3
    for sz in (sizes, many):
        ptr, n = fc.ptr_of(sz), int(sum(sz))
        for pattern in fc.DEGREE_PATTERNS:
            deg = fc.degree_pattern(pattern, n)
            pos = np.nonzero(deg > 0)[0].tolist()
            want = {"all_zero": [], "all_positive": list(range(n)), "alternating": list(range(1, n, 2)), "last_only": [n - 1],
                    "first_only": [0]}[pattern]
            assert pos == want and deg.dtype == np.int32
            e = fc.split_expected(deg, ptr)
            assert e["frame_nonempty"].sum() == e["count_nonempty"] == len(pos) and e["count_empty"] == n - len(pos)
            assert np.array_equal(np.sort(np.concatenate([e["list_empty"], e["list_nonempty"]])), np.arange(n))
            assert (e["slot"][e["list_nonempty"]] == -1).all()
            assert np.array_equal(e["list_empty"][e["slot"][e["list_empty"]]], e["list_empty"])
            for f in range(len(sz)):
                assert e["frame_nonempty"][f] == (deg[int(ptr[f]):int(ptr[f + 1])] > 0).sum()
    # in the many-frames batch the nodes with edges of frames beyond the 1 024th matter to the frames after them
    e = fc.split_expected(fc.degree_pattern("alternating", int(many.sum())), fc.ptr_of(many))
    assert e["frame_nonempty"][:S].sum() > 0 and e["frame_nonempty"][S:-1].sum() > 0


# ================================================================================================ padded lists
def test_pad_cases_stand_on_the_tile_edges():
    P = fc.PAD_ROWS
    assert (P, fc.PANEL_ROWS) == (256, 128) and set(fc.PAD_ENTRY_COUNTS) == {0, 1, P - 1, P, P + 1, 2 * P}
    cases = fc.pad_cases()
    per_segment = {}
    for name, (buf, count, seg) in cases.items():
        ids = buf[:count]
        assert buf.dtype == np.int32 and seg.dtype == np.int64
        assert len(buf) >= count + 256 and (buf[count:] == fc.PAD_GARBAGE).all()        # longer than the list, garbage behind it
        assert (np.diff(ids) > 0).all() and (count == 0 or (ids[0] >= 0 and ids[-1] < seg[-1] < fc.PAD_GARBAGE))
        per_segment[name] = [int(((ids >= seg[f]) & (ids < seg[f + 1])).sum()) for f in range(len(seg) - 1)]
        out, tiles, start = fc.pad_expected(buf, count, seg)
        assert len(out) % P == 0 and len(tiles) == len(out) // P and start[-1] == len(out) // fc.PANEL_ROWS
        assert np.array_equal(out[out >= 0], ids) and len(start) == len(seg)
    for k in fc.PAD_ENTRY_COUNTS:
        assert per_segment[f"one_segment_{k}"] == [k]
    big = per_segment["257_segments"]
    assert len(big) == 257 == P + 1 and set(big) == set(fc.PAD_ENTRY_COUNTS)
    assert big[P] > 0                                                                  # the segment beyond the prefix loop's stride
    seg = cases["257_segments"][2]
    assert (np.diff(seg) == 0).any() and ((np.diff(seg) > 0) & (np.array(big) == 0)).any()     # no rows; rows but no entries
    short = per_segment["257_segments_short_list"]
    assert short[-1] == 0 and seg[-1] > seg[-2] and short[:-1] == big[:-1]
    assert cases["257_segments_short_list"][2][-1] - cases["257_segments_short_list"][2][-2] == 300
    inside = per_segment["all_in_one_of_eleven"]
    assert sorted(inside)[-1] == 512 == cases["all_in_one_of_eleven"][1] and sorted(inside)[-2] == 0
    assert cases["count_zero"][1] == 0 and len(fc.pad_expected(*cases["count_zero"])[0]) == 0
    assert cases["one_segment_no_rows"][2].tolist() == [0, 0]


# ================================================================================================ counts
def test_count_inputs_stand_on_the_load_and_threshold_edges():
    R, T = fc.COUNT_TRIP, 4 * fc.COUNT_TRIP
    assert R == 4 * 4 * 1024                         # four 16-byte loads of four entries in each of 1 024 threads
    assert {0, 1, 3, 4, 5, 4095, 4096, 4097, R - 1, R, R + 1, T - 1, T, T + 1, T + 7} == set(fc.COUNT_SIZES)
    assert [n % 4 for n in (3, 5, 4095, 4097, R - 1, R + 1, T - 1, T + 1, T + 7)] == [3, 1, 3, 1, 3, 1, 3, 1, 3]   # scalar tails
    for thr in (fc.COUNT_THRESHOLD, 0):
        deg = fc.count_degrees(T + 7, thr)
        assert (deg == thr).any() and (deg == thr + 1).any() and (deg < thr).any() == (thr > 0) and deg[-1] == thr + 1
        strict, loose = fc.count_expected(deg, thr), int(deg.astype(np.int64)[deg >= thr].sum())
        assert (strict != loose) == (thr > 0)                                          # >= for > changes the answer
        assert fc.count_expected(deg[:-1], thr) != strict
    assert all((4 * k) % 16 != 0 for k in (1, 2, 3))                                   # views buf[1:], [2:], [3:]: no 16-byte alignment
    sat = fc.count_saturating()
    assert int(sat.astype(np.int64).sum()) == 2 ** 32 and fc.count_expected(sat, 0) == 0x7FFFFFFF
    assert fc.count_expected(sat[:2047], 0) == 2047 * 2 ** 20 < 0x7FFFFFFF


# ================================================================================================ comparing
def test_bit_comparison_helpers():
    a = np.array([0.0, -0.0, np.nan, 1.0, np.inf])
    assert fc.bits(a)[0] != fc.bits(a)[1]
    assert np.array_equal(fc.bits(a), fc.bits(np.array([0.0, -0.0, -np.nan, 1.0, np.inf])))
    assert fc.bits(a.astype(np.float32)).dtype == np.int32
    assert fc.ulp_distance(np.array([1.0, -1.0]), np.array([np.nextafter(1.0, 2), np.nextafter(-1.0, -2)])) == 1
    assert fc.ulp_distance(np.float32([90.0]), np.nextafter(np.float32([90.0]), np.float32(0))) == 1
