"""The feature, time-index and row-list kernels (csrc/features.hip) ON their edges: rounds of the time index's frame walk, the
hash set's wrap-around and its limit of distinct values, empty frames wherever they can stand, NaN rows of the undirected
point-pair features, the relative-position fast path against the general kernel, block / strip / tile sizes of every launch,
the aligned and the scalar path of the count kernel, and the frame_nonempty contract of rgnn_node_features_time_index.
tests/test_gpu_graph.py, test_gpu_fused_stage.py and test_gpu_frame_bn.py run the same kernels on golden frames and realistic
batches, which stand on none of these places.

Inputs and expectations: tests/feature_edge_cases.py (tests/test_feature_edge_cases.py proves on the CPU that each input stands
on its edge).  Reference: oracle/graph_oracle.py and a few lines of numpy; nothing here compares the device with itself except
where the second path is ALSO held to the oracle.  Everything goes through radargnn_amd.ops.

Bars.  Integer outputs (time index, frame_nonempty, row lists, counts, slots, padded list, tile map, panel starts, radius
counts): exact.  Every float64 column built from -, x, +, sqrt, fabs and / (distances, relative position and velocity, all node
columns): the oracle's bit pattern, sign of zero included, NaN = NaN -- what -ffp-contract=off and IEEE rounding give; no
column had to fall back from this on the device.  The three angle columns of the point-pair features: the oracle's NaN
pattern, finite values within rtol 1e-12 / atol 1e-9 (only acos itself can differ).  float32 output: the oracle's float64 result
cast with astype(float32), bit-equal on the exact columns (overflow to inf, underflow to subnormal or zero included), within one
float32 ulp on the angles."""
import functools

import numpy as np
import pytest
import torch

import feature_edge_cases as fc
from oracle import graph_oracle as go

pytestmark = pytest.mark.gpu

DTYPES = {"f64": torch.float64, "f32": torch.float32}
MODES = ("directed", "undirected")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    from radargnn_amd import ops as _ops
    return _ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def host(t):
    return t.detach().cpu().numpy()


def cast(want64, dtype):
    if dtype == "f64":
        return want64
    with np.errstate(over="ignore", under="ignore"):
        return want64.astype(np.float32)


def assert_same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    gb, wb = fc.bits(got), fc.bits(want)
    if not np.array_equal(gb, wb):
        bad = np.argwhere(gb != wb)
        finite = np.isfinite(got) & np.isfinite(want)
        ulps = fc.ulp_distance(got[finite], want[finite])
        first = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} entries differ in their bits (largest finite distance {ulps} ulp); first at "
                             f"{first}: got {got[first]!r}, expected {want[first]!r}")


# ================================================================================================ time index
TI_PATHS = ("one_block", "spread_out", "feature_launch")
TI_BATCHES = {"frame_sizes": fc.ti_size_batch, "value_kinds": fc.ti_value_batch, "distinct_counts": fc.ti_distinct_batch,
              "probe_wrap": fc.ti_wrap_batch, "frames_1025": fc.ti_many_frames,
              "no_frames": lambda: (np.zeros(0), np.zeros(1, dtype=np.int64))}


@functools.lru_cache(maxsize=None)
def ti_batch(name):
    ts, ptr = TI_BATCHES[name]()
    return ts, ptr, fc.ti_expected(ts, ptr)


def run_time_index(ops, ts, ptr, path):
    """The time index of a batch through one of the three instances -> (float64 [n] on the host, status word)."""
    T, P = dev(ts), dev(ptr)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    if path == "one_block":
        out, _ = ops.time_index(T, P, status)
    elif path == "spread_out":
        out, _ = ops.time_index(T, P, status, max_frame_points=fc.TI_SPREAD_HINT)
    else:
        X = torch.zeros((len(ts), 2), dtype=torch.float64, device="cuda")
        out = ops.node_features_time_index(X, None, None, T, P, None, ["time_index"], dtype=torch.float64, status=status)
        assert out.shape == (len(ts), 1)
        out = out.reshape(-1)
    torch.cuda.synchronize()
    return host(out), int(status.item())


@pytest.mark.parametrize("path", TI_PATHS)
@pytest.mark.parametrize("name", list(TI_BATCHES))
def test_time_index_at_every_edge(ops, name, path):
    """Frames of 1 / 1023 / 1024 / 1025 / 4095 / 4096 / 4097 / 8193 points with empty frames in front, doubled and at the back;
    every kind of value (-0.0 = 0.0, +-inf, +-5e-324, neighbours one ulp apart, ...); 1, 2, 3 071 and 3 072 distinct values; probe
    chains across slot 4 095 -> 0; 1 025 frames (where the spread-out hint is dropped); no frame at all -- np.unique's ranks and a
    clean status from k_time_index, from the k_ti_insert / sort / rank chain and from the feature launch."""
    ts, ptr, want = ti_batch(name)
    got, status = run_time_index(ops, ts, ptr, path)
    assert status == 0
    assert got.dtype == np.float64 and np.array_equal(got, want)


@pytest.mark.parametrize("path", TI_PATHS)
def test_time_index_overflow_flag_beyond_3072_distinct_values(ops, path):
    """A frame with 3 073 distinct timestamps raises STATUS_TIME_INDEX_OVERFLOW on every path (the output is not looked at)."""
    ts, ptr = fc.ti_overflow_batch()
    _, status = run_time_index(ops, ts, ptr, path)
    assert status == ops.STATUS_TIME_INDEX_OVERFLOW


# ================================================================================================ edge features
def check_edge_rows(got, want64, names, dtype, what):
    want = cast(want64, dtype)
    got = host(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    exact, angle = fc.edge_columns(names)
    assert_same_bits(got[:, exact], want[:, exact], (what, "exact columns"))
    if len(angle) and got.shape[0]:
        ga, wa = got[:, angle], want[:, angle]
        assert np.array_equal(np.isnan(ga), np.isnan(wa)), (what, "NaN pattern of the angles")
        ok = ~np.isnan(wa)
        if dtype == "f64":
            np.testing.assert_allclose(ga[ok], wa[ok], rtol=1e-12, atol=1e-9, err_msg=str(what))
        else:
            assert fc.ulp_distance(ga[ok], wa[ok]) <= 1, (what, "float32 angles beyond one ulp")


def edge_inputs(X, V, E):
    return dev(X), dev(V), dev(np.ascontiguousarray(E.T.astype(np.int64)))


def run_edge_features(ops, Xd, Vd, ei, names, mode, dtype):
    out, status = ops.edge_features(Xd, Vd, ei, names, mode, dtype=DTYPES[dtype])
    assert int(status.item()) == 0
    return out


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("mode", MODES)
def test_edge_features_on_lattice_degenerate_and_extreme_rows(ops, mode, dtype):
    """All five features on the 2 175 edges of the pool: velocities parallel, anti-parallel and perpendicular to lattice edges
    (u . u rounds above 1 in 24 of 168 directions: NaN rows in undirected mode, exactly 0 / 180 degrees in directed mode; mixed
    rows whose NaN survives Python's min / max in one edge direction only), coincident end points, a self loop, zero and -0.0
    velocities, coordinates of 1e39 and differences of 1e-46, a ring of generic points whose squares round."""
    X, V, E = fc.edge_pool()
    names = list(fc.EDGE_NAMES)
    want = go.edge_features(X, V, E, names, mode)
    assert np.isnan(want).any() == (mode == "undirected")
    got = run_edge_features(ops, *edge_inputs(X, V, E), names, mode, dtype)
    check_edge_rows(got, want, names, dtype, (mode, dtype))


@pytest.mark.parametrize("mode", MODES)
def test_edge_feature_lists(ops, mode):
    """Each name alone, all five in their five rotations, sixteen names (64 columns of point-pair features; a mixed list) on 513
    edges of the pool, float64 and float32: every column sits where its list puts it."""
    X, V, E = fc.sized_edges(513)
    Xd, Vd, ei = edge_inputs(X, V, E)
    for names in fc.edge_lists():
        want = go.edge_features(X, V, E, names, mode)
        for dtype in DTYPES:
            got = run_edge_features(ops, Xd, Vd, ei, names, mode, dtype)
            check_edge_rows(got, want, names, dtype, (names, dtype))
    assert go.edge_features(X, V, E, ["point_pair_features"] * 16, mode).shape == (513, 64)


@pytest.mark.parametrize("n_edges", fc.EDGE_SIZES)
def test_edge_feature_sizes(ops, n_edges):
    """0, 1, 255, 256, 257 and 513 edges (one thread per edge, 256 per block) through the general kernel and the
    relative-position fast path, both modes and dtypes."""
    X, V, E = fc.sized_edges(n_edges)
    Xd, Vd, ei = edge_inputs(X, V, E)
    for names in (list(fc.EDGE_NAMES), ["relative_position"]):
        for mode in MODES:
            want = go.edge_features(X, V, E, names, mode)
            for dtype in DTYPES:
                got = run_edge_features(ops, Xd, Vd, ei, names, mode, dtype)
                assert got.shape == (n_edges, sum(go.EDGE_FEATURE_WIDTH[nm] for nm in names))
                check_edge_rows(got, want, names, dtype, (names, mode, dtype))


def test_edge_feature_list_limits(ops):
    """The empty list gives [E, 0]; seventeen names are refused with ValueError; an unknown name raises the reference's message."""
    X, V, E = fc.sized_edges(257)
    Xd, Vd, ei = edge_inputs(X, V, E)
    rev = dev(np.arange(5, dtype=np.int32))
    for mode in MODES:
        for dtype in DTYPES.values():
            out, _ = ops.edge_features(Xd, Vd, ei, [], mode, dtype=dtype)
            assert out.shape == (257, 0) and out.dtype == dtype
            out, _ = ops.edge_features_reversed(Xd, Vd, ei, rev, [], mode, dtype=dtype)
            assert out.shape == (5, 0) and out.dtype == dtype
    with pytest.raises(ValueError):
        ops.edge_features(Xd, Vd, ei, ["relative_position"] * 17, "directed")
    with pytest.raises(ValueError):
        ops.edge_features_reversed(Xd, Vd, ei, rev, ["relative_position"] * 17, "directed")
    with pytest.raises(Exception, match="^Invalid feature specified$"):
        ops.edge_features(Xd, Vd, ei, ["relative_position", "bogus"], "directed")
    with pytest.raises(Exception, match="^Invalid feature specified$"):
        go.edge_features(X, V, E, ["relative_position", "bogus"], "directed")


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("mode", MODES)
def test_relative_position_fast_path_equals_the_general_kernel(ops, mode, dtype):
    """["relative_position"] alone (k_edge_relative_position) = the first two columns of ["relative_position",
    "relative_velocity"] (k_edge_features) on the pool's edges, bit for bit -- and both are the oracle's."""
    X, V, E = fc.edge_pool()
    Xd, Vd, ei = edge_inputs(X, V, E)
    fast = run_edge_features(ops, Xd, Vd, ei, ["relative_position"], mode, dtype)
    general = run_edge_features(ops, Xd, Vd, ei, ["relative_position", "relative_velocity"], mode, dtype)
    assert_same_bits(host(fast), host(general)[:, :2].copy(), (mode, dtype))
    want = go.edge_features(X, V, E, ["relative_position"], mode)
    assert (want < 0).any() == (mode == "directed")
    check_edge_rows(fast, want, ["relative_position"], dtype, (mode, dtype))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("mode", MODES)
def test_reversed_edge_features(ops, mode, dtype):
    """ops.edge_features_reversed with reversed_of a permuted subset, a list with repeats, and 0 / 1 / 257 rows of a 513-edge list:
    the oracle's features of the swapped end points, and bit for bit ops.edge_features on the swapped edge list."""
    X, V, E = fc.sized_edges(513)
    Xd, Vd, ei = edge_inputs(X, V, E)
    names = list(fc.EDGE_NAMES)
    for what, rev in fc.reversed_lists(len(E)).items():
        swapped = np.ascontiguousarray(E[rev.astype(np.int64)][:, ::-1])
        got, status = ops.edge_features_reversed(Xd, Vd, ei, dev(rev), names, mode, dtype=DTYPES[dtype])
        assert int(status.item()) == 0 and got.shape == (len(rev), 10)
        check_edge_rows(got, go.edge_features(X, V, swapped, names, mode), names, dtype, (what, mode, dtype))
        own = run_edge_features(ops, Xd, Vd, dev(np.ascontiguousarray(swapped.T)), names, mode, dtype)
        assert_same_bits(host(got), host(own), (what, mode, dtype, "reversed against the swapped list"))


# ================================================================================================ node features
@pytest.mark.parametrize("n", fc.NODE_SIZES)
def test_node_features_at_block_edges(ops, n):
    """0, 1, 255, 256 and 257 nodes; each of the six names alone, in six rotations, and sixteen names; degrees 0, 2^24 + 1 and
    2^31 - 1, rcs with -0.0, +-inf and NaN, coordinates and velocities of 1e39 and 1e-46: ops.node_features with a given time-index
    column and the fused launch with its own (three frames, the middle one empty) give the oracle's bits in float64 and the bits of
    its astype(float32) in float32."""
    c = fc.node_case(n)
    X, V, rcs, deg = dev(c["X"]), dev(c["V"]), dev(c["rcs"]), dev(c["degree"])
    tidx, ts, ptr = dev(c["time_index"]), dev(c["timestamp"]), dev(c["frame_ptr"])
    own_index = fc.ti_expected(c["timestamp"], c["frame_ptr"])
    for names in fc.node_lists():
        width = sum(go.NODE_FEATURE_WIDTH[nm] for nm in names)
        want_given, want_own = fc.node_expected(c, names, c["time_index"]), fc.node_expected(c, names, own_index)
        assert want_given.shape == (n, width)
        for dtype, tdtype in DTYPES.items():
            got = ops.node_features(X, V, rcs, tidx, deg, names, dtype=tdtype)
            assert_same_bits(host(got), cast(want_given, dtype), (names, dtype, "node_features"))
            status = torch.zeros(1, dtype=torch.int32, device="cuda")
            got = ops.node_features_time_index(X, V, rcs, ts, ptr, deg, names, dtype=tdtype, status=status)
            assert int(status.item()) == 0
            assert_same_bits(host(got), cast(want_own, dtype), (names, dtype, "node_features_time_index"))


def test_node_features_without_a_time_index(ops):
    """time_index=None is accepted by a list that does not ask for it and refused by one that does."""
    from radargnn_amd._lib import RgnnError
    c = fc.node_case(257)
    X, V, rcs, deg = dev(c["X"]), dev(c["V"]), dev(c["rcs"]), dev(c["degree"])
    names = [nm for nm in fc.NODE_NAMES if nm != "time_index"]
    got = ops.node_features(X, V, rcs, None, deg, names, dtype=torch.float64)
    assert_same_bits(host(got), fc.node_expected(c, names, None), "without time_index")
    with pytest.raises(RgnnError, match="time_index requested but NULL"):
        ops.node_features(X, V, rcs, None, deg, list(fc.NODE_NAMES), dtype=torch.float64)


# ================================================================================================ frame split
SPLIT_BATCHES = {"strip_edges": lambda: np.array(fc.SPLIT_FRAME_SIZES), "frames_1030": fc.split_many_frame_sizes}


def check_split(ops, degree, ptr, frame_nonempty, want, what):
    lst, cnt, slot, lst_ne, cnt_ne = ops.split_by_degree_frames(degree, ptr, frame_nonempty)
    torch.cuda.synchronize()
    assert (int(cnt.item()), int(cnt_ne.item())) == (want["count_empty"], want["count_nonempty"]), what
    assert np.array_equal(host(lst)[:want["count_empty"]], want["list_empty"]), what
    assert np.array_equal(host(lst_ne)[:want["count_nonempty"]], want["list_nonempty"]), what
    assert np.array_equal(host(slot)[:len(want["slot"])], want["slot"]), what


@pytest.mark.parametrize("pattern", fc.DEGREE_PATTERNS)
@pytest.mark.parametrize("name", list(SPLIT_BATCHES))
def test_split_by_degree_frames_at_strip_and_frame_edges(ops, name, pattern):
    """Frames of 0 / 1 / 1023 / 1024 / 1025 / 0 / 0 / 2049 / 1 nodes, and 1 030 frames of 0 ... 3 nodes; degrees all zero, all
    positive, alternating, only the last and only the first node positive.  frame_nonempty once counted with numpy and once as the
    side output of ops.node_features_time_index (which must equal it): np.nonzero's two lists, their counts and the slots."""
    sizes = SPLIT_BATCHES[name]()
    ptr_h, n = fc.ptr_of(sizes), int(sizes.sum())
    deg_h = fc.degree_pattern(pattern, n)
    want = fc.split_expected(deg_h, ptr_h)
    degree, ptr = dev(deg_h), dev(ptr_h)
    check_split(ops, degree, ptr, dev(want["frame_nonempty"]), want, "numpy counts")
    side = torch.full((len(sizes),), -7, dtype=torch.int32, device="cuda")
    X = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    x = ops.node_features_time_index(X, None, None, torch.zeros(n, dtype=torch.float64, device="cuda"), ptr, degree,
                                     ["degree", "time_index"], dtype=torch.float32, frame_nonempty=side)
    assert np.array_equal(host(side), want["frame_nonempty"])
    assert np.array_equal(host(x), np.stack([deg_h.astype(np.float32), np.zeros(n, dtype=np.float32)], 1))
    check_split(ops, degree, ptr, side, want, "side output")


# ================================================================================================ padded lists
@functools.lru_cache(maxsize=None)
def pad_cases():
    return fc.pad_cases()


def check_padded(result, want, what):
    out, total, tiles, start = result
    want_out, want_tiles, want_start = want
    assert int(total.item()) == len(want_out), what
    assert np.array_equal(host(out)[:len(want_out)], want_out), what
    assert np.array_equal(host(tiles)[:len(want_out) // fc.PAD_ROWS], want_tiles), what
    assert np.array_equal(host(start), want_start), what


@pytest.mark.parametrize("name", list(fc.pad_cases()))
def test_pad_list_by_segment_at_tile_and_segment_edges(ops, name):
    """One segment and 257 segments (beyond the prefix loop's stride of 256) with 0 / 1 / 255 / 256 / 257 / 512 entries, empty
    row ranges, ranges without entries, the whole list inside one segment, a list that ends before the last segment, count = 0;
    the buffer is longer than the list and full of garbage there."""
    buf, count, seg = pad_cases()[name]
    result = ops.pad_list_by_segment(dev(buf), torch.tensor([count], dtype=torch.int64, device="cuda"), dev(seg))
    torch.cuda.synchronize()
    check_padded(result, fc.pad_expected(buf, count, seg), name)


def test_pad_list_pair_equals_two_single_calls(ops):
    """ops.pad_list_pair_by_segment (the form gnn/linear.py uses) over 257 segments with two lists of different length -- the full
    one, every third entry of it, and an empty one, in either place: each half is numpy's padding of ITS list and what the
    single-list call returns."""
    buf, count, seg = pad_cases()["257_segments"]
    third = np.full(len(buf), fc.PAD_GARBAGE, dtype=np.int32)
    third[:len(buf[:count:3])] = buf[:count:3]
    lists = {"full": (buf, count), "third": (third, len(buf[:count:3])), "empty": (np.full(40, fc.PAD_GARBAGE, dtype=np.int32), 0)}
    assert lists["third"][1] not in (0, count)
    S = dev(seg)
    on_dev = {k: (dev(b), torch.tensor([c], dtype=torch.int64, device="cuda")) for k, (b, c) in lists.items()}
    want = {k: fc.pad_expected(b, c, seg) for k, (b, c) in lists.items()}
    single = {k: ops.pad_list_by_segment(*on_dev[k], S) for k in lists}
    for a, b in (("full", "third"), ("third", "full"), ("full", "empty"), ("empty", "third")):
        ra, rb = ops.pad_list_pair_by_segment(*on_dev[a], *on_dev[b], S)
        torch.cuda.synchronize()
        for half, key in ((ra, a), (rb, b)):
            check_padded(half, want[key], (a, b, key))
            n = len(want[key][0])
            assert int(half[1].item()) == int(single[key][1].item())
            assert torch.equal(half[0][:n], single[key][0][:n]) and torch.equal(half[2][:n // fc.PAD_ROWS], single[key][2][:n // fc.PAD_ROWS])
            assert torch.equal(half[3], single[key][3])


# ================================================================================================ counts
@pytest.mark.parametrize("n", fc.COUNT_SIZES)
def test_radius_counts_on_every_load_path(ops, n):
    """n around 4 entries (one 16-byte load), 4 096, one trip (16 384) and four trips (65 536) of the 16-byte loop, with scalar
    tails of 1 and 3; the same degrees through an aligned view and through views 4, 8 and 12 bytes off (the scalar path);
    degrees equal to the threshold (not counted) and one above (counted), threshold 60 and 0; rowptr an array of its own whose
    last entry comes back as out[0]."""
    for threshold in (fc.COUNT_THRESHOLD, 0):
        deg_h = fc.count_degrees(n, threshold)
        want = fc.count_expected(deg_h, threshold)
        rowptr_h = np.arange(n + 1, dtype=np.int32) * 3 + 11
        rowptr_h[-1] = 987654 + n
        rowptr = dev(rowptr_h)
        for off in range(4):
            buf = torch.full((n + 8,), 1 << 20, dtype=torch.int32, device="cuda")
            view = buf[off:off + n]
            view.copy_(torch.from_numpy(deg_h))
            if n:
                assert view.data_ptr() % 16 == 4 * off
            got = ops.radius_counts(view, rowptr, threshold).tolist()
            assert got == [987654 + n, want], (threshold, off)


def test_radius_counts_saturate(ops):
    """4 096 degrees of 2^20 add up to 2^32: out[1] is 0x7fffffff, on the 16-byte path and on the scalar path; 2 047 of them do
    not saturate."""
    deg_h = fc.count_saturating()
    rowptr = dev(np.full(len(deg_h) + 1, 5, dtype=np.int32))
    for off in (0, 1):
        buf = torch.zeros(len(deg_h) + 4, dtype=torch.int32, device="cuda")
        view = buf[off:off + len(deg_h)]
        view.copy_(torch.from_numpy(deg_h))
        assert ops.radius_counts(view, rowptr, 0).tolist() == [5, fc.COUNT_SATURATED]
        assert ops.radius_counts(view[:2047], rowptr[:2048], 0).tolist() == [5, 2047 * 2 ** 20]


# ================================================================================================ the frame_nonempty contract
def test_frame_nonempty_is_filled_when_there_are_no_nodes(ops):
    """rgnn_node_features_time_index with n == 0 and three (empty) frames: frame_nonempty comes back as zeros, and the split that
    reads it returns two empty lists."""
    ptr = torch.zeros(4, dtype=torch.int64, device="cuda")
    empty = torch.zeros(0, dtype=torch.float64, device="cuda")
    degree = torch.zeros(0, dtype=torch.int32, device="cuda")
    side = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    x = ops.node_features_time_index(empty.reshape(0, 2), None, empty, empty, ptr, degree, ["rcs", "degree", "time_index"],
                                     frame_nonempty=side)
    assert x.shape == (0, 3) and side.tolist() == [0, 0, 0]
    lst, cnt, slot, lst_ne, cnt_ne = ops.split_by_degree_frames(degree, ptr, side)
    assert (int(cnt.item()), int(cnt_ne.item())) == (0, 0)


def test_frame_nonempty_is_filled_under_an_empty_feature_list(ops):
    """rgnn_node_features_time_index with an empty feature list and degrees given (frames at the strip edges, alternating
    degrees): frame_nonempty is numpy's count per frame, and the split that reads it is numpy's."""
    sizes = np.array(fc.SPLIT_FRAME_SIZES)
    ptr_h, n = fc.ptr_of(sizes), int(sizes.sum())
    deg_h = fc.degree_pattern("alternating", n)
    want = fc.split_expected(deg_h, ptr_h)
    degree, ptr = dev(deg_h), dev(ptr_h)
    side = torch.full((len(sizes),), -7, dtype=torch.int32, device="cuda")
    X = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    x = ops.node_features_time_index(X, None, None, None, ptr, degree, [], frame_nonempty=side)
    assert x.shape == (n, 0) and np.array_equal(host(side), want["frame_nonempty"])
    check_split(ops, degree, ptr, side, want, "empty feature list")
