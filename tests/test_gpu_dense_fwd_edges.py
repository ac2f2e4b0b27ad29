"""The forward dense layer rgnn_linear_fwd -- k_linear_tiny, the fp32 MFMA kernel, k_linear_x3 and the LDS-DMA kernel in both forms
and under all three schedules -- on the hand-built operands of tests/dense_fwd_cases.py: every output is a sum of integers below
2^24 in its sum of |terms|, so every planned instance must return the int64 reference BIT FOR BIT: a wrong last column of a
ragged tile, a k-tail element, a bias from the neighbouring column, a split product dropped in one instance, a row the launch
should not have touched each fail an equality.  Every case first asks rgnn_linear_fwd_plan with its real arguments and asserts
the instance it was built for (tests/test_dense_fwd_cases.py proves the same rows on the CPU), then launches through
RgnnLinearArgs itself; a few cases at the end go through ops.linear to pin the wrapper's plumbing on views."""
import ctypes as C

import numpy as np
import pytest
import torch

import dense_fwd_cases as fc

pytestmark = pytest.mark.gpu
IDS = lambda c: c.name


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    from radargnn_amd import ops as o
    return o


@pytest.fixture(scope="module")
def scratch(ops):
    """The split-K / stream-K scratch of this file: zeroed ONCE; every launch must leave its flag words zero again."""
    from radargnn_amd._lib import lib
    return torch.zeros(int(lib.rgnn_linear_splitk_ws_bytes()), dtype=torch.uint8, device="cuda")


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def set_switches(ops, monkeypatch, env):
    for name in fc.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name in env:
        monkeypatch.setenv(name, "1")
    ops.reload_env()                                  # (undone after the test: monkeypatch, then conftest's autouse reload)


def first_difference(got, want, what):
    bad = (got != want) | (torch.isnan(got) != torch.isnan(want))
    idx = bad.nonzero()[0].tolist()
    return (f"{what}: {int(bad.sum())} of {bad.numel()} words differ, first at {idx}: {got[tuple(idx)].item()!r} != "
            f"{want[tuple(idx)].item()!r}; rows {sorted(set(bad.nonzero()[:, 0].tolist()))[:8]}, "
            f"columns {sorted(set(bad.nonzero()[:, -1].tolist()))[:8]}")


class Launch:
    """Case ``c`` on the device: every operand a view into its wider allocation, the arguments filled by dense_fwd_cases.fields
    from the allocations' addresses."""

    def __init__(self, ops, c, scratch=None):
        from radargnn_amd import _lib
        self.ops, self.c, self.lib = ops, c, _lib.lib
        op = self.op = fc.Operands(c)
        self.lst, self.count, t = op.list, (c.rows[1] if c.rows else None), {}
        if c.affine == "segments":                    # the list and the tile -> table map come from the library
            base = fc.segment_base_list(c)
            padded, total, tiles, _ = ops.pad_list_by_segment(cuda(base), torch.tensor([len(base)], dtype=torch.int64, device="cuda"),
                                                              torch.tensor(c.segments, dtype=torch.int64, device="cuda"))
            self.count = int(total.item())
            self.lst = padded[:self.count].cpu().numpy()
            want_list, want_tiles = fc.pad_list_emulated(c)
            assert np.array_equal(self.lst, want_list) and np.array_equal(tiles[:self.count // 256].cpu().numpy(), want_tiles)
            t["rows"], t["mdev"], t["segs"] = padded, total, tiles
        elif c.rows is not None:
            t["rows"] = cuda(self.lst)
            if self.count is not None:
                t["mdev"] = torch.tensor([self.count], dtype=torch.int64, device="cuda")
        self.ref = op.reference(self.lst, self.count)
        for which in ("a1", "a2", "w") + (("res",) if c.residual else ()):
            t[which] = cuda(op.wide(which, self.lst))
        t["b1"], t["b2"] = cuda(op.bias_alloc("b1")), cuda(op.bias_alloc("b2"))
        self.out0 = cuda(op.out_alloc())
        t["out"] = self.out0.clone()
        if c.residual == "index":
            t["resindex"] = cuda(op.res_index)
        self.panels = fc.ceil_div(max(self.ref["M"], c.m), fc.BM) + 1              # one more than any launch may write
        if c.stats:
            t["stats"] = torch.full((self.panels, fc.STAT_ROWS, c.n), float(fc.STAT_SENTINEL), dtype=torch.float32, device="cuda")
        kp = int(self.lib.rgnn_linear_planes_kp(c.k))
        off = c.view("w")[0]
        w_view = t["w"][:, off:off + c.k]
        if c.form != "fp32":
            t["planes"], kp_ = ops.weight_planes(w_view, None, c.k, cache=False)
            assert kp_ == kp and kp % fc.BK == 0 and kp >= c.k
        if c.form == "f16x2":
            t["planes16"] = ops.weight_planes_f16(w_view, None, c.k, cache=False)
            b1, b2 = op.bounds(self.lst)
            t["bound1"] = ops.make_bound(torch.tensor(b1, dtype=torch.float32, device="cuda"))
            t["bound2"] = ops.make_bound(torch.tensor(b2, dtype=torch.float32, device="cuda"))
        if c.absmax:
            t["absmax"] = torch.zeros(fc.BOUND_SLOTS, dtype=torch.float32, device="cuda")
        if c.affine:
            t["table"] = cuda(op.table)
        if c.ws:
            t["ws"] = scratch
        self.t = t
        base = {name: (t[name].data_ptr() if name in t else 0) for name in fc.ALLOCATIONS}
        f = fc.fields(c, base, kp, scratch.numel() if c.ws else 0)
        self.args = _lib.RgnnLinearArgs()
        for k, v in f.items():
            setattr(self.args, k, v)

    def plan(self):
        out = (C.c_int32 * 8)()
        self.lib.rgnn_linear_fwd_plan(C.byref(self.args), C.byref(out))
        return tuple(out)

    def launch(self):
        return self.lib.rgnn_linear_fwd(C.byref(self.args), self.ops._stream())

    def reset(self):
        self.t["out"].copy_(self.out0)
        if "absmax" in self.t:
            self.t["absmax"].zero_()
        if "stats" in self.t:
            self.t["stats"].fill_(float(fc.STAT_SENTINEL))

    def check(self, what=""):
        c, ref, t, ops = self.c, self.ref, self.t, self.ops
        name = c.name + what
        got, want = t["out"].cpu(), torch.from_numpy(ref["out"].astype(np.float32))
        assert torch.equal(got, want), first_difference(got, want, name + " out (result, sentinel rows, columns and ldo padding)")
        if c.stats:
            st = t["stats"]
            P = ref["panels_written"]
            for p in range(P):
                cnt, s1, s2 = (x.cpu() for x in ops.stats_to_sums(st[p:p + 1]))
                print(f"[{name}] panel {p}: rows {cnt[0].item():.0f}")
                for got_, want_, nm in ((cnt, ref["stats"][p, 0], "count"), (s1, ref["stats"][p, 1], "sum"), (s2, ref["stats"][p, 2], "sum of squares")):
                    want_ = torch.from_numpy(want_)
                    assert torch.equal(got_, want_), first_difference(got_[None], want_[None], f"{name} statistics panel {p} {nm}")
            assert bool((st[P:] == float(fc.STAT_SENTINEL)).all()), f"{name}: a statistics panel beyond the launch's rows was written"
        if c.absmax:
            got_max = float(t["absmax"].max().item())
            print(f"[{name}] out_absmax {got_max} reference {ref['absmax']}")
            assert got_max == ref["absmax"], (name, "out_absmax", got_max, ref["absmax"], "absent rows would give", ref["phantom"])
        if c.ws:
            flags = t["ws"][-fc.SPLITK_FLAG_BYTES:].view(torch.int32)
            assert int(flags[fc.SPLITK_TIMEOUT_WORD].item()) == 0, f"{name}: a work-group gave up waiting for a partial tile"
            assert not bool(flags.any()), f"{name}: flag words left set: {flags.nonzero().flatten().tolist()[:8]}"


def run(ops, c, monkeypatch, scratch, repeats=1):
    set_switches(ops, monkeypatch, c.env)
    L = Launch(ops, c, scratch)
    assert L.plan() == c.expect, (c.name, L.plan(), c.expect)
    for i in range(repeats):
        if i:
            L.reset()
        rc = L.launch()
        if c.rc != 0:
            assert rc == c.rc, (c.name, rc)
            assert torch.equal(L.t["out"], L.out0)                   # refused, not launched
            return L
        assert rc == 0, (c.name, L.lib.rgnn_last_error().decode())
        L.check("" if repeats == 1 else f" (launch {i + 1})")
    return L


# ------------------------------------------------------------------------------------------------ the families
@pytest.mark.parametrize("c", fc.TINY_CASES, ids=IDS)
def test_tiny_kernel_is_exact(ops, scratch, monkeypatch, c):
    run(ops, c, monkeypatch, scratch)


@pytest.mark.parametrize("c", fc.FP32_CASES, ids=IDS)
def test_fp32_kernel_is_exact(ops, scratch, monkeypatch, c):
    """Every tile width, loader and epilogue of k_linear; a case the dispatcher must refuse returns RGNN_ERR_UNSUPPORTED and
    stores nothing."""
    run(ops, c, monkeypatch, scratch)


@pytest.mark.parametrize("c", fc.X3_CASES, ids=IDS)
def test_register_staged_split_product_is_exact(ops, scratch, monkeypatch, c):
    """k_linear_x3 at its four tile widths, direct and on a row list, with NaN behind the k columns of every activation row
    against planes zero-padded to kp > k."""
    run(ops, c, monkeypatch, scratch)


@pytest.mark.parametrize("c", fc.DMA_CASES, ids=IDS)
def test_lds_dma_kernel_is_exact(ops, scratch, monkeypatch, c):
    """Every TN of both forms, direct and subset; out_absmax is the exact maximum of what the launch stores."""
    run(ops, c, monkeypatch, scratch)


@pytest.mark.parametrize("c", fc.SCHEDULE_CASES, ids=IDS)
def test_lds_dma_schedules_are_exact_and_leave_the_flags_zero(ops, scratch, monkeypatch, c):
    """Static, parallel split-K and the stream-K hand-over all return the same int64 reference; twice in a row on the same
    scratch, whose whole flag area is zero after either launch."""
    run(ops, c, monkeypatch, scratch, repeats=2)


def test_two_subset_launches_share_one_out_and_one_bound(ops, scratch, monkeypatch):
    """The two halves of a conv layer's update: disjoint row lists into one `out`, one out_absmax raised by both."""
    set_switches(ops, monkeypatch, ("RGNN_DMA_NO_SMALL_M",))
    for form in ("bf16x3", "f16x2"):
        c = fc.Case(f"pair_{form}", 600, 100, 32, 16, form=form, rows=("perm", 513), absmax=True, env=("RGNN_DMA_NO_SMALL_M",))
        A = Launch(ops, c, scratch)
        # second launch: the rows the first did not name, same operands, same out, same bound
        rest = np.setdiff1d(np.arange(c.m), A.op.named_rows()).astype(np.int32)
        assert len(rest) == 87
        B = Launch(ops, c, scratch)
        B.lst = np.concatenate([rest[::-1], np.full(5, fc.LIST_TAIL, dtype=np.int32)]).astype(np.int32)
        B.t["rows"], B.t["mdev"] = cuda(B.lst), torch.tensor([len(rest)], dtype=torch.int64, device="cuda")
        for which in ("a1", "a2"):                                   # every row live now: the first launch's rows stay what they were
            full = np.where(np.isnan(A.op.wide(which, A.lst)), A.op.wide(which, B.lst), A.op.wide(which, A.lst))
            A.t[which].copy_(cuda(full))
        for name in ("a1", "a2", "out", "absmax"):
            B.t[name] = A.t[name]
        f = fc.fields(c, {n: (B.t[n].data_ptr() if n in B.t else 0) for n in fc.ALLOCATIONS}, int(A.lib.rgnn_linear_planes_kp(c.k)), 0)
        for k, v in f.items():
            setattr(B.args, k, v)
        assert A.plan()[:5] == B.plan()[:5] == (fc.DMA, 1 if form == "bf16x3" else 2, 128, 1, 1)
        assert A.launch() == 0
        first = float(A.t["absmax"].max().item())
        assert first == A.ref["absmax"]
        assert B.launch() == 0
        ref_b = A.op.reference(B.lst, len(rest))
        want = A.ref["out"].copy()
        want[ref_b["touched"]] = ref_b["out"][ref_b["touched"]]
        got, want = A.t["out"].cpu(), torch.from_numpy(want.astype(np.float32))
        assert torch.equal(got, want), first_difference(got, want, c.name)
        assert bool((got[:c.m, 4:4 + c.n] != float(fc.SENTINEL)).all())             # every row written by one of the two
        assert float(A.t["absmax"].max().item()) == max(A.ref["absmax"], ref_b["absmax"])


# ------------------------------------------------------------------------------------------------ through ops.linear
def _int_matrix(rng, rows, cols, amp, ld, off=0):
    """(values int64 [rows, cols], their float32 view into a NaN-filled [rows, ld] allocation on the device)."""
    x = rng.integers(1, amp + 1, size=(rows, cols)) * rng.choice([-1, 1], size=(rows, cols))
    wide = np.full((rows, ld), np.nan, dtype=np.float32)
    wide[:, off:off + cols] = x
    return x, cuda(wide)[:, off:off + cols]


def test_wrapper_out_view_and_two_weight_views(ops):
    """ops.linear with out= a column view of a wider matrix and w1 / w2 column views of ONE weight allocation."""
    rng = np.random.default_rng(11)
    m, k, n1, n2 = 131, 36, 40, 24
    a, a_dev = _int_matrix(rng, m, k, 7, k + 12, 4)
    w, w_dev = _int_matrix(rng, n1 + n2, k, 7, k + 8, 4)
    b1, b2 = np.arange(n1) % 23 - 11, np.arange(n2) % 19 - 9
    out_wide = torch.full((m, n1 + n2 + 9), float(fc.SENTINEL), device="cuda")
    out = out_wide[:, 5:5 + n1 + n2]
    got = ops.linear(a_dev, w_dev[:n1], cuda(b1.astype(np.float32)), w2=w_dev[n1:], bias2=cuda(b2.astype(np.float32)), relu=True, relu_from=n1, out=out)
    want = a @ w.T + np.concatenate([b1, b2])
    want[:, n1:] = np.maximum(want[:, n1:], 0)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out.cpu(), torch.from_numpy(want.astype(np.float32)))
    edge = torch.cat([out_wide[:, :5], out_wide[:, 5 + n1 + n2:]], dim=1)
    assert bool((edge == float(fc.SENTINEL)).all())


@pytest.mark.parametrize("k2", [40, 48], ids=["x3", "dma"])
def test_wrapper_a2_from_padded_rows_with_nan_padding(ops, k2):
    """A2 as ops.padded_rows hands it out (row stride rounded up to 32 floats, the padding uninitialised -- NaN here) against
    planes zero-padded to kp = 96 > k: k2 = 40 takes k_linear_x3 (K = 72), k2 = 48 the LDS-DMA kernel (K = 80)."""
    rng = np.random.default_rng(12 + k2)
    m, k1, n = 300, 32, 72
    a1, a1_dev = _int_matrix(rng, m, k1, 7, k1, 0)
    a2 = rng.integers(-7, 8, size=(m, k2))
    a2_dev = ops.padded_rows(m, k2, "cuda")
    assert a2_dev.stride(0) == 64 and a2_dev._base is not None
    a2_dev._base.fill_(float("nan"))
    a2_dev.copy_(cuda(a2.astype(np.float32)))
    assert bool(torch.isnan(a2_dev._base[:, k2:]).all())
    w, w_dev = _int_matrix(rng, n, k1 + k2, 7, k1 + k2, 0)
    b = np.arange(n) % 23 - 11
    out, stats = ops.linear(a1_dev, w_dev, cuda(b.astype(np.float32)), a2=a2_dev, relu=False, want_stats=True)
    want = np.concatenate([a1, a2], axis=1) @ w.T + b
    assert torch.equal(out.cpu(), torch.from_numpy(want.astype(np.float32)))
    cnt = ops.stats_to_sums(stats)[0].cpu()
    assert torch.equal(cnt, torch.full((n,), float(m), dtype=torch.float64))


def test_wrapper_row_list_f16x2_with_tracked_bound(ops):
    """ops.linear on a row list inside bound tracking: the f16x2 form is taken, rows outside the list keep what they held, and
    the bound attached to the result is the exact maximum of the stored values."""
    rng = np.random.default_rng(14)
    m, k, n, cnt = 400, 48, 100, 257
    a, a_dev = _int_matrix(rng, m, k, 7, k + 16, 8)
    w, w_dev = _int_matrix(rng, n, k, 7, k, 0)
    b = np.arange(n) % 23 - 11
    lst = rng.permutation(m)[:cnt]
    rows = cuda(np.concatenate([lst, np.full(m - cnt, 0)]).astype(np.int32))          # (the wrapper bounds the matrix rows by the list's length)
    out = torch.full((m, n), float(fc.SENTINEL), device="cuda")
    before = ops.COUNTERS.get("f16x2", 0)
    with ops.bound_tracking("cuda"):
        ops.set_bound(a_dev, ops.make_bound(torch.tensor(7.0, device="cuda")))
        got = ops.linear(a_dev, w_dev, cuda(b.astype(np.float32)), relu=True, out=out, row_index=rows,
                         m_dev=torch.tensor([cnt], dtype=torch.int64, device="cuda"))
        word = ops.bound_of(got)
    assert ops.COUNTERS.get("f16x2", 0) == before + 1
    want = np.full((m, n), float(fc.SENTINEL))
    want[lst] = np.maximum(a[lst] @ w.T + b, 0)
    assert torch.equal(out.cpu(), torch.from_numpy(want.astype(np.float32)))
    assert word is not None and float(word.max().item()) == float(want[lst].max())
