"""The dense-layer dispatch on the host (no GPU): rgnn_linear_fwd decides its kernel in ONE launch plan (plan_linear, linear.hip),
and rgnn_linear_fwd_path, rgnn_linear_fwd_fuses_a1_affine and rgnn_linear_fwd_plan are views of it.  The fixture
tests/golden/linear_dispatch_queries.npz holds what the two queries answered before the plan existed, when the decision was kept
in three copies (tests/golden/make_linear_dispatch_golden.py): 125 960 argument sets, under four settings of the environment."""
import ctypes as C
import os

import numpy as np
import pytest

import linear_dispatch_cases as cases
from conftest import GOLDEN

NONE, TINY, FP32, X3, DMA = range(5)                           # RGNN_LINEAR_FAMILY_*
# the tile widths each family instantiates (linear.hip: launch / launch_x3; linear_dma.hip: RGNN_DMA), by operand form
TILE_COLS = {(FP32, 0): {32, 64, 128, 96, 160, 192, 224}, (X3, 1): {32, 64, 128, 256},
             (DMA, 1): set(range(64, 225, 32)), (DMA, 2): set(range(64, 257, 32))}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "linear_dispatch_queries.npz"))


def _sweep(variant, monkeypatch, want_plan=False):
    from radargnn_amd import _lib, ops
    if variant != "default":
        monkeypatch.setenv(variant, "1")
    ops.reload_env()                                           # (undone after the test: monkeypatch, then conftest's autouse reload)
    return cases.sweep(_lib.lib, _lib.RgnnLinearArgs, want_plan)


def test_the_recorded_table_covers_the_grid_and_every_answer(golden):
    main = golden["section"] == "main"
    for name, values in cases.AXES:
        assert golden["axis_" + name].tolist() == list(values)
    assert int(main.sum()) == int(np.prod([len(v) for _, v in cases.AXES])) == 112640
    assert set(golden["section"].tolist()) == {"main", *cases.MODS}
    pairs = set(zip(golden["path_default"][main].tolist(), golden["fuses_default"][main].tolist()))
    assert pairs == {(p, f) for p in (0, 1, 2) for f in (0, 1)}          # all six: the grid has not degenerated


@pytest.mark.parametrize("variant", cases.VARIANTS)
def test_queries_and_plan_reproduce_the_recorded_dispatch(variant, golden, monkeypatch):
    sections, path, fuses, plan, n = _sweep(variant, monkeypatch, want_plan=True)
    assert sections.tolist() == golden["section"].tolist()
    for name, got in (("path", path), ("fuses", fuses)):
        want = golden[f"{name}_{variant}"]
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{name}: {bad.size} answers differ, first at case {bad[0]} ({sections[bad[0]]}): {got[bad[0]]} != {want[bad[0]]}"
    # the third view says the same as the other two, everywhere
    family, form, tile_cols, nt, subset, bufl, affine, split_k = plan.T
    assert np.array_equal(family == DMA, path != 0)
    assert np.array_equal((family == DMA) & (form == 2), path == 2)
    assert np.array_equal(np.where(family == DMA, form, 0), path)
    assert np.array_equal(affine, fuses)
    assert not (family == NONE).any() and not split_k.any()              # valid calls, none of which carries the scratch
    # tiles: the <= 8-wide-input kernel has none; every other family covers n with a width it instantiates
    tiny = family == TINY
    assert not tile_cols[tiny].any() and not nt[tiny].any()
    assert (tile_cols[~tiny] * nt[~tiny] >= n[~tiny]).all() and (tile_cols[~tiny] * (nt[~tiny] - 1) < n[~tiny]).all()
    for fam, frm, cols in set(zip(family[~tiny].tolist(), form[~tiny].tolist(), tile_cols[~tiny].tolist())):
        assert cols in TILE_COLS[(fam, frm)], (fam, frm, cols)
    assert not subset[(family != X3) & (family != DMA)].any() and bufl[(family == X3) | (family == DMA)].all()
    if variant == "default":
        assert {TINY, FP32, X3, DMA} == set(family.tolist())


def _one(fields):
    from radargnn_amd import _lib
    args, out = cases.fill(_lib.RgnnLinearArgs(), fields), (C.c_int32 * 8)()
    _lib.lib.rgnn_linear_fwd_plan(C.byref(args), C.byref(out))
    return _lib.lib.rgnn_linear_fwd_path(C.byref(args)), _lib.lib.rgnn_linear_fwd_fuses_a1_affine(C.byref(args)), list(out)


def test_an_unused_misaligned_w2_no_longer_promises_a_fused_affine():
    """w_split >= n, so W2 is unused, but it is not 16-byte aligned: rgnn_linear_fwd then leaves the buffer-descriptor path, on
    which alone the fp32 kernel applies a1_scale_shift.  The query used to leave W2 out of its alignment test, answered 1, and the
    launch refused with an `internal:` error; the query now follows the launch."""
    from radargnn_amd import _lib
    fields = cases.base_fields(3000, 64, 32, 0, 0, 0, 0, planes_kp=_lib.lib.rgnn_linear_planes_kp)
    assert _one(fields)[1:] == (1, [FP32, 0, 64, 1, 0, 1, 1, 0])
    fields.update(W2=cases.W2 + 4, a1_scale_shift=cases.TABLE)
    assert _one(fields) == (0, 0, [FP32, 0, 64, 1, 0, 0, 0, 0])
    # (no GPU needed: the refusal comes before any launch)
    args = cases.fill(_lib.RgnnLinearArgs(), fields)
    assert _lib.lib.rgnn_linear_fwd(C.byref(args), None) == -3 and b"internal" not in _lib.lib.rgnn_last_error()
    assert b"apply rgnn_scale_shift_act to A1 instead" in _lib.lib.rgnn_last_error()


def test_plan_of_calls_that_launch_nothing_and_split_k():
    from radargnn_amd import _lib
    kp = _lib.lib.rgnn_linear_planes_kp
    out = (C.c_int32 * 8)()
    _lib.lib.rgnn_linear_fwd_plan(None, C.byref(out))
    assert list(out) == [NONE] + [0] * 7
    assert _lib.lib.rgnn_linear_fwd_path(None) == 0 and _lib.lib.rgnn_linear_fwd_fuses_a1_affine(None) == 0
    for empty in (dict(m=0), dict(n=0), dict(k1=0, k2=0), dict(W1=None), dict(w_split=8)):
        fields = cases.base_fields(3000, 224, 224, 0, 1, 1, 0, planes_kp=kp)
        fields.update(empty)
        assert _one(fields) == (0, 0, [NONE] + [0] * 7), empty
    fields = cases.base_fields(3000, 224, 224, 0, 1, 1, 0, planes_kp=kp)
    assert _one(fields)[2][7] == 0
    fields.update(splitk_ws=cases.RES, splitk_ws_bytes=_lib.lib.rgnn_linear_splitk_ws_bytes())
    assert _one(fields)[2][0] == DMA and _one(fields)[2][7] == 1
    fields.update(splitk_ws_bytes=_lib.lib.rgnn_linear_splitk_ws_bytes() - 1)
    assert _one(fields)[2][7] == 0
