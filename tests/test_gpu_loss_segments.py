"""The detection loss with one result per group of rows (csrc/loss.hip: k_loss_seg, k_loss_seg_bwd; ``ops.detection_loss(...,
group_ptr=)``, ``losses.detection_loss(..., group_ptr=)``).

References: ``oracle.loss_oracle.detection_loss`` on each group in float64, and the existing single-result entry point on each
group's slice.  Bars: those of tests/test_gpu_loss_edges.py (its ``check``), applied per group; the gradient of
``sum_g coef[g] loss_g`` is held to ``coef[g]`` times the group's reference gradient, with the d cls bar scaled by ``coef[g]``."""
import math

import pytest
import torch

import test_gpu_loss_edges as E

pytestmark = pytest.mark.gpu
K, W, BG = 6, 5, 5


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    from radargnn_amd.gnn import losses
    return losses


@pytest.fixture(scope="module")
def ops(L):
    from radargnn_amd import ops
    return ops


def ptr_of(sizes):
    return torch.tensor([0] + list(torch.tensor(sizes).cumsum(0).tolist()), dtype=torch.int64)


def grouped(L, cls, bb, y, ptr, weights, coef=None, combine=None):
    c, b = cls.cuda().requires_grad_(True), bb.cuda().requires_grad_(True)
    outs = L.detection_loss(c, b, y.cuda(), BG, weights, E.ALPHA, E.BETA, group_ptr=ptr.cuda())
    g = ptr.numel() - 1
    assert all(o.shape == (g,) and o.dtype == torch.float32 for o in outs)
    if combine is not None:
        combine(outs).backward()
    else:
        torch.autograd.backward([outs[0]], [torch.ones(g, device="cuda") if coef is None else coef.cuda()])
    return [o.detach().cpu() for o in outs], c.grad.cpu(), b.grad.cpu()


def check_groups(L, name, cls, bb, y, sizes, weights, coef=None):
    ptr = ptr_of(sizes)
    (loss, lc, lb), dc, db = grouped(L, cls, bb, y, ptr, weights, coef)
    for g, (a, b) in enumerate(zip(ptr[:-1].tolist(), ptr[1:].tolist())):
        cf = 1.0 if coef is None else float(coef[g])
        if b == a:                                          # an empty group: what an empty batch gives
            assert math.isnan(float(loss[g])) and math.isnan(float(lc[g])) and float(lb[g]) == 0.0
            continue
        sl = slice(a, b)
        ref = E.reference(cls[sl], bb[sl], y[sl], BG, weights, E.ALPHA, E.BETA)
        ref["dc"], ref["db"] = ref["dc"] * cf, ref["db"] * cf
        got = {"loss": float(loss[g]), "lc": float(lc[g]), "lb": float(lb[g]), "dc": dc[sl], "db": db[sl]}
        scale = E.row_scale(cls[sl], y[sl], weights, E.ALPHA) * cf
        E.check(f"{name} group {g} rows {b - a}", got, ref, cls[sl], y[sl], weights, E.ALPHA, E.BETA, cls_scale=scale)
        if coef is None:                                    # the existing entry point on the slice, at the same bars
            one = E.device(L, cls[sl], bb[sl], y[sl], BG, weights, E.ALPHA, E.BETA)
            ref1 = E.reference(cls[sl], bb[sl], y[sl], BG, weights, E.ALPHA, E.BETA)
            E.check(f"{name} group {g} as a call of its own", one, ref1, cls[sl], y[sl], weights, E.ALPHA, E.BETA)
    return loss, lc, lb, dc, db


@pytest.mark.parametrize("sizes", [[257], [255, 256], [1, 255, 256, 257]], ids=["G1", "G2", "block-edges"])
@pytest.mark.parametrize("weights", [E.WEIGHTS6, None], ids=["weights", "no-weights"])
def test_groups_against_the_oracle(L, sizes, weights):
    n = sum(sizes)
    cls, bb, y = E.make(n, K, W, BG, 300 + n)
    y[0, 0] = 4.0                                           # (a one-row group must be an object for its box term to exist)
    check_groups(L, f"sizes {sizes}", cls, bb, y, sizes, weights)


def test_seven_groups_with_every_special_group_and_unequal_coefficients(L):
    """G = 7: one row, 255, none, 256 with an ignored label, 257, 40 rows without an object, 33 rows with a NaN box target --
    whose neighbours keep their box terms; coef differs from group to group."""
    sizes = [1, 255, 0, 256, 257, 40, 33]
    ptr = ptr_of(sizes)
    n = sum(sizes)
    cls, bb, y = E.make(n, K, W, BG, 77)
    y[0, 0] = 2.0
    y[int(ptr[3]) + 5, 0] = -100.0                          # a label outside [0, K): out of the cross entropy, still an object
    y[int(ptr[5]):int(ptr[6]), 0] = float(BG)               # a group without object nodes
    a = int(ptr[6])
    y[a + 3, 0] = 1.0
    y[a + 3, 2] = float("nan")                              # an object node's box target holds a NaN
    coef = torch.tensor([0.5, 2.0, 1.0, 0.25, 3.0, 1.5, 0.75])
    loss, lc, lb, dc, db = check_groups(L, "G7", cls, bb, y, sizes, E.WEIGHTS6, coef)
    assert float(lb[5]) == 0.0 and float(lb[6]) == 0.0 and float(lb[4]) > 0 and float(lb[3]) > 0
    assert bool((db[int(ptr[5]):] == 0).all()) and bool(torch.isfinite(dc).all()) and bool(torch.isfinite(db).all())
    assert float(dc[int(ptr[3]) + 5].abs().max()) == 0.0 and float(db[int(ptr[3]) + 5].abs().min()) > 0
    # the same with all-equal coefficients, as the trainer passes them (1 / 8: a power of two scales the reference exactly)
    check_groups(L, "G7 equal", cls, bb, y, sizes, E.WEIGHTS6, torch.full((7,), 1.0 / 8))


def test_sums_per_group_and_run_to_run_bits(L, ops):
    sizes = [255, 0, 257, 64]
    ptr = ptr_of(sizes).cuda()
    cls, bb, y = (t.cuda() for t in E.make(sum(sizes), K, W, BG, 5))
    w = torch.tensor(E.WEIGHTS6).cuda()
    out, sums = ops.detection_loss(cls, bb, y, w, BG, 1.0, E.ALPHA, E.BETA, group_ptr=ptr)
    assert out.shape == (4, 3) and sums.shape == (4, 4) and sums.dtype == torch.float64
    for g, (a, b) in enumerate(zip(ptr[:-1].tolist(), ptr[1:].tolist())):
        if a == b:
            assert sums[g].tolist() == [0.0, 0.0, 0.0, 0.0]
            continue
        _, one = ops.detection_loss(cls[a:b], bb[a:b], y[a:b], w, BG, 1.0, E.ALPHA, E.BETA)
        assert float(sums[g, 3]) == float(one[3])                                        # the number of object nodes
        assert torch.allclose(sums[g], one, rtol=1e-12, atol=0)                          # the same float terms, another order
    out2, sums2 = ops.detection_loss(cls, bb, y, w, BG, 1.0, E.ALPHA, E.BETA, group_ptr=ptr)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and torch.equal(sums.view(torch.int64), sums2.view(torch.int64))
    coef = torch.tensor([0.5, 1.0, 2.0, 0.25]).cuda()
    first = ops.detection_loss_bwd(cls, bb, y, w, BG, 1.0, E.ALPHA, E.BETA, sums, coef, group_ptr=ptr)
    second = ops.detection_loss_bwd(cls, bb, y, w, BG, 1.0, E.ALPHA, E.BETA, sums, coef, group_ptr=ptr)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_gradients_through_loss_cls_and_loss_bb(L):
    """``sum_g (2 loss_cls_g + 3 loss_bb_g)`` against the same expression over calls on the slices."""
    sizes = [65, 130]
    ptr = ptr_of(sizes)
    cls, bb, y = E.make(sum(sizes), K, W, BG, 91)
    _, dc, db = grouped(L, cls, bb, y, ptr, E.WEIGHTS6, combine=lambda o: (2.0 * o[1] + 3.0 * o[2]).sum())
    for a, b in zip(ptr[:-1].tolist(), ptr[1:].tolist()):
        one = E.device(L, cls[a:b], bb[a:b], y[a:b], BG, E.WEIGHTS6, E.ALPHA, E.BETA, 1.0, lambda o: 2.0 * o[1] + 3.0 * o[2])
        assert torch.allclose(dc[a:b], one["dc"], rtol=1e-5, atol=1e-9) and torch.allclose(db[a:b], one["db"], rtol=1e-5, atol=1e-9)
        assert float(one["dc"].abs().max()) > 0 and float(one["db"].abs().max()) > 0


def test_rows_outside_every_group_get_zero_gradients(L):
    cls, bb, y = E.make(12, K, W, BG, 13, obj_frac=0.9)
    ptr = torch.tensor([2, 6, 10], dtype=torch.int64)
    (loss, _, _), dc, db = grouped(L, cls, bb, y, ptr, E.WEIGHTS6)
    ref = E.reference(cls[2:6], bb[2:6], y[2:6], BG, E.WEIGHTS6, E.ALPHA, E.BETA)
    assert abs(float(loss[0]) - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    outside = [0, 1, 10, 11]
    assert bool((dc[outside] == 0).all()) and bool((db[outside] == 0).all()) and float(dc[2:10].abs().min()) > 0
