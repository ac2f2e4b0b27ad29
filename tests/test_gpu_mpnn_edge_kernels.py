"""The per-edge kernels of csrc/mpnn.hip on codes 0 - 2 (max | mean | add) and on the edge-hidden store, pinned on the hand-built CSRs
of tests/mpnn_csr_cases.py: k_mpnn (a launch without a chunk table, or rows that are no multiple of 16 bytes) and k_mpnn_fast (a launch
with ``ops.mpnn_partition``'s table where d % 4 == 0).  tests/test_gpu_aggr_ext.py pins codes 3 - 5 on the same cases; the layer
tests reach codes 0 - 2 only on random graphs at 1e-5.

Every case runs with and without the chunk table, with and without ``node_order``, with and without the target term P + p_bias (max
with the term is k_mpnn_fast's; without it and de <= 8 the launch is k_mpnn_max's, which tests/test_gpu_mpnn_bwd_edges.py pins), on both
variants of ``mc.int_inputs``.  Widths: d = 260 is two channel groups per lane with a ragged second one, 516 two blocks in y of two
groups each; d = 1 and 33 are no multiple of 4 and stay on k_mpnn; de = 3 | 8 | 9, 16 | 17, 32 are the attribute depths 4 | 8 | 16 | 32
(past 8 attributes k_mpnn_fast holds one channel group per lane).

Bars (integer data, float64 reference):
* max and add: the float64 reference cast to float32, bit for bit; rows of targets without edges exactly 0.
* add is exact in fp32 in ANY order because, per segment and channel, sum_e |m_e| + cnt |pn| < 2^24 (pn = P[t] + b): every partial
  sum and cnt * pn is an integer below 2^24.  Asserted here on the reference alone, on the CPU.
* mean: the float32 evaluation pn + float32(sum) / float32(cnt), bit for bit: the sum is exact, the division is correctly rounded
  and the sum with pn is rounded once.
* edge hidden: row e = relu?(P[t] + b + Q[s_e] + W_e a_e), bit for bit (integers far below 2^24)."""
import pytest
import torch

import mpnn_csr_cases as mc
from test_gpu_aggr_ext import FWD_CASES, f32, messages, target_nodes

pytestmark = pytest.mark.gpu

CHANNELS = (1, 8, 33, 224, 260, 516)
EDGE_WIDTHS = (0, 3, 8, 9, 16, 17, 32)
FULL_CROSS = ("degrees_1_to_8/empty_ends", "leftover_blocks")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test but no GPU visible")
    from radargnn_amd import ops as _ops
    return _ops


def widths(name):
    if name in FULL_CROSS:
        return [(d, de) for d in CHANNELS for de in EDGE_WIDTHS]
    return [(d, de) for d in (8, 260) for de in (3, 9)]


def same_bits(a, b) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def inputs(c, d, de, with_p, negative):
    """Integer tensors (int64): Q, We, ea, P, b -- ``mc.int_inputs`` and a target term in [-4, 4]."""
    Q, We, ea, b = mc.int_inputs(c, d=d, de=de, with_bias=with_p, negative=negative)
    P = torch.randint(-4, 5, (c.n, d), generator=torch.Generator().manual_seed(d + de)) if with_p else None
    return Q, We, ea, P, b


def variants(c, name):
    """(what, host tensors, device tensors, msg float64 [E, d]) for every width, input variant and target term."""
    for d, de in widths(name):
        for negative in (False, True):
            for with_p in (False, True):
                host = inputs(c, d, de, with_p, negative)
                Q, We, ea, P, b = host
                dev = tuple(f32(t) for t in host)
                yield f"{name} d={d} de={de} negative={negative} P={with_p}", host, dev, messages(c, Q, We, ea, torch.float64)


def target_term(c, P, b, d):
    pn = torch.zeros((c.n, d), dtype=torch.float64)
    if b is not None:
        pn = pn + b.double()
    if P is not None:
        pn = pn + P.double()
    return pn


@pytest.mark.parametrize("name", FWD_CASES)
def test_max_mean_add_are_bit_equal_on_integers(ops, name):
    c = mc.case(name)
    rowptr, src = c.rowptr_t.cuda(), c.src_sorted.cuda()
    table = ops.mpnn_partition(rowptr, c.n_edges)                            # (every launch leaves its ticket counters at zero)
    for what, (Q, We, ea, P, b), (Qd, Wd, ead, Pd, bd), msg in variants(c, name):
        d = Q.shape[1]
        pn = target_term(c, P, b, d)
        for order in c.orders():
            node = target_nodes(c, order)
            cnt = torch.bincount(node, minlength=c.n).double().view(-1, 1)
            has = (cnt > 0).expand(-1, d)
            total = torch.zeros((c.n, d), dtype=torch.float64).index_add_(0, node, msg)
            mag = torch.zeros((c.n, d), dtype=torch.float64).index_add_(0, node, msg.abs()) + cnt * pn.abs()
            assert float(mag.max()) < 2.0 ** 24, f"{what}: the sums of this case are not exact in fp32"
            top = torch.full((c.n, d), -float("inf"), dtype=torch.float64)
            if c.n_edges:
                top.scatter_reduce_(0, node[:, None].expand(-1, d), msg, "amax", include_self=True)
            zero64, zero32 = torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float32)
            pn32, total32, cnt32 = pn.to(torch.float32), total.to(torch.float32), cnt.to(torch.float32)
            exp = {"max": torch.where(has, pn + top, zero64).to(torch.float32),
                   "add": torch.where(has, cnt * pn + total, zero64).to(torch.float32),
                   "mean": torch.where(has, pn32 + total32 / cnt32.clamp(min=1.0), zero32)}
            od = None if order is None else order.cuda()
            for chunks in (None, table):
                for aggr in ("max", "mean", "add"):
                    out = ops.mpnn_aggregate(Pd, bd, Qd, Wd, ead, rowptr, src, aggr, node_order=od, chunks=chunks).cpu()
                    where = f"{what} order={order is not None} chunks={chunks is not None} {aggr}"
                    assert same_bits(out, exp[aggr]), f"{where}: {int((out != exp[aggr]).sum())} elements differ"
                    assert bool((out[~has] == 0).all()), where


@pytest.mark.parametrize("name", FWD_CASES)
def test_edge_hidden_is_bit_equal_on_integers(ops, name):
    c = mc.case(name)
    rowptr, src = c.rowptr_t.cuda(), c.src_sorted.cuda()
    table = ops.mpnn_partition(rowptr, c.n_edges)
    for what, (Q, We, ea, P, b), (Qd, Wd, ead, Pd, bd), msg in variants(c, name):
        d = Q.shape[1]
        pn = target_term(c, P, b, d)
        for order in c.orders():
            rows = (pn[target_nodes(c, order)] + msg).to(torch.float32)      # [E, d] in CSR order
            od = None if order is None else order.cuda()
            for chunks in (None, table):
                for relu in (False, True):
                    out = ops.mpnn_edge_hidden(Pd, bd, Qd, Wd, ead, rowptr, src, relu, node_order=od, chunks=chunks).cpu()
                    exp = rows.relu() if relu else rows
                    where = f"{what} order={order is not None} chunks={chunks is not None} relu={relu}"
                    assert same_bits(out, exp), f"{where}: {int((out != exp).sum())} elements differ"
