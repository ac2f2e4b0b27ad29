"""CPU restatement of the aggregations min | var | std as the reference's layers get them from torch_geometric 2.1.0
(``MessagePassing(aggr=...)`` -> ``nn/aggr/basic.py``) and torch-scatter, in plain torch index ops.  TEST INFRASTRUCTURE ONLY; needs
no GPU.  Neither package can be imported here, so the semantics are restated from their published behaviour, next to the ones
``oracle/gnn_oracle.py`` states for max | mean | add.  Per channel, m_e the messages of the edges into target t, cnt their number:

* ``min``  min_e m_e; an empty segment gives exactly 0.  Backward (torch-scatter ``arg_out``): the whole gradient goes to the first
           edge of the segment, in the order the edges are given, that attains the minimum.
* ``var``  mean_e(m_e^2) - (mean_e m_e)^2 (``VarAggregation``: two mean reductions; mean divides by max(cnt, 1)); not clamped; an
           empty segment gives 0.  d var / d m_e = 2 (m_e - mean) / cnt.
* ``std``  sqrt(relu(var) + 1e-5) (``StdAggregation``); an empty segment, so every isolated node, gives sqrt(1e-5), not 0.  Where
           var <= 0 the gradient is 0 (relu' (0) = 0); otherwise d std / d m_e = (m_e - mean) / (cnt std).

``reduce_rows`` is that, literally, in the dtype of its input: float64 is the reference of the tests, float32 -- with the target term
inside the message, as the reference's layers have it -- is the reference-shaped evaluation whose own error the device is measured
against.  ``mpnn_conv`` / ``radar_point_gnn_conv`` / ``det_net_basic`` restate the layers and the model around it and reuse
``oracle.gnn_oracle.run_sequential`` and ``batch_norm`` for everything but the reduction.  Everything is differentiable by torch's
autograd with the gradient conventions above (min is written as a gather of the first minimiser, not as ``scatter_reduce('amin')``,
whose autograd spreads the gradient over ties)."""
from typing import Dict

import torch

from oracle import gnn_oracle

STD_EPS = 1e-5
AGGRS = ("min", "var", "std")


def first_argmin(msg: torch.Tensor, index: torch.Tensor, n: int):
    """-> (arg [n, D] int64: the lowest row number of ``msg`` that attains the minimum of its segment, 0 where the segment is empty;
    has [n] bool)."""
    e, d = msg.shape
    idx = index.view(-1, 1).expand(-1, d)
    has = torch.zeros(n, dtype=torch.bool)
    has[index] = True
    with torch.no_grad():
        low = torch.zeros((n, d), dtype=msg.dtype).scatter_reduce(0, idx, msg.detach(), reduce="amin", include_self=False)
        row = torch.arange(e).view(-1, 1).expand(-1, d)
        big = torch.iinfo(torch.int64).max
        cand = torch.where(msg.detach() == low[index], row, torch.full_like(row, big))
        arg = torch.full((n, d), big, dtype=torch.int64).scatter_reduce(0, idx, cand, reduce="amin", include_self=True)
        arg[~has] = 0
    return arg, has


def reduce_rows(msg: torch.Tensor, index: torch.Tensor, n: int, aggr: str) -> torch.Tensor:
    """Rows of ``msg`` [E, D] reduced into [n, D] keyed by ``index`` [E] (int64), in ``msg.dtype``."""
    d = msg.shape[1]
    zeros = torch.zeros((n, d), dtype=msg.dtype)
    if aggr == "min":
        if msg.shape[0] == 0:
            return zeros
        arg, has = first_argmin(msg, index, n)
        return torch.where(has.view(-1, 1), msg.gather(0, arg), zeros)
    if aggr not in ("var", "std"):
        raise ValueError(aggr)
    cnt = torch.bincount(index, minlength=n).clamp(min=1).to(msg.dtype).view(-1, 1)
    mean = zeros.index_add(0, index, msg) / cnt
    mean_2 = zeros.index_add(0, index, msg * msg) / cnt
    var = mean_2 - mean * mean
    if aggr == "var":
        return var
    return torch.sqrt(torch.relu(var) + STD_EPS)


def closed_form_grad(msg: torch.Tensor, index: torch.Tensor, n: int, aggr: str, dM: torch.Tensor) -> torch.Tensor:
    """d loss / d msg [E, D] for loss = sum(dM * reduce_rows(msg)) by the closed forms of the module docstring."""
    d = msg.shape[1]
    g = dM[index]
    if aggr == "min":
        arg, _ = first_argmin(msg, index, n)
        row = torch.arange(msg.shape[0]).view(-1, 1).expand(-1, d)
        return torch.where(arg[index] == row, g, torch.zeros_like(g))
    zeros = torch.zeros((n, d), dtype=msg.dtype)
    cnt = torch.bincount(index, minlength=n).clamp(min=1).to(msg.dtype).view(-1, 1)
    mean = zeros.index_add(0, index, msg) / cnt
    var = zeros.index_add(0, index, msg * msg) / cnt - mean * mean
    if aggr == "var":
        return g * 2 * (msg - mean[index]) / cnt[index]
    std = torch.sqrt(torch.relu(var) + STD_EPS)
    return torch.where(var[index] > 0, g * (msg - mean[index]) / (cnt[index] * std[index]), torch.zeros_like(g))


def _reduce(m, dst, n, aggr):
    return reduce_rows(m, dst, n, aggr) if aggr in AGGRS else gnn_oracle.scatter_reduce_rows(m, dst, n, aggr)


def mpnn_conv(x, edge_index, edge_attr, sd, prefix: str, aggr: str) -> torch.Tensor:
    """``oracle.gnn_oracle.mpnn_conv`` with the reduction of this module."""
    src, dst = edge_index[0], edge_index[1]
    e = edge_attr
    if prefix + "edge_encoder.weight" in sd:
        e = torch.nn.functional.linear(e, sd[prefix + "edge_encoder.weight"].to(x.dtype), sd[prefix + "edge_encoder.bias"].to(x.dtype))
    m = gnn_oracle.run_sequential(torch.cat([x[dst], x[src], e], dim=-1), sd, prefix + "pre_mlp.")
    agg = _reduce(m, dst, x.shape[0], aggr)
    return gnn_oracle.run_sequential(torch.cat([x, agg], dim=-1), sd, prefix + "post_mlp.")


def radar_point_gnn_conv(x, edge_index, edge_attr, sd, prefix: str, aggr: str) -> torch.Tensor:
    src, dst = edge_index[0], edge_index[1]
    m = gnn_oracle.run_sequential(torch.cat([x[src], edge_attr], dim=-1), sd, prefix + "pre_mlp.")
    agg = _reduce(m, dst, x.shape[0], aggr)
    return gnn_oracle.run_sequential(torch.cat([x, agg], dim=-1), sd, prefix + "post_mlp.") + x


def det_net_basic(x, edge_index, edge_attr, sd: Dict[str, torch.Tensor], conv_layer_type: str, aggr: str, training: bool = True,
                  dtype=torch.float64):
    """``oracle.gnn_oracle.det_net_basic`` with the reduction of this module.  Floating-point entries of ``sd`` that require a
    gradient keep their place on the autograd tape (``.to(dtype)`` is differentiable)."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    x, edge_attr = x.to(dtype), edge_attr.to(dtype)
    if any(k.startswith("node_emb_mlp.") for k in sd):
        x = gnn_oracle.run_sequential(x, sd, "node_emb_mlp.", training)
    if any(k.startswith("edge_emb_mlp.") for k in sd):
        edge_attr = gnn_oracle.run_sequential(edge_attr, sd, "edge_emb_mlp.", training)
    n_layers = len({k.split(".")[1] for k in sd if k.startswith("convs.")})
    conv = mpnn_conv if conv_layer_type == "MPNNConv" else radar_point_gnn_conv
    for l in range(n_layers):
        x = conv(x, edge_index, edge_attr, sd, f"convs.{l}.", aggr)
        x = torch.relu(gnn_oracle.batch_norm(x, sd, f"batch_norms.{l}.module.", training, update=False))
    return (gnn_oracle.run_sequential(x, sd, "classification_head.", training),
            gnn_oracle.run_sequential(x, sd, "regression_head.", training))
