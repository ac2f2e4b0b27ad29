"""Parts of a collated batch on the device (csrc/subgraph.hip): node masks, edge masks, node and edge dropout -- what PyG users take
from ``torch_geometric.utils.subgraph`` / ``Batch.subgraph`` / ``dropout_node`` / ``dropout_edge``.

    part = subgraph(batch, keep_nodes=mask)                               # a new Batch: the kept points and the edges between them
    part = subgraph(batch, keep_edges=edge_mask)                          # every node, fewer edges
    part, node_ids, edge_ids = subgraph(batch, mask, return_maps=True)    # ... and where every kept row came from
    fg = subgraph(batch, class_pred != bg_index)                          # the foreground of a prediction, for a second stage
    crop = subgraph(batch, (batch.pos.abs() < 50.0).all(dim=1))           # a region
    loaders["train"] = TransformedLoader(loaders["train"], RandomNodeDropout(0.1))
    loaders["train"] = TransformedLoader(loaders["train"], RandomEdgeDropout(0.2, pairs=True))     # radius / undirected graphs
    frames = drop_points(frame_batch, keep)                               # the same on a FrameBatch, before the graph is built

The order of nodes and edges is preserved, so PyG's numbering holds: ``batch``, ``ptr`` and ``_edge_ptr`` are rebuilt, ``edge_index``
is relabelled, every other tensor attribute moves by its kind as ``GraphStore`` classifies it (E rows and ``edge`` in its name: with
the edges; N rows: with the nodes), and ``to_data_list()`` works on the result.  A graph may come out empty; its offsets then
coincide.  ``y`` rows travel with their points: a box keeps describing the labelled object when some of its points are gone -- the
stance of "boxes move as rigid bodies" (transforms.py); re-creating the targets from the kept points is ``GroundTruthCreator``'s job.

Cost: the kernels size their result on the device, and the host reads 16 bytes (N', E' and the status word) to allocate it.  That
copy is the ONLY host read of ``subgraph`` -- and it synchronises: a ``TransformedLoader`` with a dropout costs one host read per
loader batch, where the rigid motions cost none.  ``drop_points`` reads the new ``frame_ptr`` as well (``frame_sizes`` is a host
array).  Nothing here writes into its input or into the ``GraphStore`` behind it.  There is no CPU path.

The ``degree`` node feature: ``degree="keep"`` (default) leaves the stored column -- the degree in the ORIGINAL graph, which is what a
model trained on whole graphs saw for that point, and costs nothing; ``degree="recompute"`` rewrites it with the undirected degree of
the kept graph (rgnn_undirected_degree's number, ``Graph.get_degree``), which is what building the graph from the kept points'
edge list would store, at the price of a CSR build and three more launches.  Take ``recompute`` when the part is handed on as a graph
in its own right, ``keep`` for light dropout used as noise.
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from .data import Batch
from .frames import FrameBatch

_STATUS_TEXT = ((ops.STATUS_SUBGRAPH_BAD_ENDPOINT, "an edge with an end outside [0, N)"),
                (ops.STATUS_SUBGRAPH_BAD_GRAPH, "a graph id outside [0, B) in `batch`, or an offset outside [0, N] in `ptr`"),
                (ops.STATUS_SUBGRAPH_CROSS_GRAPH, "an edge whose ends lie in two graphs"),
                (ops.STATUS_SUBGRAPH_EDGE_ORDER, "an edge list that is not grouped by graph in ascending order"))


def _check_mask(mask, count: int, name: str):
    """shape and dtype first (host facts), the device afterwards: argument errors come before anything touches the library"""
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"`{name}` must be a bool or uint8 tensor")
    if mask.shape != (count,):
        raise ValueError(f"`{name}` must hold one entry per row: [{count}], got {tuple(mask.shape)}")
    return mask


def _check_probability(p) -> float:
    ops.pair_threshold(p)
    return float(p)


def _degree_column(degree: str, node_features: Optional[Sequence[str]]) -> Optional[int]:
    if degree not in ("keep", "recompute"):
        raise ValueError(f"degree must be 'keep' or 'recompute', got {degree!r}")
    if degree == "keep":
        return None
    names = list(node_features) if node_features is not None else []
    unknown = [nm for nm in names if nm not in ops.NODE_FEATURE_WIDTH]
    if unknown:
        raise ValueError(f"unknown node feature(s) {unknown}; known: {sorted(ops.NODE_FEATURE_WIDTH)}")
    if "degree" not in names:
        raise ValueError("degree='recompute' needs `node_features`, the list x was built with, and 'degree' in it")
    return sum(ops.NODE_FEATURE_WIDTH[nm] for nm in names[:names.index("degree")])


def _raise_status(bits: int) -> None:
    found = [text for bit, text in _STATUS_TEXT if bits & bit]
    if found:
        raise ValueError("subgraph: the batch holds " + "; ".join(found) + " (such edges are dropped; check=False returns the rest)")


def subgraph(batch: Batch, keep_nodes: Optional[torch.Tensor] = None, keep_edges: Optional[torch.Tensor] = None, *,
             node_features: Optional[Sequence[str]] = None, degree: str = "keep", return_maps: bool = False, check: bool = True):
    """-> a new ``Batch``: the nodes with ``keep_nodes[i]`` and the edges with ``keep_edges[e]`` whose two ends are kept (a mask that
    is None keeps everything; both None is an error).  Masks: bool / uint8 tensors [N] / [E] on the batch's device.

    ``return_maps``: -> (batch, node_ids int64 [N'], edge_ids int64 [E']), the original positions of the kept rows.
    ``degree`` / ``node_features``: see the module text.  ``check``: a batch whose edges are unsound (an end outside [0, N), ends in
    two graphs, edges not grouped by graph) raises ``ValueError``; with ``check=False`` those edges are dropped, the rest is
    returned and the bits are left in the result's ``_status`` (ops.STATUS_SUBGRAPH_*).  Either way no such value is used as an index.

    One host read of 16 bytes (it synchronises); 5 - 7 launches for the structure, one per moved attribute."""
    if keep_nodes is None and keep_edges is None:
        raise ValueError("subgraph: give keep_nodes, keep_edges or both (both None keeps the whole batch)")
    column = _degree_column(degree, node_features)
    for name in ("batch", "ptr", "edge_index"):
        if not isinstance(getattr(batch, name, None), torch.Tensor):
            raise ValueError(f"subgraph: the batch carries no `{name}`")
    bvec, ptr, edge_index = batch.batch, batch.ptr, batch.edge_index
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or bvec.dim() != 1 or ptr.dim() != 1 or ptr.numel() < 1:
        raise ValueError("subgraph: edge_index must be [2, E], batch [N] and ptr [B + 1]")
    n, e = bvec.numel(), edge_index.shape[1]
    _check_mask(keep_nodes, n, "keep_nodes"), _check_mask(keep_edges, e, "keep_edges")
    moves = []
    for k in batch.keys:
        v = getattr(batch, k)
        if k in ("batch", "ptr", "edge_index") or not torch.is_tensor(v):
            continue
        rows = v.shape[0] if v.dim() else -1
        if "edge" in k and rows == e:
            moves.append((k, "edge"))
        elif rows == n:
            moves.append((k, "node"))
        else:
            raise ValueError(f"subgraph: `{k}` has {rows} rows, neither the batch's {n} nodes nor (with `edge` in its name) its "
                             f"{e} edges: it cannot be moved")
        ops._words_per_row(v)                                   # raises for dtypes the gather cannot move
    if column is not None:
        x = getattr(batch, "x", None)
        if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] <= column:
            raise ValueError(f"degree='recompute': x must be float32 [N, D] with the degree in column {column}")
    # ---- the device from here on
    for t, name in ((bvec, "batch"), (ptr, "ptr"), (edge_index, "edge_index")):
        ops._dev(t, name, torch.int64)
    kn, ke = ops.keep_mask(keep_nodes, n, "keep_nodes"), ops.keep_mask(keep_edges, e, "keep_edges")
    st = ops.subgraph_structure(edge_index, bvec, ptr, n, kn, ke)
    if check:
        _raise_status(st["status"])
    out = Batch()
    for k in batch.keys:
        v = getattr(batch, k)
        if k == "edge_index":
            val = st["edge_index"]
        elif k == "batch":
            val = st["batch"]
        elif k == "ptr":
            val = st["ptr"]
        elif (k, "edge") in moves:
            val = ops.gather_rows_by_id(v, st["edge_ids"])
        elif (k, "node") in moves:
            val = ops.gather_rows_by_id(v, st["node_ids"])
        else:
            val = v
        setattr(out, k, val)
    object.__setattr__(out, "_edge_ptr", st["edge_ptr"])
    object.__setattr__(out, "_status", st["status"])
    if column is not None and st["node_ids"].numel():
        n_out = st["node_ids"].numel()
        if st["edge_ids"].numel():
            rowptr_t, src_sorted, _ = ops.csr_by_target(st["edge_index"], n_out)
            deg = ops.undirected_degree(rowptr_t, src_sorted, n_out)      # |in U out| does not change under transposition
        else:
            deg = torch.zeros(n_out, dtype=torch.int32, device=bvec.device)
        ops.store_degree_column(out.x, deg, column)                      # out.x is this call's own gather result
    return (out, st["node_ids"], st["edge_ids"]) if return_maps else out


class RandomNodeDropout:
    """``Batch -> Batch`` for ``TransformedLoader``: every point is dropped with probability ``p``, independently
    (``torch.rand(N) >= p`` on the batch's device, from ``generator``: a generator OF that device), with the edges at it.
    ``p = 0`` returns the input's values, ``p = 1`` empty graphs.  ``degree`` / ``node_features``: as for ``subgraph``.  One host
    read per call (``subgraph``)."""

    def __init__(self, p: float, generator: Optional[torch.Generator] = None, degree: str = "keep",
                 node_features: Optional[Sequence[str]] = None):
        self.p, self.generator, self.degree = _check_probability(p), generator, degree
        self.node_features = None if node_features is None else list(node_features)
        _degree_column(degree, self.node_features)

    def __call__(self, batch: Batch) -> Batch:
        bvec = ops._dev(batch.batch, "batch", torch.int64)
        keep = torch.rand(bvec.numel(), device=bvec.device, generator=self.generator) >= self.p
        return subgraph(batch, keep_nodes=keep, degree=self.degree, node_features=self.node_features)


class RandomEdgeDropout:
    """``Batch -> Batch`` for ``TransformedLoader`` (DropEdge): every edge is dropped with probability ``p``; all nodes stay.
    ``pairs=False``: independently per directed edge (``torch.rand(E) >= p``).  ``pairs=True``: per UNORDERED pair, so that (s, t)
    and (t, s) fall together -- for radius graphs and ``edge_mode="undirected"``: a seed is drawn with ``torch.randint`` on the
    device (never read back) and hashed with the pair (``ops.edge_pair_mask``).  ``generator``: a generator of the batch's device.
    One host read per call (``subgraph``)."""

    def __init__(self, p: float, generator: Optional[torch.Generator] = None, pairs: bool = False):
        self.p, self.generator, self.pairs = _check_probability(p), generator, bool(pairs)

    def __call__(self, batch: Batch) -> Batch:
        edge_index = ops._dev(batch.edge_index, "edge_index", torch.int64)
        dev = edge_index.device
        if self.pairs:
            seed = torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64, device=dev, generator=self.generator)
            keep = ops.edge_pair_mask(edge_index, batch.batch.numel(), seed, self.p)
        else:
            keep = torch.rand(edge_index.shape[1], device=dev, generator=self.generator) >= self.p
        return subgraph(batch, keep_edges=keep)


def drop_points(frame_batch: FrameBatch, keep: torch.Tensor) -> FrameBatch:
    """-> a new ``FrameBatch`` with the points whose ``keep`` (bool / uint8 [N], on the device) is set: ``X``, ``V``, ``rcs`` and
    ``timestamp`` gathered by the node kernels of ``subgraph``, ``frame_ptr`` rebuilt; a frame may come out empty.  Two host reads:
    the 16 bytes that size the result and the new ``frame_ptr`` (``frame_sizes`` is a host array).  For the ``HotPath`` pipeline:
    drop before the graph is built, and degree, edges and features are those of the kept cloud."""
    n = frame_batch.X.shape[0]
    _check_mask(keep, n, "keep")
    if keep is None:
        raise ValueError("drop_points: `keep` is required")
    fields = {name: getattr(frame_batch, name) for name in ("X", "V", "rcs", "timestamp")}
    for name, t in fields.items():
        if not isinstance(t, torch.Tensor) or t.dim() < 1 or t.shape[0] != n:
            raise ValueError(f"drop_points: `{name}` must hold one row per point")
    if frame_batch.frame_ptr.dim() != 1 or frame_batch.frame_ptr.numel() != frame_batch.num_frames + 1:
        raise ValueError("drop_points: frame_ptr must hold B + 1 offsets")
    frame_ptr = ops._dev(frame_batch.frame_ptr, "frame_ptr", torch.int64)
    for name, t in fields.items():
        ops._dev(t, name, torch.float64)
    st = ops.subgraph_structure(None, None, frame_ptr, n, ops.keep_mask(keep, n, "keep"), None)
    _raise_status(st["status"])
    moved = {name: ops.gather_rows_by_id(t, st["node_ids"]) for name, t in fields.items()}
    sizes = np.diff(st["ptr"].cpu().numpy())
    return dataclasses.replace(frame_batch, frame_ptr=st["ptr"], frame_sizes=sizes, **moved)
