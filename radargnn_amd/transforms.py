"""Rigid motions of frames and collated graphs on the device (csrc/transform.hip): per frame f, ``p' = R(a_f) p + t_f`` for points
and ``v' = R(a_f) v`` for velocities and differences, ``R = [[c, -s], [s, c]]``, ``a_f`` in radians, counter-clockwise.

    motion = RigidMotion.random(batch.num_graphs, max_angle=math.pi, max_shift=5.0)
    moved = transform_graphs(batch, motion, node_features, edge_features, edge_mode, aligned, bb_invariance)   # a new Batch
    frames = transform_frames(frame_batch, motion)                                                           # a new FrameBatch
    loaders["train"] = TransformedLoader(loaders["train"], RandomRigidMotion(graph_config, aligned, bb_invariance, math.pi, 5.0))

What moves in a graph: ``pos`` (point), ``vel`` (rotated), the ``spatial_coordinates`` (point) and ``velocity_vector`` (rotated)
columns of ``x``, the ``relative_position`` / ``relative_velocity`` columns of ``edge_attr`` (rotated; undirected: ``|R (q_i - q_j)|``
from the batch's own ``pos`` / ``vel``), and of a rotated box ``[c0, c1, l, w, theta]`` in ``y`` the centre (``none``: point,
``translation``: the offset rotated) and ``theta' = theta + a`` folded into [0, pi).  The ``en`` encoding, aligned boxes (relative to
their point: a shift does not move them, a rotation is refused), the label, lengths, widths and every other feature stay.

Boxes move as RIGID BODIES: the 0.5 x 0.5 square of a one-point object turns with the scene, where re-creating the targets from
the moved points (``GroundTruthCreator``) would put it back at theta = 0.  The two agree for objects of three and more points.

Nothing here reads the device back, writes into its input or into the ``GraphStore`` behind it: every call returns new containers
whose untouched tensors are the input's own.  Float64 arithmetic, one rounding at the store; a frame whose angle is exactly 0 keeps
every rotated quantity bit for bit, and the identity motion returns the input bits.  There is no CPU path.
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Sequence

import torch

from . import ops
from .data import Batch
from .frames import FrameBatch
from .ops import _dev, _ld, _ptr, _rowmajor, _stream, check, lib
from .postprocessor import INVARIANCE_CODES

_MOVING_EDGE_FEATURES = ("relative_position", "relative_velocity")


class RigidMotion:
    """One motion per frame (graph): ``angle`` float64 [B] in radians, ``shift`` float64 [B, 2], held on ``device``.

    ``rotates`` is a HOST flag fixed here and never read back from the device: host values (sequences, numpy arrays, CPU tensors)
    are looked at before they are uploaded; for tensors that already live on the device the caller states it (default True, the
    safe side: ``rotates`` only ever refuses aligned boxes and decides which tensors are shared)."""

    def __init__(self, angle, shift, device="cuda", rotates: Optional[bool] = None):
        on_device = [isinstance(t, torch.Tensor) and t.device.type != "cpu" for t in (angle, shift)]
        if rotates is None:
            rotates = True if on_device[0] else bool((torch.as_tensor(angle, dtype=torch.float64) != 0.0).any())
        as_f64 = lambda t, dev: torch.as_tensor(t, dtype=torch.float64).to(dev)
        self.angle = as_f64(angle, angle.device if on_device[0] else device).reshape(-1).contiguous()
        self.shift = as_f64(shift, shift.device if on_device[1] else device).contiguous()
        if self.shift.dim() != 2 or self.shift.shape != (self.angle.numel(), 2):
            raise ValueError(f"angle must be [B] and shift [B, 2] (got {tuple(self.angle.shape)} and {tuple(self.shift.shape)})")
        if self.angle.device != self.shift.device:
            raise ValueError("angle and shift must live on one device")
        self.rotates = bool(rotates)

    def __len__(self) -> int:
        return self.angle.numel()

    @staticmethod
    def identity(num_frames: int, device="cuda") -> "RigidMotion":
        return RigidMotion(torch.zeros(num_frames, dtype=torch.float64, device=device),
                           torch.zeros((num_frames, 2), dtype=torch.float64, device=device), device=device, rotates=False)

    @staticmethod
    def random(num_frames: int, max_angle: float, max_shift: float, generator: Optional[torch.Generator] = None,
               device="cuda") -> "RigidMotion":
        """Angles uniform in [-max_angle, max_angle), shift components uniform in [-max_shift, max_shift): two ``torch.rand`` draws
        on the device (``generator``: a generator OF that device), no host read.  ``max_angle == 0`` gives exact zeros and
        ``rotates = False``."""
        if max_angle < 0 or max_shift < 0:
            raise ValueError("max_angle and max_shift must not be negative")
        draw = lambda *shape: torch.rand(*shape, dtype=torch.float64, device=device, generator=generator)
        if max_angle == 0:
            angle = torch.zeros(num_frames, dtype=torch.float64, device=device)
        else:
            angle = (draw(num_frames) * 2.0 - 1.0) * float(max_angle)
        shift = (draw(num_frames, 2) * 2.0 - 1.0) * float(max_shift)
        return RigidMotion(angle, shift, device=device, rotates=max_angle != 0)


def _feature_codes(names: Sequence[str], table: dict, what: str):
    names = list(names)
    unknown = [nm for nm in names if nm not in table]
    if unknown:
        raise ValueError(f"unknown {what} feature(s) {unknown}; known: {sorted(table)}")
    return ops._codes(names, table, what)


def _check_motion(motion: RigidMotion, count: int, what: str) -> None:
    if not isinstance(motion, RigidMotion):
        raise TypeError("motion must be a RigidMotion")
    if len(motion) != count:
        raise ValueError(f"the motion holds {len(motion)} frames, the batch {count} {what}")


def transform_frames(batch: FrameBatch, motion: RigidMotion) -> FrameBatch:
    """-> a new ``FrameBatch`` with moved ``X`` and ``V`` (rgnn_rigid_points, one launch); ``rcs``, ``timestamp``, ``frame_ptr`` and
    ``frame_sizes`` are the input's own."""
    _check_motion(motion, batch.num_frames, "frames")
    X = _dev(batch.X, "X", torch.float64)[:, :2].contiguous()
    V = _dev(batch.V, "V", torch.float64)[:, :2].contiguous()
    frame_ptr = _dev(batch.frame_ptr, "frame_ptr", torch.int64).contiguous()
    _dev(motion.angle, "motion.angle"); _dev(motion.shift, "motion.shift")
    if frame_ptr.numel() != batch.num_frames + 1 or V.shape != X.shape:
        raise ValueError("frame_ptr must hold B + 1 offsets and V the rows of X")
    X_out, V_out = torch.empty_like(X), torch.empty_like(V)
    check(lib.rgnn_rigid_points(_ptr(X), _ptr(V), _ptr(frame_ptr), X.shape[0], batch.num_frames, _ptr(motion.angle),
                                _ptr(motion.shift), _ptr(X_out), _ptr(V_out), _stream()))
    return dataclasses.replace(batch, X=X_out, V=V_out)


def _check_plan(node_features, edge_features, edge_mode, aligned, bb_invariance, rotates: bool):
    arr_n, n_n = _feature_codes(node_features, ops.NODE_FEATURE_CODES, "node")
    arr_e, n_e = _feature_codes(edge_features, ops.EDGE_FEATURE_CODES, "edge")
    if edge_mode not in ("directed", "undirected"):
        raise ValueError(f"unknown edge_mode {edge_mode!r}")
    if bb_invariance not in INVARIANCE_CODES:
        raise ValueError(f"unknown bb_invariance {bb_invariance!r}; known: {sorted(INVARIANCE_CODES)}")
    if aligned and rotates:
        raise ValueError("aligned boxes cannot be rotated: use a motion with max_angle = 0 (shifts leave them as they are)")
    return (arr_n, n_n), (arr_e, n_e)


def transform_graphs(batch: Batch, motion: RigidMotion, node_features: Sequence[str], edge_features: Sequence[str],
                     edge_mode: str, aligned: bool, bb_invariance: str) -> Batch:
    """-> a new ``Batch``: graph g of ``batch`` moved by ``motion[g]`` (rgnn_rigid_graph_nodes + rgnn_rigid_graph_edges, one launch
    each, behind one device copy per tensor that changes).  ``node_features`` / ``edge_features``: the lists ``x`` and
    ``edge_attr`` were built with, in their order; ``aligned`` / ``bb_invariance``: the encoding of the box columns of ``y``.
    Tensors in which nothing moves are shared with ``batch``; ``batch`` itself is never written."""
    (arr_n, n_n), (arr_e, n_e) = _check_plan(node_features, edge_features, edge_mode, aligned, bb_invariance, motion.rotates
                                            if isinstance(motion, RigidMotion) else False)
    _check_motion(motion, batch.num_graphs, "graphs")
    node_features, edge_features = list(node_features), list(edge_features)
    rotates, undirected = motion.rotates, edge_mode == "undirected"
    inv = INVARIANCE_CODES[bb_invariance]
    _dev(motion.angle, "motion.angle"); _dev(motion.shift, "motion.shift")
    bvec = _dev(batch.batch, "batch", torch.int64).contiguous()
    n, b = bvec.numel(), batch.num_graphs

    def rows2(t, name):
        if t is None:
            return None
        t = _dev(t, name, torch.float32)
        if t.dim() != 2 or t.shape != (n, 2):
            raise ValueError(f"{name} must be float32 [N, 2]")
        return t.contiguous()

    pos, vel = rows2(getattr(batch, "pos", None), "pos"), rows2(getattr(batch, "vel", None), "vel")
    x, y, edge_attr = batch.x, batch.y, batch.edge_attr

    x_moves = x is not None and ("spatial_coordinates" in node_features or (rotates and "velocity_vector" in node_features))
    y_moves = y is not None and not aligned and (inv == 0 or (inv == 1 and rotates))
    e_moves = edge_attr is not None and rotates and any(nm in edge_features for nm in _MOVING_EDGE_FEATURES)
    x_in = x_out = y_in = y_out = None
    if x_moves:
        x_in = _rowmajor(_dev(x, "x", torch.float32), "x")
        if x_in.shape[0] != n or x_in.shape[1] < sum(ops.NODE_FEATURE_WIDTH[nm] for nm in node_features):
            raise ValueError(f"x {tuple(x_in.shape)} does not hold the columns of {node_features} for {n} nodes")
        x_out = x_in.clone(memory_format=torch.contiguous_format)
    box_width = 4 if aligned else 5
    if y is not None and (y.dim() != 2 or y.shape[1] != 1 + box_width):
        raise ValueError(f"y must be [N, 1 + {box_width}] (label | {'aligned' if aligned else 'rotated'} box), got {tuple(y.shape)}")
    if y_moves:
        y_in = _rowmajor(_dev(y, "y", torch.float32), "y")
        if y_in.shape[0] != n:
            raise ValueError("y must hold one row per node")
        y_out = y_in.clone(memory_format=torch.contiguous_format)
    pos_out = None if pos is None else torch.empty_like(pos)
    vel_out = None if vel is None or not rotates else torch.empty_like(vel)
    if n and (pos_out is not None or vel_out is not None or x_out is not None or y_out is not None):
        check(lib.rgnn_rigid_graph_nodes(
            _ptr(pos), _ptr(vel if vel_out is not None else None), _ptr(x_in), _ld(x_in) if x_in is not None else 0, arr_n, n_n,
            _ptr(y_in), _ld(y_in) if y_in is not None else 0, box_width, inv, _ptr(bvec), n, b, _ptr(motion.angle), _ptr(motion.shift),
            _ptr(pos_out), _ptr(vel_out), _ptr(x_out), x_out.shape[1] if x_out is not None else 0, _ptr(y_out),
            y_out.shape[1] if y_out is not None else 0, _stream()))

    e_out = None
    if e_moves:
        edge_index = _dev(batch.edge_index, "edge_index", torch.int64).contiguous()
        e_in = _rowmajor(_dev(edge_attr, "edge_attr", torch.float32), "edge_attr")
        n_edges = edge_index.shape[1]
        if e_in.shape[0] != n_edges or e_in.shape[1] < sum(ops.EDGE_FEATURE_WIDTH[nm] for nm in edge_features):
            raise ValueError(f"edge_attr {tuple(e_in.shape)} does not hold the columns of {edge_features} for {n_edges} edges")
        if undirected and (("relative_position" in edge_features and pos is None) or ("relative_velocity" in edge_features and vel is None)):
            raise ValueError("undirected relative features are recomputed from the batch's pos / vel, which it does not carry")
        e_out = e_in.clone(memory_format=torch.contiguous_format)
        if n_edges:
            check(lib.rgnn_rigid_graph_edges(_ptr(e_in), _ld(e_in), arr_e, n_e, 1 if undirected else 0, _ptr(edge_index), n_edges,
                                             _ptr(bvec), n, b, _ptr(motion.angle), _ptr(pos), _ptr(vel), _ptr(e_out), e_out.shape[1],
                                             _stream()))

    out = Batch()
    new = {"pos": pos_out, "vel": vel_out, "x": x_out, "y": y_out, "edge_attr": e_out}
    for k in batch.keys:
        setattr(out, k, new[k] if new.get(k) is not None else getattr(batch, k))
    if getattr(batch, "_edge_ptr", None) is not None:
        object.__setattr__(out, "_edge_ptr", batch._edge_ptr)
    return out


class RandomRigidMotion:
    """``Batch -> Batch``: every call draws a fresh ``RigidMotion.random`` for the batch's graphs (on the batch's device, from
    ``generator``) and applies it.  ``graph_config``: anything with ``node_features``, ``edge_features`` and ``edge_mode``
    (``frames.GraphSettings``, ``graph_constructor.GraphConstructionConfiguration``)."""

    def __init__(self, graph_config, aligned: bool, bb_invariance: str, max_angle: float, max_shift: float,
                 generator: Optional[torch.Generator] = None):
        self.node_features, self.edge_features = list(graph_config.node_features), list(graph_config.edge_features)
        self.edge_mode = graph_config.edge_mode
        self.aligned, self.bb_invariance = bool(aligned), bb_invariance
        self.max_angle, self.max_shift, self.generator = float(max_angle), float(max_shift), generator
        if self.max_angle < 0 or self.max_shift < 0:
            raise ValueError("max_angle and max_shift must not be negative")
        _check_plan(self.node_features, self.edge_features, self.edge_mode, self.aligned, bb_invariance, self.max_angle != 0)

    def __call__(self, batch: Batch) -> Batch:
        motion = RigidMotion.random(batch.num_graphs, self.max_angle, self.max_shift, self.generator, device=batch.batch.device)
        return transform_graphs(batch, motion, self.node_features, self.edge_features, self.edge_mode, self.aligned, self.bb_invariance)


class TransformedLoader:
    """A loader whose batches pass through ``transform`` (a callable ``Batch -> Batch``) as they are drawn: what ``Trainer.fit`` and
    ``Predictor`` take in place of the loader itself.  The transform runs once per loader batch, before anything the trainer does
    to it (``adapt_orientation_angle`` included)."""

    def __init__(self, loader, transform):
        self.loader, self.transform = loader, transform

    def __iter__(self):
        for batch in self.loader:
            yield self.transform(batch)

    def __len__(self) -> int:
        return len(self.loader)
