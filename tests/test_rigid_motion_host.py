"""CPU-only checks of radargnn_amd.transforms: the argument errors (raised before anything touches a device), the host-side
``rotates`` flag, the loader wrapper, and the oracle's own rigid-body property -- the corners decoded from a moved box must be
``R corners + t`` of the corners decoded from the original.  The oracle (tests/rigid_motion_oracle.py) is pure float64 there, so
the bar is its arithmetic noise with margin: 1e-12 absolute on coordinates of magnitude up to 100 (a few hundred eps64 * 100)."""
import math

import numpy as np
import pytest
import torch

import rigid_motion_oracle as O
from radargnn_amd import transforms as T
from radargnn_amd.data import Batch

NODES = ["rcs", "spatial_coordinates", "velocity_vector"]
EDGES = ["relative_position"]


def cpu_batch(sizes=(3, 2)):
    n = sum(sizes)
    b = Batch(x=torch.zeros(n, 5), edge_index=torch.zeros(2, 0, dtype=torch.long), edge_attr=torch.zeros(0, 2), y=torch.zeros(n, 6),
              pos=torch.zeros(n, 2))
    b.batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    b.ptr = torch.tensor(np.concatenate(([0], np.cumsum(sizes))))
    return b


def motion(angles, device="cpu"):
    return T.RigidMotion(angles, np.zeros((len(angles), 2)), device=device)


# ---------------------------------------------------------------------------------------------- rotates
def test_rotates_is_fixed_from_host_values():
    assert motion([0.0, 0.0]).rotates is False
    assert motion([0.0, -0.0]).rotates is False
    assert motion([0.0, 1e-300]).rotates is True
    assert motion(np.array([math.pi])).rotates is True
    assert motion(torch.tensor([0.0, 0.0])).rotates is False
    assert T.RigidMotion([0.0], [[1.0, 2.0]], device="cpu", rotates=True).rotates is True      # the caller's word wins
    m = T.RigidMotion.identity(4, device="cpu")
    assert m.rotates is False and len(m) == 4 and not m.angle.any() and not m.shift.any()
    assert m.angle.dtype == torch.float64 and m.shift.shape == (4, 2) and m.shift.dtype == torch.float64


def test_random_motion_bookkeeping():
    g = torch.Generator().manual_seed(3)
    m = T.RigidMotion.random(5, 0.0, 2.0, generator=g, device="cpu")
    assert m.rotates is False and not m.angle.any() and bool((m.shift.abs() <= 2.0).all()) and bool(m.shift.any())
    m = T.RigidMotion.random(5, 0.5, 0.0, generator=g, device="cpu")
    assert m.rotates is True and bool((m.angle.abs() <= 0.5).all()) and bool(m.angle.any()) and not m.shift.any()
    a = T.RigidMotion.random(7, 1.0, 1.0, generator=torch.Generator().manual_seed(9), device="cpu")
    b = T.RigidMotion.random(7, 1.0, 1.0, generator=torch.Generator().manual_seed(9), device="cpu")
    assert torch.equal(a.angle, b.angle) and torch.equal(a.shift, b.shift)
    assert len(T.RigidMotion.random(0, 1.0, 1.0, device="cpu")) == 0
    with pytest.raises(ValueError):
        T.RigidMotion.random(2, -1.0, 0.0, device="cpu")


def test_motion_shapes_are_checked():
    with pytest.raises(ValueError):
        T.RigidMotion([0.0, 1.0], [[0.0, 0.0]], device="cpu")
    with pytest.raises(ValueError):
        T.RigidMotion([0.0], [0.0, 0.0, 0.0], device="cpu")


# ---------------------------------------------------------------------------------------------- argument errors
def test_transform_graphs_argument_errors():
    b = cpu_batch()
    ok = motion([0.1, 0.2])
    with pytest.raises(ValueError, match="node feature"):
        T.transform_graphs(b, ok, ["rcs", "spatial_coordinate"], EDGES, "directed", False, "none")
    with pytest.raises(ValueError, match="edge feature"):
        T.transform_graphs(b, ok, NODES, ["relative_positions"], "directed", False, "none")
    with pytest.raises(ValueError, match="bb_invariance"):
        T.transform_graphs(b, ok, NODES, EDGES, "directed", False, "rotation")
    with pytest.raises(ValueError, match="edge_mode"):
        T.transform_graphs(b, ok, NODES, EDGES, "both", False, "none")
    with pytest.raises(ValueError, match="aligned"):
        T.transform_graphs(b, ok, NODES, EDGES, "directed", True, "none")
    with pytest.raises(ValueError, match="3 frames"):
        T.transform_graphs(b, motion([0.1, 0.2, 0.3]), NODES, EDGES, "directed", False, "none")
    with pytest.raises(ValueError, match="1 frames"):
        T.transform_graphs(b, motion([0.0]), NODES, EDGES, "directed", True, "none")
    with pytest.raises(TypeError):
        T.transform_graphs(b, (0.1, 0.2), NODES, EDGES, "directed", False, "none")
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # everything valid, but the tensors are on the host
        T.transform_graphs(b, ok, NODES, EDGES, "directed", False, "none")


def test_random_rigid_motion_checks_its_plan_when_it_is_made():
    from radargnn_amd.frames import GraphSettings
    cfg = GraphSettings(node_features=NODES, edge_features=EDGES)
    with pytest.raises(ValueError, match="aligned"):
        T.RandomRigidMotion(cfg, True, "none", 0.1, 1.0)
    with pytest.raises(ValueError, match="bb_invariance"):
        T.RandomRigidMotion(cfg, False, "e2", 0.1, 1.0)
    with pytest.raises(ValueError, match="node feature"):
        T.RandomRigidMotion(GraphSettings(node_features=["x"], edge_features=EDGES), False, "none", 0.1, 1.0)
    with pytest.raises(ValueError):
        T.RandomRigidMotion(cfg, False, "none", 0.1, -1.0)
    t = T.RandomRigidMotion(cfg, True, "none", 0.0, 1.0)                # aligned boxes and a pure shift: accepted
    assert t.max_angle == 0.0 and t.edge_mode == "directed"


def test_transformed_loader_applies_the_transform_per_batch():
    seen = []
    loader = T.TransformedLoader([1, 2, 3], lambda b: seen.append(b) or 10 * b)
    assert len(loader) == 3 and list(loader) == [10, 20, 30] and seen == [1, 2, 3]
    assert list(loader) == [10, 20, 30] and len(seen) == 6              # every pass draws again


# ---------------------------------------------------------------------------------------------- the oracle's rigid-body property
def same_rectangles(got, want):
    """max |got - want| over corners, per row, where theta' folded by pi lists the SAME rectangle from the opposite corner"""
    d0 = np.abs(got - want).max(axis=(1, 2))
    d2 = np.abs(got - np.roll(want, 2, axis=1)).max(axis=(1, 2))
    return np.minimum(d0, d2)


@pytest.mark.parametrize("inv", ["none", "translation"])
def test_oracle_moves_boxes_as_rigid_bodies(inv):
    rng = np.random.default_rng(11)
    sizes = [40, 1, 0, 59]
    n, batch = sum(sizes), np.repeat(np.arange(4), sizes)
    angle = np.array([0.0, math.pi, 1e-9, 2.1])
    shift = np.array([[3.0, -4.0], [0.0, 0.0], [20.0, 20.0], [-12.5, 0.0]])
    pos = rng.uniform(-40, 40, size=(n, 2))
    centre = pos + rng.normal(0, 2, size=(n, 2))
    y = np.concatenate((rng.integers(0, 5, size=(n, 1)).astype(np.float64), centre if inv == "none" else centre - pos,
                        rng.uniform(0.5, 10, size=(n, 2)), rng.uniform(0, np.pi, size=(n, 1))), axis=1)
    y[::7, 5] = 0.0
    y[3, 5], y[4, 5] = np.nextafter(O.PI, 0.0), np.pi / 2
    y[rng.uniform(size=n) < 0.3, 1:] = np.nan
    out = O.graph_nodes(pos, None, None, y, batch, angle, shift, [], False, inv, dtype=np.float64)
    box = ~np.isnan(y[:, 1])
    assert np.array_equal(np.isnan(out["y"]), np.isnan(y)) and np.array_equal(out["y"][:, [0, 3, 4]], y[:, [0, 3, 4]], equal_nan=True)
    assert bool((out["y"][box, 5] >= 0).all()) and bool((out["y"][box, 5] < np.pi).all())
    assert np.array_equal(out["y"][batch == 0, 5], y[batch == 0, 5], equal_nan=True)          # angle 0: theta keeps its bits
    want = O.move_corners(O.box_corners(y[box, 1:], pos[box], inv), angle[batch][box], shift[batch][box])
    got = O.box_corners(out["y"][box, 1:], out["pos"][box], inv)
    assert np.abs(want).max() <= 100.0
    err = same_rectangles(got, want)
    print(f"[rigid oracle] {inv}: {int(box.sum())} boxes, worst corner error {err.max():.2e} (bar 1e-12)")
    assert err.max() <= 1e-12
