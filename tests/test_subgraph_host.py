"""radargnn_amd.subgraph without a device: argument errors are raised before the library is touched, CPU tensors are refused (there is
no CPU path), and the C ABI carries the new entry points.  CPU only."""
import os

import numpy as np
import pytest
import torch

from radargnn_amd import ops, subgraph as SG
from radargnn_amd.data import Batch
from radargnn_amd.frames import FrameBatch


def cpu_batch(n=6, e=4):
    b = Batch(x=torch.zeros((n, 5)), edge_index=torch.zeros((2, e), dtype=torch.int64), edge_attr=torch.zeros((e, 2)))
    b.batch = torch.zeros(n, dtype=torch.int64)
    b.ptr = torch.tensor([0, n])
    return b


@pytest.fixture
def no_library(monkeypatch):
    """Any launch fails the test: the errors below must come first."""
    def refuse(*a, **k):
        raise AssertionError("the library was touched before the argument check")
    for name in ("subgraph_structure", "gather_rows_by_id", "edge_pair_mask", "store_degree_column", "csr_by_target"):
        monkeypatch.setattr(ops, name, refuse)


def test_both_masks_none(no_library):
    with pytest.raises(ValueError, match="keep_nodes"):
        SG.subgraph(cpu_batch())


@pytest.mark.parametrize("kn,ke", [(torch.ones(5, dtype=torch.bool), None), (None, torch.ones(6, dtype=torch.bool)),
                                   (torch.ones((6, 1), dtype=torch.bool), None), (torch.ones(6, dtype=torch.uint8), torch.ones(3, dtype=torch.uint8))])
def test_wrong_lengths(no_library, kn, ke):
    with pytest.raises(ValueError, match="one entry per row"):
        SG.subgraph(cpu_batch(), kn, ke)


def test_masks_must_be_masks(no_library):
    with pytest.raises(TypeError, match="bool or uint8"):
        SG.subgraph(cpu_batch(), torch.ones(6))
    with pytest.raises(TypeError, match="bool or uint8"):
        SG.subgraph(cpu_batch(), np.ones(6, bool))


@pytest.mark.parametrize("p", [-0.1, 1.5, float("nan"), "0.5", None, True])
def test_p_out_of_range(no_library, p):
    with pytest.raises(ValueError, match="probability"):
        SG.RandomNodeDropout(p)
    with pytest.raises(ValueError, match="probability"):
        SG.RandomEdgeDropout(p, pairs=True)


def test_thresholds():
    assert [ops.pair_threshold(p) for p in (0, 0.0, 0.3, 1, 1.0)] == [0, 0, 5033164, 2 ** 24, 2 ** 24]


def test_recompute_needs_the_degree_column(no_library):
    keep = torch.ones(6, dtype=torch.bool)
    with pytest.raises(ValueError, match="node_features"):
        SG.subgraph(cpu_batch(), keep, degree="recompute")
    with pytest.raises(ValueError, match="node_features"):
        SG.subgraph(cpu_batch(), keep, degree="recompute", node_features=["rcs", "velocity_vector"])
    with pytest.raises(ValueError, match="unknown node feature"):
        SG.subgraph(cpu_batch(), keep, degree="recompute", node_features=["rcs", "degrees"])
    with pytest.raises(ValueError, match="keep.*recompute"):
        SG.subgraph(cpu_batch(), keep, degree="drop")
    with pytest.raises(ValueError, match="node_features"):
        SG.RandomNodeDropout(0.1, degree="recompute")
    with pytest.raises(ValueError, match="column 7"):              # x has 5 columns, the list puts the degree in column 7
        SG.subgraph(cpu_batch(), keep, degree="recompute", node_features=["spatial_coordinates", "velocity_vector", "rcs", "velocity_vector", "degree"])
    assert SG._degree_column("recompute", ["rcs", "velocity_vector", "time_index", "degree"]) == 4
    assert SG._degree_column("keep", None) is None


def test_attributes_that_cannot_be_moved(no_library):
    b = cpu_batch()
    b.extra = torch.zeros(3)
    with pytest.raises(ValueError, match="extra"):
        SG.subgraph(b, torch.ones(6, dtype=torch.bool))
    b = cpu_batch()
    b.half = torch.zeros((6, 3), dtype=torch.float16)                # 6-byte rows
    with pytest.raises(NotImplementedError, match="4-byte words"):
        SG.subgraph(b, torch.ones(6, dtype=torch.bool))


def test_cpu_tensors_are_refused(no_library):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SG.subgraph(cpu_batch(), torch.ones(6, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SG.RandomNodeDropout(0.5)(cpu_batch())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SG.RandomEdgeDropout(0.5)(cpu_batch())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SG.RandomEdgeDropout(0.5, pairs=True)(cpu_batch())
    z = torch.zeros((4, 2), dtype=torch.float64)
    fb = FrameBatch(z, z, z[:, 0], z[:, 0], torch.tensor([0, 4]), np.array([4]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SG.drop_points(fb, torch.ones(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="one entry per row"):
        SG.drop_points(fb, torch.ones(5, dtype=torch.bool))


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    ei = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.subgraph_structure(ei, torch.zeros(4, dtype=torch.int64), torch.tensor([0, 4]), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gather_rows_by_id(torch.zeros((4, 2)), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.edge_pair_mask(ei, 4, torch.zeros(1, dtype=torch.int64), 0.5)
    with pytest.raises(ValueError, match="probability"):
        ops.edge_pair_mask(ei, 4, torch.zeros(1, dtype=torch.int64), 2.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.store_degree_column(torch.zeros((4, 2)), torch.zeros(4, dtype=torch.int32), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.keep_mask(torch.ones(4, dtype=torch.bool), 4, "keep")


def test_package_exports_the_module_and_the_abi():
    import radargnn_amd
    from radargnn_amd import _lib
    assert radargnn_amd.subgraph is SG
    names = {"rgnn_subgraph_flags", "rgnn_subgraph_offsets", "rgnn_subgraph_fill", "rgnn_subgraph_gather_rows", "rgnn_edge_pair_mask",
             "rgnn_store_degree_column"}
    assert names <= set(_lib.SIGNATURES) and all(hasattr(_lib.lib, nm) for nm in names)
    header = open(os.path.join(os.path.dirname(radargnn_amd.__path__[0]), "include", "rgnn.h")).read()
    assert "subgraphs (csrc/subgraph.hip)" in header
    for nm in names:
        assert f"int {nm}(" in header, nm
    bits = {"BAD_ENDPOINT": 8192, "CROSS_GRAPH": 16384, "EDGE_ORDER": 32768, "BAD_GRAPH": 65536}
    for nm, value in bits.items():
        assert getattr(ops, f"STATUS_SUBGRAPH_{nm}") == value and f"#define RGNN_STATUS_SUBGRAPH_{nm} {value}" in header
    import subgraph_oracle as S
    assert (S.BAD_ENDPOINT, S.CROSS_GRAPH, S.EDGE_ORDER, S.BAD_GRAPH) == tuple(bits.values())
    from radargnn_amd import build
    assert "subgraph.hip" in build.SOURCES
