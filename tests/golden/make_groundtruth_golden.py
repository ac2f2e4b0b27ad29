"""Writes tests/golden/groundtruth_*.npz: inputs and outputs of the reference's GroundTruthCreator.create_2D_bounding_boxes
(preprocessor/radarscenes/dataset_creation.py:232-521), produced by EXECUTING the reference's own class, loaded from
/root/reference by file path; nothing of it is restated here.  dataset_creation.py imports once the packages that are absent
(ray, torch_geometric, radar_scenes, matplotlib) and the reference modules out of scope are stubbed with MagicMock;
utils/math.py and preprocessor/bounding_box.py are loaded for real.  Runs only on the build machine; the fixtures are committed.

Stored per fixture: pos (float64 values that float32 holds), object_id, frame_ptr; the reference's four output matrices
(boxes_aligned, boxes_none, boxes_translation, boxes_en); per object ((frame, id) order, as tests/groundtruth_oracle.objects
lists them) the absolute rectangle from the reference's own minimum-rectangle and BoundingBox code, and the admissibility margins
(groundtruth_oracle.admissibility).  The clouds are re-seeded until every margin holds, so the tests leave out nothing.
"""
import importlib.util
import os
import sys
import types
from types import SimpleNamespace
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import groundtruth_oracle as O  # noqa: E402

R = "/root/reference/src/gnnradarobjectdetection"
P = "gnnradarobjectdetection"
for name in (P, P + ".utils", P + ".preprocessor", P + ".preprocessor.radarscenes", P + ".graph_constructor"):
    m = types.ModuleType(name); m.__path__ = []; sys.modules[name] = m
for name in ("ray", "torch_geometric", "torch_geometric.data", "radar_scenes", "radar_scenes.sequence", "matplotlib",
             "matplotlib.pyplot", P + ".preprocessor.configs", P + ".preprocessor.radar_point_cloud",
             P + ".preprocessor.radarscenes.configs", P + ".preprocessor.radarscenes.scene_collection",
             P + ".graph_constructor.graph"):
    sys.modules[name] = MagicMock()


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    return mod


M = load(P + ".utils.math", R + "/utils/math.py")
B = load(P + ".preprocessor.bounding_box", R + "/preprocessor/bounding_box.py")
D = load(P + ".preprocessor.radarscenes.dataset_creation", R + "/preprocessor/radarscenes/dataset_creation.py")

MODES = (("aligned", True, "translation"), ("none", False, "none"), ("translation", False, "translation"), ("en", False, "en"))


def track_ids(object_id):
    return np.array([b"" if i < 0 else str(int(i)).encode() for i in object_id])


def reference_rect(pts):
    """[cx, cy, l, w, theta in degrees] of one object by the reference's own functions."""
    if len(pts) == 1:
        return [pts[0, 0], pts[0, 1], 0.5, 0.5, 0.0]
    if len(pts) == 2:                          # the two-point branch has no function of its own: read it off the `none` encoding
        cloud = SimpleNamespace(X_cc=pts, track_id=np.array([b"a", b"a"]))
        row = D.GroundTruthCreator.create_2D_bounding_boxes(cloud, False, "none")[0]
        return [row[0], row[1], row[2], row[3], row[4] * 180 / np.pi]
    rel = B.BoundingBox(M.minimum_bounding_rectangle_with_rotation_alternative(pts), False).get_relative_bounding_box(0.0, 0.0)
    return [rel.x_center, rel.y_center, rel.l, rel.w, rel.theta]


def case(name, seed, frames, labels, n_background):
    pos, oid, ptr, tries = O.draw_admissible(seed, frames, n_background, labels)
    out = {}
    for key, aligned, inv in MODES:
        parts = []
        for a, b in zip(ptr[:-1], ptr[1:]):
            cloud = SimpleNamespace(X_cc=pos[a:b], track_id=track_ids(oid[a:b]))
            parts.append(D.GroundTruthCreator.create_2D_bounding_boxes(cloud, aligned, inv))
        out["boxes_" + key] = np.concatenate(parts)
    objs = O.objects(oid, ptr)
    rect = np.array([reference_rect(pos[rows]) for rows in objs])
    margins = O.admissibility(pos, oid, ptr)
    # the hull the oracle walks and the one the reference's Qhull returns must hold the same vertices
    from scipy.spatial import ConvexHull
    for rows in objs:
        if len(rows) >= 3:
            assert sorted(ConvexHull(pos[rows]).vertices.tolist()) == sorted(O.monotone_chain(pos[rows])), "hull vertices differ"
    np.savez_compressed(os.path.join(HERE, f"groundtruth_{name}.npz"), pos=pos, object_id=oid, frame_ptr=ptr, rect=rect,
                        seed=seed, **out, **{"margin_" + k: v for k, v in margins.items()})
    print(name, "seed", seed, "tries", tries, "points", len(pos), "objects", len(objs), {k: float(v.min()) for k, v in margins.items()})


if __name__ == "__main__":
    # every object size of {1, 2, 3, 4, 5, 17, 35, 63, 64, 65} (both sides of a wave boundary), ids reused across frames and not
    # dense, ~60 background points per frame, rows shuffled
    case("mixed", 11, [[1, 2, 3, 4, 5, 17, 35, 63], [64, 65, 2, 1, 3], [65, 63, 35, 17, 5, 4]],
         [[3, 7, 8, 12, 20, 21, 40, 41], [3, 7, 8, 12, 20], [3, 8, 9, 12, 20, 77]], 60)
