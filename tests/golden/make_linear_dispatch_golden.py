"""Writes tests/golden/linear_dispatch_queries.npz: what rgnn_linear_fwd_path and rgnn_linear_fwd_fuses_a1_affine answer for
every argument set of tests/linear_dispatch_cases.py, under the default environment and under each switch of
linear_dispatch_cases.VARIANTS.  The queries run on the host alone, so this needs no GPU.

The fixture pins the dispatch of the commit BEFORE the launch plan (plan_linear, linear.hip) replaced the three hand-kept
copies of the decision: it was recorded in a checkout of that commit, built there, with this script and
tests/linear_dispatch_cases.py copied into it (the script loads the radargnn_amd package of the tree it lies in):

    python tests/golden/make_linear_dispatch_golden.py

Run it again only when the dispatch is MEANT to change, and say in the commit which answers moved.

Stored: path_<variant>, fuses_<variant> (int8 [cases]), section (the name of each case's block: "main" or the modification),
and the axes of the main grid (axis_<name>), whose full cross, last axis fastest, is the order of the "main" cases.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import linear_dispatch_cases as cases  # noqa: E402
from radargnn_amd import _lib  # noqa: E402


def main():
    out = {"axis_" + name: np.array(values) for name, values in cases.AXES}
    for variant in cases.VARIANTS:
        if variant != "default":
            os.environ[variant] = "1"
        _lib.lib.rgnn_env_reload()
        sections, path, fuses = cases.sweep(_lib.lib, _lib.RgnnLinearArgs)
        os.environ.pop(variant, None)
        out["section"] = sections
        out["path_" + variant], out["fuses_" + variant] = path, fuses
        main_grid = sections == "main"
        pairs = sorted(set(zip(path[main_grid].tolist(), fuses[main_grid].tolist())))
        print(f"{variant}: {len(path)} cases ({int(main_grid.sum())} on the main grid), (path, fuses) pairs there: {pairs}")
    _lib.lib.rgnn_env_reload()
    target = os.path.join(HERE, "linear_dispatch_queries.npz")
    np.savez_compressed(target, **out)
    print(target, os.path.getsize(target), "bytes;  library:", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
