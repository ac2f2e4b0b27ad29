#!/usr/bin/env python3
"""Host cost of a weight-derived cache HIT, per input tensor, on CPU Parameters (the lookup is host code; the eager single-frame
path is bound by the launching thread).  Times the two key schemes the cache replaced -- the plane caches' storage key behind one dict
probe, and the per-module folds' identity key with its pairwise comparison -- against ``radargnn_amd.derived.get`` for 1 and for 6
input tensors.  Prints the best and the spread of five repeats, in microseconds per tensor.

    python tools/time_derived_lookup.py"""
import importlib.util
import os
import timeit

import torch

_spec = importlib.util.spec_from_file_location(
    "derived", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "radargnn_amd", "derived.py"))
derived = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(derived)
EPOCH = 0


# ---- the schemes that were replaced -------------------------------------------------------------------------------------------
def old_wkey(w):
    if w is None:
        return None, None
    st = w.untyped_storage()
    return st, (st._cdata, w._version, w.storage_offset(), tuple(w.shape), w.stride())


def old_plane_hit(table, w1, w2=None):
    _, k1 = old_wkey(w1)
    _, k2 = old_wkey(w2)
    return table.get((k1, k2, EPOCH))


def old_cache_key(tensors):
    return (EPOCH, tuple(tensors), tuple(t._version for t in tensors), tuple((t.data_ptr(), t.device, t.dtype) for t in tensors))


def old_same_tensor(x, y):
    return x is y or (x.data_ptr() == y.data_ptr() and x.shape == y.shape and x.stride() == y.stride() and x.dtype == y.dtype)


def old_same_key(a, b):
    return (a is not None and a[0] == b[0] and len(a[1]) == len(b[1]) and all(old_same_tensor(x, y) for x, y in zip(a[1], b[1]))
            and a[2] == b[2] and a[3] == b[3])


class OldHolder:
    pass


def old_fold_hit(holder, tensors):
    key = old_cache_key(tensors)
    if not old_same_key(getattr(holder, "_fold_key", None), key):
        raise AssertionError("miss")
    return holder._fold_val


def main():
    ps = [torch.nn.Parameter(torch.randn(16, 16)) for _ in range(6)]
    table = {}
    _, k1 = old_wkey(ps[0])
    table[(k1, None, EPOCH)] = ("planes",)
    holder = OldHolder()
    holder._fold_key, holder._fold_val = old_cache_key(ps), ("fold",)
    new_table, new_holder = derived.Table(), OldHolder()
    one, six = (ps[0], None), tuple(ps)
    derived.get(new_table, "x3", one, lambda: ("planes",))
    derived.get(new_holder, "fold", six, lambda: ("fold",))
    build = lambda: (_ for _ in ()).throw(AssertionError("miss"))
    cases = [("parent plane key, 1 tensor", lambda: old_plane_hit(table, ps[0]), 1),
             ("parent fold key + compare, 6 tensors", lambda: old_fold_hit(holder, ps), 6),
             ("derived.get on a Table, 1 tensor", lambda: derived.get(new_table, "x3", one, build), 1),
             ("derived.get on a holder, 6 tensors", lambda: derived.get(new_holder, "fold", six, build), 6)]
    n = 100_000
    runs_of = {name: [] for name, _, _ in cases}
    for _ in range(5):                       # the four cases take turns, so a change of the machine's pace hits all of them alike
        for name, fn, tensors in cases:
            assert fn() is not None
            runs_of[name].append(timeit.timeit(fn, number=n) / n / tensors * 1e6)
    for name, runs in runs_of.items():
        print(f"{name:40s} best {min(runs):.3f} us/tensor   spread {max(runs) - min(runs):.3f}   runs {' '.join(f'{r:.3f}' for r in runs)}")


if __name__ == "__main__":
    main()
