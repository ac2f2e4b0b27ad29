"""radargnn_amd.derived on CPU tensors: the one key, the one entry type and the two kinds of store of the weight-derived cache."""
import copy
import gc
import io
import weakref

import torch
from torch import nn

from radargnn_amd import derived


class _Owner(nn.Linear):
    def __getstate__(self):
        return derived.state_without_holder(self)


def _key(*inputs):
    return derived.key_of("s", inputs)


def test_key_equalities():
    t = torch.arange(12.0).view(3, 4)
    assert _key(t) == _key(t) == _key(t.detach()) == _key(t.detach()[:, :])
    m = nn.Linear(4, 3)
    k = _key(m.weight, m.bias)
    m.to(torch.float32)                                      # a no-op conversion keeps the memory
    assert k == _key(m.weight, m.bias)
    assert _key(t, None) == _key(t.detach(), None)
    assert hash(_key(t, None)) == hash(_key(t.detach(), None)) and {_key(t): 1}[_key(t.detach())] == 1


def test_key_inequalities():
    t = torch.arange(12.0).view(3, 4)
    assert _key(t[:, :2]) != _key(t) and _key(t[:, :4]) == _key(t)           # a column view against the whole
    assert _key(t) != _key(t.view(4, 3)) and _key(t) != _key(t.view(torch.int32))
    p = nn.Parameter(torch.ones(4, 4))
    k = _key(p)
    with torch.no_grad():
        p.add_(1.0)                                          # an in-place write
    assert k != _key(p)
    k, old = _key(p), p.data                                 # (``old`` keeps the first storage's address taken)
    p.data = p.data.clone()
    assert k != _key(p)
    m = nn.Linear(4, 3)
    k32, version, w, keep = _key(m.weight), m.weight._version, m.weight, m.weight.data
    m.double()                                               # same Parameter object, same version, new storage
    assert m.weight is w and m.weight._version == version and k32 != _key(m.weight)
    k64, keep64 = _key(m.weight), m.weight.data
    m.float()
    assert m.weight is w and _key(m.weight) not in (k32, k64)
    k = _key(m.weight)
    m.weight = nn.Parameter(m.weight.detach().clone())       # a replacement Parameter
    assert k != _key(m.weight)
    k = _key(m.weight)
    derived.epoch_owner.CACHE_EPOCH += 1
    assert k != _key(m.weight)
    assert _key(t, None) != _key(None, t) and _key(t, None) != _key(t, t) and _key(None) != _key(t)
    del old, keep, keep64


def test_build_runs_once_per_key_and_hits_return_the_same_object():
    calls = []

    def build():
        calls.append(1)
        return torch.zeros(2), 7

    w, v = torch.ones(3, 3), torch.ones(3)
    for store in (derived.Table(), nn.Linear(2, 2), torch.ones(1)):
        calls.clear()
        first = derived.get(store, "a", (w, None), build)
        assert derived.get(store, "a", (w, None), build) is first and derived.get(store, "a", (w.detach()[:, :], None), build) is first
        assert len(calls) == 1
        assert derived.get(store, "a", (None, w), build) is not first and len(calls) == 2
        assert derived.get(store, "b", (w, v), build) is not first and len(calls) == 3
        assert derived.get(store, "b", (w, v), build) is derived.get(store, "b", (w, v), build) and len(calls) == 3
        w.add_(1.0)
        assert derived.get(store, "b", (w, v), build) is not first and len(calls) == 4
    # a first sight with build_in_capture=False builds all the same outside a capture (CPU tensors never ask CUDA)
    assert derived.get(torch.ones(1), "c", (w,), build, build_in_capture=False) is not None


def test_entries_keep_their_inputs_alive_until_replaced_or_cleared():
    table, module = derived.Table(), nn.Linear(2, 2)
    for store, drop in ((table, table.clear), (module, lambda: derived.get(module, "a", (torch.ones(2),), lambda: 0))):
        w = torch.ones(3, 3)
        ref = weakref.ref(w)
        derived.get(store, "a", (w, None), lambda: 1)
        del w
        gc.collect()
        assert ref() is not None
        drop()
        gc.collect()
        assert ref() is None
    # an entry that lives ON one of its inputs does not keep that tensor alive
    w = torch.ones(3, 3)
    ref = weakref.ref(w)
    derived.get(w, "image", (w, None), lambda: 1)
    del w
    assert ref() is None


def test_table_replaces_older_versions_and_sweeps_at_its_limit():
    table, w, w2 = derived.Table(), torch.ones(3, 3), torch.ones(2, 3)
    for _ in range(5):
        derived.get(table, "x3", (w, w2), lambda: torch.zeros(1))
        assert len(table) == 1
        w.add_(1.0)                                          # the same views at a bumped version
    derived.get(table, "x3", (w[:, :2], w2), lambda: torch.zeros(1))
    assert len(table) == 2                                   # (other views: another entry)
    table.clear()
    keep = [torch.ones(1) for _ in range(derived.Table.LIMIT)]
    for t in keep:
        derived.get(table, "x3", (t, None), lambda: torch.zeros(1))
    assert len(table) == derived.Table.LIMIT == 128
    derived.get(table, "x3", (w, None), lambda: torch.zeros(1))
    assert len(table) == 1 and len(table.latest) == 1


def test_holder_registers_nothing_and_stays_out_of_pickles_and_copies():
    m = _Owner(3, 2)
    names, params = list(m.state_dict()), list(m.parameters())
    assert derived.get(m, "neg", (m.weight,), lambda: -m.weight.detach()) is derived.get(m, "neg", (m.weight,), lambda: None)
    assert derived.HOLDER in m.__dict__ and m.__dict__[derived.HOLDER]["neg"].inputs[0] is m.weight
    assert list(m.state_dict()) == names and len(list(m.parameters())) == len(params)
    assert all(a is b for a, b in zip(m.parameters(), params))
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    for back in (torch.load(buf, weights_only=False), copy.deepcopy(m)):
        assert derived.HOLDER not in back.__dict__ and not hasattr(back, derived.HOLDER)
        assert list(back.state_dict()) == names
        assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), m.state_dict().values()))


def test_epoch_bump_makes_every_store_miss():
    a, b = torch.ones(4), torch.ones(4)
    stores = (derived.Table(), nn.Linear(2, 2), torch.ones(1))
    first = [derived.get(s, "sum_bias", (a, b), lambda: a + b) for s in stores]
    assert all(derived.get(s, "sum_bias", (a, b), lambda: None) is f for s, f in zip(stores, first))
    derived.epoch_owner.CACHE_EPOCH += 1                     # (what ops.invalidate_weight_caches() does; the inputs did not change)
    again = [derived.get(s, "sum_bias", (a, b), lambda: a + b) for s in stores]
    assert all(x is not f and torch.equal(x, f) for x, f in zip(again, first))
    assert len(stores[0]) == 1                               # (the table's older entry went with the bump's first insert)
