"""The one cache of tensors derived from weight values: bf16 / f16 weight planes, the window kernel's operand image, folded,
negated and concatenated weights, summed biases.  One key, one entry type, one lookup; the caller chooses where an entry lives.

    key    the slot name, the epoch, and per input tensor (address, version counter, shape, strides, dtype) or None for an absent
           optional input: plain values, hashable, compared with ==.  The address names the device too (host and device
           allocations of a process share one address space; a sixth field costs 0.14 us per hit).  A tensor, its detached aliases
           and full views of them share a key; a column view, an in-place write, a swapped ``param.data`` (``module.double()``,
           ``.to(device)``), a replacement Parameter and an epoch bump each give another one.
    entry  the value, the inputs and their storages (no address in the key can be recycled while the entry exists), and the stream
           that filled it with an event recorded behind the fill: a hit from another stream waits for it.
    store  a ``Table`` for operands without an owner (weight planes), or any object with a ``__dict__`` -- a module, a tensor --
           which then carries ONE attribute, ``HOLDER``, with the newest entry per slot name.

Imports torch only: the epoch is the ``CACHE_EPOCH`` attribute of ``epoch_owner`` (radargnn_amd.ops puts itself there)."""
import types

import torch

HOLDER = "_rgnn_derived"
epoch_owner = types.SimpleNamespace(CACHE_EPOCH=0)     # read at every lookup; a bump makes every store miss
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream_id() -> int:
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())                   # (0.3 us instead of the 8 of torch.cuda.current_stream())
    return torch.cuda.current_stream().cuda_stream


class Entry:
    __slots__ = ("key", "value", "inputs", "storages", "event", "stream_id")

    def __init__(self, key, value, inputs, cuda: bool, capturing: bool):
        self.key, self.value, self.inputs = key, value, inputs
        self.storages = tuple(t.untyped_storage() for t in inputs)
        self.event = self.stream_id = None                  # (CPU tensors: no stream to order against)
        if cuda:
            st = torch.cuda.current_stream()
            self.stream_id = st.cuda_stream
            if not capturing:                               # (a capture's own launches are ordered by the graph)
                self.event = torch.cuda.Event()
                self.event.record(st)

    def order_behind(self) -> None:
        """A hit from a stream other than the one that filled the entry: wait for the fill, and tell the caching allocator that THIS
        stream reads the value too -- an entry evicted (a newer weight version, the sweep, an epoch bump) while a launch of this
        stream still reads it must not have its block handed out again before that launch is through (the allocator only orders
        reuse on the allocating stream)."""
        st = torch.cuda.current_stream()
        if self.event is not None:
            st.wait_event(self.event)
        if not torch.cuda.is_current_stream_capturing():
            for v in self.value if isinstance(self.value, tuple) else (self.value,):
                if isinstance(v, torch.Tensor) and v.is_cuda:
                    v.record_stream(st)


class Table(dict):
    """key -> Entry, for operands without an owner.  A new entry for the same views at a newer version replaces the older one (an
    optimizer step bumps every parameter: a training loop must not park 18 dead plane sets per step), and a table that has reached
    ``LIMIT`` entries is cleared first (temporaries such as the transposed weights of a backward pass)."""
    LIMIT = 128

    def __init__(self):
        self.latest = {}                                    # key without epoch and versions -> newest key

    def clear(self) -> None:
        dict.clear(self)
        self.latest.clear()

    def insert(self, key, entry: Entry) -> None:
        if len(self) >= self.LIMIT:
            self.clear()
        views = (key[0],) + tuple(None if k is None else k[:1] + k[2:] for k in key[2:])
        old = self.latest.get(views)
        if old is not None and old != key:
            self.pop(old, None)
        self.latest[views] = key
        self[key] = entry


def key_of(slot, inputs) -> tuple:
    key = [slot, epoch_owner.CACHE_EPOCH]
    for t in inputs:
        key.append(None if t is None else (t.data_ptr(), t._version, t.shape, t.stride(), t.dtype))
    return tuple(key)


def get(store, slot, inputs, build, *, build_in_capture: bool = True):
    """The value ``build()`` derives from ``inputs`` (tensors, None in optional positions), built once per key.  ``store``: a Table, or
    the module / tensor that owns the value.  ``build_in_capture=False``: a first sight inside a stream capture builds nothing and
    returns None (the value would belong to that graph's memory pool)."""
    key = [slot, epoch_owner.CACHE_EPOCH]                   # key_of(), spelled out: a call is a tenth of a one-tensor hit
    for t in inputs:
        key.append(None if t is None else (t.data_ptr(), t._version, t.shape, t.stride(), t.dtype))
    key = tuple(key)
    if store.__class__ is Table:
        e = store.get(key)
    else:
        e = store.__dict__.get(HOLDER)     # (never through nn.Module.__setattr__: it would register a cached Parameter as a second one)
        e = None if e is None else e.get(slot)
        if e is not None and e.key != key:
            e = None
    if e is not None:
        if e.stream_id is not None and e.stream_id != _stream_id():
            e.order_behind()
        return e.value
    kept = tuple(t for t in inputs if t is not None and t is not store)      # (an entry ON a tensor must not keep that tensor alive)
    cuda = any(t.is_cuda for t in kept) or (isinstance(store, torch.Tensor) and store.is_cuda)
    capturing = cuda and torch.cuda.is_current_stream_capturing()
    if capturing and not build_in_capture:
        return None
    e = Entry(key, build(), kept, cuda, capturing)
    if store.__class__ is Table:
        store.insert(key, e)
    else:
        store.__dict__.setdefault(HOLDER, {})[slot] = e     # (looked up again: build() may have filled another slot of this holder)
    return e.value


def state_without_holder(obj) -> dict:
    """``__getstate__`` of a module that owns derived values: pickles and deep copies carry parameters and buffers, not the holder."""
    return {k: v for k, v in obj.__dict__.items() if k != HOLDER}
