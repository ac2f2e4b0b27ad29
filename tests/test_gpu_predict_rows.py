"""``ops.predict_rows`` (csrc/norm.hip: k_predict_rows, rgnn_predict_rows) -- the one-launch epilogue of a prediction step: softmax
of the logits, the boxes and the two halves of ``y`` written at a row offset of whole-split buffers.

* ``prob`` carries the bits of ``ops.softmax_rows`` on the same logits (the same statements in the same order) and lies within the
  bound tests/test_gpu_loss_edges.py states and checks for that kernel (``check_softmax``: eps32 (|x - max| + n + 4) ref + 2^-126
  against ``torch.softmax(x.double(), 1)``), on that file's logit rows: +-88, +-1e4, equal entries, -inf entries, ties -- plus one
  row with a NaN, which comes out all NaN like torch's and is held to the bits only;
* the three copies are bit patterns (random words: NaN payloads, -0.0, denormals), compared as integers;
* rows of the buffers outside [row0, row0 + n) keep a sentinel; ``y=None`` leaves the target buffers alone; n = 0 writes nothing.

n crosses the wave (64) and the block (256) and takes several blocks (1000); every (W, Wy) of {4, 5}^2; contiguous inputs and views
with a row stride of width + 3."""
import itertools

import pytest
import torch

from tests.test_gpu_loss_edges import check_softmax, softmax_rows_under_test

pytestmark = pytest.mark.gpu

ROW0, TAIL = 3, 5                       # rows of the buffers in front of and behind the step's rows
N_MAX = 1000
_cache = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radargnn_amd import ops
    return ops


def logits(k):
    """[N_MAX + 1, k] on the host: the 257 rows of the softmax edge test (its planted rows on top), random rows at three scales,
    and -- k >= 2 -- a last row with one NaN.  The float64 reference work is done once per k (``reference``)."""
    if k not in _cache:
        g = torch.Generator().manual_seed(77 + k)
        x = torch.cat((softmax_rows_under_test(257, k), torch.randn(N_MAX - 257, k, generator=g) * 5,
                       torch.randn(1, k, generator=g)))
        x[600:800] *= 20
        if k >= 2:
            x[N_MAX, 1] = float("nan")
        _cache[k] = x
    return _cache[k]


def take(x, n):
    """n rows of the logits: the first n, and for k >= 2 the NaN row in place of the last (n >= 2)."""
    rows = x[:n].clone()
    if n >= 2 and x.shape[1] >= 2:
        rows[n - 1] = x[N_MAX]
    return rows


def words(shape, dtype, seed):
    """Random bit patterns of a float dtype, with -0.0 and two NaN payloads (a quiet and a signalling one) planted."""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.float32:
        t = torch.randint(-2 ** 31, 2 ** 31, shape, generator=g, dtype=torch.int64).to(torch.int32)
        plant = [-2 ** 31, 0x7FC00001, 0x7F800123]
    else:
        t = torch.randint(-2 ** 62, 2 ** 62, shape, generator=g, dtype=torch.int64) * 2 + torch.randint(0, 2, shape, generator=g)
        plant = [-2 ** 63, 0x7FF8000000000001, 0x7FF0000000000123]
    flat = t.view(-1)
    for i, p in enumerate(plant):
        if flat.numel():
            flat[i * 7 % flat.numel()] = p
    return t.view(dtype)


def as_int(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def strided(t):
    """The same values as a view with a row stride of width + 3 (and a data pointer that is not the allocation's)."""
    wide = torch.zeros((t.shape[0], t.shape[1] + 3), dtype=t.dtype, device=t.device)
    view = wide[:, 1:1 + t.shape[1]]
    as_int(view).copy_(as_int(t))
    assert t.shape[0] < 2 or view.stride(0) == t.shape[1] + 3
    return view


def sentinel(dtype) -> int:
    return 0x5A5A5A5A if dtype == torch.float32 else 0x5A5A5A5A5A5A5A5A


def buffers(n, k, w, wy, ydtype):
    """prob, bb_out, class_true, bb_true with ROW0 rows in front of and TAIL rows behind the step's n, every word a sentinel."""
    rows = ROW0 + n + TAIL
    out = (torch.empty((rows, k), device="cuda"), torch.empty((rows, w), device="cuda"),
           torch.empty(rows, dtype=ydtype, device="cuda"), torch.empty((rows, wy), dtype=ydtype, device="cuda"))
    for buf in out:
        as_int(buf).fill_(sentinel(buf.dtype))
    return out


def untouched(buf, n):
    outside = torch.cat((as_int(buf)[:ROW0], as_int(buf)[ROW0 + n:]))
    return bool((outside == sentinel(buf.dtype)).all())


@pytest.mark.parametrize("ydtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("k", [1, 6, 11])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_predict_rows_sweep(ops, n, k, ydtype):
    x = take(logits(k), n)
    xd = x.cuda()
    want = ops.softmax_rows(xd)                      # the kernel this one must agree with bit for bit (not the code under test)
    nan_row = n >= 2 and k >= 2
    for w, wy, layout in itertools.product((4, 5), (4, 5), ("contiguous", "strided")):
        bb = words((n, w), torch.float32, 10 * n + w).cuda()
        y = words((n, 1 + wy), ydtype, 20 * n + wy).cuda()
        ins = (xd, bb, y) if layout == "contiguous" else (strided(xd), strided(bb), strided(y))
        prob, bb_out, ct, bt = buffers(n, k, w, wy, ydtype)
        ops.predict_rows(*ins, prob, bb_out, ct, bt, row0=ROW0)
        tag = f"n={n} k={k} w={w} wy={wy} {ydtype} {layout}"
        got = prob[ROW0:ROW0 + n]
        assert torch.equal(as_int(got), as_int(want)), tag
        assert torch.equal(as_int(bb_out[ROW0:ROW0 + n]), as_int(bb)), tag
        assert torch.equal(as_int(ct[ROW0:ROW0 + n]), as_int(y)[:, 0]), tag
        assert torch.equal(as_int(bt[ROW0:ROW0 + n]), as_int(y)[:, 1:]), tag
        for buf in (prob, bb_out, ct, bt):
            assert untouched(buf, n), tag
    # the softmax bound of tests/test_gpu_loss_edges.py, against float64 torch (the NaN row apart: NaN everywhere, like torch's)
    host = got.cpu()
    if nan_row:
        assert bool(torch.isnan(host[n - 1]).all()) and bool(torch.isnan(torch.softmax(x[n - 1:].double(), 1)).all())
        x, host = x[:n - 1], host[:n - 1]
    check_softmax(f"predict_rows n={n} k={k}", x, host)


def test_without_y_the_target_buffers_are_not_touched(ops):
    n, k, w, wy = 257, 6, 5, 5
    xd = take(logits(k), n).cuda()
    bb = words((n, w), torch.float32, 1).cuda()
    prob, bb_out, ct, bt = buffers(n, k, w, wy, torch.float64)
    ops.predict_rows(xd, bb, None, prob, bb_out, ct, bt, row0=ROW0)
    assert torch.equal(as_int(prob[ROW0:ROW0 + n]), as_int(ops.softmax_rows(xd)))
    assert torch.equal(as_int(bb_out[ROW0:ROW0 + n]), as_int(bb))
    assert untouched(ct, 0) and untouched(bt, 0)
    ops.predict_rows(xd, bb, None, prob, bb_out, row0=ROW0)          # ... nor needed


def test_no_rows_no_launch(ops):
    from radargnn_amd import _lib
    k, w, wy = 6, 5, 5
    prob, bb_out, ct, bt = buffers(0, k, w, wy, torch.float32)
    empty = lambda c, dt=torch.float32: torch.empty((0, c), dtype=dt, device="cuda")
    ops.predict_rows(empty(k), empty(w), empty(1 + wy), prob, bb_out, ct, bt, row0=ROW0)
    for buf in (prob, bb_out, ct, bt):
        assert untouched(buf, 0)
    # the export itself returns before it looks at a pointer
    assert _lib.lib.rgnn_predict_rows(None, 0, 1, None, 0, 0, None, 0, 0, 0, 0, None, 0, None, 0, None, None, 0, None) == 0


def test_wrapper_refuses_what_the_kernel_cannot_take(ops):
    n, k, w, wy = 4, 6, 5, 5
    cls, bb = torch.randn(n, k, device="cuda"), torch.randn(n, w, device="cuda")
    y = torch.randn(n, 1 + wy, device="cuda", dtype=torch.float64)
    prob, bb_out, ct, bt = buffers(n, k, w, wy, torch.float64)
    with pytest.raises(RuntimeError):
        ops.predict_rows(cls.cpu(), bb, y, prob, bb_out, ct, bt, row0=ROW0)
    with pytest.raises(TypeError):
        ops.predict_rows(cls.double(), bb, y, prob, bb_out, ct, bt, row0=ROW0)
    with pytest.raises(TypeError):
        ops.predict_rows(cls, bb, y.float(), prob, bb_out, ct, bt, row0=ROW0)         # y and its buffers: one dtype
    with pytest.raises(TypeError):
        ops.predict_rows(cls, bb, y.long(), prob, bb_out, ct, bt, row0=ROW0)
    with pytest.raises(ValueError):
        ops.predict_rows(cls, bb[:3], y, prob, bb_out, ct, bt, row0=ROW0)
    with pytest.raises(ValueError):
        ops.predict_rows(cls, bb, y, prob, bb_out, ct, bt, row0=ROW0 + TAIL + 1)       # past the end of the buffers
    with pytest.raises(ValueError):
        ops.predict_rows(cls, bb, y, prob[:, :5], bb_out, ct, bt, row0=ROW0)           # width
    with pytest.raises(ValueError):
        ops.predict_rows(cls, bb, y, prob, bb_out.t().contiguous().t(), ct, bt, row0=ROW0)   # written in place: no copy stands in
    with pytest.raises(ValueError):
        ops.predict_rows(cls, bb, y, prob, bb_out, None, bt, row0=ROW0)
    for buf in (prob, bb_out, ct, bt):
        assert untouched(buf, 0)
    torch.cuda.synchronize()
