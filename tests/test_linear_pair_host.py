"""rgnn_linear_fwd_pair_fuses on the CPU: the rule that decides whether two dense launches run as one grid is host arithmetic on the
argument values (made-up 16-byte-aligned addresses; nothing behind them is read, nothing is launched)."""
import ctypes as C

import pytest

from radargnn_amd import _lib

ROWS = 192000                # the benchmark's node count: the planner picks the production tile widths without help


def args(n, k=224, **over):
    """A row-subset launch of the f16x2 form: x [ROWS, k] -> out [ROWS, n] on a row list, weight planes and bounds given."""
    a = _lib.RgnnLinearArgs()
    a.A1, a.lda1, a.k1 = 0x10000000, k, k
    a.W1, a.ldw, a.w_split = 0x20000000, k, n
    a.out, a.ldo, a.m, a.n = 0x30000000 + 0x10000000 * (n % 7), n, ROWS, n
    a.row_index, a.m_dev = 0x70000000, 0x70100000
    a.W_planes, a.w_planes_kp = 0x71000000, _lib.lib.rgnn_linear_planes_kp(k)
    a.W_planes_f16, a.a1_bound = 0x72000000, 0x73000000
    a.a1_scale_shift, a.a1_relu = 0x74000000, 1
    for name, v in over.items():
        setattr(a, name, v)
    return a


def fuses(first, second):
    ref = lambda a: None if a is None else C.byref(a)
    return bool(_lib.lib.rgnn_linear_fwd_pair_fuses(ref(first), ref(second)))


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in ("RGNN_NO_LINEAR_PAIR", "RGNN_DMA_WAVES", "RGNN_DMA_TN", "RGNN_DMA_NOSK", "RGNN_DMA_NOPSK", "RGNN_LINEAR_NO_F16"):
        monkeypatch.delenv(name, raising=False)
    _lib.lib.rgnn_env_reload()


@pytest.mark.parametrize("n_a,n_b,k", [(464, 224, 224), (464, 128, 224), (272, 64, 128)])
def test_the_conv_layers_pairs_fuse(n_a, n_b, k):
    assert fuses(args(n_a, k), args(n_b, k))
    assert fuses(args(n_b, k), args(n_a, k))              # the part with more tiles leads, whichever argument it is
    assert not fuses(args(n_a, k, m=256), args(n_b, k))   # ... and here that is the update: (7, 5), (4, 5), (2, 3) are not built


def test_what_keeps_a_pair_on_two_launches(monkeypatch):
    q = lambda **kw: args(464, **kw)
    u = lambda **kw: args(224, **kw)
    assert fuses(q(), u())
    assert not fuses(q(), args(96))                                           # no (5, 3) pair
    assert not fuses(q(), u(a1_panel_segment=0x75000000))                     # per-segment tables
    assert not fuses(q(a1_panel_segment=0x75000000), u())
    assert not fuses(q(), u(W_planes_f16=0))                                  # bf16x3 form
    assert not fuses(q(), u(row_index=0, m_dev=0))                            # a dense launch
    assert not fuses(q(), u(accumulate=1))
    assert not fuses(q(), u(A1=q().out))                                      # reads what the other writes
    assert not fuses(None, u()) and not fuses(q(), None)
    monkeypatch.setenv("RGNN_NO_LINEAR_PAIR", "1")
    _lib.lib.rgnn_env_reload()
    assert not fuses(q(), u())


def test_static_schedule_only():
    """With the hand-over workspace a launch of eight or more k-steps (K >= 256 in the f16x2 form) may take stream-K (one column
    tile) or parallel split-K (tiles of at most 128 columns) depending on the row count on the device: such a part never pairs."""
    ws = dict(splitk_ws=0x78000000, splitk_ws_bytes=_lib.lib.rgnn_linear_splitk_ws_bytes())
    assert fuses(args(464, 224, **ws), args(224, 224, **ws))                  # 7 k-steps: static whatever m_dev holds
    assert fuses(args(464, 256), args(224, 256))                              # no workspace: static
    assert not fuses(args(464, 256, **ws), args(224, 256, **ws))              # 8 k-steps, one column tile: stream-K possible
    assert not fuses(args(464, 256, **ws), args(128, 256, **ws))              # 128-column tile: parallel split-K possible
