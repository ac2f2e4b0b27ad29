"""Argument sets for the host-side dense-layer dispatch (rgnn_linear_fwd_path, rgnn_linear_fwd_fuses_a1_affine, rgnn_linear_fwd_plan):
none of these functions touches the device or reads behind a pointer, so the operands are made-up addresses.  Shared by
tests/golden/make_linear_dispatch_golden.py (which records the answers of a library build) and tests/test_linear_dispatch_host.py
(which compares the current build with the record); the ORDER of the cases is part of the fixture.

Only calls that rgnn_linear_fwd accepts and that ``ops.linear`` can produce: W2 is NULL whenever w_split >= n."""
import ctypes as C
import itertools

import numpy as np

# ---- the main grid: a full cross of these axes, in this order (last axis fastest)
AXES = (
    ("m", (1, 255, 3000, 4096, 192000)),
    ("n", (4, 16, 32, 33, 36, 64, 68, 96, 100, 128, 160, 224, 256, 272, 464, 928)),
    ("k1", (4, 5, 8, 16, 32, 48, 128, 224, 512, 528, 1024)),
    ("k2", (0, 4, 16, 32)),
    ("planes", (0, 1)),
    ("f16", (0, 1)),                  # f16 planes and the bounds of both activation blocks
    ("row_index", (0, 1)),
    ("col_stats", (0, 1)),
    ("relu_from_col", (0, 8)),
)
# ---- the smaller crosses: every modification below on this reduced grid
SMALL_AXES = (
    ("m", (255, 4096, 192000)),
    ("n", (16, 64, 100, 224, 464)),
    ("k1", (8, 32, 224, 528)),
    ("k2", (0, 32)),
    ("operands", ("fp32", "planes", "planes+f16")),
    ("row_index", (0, 1)),
)
MODS = ("residual", "accumulate", "gather_only", "a1_panel_segment",
        "A1+4", "A2+4", "W1+4", "out+4", "bias1+4", "residual+4",
        "lda1+1", "lda2+1", "ldw+1", "ldo+1", "ldo+2", "ldr+1",
        "w_split<n", "w_split<n,W2+4", "w_split<n,w_split%4",
        "ldo_over_2GiB", "lda1_over_2GiB")
# switches under which the whole table is recorded again
VARIANTS = ("default", "RGNN_LINEAR_FP32", "RGNN_X3_NODMA", "RGNN_LINEAR_NO_F16")

# made-up device addresses, 16-byte aligned and 256 MiB apart
A1, A2, W1, W2, OUT, BIAS1, BIAS2, RES, STATS, ROWS, MDEV, PLANES, PLANES16, BOUND1, BOUND2, TABLE, SEGMENTS, RES_INDEX = (
    (i + 1) << 28 for i in range(18))
LIM = (1 << 31) - 64


def base_fields(m, n, k1, k2, planes, f16, row_index, col_stats=0, relu_from_col=0, planes_kp=None):
    """One call of ``ops.linear``'s shape: contiguous operands, one weight block."""
    k = k1 + k2
    return dict(A1=A1, lda1=k1, k1=k1, A2=A2 if k2 else None, lda2=k2, k2=k2, W1=W1, W2=None, ldw=k, w_split=n,
                bias1=BIAS1, bias2=None, residual=None, ldr=0, out=OUT, ldo=n, m=m, n=n, relu_out=1,
                col_stats=STATS if col_stats else None, row_index=ROWS if row_index else None,
                m_dev=MDEV if row_index else None, accumulate=0, gather_only=0, residual_index=None,
                W_planes=PLANES if planes else None, w_planes_kp=planes_kp(k) if planes else 0,
                splitk_ws=None, splitk_ws_bytes=0, a1_scale_shift=None, a1_relu=1, relu_from_col=relu_from_col,
                W_planes_f16=PLANES16 if f16 else None, a1_bound=BOUND1 if f16 else None,
                a2_bound=BOUND2 if (f16 and k2) else None, out_absmax=None, a1_panel_segment=None)


def apply_mod(f, mod):
    """Returns the modified fields, or None where the modification makes no valid call."""
    f = dict(f)
    m, n = f["m"], f["n"]
    if mod == "residual":
        f.update(residual=RES, ldr=n)
    elif mod in ("accumulate", "gather_only"):
        if not f["row_index"] or (mod == "accumulate" and f["col_stats"]):
            return None
        f[mod] = 1
    elif mod == "a1_panel_segment":
        if not f["row_index"]:
            return None
        f.update(a1_scale_shift=TABLE, a1_panel_segment=SEGMENTS)
    elif mod in ("A1+4", "W1+4", "out+4", "bias1+4"):
        f[mod[:-2]] += 4
    elif mod == "A2+4":
        if not f["k2"]:
            return None
        f["A2"] += 4
    elif mod == "residual+4":
        f.update(residual=RES + 4, ldr=n)
    elif mod in ("lda1+1", "ldw+1", "ldo+1"):
        f[mod[:-2]] += 1
    elif mod == "ldo+2":
        f["ldo"] += 2
    elif mod == "lda2+1":
        if not f["k2"]:
            return None
        f["lda2"] += 1
    elif mod == "ldr+1":
        f.update(residual=RES, ldr=n + 1)
    elif mod.startswith("w_split<n"):
        split = n // 2 - (1 if mod.endswith("w_split%4") else 0)
        if split < 1:
            return None
        f.update(w_split=split, W2=W2 + (4 if mod.endswith("W2+4") else 0), bias2=BIAS2)
    elif mod == "ldo_over_2GiB":                    # the smallest row stride (a multiple of 4) whose extent passes 2^31 - 64 bytes
        if m < 2:
            return None
        f["ldo"] = ((LIM // 4 - n) // (m - 1) // 4 + 1) * 4
    elif mod == "lda1_over_2GiB":
        if m < 2:
            return None
        f["lda1"] = ((LIM // 4 - f["k1"]) // (m - 1) // 4 + 1) * 4
    else:
        raise ValueError(mod)
    return f


def cases(planes_kp):
    """Yields (section, fields) for the main grid, then for the smaller crosses.  ``planes_kp``: rgnn_linear_planes_kp."""
    for m, n, k1, k2, planes, f16, row_index, col_stats, relu_from in itertools.product(*(v for _, v in AXES)):
        yield "main", base_fields(m, n, k1, k2, planes, f16, row_index, col_stats, relu_from, planes_kp)
    for mod in MODS:
        for m, n, k1, k2, operands, row_index in itertools.product(*(v for _, v in SMALL_AXES)):
            f = apply_mod(base_fields(m, n, k1, k2, operands != "fp32", operands == "planes+f16", row_index, planes_kp=planes_kp), mod)
            if f is not None:
                yield mod, f


def fill(args, fields):
    for name, value in fields.items():
        setattr(args, name, value)
    return args


def sweep(lib, args_type, want_plan=False):
    """Runs every case through the library's queries.  Returns (sections, path int8 [cases], fuses int8 [cases]) and, with
    ``want_plan``, the rgnn_linear_fwd_plan rows int32 [cases, 8] and every case's n as well."""
    sections, path, fuses, plans, ns = [], [], [], [], []
    args, out = args_type(), (C.c_int32 * 8)()
    for section, fields in cases(lib.rgnn_linear_planes_kp):
        fill(args, fields)
        sections.append(section)
        path.append(lib.rgnn_linear_fwd_path(C.byref(args)))
        fuses.append(lib.rgnn_linear_fwd_fuses_a1_affine(C.byref(args)))
        if want_plan:
            lib.rgnn_linear_fwd_plan(C.byref(args), C.byref(out))
            plans.append(list(out))
            ns.append(fields["n"])
    res = (np.array(sections), np.array(path, dtype=np.int8), np.array(fuses, dtype=np.int8))
    return res + (np.array(plans, dtype=np.int32), np.array(ns)) if want_plan else res
