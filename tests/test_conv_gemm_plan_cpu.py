"""The implicit-GEMM dispatcher's decisions, pinned per shape (CPU only: the three queries launch nothing).

test_conv1d_elementwise_cpu.py compares the SET of labels the grid reaches with the case table; a change that moves a threshold but keeps the
set passes there.  This file compares every grid point with tests/golden/conv1d_dispatch.npz:

  sf_op_conv1d_variant        fp32 / fp32x / bf16 / fp16, groups 0 and 8        -> return code and label
  sf_op_conv1d_bwd_variant    fp32 / fp32x, stride 1, no upsampling              -> return code and label
  sf_op_conv1d_train_images   fp32 / fp32x, stride 1, no upsampling, groups 0, 8 -> image mask (-1: refused)

over GRID_CH x GRID_CH x GRID_TAPS x GRID_GEOM x GRID_ROWS of test_conv1d_elementwise_cpu.py.  The fixture holds the distinct strings once and a
small-integer index per point.  It was recorded by tools/record_conv1d_dispatch.py from the library as it stood BEFORE the dispatcher was
rebuilt around one plan per launch (ConvGemmPlan), and is regenerated only by a change that means to move a threshold.
"""
import ctypes as C
import os

import numpy as np
import pytest

from test_conv1d_elementwise_cpu import DTYPES, GRID_CH, GRID_GEOM, GRID_ROWS, GRID_TAPS

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv1d_dispatch.npz")
GROUPS = (0, 8)
TRAIN_MODES = ("fp32", "fp32x")
W_PROBE = 4096   # the weight pointer of the image query: aligned as a tensor's storage is, never read


def points(train_only=False):
    """(C, N, taps, stride, up, L) per grid point, in a fixed order; Lout = the grid's row count with pad = taps // 2 and one clip."""
    out = []
    for Cc in GRID_CH:
        for N in GRID_CH:
            for taps in GRID_TAPS:
                for stride, up in GRID_GEOM:
                    if train_only and (stride, up) != (1, 1):
                        continue
                    for rows in GRID_ROWS:
                        if rows % up:
                            continue
                        L = rows // up if up > 1 else (rows * 2 if stride == 2 else rows)
                        out.append((Cc, N, taps, stride, up, L))
    return out


def record(lib, dtypes_of):
    """Every table of the fixture from `lib`: {key: (array of return codes or masks, list of labels or None)}."""
    tables = {}
    buf = C.create_string_buffer(192)
    for dtype in DTYPES:
        for g in GROUPS:
            rcs, labels = [], []
            for Cc, N, taps, stride, up, L in points():
                rcs.append(lib.sf_op_conv1d_variant(dtypes_of[dtype], 1, L, Cc, N, taps, stride, taps // 2, up, g, buf, 192))
                labels.append(buf.value.decode())
            tables[f"variant_{dtype}_g{g}"] = (np.asarray(rcs, dtype=np.int16), labels)
    for mode in TRAIN_MODES:
        rcs, labels = [], []
        for Cc, N, taps, _, _, L in points(train_only=True):
            rcs.append(lib.sf_op_conv1d_bwd_variant(dtypes_of[mode], 1, L, Cc, N, taps, taps // 2, buf, 192))
            labels.append(buf.value.decode())
        tables[f"bwd_{mode}"] = (np.asarray(rcs, dtype=np.int16), labels)
        for g in GROUPS:
            masks = [lib.sf_op_conv1d_train_images(dtypes_of[mode], W_PROBE, 1, L, Cc, N, taps, taps // 2, g) for Cc, N, taps, _, _, L in points(train_only=True)]
            tables[f"images_{mode}_g{g}"] = (np.asarray(masks, dtype=np.int16), None)
    return tables


def pack(tables):
    """The tables as the arrays of the .npz: one list of distinct strings, an index array per labelled table."""
    strings = sorted({s for _, labels in tables.values() if labels is not None for s in labels})
    index = {s: i for i, s in enumerate(strings)}
    arrays = {"strings": np.asarray(strings)}
    for key, (codes, labels) in tables.items():
        arrays[key + "_rc"] = codes
        if labels is not None:
            arrays[key + "_label"] = np.asarray([index[s] for s in labels], dtype=np.int16)
    return arrays


@pytest.fixture(scope="module")
def now():
    from syncfusion_amd import _lib

    return record(_lib.load(), _lib.DTYPES)


@pytest.fixture(scope="module")
def pinned():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _keys():
    return ([f"variant_{d}_g{g}" for d in DTYPES for g in GROUPS] + [f"bwd_{m}" for m in TRAIN_MODES] +
            [f"images_{m}_g{g}" for m in TRAIN_MODES for g in GROUPS])


@pytest.mark.parametrize("key", _keys())
def test_every_grid_point_is_what_the_fixture_pins(key, now, pinned):
    pts = points(train_only=not key.startswith("variant"))
    codes, labels = now[key]
    want_codes = pinned[key + "_rc"]
    assert len(codes) == len(pts) == len(want_codes), "the grid changed: the fixture no longer lines up with it"
    have = [(int(c),) for c in codes]
    want = [(int(c),) for c in want_codes]
    if labels is not None:
        strings = pinned["strings"]
        have = [h + (s,) for h, s in zip(have, labels)]
        want = [w + (str(strings[i]),) for w, i in zip(want, pinned[key + "_label"])]
    bad = [(p, h, w) for p, h, w in zip(pts, have, want) if h != w]
    assert not bad, f"{key}: {len(bad)} of {len(pts)} grid points differ; first (C, N, taps, stride, up, L) -> now / pinned:\n" + "\n".join(
        f"  {p}: {h} / {w}" for p, h, w in bad[:8])


def test_the_fixture_holds_exactly_these_tables(pinned):
    assert sorted(pinned) == sorted(["strings"] + [k + "_rc" for k in _keys()] + [k + "_label" for k in _keys() if not k.startswith("images")])
