"""CPU half of the element-wise gate on the 1-D convolution kernels (conv1d_ref.py, test_gpu_conv1d_elementwise.py): no GPU needed.

  a. Coverage is pinned.  sf_op_conv1d_variant (a query: nothing is launched) is swept over a fixed grid per dtype, and the set of labels it
     returns must EQUAL the set of labels of the GPU case table: a variant that becomes reachable fails here until it has a case, and a case
     whose shape drifted to another kernel fails here too (every row's expected_label is asked for as well).
  b. Every case of the table, emulated on the CPU (same rounded operands, fp32 accumulation, one output rounding), passes the gate, and the
     accumulation part of the bound -- measured on the fp32 value before the output rounding -- is used to at most half: if a case cannot
     meet that, the derivation is wrong, not the threshold.
  c. Planted faults, each confined to one 32x32 MFMA tile (or to the rows the ragged last row tile holds) of one case, fail the gate in all
     four dtypes -- and, for bf16 and fp16, pass test_gpu_ops.TOL as a whole-tensor rel-L2, which is what the older gate misses.

Labels that the source's name tables hold but no op-level call reaches (none of them has a case, and the sweep must not return them):
  * conv_gemm<..,64x64,scalarA>: a channel count that is no multiple of 32 goes to conv_direct at op level (capi_misc.cpp, `direct`);
  * conv_gemm_mt 256x64, 128x128,2wg, 192x128,2wg, 256x64,2wg: chosen for the video geometry (geom = 1, the onset net) only; 128x192 with the
    three-slot ring and 256x256: behind tuning hooks only (conv_gemm_mt_variant);
  * conv_gemm_sk / fast / wp 64x64 and 64x32: conv_gemm_sk_variant leaves the 32x32 tile only beyond 4096 tiles of 32x32, and a launch
    reaches these families with fewer than 500 tiles of 64x64 (short_act) or fewer than 256 classic blocks of at most 128x128 (use_sk), i.e.
    with at most 4096 tiles of 32x32;
  * conv_gemm_v2<bf16 / f16,128x128> and conv_gemm_v2<f32,128x64>: conv_gemm_v2_plan never picks them for that type; conv_gemm_v2<bf16 /
    f16,128x64> wants M <= 8192, N >= 1024, K >= 2048 and at least 500 tiles of 64x64 -- 80 or more tiles of 128x128 with K >= 256, which the
    macro tiles take first;
  * conv_gemm<invalid>: a GroupNorm prologue on a channel count that is no multiple of 32 (groups > 0 is not part of this gate).
"""
import ctypes as C

import pytest
import torch

import conv1d_ref as R
from test_gpu_conv1d_elementwise import CASES, case_id
from test_gpu_ops import TOL

DTYPES = ("fp32", "fp32x", "bf16", "fp16")
GRID_CH = (8, 32, 64, 96, 128, 192, 256, 320, 512, 1024, 1536)
GRID_TAPS = (1, 3, 5)
GRID_GEOM = ((1, 1), (2, 1), (1, 2))                              # (stride, up)
GRID_ROWS = (1, 2, 31, 32, 33, 64, 100, 128, 352, 1000, 2816, 5632, 10240, 22528, 45056, 65536, 131072)   # B * Lout, one clip


def _query(dtype, B, L, Cc, N, taps, stride, pad, up):
    from syncfusion_amd import _lib

    lib = _lib.load()
    buf = C.create_string_buffer(96)
    rc = lib.sf_op_conv1d_variant(_lib.DTYPES[dtype], B, L, Cc, N, taps, stride, pad, up, 0, buf, 96)
    return rc, buf.value.decode()


@pytest.mark.parametrize("dtype", DTYPES)
def test_label_sweep_equals_case_table(dtype):
    seen = set()
    for Cc in GRID_CH:
        for N in GRID_CH:
            for taps in GRID_TAPS:
                for stride, up in GRID_GEOM:
                    for rows in GRID_ROWS:
                        if rows % up:
                            continue
                        L = rows // up if up > 1 else (rows * 2 if stride == 2 else rows)     # Lout = rows with pad = taps // 2
                        rc, label = _query(dtype, 1, L, Cc, N, taps, stride, taps // 2, up)
                        if rc != 0:
                            assert Cc % 32 != 0 and N > 32, f"query failed for {(dtype, L, Cc, N, taps, stride, up)}"   # thin path: N <= 32 only
                            continue
                        seen.add(label)
    table = {c.expected_label for c in CASES if c.dtype == dtype}
    assert seen == table, f"{dtype}: reachable without a case {sorted(seen - table)}; cases no grid point reaches {sorted(table - seen)}"


def test_every_case_names_the_kernel_it_reaches_and_stays_small():
    for c in CASES:
        rc, label = _query(c.dtype, c.B, c.L, c.C, c.N, c.taps, c.stride, c.pad, c.up)
        assert rc == 0 and label == c.expected_label, f"{case_id(c)}: the dispatcher takes {label!r}, the row says {c.expected_label!r}"
        assert c.ref_gflop() <= 20.0 and c.K <= 3072, case_id(c)
        assert (c.expected_label == "conv_direct") == (c.C % 32 != 0)
    assert len(set(CASES)) == len(CASES)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_label_has_an_aligned_and_a_ragged_case(dtype):
    for label in sorted({c.expected_label for c in CASES if c.dtype == dtype} - {"conv_direct"}):
        mine = [c for c in CASES if c.dtype == dtype and c.expected_label == label]
        assert any(c.B == 1 and c.M % 32 == 0 and c.N % 32 == 0 and c.stride == 1 and c.up == 1 for c in mine), f"{dtype} {label}: no aligned case"
        ragged = [c for c in mine if c.B >= 2 and c.L % 32 and c.M % 32 and c.taps == 3 and c.residual and c.stride == 1 and c.up == 1]
        assert ragged, f"{dtype} {label}: no ragged case"
        # families that take whole column tiles only: the register-staged kernel (N % 32 == 0, conv_gemm_rs_ok) and the 16-bit 128x64 macro
        # tile (every rule of conv_gemm_mt_variant that picks it asks for N % 64 == 0)
        if "conv_gemm_rs" not in label and "128x64,2wg" not in label:
            assert any(c.N % 32 for c in ragged), f"{dtype} {label}: no partial column tile"


def test_reference_against_torch_conv1d():
    """conv1d_ref's gather-and-multiply form against F.interpolate + F.conv1d in fp64, on every geometry kind of the table."""
    g = torch.Generator().manual_seed(3)
    for B, L, Cc, N, taps, stride, pad, up in ((2, 37, 8, 5, 3, 1, 1, 1), (3, 3, 4, 6, 3, 1, 1, 1), (4, 1, 4, 6, 3, 1, 1, 1), (2, 22, 8, 3, 3, 1, 1, 4),
                                               (2, 45, 2, 8, 9, 4, 4, 1), (2, 40, 8, 8, 5, 2, 2, 1), (2, 19, 8, 8, 3, 1, 1, 2), (2, 33, 8, 8, 1, 1, 0, 1)):
        x, w, b = torch.randn(B, L, Cc, generator=g).double(), torch.randn(N, Cc, taps, generator=g).double(), torch.randn(N, generator=g).double()
        h = x.transpose(1, 2)
        if up > 1:
            h = torch.nn.functional.interpolate(h, scale_factor=up, mode="nearest")
        want = torch.nn.functional.conv1d(h, w, b, stride=stride, padding=pad).transpose(1, 2)
        res = torch.randn(want.shape, generator=g).double()
        ref, A = R.conv1d_ref(x, w, b, res, taps, stride, pad, up)
        assert ref.shape == want.shape and float((ref - want - res).abs().max()) < 1e-12
        wantA = torch.nn.functional.conv1d(h.abs(), w.abs(), b.abs(), stride=stride, padding=pad).transpose(1, 2) + res.abs()
        assert float((A - wantA).abs().max()) < 1e-12


def test_gamma_forms():
    assert R.gamma(96, "fp32", "conv_gemm<f32,64x64>") == 99 * 2.0 ** -24 == R.gamma(96, "bf16", "conv_direct")
    assert R.gamma(96, "fp16", "conv_gemm_rs<f16,32x32>") == 2 * 99 * 2.0 ** -24
    assert R.gamma(96, "fp32x", "conv_gemm<f32,64x64>") == R.gamma(96, "fp32", "conv_gemm<f32,64x64>")          # multiplies in fp32
    extra = (R.gamma(1024, "fp32x", "conv_gemm_rs<x3,32x32>") - 1027 * 2.0 ** -24) / 2.0 ** -22
    assert abs(extra - (1027 / 4 + 3 + 1 / 64 + 1027 / 512)) < 1e-9


@pytest.mark.parametrize("dtype", DTYPES)
def test_emulated_cases_pass_the_gate(dtype):
    worst, worst_acc = 0.0, 0.0
    for c in (c for c in CASES if c.dtype == dtype):
        ops = R.operands(c)
        ref, A = R.case_ref(c, ops)
        y32 = R.case_emulate(c, ops, stored=False)
        r, _ = R.gate(R.round_to(y32, R.STORE[dtype]), ref, A, c.K, dtype, c.expected_label, case_id(c), quiet=True)
        acc = float(((y32.double() - ref).abs() / (R.gamma(c.K, dtype, c.expected_label) * A)).max())
        assert acc <= 0.5, f"{case_id(c)} [{c.expected_label}]: the fp32 accumulation uses {acc:.3f} of gamma A"
        worst, worst_acc = max(worst, r), max(worst_acc, acc)
    print(f"{dtype}: largest err/bound of the emulated cases {worst:.3f}, largest accumulation part {worst_acc:.3f}")
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# c. planted faults
# ---------------------------------------------------------------------------------------------------------------------------------
_cache = {}


def _prepared(c):
    """(ops, ref, A, y32) of a case; the last one is kept (the faults of one dtype mostly share a case)."""
    if _cache.get("case") != c:
        ops = R.operands(c)
        ref, A = R.case_ref(c, ops)
        _cache.update(case=c, val=(ops, ref, A, R.case_emulate(c, ops, stored=False)))
    return _cache["val"]


def _pick(dtype, pred):
    found = [c for c in CASES if c.dtype == dtype and pred(c)]
    assert found, f"no {dtype} case for this fault"
    return max(found, key=lambda c: c.M * c.N)


def _plain(c):
    return c.taps == 3 and c.stride == 1 and c.up == 1 and c.B >= 2 and c.residual


def _wm(c, ops):
    return R.weight_matrix(ops[2].float())                     # (K, N), k = tap * C + c


def fault_clip_boundary(c, ops, y):
    """tap -1 at position 0 of clip 1 (inside a row tile: Lout is no multiple of 32) reads clip 0's last row instead of zero; one tile's columns"""
    assert c.Lout % 32 and c.pad == 1
    y[1, 0, :32] += ops[0][0, c.L - 1] @ _wm(c, ops)[:c.C, :32]


def fault_last_k_step(c, ops, y):
    """the final 16-channel (16-bit MFMA) or 32-channel K step is dropped in the ragged last row tile; one tile's columns"""
    rows, ks = c.M % 32, 16 if c.dtype in ("bf16", "fp16") else 32
    assert rows and c.C % ks == 0
    g = R.gathered(ops[0][-1:].float(), c.taps, c.stride, c.pad, c.up)[0, c.Lout - rows:]
    y[-1, c.Lout - rows:, :32] -= g[:, c.K - ks:] @ _wm(c, ops)[c.K - ks:, :32]


def fault_no_residual(c, ops, y):
    """one 32x32 tile is stored without the residual"""
    y[0, 32:64, 32:64] -= ops[4][0, 32:64, 32:64]


def fault_column_tile_row_off(c, ops, y):
    """the partial column tile (columns 256-319 of 320) is written one row off, in the ragged last row tile"""
    rows = c.M % 32
    assert c.N == 320 and 0 < rows < c.Lout
    y[-1, c.Lout - rows:, 256:] = y[-1, c.Lout - rows - 1:c.Lout - 1, 256:].clone()


def fault_upsample_index(c, ops, y):
    """with up = 2 the source index l >> 1 is off by one, in the ragged last row tile; one tile's columns"""
    rows = c.M % 32
    assert c.up == 2 and rows
    x = ops[0][-1:].float()
    shifted = torch.cat([x[:, 1:], x[:, -1:]], 1)               # row (l >> 1) + 1, clamped at the clip's end
    d = (R.gathered(shifted, c.taps, c.stride, c.pad, c.up) - R.gathered(x, c.taps, c.stride, c.pad, c.up))[0, c.Lout - rows:]
    y[-1, c.Lout - rows:, :32] += d @ _wm(c, ops)[:, :32]


def fault_stride_padding(c, ops, y):
    """with stride = 2 the last output position's last tap reads row L - 1 where the padding belongs; one tile's columns"""
    t = c.taps - 1
    assert c.stride == 2 and (c.Lout - 1) * 2 - c.pad + t == c.L       # that tap is the first padding row
    y[0, c.Lout - 1, :32] += ops[0][0, c.L - 1] @ _wm(c, ops)[t * c.C:, :32]


FAULTS = {
    "clip_boundary": (fault_clip_boundary, lambda c: _plain(c) and c.N == 320 and c.M % 32 == 2),
    "last_k_step": (fault_last_k_step, lambda c: _plain(c) and c.N == 320 and c.M % 32 == 2),
    "no_residual": (fault_no_residual, lambda c: _plain(c) and c.N == 320 and c.M % 32 == 2),
    "column_tile_row_off": (fault_column_tile_row_off, lambda c: _plain(c) and c.N == 320 and c.M % 32 == 2),
    "upsample_index": (fault_upsample_index, lambda c: c.up == 2 and c.taps == 3 and c.residual and c.M % 32 and c.N >= 32),
    "stride_padding": (fault_stride_padding, lambda c: c.stride == 2 and c.taps == 5 and c.C % 32 == 0),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_fault_fails_the_gate(dtype, fault):
    plant, pred = FAULTS[fault]
    c = _pick(dtype, pred)
    ops, ref, A, y32 = _prepared(c)
    y = y32.clone()
    plant(c, ops, y)
    bad = R.round_to(y, R.STORE[dtype])
    changed = int((bad != R.round_to(y32, R.STORE[dtype])).sum())
    assert 0 < changed <= 2048, changed                                        # one tile (32 x 64 for the partial column tile) at the most
    with pytest.raises(AssertionError, match="over the bound") as e:
        R.gate(bad, ref, A, c.K, dtype, c.expected_label, f"{fault} in {case_id(c)}", quiet=True)
    assert c.expected_label in str(e.value) and "(clip " in str(e.value)
    rel = R.rel_l2(bad, ref)
    print(f"{dtype} {fault} in {case_id(c)}: {changed} elements changed, whole-tensor rel-L2 {rel:.3e}" + (f" (older gate {TOL[dtype]:.0e})" if dtype in ("bf16", "fp16") else ""))
    if dtype in ("bf16", "fp16"):
        assert rel < TOL[dtype], f"{fault}: rel-L2 {rel:.3e} -- the older gate would have caught this one"


def test_planted_fault_split_tile_without_lo_accumulator():
    """fp32x: one tile -- the ragged last row tile, 32 columns of it -- computed from accM alone (the lo' accumulator lost) fails the gate
    while the whole tensor passes the 1e-6 rel-L2 of test_conv_gemm_fp32x_against_fp64.  (A lost lo' costs 2^-12 of an element's
    magnitude: a full 32x32 tile of it stays below 1e-6 only from 6e7 outputs on, so the tile with the fewest rows carries it.)"""
    c = _pick("fp32x", lambda c: R.is_split(c.expected_label) and _plain(c))
    rows = c.M % 32
    assert 0 < rows <= 2
    ops, ref, A, y32 = _prepared(c)
    x, _, w_op, _, _ = ops
    _, accL = R.emulate(x[-1:, c.L - 40:], w_op[32:64], None, None, c.taps, c.stride, c.pad, c.up, "fp32x", c.expected_label, parts=True)
    y = y32.clone()
    y[-1, c.Lout - rows:, 32:64] -= (accL * (1.0 / 2048.0))[0, 40 - rows:]
    with pytest.raises(AssertionError, match="over the bound"):
        R.gate(y, ref, A, c.K, "fp32x", c.expected_label, f"no lo' accumulator in {case_id(c)}", quiet=True)
    rel = R.rel_l2(y, ref)
    print(f"fp32x tile without the lo' accumulator in {case_id(c)}: whole-tensor rel-L2 {rel:.3e} (older gate 1e-6)")
    assert rel < 1e-6
