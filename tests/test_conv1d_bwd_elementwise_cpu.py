"""CPU half of the element-wise gates on the conv1d training backward (conv1d_bwd_ref.py, test_gpu_conv1d_bwd_elementwise.py): no GPU needed.

  a. Coverage is pinned.  sf_op_conv1d_bwd_variant (a query: nothing is launched) is swept over the channel counts, tap counts and lengths the
     U-Net and the tables use.  The set of (weight-gradient kernel / staging, reducer, column-sum kernel) it returns must EQUAL the literal
     WGRAD_KEYS, the set of data-gradient labels the literal DGRAD_LABELS, and every member of either must be the expected label of a case of
     the exact-gate table that asks for that output: a path that becomes reachable fails here until it has a case.  Every row's literal label
     is what the query returns for it.
  b. The emulation of every case passes its gate; for the rounding gate it uses at most half the bound (the bound does not sit on the
     arithmetic's floor), and every exact case has max A < 2^24 (its partial sums are exact in fp32).
  c. Planted faults in the emulation fail the gates.  Next to each, the whole-tensor rel-L2 says whether the 2e-5 gate of test_gpu_train.py
     would have caught it too (printed: information, not a requirement).
"""
import ctypes as C

import pytest
import torch

import conv1d_bwd_ref as R
from conv1d_bwd_ref import Case, case_id
from test_gpu_conv1d_bwd_elementwise import EXACT_CASES, ROUNDING_CASES

MODES = ("fp32", "fp32x")
GRID_CH = (1, 2, 6, 8, 16, 17, 32, 33, 40, 64, 66, 68, 96, 128, 132, 160, 192, 256, 512)
GRID_TAPS = (1, 3, 5, 7, 9)
GRID_BL = ((1, 33), (3, 31), (2, 300), (2, 520), (2, 1050), (2, 2100), (2, 8200), (2, 9000))

WGRAD_KEYS = {
    "fp32": {
        "wgrad_lds<1>/rows direct | db generic",
        "wgrad_lds<1>/rows direct | db vec4",
        "wgrad_lds<1>/rows scalar | db generic",
        "wgrad_lds<1>/rows scalar | db vec4",
        "wgrad_lds<1>/rows vec | db generic",
        "wgrad_lds<1>/rows vec | db vec4",
        "wgrad_lds<1>/tap direct | db generic",
        "wgrad_lds<1>/tap direct | db vec4",
        "wgrad_lds<1>/tap scalar | db generic",
        "wgrad_lds<1>/tap scalar | db vec4",
        "wgrad_lds<1>/tap vec | db generic",
        "wgrad_lds<1>/tap vec | db vec4",
        "wgrad_lds<2>/rows direct | db generic",
        "wgrad_lds<2>/rows direct | db vec4",
        "wgrad_lds<2>/rows scalar | db generic",
        "wgrad_lds<2>/rows scalar | db vec4",
        "wgrad_lds<2>/rows vec | db generic",
        "wgrad_lds<2>/rows vec | db vec4",
        "wgrad_lds<2>/tap direct | db generic",
        "wgrad_lds<2>/tap direct | db vec4",
        "wgrad_lds<2>/tap scalar | db generic",
        "wgrad_lds<2>/tap scalar | db vec4",
        "wgrad_lds<2>/tap vec | db generic",
        "wgrad_lds<2>/tap vec | db vec4",
        "wgrad_thin<1,1> direct | db generic",
        "wgrad_thin<1,1> direct | db vec1",
        "wgrad_thin<1,1> direct | db vec4",
        "wgrad_thin<1,1> scalar | db generic",
        "wgrad_thin<1,1> scalar | db vec1",
        "wgrad_thin<1,1> scalar | db vec4",
        "wgrad_thin<1,1> vec | db generic",
        "wgrad_thin<1,1> vec | db vec1",
        "wgrad_thin<1,1> vec | db vec4",
        "wgrad_thin<1,2> direct | db generic",
        "wgrad_thin<1,2> direct | db vec1",
        "wgrad_thin<1,2> direct | db vec4",
        "wgrad_thin<1,2> scalar | db generic",
        "wgrad_thin<1,2> scalar | db vec1",
        "wgrad_thin<1,2> scalar | db vec4",
        "wgrad_thin<1,2> vec | db generic",
        "wgrad_thin<1,2> vec | db vec1",
        "wgrad_thin<1,2> vec | db vec4",
        "wgrad_thin<1,3> direct | db generic",
        "wgrad_thin<1,3> direct | db vec1",
        "wgrad_thin<1,3> direct | db vec4",
        "wgrad_thin<1,3> scalar | db generic",
        "wgrad_thin<1,3> scalar | db vec1",
        "wgrad_thin<1,3> scalar | db vec4",
        "wgrad_thin<1,3> vec | db generic",
        "wgrad_thin<1,3> vec | db vec1",
        "wgrad_thin<1,3> vec | db vec4",
    },
    "fp32x": {
        "wgrad_thin<1,1> direct | db generic",
        "wgrad_thin<1,1> direct | db vec1",
        "wgrad_thin<1,1> direct | db vec4",
        "wgrad_thin<1,1> scalar | db generic",
        "wgrad_thin<1,1> scalar | db vec1",
        "wgrad_thin<1,1> scalar | db vec4",
        "wgrad_thin<1,1> vec | db generic",
        "wgrad_thin<1,1> vec | db vec1",
        "wgrad_thin<1,1> vec | db vec4",
        "wgrad_thin<1,2> direct | db generic",
        "wgrad_thin<1,2> direct | db vec1",
        "wgrad_thin<1,2> direct | db vec4",
        "wgrad_thin<1,2> scalar | db generic",
        "wgrad_thin<1,2> scalar | db vec1",
        "wgrad_thin<1,2> scalar | db vec4",
        "wgrad_thin<1,2> vec | db generic",
        "wgrad_thin<1,2> vec | db vec1",
        "wgrad_thin<1,2> vec | db vec4",
        "wgrad_thin<1,3> direct | db generic",
        "wgrad_thin<1,3> direct | db vec1",
        "wgrad_thin<1,3> direct | db vec4",
        "wgrad_thin<1,3> scalar | db generic",
        "wgrad_thin<1,3> scalar | db vec1",
        "wgrad_thin<1,3> scalar | db vec4",
        "wgrad_thin<1,3> vec | db generic",
        "wgrad_thin<1,3> vec | db vec1",
        "wgrad_thin<1,3> vec | db vec4",
        "wgrad_x3<1>/rows direct | db generic",
        "wgrad_x3<1>/rows direct | db vec4",
        "wgrad_x3<1>/rows scalar | db generic",
        "wgrad_x3<1>/rows scalar | db vec4",
        "wgrad_x3<1>/rows vec | db generic",
        "wgrad_x3<1>/rows vec | db vec4",
        "wgrad_x3<1>/tap direct | db generic",
        "wgrad_x3<1>/tap direct | db vec4",
        "wgrad_x3<1>/tap scalar | db generic",
        "wgrad_x3<1>/tap scalar | db vec4",
        "wgrad_x3<1>/tap vec | db generic",
        "wgrad_x3<1>/tap vec | db vec4",
        "wgrad_x3<2>/rows direct | db generic",
        "wgrad_x3<2>/rows direct | db vec4",
        "wgrad_x3<2>/rows scalar | db generic",
        "wgrad_x3<2>/rows scalar | db vec4",
        "wgrad_x3<2>/rows vec | db generic",
        "wgrad_x3<2>/rows vec | db vec4",
        "wgrad_x3<2>/tap direct | db generic",
        "wgrad_x3<2>/tap direct | db vec4",
        "wgrad_x3<2>/tap scalar | db generic",
        "wgrad_x3<2>/tap scalar | db vec4",
        "wgrad_x3<2>/tap vec | db generic",
        "wgrad_x3<2>/tap vec | db vec4",
    },
}
DGRAD_LABELS = {
    "fp32": {"conv_direct", "conv_gemm<f32,128x128>", "conv_gemm<f32,128x32>", "conv_gemm<f32,128x64>", "conv_gemm<f32,64x64>", "conv_gemm_fast<f32,32x32>", "conv_gemm_mt<f32>", "conv_gemm_sk<f32,32x32>", "conv_gemm_v2<f32,128x128>", "conv_gemm_v2<f32,64x64>", "conv_gemm_wp<f32,32x32>", "refused"},
    "fp32x": {"conv_direct", "conv_gemm<f32,128x128>", "conv_gemm<f32,128x32>", "conv_gemm<f32,128x64>", "conv_gemm<f32,64x64>", "conv_gemm_fast<x3,32x32>", "conv_gemm_mt<x3>", "conv_gemm_sk<f32,32x32>", "conv_gemm_v2<f32,128x128>", "conv_gemm_v2<f32,64x64>", "conv_gemm_wp<x3,32x32>", "refused"},
}


def _query(mode, B, L, Cc, N, taps):
    from syncfusion_amd import _lib

    lib = _lib.load()
    buf = C.create_string_buffer(160)
    rc = lib.sf_op_conv1d_bwd_variant(_lib.DTYPES[mode], B, L, Cc, N, taps, (taps - 1) // 2, buf, 160)
    return rc, buf.value.decode()


@pytest.mark.parametrize("mode", MODES)
def test_plan_sweep_equals_the_pinned_sets_and_the_tables_reach_them(mode):
    wkeys, dlabels = set(), set()
    for Cc in GRID_CH:
        for N in GRID_CH:
            for taps in GRID_TAPS:
                for B, L in GRID_BL:
                    rc, label = _query(mode, B, L, Cc, N, taps)
                    assert rc == 0, (mode, B, L, Cc, N, taps)
                    p = R.parse(label)
                    wkeys.add(p.wgrad_key)
                    dlabels.add(p.dgrad)
    assert wkeys == WGRAD_KEYS[mode], f"{mode}: reachable and not pinned {sorted(wkeys - WGRAD_KEYS[mode])}; pinned and not reached {sorted(WGRAD_KEYS[mode] - wkeys)}"
    assert dlabels == DGRAD_LABELS[mode], f"{mode}: reachable and not pinned {sorted(dlabels - DGRAD_LABELS[mode])}; pinned and not reached {sorted(DGRAD_LABELS[mode] - dlabels)}"
    mine = [c for c in EXACT_CASES if c.mode == mode]
    have_w = {R.parse(c.expected_label).wgrad_key for c in mine if "w" in c.outs and "b" in c.outs}
    assert WGRAD_KEYS[mode] <= have_w, f"{mode}: no exact case for {sorted(WGRAD_KEYS[mode] - have_w)}"
    have_d = {R.parse(c.expected_label).dgrad for c in mine if "x" in c.outs} | {"refused"}
    assert DGRAD_LABELS[mode] <= have_d, f"{mode}: no exact case for the data gradient through {sorted(DGRAD_LABELS[mode] - have_d)}"
    assert any(R.parse(c.expected_label).dgrad == "refused" and "x" not in c.outs for c in mine)
    rounded = [c for c in ROUNDING_CASES if c.mode == mode]
    kernels = {R.parse(c.expected_label).wgrad for c in rounded if "w" in c.outs}
    assert {k.split(" ")[0] for k in WGRAD_KEYS[mode]} <= kernels, f"{mode}: the rounding table misses a weight-gradient kernel / staging"
    assert DGRAD_LABELS[mode] - {"refused"} <= {R.parse(c.expected_label).dgrad for c in rounded if "x" in c.outs}
    assert any(R.parse(c.expected_label).S > 1 for c in rounded if "w" in c.outs)


def test_fp32x_tables_reach_the_split_kernels():
    for table in (EXACT_CASES, ROUNDING_CASES):
        plans = [R.parse(c.expected_label) for c in table if c.mode == "fp32x"]
        assert {p.wgrad for p in plans} >= {f"wgrad_x3<{tw}>/{st}" for tw in (1, 2) for st in ("tap", "rows")}
        assert any(R.dgrad_split(p) for p in plans) and any(not R.dgrad_split(p) and p.dgrad.startswith("conv_gemm") for p in plans)
    scaled = {(R.parse(c.expected_label).wgrad, c.dy_scale) for c in ROUNDING_CASES if c.dy_scale != 1.0}
    assert scaled == {(f"wgrad_x3<{tw}>/{st}", s) for tw in (1, 2) for st in ("tap", "rows") for s in (1e-9, 1e6)}


def test_every_case_names_the_plan_it_reaches():
    for c in EXACT_CASES + ROUNDING_CASES:
        rc, label = _query(c.mode, c.B, c.L, c.C, c.N, c.taps)
        assert rc == 0 and label == c.expected_label, f"{case_id(c)}: the dispatcher plans {label!r}, the row says {c.expected_label!r}"
        p = R.parse(label)
        assert c.outs and set(c.outs) <= set("xwb") and ("x" not in c.outs or p.dgrad != "refused"), case_id(c)
        fam, S, rps, empty, reducer = R.plan(*c.shape)                        # the restated dispatch agrees with the label it only describes
        assert (S, reducer) == (p.S, p.reducer), case_id(c)
    assert len(set(EXACT_CASES)) == len(EXACT_CASES) and len(set(ROUNDING_CASES)) == len(ROUNDING_CASES)
    # the cases the table is there for: slices without rows on both reducers, S >= 64 on a small matrix
    for mode in MODES:
        empties = {R.parse(c.expected_label).reducer for c in EXACT_CASES if c.mode == mode and R.plan(*c.shape)[3] > 0}
        assert empties == {"vec", "scalar"}, (mode, empties)


def test_references_against_autograd():
    """The gather-and-multiply references against torch's own conv1d backward in fp64."""
    g = torch.Generator().manual_seed(5)
    for B, L, Cc, N, taps in ((2, 37, 8, 5, 3), (3, 2, 4, 6, 9), (4, 1, 4, 6, 3), (2, 19, 6, 8, 5), (2, 33, 8, 8, 1), (1, 40, 3, 2, 7)):
        pad = (taps - 1) // 2
        dy = torch.randn(B, L, N, generator=g).double()
        with torch.enable_grad():
            x = torch.randn(B, L, Cc, generator=g).double().requires_grad_()
            w = torch.randn(N, Cc, taps, generator=g).double().requires_grad_()
            b = torch.zeros(N).double().requires_grad_()
            torch.nn.functional.conv1d(x.transpose(1, 2), w, b, padding=pad).transpose(1, 2).backward(dy)
        dw, _ = R.wgrad_ref(x.detach(), dy, taps, pad)
        dx, _ = R.dgrad_ref(dy, w.detach(), taps, pad)
        db, _ = R.db_ref(dy)
        assert float((dw - w.grad).abs().max()) < 1e-12 and float((dx - x.grad).abs().max()) < 1e-12 and float((db - b.grad).abs().max()) < 1e-12


def test_gamma_forms():
    c = Case("fp32", 2, 600, 32, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/rows S=4 vec | db vec4 Sb=4")
    p = R.parse(c.expected_label)
    assert R.gamma_dw(c, p) == (1200 + 4 + 6) * 2.0 ** -24 and R.gamma_db(c, p) == 1201 * 2.0 ** -24 and R.gamma_dx(c, p) == (192 + 3) * 2.0 ** -24
    cx = c._replace(mode="fp32x", expected_label="dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<1>/rows S=4 vec | db vec4 Sb=4")
    px = R.parse(cx.expected_label)
    assert abs(R.gamma_dw(cx, px) - ((3 + 2.0 ** -7) * 2.0 ** -18 + (6 * 1200 * (1 + 2.0 ** -6) + 10) * 2.0 ** -24)) < 1e-18
    assert abs(R.gamma_dx(cx, px) - ((3 + 2.0 ** -7) * 2.0 ** -18 + (6 * 192 * (1 + 2.0 ** -6) + 3) * 2.0 ** -24)) < 1e-18
    # fp32x without a split kernel: the fp32 gamma
    ct = c._replace(mode="fp32x", expected_label="dgrad conv_gemm<f32,128x32> | wgrad_thin<1,3> S=4 vec | db vec4 Sb=4")
    assert R.gamma_dw(ct, R.parse(ct.expected_label)) == R.gamma_dw(c, p) and R.gamma_dx(ct, R.parse(ct.expected_label)) == R.gamma_dx(c, p)


@pytest.mark.parametrize("mode", MODES)
def test_emulated_exact_cases_are_bit_equal(mode):
    for c in (c for c in EXACT_CASES if c.mode == mode):
        ops = R.exact_operands(c)
        emu = R.emulate(c, ops)
        for which, (ref, A) in R.references(c, ops).items():
            assert float(A.max()) < 2.0 ** 24, f"{case_id(c)} {which}: max A {float(A.max()):.4g}"
            R.exact_gate(emu[which], ref, A, which, case_id(c), c.expected_label)


@pytest.mark.parametrize("mode", MODES)
def test_emulated_rounding_cases_use_at_most_half_the_bound(mode):
    worst = {}
    for c in (c for c in ROUNDING_CASES if c.mode == mode):
        ops = R.operands(c)
        p = R.parse(c.expected_label)
        emu, gam = R.emulate(c, ops, p), R.gammas(c, p)
        for which, (ref, A) in R.references(c, ops).items():
            r = R.rounding_gate(emu[which], ref, A, gam[which], which, case_id(c), c.expected_label)
            assert r <= 0.5, f"{case_id(c)} {which} [{c.expected_label}]: the emulation uses {r:.3f} of the bound"
            worst[which] = max(worst.get(which, 0.0), r)
    print(f"{mode}: largest err/bound of the emulated cases: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


# ---------------------------------------------------------------------------------------------------------------------------------
# c. planted faults
# ---------------------------------------------------------------------------------------------------------------------------------
def _case(table, mode, shape, outs="xwb"):
    found = [c for c in table if c.mode == mode and c.shape == shape and c.outs == outs and c.dy_scale == 1.0]
    assert len(found) == 1, (mode, shape, outs)
    return found[0]


def _wgrad_setup(c, exact):
    ops = R.exact_operands(c) if exact else R.operands(c)
    x, _, dy = ops
    p = R.parse(c.expected_label)
    part = R.emulate_wgrad_partials(x, dy, c.taps, c.pad, p.S, c.mode == "fp32x" and R.wgrad_split(p))
    ref, A = R.wgrad_ref(x, dy, c.taps, c.pad)
    good = R.reduce_partials(part, c.C, c.taps)
    return ops, p, part, ref, A, good


def _must_fail(c, exact, bad, ref, A, which, what, match):
    p = R.parse(c.expected_label)
    with pytest.raises(AssertionError, match=match) as e:
        if exact:
            R.exact_gate(bad, ref, A, which, what, c.expected_label)
        else:
            R.rounding_gate(bad, ref, A, R.gammas(c, p)[which], which, what, c.expected_label)
    assert c.expected_label in str(e.value)
    finite = torch.isfinite(bad)
    rel = R.rel_l2(torch.where(finite, bad, torch.zeros_like(bad)), ref) if not bool(finite.all()) else R.rel_l2(bad, ref)
    old = "not finite: caught" if not bool(finite.all()) else ("caught" if rel > R.OLD_REL_L2 else "MISSED")
    print(f"{what} [{'exact' if exact else 'rounding'} gate, {case_id(c)}]: {int((bad.double() != ref).sum())} of {bad.numel()} elements differ, whole-tensor rel-L2 "
          f"{rel:.3e} -- the 2e-5 gate: {old}")


SPLIT_SHAPE = (2, 8200, 32, 64, 3)        # S = 64, 7 trailing slices without rows (exact table)
WHOLE_ROWS = (5, 333, 32, 64, 3)          # S = 6, clip boundaries inside chunks (both tables)
DIRECT = (3, 31, 64, 64, 3)               # S = 1: the kernel writes dw itself (both tables)


@pytest.mark.parametrize("exact", (True, False), ids=("exact", "rounding"))
@pytest.mark.parametrize("mode", MODES)
def test_fault_one_row_dropped_from_one_slice(mode, exact):
    c = _case(EXACT_CASES if exact else ROUNDING_CASES, mode, SPLIT_SHAPE if exact else WHOLE_ROWS)
    ops, p, part, ref, A, good = _wgrad_setup(c, exact)
    s = p.S // 2
    r = s * R.rows_per_slice(c.rows, p.S) + 5
    g = R.gathered(ops[0].float(), c.taps, 1, c.pad, 1).reshape(c.rows, -1)
    part[s] -= torch.outer(ops[2].reshape(c.rows, -1)[r], g[r])
    _must_fail(c, exact, R.reduce_partials(part, c.C, c.taps), ref, A, "dw", f"row {r} dropped from slice {s}", "differ from the exact" if exact else "over the bound")


@pytest.mark.parametrize("mode", MODES)
def test_fault_empty_trailing_slice_left_as_poison(mode):
    c = _case(EXACT_CASES, mode, SPLIT_SHAPE)
    ops, p, part, ref, A, good = _wgrad_setup(c, True)
    assert R.plan(*c.shape)[3] >= 1 and float(part[-1].abs().max()) == 0.0          # the last slice owns no rows: a correct kernel writes zeros
    part[-1] = float("nan")                                                          # 0xFF workspace bytes read as fp32
    bad = R.reduce_partials(part, c.C, c.taps)
    _must_fail(c, True, bad, ref, A, "dw", "last slice left unwritten", "non-finite")
    with pytest.raises(AssertionError, match="non-finite"):
        R.rounding_gate(bad, ref, A, 1.0, "dw", "last slice left unwritten", c.expected_label)


@pytest.mark.parametrize("exact", (True, False), ids=("exact", "rounding"))
@pytest.mark.parametrize("mode", MODES)
def test_fault_clip_mask_skipped_for_one_tap_at_one_boundary(mode, exact):
    c = _case(EXACT_CASES if exact else ROUNDING_CASES, mode, WHOLE_ROWS)
    ops, p, part, ref, A, good = _wgrad_setup(c, exact)
    r = c.L                                                                          # position 0 of clip 1, inside a 32-row chunk (L % 32 != 0)
    assert c.L % 32 and c.pad == 1
    s = r // R.rows_per_slice(c.rows, p.S)
    # tap 0 reads row r - 1, the last row of clip 0, where the padding belongs: columns q = 0 ... C - 1
    part[s][:, :c.C] += torch.outer(ops[2].reshape(c.rows, -1)[r], ops[0].reshape(c.rows, -1)[r - 1])
    _must_fail(c, exact, R.reduce_partials(part, c.C, c.taps), ref, A, "dw", "clip mask skipped for tap 0 at the first row of clip 1",
               "differ from the exact" if exact else "over the bound")


@pytest.mark.parametrize("exact", (True, False), ids=("exact", "rounding"))
@pytest.mark.parametrize("mode", MODES)
def test_fault_one_tile_zeroed(mode, exact):
    c = _case(EXACT_CASES if exact else ROUNDING_CASES, mode, WHOLE_ROWS)
    ops, p, part, ref, A, good = _wgrad_setup(c, exact)
    part[:, 32:64, 32:64] = 0.0
    _must_fail(c, exact, R.reduce_partials(part, c.C, c.taps), ref, A, "dw", "one 32x32 tile zeroed", "differ from the exact" if exact else "over the bound")


@pytest.mark.parametrize("exact", (True, False), ids=("exact", "rounding"))
@pytest.mark.parametrize("mode", MODES)
def test_fault_direct_store_in_the_partial_layout(mode, exact):
    c = _case(EXACT_CASES if exact else ROUNDING_CASES, mode, DIRECT)
    ops, p, part, ref, A, good = _wgrad_setup(c, exact)
    assert p.S == 1 and p.reducer == "direct"
    bad = part[0].reshape(c.N, c.C, c.taps).clone()                                  # [n][t][c] written where [n][c][t] belongs
    _must_fail(c, exact, bad, ref, A, "dw", "dw stored as [n][t][c]", "differ from the exact" if exact else "over the bound")


@pytest.mark.parametrize("exact", (True, False), ids=("exact", "rounding"))
@pytest.mark.parametrize("mode", MODES)
def test_fault_dgrad_taps_not_flipped(mode, exact):
    c = _case(EXACT_CASES if exact else ROUNDING_CASES, mode, (2, 600, 32, 64, 9))    # fp32x: a data-gradient label with "<x3"
    ops = R.exact_operands(c) if exact else R.operands(c)
    p = R.parse(c.expected_label)
    assert mode == "fp32" or R.dgrad_split(p)
    ref, A = R.dgrad_ref(ops[2], ops[1], c.taps, c.pad)
    bad = R.emulate_dx(ops[2], ops[1], c.taps, c.pad, c.mode == "fp32x" and R.dgrad_split(p), flip=False)
    _must_fail(c, exact, bad, ref, A, "dx", "data-gradient taps not flipped", "differ from the exact" if exact else "over the bound")


def test_fault_split_product_dropped():
    """fp32x: the lo_a hi_b product of the split lost in the whole weight gradient.  The rounding gate catches it on a short reduction (the
    accumulation part of the bound grows with the rows, the lost product's sum only with their square root).  The exact gate cannot, by
    construction: the split of a small integer has lo = 0, so the lost product is zero -- asserted here so that nobody relies on it."""
    c = _case(ROUNDING_CASES, "fp32x", (1, 33, 64, 64, 3))
    p = R.parse(c.expected_label)
    assert R.wgrad_split(p)
    x, _, dy = R.operands(c)
    ref, A = R.wgrad_ref(x, dy, c.taps, c.pad)
    bad = R.reduce_partials(R.emulate_wgrad_partials(x, dy, c.taps, c.pad, p.S, True, drop_lo_hi=True), c.C, c.taps)
    _must_fail(c, False, bad, ref, A, "dw", "lo hi product of the split dropped", "over the bound")
    ce = _case(EXACT_CASES, "fp32x", (1, 33, 64, 64, 3))
    xe, _, dye = R.exact_operands(ce)
    refe, Ae = R.wgrad_ref(xe, dye, ce.taps, ce.pad)
    same = R.reduce_partials(R.emulate_wgrad_partials(xe, dye, ce.taps, ce.pad, 1, True, drop_lo_hi=True), ce.C, ce.taps)
    R.exact_gate(same, refe, Ae, "dw", "lo hi product dropped, integer operands", ce.expected_label)      # passes: nothing was lost
