"""CPU half of the gates on the shared GEMM epilogue (gemm_epilogue_ref.py, test_gpu_gemm_epilogue.py): no GPU needed.

  a. Every row of the GPU tables names the kernel family and the flags the dispatcher's plan gives it (the _variant queries launch nothing), and
     a sweep of the two queries pins the set of (label, rowpart, gnpart) triples reachable with the statistics armed: every triple the sweep
     reaches has a row, so a family that starts (or stops) honouring an output fails here until the table follows.
  b. The faithful fp32 emulation of row32_stats, gn_tile_stats, ln_pool_row / ln_fold, the operand transform and epi_values passes every gate on
     every case of the GPU tables with at least 3 x headroom (the two row gates, whose whole bounds are 6 and 10 roundings: 2 x).  For the
     values the headroom is measured on the fp32 value BEFORE the output
     rounding against the bound without its u_T |ref| term (one rounding to T uses that term up to 1 x by itself).
  c. Each planted fault fails its gate by at least 10 x on at least one case -- except "no_clamp", which changes no bit on any case
     (gemm_epilogue_ref.py, GNPART: the clamp cannot bite on finite data); that is asserted as bit identity.
"""
import pytest
import torch

import conv1d_ref as R
import gemm_epilogue_ref as E
from test_gpu_gemm_epilogue import CB_CASES, DTYPES, EPI_CASES, LN_CASES, cb_producer, epi_id, ln_id, ln_producer

HEADROOM = 1.0 / 3.0
# The two row gates have 6 and 10 units in all (five roundings of a depth-5 sum; 2 + 7 of the squares): over 10^4 rows the worst row of
# same-signed values reaches 2.3 of the 6, and a row that relu left with one dominant value 4.1 of the 10 (every rounding falls on the same
# term).  3 x headroom is not there to have; the bounds stay as derived and these two gates are held to 2 x.
HEADROOM_OF = {"rowpart.mean": 0.5, "rowpart.M2": 0.5}
MISS = 10.0


def test_every_row_names_the_kernel_and_flags_it_reaches():
    for c in EPI_CASES:
        got = E.query_epi(E.epi_desc(c, **E.epi_probe_ptrs(c)))
        assert got == (0, c.label, c.row, c.gn), f"{epi_id(c)}: the dispatcher gives {got}"
        assert c.K + 2 <= R.K_MAX and 2 * 2.0 * c.M * c.N * c.K / 1e9 <= 2.0, epi_id(c)
    for c in LN_CASES:
        rc, label, _ = E.query_ln(E.ln_desc(c, **E.ln_probe_ptrs(c)))
        assert (rc, label) == (0, c.label), f"{ln_id(c)}: the dispatcher gives {(rc, label)}"
        rc, label, row = E.query_ln(E.ln_desc(c, rowpart=E.PROBE, **E.ln_probe_ptrs(c)))
        assert (rc, label, row) == (0, c.label, c.N % 32 == 0), f"{ln_id(c)}: chaining the row partials moves the launch to {(rc, label, row)}"
        p = ln_producer(c)
        got = E.query_epi(E.epi_desc(p, **E.epi_probe_ptrs(p)))
        assert got == (0, p.label, True, False), f"{ln_id(c)}: the producer in front gives {got}"
    for dtype, shape, source in CB_CASES:
        p = cb_producer(dtype, shape)
        got = E.query_epi(E.epi_desc(p, **E.epi_probe_ptrs(p)))
        assert got == (0, p.label, False, True), f"conv_cb {dtype} {shape}: the producer in front gives {got}"
    assert len(set(EPI_CASES)) == len(EPI_CASES) and len(set(LN_CASES)) == len(LN_CASES)
    assert len(EPI_CASES) == 300 and len(LN_CASES) == 44 and len(CB_CASES) == 18


@pytest.mark.parametrize("dtype", DTYPES)
def test_triple_sweep_is_covered_by_the_table(dtype):
    """(label, rowpart, gnpart) over a grid of 32x32-family shapes with both statistics armed, and the consumer's labels over a grid of its own."""
    seen = set()
    for Cc in (64, 96, 128, 256, 512, 1024):
        for taps in (1, 3):
            for N in (24, 32, 40, 64, 96):
                for B, L in ((1, 32), (4, 20), (5, 25), (7, 37), (3, 1877), (1, 5632)):
                    if taps * Cc > 3072:
                        continue
                    c = E.EpiCase("sweep", dtype, B, L, Cc, 0, N, taps, 1, taps // 2, 1, "br", 0, False, True, True, False, "", "", False, False)
                    rc, label, row, gn = E.query_epi(E.epi_desc(c, **E.epi_probe_ptrs(c)))
                    assert rc == 0, (dtype, B, L, Cc, N, taps)
                    if row or gn:
                        seen.add((label, row, gn))
    table = {(c.label, c.row, c.gn) for c in EPI_CASES if c.dtype == dtype and (c.row or c.gn) and "conv_gemm_mt" not in c.label}
    assert seen == table, f"{dtype}: reachable without a row {sorted(seen - table)}; rows no grid point reaches {sorted(table - seen)}"
    seen_ln = set()
    for Cc in (128, 256, 512, 1024):
        for N in (64, 96, 256):
            for form in ("acc", "ss", "plain"):
                c = E.LnCase("sweep", dtype, 3, 37, Cc, N, form, 0, "", "")
                rc, label, _ = E.query_ln(E.ln_desc(c, **E.ln_probe_ptrs(c)))
                assert rc == 0, (dtype, Cc, N, form)
                seen_ln.add((label, form == "acc"))
    table_ln = {(c.label, c.form == "acc") for c in LN_CASES if c.dtype == dtype}
    assert seen_ln == table_ln, f"{dtype}: consumer launches without a row {sorted(seen_ln - table_ln)}; rows not reached {sorted(table_ln - seen_ln)}"


def test_queries_refuse_what_no_kernel_takes():
    from syncfusion_amd import _lib as _l

    ok = E.EpiCase("q", "bf16", 2, 37, 256, 0, 64, 1, 1, 0, 1, "br", 0, False, True, True, False, "", "", False, False)
    for bad in (ok._replace(C=100), ok._replace(C2=32, taps=3, pad=1), ok._replace(act=4), ok._replace(up=3)):
        rc, _, _, _ = E.query_epi(E.epi_desc(bad, **E.epi_probe_ptrs(bad)))
        assert rc == 6, (bad, rc, _l.load().sf_last_error())                                  # SF_ERR_UNSUPPORTED
    ln = E.LnCase("q", "bf16", 3, 20, 256, 64, "acc", 0, "", "")                               # Lout < 32: no LayerNorm-consumer kernel
    assert E.query_ln(E.ln_desc(ln, **E.ln_probe_ptrs(ln)))[0] == 6
    ln3 = E.ln_desc(E.LnCase("q", "bf16", 3, 37, 256, 64, "acc", 0, "", ""), **E.ln_probe_ptrs(ln))
    ln3.taps, ln3.pad = 3, 1
    assert E.query_ln(ln3)[0] == 6


def test_reference_statistics_against_torch():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(74, 64, generator=g) * 3 + 1
    ref, _ = E.gnpart64(x, 37)
    for mt in range(3):
        for seg, (lo, hi) in enumerate(E.segments(74, 37, mt)):
            blk = x[mt * 32 + lo:mt * 32 + hi, 32:64].double()
            want = (float(blk.mean()), float(((blk - blk.mean()) ** 2).sum())) if hi > lo else (0.0, 0.0)
            assert abs(float(ref[mt, 1, seg, 0]) - want[0]) < 1e-12 and abs(float(ref[mt, 1, seg, 1]) - want[1]) < 1e-9
    assert E.segments(74, 37, 0) == ((0, 32), (32, 32)) and E.segments(74, 37, 1) == ((0, 5), (5, 32)) and E.segments(74, 37, 2) == ((0, 10), (10, 10))


_cache = {}


def _ref_of(c):
    if c not in _cache:
        o = E.epi_operands(c)
        _cache[c] = (o, E.epi_ref(c, o))
    return _cache[c]


@pytest.mark.parametrize("dtype", DTYPES)
def test_faithful_emulation_passes_every_gate_with_headroom(dtype):
    worst = {}
    for c in (c for c in EPI_CASES if c.dtype == dtype):
        o, (ref, bound, _) = _ref_of(c)
        stored = E.emulate_values(c, o)
        E.check(stored, ref, bound, epi_id(c) + " values")
        uT = E.U["fp32"] if c.out_f32 else E.U[R.STORE[c.dtype]]
        r = E.ratio_of(E.emulate_values(c, o, stored=False), ref, bound - uT * ref.abs())
        worst["values"] = max(worst.get("values", 0.0), r)
        if c.row or c.gn:
            s2 = stored.reshape(c.M, c.N)
            mean, m2 = E.emulate_row32(s2)
            got = E.check_stats(s2, torch.stack([mean, m2], -1) if c.row else None, E.emulate_gnpart(s2, c.Lout) if c.gn else None, c.Lout, epi_id(c))
            for k, v in got.items():
                worst[k] = max(worst.get(k, 0.0), v)
    for c in (c for c in LN_CASES if c.dtype == dtype):
        o = E.ln_operands(c)
        part, e_in, q_in = E.ln_inputs_direct(o["x"])
        ref, bound = E.ln_ref(c, o, o["x"], e_in, q_in, c.label)
        got = E.emulate_ln(c, o, o["x"], part, c.label)
        E.check(got, ref, bound, ln_id(c))
        # chained: the partials an emulated producer leaves for its own stored rows
        mean, m2 = E.emulate_row32(o["x"].reshape(c.M, c.C))
        e2, q2 = E.ln_inputs_chained(o["x"])
        ref2, bound2 = E.ln_ref(c, o, o["x"], e2, q2, c.label)
        E.check(E.emulate_ln(c, o, o["x"], torch.stack([mean, m2], -1), c.label), ref2, bound2, ln_id(c) + " chained")
    print(dtype, {k: round(v, 3) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= HEADROOM_OF.get(k, HEADROOM), f"{dtype}: the faithful emulation uses {v:.3f} of the {k} bound: the derivation is too tight or the emulation wrong"


GN_FAULTS = ("seg_plus", "seg_minus", "rows_past_M", "transposed", "swapped", "no_32d2")


@pytest.mark.parametrize("fault", GN_FAULTS)
def test_planted_gnpart_fault_is_caught(fault):
    best = 0.0
    for c in (c for c in EPI_CASES if c.gn and c.dtype in ("bf16", "fp32")):
        o, _ = _ref_of(c)
        s2 = E.emulate_values(c, o).reshape(c.M, c.N)
        got = E.check_stats(s2, None, E.emulate_gnpart(s2, c.Lout, fault), c.Lout, epi_id(c), assert_=False)
        best = max(best, max(got.values()))
    assert best >= MISS, f"{fault}: worst miss {best:.2f} x the bound: no case of the table sees it"


ADVERSARIAL_ROWS = [float.fromhex(h) for h in """0x1.7ae81a0000000p-4,
0x1.5be1300000000p+2,
0x1.5bbf6a0000000p+2,
0x1.5ba80a0000000p+2,
0x1.5b697a0000000p+2,
0x1.5bb5fc0000000p+2,
0x1.5bbdf80000000p+2,
0x1.5bc2880000000p+2,
0x1.5bf1e20000000p+2,
0x1.5b9fc80000000p+2,
0x1.5b77460000000p+2,
0x1.5b92c60000000p+2,
0x1.5b582a0000000p+2,
0x1.5bd48e0000000p+2,
0x1.5bde8e0000000p+2,
0x1.5ba5ec0000000p+2,
0x1.5b8a0e0000000p+2,
0x1.5bbdee0000000p+2,
0x1.5bad860000000p+2,
0x1.5bfc6c0000000p+2,
0x1.5bf50c0000000p+2,
0x1.5b61900000000p+2,
0x1.5b970e0000000p+2,
0x1.5b6d900000000p+2,
0x1.5b6abe0000000p+2,
0x1.5b87b60000000p+2,
0x1.5b75fe0000000p+2,
0x1.5bc8fa0000000p+2,
0x1.5bce320000000p+2,
0x1.5b767c0000000p+2,
0x1.5bb8800000000p+2,
0x1.5bf0c00000000p+2""".replace("\n", " ").split(", ")]


def test_adversarial_segment_stays_inside_the_candidate_bound():
    """The segment a greedy search built against the gnpart M2 bound: 32 constant rows, the first far from the rest (P ~ S), each later row
    mean picked among 24 neighbours so that the roundings of t1 and t2 push the result the same way.  It reaches about 0.6 of the issue's
    candidate bound, the most any emulated segment did; the worst-case term (2 k + 2) u P of the derivation is not needed."""
    x = torch.tensor(ADVERSARIAL_ROWS, dtype=torch.float32).reshape(32, 1).expand(32, 32).contiguous()
    got = E.check_stats(x, None, E.emulate_gnpart(x, 32), 32, "adversarial segment")
    print(got)
    assert 0.3 <= got["gnpart.M2"] <= 1.0


def test_clamp_is_not_load_bearing():
    for c in (c for c in EPI_CASES if c.gn and c.dtype in ("bf16", "fp32")):
        o, _ = _ref_of(c)
        s2 = E.emulate_values(c, o).reshape(c.M, c.N)
        assert torch.equal(E.emulate_gnpart(s2, c.Lout), E.emulate_gnpart(s2, c.Lout, "no_clamp")), epi_id(c)


@pytest.mark.parametrize("fault", ("bscale_after_res", "badd_by_row"))
def test_planted_value_fault_is_caught(fault):
    best = 0.0
    for c in (c for c in EPI_CASES if c.name in ("operands", "cat") and c.M <= 1000):
        o, (ref, bound, _) = _ref_of(c)
        best = max(best, E.ratio_of(E.emulate_values(c, o, fault), ref, bound))
    assert best >= MISS, f"{fault}: worst miss {best:.2f} x the bound"


@pytest.mark.parametrize("fault", ("mean_div_32", "cu_first_column"))
def test_planted_ln_fault_is_caught(fault):
    best = 0.0
    for c in (c for c in LN_CASES if c.form == "acc"):
        o = E.ln_operands(c)
        part, e_in, q_in = E.ln_inputs_direct(o["x"])
        ref, bound = E.ln_ref(c, o, o["x"], e_in, q_in, c.label)
        best = max(best, E.ratio_of(E.emulate_ln(c, o, o["x"], part, c.label, fault), ref, bound))
    assert best >= MISS, f"{fault}: worst miss {best:.2f} x the bound"


def test_every_fault_of_the_emulation_has_a_test():
    assert set(E.FAULTS) == set(GN_FAULTS) | {"no_clamp", "bscale_after_res", "badd_by_row", "mean_div_32", "cu_first_column"}
