"""The pre-split row format of the fp32x engine on the CPU (x3rows_ref.py): the round trip and its bound, the byte layout against st4_x3's
address arithmetic, every seeded fault shown to fail the comparison test_gpu_x3rows.py makes on the same inputs (byte equality for a
producer, conv1d_ref's fp64 gate for the consumer), the restated dispatch rules, and the plans of the consumer cases through the device-free
query sf_op_conv1d_epi_variant."""
import struct

import pytest
import torch

import conv1d_ref as R
import gemm_epilogue_ref as E
import x3rows_ref as X

SMALL = X.CONS_CASES[0]._replace(name="qkv-cpu", L=96)       # the consumer's arithmetic at a size the CPU multiplies in no time (no plan is asked for it)


# ---------------------------------------------------------------------------------------------------------------------------------
# round trip and layout
# ---------------------------------------------------------------------------------------------------------------------------------
def _regime(name: str) -> torch.Tensor:
    g = torch.Generator().manual_seed(11)
    n = 64 * 1024
    mant = 1.0 + torch.rand(n, generator=g)
    if name == "normal":
        v = mant * torch.exp2(torch.randint(-13, 15, (n,), generator=g).float())
    elif name == "below_2^-14":                               # hi is a subnormal fp16, or zero (below 2^-25)
        v = mant * torch.exp2(torch.randint(-40, -14, (n,), generator=g).float())
    elif name == "zeros":
        v = torch.zeros(n)
        v[1::2] = -0.0
    elif name == "negative":
        v = -mant * torch.exp2(torch.randint(-20, 15, (n,), generator=g).float())
    elif name == "near_6e4":                                  # up to the largest value whose hi is finite (65519.99: fp16(v) = 65504)
        v = 57344.0 + 8175.0 * torch.rand(n, generator=g)
        v[0], v[1] = 65504.0, 65519.0
    elif name == "ties":                                      # v exactly between two fp16 values, and residuals exactly between two lo' values
        h = (mant * 1024).floor() / 1024
        v = torch.cat([(h + 2.0 ** -11)[: n // 2], (h + 2.0 ** -11 + 2.0 ** -23)[n // 2:]])
    else:
        raise ValueError(name)
    sign = 1.0 if name in ("negative", "zeros") else torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    return (v * sign).reshape(-1, 64)


@pytest.mark.parametrize("regime", ["normal", "below_2^-14", "zeros", "negative", "near_6e4", "ties"])
def test_round_trip_within_the_derived_bound(regime):
    """|decode(encode(v)) - v| <= max(2^-22 |v|, 2^-36) (x3rows_ref.py, ROUND TRIP), every element; zeros come back as zeros."""
    v = _regime(regime)
    rows = X.encode(v)
    assert rows.dtype == torch.float16 and rows.shape == (v.shape[0], 128) and bool(torch.isfinite(rows.float()).all())
    err = (X.decode(rows) - v.double()).abs()
    ratio = float((err / X.round_trip_bound(v)).max())
    print(f"round trip {regime}: max err / bound {ratio:.3f}")
    assert ratio <= 1.0
    if regime == "zeros":
        assert bool((X.decode(rows) == 0).all())
    if regime == "below_2^-14":
        assert bool((X.halves(rows)[0].abs() <= 2.0 ** -14).all())          # the regime was reached: every hi subnormal, zero, or rounded up to 2^-14


def test_halves_are_conv1d_refs_split():
    v = _regime("normal")
    hi, lo = X.halves(X.encode(v))
    h2, l2 = R.x3_split(v)
    assert torch.equal(hi, h2) and torch.equal(lo, l2)


def test_layout_is_st4_x3s_address_arithmetic():
    """common.h st4_x3: channel c of a row goes to byte (c >> 5) * 128 + (c & 31) * 2 (hi) and 64 bytes further (lo'), little endian."""
    g = torch.Generator().manual_seed(5)
    v = torch.randn(3, 160, generator=g) * 7
    raw = X.as_f32(X.encode(v)).numpy().tobytes()
    hi, lo = R.x3_split(v)
    for r in range(3):
        for c in range(160):
            p = r * 640 + (c >> 5) * 128 + (c & 31) * 2
            assert struct.unpack_from("<e", raw, p)[0] == float(hi[r, c]) and struct.unpack_from("<e", raw, p + 64)[0] == float(lo[r, c])
    assert X.same_bytes(X.rows_of(X.as_f32(X.encode(v))), X.encode(v))


def test_trunc16_truncates():
    v = _regime("normal")
    t = X.trunc16(v)
    assert bool((t.abs() <= v.abs()).all()) and bool(((v.abs() - t.abs()) < 2.0 ** -10 * v.abs()).all())
    assert bool((t != v.half().float()).any())


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded faults: producers (byte equality)
# ---------------------------------------------------------------------------------------------------------------------------------
def _producer_outputs():
    """The plain fp32 output of each producer on test_gpu_x3rows.py's inputs (one shape each), from the fp64 references."""
    x, ga, be = X.gn_inputs(2, 353, 256, 32)
    yield "gn_silu", X.gn_silu_ref(x, 32, ga, be, 1e-5)[0].float()
    x, ss = X.ln_inputs(2, 100, 128, True)
    yield "ln_modulate", X.ln_modulate_ref(x, ss, 1e-6)[0].float()
    qkv = X.attn_inputs(2, 2, 100)
    yield "attention", X.attention_ref(qkv[..., :128], qkv[..., 128:256], qkv[..., 256:], 2)[0].float()


PRODUCED = dict(_producer_outputs())


@pytest.mark.parametrize("producer", list(PRODUCED))
def test_producer_inputs_exercise_the_format(producer):
    """The outputs the byte comparison runs on reach below 2^-14 (subnormal hi), above 2^6, both signs, and stay below the fp16 range."""
    y = PRODUCED[producer]
    a = y.abs()
    assert bool(torch.isfinite(y).all()) and float(a.max()) < 65504.0
    assert bool(((a < 2.0 ** -14) & (a > 0)).any()) and bool((a > 64.0).any()) and bool((y < 0).any()) and bool((y > 0).any())


@pytest.mark.parametrize("fault", X.FAULTS)
@pytest.mark.parametrize("producer", list(PRODUCED))
def test_writer_faults_fail_the_byte_comparison(producer, fault):
    """A producer that wrote encode(plain, fault) into its NaN-filled buffer fails `rows == encode(plain)`, with a message that names the spot."""
    y = PRODUCED[producer]
    assert X.byte_diff(X.encode(y), X.encode(y), producer) == ""
    msg = X.byte_diff(X.encode(y, fault), X.encode(y), f"{producer} {fault}")
    assert msg and "differ" in msg, f"{fault} went unnoticed on {producer}"


def test_head_local_chunk_is_invisible_below_two_chunks():
    """Why the attention cases take H >= 2 and the norm cases C >= 128: on a 64-channel row the head-local chunk index is the row's."""
    v = torch.randn(4, 64)
    assert X.same_bytes(X.encode(v, "head_local_chunk"), X.encode(v))


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded faults: the consumer (fp64 gate)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_consumer():
    o = X.cons_operands(SMALL)
    ref, A, K = X.cons_ref(SMALL, o)
    return o, ref, A, K


def _gate(dev, ref, A, K, what):
    return R.gate(dev, ref, A, K, "fp32x", X.SPLIT_LABEL, what, quiet=True)


def test_consumer_emulation_passes_the_gate_and_equals_the_in_register_split(small_consumer):
    o, ref, A, K = small_consumer
    dev = X.emulate_src_x3(X.encode(o["x"]), o["w3"], o["bias"], o["res"], SMALL.taps, 1, SMALL.pad, 1)
    r, _ = _gate(dev, ref, A, K, "correct reader")
    assert r < 0.25                                                         # worst-case bound, random-sign errors
    plain = R.emulate(o["x"], o["w3"], o["bias"], o["res"], SMALL.taps, 1, SMALL.pad, 1, "fp32x", X.SPLIT_LABEL, stored=False)
    assert torch.equal(dev, plain)                                          # both paths form the same halves: the GPU test's bit equality


@pytest.mark.parametrize("fault", [f for f in X.FAULTS if f not in X.WRITER_ONLY])
def test_reader_faults_fail_the_gate(small_consumer, fault):
    o, ref, A, K = small_consumer
    dev = X.emulate_src_x3(X.encode(o["x"]), o["w3"], o["bias"], o["res"], SMALL.taps, 1, SMALL.pad, 1, fault)
    with pytest.raises(AssertionError, match="err/bound|non-finite"):
        _gate(dev, ref, A, K, f"reader {fault}")


@pytest.mark.parametrize("fault", ["halves_swapped", "pitch_64", "head_local_chunk"])
def test_layout_faults_of_a_writer_fail_the_gate_behind_a_correct_reader(small_consumer, fault):
    """The chained tests (producer -> consumer on the device) see a misplaced half through the GEMM gate as well."""
    o, ref, A, K = small_consumer
    dev = X.emulate_src_x3(X.encode(o["x"], fault), o["w3"], o["bias"], o["res"], SMALL.taps, 1, SMALL.pad, 1)
    with pytest.raises(AssertionError, match="err/bound|non-finite"):
        _gate(dev, ref, A, K, f"writer {fault}")


def test_a_truncated_hi_is_seen_by_the_byte_comparison_only(small_consumer):
    """hi_truncated decodes to v within 2^-21 |v|: the consumer's gate passes on it (so no accuracy test can stand in for the producers' byte
    comparison), the bytes differ in about half of the words."""
    o, ref, A, K = small_consumer
    rows = X.encode(o["x"], "hi_truncated")
    err = (X.decode(rows) - o["x"].double()).abs()
    assert bool((err <= 2.0 ** -21 * o["x"].double().abs() + 2.0 ** -36).all())
    r, _ = _gate(X.emulate_src_x3(rows, o["w3"], o["bias"], o["res"], SMALL.taps, 1, SMALL.pad, 1), ref, A, K, "writer hi_truncated")
    assert r < 1.0
    assert not X.same_bytes(rows, X.encode(o["x"]))


def test_zero_padding_rows_of_a_three_tap_window_read_as_garbage_fail_the_gate():
    """conv1-like: the rows a 3-tap window reads beyond a clip's ends are zeros.  A reader that takes the neighbouring clip's row instead
    (no padding mask) misses the gate on the first and last position of the clips."""
    c = X.CONS_CASES[2]._replace(name="conv1-cpu", L=45)
    o = X.cons_operands(c)
    ref, A, K = X.cons_ref(c, o)
    good = X.emulate_src_x3(X.encode(o["x"]), o["w3"], o["bias"], o["res"], 3, 1, 1, 1)
    _gate(good, ref, A, K, "conv1 correct")
    hi, lo = X.halves(X.encode(o["x"]))
    flat = lambda t: torch.nn.functional.pad(t.reshape(1, c.M, c.C), (0, 0, 1, 1))                       # noqa: E731  one clip of B L rows
    win = lambda t: torch.cat([flat(t)[:, k:k + c.M] for k in range(3)], dim=-1).reshape(c.B, c.L, 3 * c.C)   # noqa: E731
    wh, wl = R.x3_split(R.weight_matrix(o["w3"]))
    bad = win(hi) @ wh + (win(hi) @ wl + win(lo) @ wh) / 2048.0 + o["bias"] + o["res"]
    assert torch.equal(bad[:, 1:-1], good[:, 1:-1])
    with pytest.raises(AssertionError, match="err/bound"):
        _gate(bad, ref, A, K, "conv1 without the padding mask")


# ---------------------------------------------------------------------------------------------------------------------------------
# producers' error bounds: an fp32 evaluation in another order stays inside them
# ---------------------------------------------------------------------------------------------------------------------------------
def test_producer_bounds_hold_for_an_fp32_evaluation():
    """The bounds da of x3rows_ref.py hold for torch's own fp32 evaluation of the three producers on the chained tests' ordinary inputs (a
    sanity check of their size: fp32 torch sums in another order than the kernels, with comparable depth, but about no pivot -- so not at
    offset rows), and are small next to the values."""
    F = torch.nn.functional
    g = torch.Generator().manual_seed(2)
    x, ga, be = E.clip_input(2, 353, 256, g, "fp32"), 1 + 0.2 * torch.randn(256, generator=g), 0.1 * torch.randn(256, generator=g)
    a, da = X.gn_silu_ref(x, 32, ga, be, 1e-5)
    got = F.silu(F.group_norm(x.transpose(1, 2), 32, ga, be, eps=1e-5)).transpose(1, 2)
    assert float(((got.double() - a).abs() / da).max()) <= 1.0
    x, ss = E.clip_input(2, 100, 256, g, "fp32"), 0.3 * torch.randn(2, 512, generator=g)
    a, da = X.ln_modulate_ref(x, ss, 1e-6)
    got = F.layer_norm(x, (256,), eps=1e-6) * (1 + ss[:, None, :256]) + ss[:, None, 256:]
    assert float(((got.double() - a).abs() / da).max()) <= 1.0
    qkv = X.attn_inputs(2, 2, 100, v_spread=False)
    q, k, v = qkv[..., :128], qkv[..., 128:256], qkv[..., 256:]
    a, da = X.attention_ref(q, k, v, 2)
    got = E.nx.attention64(q, k, v, 2).float()
    assert float(((got.double() - a).abs() / da).max()) <= 1.0 and float(da.max()) < 1e-3 * float(a.abs().max())


# ---------------------------------------------------------------------------------------------------------------------------------
# dispatch rules and plans
# ---------------------------------------------------------------------------------------------------------------------------------
def test_restated_dispatch_rules():
    gn = {L: X.gn_silu_kernel_name(L, 256, 32) for L in (353, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097)}
    assert gn == {353: "gn_silu_reg_kernel<fp32,2>", 512: "gn_silu_reg_kernel<fp32,2>", 513: "gn_silu_reg_kernel<fp32,4>", 1024: "gn_silu_reg_kernel<fp32,4>",
                  1025: "gn_silu_reg_kernel<fp32,8>", 2048: "gn_silu_reg_kernel<fp32,8>", 2049: "gn_silu_reg_kernel<fp32,16>",
                  4096: "gn_silu_reg_kernel<fp32,16>", 4097: "gn_silu_kernel<fp32,4>"}
    assert [X.ln_plan(C) for C in (128, 256, 512, 1024)] == [(32, 1), (64, 1), (64, 2), (64, 4)]
    a16 = {s: X.attention_kernel_name("bf16", *s) for s in ((2, 3, 100), (2, 3, 352), (9, 8, 1100), (4, 8, 2048), (40, 8, 300), (16, 8, 200), (32, 8, 100))}
    assert [v.split("<")[0] for v in a16.values()] == ["attention_ksplit_kernel", "attention_ksplit_kernel", "attention_mfma4_kernel", "attention_mfma4_kernel",
                                                       "attention_mfma4_kernel", "attention_mfma_kernel", "attention_mfma_kernel"]
    assert X.attention_kernel_name("fp32x", 2, 8, 100) == "attn_fwd_x3_kernel" and X.attention_kernel_name("fp16", 16, 8, 200) == "attention_mfma_kernel<f16>"
    assert X.mt_x3_min_cols(2000) == 512 and X.mt_x3_min_cols(2048) == 512 and X.mt_x3_min_cols(1800) == 576
    assert not X.mt_x3_prefers(2000, 448, 256) and X.mt_x3_prefers(2000, 449, 256) and not X.mt_x3_prefers(2048, 512, 224)


@pytest.mark.parametrize("case", X.CONS_CASES, ids=X.cons_id)
def test_consumer_cases_take_the_macro_tiles_and_their_variant(case):
    """Every consumer case is at the macro-tile threshold or above it by the restated rule, names the tile variant that rule gives, and the
    query (no device) honours src_x3 for it with the label the plain call gets."""
    assert X.mt_x3_prefers(case.M, case.N, case.K) and X.mt_x3_variant(case.M, case.N, case.solo) == case.variant
    for src_x3 in (1, 0):
        rc, label, row, gn = E.query_epi(X.cons_desc(case, src_x3, **X.cons_probe_ptrs(case)))
        assert (rc, label, row, gn) == (0, X.SPLIT_LABEL, False, False), (src_x3, rc, label)
    assert {c.variant for c in X.CONS_CASES} == {0, 5, 7} and any(c.solo and c.variant == 7 for c in X.CONS_CASES)


def test_src_x3_refusals_of_the_query():
    """SF_ERR_UNSUPPORTED (6) from the query, as from the launch: any dtype but fp32x, a second source, a shape below the macro-tile
    threshold, the LayerNorm-consumer entry; the same descriptors without the flag are taken."""
    c = X.CONS_CASES[0]
    p = X.cons_probe_ptrs(c)
    for dt in ("bf16", "fp16", "fp32"):
        assert E.query_epi(X.cons_desc(c, 1, dtype=dt, **p))[0] == 6 and E.query_epi(X.cons_desc(c, 0, dtype=dt, **p))[0] == 0
    assert E.query_epi(X.cons_desc(c, 1, C2=64, x2=E.PROBE, **p))[0] == 6 and E.query_epi(X.cons_desc(c, 0, C2=64, x2=E.PROBE, **p))[0] == 0
    below = c._replace(L=512)
    assert not X.mt_x3_prefers(below.M, below.N, below.K)
    rc, label, _, _ = E.query_epi(X.cons_desc(below, 0, **p))
    assert rc == 0 and "conv_gemm_mt" not in label
    assert E.query_epi(X.cons_desc(below, 1, **p))[0] == 6
    d = X.cons_desc(c, 1, ln_part=E.PROBE, **p)
    assert E.query_ln(d)[0] == 6


def test_desc_mirror_keeps_its_layout():
    """src_x3 took the place of the reserved word: same offset, same struct size (the header's struct is 72 bytes of int32 / float, then pointers)."""
    from syncfusion_amd import _lib as _l
    import ctypes as C

    assert _l.Conv1dEpiDesc.src_x3.offset == 68 and _l.Conv1dEpiDesc.x.offset == 72 and C.sizeof(_l.Conv1dEpiDesc) == 72 + 12 * 8
