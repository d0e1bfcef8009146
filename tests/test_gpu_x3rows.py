"""The fp32x engine's pre-split activation rows on the MI355X, at their writers and their reader (x3rows_ref.py holds the layout, the faults
test_x3rows_cpu.py seeds against these same comparisons, the restated dispatch rules and the bounds).

PRODUCERS (sf_op_gn_silu_rows, sf_op_ln_modulate_rows, sf_op_attention_rows): each runs twice on the same input into NaN-filled buffers, with
xfmt = 0 and xfmt = 1; the xfmt = 1 buffer must hold encode(plain output) byte for byte -- the flag selects only the store, so no tolerance
enters.  The inputs mix numerics.py's regimes per group / row and spread gamma, beta, scale, shift and V over 2^-14 .. 2^10, so that hi and lo'
are exercised from subnormal fp16 to 2^12.  Each id names the kernel the launcher's rule picks for the shape:
  gn_silu, C 256, G 32, B 2: gn_silu_reg_kernel<fp32, 2 / 4 / 8 / 16> (L 353 and 512, 700, 1500, 2049) and gn_silu_kernel<fp32,4> (L 4097, one
    past gn_reg_max_rv() * 512 / (cpg / 4) = 4096).  The fourth xfmt store in norms.hip, gn_silu_apply_kernel's, is unreachable: its only
    launch (gn_silu_ws_go) passes no xfmt, and launch_gn_silu_ws has no such argument;
  ln_modulate, C 128 / 256 / 512 / 1024: ln_modulate_kernel<fp32, 1 / 1 / 2 / 4> at 32 / 64 / 64 / 64 threads per row, with and without
    scale_shift, B L = 2 x 100 (exactly 25 / 50 workgroups) and 2 x 101 (a ragged last workgroup);
  attention, fp32x: attn_fwd_x3_kernel at H 2 / 8 (ldo 128 / 512), L 1 / 100 / 129 / 352, on the engine's packed q | k | v rows.
CONSUMER (sf_op_conv1d_epi with src_x3 = 1 on encode(x) built on the host): x3rows_ref.CONS_CASES, one per tile variant of
conv_gemm_mt_x3_variant at the smallest shapes that take the macro tiles.  The query must honour the flag; the output is gated element-wise
by conv1d_ref.gate with the split-label bound, and equals bit for bit the same call with src_x3 = 0 on the plain x (same label: both paths
form the same halves and issue the same MFMA sequence).  Only the `wide` case reads a subset of rows for the fp64 gate.
CHAINS, the pre-split buffer staying on the device, one per engine site: gn_silu -> conv3, ln_modulate -> projection, attention -> output
projection, each against fp64 of the whole pair with the producer's error bound folded into the GEMM gate (x3rows_ref.chain_gate).
ATTENTION at the engine's packed strides (ldq = ldkv = 3 H 64, kv = q + H 64 elements) in all four dtypes, and the 2-wave kernel
attention_mfma_kernel, which no other op-level shape reaches: test_gpu_numerics.py's two checks and tolerances on
  (2, 3, 100)   attention_ksplit_kernel       (9, 8, 1100)  attention_mfma4_kernel
  (16, 8, 200), (32, 8, 100)   attention_mfma_kernel (ceil(L / 64) H B 2 = 1024 waves, L < 256), also at contiguous strides through sf_op_attention
for bf16 / fp16; fp32 runs attn_fwd_f32_mfma_kernel and fp32x attn_fwd_x3_kernel on every shape (x3rows_ref.attention_kernel_name).
"""
import ctypes as C

import pytest
import torch

import conv1d_ref as R
import gemm_epilogue_ref as E
import numerics as nx
import x3rows_ref as X

pytestmark = pytest.mark.gpu

TD = {"fp32": torch.float32, "fp32x": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
UNSUPPORTED = 6
_lines = []


def _lib():
    from syncfusion_amd import _lib

    return _lib, _lib.load()


@pytest.fixture(scope="module", autouse=True)
def _report():
    """What ran, printed at the end of the module: kernel per case and err / bound per gated case."""
    yield
    print("\npre-split rows, per case:\n" + "\n".join(_lines))


def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _check_rows(plain: torch.Tensor, rows: torch.Tensor, what: str):
    """The producers' comparison: plain finite everywhere, and the xfmt buffer == encode(plain) byte for byte."""
    p = plain.cpu()
    assert bool(torch.isfinite(p).all()), f"{what}: the plain output has non-finite values"
    assert float(p.abs().max()) < 65504.0, f"{what}: the plain output leaves the fp16 range (a fault of the test's inputs)"
    msg = X.byte_diff(X.rows_of(rows), X.encode(p), what)
    assert not msg, msg
    _lines.append(f"{what}: byte-equal, {p.numel()} values, |v| {float(p.abs()[p != 0].min()):.2e} .. {float(p.abs().max()):.2e}")


# ----------------------------------------------------------------------------------------------------------------------------------
# producers
# ----------------------------------------------------------------------------------------------------------------------------------
def _gn_rows(cuda, xd, gd, bd, G, xfmt, dtype="fp32", out=None, out_ld=None):
    _l, lib = _lib()
    B, L, Cc = xd.shape
    out = nx.nan_like(xd.shape, xd.dtype, cuda) if out is None else out
    rc = lib.sf_op_gn_silu_rows(_l.DTYPES[dtype], xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), G, 1e-5, B, L, Cc, out.data_ptr(), out_ld or Cc, xfmt,
                                _l.stream_ptr(cuda))
    torch.cuda.synchronize()
    return rc, out


GN_L = (353, 512, 700, 1500, 2049, 4097)


@pytest.mark.parametrize("L", GN_L, ids=[f"L{L}-{X.gn_silu_kernel_name(L, 256, 32)}" for L in GN_L])
def test_gn_silu_rows_are_the_encoded_plain_output(cuda, L):
    """gn_silu_reg_kernel<fp32, 2 / 2 / 4 / 8 / 16> and, at L = 4097, the two-pass gn_silu_kernel<fp32,4> (x3rows_ref.gn_silu_kernel_name);
    B = 2: the second clip's base offset."""
    _l, _ = _lib()
    B, Cc, G = 2, 256, 32
    x, ga, be = X.gn_inputs(B, L, Cc, G)
    xd, gd, bd = x.to(cuda), ga.to(cuda), be.to(cuda)
    rc0, plain = _gn_rows(cuda, xd, gd, bd, G, 0)
    rc1, rows = _gn_rows(cuda, xd, gd, bd, G, 1)
    _l.check(rc0, "sf_op_gn_silu_rows")
    _l.check(rc1, "sf_op_gn_silu_rows (xfmt)")
    _check_rows(plain, rows, f"gn_silu B={B} L={L} C={Cc} G={G} [{X.gn_silu_kernel_name(L, Cc, G)}]")


def test_gn_silu_shapes_reach_every_kernel():
    names = {X.gn_silu_kernel_name(L, 256, 32) for L in GN_L}
    assert names == {f"gn_silu_reg_kernel<fp32,{rv}>" for rv in (2, 4, 8, 16)} | {"gn_silu_kernel<fp32,4>"}
    assert X.gn_silu_kernel_name(4096, 256, 32) == "gn_silu_reg_kernel<fp32,16>"          # 4097 is just beyond the register form


def _ln_rows(cuda, xd, sd, xfmt, dtype="fp32", out=None, out_ld=None):
    _l, lib = _lib()
    B, L, Cc = xd.shape
    out = nx.nan_like(xd.shape, xd.dtype, cuda) if out is None else out
    rc = lib.sf_op_ln_modulate_rows(_l.DTYPES[dtype], xd.data_ptr(), sd.data_ptr() if sd is not None else None, 1e-6, B, L, Cc, out.data_ptr(),
                                    out_ld or Cc, xfmt, _l.stream_ptr(cuda))
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("L", [100, 101])
@pytest.mark.parametrize("mod", [True, False], ids=["scale_shift", "plain"])
@pytest.mark.parametrize("Cc", [128, 256, 512, 1024], ids=[f"C{c}-{X.ln_kernel_name(c)}" for c in (128, 256, 512, 1024)])
def test_ln_modulate_rows_are_the_encoded_plain_output(cuda, Cc, mod, L):
    """ln_modulate_kernel<fp32, 1 / 1 / 2 / 4> with 32 / 64 / 64 / 64 threads per row (x3rows_ref.ln_plan, from ln_go).  2 x 100 rows fill
    the 25 (50) workgroups of 8 (4) rows exactly; 2 x 101 rows leave the last one ragged."""
    _l, _ = _lib()
    B = 2
    tpr, _vpt = X.ln_plan(Cc)
    assert ((B * L) % (256 // tpr) != 0) == (L == 101)
    x, ss = X.ln_inputs(B, L, Cc, mod)
    xd, sd = x.to(cuda), (ss.to(cuda) if mod else None)
    rc0, plain = _ln_rows(cuda, xd, sd, 0)
    rc1, rows = _ln_rows(cuda, xd, sd, 1)
    _l.check(rc0, "sf_op_ln_modulate_rows")
    _l.check(rc1, "sf_op_ln_modulate_rows (xfmt)")
    _check_rows(plain, rows, f"ln_modulate B={B} L={L} C={Cc} {'scale_shift' if mod else 'plain'} [{X.ln_kernel_name(Cc)}]")


def _attention_rows(cuda, dtype, qkv_dev, H, xfmt, out=None, ldo=None):
    """sf_op_attention_rows on packed rows (B, L, 3 H 64): q at column 0, kv at column H 64 of the same buffer, ldq = ldkv = 3 H 64."""
    _l, lib = _lib()
    B, L, w = qkv_dev.shape
    hd = H * X.HEAD
    assert w == 3 * hd
    out = nx.nan_like((B, L, hd), qkv_dev.dtype, cuda) if out is None else out
    rc = lib.sf_op_attention_rows(_l.DTYPES[dtype], qkv_dev.data_ptr(), 3 * hd, qkv_dev.data_ptr() + hd * qkv_dev.element_size(), 3 * hd, B, L, H, X.HEAD,
                                  out.data_ptr(), ldo or hd, xfmt, _l.stream_ptr(cuda))
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("L", [1, 100, 129, 352])
@pytest.mark.parametrize("H", [2, 8])
def test_attention_rows_are_the_encoded_plain_output(cuda, H, L):
    """attn_fwd_x3_kernel (fp32x) on packed rows, ldo = 128 / 512; L = 1, 100, 129 and 352 leave the last 128-query tile at 1, 100, 1 and 96
    queries."""
    _l, _ = _lib()
    B = 2
    qkv = X.attn_inputs(B, H, L).to(cuda)
    rc0, plain = _attention_rows(cuda, "fp32x", qkv, H, 0)
    rc1, rows = _attention_rows(cuda, "fp32x", qkv, H, 1)
    _l.check(rc0, "sf_op_attention_rows")
    _l.check(rc1, "sf_op_attention_rows (xfmt)")
    _check_rows(plain, rows, f"attention B={B} H={H} L={L} packed [{X.attention_kernel_name('fp32x', B, H, L)}]")


def test_producer_refusals_launch_nothing(cuda):
    """SF_ERR_UNSUPPORTED with the output still NaN, on the launchers' own conditions: C % 32, out_ld != C, (C / G) % 4, a 16-bit dtype with
    xfmt; attention: fp32 or a 16-bit dtype with xfmt, ldo != H 64."""
    g = torch.Generator().manual_seed(1)

    def untouched(rc, out, what):
        assert rc == UNSUPPORTED, f"{what}: returned {rc}"
        assert bool(torch.isnan(out.float()).all()), f"{what}: the refused call wrote its output"

    for Cc, G, ld, dt, what in ((48, 4, 48, "fp32", "C % 32"), (256, 32, 288, "fp32", "out_ld != C"), (64, 32, 64, "fp32", "(C / G) % 4"),
                                (256, 32, 256, "bf16", "bf16"), (256, 32, 256, "fp16", "fp16")):
        x = torch.randn(2, 40, Cc, generator=g).to(TD[dt]).to(cuda)
        ga, be = torch.ones(Cc, device=cuda), torch.zeros(Cc, device=cuda)
        out = nx.nan_like((2, 40, ld), TD[dt], cuda)
        untouched(_gn_rows(cuda, x, ga, be, G, 1, dt, out, ld)[0], out, f"gn_silu xfmt, {what}")
        if what != "(C / G) % 4":
            out = nx.nan_like((2, 40, ld), TD[dt], cuda)
            untouched(_ln_rows(cuda, x, None, 1, dt, out, ld)[0], out, f"ln_modulate xfmt, {what}")
    for dt, ldo, what in (("fp32", 128, "fp32"), ("bf16", 128, "bf16"), ("fp16", 128, "fp16"), ("fp32x", 160, "ldo != H 64")):
        qkv = torch.randn(2, 40, 384, generator=g).to(TD[dt]).to(cuda)
        out = nx.nan_like((2, 40, ldo), TD[dt], cuda)
        untouched(_attention_rows(cuda, dt, qkv, 2, 1, out=out, ldo=ldo)[0], out, f"attention xfmt, {what}")


# ----------------------------------------------------------------------------------------------------------------------------------
# consumer
# ----------------------------------------------------------------------------------------------------------------------------------
def _ptr(t):
    return t.data_ptr() if t is not None else None


def _consume(cuda, c, o, x_dev, src_x3, dtype="fp32x", C2=0, x2_dev=None, expect_rc=0):
    """One sf_op_conv1d_epi launch of case `c` on x_dev (pre-split rows when src_x3) -> (rc of the query, label, rc of the launch, out)."""
    _l, lib = _lib()
    td = TD[dtype]
    f = {k: (o[k].to(cuda).contiguous() if o[k] is not None else None) for k in ("bias", "badd")}
    w = o["w"] if C2 == 0 else torch.cat([o["w"], torch.zeros(c.N, C2)], dim=1)
    wd = w.to(cuda).contiguous()
    res = o["res"].to(td).to(cuda) if o["res"] is not None else None
    out = nx.nan_like((c.B, c.L, c.N), td, cuda)
    d = X.cons_desc(c, src_x3, dtype, C2, x=_ptr(x_dev), x2=_ptr(x2_dev), w=_ptr(wd), bias=_ptr(f["bias"]), badd=_ptr(f["badd"]), residual=_ptr(res), out=_ptr(out))
    qrc, label, _, _ = E.query_epi(d)
    ws = nx.poisoned_workspace(lib.sf_op_conv1d_epi_workspace_bytes(C.byref(d)), cuda)
    rc = lib.sf_op_conv1d_epi(C.byref(d), None, None, ws.data_ptr(), ws.numel(), _l.stream_ptr(cuda))
    torch.cuda.synchronize()
    if expect_rc == 0:
        assert qrc == 0, f"{X.cons_id(c)} src_x3={src_x3}: the query refuses ({qrc})"
        _l.check(rc, f"sf_op_conv1d_epi src_x3={src_x3}")
    return qrc, label, rc, out


@pytest.mark.parametrize("case", X.CONS_CASES, ids=X.cons_id)
def test_consumer_reads_presplit_rows(cuda, case):
    """conv_gemm_mt<x3> reading encode(x): tile variant 5 (128x128, two slots: qkv, conv1 with three taps, bias, residual and clip boundaries
    inside row tiles, attn_out with residual and badd), 7 (128x64: through `solo` on 2000 ragged rows, and N = 64), 0 (256x128: 16384 x 1024)
    -- x3rows_ref.mt_x3_variant, asserted against the table on the CPU.  Gate: conv1d_ref.gate, split label; then bit equality with the
    in-register split of the plain x."""
    o = X.cons_operands(case)
    rows_dev = X.as_f32(X.encode(o["x"])).to(cuda)
    _, label1, _, out1 = _consume(cuda, case, o, rows_dev, 1)
    assert label1 == X.SPLIT_LABEL, f"{X.cons_id(case)}: src_x3 = 1 is planned on {label1!r}, which reads no pre-split rows"
    _, label0, _, out0 = _consume(cuda, case, o, o["x"].to(cuda), 0)
    rows = X.cons_rows(case)
    ref, A, K = X.cons_ref(case, o, rows)
    got = out1.cpu()
    if rows is not None:
        assert bool(torch.isfinite(got).all()), f"{X.cons_id(case)} [{label1}]: non-finite outputs outside the gated rows"
        got = got.reshape(case.M, case.N)[rows][None]
    r, rel = R.gate(got, ref, A, K, "fp32x", label1, X.cons_id(case) + " src_x3")
    same = _bits_equal(out1, out0) if label0 == label1 else None
    _lines.append(f"consumer {X.cons_id(case)} [{label1}, tile variant {case.variant}]: err/bound {r:.3f}, rel-L2 {rel:.2e}, "
                  f"{'all' if rows is None else len(rows)} rows gated; src_x3 = 0 on the plain x [{label0}]: " +
                  ("bit-equal" if same else "DIFFERENT BITS" if same is not None else "another kernel, not compared"))
    if same is not None and not same:
        d = (out1.cpu() != out0.cpu()) | (torch.isnan(out1.cpu()) != torch.isnan(out0.cpu()))
        b, l, n = nx._unravel(int(d.flatten().nonzero()[0]), tuple(d.shape))
        raise AssertionError(f"{X.cons_id(case)} [{label1}]: {int(d.sum())} of {d.numel()} outputs differ between src_x3 = 1 and the in-register split, first at "
                             f"(clip {b}, position {l}, channel {n}): {float(out1[b, l, n]):.9g} vs {float(out0[b, l, n]):.9g}")


def test_consumer_refusals_launch_nothing(cuda):
    """SF_ERR_UNSUPPORTED from the query and from the launch alike, the output still NaN: src_x3 with bf16 / fp16 / fp32, with a second
    source, and on a shape below the macro-tile threshold (64 tiles of 128x64)."""
    c = X.CONS_CASES[0]
    o = X.cons_operands(c)
    rows_dev = X.as_f32(X.encode(o["x"])).to(cuda)

    def refused(qrc, label, rc, out, what):
        assert (qrc, rc) == (UNSUPPORTED, UNSUPPORTED), f"{what}: query {qrc}, launch {rc} (label {label!r})"
        assert bool(torch.isnan(out.float()).all()), f"{what}: the refused launch wrote its output"

    for dt in ("bf16", "fp16", "fp32"):
        xd = o["x"].to(TD[dt]).to(cuda)
        refused(*_consume(cuda, c, o, xd, 1, dtype=dt, expect_rc=UNSUPPORTED), f"src_x3 with {dt}")
    x2 = torch.zeros(c.B, c.L, 64, device=cuda)
    refused(*_consume(cuda, c, o, rows_dev, 1, C2=64, x2_dev=x2, expect_rc=UNSUPPORTED), "src_x3 with C2 = 64")
    below = c._replace(L=512)
    assert not X.mt_x3_prefers(below.M, below.N, below.K)
    ob = X.cons_operands(below)
    refused(*_consume(cuda, below, ob, X.as_f32(X.encode(ob["x"])).to(cuda), 1, expect_rc=UNSUPPORTED), "src_x3 below the macro-tile threshold")


# ----------------------------------------------------------------------------------------------------------------------------------
# guard bands (test_gpu_guards.py's method): the new entries neither write nor read outside what they are handed
# ----------------------------------------------------------------------------------------------------------------------------------
GUARDED = [(p, x) for p in ("gn_silu-L353", "gn_silu-L4097", "ln_modulate-C128-L101", "attention-fp32x-H2-L129") for x in (0, 1)] + \
          [("attention-bf16-B16-H8-L200", 0)]          # (xfmt with a 16-bit dtype is a refusal)


@pytest.mark.parametrize("producer,xfmt", GUARDED, ids=[f"{p}-xfmt{x}" for p, x in GUARDED])
def test_producers_stay_inside_their_buffers(cuda, producer, xfmt):
    """Every device pointer inside guard bands, the packed q | k | v buffer included (kv points hd elements into it): guards untouched, inputs
    unchanged, the output equal to the run on plain allocations byte for byte."""
    import test_gpu_guards as GB

    _l, lib = _lib()
    st = _l.stream_ptr(cuda)
    kind = producer.split("-")[0]
    if kind == "gn_silu":
        B, L, Cc, G = 2, int(producer.split("-L")[1]), 256, 32
        x, ga, be = X.gn_inputs(B, L, Cc, G)

        def run(a):
            xs, gs, bs, out = a.inp(x, "x"), a.inp(ga, "gamma"), a.inp(be, "beta"), a.out((B, L, Cc), torch.float32, "out")
            return lib.sf_op_gn_silu_rows(_l.SF_F32, xs.ptr, gs.ptr, bs.ptr, G, 1e-5, B, L, Cc, out.ptr, Cc, xfmt, st), [out]
    elif kind == "ln_modulate":
        B, L, Cc = 2, 101, 128
        x, ss = X.ln_inputs(B, L, Cc, True)

        def run(a):
            xs, sd, out = a.inp(x, "x"), a.inp(ss, "scale_shift"), a.out((B, L, Cc), torch.float32, "out")
            return lib.sf_op_ln_modulate_rows(_l.SF_F32, xs.ptr, sd.ptr, 1e-6, B, L, Cc, out.ptr, Cc, xfmt, st), [out]
    else:
        dtype = producer.split("-")[1]
        B, H, L = (16, 8, 200) if dtype == "bf16" else (2, 2, 129)
        hd, td = H * X.HEAD, TD[dtype]
        qkv = X.attn_inputs(B, H, L, v_spread=False).to(td)

        def run(a):
            qs, out = a.inp(qkv, "qkv"), a.out((B, L, hd), td, "out")
            return lib.sf_op_attention_rows(_l.DTYPES[dtype], qs.ptr, 3 * hd, qs.ptr + hd * qkv.element_size(), 3 * hd, B, L, H, X.HEAD, out.ptr, hd, xfmt, st), [out]

    GB._run_case(cuda, f"{producer} xfmt={xfmt}", run, nan_ok=(0,) if xfmt else ())      # (pre-split rows are not fp32 values)


def test_consumer_stays_inside_its_buffers(cuda):
    """src_x3 = 1 on 2000 ragged rows (the last 128-row tile holds 80): rows, weight, output and an exactly sized workspace inside guard bands."""
    import test_gpu_guards as GB

    _l, lib = _lib()
    c = X.CONS_CASES[1]
    o = X.cons_operands(c)
    rows = X.as_f32(X.encode(o["x"]))

    def run(a):
        xs, ws_, out = a.inp(rows, "rows"), a.inp(o["w"], "w"), a.out((c.B, c.L, c.N), torch.float32, "out")
        d = X.cons_desc(c, 1, x=xs.ptr, w=ws_.ptr, out=out.ptr)
        n = lib.sf_op_conv1d_epi_workspace_bytes(C.byref(d))
        wk = a.ws(n, "ws")
        return lib.sf_op_conv1d_epi(C.byref(d), None, None, wk.ptr, n, _l.stream_ptr(cuda)), [out]

    GB._run_case(cuda, "sf_op_conv1d_epi src_x3", run)


# ----------------------------------------------------------------------------------------------------------------------------------
# chains: producer (xfmt) -> consumer (src_x3), the pre-split buffer on the device
# ----------------------------------------------------------------------------------------------------------------------------------
def _chain(cuda, case, o, act_dev, a, da, what):
    _, label, _, out = _consume(cuda, case, o, act_dev, 1)
    assert label == X.SPLIT_LABEL
    r, rel = X.chain_gate(out.cpu(), a, da, o["w3"], o["bias"], o["res"], o["badd"], case.taps, case.pad, label, what)
    _lines.append(f"chain {what} [{label}, tile variant {case.variant}]: err/bound {r:.3f}, rel-L2 {rel:.2e}")


def test_chain_gn_silu_into_conv3(cuda):
    """unet_engine.cpp conv3: launch_gn_silu(xfmt) -> the three-tap convolution with bias and residual, 3 x 1323 rows (gn_silu_reg_kernel<fp32,8>,
    conv_gemm_mt<x3> 128x128)."""
    _l, _ = _lib()
    c = X.CONS_CASES[2]
    o = X.cons_operands(c)
    g = torch.Generator().manual_seed(21)
    ga, be = 1 + 0.2 * torch.randn(c.C, generator=g), 0.1 * torch.randn(c.C, generator=g)
    rc, act = _gn_rows(cuda, o["x"].to(cuda), ga.to(cuda), be.to(cuda), 32, 1)
    _l.check(rc, "sf_op_gn_silu_rows (xfmt)")
    a, da = X.gn_silu_ref(o["x"], 32, ga, be, 1e-5)
    _chain(cuda, c, o, act, a, da, f"gn_silu[{X.gn_silu_kernel_name(c.L, c.C, 32)}] -> conv3 {X.cons_id(c)}")


def test_chain_ln_modulate_into_projection(cuda):
    """unet_engine.cpp, the attention block's pre-norm: launch_ln_modulate(xfmt) -> the qkv-like projection, 2 x 1024 rows of 256 channels."""
    _l, _ = _lib()
    c = X.CONS_CASES[0]
    o = X.cons_operands(c)
    ss = 0.3 * torch.randn(c.B, 2 * c.C, generator=torch.Generator().manual_seed(22))
    rc, act = _ln_rows(cuda, o["x"].to(cuda), ss.to(cuda), 1)
    _l.check(rc, "sf_op_ln_modulate_rows (xfmt)")
    a, da = X.ln_modulate_ref(o["x"], ss, 1e-6)
    _chain(cuda, c, o, act, a, da, f"ln_modulate[{X.ln_kernel_name(c.C)}] -> projection {X.cons_id(c)}")


def test_chain_attention_into_output_projection(cuda):
    """unet_engine.cpp, attention on the packed q | k | v rows with xfmt -> the output projection with residual (and badd), H = 8, 2 x 1024."""
    _l, _ = _lib()
    c = X.CONS_CASES[3]
    H = c.C // X.HEAD
    o = X.cons_operands(c)
    qkv = X.attn_inputs(c.B, H, c.L, v_spread=False)
    rc, act = _attention_rows(cuda, "fp32x", qkv.to(cuda), H, 1)
    _l.check(rc, "sf_op_attention_rows (xfmt)")
    a, da = X.attention_ref(qkv[..., :c.C], qkv[..., c.C:2 * c.C], qkv[..., 2 * c.C:], H)
    _chain(cuda, c, o, act, a, da, f"attention[attn_fwd_x3_kernel] -> output projection {X.cons_id(c)}")


# ----------------------------------------------------------------------------------------------------------------------------------
# attention at the engine's packed strides, and the 2-wave kernel
# ----------------------------------------------------------------------------------------------------------------------------------
ATT_SHAPES = [(2, 3, 100), (9, 8, 1100), (16, 8, 200), (32, 8, 100)]          # B, H, L
TWO_WAVE = [(16, 8, 200), (32, 8, 100)]
ATT_CASES = [(s, "packed") for s in ATT_SHAPES] + [(s, "contiguous") for s in TWO_WAVE]
_att_ref = {}


def _cached(key, make):
    """(q, k, v, ref) of one (kind, B, H, L, ..., storage type): fp32 and fp32x share an entry; only the current shape's entries are kept."""
    if any(k[:4] != key[:4] for k in _att_ref):
        _att_ref.clear()
    if key not in _att_ref:
        _att_ref[key] = make()
    return _att_ref[key]


def _att_id(p):
    (B, H, L), layout = p
    return f"B{B}-H{H}-L{L}-{layout}-{X.attention_kernel_name('bf16', B, H, L).split('<')[0]}"


def _k(dtype):
    return nx.MAX_K16 if dtype in ("bf16", "fp16") else nx.MAX_K


def _run_attention(cuda, dtype, q, k, v, H, layout):
    """q, k, v (B, L, H 64) fp32 holding dtype-rounded values -> the op's output in fp32 on the host, out NaN-filled beforehand."""
    _l, lib = _lib()
    td = TD[dtype]
    B, L, hd = q.shape
    if layout == "packed":
        rc, out = _attention_rows(cuda, dtype, torch.cat([q, k, v], dim=-1).to(td).to(cuda), H, 0)
        _l.check(rc, "sf_op_attention_rows")
    else:
        qd, kvd = q.to(td).to(cuda), torch.cat([k, v], dim=-1).to(td).to(cuda)
        out = nx.nan_like(qd.shape, td, cuda)
        _l.check(lib.sf_op_attention(_l.DTYPES[dtype], qd.data_ptr(), kvd.data_ptr(), B, L, H, X.HEAD, out.data_ptr(), _l.stream_ptr(cuda)), "sf_op_attention")
        torch.cuda.synchronize()
    return out.float().cpu()


@pytest.mark.parametrize("dtype", ["fp32", "fp32x", "bf16", "fp16"])
@pytest.mark.parametrize("peak", nx.PEAK_STDS)
@pytest.mark.parametrize("shape_layout", ATT_CASES, ids=_att_id)
def test_attention_peaked_at_engine_strides(cuda, dtype, peak, shape_layout):
    """test_gpu_numerics.py::test_attention_peaked's check and tolerances, dominant key in the ragged last key block, on the packed q | k | v
    buffer (and, for the 2-wave shapes, at contiguous strides).  16-bit kernels by attention_mfma_go's rule: (2, 3, 100) key split (24 waves),
    (9, 8, 1100) 4-wave (648 workgroups, L >= 256), (16, 8, 200) and (32, 8, 100) 2-wave (1024 waves, L < 256); fp32: attn_fwd_f32_mfma_kernel,
    fp32x: attn_fwd_x3_kernel."""
    (B, H, L), layout = shape_layout
    D = X.HEAD
    td = TD[dtype]

    def make():
        g = torch.Generator().manual_seed(B * 100 + L + int(peak))
        q, k = nx.peaked_qk(B, L, H, D, peak, "last", g)
        v = torch.randn(B, L, H * D, generator=g)
        q, k, v = (t.to(td).float() for t in (q, k, v))
        return q, k, v, nx.attention64(q, k, v, H)

    q, k, v, ref = _cached(("peaked", B, H, L, peak, td), make)
    got = _run_attention(cuda, dtype, q, k, v, H, layout)
    tol = 1e-5 if dtype in ("fp32", "fp32x") else 8e-3
    kern = X.attention_kernel_name(dtype, B, H, L)
    rel = nx.check_close(got, ref, tol, f"attention {dtype} peak {peak:g} at last B={B} H={H} L={L} {layout} [{kern}]", k=_k(dtype), dims=("clip", "query", "channel"))
    _lines.append(f"attention peaked {dtype} peak {peak:g} B={B} H={H} L={L} {layout} [{kern}]: rel-L2 {rel:.2e} (gate {tol:.0e})")


@pytest.mark.parametrize("dtype", ["fp32", "fp32x", "bf16", "fp16"])
@pytest.mark.parametrize("shape_layout", ATT_CASES, ids=_att_id)
def test_attention_uniform_weights_at_engine_strides(cuda, dtype, shape_layout):
    """test_gpu_numerics.py's q = 0 check (every weight 1 / L, integer V: a key block dropped or counted twice moves the output by >= 1 / L of
    a whole value) at the same shapes, layouts and kernels as test_attention_peaked_at_engine_strides."""
    (B, H, L), layout = shape_layout
    D = X.HEAD

    def make():
        g = torch.Generator().manual_seed(L + 1)
        q = torch.zeros(B, L, H * D)
        k = torch.randn(B, L, H * D, generator=g).to(TD[dtype]).float()
        v = torch.randint(0, 9, (B, L, H * D), generator=g).float()
        return q, k, v, v.double().mean(1, keepdim=True).expand(B, L, H * D)

    q, k, v, ref = _cached(("uniform", B, H, L, TD[dtype]), make)
    got = _run_attention(cuda, dtype, q, k, v, H, layout)
    tol = 1e-6 if dtype in ("fp32", "fp32x") else 4e-3
    kern = X.attention_kernel_name(dtype, B, H, L)
    rel = nx.check_close(got, ref, tol, f"attention q=0 {dtype} B={B} H={H} L={L} {layout} [{kern}]", k=2.0, dims=("clip", "query", "channel"))
    _lines.append(f"attention q=0 {dtype} B={B} H={H} L={L} {layout} [{kern}]: rel-L2 {rel:.2e} (gate {tol:.0e})")


def test_attention_shapes_reach_every_mfma_kernel():
    for dt, t in (("bf16", "bf16"), ("fp16", "f16")):
        assert [X.attention_kernel_name(dt, *s) for s in ATT_SHAPES] == [f"attention_ksplit_kernel<{t}>", f"attention_mfma4_kernel<{t}>",
                                                                        f"attention_mfma_kernel<{t}>", f"attention_mfma_kernel<{t}>"]
