"""The shared back half of the small-batch implicit-GEMM kernels (csrc/gemm_epilogue.h) against fp64 on the MI355X, one launch at a time through
sf_op_conv1d_epi and sf_op_conv1d_ln: every element of every output -- the values, the row partials (rowpart), the GroupNorm tile statistics
(gnpart) and the LayerNorm consumer's output -- is held to the bounds derived in gemm_epilogue_ref.py.  Every case first asks the _variant query
and asserts the kernel family and the flags its row names, NaN-fills its outputs and poisons the workspace.

EPI_CASES:
  * producers (rowpart + gnpart; conv_gemm_rs for bf16 / fp16 / fp32x, conv_gemm_wp for fp32 and where rs refuses: K > 2048, split K > 1280):
    one tap of 256 channels and three taps of 128, N in {32, 64, 96}, and (B, L) chosen for where the clip boundaries fall inside the 32-row
    tiles: (1, 32) tile = clip; (1, 45) 13 rows in the last tile; (2, 32); (7, 37) boundaries at offsets 5, 10, .., 30, 3; (3, 63);
    (2, 50) with stride 2 over a x2-upsampled source; Lout = 20 < 32: gnpart declined, rowpart still honoured (the buffer stays NaN);
  * rowpart only: conv_gemm_fast from 513 tiles on, and the one macro-tile row with mt_ln (16-bit);
  * statistics regimes of the stored output on one rs and one wp shape: rows at mean / std = 3, 30, 300, constant rows, first row + 50;
  * epilogue operands: bias + bscale + residual + badd on each family's ragged shape of test_gpu_conv1d_elementwise.py (sk, v2, fast, wp, rs),
    act 0 .. 3, out_f32 on and off for the 16-bit types, and a second source of 32 .. 160 channels on every family.
LN_CASES (all four dtypes, each run with partials computed by the test in fp64 and again chained behind a producer launch that wrote both the
source and the partials): accumulator side on rs (K = 1024; fp32: fast) and on fast (K = 128), operand side with ln_ss, with ln_ss + res_ln and
plain; source rows at mean / std = 3, 30, 300.  The first run arms the consumer's own rowpart output and checks it like a producer's.
CB_CASES: sf_op_conv_cb_tiles, the one consumer of gnpart (conv_cb prologue 2 + cb_reduce_gn), bf16 / fp16 / fp32x at (2, 44, C 128, G 4),
(3, 77, C 256, G 2) and (1, 352, C 256, G 8), tile statistics from the test (fp64 -> fp32) and chained behind a 1x1 producer launch.
(The accumulator-side fold of conv_gemm_wp exists behind a tuning hook of the tuning build only and has no row.)

FOUND by these cases and fixed (csrc/conv_gemm_rs.hip): the accumulator-side LayerNorm on conv_gemm_rs read the M2 half of each ln_part pair
as the mean (the compiler turned __builtin_bit_cast of the vector element lp[e][1] into a read of element 0: a dword load in the ISA), so the
pooled variance was that of the 32-channel means alone plus mean / 32.  The acc-rs rows (C = 1024; bf16, fp16, fp32x) missed their gate by
2.8e3 .. 1.5e4 x the bound (element (54, 9): got 56.5, ref 3.936) and returned NaN on rows with a negative mean; conv_gemm_fast and
conv_gemm_wp passed the same arguments.
"""
import ctypes as C

import pytest
import torch

import gemm_epilogue_ref as E
import numerics as nx
from gemm_epilogue_ref import EpiCase, LnCase

pytestmark = pytest.mark.gpu

DTYPES = ("bf16", "fp16", "fp32", "fp32x")
TAG = {"bf16": "bf16", "fp16": "f16", "fp32": "f32", "fp32x": "x3"}


def fam_label(dtype: str, fam: str) -> str:
    """The label of `fam`'s 32x32 kernel in `dtype` (v2: its 64x64 single-tile form).  fp32 has no register-staged kernel: wp takes its rows;
    sk and v2 have no split form: fp32x runs their fp32 kernels."""
    if fam == "rs" and dtype == "fp32":
        fam = "wp"
    tag = "f32" if dtype == "fp32x" and fam in ("sk", "v2") else TAG[dtype]
    return f"conv_gemm_{fam}<{tag},{'64x64' if fam == 'v2' else '32x32'}>"


def _epi_cases():
    cs = []
    for dt in DTYPES:
        # producers: name, dtype, B, L, C, C2, N, taps, stride, pad, up, ops, act, out_f32, want_row, want_gn, mt_ln, regime, label, row, gn
        for B, L in ((1, 32), (1, 45), (2, 32), (7, 37), (3, 63)):
            for Cc, taps, pad in ((256, 1, 0), (128, 3, 1)):
                for N in (32, 64, 96):
                    cs.append(EpiCase("producer", dt, B, L, Cc, 0, N, taps, 1, pad, 1, "br", 0, False, True, True, False, "", fam_label(dt, "rs"), True, True))
        cs.append(EpiCase("producer-up2-s2", dt, 2, 50, 128, 0, 64, 3, 2, 1, 2, "br", 0, False, True, True, False, "", fam_label(dt, "rs"), True, True))
        cs.append(EpiCase("producer-cat", dt, 7, 37, 256, 64, 64, 1, 1, 0, 1, "bra", 0, False, True, True, False, "", fam_label(dt, "rs"), True, True))
        cs.append(EpiCase("producer-short", dt, 4, 20, 256, 0, 64, 1, 1, 0, 1, "br", 0, False, True, True, False, "", fam_label(dt, "rs"), True, False))
        kc = 512 if dt == "fp32x" else 1024      # rs refuses: K = 3 * kc > 2048 (split form: > 1280)
        cs.append(EpiCase("producer-wp", dt, 2, 37, kc, 0, 64, 3, 1, 1, 1, "br", 0, False, True, True, False, "", fam_label(dt, "wp"), True, True))
        cs.append(EpiCase("producer-wp-short", dt, 4, 20, kc, 0, 64, 3, 1, 1, 1, "br", 0, False, True, True, False, "", fam_label(dt, "wp"), True, False))
        # rowpart only
        cs.append(EpiCase("fast-rowpart", dt, 1, 5632, 256, 0, 96, 1, 1, 0, 1, "br", 0, False, True, True, False, "", fam_label(dt, "fast"), True, False))
        cs.append(EpiCase("fast-rowpart", dt, 3, 1877, 128, 0, 96, 3, 1, 1, 1, "br", 0, False, True, True, False, "", fam_label(dt, "fast"), True, False))
        if dt in ("bf16", "fp16"):
            cs.append(EpiCase("mt-rowpart", dt, 7, 1463, 256, 0, 96, 1, 1, 0, 1, "br", 0, False, True, False, True, "", f"conv_gemm_mt<{TAG[dt]},128x128>", True, False))
        # epilogue operands on each family's ragged shape, and a second source
        for fam, (B, L, Cc, N) in (("sk", (5, 25, 96, 24)), ("v2", (5, 25, 64, 24)), ("fast", (3, 2731, 128, 40)), ("wp", (5, 25, 128, 24)), ("rs", (5, 25, 128, 32))):
            for act in range(4):
                for of32 in ((False, True) if dt in ("bf16", "fp16") else (False,)):
                    row = fam == "rs"                          # N % 32 == 0 only there: the row partials are honoured and checked as well
                    cs.append(EpiCase("operands", dt, B, L, Cc, 0, N, 3, 1, 1, 1, "bsra", act, of32, row, False, False, "", fam_label(dt, fam), row, False))
        for fam, (B, L, Cc, C2, N) in (("sk", (5, 25, 96, 160, 24)), ("v2", (5, 25, 64, 64, 24)), ("fast", (3, 2731, 256, 32, 40)), ("wp", (5, 25, 256, 32, 24)),
                                       ("rs", (5, 25, 256, 64, 32))):
            cs.append(EpiCase("cat", dt, B, L, Cc, C2, N, 1, 1, 0, 1, "bsra", 0, False, fam == "rs", False, False, "", fam_label(dt, fam), fam == "rs", False))
    # statistics regimes of the stored output: one rs shape, one wp shape
    for dt in ("bf16", "fp32"):
        for regime in [f"offset:{r:g}" for r in nx.OFFSET_RATIOS] + ["const", "first50"]:
            cs.append(EpiCase("regime", dt, 7, 37, 256, 0, 64, 1, 1, 0, 1, "br", 0, False, True, True, False, regime, fam_label(dt, "rs"), True, True))
    return cs


def _ln_cases():
    cs = []
    for dt in DTYPES:
        rs = fam_label(dt, "rs") if dt != "fp32" else fam_label(dt, "fast")      # fp32: no register-staged kernel, the staged one carries the fold
        fast, prod = fam_label(dt, "fast"), fam_label(dt, "rs")
        cs.append(LnCase("acc-rs", dt, 4, 44, 1024, 96, "acc", 0, rs, prod))
        cs.append(LnCase("acc-fast", dt, 3, 37, 128, 64, "acc", 0, fast, prod))
        cs.append(LnCase("operand-ss", dt, 3, 37, 256, 64, "ss", 0, fast, prod))
        cs.append(LnCase("operand-ss-res", dt, 3, 37, 256, 256, "ss_res", 0, fast, prod))
        cs.append(LnCase("operand-plain", dt, 3, 37, 256, 64, "plain", 0, fast, prod))
        for ratio in nx.OFFSET_RATIOS:
            cs.append(LnCase("acc-rs-offset", dt, 4, 44, 1024, 96, "acc", ratio, rs, prod))
            cs.append(LnCase("operand-ss-offset", dt, 3, 37, 256, 64, "ss", ratio, fast, prod))
    return cs


EPI_CASES = _epi_cases()
LN_CASES = _ln_cases()


def epi_id(c: EpiCase) -> str:
    return (f"{c.name}-{c.dtype}-B{c.B}-L{c.L}-C{c.C}{f'+{c.C2}' if c.C2 else ''}-N{c.N}-k{c.taps}-{c.ops}-act{c.act}{'-f32out' if c.out_f32 else ''}"
            f"{'-' + c.regime if c.regime else ''}")


def ln_id(c: LnCase) -> str:
    return f"{c.name}-{c.dtype}-B{c.B}-L{c.L}-C{c.C}-N{c.N}{f'-ratio{c.ratio:g}' if c.ratio else ''}"


TD = {"fp32": torch.float32, "fp32x": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
_worst = {}
_per_case = []


def _note(key: str, r: float):
    _worst[key] = max(_worst.get(key, 0.0), r)


def _case_line(case_id: str, label: str, ratios: dict):
    _per_case.append(f"{case_id} [{label}]: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


@pytest.fixture(scope="module", autouse=True)
def _report():
    """Worst err / bound per gate and dtype, printed at the end of the module (profiles/gemm_epilogue_test.txt is a copy of it)."""
    yield
    print("\ngemm epilogue gates, err / bound per case:\n" + "\n".join(_per_case))
    print("\ngemm epilogue gates, worst err / bound:\n" + "\n".join(f"{k}: {v:.4f}" for k, v in sorted(_worst.items())))


def _ptr(t):
    return t.data_ptr() if t is not None else None


def launch_epi(lib, _l, c: EpiCase, o: dict, dev):
    """One sf_op_conv1d_epi launch of `c` on operands `o` -> (out, rowpart, gnpart, label) on the device; the outputs NaN-filled beforehand."""
    td = TD[c.dtype]
    t = {k: (o[k].to(td).to(dev) if o[k] is not None else None) for k in ("x", "x2", "res")}
    f = {k: (o[k].to(dev).contiguous() if o[k] is not None else None) for k in ("w", "bias", "bscale", "badd")}
    out = nx.nan_like((c.B, c.Lout, c.N), torch.float32 if c.out_f32 else td, dev)
    mt, nt = (c.M + 31) // 32, max(c.N // 32, 1)
    rowpart = nx.nan_like((c.M, nt, 2), torch.float32, dev) if c.want_row else None
    gnpart = nx.nan_like((mt, nt, 2, 2), torch.float32, dev) if c.want_gn else None
    d = E.epi_desc(c, x=_ptr(t["x"]), x2=_ptr(t["x2"]), w=_ptr(f["w"]), bias=_ptr(f["bias"]), bscale=_ptr(f["bscale"]), badd=_ptr(f["badd"]),
                   residual=_ptr(t["res"]), out=_ptr(out), rowpart=_ptr(rowpart), gnpart=_ptr(gnpart))
    rc, label, row, gn = E.query_epi(d)
    assert rc == 0 and (label, row, gn) == (c.label, c.row, c.gn), f"{epi_id(c)}: the dispatcher takes {(label, row, gn)}, the row is written for {(c.label, c.row, c.gn)}"
    ws = nx.poisoned_workspace(lib.sf_op_conv1d_epi_workspace_bytes(C.byref(d)), dev)
    row_done, gn_done = C.c_int(-1), C.c_int(-1)
    _l.check(lib.sf_op_conv1d_epi(C.byref(d), C.byref(row_done), C.byref(gn_done), ws.data_ptr(), ws.numel(), _l.stream_ptr(dev)), "sf_op_conv1d_epi")
    assert (row_done.value, gn_done.value) == (int(c.row), int(c.gn)), f"{epi_id(c)}: the launch reports {(row_done.value, gn_done.value)}"
    torch.cuda.synchronize()
    if c.want_row and not c.row:
        assert bool(torch.isnan(rowpart).all()), "a declined rowpart buffer was written"
    if c.want_gn and not c.gn:
        assert bool(torch.isnan(gnpart).all()), "a declined gnpart buffer was written"
    return out, (rowpart if c.row else None), (gnpart if c.gn else None), label


@pytest.mark.parametrize("case", EPI_CASES, ids=epi_id)
def test_epilogue(cuda, case):
    from syncfusion_amd import _lib as _l

    lib = _l.load()
    o = E.epi_operands(case)
    out, rowpart, gnpart, label = launch_epi(lib, _l, case, o, cuda)
    ref, bound, _ = E.epi_ref(case, o)
    what = epi_id(case)
    r = E.check(out.float().cpu(), ref, bound, what + " values")
    _note(f"values act{case.act} {case.dtype}", r)
    stored = out.float().cpu().reshape(case.M, case.N)
    fam = E.family(label)
    ratios = {"values": r}
    for k, v in E.check_stats(stored, rowpart.cpu() if rowpart is not None else None, gnpart.cpu() if gnpart is not None else None, case.Lout, what, fam=fam).items():
        _note(f"{k} {case.dtype}", v)
        ratios[k] = v
    _case_line(what, label, ratios)


def launch_ln(lib, _l, c: LnCase, o: dict, src_dev, part_dev, dev, arm_rowpart: bool = False):
    td = TD[c.dtype]
    f = {k: (o[k].to(dev).contiguous() if o.get(k) is not None else None) for k in ("w", "bias", "ss")}
    out = nx.nan_like((c.B, c.L, c.N), td, dev)
    rowpart = nx.nan_like((c.M, c.N // 32, 2), torch.float32, dev) if arm_rowpart else None      # the engine chains these launches
    d = E.ln_desc(c, x=_ptr(src_dev), w=_ptr(f["w"]), bias=_ptr(f["bias"]), out=_ptr(out), ln_part=_ptr(part_dev), ln_ss=_ptr(f["ss"]),
                  residual=_ptr(src_dev) if c.form == "ss_res" else None, rowpart=_ptr(rowpart))
    rc, label, row = E.query_ln(d)
    assert rc == 0 and label == c.label and row == arm_rowpart, f"{ln_id(c)}: the dispatcher takes {(label, row)}, the row is written for {c.label!r}"
    ws = nx.poisoned_workspace(lib.sf_op_conv1d_epi_workspace_bytes(C.byref(d)), dev)
    done = C.c_int(-1)
    _l.check(lib.sf_op_conv1d_ln(C.byref(d), C.byref(done), ws.data_ptr(), ws.numel(), _l.stream_ptr(dev)), "sf_op_conv1d_ln")
    assert done.value == int(arm_rowpart)
    torch.cuda.synchronize()
    return (out, rowpart) if arm_rowpart else out


def ln_producer(c: LnCase) -> EpiCase:
    """The 1x1 launch in front of the chained run: 256 channels -> the consumer's C, residual in the consumer's source regime."""
    return EpiCase("ln-producer", c.dtype, c.B, c.L, 256, 0, c.C, 1, 1, 0, 1, "br", 0, False, True, False, False, f"offset:{c.ratio:g}" if c.ratio else "",
                   c.producer, True, False)


@pytest.mark.parametrize("case", LN_CASES, ids=ln_id)
def test_ln_consumer(cuda, case):
    from syncfusion_amd import _lib as _l

    lib = _l.load()
    o = E.ln_operands(case)
    td = TD[case.dtype]
    # 1. partials computed by the test in fp64, rounded to fp32
    part, e_in, q_in = E.ln_inputs_direct(o["x"])
    # (this run also arms the consumer's OWN row partials, as the engine chains these launches: they are of its stored output)
    out, own = launch_ln(lib, _l, case, o, o["x"].to(td).to(cuda), part.to(cuda).contiguous(), cuda, arm_rowpart=True)
    ref, bound = E.ln_ref(case, o, o["x"], e_in, q_in, case.label)
    r1 = E.check(out.float().cpu().reshape(case.M, case.N), ref, bound, ln_id(case) + " (partials from fp64)")
    own_r = E.check_stats(out.float().cpu().reshape(case.M, case.N), own.cpu(), None, case.L, ln_id(case) + " own", fam=E.family(case.label))
    # 2. chained behind the producer launch that wrote the source and its partials: both sides must agree on the layout
    p = ln_producer(case)
    po = E.epi_operands(p, seed=1)
    src_dev, rowpart, _, _ = launch_epi(lib, _l, p, po, cuda)
    src = src_dev.float().cpu()
    E.check_stats(src.reshape(p.M, p.N), rowpart.cpu(), None, p.Lout, ln_id(case) + " producer", fam=E.family(p.label))
    out2 = launch_ln(lib, _l, case, o, src_dev, rowpart, cuda)
    e_in2, q_in2 = E.ln_inputs_chained(src)
    ref2, bound2 = E.ln_ref(case, o, src, e_in2, q_in2, case.label)
    r2 = E.check(out2.float().cpu().reshape(case.M, case.N), ref2, bound2, ln_id(case) + " (chained)")
    _note(f"ln {case.form} {case.dtype}", max(r1, r2))
    for k, v in own_r.items():
        _note(f"ln own {k} {case.dtype}", v)
    _case_line(ln_id(case), case.label, {"fp64 partials": r1, "chained": r2, **{"own " + k: v for k, v in own_r.items()}})
    print(f"{case.label}: err/bound {r1:.3f} (fp64 partials), {r2:.3f} (chained behind {p.label})")


def test_c_act(cuda):
    """The measurement behind gemm_epilogue_ref.C_ACT: the error of the device's erff / expf / division alone.  The fp32 sk case run with act 0
    gives the device's own y bit for bit (same kernel, same operands), so |dev - act64(y_dev)| / (u |y_dev|) isolates apply_act's arithmetic.
    Asserts that the constant in use is at least 2 x the value measured now (it was fixed at 4 x the first measurement)."""
    from syncfusion_amd import _lib as _l

    lib = _l.load()
    base = next(c for c in EPI_CASES if c.name == "operands" and c.dtype == "fp32" and "sk" in c.label and c.act == 0)
    o = E.epi_operands(base)
    y, _, _, _ = launch_epi(lib, _l, base, o, cuda)
    y = y.double().cpu()
    for act in (2, 3):
        c = base._replace(act=act)
        out, _, _, _ = launch_epi(lib, _l, c, o, cuda)
        err = (out.double().cpu() - E.act64(y, act)).abs() / (E.u * y.abs().clamp_min(1e-30))
        m = float(err.max())
        _note(f"c_act measured act{act}", m)
        print(f"act {act}: max |dev - act64(y_dev)| / (u |y_dev|) = {m:.3f}; C_ACT = {E.C_ACT[act]:.3f}")
        assert 2.0 * m <= E.C_ACT[act], f"act {act}: measured {m:.3f}, C_ACT {E.C_ACT[act]:.3f} leaves less than 2 x"


# ---------------------------------------------------------------------------------------------------------------------------------
# conv_cb prologue 2: the one consumer of gnpart (sf_op_conv_cb_tiles)
# ---------------------------------------------------------------------------------------------------------------------------------
CB_TOL = {"bf16": 2e-2, "fp16": 4e-3, "fp32x": 2e-5}          # test_gpu_numerics.test_conv_cb_chain_offset's gates on h
CB_SHAPES = ((2, 44, 128, 4), (3, 77, 256, 2), (1, 352, 256, 8))   # (B, L, C, G)
CB_CASES = [(dt, shape, src) for dt in ("bf16", "fp16", "fp32x") for shape in CB_SHAPES for src in ("fp64", "chained")]


def cb_producer(dtype: str, shape) -> EpiCase:
    """The 1x1 launch in front of the chained run, as the engine chains InjectChannels into the next item: 256 channels -> C with a residual."""
    B, L, Cc, _ = shape
    return EpiCase("cb-producer", dtype, B, L, 256, 0, Cc, 1, 1, 0, 1, "br", 0, False, False, True, False, "", fam_label(dtype, "rs"), False, True)


@pytest.mark.parametrize("dtype,shape,source", CB_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_conv_cb_tiles(cuda, dtype, shape, source):
    """h = conv3(SiLU(GroupNorm(x))) + b through conv_cb's tile-statistics prologue and cb_reduce_gn, per element (numerics.check_close at the
    channel-block tests' tolerance) against fp64 from the rows the launch reads.  source = fp64: the tile statistics are the test's, fp64
    rounded to fp32 in gnpart's layout; chained: x and the statistics both come from a producer launch's epilogue, so the prologue must read
    the (m tile, n tile, segment, 2) layout gn_tile_stats writes and pool the two segments of a tile to the right clips.  The reducer's chunk
    statistics of the stored h are held to test_cb_direct_statistics' bound (the same bits by contract), chunk by chunk (ragged last chunk)."""
    from syncfusion_amd import _lib as _l

    lib = _l.load()
    B, L, Cc, G = shape
    td = TD[dtype]
    T = E.R.STORE[dtype]
    g = torch.Generator().manual_seed(B * 1000 + L + Cc)
    if source == "fp64":
        x = E.clip_input(B, L, Cc, g, T)
        x_dev = x.to(td).to(cuda)
        ts_dev = E.gnpart64(x.reshape(B * L, Cc), L)[0].float().to(cuda).contiguous()
    else:
        p = cb_producer(dtype, shape)
        x_dev, _, ts_dev, _ = launch_epi(lib, _l, p, E.epi_operands(p, seed=2), cuda)
        x = x_dev.float().cpu()
        E.check_stats(x.reshape(B * L, Cc), None, ts_dev.cpu(), L, "cb producer", fam=E.family(p.label))
    w = torch.randn(Cc, Cc, 3, generator=g) / (3 * Cc) ** 0.5
    bias, gam, bet = torch.randn(Cc, generator=g) * 0.1, 1 + 0.2 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    keep = [t.contiguous().to(cuda) for t in (w, bias, gam, bet)]
    h = nx.nan_like((B, L, Cc), td, cuda)
    stats = nx.nan_like((B * 32 * G * 2,), torch.float32, cuda)           # (B, nch, G, 2) with nch <= 32: the tail must stay NaN
    nbytes = lib.sf_op_conv_cb_tiles_workspace_bytes(_l.DTYPES[dtype], B, L, Cc)
    assert nbytes > 0
    ws = nx.poisoned_workspace(nbytes, cuda)
    nch, rows = C.c_int(-1), C.c_int(-1)
    _l.check(lib.sf_op_conv_cb_tiles(_l.DTYPES[dtype], x_dev.data_ptr(), *[t.data_ptr() for t in keep], G, 1e-5, ts_dev.data_ptr(), B, L, Cc,
                                     h.data_ptr(), stats.data_ptr(), C.byref(nch), C.byref(rows), ws.data_ptr(), ws.numel(), _l.stream_ptr(cuda)),
             "sf_op_conv_cb_tiles")
    torch.cuda.synchronize()
    F = torch.nn.functional
    a = F.silu(F.group_norm(x.double().transpose(1, 2), G, gam.double(), bet.double(), eps=1e-5))
    wr = w.to(td).double() if T != "fp32" else w.double()
    h_ref = (F.conv1d(a, wr, bias.double(), padding=1)).transpose(1, 2)
    hs = h.float().cpu()
    rel = nx.check_close(hs, h_ref, CB_TOL[dtype], f"conv_cb tiles {dtype} {shape} {source}", k=nx.MAX_K16 if T != "fp32" else nx.MAX_K)
    _note(f"conv_cb tiles rel-L2 {dtype}", rel)
    # the reducer's chunk statistics of the STORED h
    nch, rows = nch.value, rows.value
    assert nch * rows >= L > (nch - 1) * rows and nch <= 32
    used = B * nch * G * 2
    st = stats[:used].reshape(B, nch, G, 2).double().cpu()
    assert bool(torch.isfinite(st).all()) and bool(torch.isnan(stats[used:]).all())
    cpg = Cc // G
    worst = 0.0
    for ch in range(nch):
        blk = hs.double()[:, ch * rows:min(L, (ch + 1) * rows)].reshape(B, -1, G, cpg)
        n = blk.shape[1] * cpg
        mean64 = blk.mean(dim=(1, 3))
        m2_64 = (blk - mean64[:, None, :, None]).pow(2).sum(dim=(1, 3))
        gam_n, gam_n3 = n * E.u / (1 - n * E.u), (n + 3) * E.u / (1 - (n + 3) * E.u)
        b_mean = gam_n * blk.abs().mean(dim=(1, 3))
        b_m2 = gam_n3 * m2_64 + (1 + gam_n3) * n * b_mean.pow(2)
        worst = max(worst, E.check(st[:, ch, :, 0], mean64, b_mean, f"chunk {ch} mean"), E.check(st[:, ch, :, 1], m2_64, b_m2, f"chunk {ch} M2"))
    _note(f"conv_cb tiles chunk statistics {dtype}", worst)
    _case_line(f"conv_cb-tiles-{dtype}-{'x'.join(map(str, shape))}-{source}", "conv_cb pro 2 + cb_reduce_gn", {"h rel-L2 / tol": rel / CB_TOL[dtype], "chunk statistics": worst})
