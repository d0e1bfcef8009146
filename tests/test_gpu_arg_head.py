"""Argument heads (MI355X): the kernels whose launch-critical arguments travel as leading scalar parameters in front of their argument
block (kernels.h, "argument heads": conv_gemm_rs, conv_cb) at RAGGED shapes, against torch in fp64.  conv_gemm_fast keeps its block-first
signature; its cases stay as the neighbour the plan falls to from 513 tiles on.

A head field that is swapped with a same-typed neighbour, or left stale, does not show at the workload's shapes (M, N and L multiples of
the tiles, equal clip lengths everywhere): it shows where M is not a multiple of 32 or below 32, L is not a multiple of 32, the last
column tile is ragged, a second source is concatenated, the stride is not 1 (with and without an upsampled source, so that Lout != Lsrc
is among the cases) and a geometry the head's packed dword cannot hold (stride 16) goes to another kernel.  Every case goes through the
op-level entry points of the existing op tests (test_gpu_ops.py, test_gpu_cb_direct.py) and is held to the tolerance the existing test
of its family uses: test_gpu_ops.TOL for the 16-bit types and the channel-block chain, and the fp64 gates of
test_conv_gemm_fp32x_against_fp64 (fp32 2e-6, fp32x 1e-6) for the fp32 GEMMs.  The references are fp64 from the same dtype-rounded inputs.

What the op level cannot reach is left to the engine case at the end: the tile-statistics prologue of conv_cb (pro 2; only the engine
arms ConvGemmArgs::gnpart_out), a concatenated second source in the fp32 types (sf_op_inject_prenorm_proj is 16-bit only), and the
hosted-prefetch branch of every kernel; the engine case asserts that the changed families are on its path.  The conv_cb ops take dense
rows (src_ld == N == C), so a swap of those two adjacent head fields is not visible here.  conv_cb
needs clips of at least 44 positions, so it has no M < 32 case, and its direct epilogues refuse L = 32: that refusal is asserted.
conv_gemm_fast is reached by the automatic plan from 513 tiles of 32 x 32 on, so it has no M < 32 case either.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_gpu_ops import TD, TOL

pytestmark = pytest.mark.gpu

GEMM_TOL = {"bf16": TOL["bf16"], "fp32": 2e-6, "fp32x": 1e-6}


def _lib():
    from syncfusion_amd import _lib

    return _lib, _lib.load()


def _rel(got, ref):
    return float((got.double() - ref).norm() / ref.norm())


def _label(dtype, B, L, C, N, taps, stride, pad, up):
    _l, lib = _lib()
    buf = ctypes.create_string_buffer(128)
    _l.check(lib.sf_op_conv1d_variant(_l.DTYPES[dtype], B, L, C, N, taps, stride, pad, up, 0, buf, 128), "sf_op_conv1d_variant")
    return buf.value.decode()


# ----------------------------------------------------------------------------------------------------------
# conv_gemm_rs / conv_gemm_fast through sf_op_conv1d_cl
# ----------------------------------------------------------------------------------------------------------
GEMM_CASES = [
    # family the 16-bit / fp32x launch takes, (B, L, C, N, taps, stride, pad, up), residual
    ("conv_gemm_rs", (1, 19, 256, 64, 1, 1, 0, 1), True),        # one clip, M = 19 < 32, one tap
    ("conv_gemm_rs", (3, 37, 256, 64, 3, 1, 1, 1), False),       # three clips of 37, M = 111, three taps: tiles straddle clips
    ("conv_gemm_rs", (1, 45, 128, 96, 3, 1, 1, 1), True),        # one clip, M = 45, three column tiles
    ("conv_gemm_rs", (2, 50, 128, 96, 3, 2, 1, 2), True),        # stride 2 over a nearest x2 source (up_shift 1), M = 100
    ("conv_gemm_rs", (2, 51, 128, 96, 3, 2, 1, 1), True),        # stride 2, no upsampling: Lout = 26 != Lsrc = 51, M = 52
    ("conv_gemm_rs", (3, 39, 64, 64, 4, 4, 0, 1), False),        # patchify, taps = stride = 4, no padding: Lout = 9, M = 27 < 32
    ("conv_gemm_fast", (1, 2001, 256, 296, 1, 1, 0, 1), True),   # one clip, M = 2001, one tap, ragged last column tile (296 = 9 x 32 + 8)
    ("conv_gemm_fast", (3, 667, 128, 328, 3, 1, 1, 1), False),   # three clips of 667, three taps, ragged N
    ("conv_gemm_fast", (3, 500, 128, 360, 3, 2, 1, 2), True),    # stride 2 with up_shift 1, ragged N
]
_GEMM_REF = {}


def _gemm_inputs(dtype, shape, residual):
    """inputs and the fp64 reference of one case, built once per (rounding, shape)"""
    key = (TD[dtype], shape, residual)
    if key in _GEMM_REF:
        return _GEMM_REF[key]
    B, L, C, N, taps, stride, pad, up = shape
    td = TD[dtype]
    g = torch.Generator().manual_seed(L * 7 + N)
    x = torch.randn(B, C, L, generator=g) * 1.5 + 0.3
    w = torch.randn(N, C, taps, generator=g) / (C * taps) ** 0.5
    bias = torch.randn(N, generator=g) * 0.1
    h = x.to(td).double()
    if up > 1:
        h = F.interpolate(h, scale_factor=up, mode="nearest")
    ref = F.conv1d(h, w.to(td).double(), bias.double(), stride=stride, padding=pad)
    res = torch.randn(B, N, ref.shape[-1], generator=g) if residual else None
    if residual:
        ref = ref + res.to(td).double()
    _GEMM_REF[key] = (x, w, bias, res, ref)
    return _GEMM_REF[key]


@pytest.mark.parametrize("dtype", ["bf16", "fp32", "fp32x"])
@pytest.mark.parametrize("family,shape,residual", GEMM_CASES, ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}" for c in GEMM_CASES])
def test_gemm_heads_ragged(cuda, dtype, family, shape, residual):
    _l, lib = _lib()
    B, L, C, N, taps, stride, pad, up = shape
    label = _label(dtype, *shape)
    if dtype != "fp32" or family == "conv_gemm_fast":   # (plain fp32 has no register-staged form: those launches take the wave-private kernel)
        assert label.startswith(family), label
    td = TD[dtype]
    x, w, bias, res, ref = _gemm_inputs(dtype, shape, residual)
    Lout = ref.shape[-1]
    xd = x.transpose(1, 2).contiguous().to(td).to(cuda)
    rd = res.transpose(1, 2).contiguous().to(td).to(cuda) if residual else None
    out = torch.full((B, Lout, N), float("nan"), dtype=td, device=cuda)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=cuda)
    wd, bd = w.to(cuda), bias.to(cuda)
    _l.check(lib.sf_op_conv1d_cl(_l.DTYPES[dtype], xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), None, None, 0, 1e-5, rd.data_ptr() if residual else None,
                                 B, L, C, N, taps, stride, pad, up, out.data_ptr(), ws.data_ptr(), ws.numel(), _l.stream_ptr(cuda)), "sf_op_conv1d_cl")
    torch.cuda.synchronize()
    e = _rel(out.cpu().transpose(1, 2), ref)
    print(f"{label} {dtype} {shape}: rel-L2 vs fp64 {e:.3e}")
    assert e < GEMM_TOL[dtype]


@pytest.mark.parametrize("dtype", ["bf16", "fp32", "fp32x"])
def test_stride_16_leaves_the_register_staged_kernel(cuda, dtype):
    """A patchify convolution with taps = stride = 16 (K = 512, fragment-ordered weights at hand) is a register-staged shape in everything
    but its stride, which the head's packed geometry dword (4 bits) cannot hold: the plan must name another kernel, and the op computes it."""
    _l, lib = _lib()
    shape = (2, 16 * 23 + 5, 32, 64, 16, 16, 0, 1)   # Lout = 23, M = 46; five trailing positions no window reaches
    B, L, C, N, taps, stride, pad, up = shape
    label = _label(dtype, *shape)
    assert not label.startswith("conv_gemm_rs"), label
    td = TD[dtype]
    x, w, bias, _, ref = _gemm_inputs(dtype, shape, False)
    assert ref.shape[-1] == 23
    xd = x.transpose(1, 2).contiguous().to(td).to(cuda)
    out = torch.full((B, 23, N), float("nan"), dtype=td, device=cuda)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=cuda)
    wd, bd = w.to(cuda), bias.to(cuda)
    _l.check(lib.sf_op_conv1d_cl(_l.DTYPES[dtype], xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), None, None, 0, 1e-5, None,
                                 B, L, C, N, taps, stride, pad, up, out.data_ptr(), ws.data_ptr(), ws.numel(), _l.stream_ptr(cuda)), "sf_op_conv1d_cl")
    torch.cuda.synchronize()
    e = _rel(out.cpu().transpose(1, 2), ref)
    print(f"{label} {dtype} {shape}: rel-L2 vs fp64 {e:.3e}")
    assert e < GEMM_TOL[dtype]


# ----------------------------------------------------------------------------------------------------------
# the concatenated second source (cin2 > 0) and the LayerNorm consumer: sf_op_inject_prenorm_proj (16-bit types)
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [
    # B, L, C, C2, N
    (1, 19, 256, 64, 96),     # one clip, M = 19 < 32: K = 320, five fragments per wave, the second source is the last of them
    (3, 37, 256, 64, 96),     # three clips of 37, M = 111
    (3, 37, 128, 32, 64),     # K = 160: not a multiple of 64, the staged 32x32 kernels
    (3, 667, 384, 64, 320),   # 756 tiles: the staged kernel (conv_gemm_fast) with the second source, M = 2001
])
def test_second_source_heads_ragged(cuda, dtype, shape):
    _l, lib = _lib()
    B, L, C, C2, N = shape
    td = TD[dtype]
    g = torch.Generator().manual_seed(B * 1000 + L + C)
    m = torch.randn(B, L, C, generator=g) * 1.3 + 0.4
    ctx = torch.randn(B, L, C2, generator=g)
    w_inj = torch.randn(C, C + C2, generator=g) / (C + C2) ** 0.5
    b_inj = torch.randn(C, generator=g) * 0.1
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    w_q = torch.randn(N, C, generator=g) / C ** 0.5
    mr, cr = m.to(td).double(), ctx.to(td).double()
    z_ref = mr + F.linear(torch.cat([mr, cr], dim=-1), w_inj.to(td).double(), b_inj.double())
    q_ref = F.linear(F.layer_norm(z_ref.to(td).double(), (C,), gamma.double(), beta.double(), eps=1e-5), w_q.double())
    dev = lambda t: t.contiguous().to(cuda)   # noqa: E731
    md, cd = dev(m.to(td)), dev(ctx.to(td))
    z = torch.full((B, L, C), float("nan"), dtype=td, device=cuda)
    q = torch.full((B, L, N), float("nan"), dtype=td, device=cuda)
    n = lib.sf_op_inject_prenorm_proj_workspace_bytes(B, L, C, C2, N)
    assert n > 0
    ws = torch.empty(n, dtype=torch.uint8, device=cuda)
    fused = ctypes.c_int(-1)
    args = [dev(t) for t in (w_inj, b_inj, gamma, beta, w_q)]
    _l.check(lib.sf_op_inject_prenorm_proj(_l.DTYPES[dtype], md.data_ptr(), cd.data_ptr(), args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(),
                                           args[3].data_ptr(), 1e-5, args[4].data_ptr(), B, L, C, C2, N, z.data_ptr(), q.data_ptr(), ctypes.byref(fused),
                                           ws.data_ptr(), ws.numel(), _l.stream_ptr(cuda)), "sf_op_inject_prenorm_proj")
    torch.cuda.synchronize()
    ez, eq = _rel(z.cpu(), z_ref), _rel(q.cpu(), q_ref)
    print(f"inject + pre-norm projection {dtype} {shape}: fused {fused.value}, z {ez:.3e}, q {eq:.3e}")
    assert ez < TOL[dtype] and eq < TOL[dtype]


# ----------------------------------------------------------------------------------------------------------
# conv_cb: the slab chain (prologue 0 in the first convolution, 1 in the second; one and two row tiles; one and two channel blocks)
# ----------------------------------------------------------------------------------------------------------
CB_SHAPES = [
    # B, L, C, modulated, channel blocks per workgroup
    (1, 45, 128, False, 1),    # one clip, 45 rows: one row tile per workgroup, a single channel slice
    (3, 45, 256, True, 1),     # three clips of 45, M = 135: row tiles straddle clips
    (7, 83, 512, True, 1),     # M = 581: ten 64-row workgroups x 16 weight slices = 160 -> two row tiles per workgroup, the last one ragged
    (3, 61, 512, True, 2),     # two channel blocks per workgroup (16-bit types: the split-operand form takes one)
]


@pytest.mark.parametrize("dtype,shape", [(d, s) for d in ("bf16", "fp32x") for s in CB_SHAPES if not (d == "fp32x" and s[4] == 2)])
def test_conv_cb_heads_ragged(cuda, dtype, shape):
    _l, lib = _lib()
    B, L, C, mod, kb = shape
    G = 8
    td = TD[dtype]
    g = torch.Generator().manual_seed(B * 1000 + L + C)
    x = torch.randn(B, C, L, generator=g) * 1.3 + 0.2
    w1 = torch.randn(C, C, 3, generator=g) / (3 * C) ** 0.5
    w2 = torch.randn(C, C, 3, generator=g) / (3 * C) ** 0.5
    b1, b2 = torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    gam = [1 + 0.2 * torch.randn(C, generator=g) for _ in range(2)]
    bet = [0.1 * torch.randn(C, generator=g) for _ in range(2)]
    ss = torch.randn(B, 2 * C, generator=g) * 0.3 if mod else None
    d = lambda t: t.double()   # noqa: E731
    xr = x.to(td).double()
    h_ref = F.conv1d(F.silu(F.group_norm(xr, G, d(gam[0]), d(bet[0]), eps=1e-5)), w1.to(td).double(), d(b1), padding=1)
    y = xr + F.conv1d(F.silu(F.group_norm(h_ref, G, d(gam[1]), d(bet[1]), eps=1e-5)), w2.to(td).double(), d(b2), padding=1)
    m_ref = F.layer_norm(y.transpose(1, 2), (C,), eps=1e-6)
    if mod:
        m_ref = m_ref * (1 + d(ss)[:, None, :C]) + d(ss)[:, None, C:]
    dev = lambda t: t.to(cuda)   # noqa: E731
    x_cl = dev(x.transpose(1, 2).contiguous().to(td))
    h = torch.full((B, L, C), float("nan"), dtype=td, device=cuda)
    m = torch.full((B, L, C), float("nan"), dtype=td, device=cuda)
    nbytes = lib.sf_op_resnet_mod_cb_workspace_bytes(B, L, C)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    keep = [dev(t) for t in (w1, b1, w2, b2, gam[0], bet[0], gam[1], bet[1])]
    ssd = dev(ss) if mod else None
    _l.check(lib.sf_op_resnet_mod_cb(_l.DTYPES[dtype], x_cl.data_ptr(), *[t.data_ptr() for t in keep], G, 1e-5, ssd.data_ptr() if mod else None, 1e-6,
                                     B, L, C, kb, h.data_ptr(), m.data_ptr(), ws.data_ptr(), ws.numel(), _l.stream_ptr(cuda)), "sf_op_resnet_mod_cb")
    torch.cuda.synchronize()
    e_h, e_m = _rel(h.cpu().transpose(1, 2), h_ref), _rel(m.cpu(), m_ref)
    print(f"conv_cb chain {dtype} {shape}: h {e_h:.3e}  m {e_m:.3e}")
    assert e_h < TOL[dtype] and e_m < TOL[dtype]


# ----------------------------------------------------------------------------------------------------------
# conv_cb: the direct epilogues at C = N = 128 (sf_op_resnet_mod_cbd, with the InjectChannels GEMM over cat[m, ctx] behind them)
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [
    # B, L, G, modulated (the shapes of test_gpu_cb_direct: its inputs are shared)
    (1, 64, 8, True),        # one clip, two row tiles
    (3, 96, 8, True),        # three clips of three tiles
    (3, 96, 2, False),       # a group spans two waves, plain LayerNorm
    (10, 1024, 8, True),     # 10240 rows: two row tiles per workgroup
])
def test_conv_cb_direct_heads(cuda, dtype, shape):
    from test_gpu_cb_direct import C, C2, _case, _run_direct

    B, L, G, mod = shape
    td = TD[dtype]
    c = _case(dtype, shape)
    w1, b1, w2, b2, g1, be1, g2, be2 = [t.double() for t in c["params"]]
    xr = c["x"].double().transpose(1, 2)
    h_ref = F.conv1d(F.silu(F.group_norm(xr, G, g1, be1, eps=1e-5)), w1.to(td).double(), b1, padding=1)
    y = xr + F.conv1d(F.silu(F.group_norm(h_ref, G, g2, be2, eps=1e-5)), w2.to(td).double(), b2, padding=1)
    m_ref = F.layer_norm(y.transpose(1, 2), (C,), eps=1e-6)
    if mod:
        m_ref = m_ref * (1 + c["ss"].double()[:, None, :C]) + c["ss"].double()[:, None, C:]
    m16 = m_ref.to(td).double()
    cat = torch.cat([m16, c["ctx"][..., :C2].double()], dim=-1)
    z_ref = m16 + cat @ c["wi"].to(td).double().t() + c["bi"].double() + c["badd"].double()[:, None, :]
    h, m, z, _ = _run_direct(cuda, dtype, shape, True)
    e_h, e_m, e_z = _rel(h.cpu().transpose(1, 2), h_ref), _rel(m.cpu(), m_ref), _rel(z.cpu(), z_ref)
    print(f"conv_cb direct {dtype} {shape}: h {e_h:.3e}  m {e_m:.3e}  z {e_z:.3e}")
    assert e_h < TOL[dtype] and e_m < TOL[dtype] and e_z < TOL[dtype]


def test_conv_cb_direct_refuses_clips_of_32(cuda):
    """C = N = 128 at L = 32: conv_cb stages panels that may touch four clips only from 44 positions per clip on (conv_cb_shape_ok), so the
    direct epilogues do not exist there: a non-zero code, nothing written."""
    _l, lib = _lib()
    B, L, Cx = 2, 32, 128
    t = torch.zeros(B, L, Cx, dtype=torch.bfloat16, device=cuda)
    f = torch.zeros(3 * Cx * Cx + 2 * B * Cx, device=cuda)
    outs = [torch.full((B, L, Cx), 7.0, dtype=torch.bfloat16, device=cuda) for _ in range(2)]
    stats = torch.full((B * 64 * 8 * 2,), 7.0, device=cuda)
    ws = torch.full((1 << 20,), 7, dtype=torch.uint8, device=cuda)
    rc = lib.sf_op_resnet_mod_cbd(_l.DTYPES["bf16"], t.data_ptr(), *[f.data_ptr()] * 8, 8, 1e-5, None, 1e-6, B, L, Cx, None, None, None, Cx, 0, None,
                                  outs[0].data_ptr(), outs[1].data_ptr(), None, stats.data_ptr(), ws.data_ptr(), ws.numel(), _l.stream_ptr(cuda))
    torch.cuda.synchronize()
    assert rc != 0
    assert all(bool((o == 7.0).all()) for o in outs) and bool((stats == 7.0).all()) and bool((ws == 7).all())


# ----------------------------------------------------------------------------------------------------------
# engine level: the full-size net at (B, L0) = (1, 1024)
# ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_model(cuda):
    from helpers import reference_model_config
    import syncfusion_amd as sa

    torch.manual_seed(1234)
    return sa.instantiate(reference_model_config()).to(cuda)


@pytest.mark.parametrize("L0", [1024, 45056])
def test_engine_one_clip_bf16(cuda, full_model, L0):
    """One evaluation of the full-size 16-bit engine at one clip: its launches host real weight prefetches (the extra workgroups behind a
    kernel's own grid take the `blockIdx >= tiles` branch in front of everything else), the concatenated second source and the
    tile-statistics prologue run with the engine's own arguments.  1024 samples: every GEMM of the deep levels is a register-staged
    launch of a few rows; 45056: the channel-block chains and the staged kernel are on the path too (the counts are printed).  Two calls
    are equal bit for bit, and the result is the fp32 engine's within the one-evaluation gate of test_gpu_models (LOWP_EVAL_TOL)."""
    from helpers import rel_l2
    from test_gpu_models import LOWP_EVAL_TOL, _compute_dtype, _full_inputs

    model = full_model
    x, sigma, emb, chans = _full_inputs(model, 1, L0, 83)
    gx, gs, ge, gc = x.to(cuda), sigma.to(cuda), emb.to(cuda), [t.to(cuda) for t in chans]
    with _compute_dtype(model, "fp32") as net:
        out32 = net(gx, gs, embedding=ge, channels=gc).cpu()
    with _compute_dtype(model, "bf16") as net:
        recs = net.engine().profile_forward(gx, gs, gc, ge, 1.0)
        a = net(gx, gs, embedding=ge, channels=gc).cpu()
        b = net(gx, gs, embedding=ge, channels=gc).cpu()
        count = net.engine().launch_count()
    labels = [r[0] for r in recs]
    heads = {k: sum(1 for s in labels if s.startswith(k)) for k in ("conv_gemm_rs", "conv_gemm_fast", "conv_cb")}
    e = rel_l2(a, out32)
    print(f"bf16 engine at (1, {L0}): {count} launches per evaluation, {heads}; output vs the fp32 engine rel-L2 {e:.3e}")
    assert heads["conv_gemm_rs"] > 0, heads
    if L0 == 45056:
        assert heads["conv_cb"] > 0, heads
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a, b), "two evaluations of the same inputs differ"
    assert e < LOWP_EVAL_TOL["bf16"]
