"""Normalisation statistics and softmax at the inputs where they go wrong (MI355X): groups and rows whose mean is large next to their
spread, near-constant ("dead") and constant groups, and peaked attention scores -- each kernel against fp64 torch on the CPU from the
same dtype-rounded inputs.  The regimes, references and gates are in numerics.py; test_numerics_cpu.py shows that a one-pass variance
fails these gates and a shifted one passes them.

Gates: the existing per-test tolerances (test_gpu_ops.py) at mean/std <= 30; at larger ratios, for fp32 and fp32x,
max(tolerance, 8 * 2^-24 * mean/std) (numerics.offset_gate: what an exact-but-fp32 mean reaches).  Every check is the whole-tensor
rel-L2 plus max|err| <= 8 * gate * rms(ref), naming the worst (clip, row, channel).  Outputs start as NaN, workspaces as 0xFF bytes.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import numerics as nx

pytestmark = pytest.mark.gpu

TD = {"fp32": torch.float32, "fp32x": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
REGIMES = ["offset:3", "offset:30", "offset:300", "dead:1", "dead:4", "const"]


def _lib():
    from syncfusion_amd import _lib

    return _lib, _lib.load()


def _ratio(regime):
    kind, _, val = regime.partition(":")
    return {"offset": lambda: float(val), "dead": lambda: 1e3, "const": lambda: 1.0}[kind]()


def _k(dtype):
    return nx.MAX_K16 if dtype in ("bf16", "fp16") else nx.MAX_K


def _gate(dtype, tol16, tol32, regime):
    """16-bit types: the existing tolerance.  fp32 / fp32x: the existing tolerance up to mean/std 30, then 8 * 2^-24 * mean/std."""
    if dtype in ("bf16", "fp16"):
        return tol16
    r = _ratio(regime)
    return tol32 if r <= 30 else nx.offset_gate(tol32, r)


# ----------------------------------------------------------------------------------------------------------------------------------
# GroupNorm + SiLU materialised (norms.hip): the chunked form (gn_stats -> gn_silu_apply), the register-resident form, the pivot form
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("B,L,C,with_ws,form", [
    (2, 2048, 256, True, "chunked"),       # gn_stats + apply: 32 chunks of 64 rows
    (3, 1000, 512, True, "chunked"),       # ragged last chunk
    (2, 64, 4096, True, "ws-wide"),        # wide rows (C / V > 256 vectors): gn_stats' per-group branch when the chunked form is taken
    (3, 44, 1024, False, "register"),      # register-resident two-pass kernel (control)
    (1, 4096, 256, False, "pivot"),        # one workgroup per (clip, group), pivot-shifted sums (control)
])
def test_gn_silu_offset(cuda, dtype, regime, B, L, C, with_ws, form):
    _l, lib = _lib()
    G = 8
    td = TD[dtype]
    g = torch.Generator().manual_seed(B * 7 + L + C)
    x = nx.grouped_input(B, L, C, G, regime, g, td)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ref = nx.gn_silu_cl64(x, G, gamma, beta, 1e-5)
    xd, gd, bd = x.to(td).to(cuda), gamma.to(cuda), beta.to(cuda)
    out = nx.nan_like(xd.shape, td, cuda)
    ws = nx.poisoned_workspace(B * 32 * G * 2 * 4, cuda) if with_ws else None
    _l.check(lib.sf_op_gn_silu(_l.DTYPES[dtype], xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), G, 1e-5, B, L, C, out.data_ptr(),
                               ws.data_ptr() if with_ws else None, ws.numel() if with_ws else 0, _l.stream_ptr(cuda)), "sf_op_gn_silu")
    torch.cuda.synchronize()
    # measured fp32 rel-L2 (every form alike): 1.5e-7 / 9.8e-7 / 8.4e-6 at mean/std 3 / 30 / 300 (gates 2e-6 / 2e-6 / 1.4e-4), 3.4e-5 on
    # dead groups (gate 4.8e-4), 4.2e-8 on constant ones (gate 2e-6); bf16 / fp16 <= 1.8e-3 / 2.3e-4 (gate 6e-3).  The one-pass chunk
    # statistics measured 1.0e-3 at mean/std 300, 6.9e-3 on dead groups, 3.4e-4 on constant groups
    nx.check_close(out.float().cpu(), ref, _gate(dtype, 6e-3, 2e-6, regime), f"gn_silu {form} {dtype} {regime} B={B} L={L} C={C}", k=_k(dtype))


# ----------------------------------------------------------------------------------------------------------------------------------
# Convolutions with the GroupNorm+SiLU prologue (sf_op_conv1d_cl, groups > 0): every family the dispatcher picks for these shapes
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("regime", ["offset:30", "offset:300", "dead:4"])
@pytest.mark.parametrize("shape", [
    # B, L, C, N, taps, groups, residual
    (2, 352, 64, 64, 3, 8, True),        # ResnetItem conv, 64x64 tiles
    (3, 704, 128, 128, 3, 8, True),      # 128-wide tiles
    (2, 1408, 32, 32, 3, 8, False),      # BN = 32 tiles
    (2, 44, 256, 256, 3, 8, True),       # short clips: tiles span several clips
    (1, 1000, 64, 96, 3, 4, False),      # ragged M, N not a tile multiple
    (8, 5632, 64, 128, 3, 8, True),      # long activations: macro tiles
    (4, 88, 1024, 1024, 3, 8, True),     # deep conv, few rows: wave-private split-K
    (2, 2816, 8, 8, 3, 8, True),         # U-Net depth 0 (thin / direct / depth-0 kernels)
    (2, 2816, 32, 32, 3, 8, True),       # depth-1 width, long clips
    (2, 640, 2, 2, 3, 2, True),          # Encoder1d ResnetBlock1d(groups=2)
])
def test_conv1d_groupnorm_prologue_offset(cuda, dtype, regime, shape):
    _l, lib = _lib()
    B, L, C, N, taps, G, residual = shape
    td = TD[dtype]
    g = torch.Generator().manual_seed(B * 1000 + L + C)
    x = nx.grouped_input(B, L, C, G, regime, g, td)                       # (B, L, C), dtype-rounded
    w = torch.randn(N, C, taps, generator=g) / (C * taps) ** 0.5
    bias = torch.randn(N, generator=g) * 0.1
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    res = torch.randn(B, L, N, generator=g).to(td).float() if residual else None
    wr = w.to(td).float() if C % 32 == 0 else w                            # the 16-bit GEMMs round their weights, the thin kernels do not
    ref = F.conv1d(nx.gn_silu_cl64(x, G, gamma, beta, 1e-5).transpose(1, 2), wr.double(), bias.double(), padding=taps // 2).transpose(1, 2)
    if residual:
        ref = ref + res.double()
    x_cl = x.to(td).to(cuda)
    res_cl = res.to(td).to(cuda) if residual else None
    out = nx.nan_like((B, L, N), td, cuda)
    ws = nx.poisoned_workspace(64 << 20, cuda)
    wd, bd, gd, bed = w.to(cuda), bias.to(cuda), gamma.to(cuda), beta.to(cuda)
    _l.check(lib.sf_op_conv1d_cl(_l.DTYPES[dtype], x_cl.data_ptr(), wd.data_ptr(), bd.data_ptr(), gd.data_ptr(), bed.data_ptr(), G, 1e-5,
                                 res_cl.data_ptr() if residual else None, B, L, C, N, taps, 1, taps // 2, 1, out.data_ptr(), ws.data_ptr(),
                                 ws.numel(), _l.stream_ptr(cuda)), "sf_op_conv1d_cl")
    torch.cuda.synchronize()
    tol = {"fp32": 2e-5, "bf16": 2e-2, "fp16": 4e-3}[dtype]
    # measured fp32: 1.5e-6 / 1.1e-5 / 6.4e-5 at mean/std 30 / 300 / dead (gates 2e-5 / 1.4e-4 / 4.8e-4); the one-pass statistics
    # measured 2.9e-5 / 2.7e-3 / 8.5e-3
    nx.check_close(out.float().cpu(), ref, _gate(dtype, tol, tol, regime), f"conv1d+GN {dtype} {regime} {shape}", k=_k(dtype))


# ----------------------------------------------------------------------------------------------------------------------------------
# Channel-block chain (conv_cb.hip): offset x loads the first GroupNorm, an offset conv1 bias b1 loads the chunk statistics of h
# that cb_reduce_gn leaves and the second convolution's panel prologue merges
# ----------------------------------------------------------------------------------------------------------------------------------
CB_SHAPES = [
    # B, L, C, channel blocks per workgroup
    (4, 44, 1024, 1),      # depth 7: one group per channel block, 6 chunks of 8 rows
    (4, 176, 512, 1),      # depth 5: two groups per block, 22 chunks
    (4, 352, 256, 1),      # depth 4: four groups per block, 16-row chunks
    (5, 61, 512, 1),       # row tiles that start and end inside clips, ragged last chunk
    (16, 44, 1024, 2),     # two channel blocks per workgroup (16-bit only: the split-operand form takes one)
]


@pytest.mark.parametrize("ratio", [30.0, 300.0])
@pytest.mark.parametrize("which", ["x", "b1"])
@pytest.mark.parametrize("dtype,shape", [(d, s) for d in ("bf16", "fp16", "fp32x") for s in CB_SHAPES if not (d == "fp32x" and s[3] == 2)])
def test_conv_cb_chain_offset(cuda, dtype, ratio, which, shape):
    """which = 'x': the input groups sit at mean/std = ratio (the first GroupNorm; checked through h).  which = 'b1': the input is
    ordinary and conv1's bias puts every group of h at mean/std = ratio (the chunk statistics cb_reduce_gn leaves and the second
    convolution's prologue merges; checked through m, whose residual x then does not drown the second GroupNorm's output)."""
    _l, lib = _lib()
    B, L, C, kb = shape
    G = 8
    td = TD[dtype]
    g = torch.Generator().manual_seed(B * 1000 + L + C + int(ratio))
    if which == "x":
        x = nx.grouped_input(B, L, C, G, f"offset:{ratio:g}", g, td).transpose(1, 2)   # (B, C, L)
    else:
        x = (torch.randn(B, C, L, generator=g) * 1.3 + 0.2).to(td).float()
    w1 = torch.randn(C, C, 3, generator=g) / (3 * C) ** 0.5
    w2 = torch.randn(C, C, 3, generator=g) / (3 * C) ** 0.5
    b2 = torch.randn(C, generator=g) * 0.1
    gam = [1 + 0.2 * torch.randn(C, generator=g) for _ in range(2)]
    bet = [0.1 * torch.randn(C, generator=g) for _ in range(2)]
    ss = torch.randn(B, 2 * C, generator=g) * 0.3
    w1r, w2r = w1.to(td).double(), w2.to(td).double()
    a1 = F.silu(F.group_norm(x.double(), G, gam[0].double(), bet[0].double(), eps=1e-5))
    h0 = F.conv1d(a1, w1r, padding=1)
    if which == "b1":   # per group, `ratio` times the spread of conv1's output, plus a little per-channel variation
        sd = h0.reshape(B, G, -1).std(-1).mean(0)
        sign = torch.where(torch.rand(G, generator=g) < 0.5, -1.0, 1.0)
        b1 = (sign * ratio * sd.float()).repeat_interleave(C // G) + 0.01 * torch.randn(C, generator=g)
    else:
        b1 = torch.randn(C, generator=g) * 0.1
    h_ref = h0 + b1.double()[None, :, None]
    reached = nx.group_ratio((x if which == "x" else h_ref).transpose(1, 2), G)
    assert reached >= 0.7 * ratio, f"regime not reached: max group mean/std {reached:.1f}"
    dev = lambda t: t.contiguous().to(cuda)   # noqa: E731
    x_cl = dev(x.transpose(1, 2).to(td))
    h = nx.nan_like((B, L, C), td, cuda)
    m = nx.nan_like((B, L, C), td, cuda)
    nbytes = lib.sf_op_resnet_mod_cb_workspace_bytes(B, L, C)
    assert nbytes > 0
    ws = nx.poisoned_workspace(nbytes, cuda)
    keep = [dev(t) for t in (w1, b1, w2, b2, gam[0], bet[0], gam[1], bet[1])]
    ssd = dev(ss)
    _l.check(lib.sf_op_resnet_mod_cb(_l.DTYPES[dtype], x_cl.data_ptr(), *[t.data_ptr() for t in keep], G, 1e-5, ssd.data_ptr(), 1e-6,
                                     B, L, C, kb, h.data_ptr(), m.data_ptr(), ws.data_ptr(), ws.numel(), _l.stream_ptr(cuda)),
             "sf_op_resnet_mod_cb")
    torch.cuda.synchronize()
    tol = {"bf16": 2e-2, "fp16": 4e-3, "fp32x": 2e-5}[dtype]
    gate = _gate(dtype, tol, tol, f"offset:{ratio:g}")
    # measured fp32x, b1 at mean/std 300: m 9.1e-6 (gate 1.4e-4; the raw chunk sums measured 2.4e-3); fp16 2.2e-4 (gate 4e-3; raw
    # sums 1.9e-3); x at mean/std 300: h 8.2e-6
    hg = h.float().cpu()
    nx.check_close(hg, h_ref.transpose(1, 2), gate, f"conv_cb h {dtype} {which} ratio {ratio:g} {shape}", k=_k(dtype))
    # the second half from the h the chain STORED (16-bit h is rounded at ~2^-9 of its offset mean: the reference must see the same values)
    hs = hg.double().transpose(1, 2)
    y = x.double() + F.conv1d(F.silu(F.group_norm(hs, G, gam[1].double(), bet[1].double(), eps=1e-5)), w2r, b2.double(), padding=1)
    m_ref = F.layer_norm(y.transpose(1, 2), (C,), eps=1e-6) * (1 + ss.double()[:, None, :C]) + ss.double()[:, None, C:]
    nx.check_close(m.float().cpu(), m_ref, gate, f"conv_cb m {dtype} {which} ratio {ratio:g} {shape}", k=_k(dtype))


# ----------------------------------------------------------------------------------------------------------------------------------
# Row LayerNorms: ln_modulate, and the LayerNorm applied to the projection's accumulator (rstd (acc - mean colsum))
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("C", [64, 1024])
def test_ln_modulate_offset(cuda, dtype, regime, C):
    _l, lib = _lib()
    B, L = 3, 37
    td = TD[dtype]
    g = torch.Generator().manual_seed(C + 5)
    x = nx.row_input(B, L, C, regime, g, td)
    ss = torch.randn(B, 2 * C, generator=g) * 0.3
    ref = F.layer_norm(x.double(), (C,), eps=1e-6) * (1 + ss.double()[:, None, :C]) + ss.double()[:, None, C:]
    xd, sd = x.to(td).to(cuda), ss.to(cuda)
    out = nx.nan_like(xd.shape, td, cuda)
    _l.check(lib.sf_op_ln_modulate(_l.DTYPES[dtype], xd.data_ptr(), sd.data_ptr(), 1e-6, B, L, C, out.data_ptr(), _l.stream_ptr(cuda)),
             "sf_op_ln_modulate")
    torch.cuda.synchronize()
    # measured fp32: 7.8e-7 / 7.9e-6 / 3.2e-5 at mean/std 30 / 300 / dead; constant rows exact (an unshifted mean measured 3.1e-4)
    nx.check_close(out.float().cpu(), ref, _gate(dtype, 8e-3, 1e-5, regime), f"ln_modulate {dtype} {regime} C={C}", k=_k(dtype))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("ratio", [3.0, 30.0])
@pytest.mark.parametrize("shape", [
    # B, L, C, C2, N
    (32, 44, 1024, 256, 1536),    # macro tiles on both GEMMs
    (7, 301, 256, 64, 384),       # ragged rows
    (4, 44, 1024, 256, 1536),     # the 32x32 kernels carry the fusion
])
def test_inject_prenorm_projection_offset(cuda, dtype, ratio, shape):
    """rows of z whose mean is `ratio` times their spread: the LayerNorm on the accumulator subtracts mean * colsum from the raw product"""
    _l, lib = _lib()
    B, L, C, C2, N = shape
    td = TD[dtype]
    g = torch.Generator().manual_seed(B * 1000 + L + C + int(ratio))
    m = nx.row_input(B, L, C, f"offset:{ratio:g}", g, td)
    ctx = torch.randn(B, L, C2, generator=g).to(td).float()
    w_inj = torch.randn(C, C + C2, generator=g) / (C + C2) ** 0.5
    w_inj[:, :C] -= w_inj[:, :C].mean(1, keepdim=True)      # W m adds no multiple of m's row mean: z keeps the offset m carries
    b_inj = torch.randn(C, generator=g) * 0.1
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    w_q = torch.randn(N, C, generator=g) / C ** 0.5
    z_ref = m.double() + F.linear(torch.cat([m, ctx], dim=-1).double(), w_inj.to(td).double(), b_inj.double())
    dev = lambda t: t.contiguous().to(cuda)   # noqa: E731
    md, cd = dev(m.to(td)), dev(ctx.to(td))
    z = nx.nan_like((B, L, C), td, cuda)
    q = nx.nan_like((B, L, N), td, cuda)
    n = lib.sf_op_inject_prenorm_proj_workspace_bytes(B, L, C, C2, N)
    assert n > 0
    ws = nx.poisoned_workspace(n, cuda)
    fused = ctypes.c_int(-1)
    args = [dev(t) for t in (w_inj, b_inj, gamma, beta, w_q)]
    _l.check(lib.sf_op_inject_prenorm_proj(_l.DTYPES[dtype], md.data_ptr(), cd.data_ptr(), args[0].data_ptr(), args[1].data_ptr(),
                                           args[2].data_ptr(), args[3].data_ptr(), 1e-5, args[4].data_ptr(), B, L, C, C2, N, z.data_ptr(),
                                           q.data_ptr(), ctypes.byref(fused), ws.data_ptr(), ws.numel(), _l.stream_ptr(cuda)),
             "sf_op_inject_prenorm_proj")
    torch.cuda.synchronize()
    zg = z.float().cpu()
    assert nx.group_ratio(z_ref.reshape(B * L, 1, C), 1) >= 0.5 * ratio      # the regime was reached (rows of z)
    tol = {"bf16": 2e-2, "fp16": 4e-3}[dtype]
    nx.check_close(zg, z_ref, tol, f"inject z {dtype} ratio {ratio:g} {shape}", k=_k(dtype))
    # q from the z the first GEMM stored (the second GEMM reads those 16-bit values)
    q_ref = F.linear(F.layer_norm(zg.double(), (C,), gamma.double(), beta.double(), eps=1e-5), w_q.to(td).double())
    nx.check_close(q.float().cpu(), q_ref, tol, f"pre-norm projection q {dtype} ratio {ratio:g} {shape} (fused {fused.value})", k=_k(dtype))


# ----------------------------------------------------------------------------------------------------------------------------------
# Attention (sf_op_attention): peaked scores with the dominant key in the first, a middle or the ragged last key block; q = 0
# ----------------------------------------------------------------------------------------------------------------------------------
ATT_SHAPES = [
    # B, H, L           the short-L key-split family, then the long-L 4-wave family (16-bit) / fp32 kernels
    (2, 3, 100),
    (2, 3, 352),
    (9, 8, 1100),
]


def _attention(cuda, dtype, q, kv, B, L, H, D):
    _l, lib = _lib()
    td = TD[dtype]
    qd, kvd = q.to(td).to(cuda), kv.to(td).to(cuda)
    out = nx.nan_like(qd.shape, td, cuda)
    _l.check(lib.sf_op_attention(_l.DTYPES[dtype], qd.data_ptr(), kvd.data_ptr(), B, L, H, D, out.data_ptr(), _l.stream_ptr(cuda)),
             "sf_op_attention")
    torch.cuda.synchronize()
    return out.float().cpu()


@pytest.mark.parametrize("dtype", ["fp32", "fp32x", "bf16", "fp16"])
@pytest.mark.parametrize("peak", nx.PEAK_STDS)
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("B,H,L", ATT_SHAPES)
def test_attention_peaked(cuda, dtype, peak, where, B, H, L):
    D = 64
    td = TD[dtype]
    g = torch.Generator().manual_seed(B * 100 + L + int(peak))
    q, k = nx.peaked_qk(B, L, H, D, peak, where, g)
    v = torch.randn(B, L, H * D, generator=g)
    q, k, v = (t.to(td).float() for t in (q, k, v))
    ref = nx.attention64(q, k, v, H)
    got = _attention(cuda, dtype, q, torch.cat([k, v], dim=-1), B, L, H, D)
    tol = 1e-5 if dtype in ("fp32", "fp32x") else 8e-3
    # measured: fp32 / fp32x <= 3.1e-7; bf16 / fp16 <= 2.9e-4 / 4.3e-5, max/rms <= 9.6e-3.  The 4-wave kernel (L = 1100) with q
    # pre-scaled by log2(e) in 16 bits measured max/rms 0.24 (bf16) / 0.038 (fp16)
    nx.check_close(got, ref, tol, f"attention {dtype} peak {peak:g} at {where} B={B} H={H} L={L}", k=_k(dtype), dims=("clip", "query", "channel"))


@pytest.mark.parametrize("dtype", ["fp32", "fp32x", "bf16", "fp16"])
@pytest.mark.parametrize("B,H,L", ATT_SHAPES)
def test_attention_uniform_weights_average_every_key_once(cuda, dtype, B, H, L):
    """q = 0: every weight is 1 / L and the output is the plain mean of V.  Integer V (0..8) is exact in every type, so a key block
    that is dropped or counted twice moves the output by >= 1 / L of a whole value."""
    D = 64
    g = torch.Generator().manual_seed(L + 1)
    q = torch.zeros(B, L, H * D)
    k = torch.randn(B, L, H * D, generator=g)
    v = torch.randint(0, 9, (B, L, H * D), generator=g).float()
    ref = v.double().mean(1, keepdim=True).expand(B, L, H * D)
    got = _attention(cuda, dtype, q, torch.cat([k.to(TD[dtype]).float(), v], dim=-1), B, L, H, D)
    tol = 1e-6 if dtype in ("fp32", "fp32x") else 4e-3                    # (16-bit: the output's own rounding, 2^-9 of ~4)
    nx.check_close(got, ref, tol, f"attention q=0 {dtype} B={B} H={H} L={L}", k=2.0, dims=("clip", "query", "channel"))


# ----------------------------------------------------------------------------------------------------------------------------------
# One engine-level evaluation with offset activations: the full-size U-Net (configs[1] per branch: batch 8 x 45056 keeps the
# channel-block chain and the GEMM-epilogue GroupNorm tile statistics live) with the biases of the convolutions that feed GroupNorms
# moved by a per-group constant, so that the residual stream carries groups whose mean is large next to their spread
# ----------------------------------------------------------------------------------------------------------------------------------
ENGINE_OFFSET = 8.0       # added per (output) group to the biases below, signs alternating by group
ENGINE_MIN_RATIO = 10.0   # the oracle's block taps must reach this max group mean/std, or the test tests nothing


@pytest.fixture(scope="module")
def offset_full_model(cuda):
    from helpers import reference_model_config
    import syncfusion_amd as sa

    torch.manual_seed(1234)
    model = sa.instantiate(reference_model_config())
    net = model.model.net
    G = net.hparams["resnet_groups"]
    with torch.no_grad():
        for name, p in net.named_parameters():
            # conv1 feeds gn2 (cb_reduce_gn / gn_stats statistics); the down-sampling conv and InjectChannels feed the next item's gn1
            # (the GEMM-epilogue tile statistics at the channel-block levels)
            if name.endswith(("resnet.conv1.bias", ".down.bias", "inject.conv.bias")) and p.numel() % G == 0:
                sign = torch.tensor([1.0 if (i % 2 == 0) else -1.0 for i in range(G)])
                p += (ENGINE_OFFSET * sign).repeat_interleave(p.numel() // G)
    return model.to(cuda)


_ENGINE_REF = {}


@pytest.mark.parametrize("dtype", ["fp32", "fp32x", "bf16", "fp16"])
def test_full_size_engine_offset_activations(cuda, offset_full_model, dtype):
    from helpers import rel_l2, synth_inputs
    from oracle import unet_ref
    from helpers import oracle_params

    net = offset_full_model.model.net
    B, L0 = 8, 45056
    x, sigma, emb, chans = synth_inputs(dict(net.hparams), B, L0, 81)
    if "ref" not in _ENGINE_REF:
        taps_ref = {}
        P, cfg = oracle_params(net, "net."), dict(net.hparams)
        ref = unet_ref.unet_forward(P, cfg, x, sigma, embedding=emb, channels=chans, embedding_scale=1.0, taps=taps_ref)
        _ENGINE_REF.update(ref=ref, taps=taps_ref)
    ref, taps_ref = _ENGINE_REF["ref"], _ENGINE_REF["taps"]
    G = net.hparams["resnet_groups"]
    ratios = {n: nx.group_ratio(t.transpose(1, 2), G) for n, t in taps_ref.items() if t.shape[1] % G == 0}
    assert all(bool(torch.isfinite(t).all()) for t in taps_ref.values()) and bool(torch.isfinite(ref).all())
    assert max(ratios.values()) >= ENGINE_MIN_RATIO, f"regime not reached: max group mean/std {max(ratios.values()):.1f}"
    # measured output rel-L2: fp32 1.4e-7, fp32x 1.1e-7, bf16 8.1e-4, fp16 6.4e-5; worst fp32 tap 4.1e-7 (4.1e-6 with the one-pass
    # statistics); group mean/std reaches 10-15 at depths 4-7 and ~500 at depth 0
    tap_tol = 1e-4 if dtype in ("fp32", "fp32x") else 5e-2                                  # test_gpu_models.py: FP32_TOL, LOWP_TAP_TOL
    out_tol = {"fp32": 1e-4, "fp32x": 1e-4, "bf16": 1e-3, "fp16": 1.5e-4}[dtype]             # FP32_TOL, LOWP_EVAL_TOL
    prev = net.compute_dtype
    net.compute_dtype = dtype
    try:
        gx, gs, ge, gc = x.to(cuda), sigma.to(cuda), emb.to(cuda), [c.to(cuda) for c in chans]
        out_t, taps = net.engine().forward_with_taps(gx, gs, gc, ge, 1.0, cap_floats=1 << 27)
        out = net(gx, gs, embedding=ge, channels=gc)
    finally:
        net.compute_dtype = prev
    worst = ("", 0.0)
    for name, t in taps_ref.items():
        got = taps[name].cpu().reshape(B, -1, t.shape[1]).transpose(1, 2)
        e = rel_l2(got, t)
        worst = max(worst, (name, e), key=lambda p: p[1])
        assert e < tap_tol, f"{dtype} tap {name} (group mean/std up to {ratios.get(name, 0):.1f}): rel-L2 {e:.3e}"
    e_t, e_o = rel_l2(out_t.cpu(), ref), rel_l2(out.cpu(), ref)
    top = max(ratios, key=ratios.get)
    print(f"{dtype} offset full-size B=8 eval: rel-L2 {e_o:.3e} (taps run {e_t:.3e}); worst tap {worst[0]} {worst[1]:.3e}; "
          f"max group mean/std {ratios[top]:.1f} at {top}")
    assert e_t < out_tol and e_o < out_tol


# ----------------------------------------------------------------------------------------------------------------------------------
# Training: GroupNorm+SiLU -> conv forward and every gradient, LayerNorm-modulate gradients, attention forward / backward, in both
# GEMM arithmetics (autograd.GEMM_DTYPE), against fp64 autograd of the same ops.  Gate: test_gpu_train.py's 2e-5, raised to
# 8 * 2^-24 * mean/std past mean/std 30 (numerics.offset_gate)
# ----------------------------------------------------------------------------------------------------------------------------------
TRAIN_TOL = 2e-5


def _train_gate(regime):
    r = _ratio(regime)
    return TRAIN_TOL if r <= 30 else nx.offset_gate(TRAIN_TOL, r)


@pytest.mark.autograd
@pytest.mark.parametrize("mode", ["fp32", "fp32x"])
@pytest.mark.parametrize("regime", ["offset:30", "offset:300", "dead:4"])
@pytest.mark.parametrize("B,L,C,N,taps", [
    (2, 352, 64, 64, 3),        # thin level
    (3, 700, 256, 256, 3),      # ragged length, MFMA paths
    (2, 2816, 8, 8, 3),         # depth 0: one channel per group
    (4, 4096, 128, 128, 3),     # macro-tile dgrad, chunked statistics over long clips
])
def test_train_gn_silu_conv_offset(cuda, monkeypatch, mode, regime, B, L, C, N, taps):
    from syncfusion_amd import autograd as sfa

    monkeypatch.setattr(sfa, "GEMM_DTYPE", mode)
    G = 8
    g = torch.Generator().manual_seed(B * 1000 + L + C)
    x = nx.grouped_input(B, L, C, G, regime, g).transpose(1, 2).contiguous()     # (B, C, L)
    w = torch.randn(N, C, taps, generator=g) / (C * taps) ** 0.5
    b = torch.randn(N, generator=g) * 0.1
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    dy = torch.randn(B, N, L, generator=g)
    ref_leaves = [t.double().requires_grad_() for t in (x, w, b, gamma, beta)]
    xr, wr, br, gr, ber = ref_leaves
    y_ref = F.conv1d(F.silu(F.group_norm(xr, G, gr, ber, eps=1e-5)), wr, br, padding=taps // 2)
    y_ref.backward(dy.double())
    leaves = [t.clone().to(cuda).requires_grad_() for t in (x, w, b, gamma, beta)]
    y = sfa.gn_silu_conv1d(*leaves, G)
    gate = _train_gate(regime)
    # measured (both modes): forward 3.1e-6 / 4.1e-5 / 1.5e-4 at mean/std 30 / 300 / dead (gates 2e-5 / 1.4e-4 / 4.8e-4), gradients
    # <= 5.6e-6 / 4.2e-5 / 1.5e-4; the one-pass statistics measured 2.3e-3 on the forward at mean/std 300
    what = f"{mode} {regime} B={B} L={L} C={C}"
    nx.check_close(y.detach().cpu(), y_ref.detach(), gate, f"train forward {what}", dims=("clip", "channel", "row"))
    y.backward(dy.to(cuda))
    for nm, got, ref in zip(("dx", "dw", "db", "dgamma", "dbeta"), leaves, ref_leaves):
        nx.check_close(got.grad.cpu(), ref.grad, gate, f"{nm} {what}", dims=("clip", "channel", "row") if nm == "dx" else None)


@pytest.mark.autograd
@pytest.mark.parametrize("regime", ["offset:30", "offset:300", "dead:4", "const"])
@pytest.mark.parametrize("B,L,C", [(2, 352, 64), (2, 44, 1024), (2, 5000, 128)])
def test_train_ln_modulate_offset(cuda, regime, B, L, C):
    from syncfusion_amd import autograd as sfa

    g = torch.Generator().manual_seed(L + C)
    x = nx.row_input(B, L, C, regime, g)
    ss = 0.3 * torch.randn(B, 2 * C, generator=g)
    dy = torch.randn(B, L, C, generator=g)
    xr, ssr = x.double().requires_grad_(), ss.double().requires_grad_()
    y_ref = F.layer_norm(xr, (C,), eps=1e-5) * (1 + ssr[:, None, :C]) + ssr[:, None, C:]
    y_ref.backward(dy.double())
    xs, sss = x.clone().to(cuda).requires_grad_(), ss.clone().to(cuda).requires_grad_()
    y = sfa.ln_modulate(xs, sss, 1e-5)
    gate = _train_gate(regime)
    nx.check_close(y.detach().cpu(), y_ref.detach(), gate, f"train ln_modulate {regime} B={B} L={L} C={C}")
    y.backward(dy.to(cuda))
    if regime != "const":   # a constant row has dx = 0 up to rounding on both sides: no relative gate means anything there
        nx.check_close(xs.grad.cpu(), xr.grad, gate, f"ln_modulate dx {regime} B={B} L={L} C={C}")
    nx.check_close(sss.grad.cpu(), ssr.grad, gate, f"ln_modulate dss {regime} B={B} L={L} C={C}", dims=("clip", "channel"))


@pytest.mark.autograd
@pytest.mark.parametrize("mode", ["fp32", "fp32x"])
@pytest.mark.parametrize("peak", nx.PEAK_STDS)
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("B,L,H", [(2, 100, 2), (1, 352, 8), (1, 2500, 1)])
def test_train_attention_peaked(cuda, monkeypatch, mode, peak, where, B, L, H):
    from syncfusion_amd import autograd as sfa

    monkeypatch.setattr(sfa, "GEMM_DTYPE", mode)
    D = 64
    g = torch.Generator().manual_seed(L * 10 + H + int(peak))
    q, k = nx.peaked_qk(B, L, H, D, peak, where, g)
    v = torch.randn(B, L, H * D, generator=g)
    kv = torch.cat([k, v], dim=-1)
    do = torch.randn(B, L, H * D, generator=g)
    qr, kvr = q.double().requires_grad_(), kv.double().requires_grad_()
    o_ref = nx.attention64(qr, kvr[..., : H * D], kvr[..., H * D:], H)
    o_ref.backward(do.double())
    qs, kvs = q.clone().to(cuda).requires_grad_(), kv.clone().to(cuda).requires_grad_()
    o = sfa.attention(qs, kvs, H)
    what = f"{mode} peak {peak:g} at {where} B={B} L={L} H={H}"
    dims = ("clip", "query", "channel")
    nx.check_close(o.detach().cpu(), o_ref.detach(), TRAIN_TOL, f"train attention {what}", dims=dims)
    o.backward(do.to(cuda))
    # The backward recomputes P = exp(s - lse) from fp32 scores s of size up to ~8 peak: an exact-but-fp32 score is off by 2^-24 |s|,
    # and unlike the forward (o = sum P v / sum P) nothing divides that error out again -> max(2e-5, 8 * 2^-24 * max|s|).  The
    # max-error factor grows by sqrt(L): rms(dv) is one dominant key row per (clip, head) spread over L rows.  (measured rel-L2
    # 6e-6 ... 4e-5, max/rms <= 2.5e-3 at peak 30)
    s_max = float((q.double().reshape(B, L, H, D).transpose(1, 2) @ k.double().reshape(B, L, H, D).transpose(1, 2).transpose(-1, -2)).abs().max()) * D ** -0.5
    gate = max(TRAIN_TOL, 8.0 * nx.U24 * s_max)
    nx.check_close(kvs.grad[..., H * D:].cpu(), kvr.grad[..., H * D:], gate, f"attention dv {what}", k=nx.MAX_K * L ** 0.5,
                   dims=("clip", "key", "channel"))
    # dq, dk are not gated here: they pass through dS = P (dP - rowsum(dO o)), and with one key holding all but e^-30 of a query's
    # weight the exact dS is ~0 while both fp32 terms are ~dP of that key -- the device result is their rounding, relative to
    # nothing.  test_gpu_train.py::test_attention_gradients gates dq / dk at ordinary scores
