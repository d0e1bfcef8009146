"""The 128-channel item head on conv_cb's direct epilogues (MI355X): sf_op_resnet_mod_cbd and the engine level that runs it.

At C = 128 one channel block is the whole reduction and the whole row, so the two convolutions finish their own results: the first
stores h = acc + b1 and the GroupNorm chunk statistics of the stored h (direct_gn, chunked and summed as the chain's reducer does), the second applies GroupNorm+SiLU from them while
staging its panel and finishes + b2 + x, LayerNorm over the row and Modulation in its epilogue (direct_ln).  The plain InjectChannels
GEMM follows (w_inj set).  Checked here:
  1. h, m and z against the fp32 composition on the CPU from the same 16-bit-rounded inputs, at test_gpu_ops.TOL;
  2. against the existing chain sf_op_resnet_mod_cb(kb = 1): h bit for bit, m within one 16-bit ulp, the emitted statistics against an
     fp64 recomputation from the device's own h;
  3. refusals: a non-zero code and no byte written;
  4. guard bands around every buffer;
  5. the full-size 16-bit engine: depth-3 taps against the fp32 engine's, and the launch count of one evaluation.
"""
import pytest
import torch
import torch.nn.functional as F

from helpers import rel_l2
from numerics import U24
from test_gpu_ops import TD, TOL   # the op-level gates of the channel-block chain (test_conv_cb_chain)

pytestmark = pytest.mark.gpu

C = 128
C2 = 32        # context channels of the InjectChannels GEMM
CTX_LD = 40    # its row pitch: wider than C2, as the engine's padded context buffer
SHAPES = [
    # B, L, G, modulated
    (1, 64, 8, True),       # two chunks
    (3, 96, 8, True),       # clips of three tiles, nine row tiles
    (2, 1024, 8, True),     # nch = 32, the limit
    (4, 704, 8, True),      # the workload's own per-branch level: 2816 rows
    (3, 96, 2, False),      # 64 channels per group (a group spans two waves), plain LayerNorm
    (10, 1024, 8, True),    # 10240 rows: the launcher takes two row tiles per workgroup from 10177 rows on
]
_CASES = {}


def _chunk_rows(L):
    """rows per statistics chunk: cb_gn_plan of conv_cb.hip (8 P with the fewest passes that keep the chunk count within 32)"""
    P = 1
    while P < 4 and (L + 8 * P - 1) // (8 * P) > 32:
        P *= 2
    return 8 * P


def _lib():
    from syncfusion_amd import _lib

    return _lib, _lib.load()


def _case(dtype, shape):
    """Inputs and CPU references of one (dtype, shape), built once and shared: h_ref / m_ref exactly as test_conv_cb_chain builds them,
    z_ref = m16 + conv1x1(cat[m16, ctx]) + b + badd with m16 the rounded m."""
    key = (dtype, shape)
    if key in _CASES:
        return _CASES[key]
    B, L, G, mod = shape
    td = TD[dtype]
    g = torch.Generator().manual_seed(B * 1000 + L + C)
    x = torch.randn(B, C, L, generator=g) * 1.3 + 0.2
    w1 = torch.randn(C, C, 3, generator=g) / (3 * C) ** 0.5
    w2 = torch.randn(C, C, 3, generator=g) / (3 * C) ** 0.5
    b1, b2 = torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    gam = [1 + 0.2 * torch.randn(C, generator=g) for _ in range(2)]
    bet = [0.1 * torch.randn(C, generator=g) for _ in range(2)]
    ss = torch.randn(B, 2 * C, generator=g) * 0.3 if mod else None
    wi = torch.randn(C, C + C2, generator=g) / (C + C2) ** 0.5
    bi = torch.randn(C, generator=g) * 0.1
    ctx = torch.randn(B, L, CTX_LD, generator=g)
    badd = torch.randn(B, C, generator=g) * 0.2
    xr = x.to(td).float()
    w1r, w2r = w1.to(td).float(), w2.to(td).float()
    h_ref = F.conv1d(F.silu(F.group_norm(xr, G, gam[0], bet[0], eps=1e-5)), w1r, b1, padding=1)
    y = xr + F.conv1d(F.silu(F.group_norm(h_ref, G, gam[1], bet[1], eps=1e-5)), w2r, b2, padding=1)
    m_ref = F.layer_norm(y.transpose(1, 2), (C,), eps=1e-6)
    if mod:
        m_ref = m_ref * (1 + ss[:, None, :C]) + ss[:, None, C:]
    m16 = m_ref.to(td).float()
    cat = torch.cat([m16, ctx[..., :C2].to(td).float()], dim=-1)
    z_ref = m16 + cat @ wi.to(td).float().t() + bi + badd[:, None, :]
    c = dict(x=x.transpose(1, 2).contiguous().to(td), params=(w1, b1, w2, b2, gam[0], bet[0], gam[1], bet[1]), ss=ss, wi=wi, bi=bi,
             ctx=ctx.to(td), badd=badd, h_ref=h_ref.transpose(1, 2), m_ref=m_ref, z_ref=z_ref)
    _CASES[key] = c
    return c


def _run_direct(cuda, dtype, shape, inject):
    """-> (h, m, z or None, stats) of sf_op_resnet_mod_cbd on the device"""
    _l, lib = _lib()
    B, L, G, mod = shape
    td = TD[dtype]
    c = _case(dtype, shape)
    dev = lambda t: t.to(cuda)   # noqa: E731
    x = dev(c["x"])
    keep = [dev(t) for t in c["params"]]
    ssd = dev(c["ss"]) if mod else None
    h = torch.full((B, L, C), float("nan"), dtype=td, device=cuda)
    m, z = torch.full_like(h, float("nan")), torch.full_like(h, float("nan"))
    stats = torch.full((B, L // _chunk_rows(L), G, 2), float("nan"), device=cuda)
    nbytes = lib.sf_op_resnet_mod_cbd_workspace_bytes(B, L, C, C2 if inject else 0)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    inj = [dev(c["wi"]), dev(c["bi"]), dev(c["ctx"]), dev(c["badd"])] if inject else None
    rc = lib.sf_op_resnet_mod_cbd(_l.DTYPES[dtype], x.data_ptr(), *[t.data_ptr() for t in keep], G, 1e-5, ssd.data_ptr() if mod else None, 1e-6,
                                  B, L, C, inj[0].data_ptr() if inject else None, inj[1].data_ptr() if inject else None,
                                  inj[2].data_ptr() if inject else None, CTX_LD, C2 if inject else 0, inj[3].data_ptr() if inject else None,
                                  h.data_ptr(), m.data_ptr(), z.data_ptr() if inject else None, stats.data_ptr(), ws.data_ptr(), ws.numel(),
                                  _l.stream_ptr(cuda))
    _l.check(rc, "sf_op_resnet_mod_cbd")
    torch.cuda.synchronize()
    return h, m, (z if inject else None), stats


@pytest.mark.parametrize("inject", [False, True], ids=["two_launches", "with_inject"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_cb_direct_against_cpu(cuda, dtype, shape, inject):
    """h, m (and z) against the fp32 torch composition on the CPU from the same 16-bit-rounded inputs, at the chain's own gate."""
    c = _case(dtype, shape)
    h, m, z, _ = _run_direct(cuda, dtype, shape, inject)
    e_h, e_m = rel_l2(h.float().cpu(), c["h_ref"]), rel_l2(m.float().cpu(), c["m_ref"])
    e_z = rel_l2(z.float().cpu(), c["z_ref"]) if inject else 0.0
    print(f"cb direct {dtype} {shape} inject={inject}: h {e_h:.3e}  m {e_m:.3e}  z {e_z:.3e}")
    assert e_h < TOL[dtype] and e_m < TOL[dtype] and e_z < TOL[dtype]


def _ulp_steps(a, b):
    """distance of two 16-bit tensors in representable values (sign-magnitude bit patterns mapped to a monotone integer line)"""
    def line(t):
        i = t.view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (line(a) - line(b)).abs()


_CHAIN = {}


def _both(cuda, dtype, shape):
    """(h, m, stats) of the direct form and (h, m) of sf_op_resnet_mod_cb(kb = 1) on the same inputs, run once per (dtype, shape)"""
    key = (dtype, shape)
    if key in _CHAIN:
        return _CHAIN[key]
    _l, lib = _lib()
    B, L, G, mod = shape
    c = _case(dtype, shape)
    h, m, _, stats = _run_direct(cuda, dtype, shape, False)
    dev = lambda t: t.to(cuda)   # noqa: E731
    x = dev(c["x"])
    keep = [dev(t) for t in c["params"]]
    ssd = dev(c["ss"]) if mod else None
    h0, m0 = torch.empty_like(h), torch.empty_like(m)
    nbytes = lib.sf_op_resnet_mod_cb_workspace_bytes(B, L, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    rc = lib.sf_op_resnet_mod_cb(_l.DTYPES[dtype], x.data_ptr(), *[t.data_ptr() for t in keep], G, 1e-5, ssd.data_ptr() if mod else None, 1e-6,
                                 B, L, C, 1, h0.data_ptr(), m0.data_ptr(), ws.data_ptr(), ws.numel(), _l.stream_ptr(cuda))
    _l.check(rc, "sf_op_resnet_mod_cb")
    torch.cuda.synchronize()
    _CHAIN[key] = tuple(t.cpu() for t in (h, m, stats, h0, m0))
    return _CHAIN[key]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_cb_direct_h_equals_chain(cuda, dtype, shape):
    """Same inputs through sf_op_resnet_mod_cb(kb = 1): h bit for bit (same accumulation order, acc + bias, one rounding)."""
    h, _, _, h0, _ = _both(cuda, dtype, shape)
    assert torch.equal(h.view(torch.int16), h0.view(torch.int16)), "h differs from the chain's h"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_cb_direct_m_within_one_ulp_of_chain(cuda, dtype, shape):
    """m of the direct form against m of the chain: at most one 16-bit ulp per element.  direct_gn chunks and sums the statistics of h as
    cb_reduce_gn does and direct_ln adds the row sums in cb_reduce_ln's order, so the second convolution sees the same (mean, rstd), forms
    the same accumulators and m is expected equal bit for bit: the count of differing elements is printed."""
    _, m, _, _, m0 = _both(cuda, dtype, shape)
    steps = _ulp_steps(m, m0)
    ndiff, worst = int((steps != 0).sum()), int(steps.max())
    dmax = float((m.float() - m0.float()).abs().max())
    print(f"cb direct vs chain {dtype} {shape}: m differs in {ndiff} of {m.numel()} elements, at most {worst} ulp, max |diff| {dmax:.3e}")
    assert worst <= 1


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_cb_direct_statistics(cuda, dtype, shape):
    """The emitted (mean, M2) per chunk (8, 16 or 32 rows: _chunk_rows) and group against fp64 from the device's own stored h.

    Bound (u = numerics.U24, n = rows * C / G values per chunk and group, any summation order, Higham's gamma_n = n u / (1 - n u)):
      mean:  |mean_dev - mean_64| <= gamma_n * mean|x|                       (a sum of n fp32 terms and one multiply by 1 / n)
      M2:    sum (x - mean_dev)^2 = M2 + n (mean_dev - mean)^2 exactly, and its fp32 evaluation (one subtraction, one fma per term, a
             sum of n terms) is within gamma_(n+3) of that:  |M2_dev - M2_64| <= gamma_(n+3) * M2_64 + (1 + gamma_(n+3)) * n * (gamma_n * mean|x|)^2
    """
    B, L, G, _ = shape
    h, _, stats, _, _ = _both(cuda, dtype, shape)
    R = _chunk_rows(L)
    n = R * (C // G)
    hd = h.double().reshape(B, L // R, R, G, C // G)
    mean64 = hd.mean(dim=(2, 4))
    m2_64 = (hd - mean64[:, :, None, :, None]).pow(2).sum(dim=(2, 4))
    mabs = hd.abs().mean(dim=(2, 4))
    gam_n, gam_n3 = n * U24 / (1 - n * U24), (n + 3) * U24 / (1 - (n + 3) * U24)
    st = stats.double()
    assert bool(torch.isfinite(st).all())
    d_mean, d_m2 = (st[..., 0] - mean64).abs(), (st[..., 1] - m2_64).abs()
    b_mean = gam_n * mabs
    b_m2 = gam_n3 * m2_64 + (1 + gam_n3) * n * b_mean.pow(2)
    print(f"cb direct statistics {dtype} {shape}: mean err / bound {float((d_mean / b_mean).max()):.3f}, M2 err / bound {float((d_m2 / b_m2).max()):.3f}")
    assert bool((d_mean <= b_mean).all()) and bool((d_m2 <= b_m2).all())


@pytest.mark.parametrize("dtype,B,L,Cx,inject", [
    ("bf16", 2, 80, 128, False),     # L is not a multiple of 32: a tile would straddle two clips
    ("bf16", 2, 1056, 128, False),   # 33 chunks per clip
    ("bf16", 2, 64, 256, True),      # two channel slices: the accumulators are partial sums (w_inj requested)
    ("fp16", 2, 64, 256, False),     # ... (m_out requested)
    ("fp32", 2, 64, 128, False),     # 16-bit engines only
])
def test_cb_direct_refusals(cuda, dtype, B, L, Cx, inject):
    """Shapes outside the direct epilogues' coverage: a non-zero code, and no output or workspace byte written."""
    _l, lib = _lib()
    td = TD[dtype]
    t = torch.zeros(B, L, Cx, dtype=td, device=cuda)
    f = torch.zeros(3 * Cx * Cx + 2 * B * Cx, device=cuda)
    outs = [torch.full((B, L, Cx), 7.0, dtype=td, device=cuda) for _ in range(3)]
    stats = torch.full((B * 64 * 8 * 2,), 7.0, device=cuda)
    ws = torch.full((max(int(lib.sf_op_resnet_mod_cbd_workspace_bytes(B, L, Cx, C2)), 1 << 20),), 7, dtype=torch.uint8, device=cuda)
    rc = lib.sf_op_resnet_mod_cbd(_l.DTYPES[dtype], t.data_ptr(), *[f.data_ptr()] * 8, 8, 1e-5, None, 1e-6, B, L, Cx,
                                  f.data_ptr() if inject else None, f.data_ptr() if inject else None, t.data_ptr() if inject else None, Cx,
                                  C2 if inject else 0, None, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr() if inject else None,
                                  stats.data_ptr(), ws.data_ptr(), ws.numel(), _l.stream_ptr(cuda))
    torch.cuda.synchronize()
    assert rc != 0
    for o in outs:
        assert bool((o == 7.0).all())
    assert bool((stats == 7.0).all()) and bool((ws == 7).all())


@pytest.mark.parametrize("inject", [False, True], ids=["two_launches", "with_inject"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_cb_direct_guards(cuda, dtype, inject):
    """Every pointer of the op inside guard bands (tests/guards.py), the workspace exactly as long as the query says: nothing outside
    h, m, z, stats or the workspace changes, no input is written, and the results equal the unguarded run bit for bit."""
    from test_gpu_guards import _run_case

    _l, lib = _lib()
    B, L, G = 3, 96, 8
    td = TD[dtype]
    c = _case(dtype, (B, L, G, True))
    names = ("w1", "b1", "w2", "b2", "gn1_g", "gn1_b", "gn2_g", "gn2_b")
    nws = int(lib.sf_op_resnet_mod_cbd_workspace_bytes(B, L, C, C2 if inject else 0))
    assert nws > 0

    def run(a):
        xs = a.inp(c["x"], "x")
        keep = [a.inp(t, n) for t, n in zip(c["params"], names)]
        sd = a.inp(c["ss"], "scale_shift")
        inj = [a.inp(c["wi"], "w_inj"), a.inp(c["bi"], "b_inj"), a.inp(c["ctx"], "ctx"), a.inp(c["badd"], "badd")] if inject else None
        h, m = a.out((B, L, C), td, "h_out"), a.out((B, L, C), td, "m_out")
        z = a.out((B, L, C), td, "z_out") if inject else None
        st = a.out((B, L // _chunk_rows(L), G, 2), torch.float32, "stats_out")
        wk = a.ws(nws, "ws")
        rc = lib.sf_op_resnet_mod_cbd(_l.DTYPES[dtype], xs.ptr, *[t.ptr for t in keep], G, 1e-5, sd.ptr, 1e-6, B, L, C,
                                      inj[0].ptr if inject else None, inj[1].ptr if inject else None, inj[2].ptr if inject else None, CTX_LD,
                                      C2 if inject else 0, inj[3].ptr if inject else None, h.ptr, m.ptr, z.ptr if inject else None, st.ptr,
                                      wk.ptr, nws, _l.stream_ptr(cuda))
        return rc, [h, m, st] + ([z] if inject else [])

    _run_case(cuda, "sf_op_resnet_mod_cbd", run)


# ----------------------------------------------------------------------------------------------------------
# engine level: the full-size 16-bit net, depth 3 (C = 128, L = 704 at L0 = 45056)
# ----------------------------------------------------------------------------------------------------------
# Launches of ONE evaluation of the full-size 16-bit engine at L0 = 45056 ("direct chain at the 128-channel level").  The
# switch that turns the direct chain off exists only in the tuning build, so the count without it is the recorded one: every depth-3 item
# takes one launch less (four items per branch).
LAUNCHES_WITHOUT_DIRECT = {2: 223, 8: 449}
ITEMS_D3 = 4


@pytest.fixture(scope="module")
def full_model(cuda):
    from helpers import reference_model_config
    import syncfusion_amd as sa

    torch.manual_seed(1234)
    return sa.instantiate(reference_model_config()).to(cuda)


@pytest.fixture(scope="module")
def fp32_taps(cuda, full_model):
    """depth-3 taps and the output of the fp32 engine, per batch size (computed once, shared by the dtypes)"""
    memo = {}

    def get(B, L0):
        if B not in memo:
            from test_gpu_models import _compute_dtype, _full_inputs

            x, sigma, emb, chans = _full_inputs(full_model, B, L0, 81)
            gx, gs, ge, gc = x.to(cuda), sigma.to(cuda), emb.to(cuda), [t.to(cuda) for t in chans]
            with _compute_dtype(full_model, "fp32") as net:
                out, taps = net.engine().forward_with_taps(gx, gs, gc, ge, 1.0, cap_floats=1 << 27)
            memo[B] = ((gx, gs, ge, gc), out.cpu(), {k: v.cpu() for k, v in taps.items() if k.startswith("d3.")})
        return memo[B]

    return get


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B", [2, 4])
def test_engine_depth3_taps(cuda, full_model, fp32_taps, dtype, B):
    """Depth-3 block activations of the 16-bit engine on the direct chain against the fp32 engine's, at the tolerance
    test_full_size_lowp_eval_parity_with_taps applies to them.  A run with taps is one branch, so 2 and 4 clips (1408 and 2816 rows, the
    cap of the dispatch rule) are the batch sizes at which it takes the direct chain; 8 clips in two branches are test_engine_launch_count's."""
    from test_gpu_models import LOWP_TAP_TOL, _compute_dtype

    (gx, gs, ge, gc), _, ref = fp32_taps(B, 45056)
    with _compute_dtype(full_model, dtype) as net:
        _, taps = net.engine().forward_with_taps(gx, gs, gc, ge, 1.0, cap_floats=1 << 27)
    names = [k for k in ref if k.startswith("d3.items_") or k == "d3.out"]
    assert len(names) == ITEMS_D3 + 1
    worst = ("", 0.0)
    for k in names:
        e = rel_l2(taps[k].cpu(), ref[k])
        worst = max(worst, (k, e), key=lambda p: p[1])
        assert e < LOWP_TAP_TOL, f"{dtype} B={B} tap {k}: rel-L2 {e:.3e}"
    print(f"{dtype} B={B} depth-3 taps vs the fp32 engine: worst {worst[0]} {worst[1]:.3e}")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B", [2, 8])
def test_engine_launch_count(cuda, full_model, fp32_taps, dtype, B):
    """The production dispatch (one branch at 2 clips, two at 8) took the direct chain: one conv_cb_gn and one conv_cb_ln launch per depth-3
    item and branch, the evaluation one launch per such item shorter than recorded without it, and the output still the fp32 engine's."""
    from test_gpu_models import LOWP_EVAL_TOL, _compute_dtype

    (gx, gs, ge, gc), out32, _ = fp32_taps(B, 45056)
    nbr = 2 if B >= 4 else 1
    with _compute_dtype(full_model, dtype) as net:
        recs = net.engine().profile_forward(gx, gs, gc, ge, 1.0)
        out = net(gx, gs, embedding=ge, channels=gc)
        count = net.engine().launch_count()
    labels = [r[0] for r in recs]
    assert labels.count("conv_cb_gn") == ITEMS_D3 * nbr and labels.count("conv_cb_ln") == ITEMS_D3 * nbr
    assert count == LAUNCHES_WITHOUT_DIRECT[B] - ITEMS_D3 * nbr, count
    e = rel_l2(out.cpu(), out32)
    print(f"{dtype} B={B}: {count} launches per evaluation; output vs the fp32 engine rel-L2 {e:.3e}")
    assert e < LOWP_EVAL_TOL[dtype]
