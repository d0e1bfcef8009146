"""The item tail of the thin levels at op level (MI355X): sf_op_thin_tail = thin_tail_kernel of conv_thin.hip, the launch that computes
y = x + conv3(silu(groupnorm(h))), LayerNorm + Modulation and InjectChannels on the 32- and 64-channel levels.

The 16-bit workgroups of up to 4 tiles at 64 channels and 6 at 32 issue every global read -- rows, statistics partials, modulation
operands, weights -- before their first wait; addresses of lanes beyond a buffer's end are clamped or the lane is predicated off.
Larger workgroups stage weights and statistics with loops.  Checked here, at the smallest shapes that take each path (one tile and the
4-wave staging floor, two partials per lane, the fold loop beyond the up-front partials, a partial tile behind a short last chunk, 6
waves, and 8 waves on the loop form; the second rw of a shape usually lands on the other form):
  1. z against the fp32 composition on the CPU from the same 16-bit-rounded inputs, at test_gpu_ops.TOL (the statistics of h are
     computed in fp64 on the CPU and handed in);
  2. z bit for bit the same for two different rw (rows do not depend on the chunking);
  3. the emitted (mean, M2) per workgroup and group against fp64 from the device's own z, with test_cb_direct_statistics' bound;
  4. guard bands around every buffer, the workspace exactly as long as the query says;
  5. refusals: a non-zero code and no byte written.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from helpers import rel_l2
from numerics import U24
from test_gpu_ops import TD, TOL

pytestmark = pytest.mark.gpu

G = 8
CTX_PAD = 8    # the context rows are wider than C2, as the engine's padded buffer
SHAPES = [
    # B, L, C, C2, rw, rw of the second run
    (1, 64, 64, 32, 32, 64),        # one tile per workgroup: the waves beyond it only stage weights
    (2, 2816, 64, 32, 64, 352),     # the workload's geometry: nch_in = 44, two partials per lane
    (3, 200, 64, 64, 64, 32),       # last chunk of 8 rows: a partial tile and a short last statistics chunk
    (1, 11264, 32, 32, 64, 512),    # nch_in = 176: the fold loop beyond the up-front partials
    (2, 704, 32, 32, 192, 64),      # 6 waves; nch_in <= 32
    (2, 4096, 64, 32, 352, 96),     # 8 waves, the product maximum
]
IDS = [f"B{s[0]}_L{s[1]}_C{s[2]}_{s[3]}_rw{s[4]}" for s in SHAPES]
_CASES, _RUNS = {}, {}


def _lib():
    from syncfusion_amd import _lib

    return _lib, _lib.load()


def _chunk_stats(t, rows):
    """(mean, M2) in fp64 per chunk of `rows` positions (the last one short) and group of t:(B, L, C) -> (B, nch, G, 2) fp32"""
    B, L, C = t.shape
    out = []
    for r0 in range(0, L, rows):
        v = t[:, r0:r0 + rows].double().reshape(B, -1, G, C // G)
        mean = v.mean(dim=(1, 3))
        out.append(torch.stack([mean, (v - mean[:, None, :, None]).pow(2).sum(dim=(1, 3))], dim=-1))
    return torch.stack(out, dim=1)


def _case(dtype, shape):
    """Inputs and the CPU reference of one (dtype, shape), built once and shared: z_ref = m16 + conv1x1(cat[m16, ctx]) + b + badd with m16
    the rounded m, as test_gpu_cb_direct._case builds it; the statistics of h per chunk of rw rows in fp64."""
    key = (dtype, shape)
    if key in _CASES:
        return _CASES[key]
    B, L, C, C2, rw, _ = shape
    td = TD[dtype]
    g = torch.Generator().manual_seed(B * 1000 + L + C + C2)
    h = (torch.randn(B, L, C, generator=g) * 1.1 + 0.15).to(td)
    x = (torch.randn(B, L, C, generator=g) * 1.3 + 0.2).to(td)
    ctx = torch.randn(B, L, C2 + CTX_PAD, generator=g).to(td)
    w2 = torch.randn(C, C, 3, generator=g) / (3 * C) ** 0.5
    b2 = torch.randn(C, generator=g) * 0.1
    gam, bet = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ss = torch.randn(B, 2 * C, generator=g) * 0.3
    wi = torch.randn(C, C + C2, generator=g) / (C + C2) ** 0.5
    bi = torch.randn(C, generator=g) * 0.1
    badd = torch.randn(B, C, generator=g) * 0.2
    hr, xr = h.float().transpose(1, 2), x.float().transpose(1, 2)
    y = xr + F.conv1d(F.silu(F.group_norm(hr, G, gam, bet, eps=1e-5)), w2.to(td).float(), b2, padding=1)
    m = F.layer_norm(y.transpose(1, 2), (C,), eps=1e-6) * (1 + ss[:, None, :C]) + ss[:, None, C:]
    m16 = m.to(td).float()
    cat = torch.cat([m16, ctx[..., :C2].float()], dim=-1)
    z_ref = m16 + cat @ wi.to(td).float().t() + bi + badd[:, None, :]
    c = dict(h=h, x=x, ctx=ctx, stats=_chunk_stats(h, rw).float(), w2=w2, b2=b2, gam=gam, bet=bet, ss=ss, wi=wi, bi=bi, badd=badd, z_ref=z_ref)
    _CASES[key] = c
    return c


NAMES = ("h", "x", "ctx", "stats", "w2", "b2", "gam", "bet", "ss", "wi", "bi", "badd")


def _call(lib, _l, cuda, dtype, shape, rw, ptr, z, st, ws, nws):
    """one sf_op_thin_tail call; ptr: name -> device address of the case's inputs"""
    B, L, C, C2, rw_in, _ = shape
    return lib.sf_op_thin_tail(_l.DTYPES[dtype], ptr["h"], ptr["x"], ptr["ctx"], C2 + CTX_PAD, C2, C2, ptr["stats"], (L + rw_in - 1) // rw_in, rw_in,
                               ptr["w2"], ptr["b2"], ptr["gam"], ptr["bet"], G, 1e-5, ptr["ss"], 1e-6, ptr["wi"], ptr["bi"], ptr["badd"], B, L, C,
                               rw, z, st, None, ws, nws, _l.stream_ptr(cuda))


def _run(cuda, dtype, shape, rw):
    """-> (z, stats_out) of the op on the device, as CPU tensors; run once per (dtype, shape, rw)"""
    key = (dtype, shape, rw)
    if key in _RUNS:
        return _RUNS[key]
    _l, lib = _lib()
    B, L, C, C2 = shape[:4]
    c = _case(dtype, shape)
    dev = {n: c[n].to(cuda).contiguous() for n in NAMES}
    z = torch.full((B, L, C), float("nan"), dtype=TD[dtype], device=cuda)
    st = torch.full((B, (L + rw - 1) // rw, G, 2), float("nan"), device=cuda)
    nws = int(lib.sf_op_thin_tail_workspace_bytes(_l.DTYPES[dtype], C, C2))
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device=cuda)
    rc = _call(lib, _l, cuda, dtype, shape, rw, {n: t.data_ptr() for n, t in dev.items()}, z.data_ptr(), st.data_ptr(), ws.data_ptr(), nws)
    _l.check(rc, "sf_op_thin_tail")
    torch.cuda.synchronize()
    _RUNS[key] = (z.cpu(), st.cpu())
    return _RUNS[key]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_thin_tail_against_cpu(cuda, dtype, shape):
    """z against the fp32 torch composition on the CPU from the same 16-bit-rounded inputs, at the op-level gate."""
    z, _ = _run(cuda, dtype, shape, shape[4])
    assert bool(torch.isfinite(z.float()).all())
    e = rel_l2(z.float(), _case(dtype, shape)["z_ref"])
    print(f"thin tail {dtype} {shape}: z {e:.3e}")
    assert e < TOL[dtype]


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=[IDS[0], IDS[2]])
def test_thin_tail_fp32(cuda, shape):
    """The op's fp32 coverage (those instantiations keep their staging loops): the same comparison at the fp32 gate."""
    z, _ = _run(cuda, "fp32", shape, shape[4])
    e = rel_l2(z, _case("fp32", shape)["z_ref"])
    print(f"thin tail fp32 {shape}: z {e:.3e}")
    assert e < TOL["fp32"]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_thin_tail_rw_independent(cuda, dtype, shape):
    """The same inputs (and the same input statistics) with another rw: other workgroup sizes, wave counts and staging rounds, the same
    rows -- z is the same bits."""
    z0, _ = _run(cuda, dtype, shape, shape[4])
    z1, _ = _run(cuda, dtype, shape, shape[5])
    ndiff = int((z0.view(torch.int16) != z1.view(torch.int16)).sum())
    assert ndiff == 0, f"z differs between rw = {shape[4]} and rw = {shape[5]} in {ndiff} of {z0.numel()} elements"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_thin_tail_statistics(cuda, dtype, shape):
    """The emitted (mean, M2) per workgroup (rw rows, the last one short) and group against fp64 from the device's own stored z, with the
    bound of test_gpu_cb_direct.test_cb_direct_statistics (u = numerics.U24, n values per chunk and group, gamma_n = n u / (1 - n u)):
      mean: |mean_dev - mean_64| <= gamma_n * mean|z|;   M2: |M2_dev - M2_64| <= gamma_(n+3) * M2_64 + (1 + gamma_(n+3)) * n * (gamma_n * mean|z|)^2
    """
    B, L, C, _, rw, _ = shape
    z, stats = _run(cuda, dtype, shape, rw)
    st = stats.double()
    assert bool(torch.isfinite(st).all())
    worst_mean = worst_m2 = 0.0
    for i, r0 in enumerate(range(0, L, rw)):
        v = z[:, r0:r0 + rw].double().reshape(B, -1, G, C // G)
        n = v.shape[1] * (C // G)
        mean64 = v.mean(dim=(1, 3))
        m2_64 = (v - mean64[:, None, :, None]).pow(2).sum(dim=(1, 3))
        mabs = v.abs().mean(dim=(1, 3))
        gam_n, gam_n3 = n * U24 / (1 - n * U24), (n + 3) * U24 / (1 - (n + 3) * U24)
        b_mean = gam_n * mabs
        b_m2 = gam_n3 * m2_64 + (1 + gam_n3) * n * b_mean.pow(2)
        d_mean, d_m2 = (st[:, i, :, 0] - mean64).abs(), (st[:, i, :, 1] - m2_64).abs()
        worst_mean, worst_m2 = max(worst_mean, float((d_mean / b_mean).max())), max(worst_m2, float((d_m2 / b_m2).max()))
        assert bool((d_mean <= b_mean).all()) and bool((d_m2 <= b_m2).all()), f"chunk {i}: mean err / bound {float((d_mean / b_mean).max()):.3f}, M2 err / bound {float((d_m2 / b_m2).max()):.3f}"
    print(f"thin tail statistics {dtype} {shape}: mean err / bound {worst_mean:.3f}, M2 err / bound {worst_m2:.3f}")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[3]], ids=[IDS[0], IDS[2], IDS[3]])
def test_thin_tail_guards(cuda, dtype, shape):
    """Every pointer of the op inside guard bands (tests/guards.py), the workspace exactly as long as the query says: nothing outside z,
    the statistics or the workspace changes, no input is written, no guard byte enters the arithmetic, and the results equal the unguarded
    run bit for bit."""
    from test_gpu_guards import _run_case

    _l, lib = _lib()
    B, L, C, C2, rw, _ = shape
    c = _case(dtype, shape)
    nws = int(lib.sf_op_thin_tail_workspace_bytes(_l.DTYPES[dtype], C, C2))
    assert nws > 0

    def run(a):
        ins = {n: a.inp(c[n], n) for n in NAMES}
        z = a.out((B, L, C), TD[dtype], "z_out")
        st = a.out((B, (L + rw - 1) // rw, G, 2), torch.float32, "stats_out")
        wk = a.ws(nws, "ws")
        rc = _call(lib, _l, cuda, dtype, shape, rw, {n: t.ptr for n, t in ins.items()}, z.ptr, st.ptr, wk.ptr, nws)
        return rc, [z, st]

    _run_case(cuda, "sf_op_thin_tail", run)


@pytest.mark.parametrize("what", ["rw_not_a_multiple_of_32", "C_48", "null_modulation"])
def test_thin_tail_refusals(cuda, what):
    """Unsupported arguments: a non-zero code, and no output or workspace byte written."""
    _l, lib = _lib()
    B, L, C, C2, rw = 2, 96, 64, 32, 32
    if what == "rw_not_a_multiple_of_32":
        rw = 48
    if what == "C_48":
        C = 48
    t = torch.zeros(B, L, 64, dtype=torch.bfloat16, device=cuda)
    f = torch.zeros(4 * 64 * 64 + B * L * 2, device=cuda)
    z = torch.full((B, L, 64), 7.0, dtype=torch.bfloat16, device=cuda)
    st = torch.full((B * L * 2,), 7.0, device=cuda)
    ws = torch.full((1 << 20,), 7, dtype=torch.uint8, device=cuda)
    used = ctypes.c_int(-1)
    rc = lib.sf_op_thin_tail(_l.DTYPES["bf16"], t.data_ptr(), t.data_ptr(), t.data_ptr(), 64, C2, C2, f.data_ptr(), 3, 32, f.data_ptr(), f.data_ptr(),
                             f.data_ptr(), f.data_ptr(), 8, 1e-5, None if what == "null_modulation" else f.data_ptr(), 1e-6, f.data_ptr(),
                             f.data_ptr(), None, B, L, C, rw, z.data_ptr(), st.data_ptr(), ctypes.byref(used), ws.data_ptr(), ws.numel(),
                             _l.stream_ptr(cuda))
    torch.cuda.synchronize()
    assert rc != 0 and used.value == -1
    assert bool((z == 7.0).all()) and bool((st == 7.0).all()) and bool((ws == 7).all())
