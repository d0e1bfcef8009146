"""Guidance schedules on the MI355X: the statistics and update launches element by element against fp64, ``sample(...)`` under per-clip /
per-step scales, rescale and interval guidance against the fp64 restatement (tests/guidance_ref.py) around the oracle U-Net, the seams
between segments, graph replay with a new table, and guard bands around one ``sf_vsample_gx`` call."""
import functools

import numpy as np
import pytest
import torch

import guidance_ref
from helpers import SMALL_UNET, oracle_params, rel_l2, synth_inputs
from test_gpu_guards import _G, _bytes, _unet_args
from test_gpu_models import FP32_TOL, _small_diffusion

pytestmark = pytest.mark.gpu

B, L0, T = 2, 16 * 44, 6
SIG = np.linspace(1.0, 0.0, T + 1, dtype=np.float32)
INTERVAL = (0.3, 0.8)                                        # steps 2, 3, 4 of SIG: the plan is single / two / single
RAMP = np.array([[1.0, 1.0], [1.0, 2.0], [2.0, 3.0], [3.0, 1.0], [1.0, 1.0], [0.5, 1.0]])

# name -> (embedding_scale, guidance_rescale, guidance_interval)
CASES = {
    "per_clip": (np.array([1.0, 3.0]), 0.0, None),
    "ramp": (RAMP, 0.0, None),
    "rescale": (4.0, 0.7, None),
    "interval": (3.0, 0.0, INTERVAL),
}


@functools.lru_cache(maxsize=None)
def _model(dtype="fp32"):
    return _small_diffusion(torch.device("cuda:0"), dtype)


@functools.lru_cache(maxsize=None)
def _inputs(batch=B, seed=31):
    x0, _, emb, chans = synth_inputs(SMALL_UNET, batch, L0, seed=seed)
    return x0, emb, chans


def _case(cuda, batch=B):
    x0, emb, chans = _inputs(batch)
    return x0.to(cuda), dict(channels=[c.to(cuda) for c in chans], embedding=emb.to(cuda))


@functools.lru_cache(maxsize=None)
def _oracle(case, solver):
    """The restated loop around the oracle U-Net (fp64 update, fp32 net): once per case, shared by the engines and by graph / eager."""
    scale, phi, interval = CASES[case]
    m = _model("fp32")
    x0, emb, chans = _inputs()
    net_c, net_u = guidance_ref.unet_nets(oracle_params(m.net, "net."), dict(m.net.hparams), emb, chans)
    with torch.no_grad():
        return guidance_ref.sample(net_c, net_u, x0, SIG, solver, guidance_ref.scales(scale, SIG, B, interval), phi)


def _sample(m, graph, *a, **k):
    m.sampler.use_graph = graph
    try:
        return m.sample(*a, **k)
    finally:
        m.sampler.use_graph = True


def _off(t, shift, cuda):
    """The tensor at an offset of `shift` elements from a fresh allocation."""
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device=cuda)
    buf[shift:shift + t.numel()] = t.to(cuda)
    return buf[shift:shift + t.numel()]


def _stats(lib, _lib, cuda, vd, ud, gtab_d, step, nb, clip):
    nbytes = int(lib.sf_op_guidance_stats_bytes(nb, clip))
    assert nbytes > 0
    part = torch.empty(nbytes // 8, dtype=torch.float64, device=cuda)
    _lib.check(lib.sf_op_guidance_stats(vd.data_ptr(), ud.data_ptr() if ud is not None else None, gtab_d.data_ptr(), step.data_ptr(), nb, clip,
                                        part.data_ptr(), nbytes, _lib.stream_ptr(cuda)), "sf_op_guidance_stats")
    return part


def _factor64(v, vu, s, phi):
    g = v.double() if s == 1.0 else vu.double() + s * (v.double() - vu.double())
    sg = float(g.std(unbiased=False))
    return 1.0 if phi == 0.0 or sg == 0.0 else 1.0 + phi * (float(v.double().std(unbiased=False)) / sg - 1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the update launch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi", [0.0, 0.7], ids=["plain", "rescale"])
def test_update_launch_is_independent_of_range_split_and_alignment(cuda, phi):
    """One sf_op_vsampler_update_g over three clips of 1027 elements: 4-groups straddle the clip boundaries (1027 % 4 == 3) and go element
    by element there.  Cut into ranges off the group boundaries, and run from pointers one element off the 16-byte boundary, it must give
    the same bits in x and in the history; against fp64 both are held to the roundings of their fp32 operations.  Clip 0 has scale 1: its
    bits are those of the launch without v_uncond."""
    from syncfusion_amd import _lib
    from syncfusion_amd.solvers import pack_table, solver_table

    lib = _lib.load()
    nb, clip, k = 3, 1027, 3
    n = nb * clip
    scales = [1.0, 3.0, 2.0]
    g = torch.Generator().manual_seed(29)
    x0, v, vu, h0 = (torch.randn(n, generator=g) for _ in range(4))
    tab = pack_table(solver_table(np.linspace(1.0, 0.0, 9, dtype=np.float32), "ab2"))
    assert tab[k, 4] != 0.0
    tab_d = torch.from_numpy(tab).to(cuda)
    gtab = np.full((5, nb), 9.0, dtype=np.float32)             # (only row k is this step's)
    gtab[k] = scales
    gtab_d = torch.from_numpy(gtab).to(cuda)
    step = torch.tensor([k], dtype=torch.int32, device=cuda)

    def run(ranges, shift, with_vu=True):
        xd, vd, ud, hd = (_off(t, shift, cuda) for t in (x0, v, vu, h0))
        if not with_vu:
            ud = None
        part = _stats(lib, _lib, cuda, vd, ud, gtab_d, step, nb, clip) if phi > 0 else None
        fac = torch.full((nb,), -1.0, device=cuda)
        for e0, e1 in ranges:
            _lib.check(lib.sf_op_vsampler_update_g(xd.data_ptr(), vd.data_ptr(), ud.data_ptr() if with_vu else None, hd.data_ptr(), tab_d.data_ptr(),
                                                   gtab_d.data_ptr(), step.data_ptr(), part.data_ptr() if phi > 0 else None, phi, nb, clip,
                                                   fac.data_ptr(), e0, e1, _lib.stream_ptr(cuda)), "sf_op_vsampler_update_g")
        return xd.cpu(), hd.cpu(), fac.cpu()

    wx, wh, wf = run([(0, n)], 0)
    cx_, ch_, cf = run([(0, 1026), (1026, 1027), (1027, 2050), (2050, 2051), (2051, 2057), (2057, n)], 0)
    assert torch.equal(wx, cx_) and torch.equal(wh, ch_) and torch.equal(wf, cf), "ranges cut off the group boundaries"
    sx, sh, sf_ = run([(0, n)], 1)
    assert torch.equal(wx, sx) and torch.equal(wh, sh) and torch.equal(wf, sf_), "pointers off the 16-byte boundary"
    tx, th, _ = run([(0, 1500), (1500, n)], 3)
    assert torch.equal(wx, tx) and torch.equal(wh, th), "pointers off the boundary and a cut range"
    nx, nh, nf = run([(0, n)], 0, with_vu=False)
    assert torch.equal(wx[:clip], nx[:clip]) and torch.equal(wh[:clip], nh[:clip]), "a clip with scale 1 is the launch without v_uncond"
    assert not torch.equal(wx[clip:], nx[clip:])
    assert float(wf[0]) == 1.0 and torch.equal(nf, torch.ones(nb)), "g == v_c: the factor is exactly 1"

    al, be, cx, c0, c1 = (float(c) for c in tab[k, :5].astype(np.float64))
    xx, hh = x0.double(), h0.double()
    f64 = [_factor64(v[b * clip:(b + 1) * clip], vu[b * clip:(b + 1) * clip], scales[b], phi) for b in range(nb)]
    vg = torch.cat([(v[b * clip:(b + 1) * clip].double() if scales[b] == 1.0 else
                     vu[b * clip:(b + 1) * clip].double() + scales[b] * (v[b * clip:(b + 1) * clip].double() - vu[b * clip:(b + 1) * clip].double()))
                    for b in range(nb)])
    vv = torch.cat([vg[b * clip:(b + 1) * clip] * f64[b] for b in range(nb)])
    X = al * xx - be * vv
    ref = cx * xx + c0 * X + c1 * hh
    # The 8 fp32 roundings of sf_op_vsampler_update_ms's path (tests/test_gpu_solvers.py) and two more for the rescale (the factor's own
    # rounding and the product), each below 2**-24 of the largest intermediate magnitude; the factor multiplies the magnitude of v.
    fmax = max(1.0, max(f64))
    gate = 10 * 2.0 ** -24 * (2.0 * float(torch.stack([xx.abs(), vg.abs() * fmax, hh.abs()]).max()) * float(np.abs(tab[k, :5]).max()))
    ex, eh = float((wx.double() - ref).abs().max()), float((wh.double() - X).abs().max())
    ef = max(abs(float(wf[b]) - f64[b]) / f64[b] for b in range(nb))
    print(f"sf_op_vsampler_update_g phi {phi} vs fp64: x {ex:.3e}, hist {eh:.3e} (gate {gate:.3e}); factor rel {ef:.3e}, factors {f64}")
    assert ex < gate and eh < gate
    assert ef <= 2 * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the statistics at offset inputs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [1027, 2 ** 18], ids=["1027", "2^18"])
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "off16"])
def test_rescale_factor_at_offset_inputs(cuda, clip, shift):
    """v_c = 100 + N(0, 1), v_u = 100 + 0.5 N(0, 1): a one-pass fp32 variance loses every digit here.  The factor must be fp64's to two
    fp32 roundings, and the same bits over two runs (fixed-order reduction, no atomics)."""
    from syncfusion_amd import _lib

    lib = _lib.load()
    nb, phi, scales = 2, 0.7, [3.0, 7.5]
    n = nb * clip
    g = torch.Generator().manual_seed(clip)
    v = 100.0 + torch.randn(n, generator=g)
    vu = 100.0 + 0.5 * torch.randn(n, generator=g)
    vd, ud = _off(v, shift, cuda), _off(vu, shift, cuda)
    gtab_d = torch.tensor([scales], dtype=torch.float32, device=cuda)
    tab_d = torch.zeros(8, dtype=torch.float32, device=cuda)
    step = torch.zeros(1, dtype=torch.int32, device=cuda)
    xd, hd = torch.zeros(n, device=cuda), torch.zeros(n, device=cuda)

    def factors():
        part = _stats(lib, _lib, cuda, vd, ud, gtab_d, step, nb, clip)
        fac = torch.full((nb,), -1.0, device=cuda)
        _lib.check(lib.sf_op_vsampler_update_g(xd.data_ptr(), vd.data_ptr(), ud.data_ptr(), hd.data_ptr(), tab_d.data_ptr(), gtab_d.data_ptr(),
                                               step.data_ptr(), part.data_ptr(), phi, nb, clip, fac.data_ptr(), 0, 1, _lib.stream_ptr(cuda)),
                   "sf_op_vsampler_update_g")
        return fac.cpu(), part.cpu()

    f1, p1 = factors()
    f2, p2 = factors()
    assert torch.equal(f1, f2) and torch.equal(p1, p2), "two runs must give the same bits"
    for b in range(nb):
        want = _factor64(v[b * clip:(b + 1) * clip], vu[b * clip:(b + 1) * clip], scales[b], phi)
        rel = abs(float(f1[b]) - want) / want
        print(f"clip of {clip} elements, scale {scales[b]}: factor {float(f1[b]):.9f}, fp64 {want:.12f}, rel {rel:.3e}")
        assert rel <= 2 * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. a constant table without rescale is sample(embedding_scale=s)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False], ids=["graphed", "eager"])
@pytest.mark.parametrize("solver", ["ab2", "ddim"])
def test_constant_table_equals_float_scale(cuda, solver, graph):
    m = _model()
    x0, cond = _case(cuda)
    kw = dict(x_noisy=x0, num_steps=T, solver=solver, sigmas=SIG, **cond)
    want = _sample(m, graph, embedding_scale=2.0, **kw)                      # a float scale on explicit sigmas: sf_vsample_ms
    assert m.sampler.last_segments is None
    for form in (np.full((T, B), 2.0), np.full(B, 2.0), torch.full((T,), 2.0, device=cuda)):
        got = _sample(m, graph, embedding_scale=form, **kw)
        assert m.sampler.last_segments == [(0, T, True)]
        assert torch.equal(got, want)
    ones = _sample(m, graph, embedding_scale=np.ones((T, B)), **kw)          # nothing to guide: one single-pass segment
    assert m.sampler.last_segments == [(0, T, False)]
    assert torch.equal(ones, _sample(m, graph, embedding_scale=1.0, **kw))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. loop parity
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp32x"])
@pytest.mark.parametrize("solver", ["ddim", "ab2"])
@pytest.mark.parametrize("graph", [True, False], ids=["graphed", "eager"])
@pytest.mark.parametrize("case", list(CASES))
def test_guidance_parity(cuda, case, graph, solver, dtype):
    scale, phi, interval = CASES[case]
    m = _model(dtype)
    x0, cond = _case(cuda)
    ref = _oracle(case, solver)
    out = _sample(m, graph, x_noisy=x0, num_steps=T, solver=solver, sigmas=SIG, embedding_scale=scale, guidance_rescale=phi,
                  guidance_interval=interval, **cond)
    e = rel_l2(out.cpu().double(), ref)
    print(f"guidance parity {case} {solver} {'graph' if graph else 'eager'} {dtype}: rel-L2 {e:.3e}, plan {m.sampler.last_segments}")
    assert out.shape == x0.shape and out.dtype == torch.float32 and e < FP32_TOL
    if case == "interval":
        assert m.sampler.last_segments == [(0, 2, False), (2, 5, True), (5, 6, False)]


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. seams
# ---------------------------------------------------------------------------------------------------------------------------------
def _three_calls(m, x0, cond, solver, scale):
    x = x0
    for i0, i1, two in [(0, 2, False), (2, 5, True), (5, 6, False)]:
        x = m.sample(x_noisy=x, num_steps=i1 - i0, solver=solver, sigmas=SIG[i0:i1 + 1], embedding_scale=scale if two else 1.0, **cond)
    return x


def test_seams_ddim_is_three_consecutive_calls(cuda):
    from syncfusion_amd.guidance import evaluation_rows

    m = _model()
    x0, cond = _case(cuda)
    out = m.sample(x_noisy=x0, num_steps=T, solver="ddim", sigmas=SIG, embedding_scale=3.0, guidance_interval=INTERVAL, **cond)
    plan = m.sampler.last_segments
    assert plan == [(0, 2, False), (2, 5, True), (5, 6, False)]
    assert evaluation_rows(plan, B) == 3 * B + 3 * 2 * B < 2 * T * B
    assert torch.equal(out, _three_calls(m, x0, cond, "ddim", 3.0)), "a first-order rule has no history: the cuts are exact"


def test_seams_ab2_carries_the_history(cuda):
    m = _model()
    x0, cond = _case(cuda)
    out = m.sample(x_noisy=x0, num_steps=T, solver="ab2", sigmas=SIG, embedding_scale=3.0, guidance_interval=INTERVAL, **cond)
    plan = m.sampler.last_segments
    restarted = _three_calls(m, x0, cond, "ab2", 3.0)
    assert m.sampler.last_segments is None, "a call without a guidance schedule has no plan"
    d = rel_l2(out.cpu().double(), restarted.cpu().double())
    e = rel_l2(out.cpu().double(), _oracle("interval", "ab2"))
    print(f"ab2 over the seams: carried vs restarted rel-L2 {d:.3e}; carried vs fp64 {e:.3e}")
    assert e < FP32_TOL < d, "the history crosses the seams: the run is the uncut second-order loop, not three first-order starts"
    # the engine's hist_io by hand: the same three calls with ONE history tensor and the rows of the whole table are the run, bit for bit
    from syncfusion_amd import _lib
    from syncfusion_amd.guidance import scale_table
    from syncfusion_amd.solvers import pack_table, solver_table

    lib, eng = _lib.load(), m.net.engine()
    tab, sc = pack_table(solver_table(SIG, "ab2")), scale_table(3.0, SIG, B, INTERVAL)
    ctx = [c.contiguous() for c in cond["channels"]]
    nws = max(int(lib.sf_vsample_gx_workspace_bytes(eng.handle, B, L0, two, T)) for two in (0, 1))
    ws = torch.empty(nws, dtype=torch.uint8, device=cuda)
    x, hist = x0.clone(), torch.zeros_like(x0)
    for i0, i1, two in plan:
        s_sig, s_tab, s_sc = SIG[i0:i1 + 1].copy(), tab[i0:i1].copy(), sc[i0:i1].copy()
        rc = lib.sf_vsample_gx(eng.handle, x.data_ptr(), _lib.ptr_array(ctx), cond["embedding"].data_ptr(), B, L0, i1 - i0, s_sig.ctypes.data,
                               s_tab.ctypes.data, s_sc.ctypes.data, 0.0, hist.data_ptr(), 0, ws.data_ptr(), nws, _lib.stream_ptr(cuda))
        assert rc == 0, lib.sf_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(x, out)
    assert bool((hist != 0).any()), "the history comes back"


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. a new table of the same shape replays the cached graphs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi", [0.0, 0.7], ids=["plain", "rescale"])
def test_new_table_replays_the_cached_graph(cuda, phi):
    m = _small_diffusion(cuda)
    eng = m.net.engine()
    x0, cond = _case(cuda)
    kw = dict(x_noisy=x0, num_steps=T, solver="ab2", sigmas=SIG, guidance_rescale=phi, **cond)
    c0 = eng.graph_captures()
    first = m.sample(embedding_scale=np.array([1.0, 3.0]), **kw)
    c1 = eng.graph_captures()
    assert c1 > c0, "the graphed call did not capture a step graph"
    second = m.sample(embedding_scale=RAMP + 1.0, **kw)                       # another (T, B) table, every step guided
    third = m.sample(embedding_scale=7.5, guidance_interval=(0.0, 1.0), **kw)
    assert eng.graph_captures() == c1, "a table of the same shape must replay the cached graph"
    for got, scale in ((first, np.array([1.0, 3.0])), (second, RAMP + 1.0), (third, np.full((T, B), 7.5))):
        assert torch.equal(got, _sample(m, False, embedding_scale=scale, **kw)), "the replay must read ITS table"
    assert not torch.equal(first, second) and not torch.equal(second, third)
    # another rescale weight is another graph (phi is a kernel argument)
    m.sample(embedding_scale=RAMP + 1.0, **dict(kw, guidance_rescale=0.3))
    assert eng.graph_captures() > c1


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. guard bands
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graphed"])
@pytest.mark.parametrize("two", [True, False], ids=["two", "single"])
def test_vsample_gx_guard_bands(cuda, two, use_graph):
    """One continuing segment (rows 2 .. 5 of a 7-step ab2 table: row 0 has c1 != 0) with a caller's history, per-clip scales and rescale."""
    from syncfusion_amd import _lib as _l
    from syncfusion_amd.solvers import pack_table, solver_table

    lib = _l.load()
    m = _small_diffusion(cuda)
    eng = m.net.engine()
    Bg, Lg, steps, phi = 3, 16 * 7, 4, 0.7
    x, _, emb, chans = synth_inputs(SMALL_UNET, Bg, Lg, seed=4)
    full = np.linspace(1.0, 0.0, 8, dtype=np.float32)
    sig = full[2:2 + steps + 1].copy()
    tab = pack_table(solver_table(full, "ab2"))[2:2 + steps].copy()
    assert tab[0, 4] != 0.0
    sc = np.tile(np.array([[1.0, 3.0, 2.0]], dtype=np.float32), (steps, 1)) if two else None
    h0 = torch.randn(x.shape, generator=torch.Generator().manual_seed(8)) * 0.1
    nws = int(lib.sf_vsample_gx_workspace_bytes(eng.handle, Bg, Lg, int(two), steps))
    assert nws > 0 and (two or nws == int(lib.sf_vsample_ms_workspace_bytes(eng.handle, Bg, Lg, 0, steps)))

    def call(xp, hp, arr, ep, wp):
        return lib.sf_vsample_gx(eng.handle, xp, arr, ep, Bg, Lg, steps, sig.ctypes.data, tab.ctypes.data, sc.ctypes.data if two else None, phi, hp,
                                 int(use_graph), wp, nws, _l.stream_ptr(cuda))

    px, ph = x.to(cuda).clone(), h0.to(cuda).clone()
    pe, pc = emb.to(cuda).contiguous(), [c.to(cuda).contiguous() for c in chans]
    pw = torch.empty(nws, dtype=torch.uint8, device=cuda)
    assert call(px.data_ptr(), ph.data_ptr(), _l.ptr_array(pc), pe.data_ptr(), pw.data_ptr()) == 0, lib.sf_last_error().decode()
    torch.cuda.synchronize()
    g = _G(cuda)
    _, _, es, cs, arr = _unet_args(g, x, None, emb, chans)
    g.items.pop(0)                      # (x is the in/out buffer below, not an input)
    xio = g.inout(x, "x_inout")
    hio = g.inout(h0, "hist_io")
    wk = g.ws(nws, "ws")
    rc = call(xio.ptr, hio.ptr, arr, es.ptr, wk.ptr)
    assert rc == 0, lib.sf_last_error().decode()
    g.verify_all()
    assert bool(torch.isfinite(xio.payload).all()) and bool(torch.isfinite(hio.payload).all())
    assert torch.equal(_bytes(xio.payload), _bytes(px)) and torch.equal(_bytes(hio.payload), _bytes(ph))
    assert not torch.equal(ph.cpu(), h0), "the history is written back"
    # the caller's history is read: another one gives another x
    qx, qh = x.to(cuda).clone(), torch.zeros_like(ph)
    assert call(qx.data_ptr(), qh.data_ptr(), _l.ptr_array(pc), pe.data_ptr(), pw.data_ptr()) == 0
    torch.cuda.synchronize()
    assert not torch.equal(qx, px)


def test_bad_arguments_raise(cuda):
    from syncfusion_amd import _lib
    from syncfusion_amd.solvers import pack_table, solver_table

    m = _model()
    x0, cond = _case(cuda)
    kw = dict(x_noisy=x0, num_steps=T, sigmas=SIG, **cond)
    for bad in (dict(embedding_scale=np.ones(5)), dict(embedding_scale=np.array([1.0, np.nan])), dict(guidance_rescale=1.5),
                dict(guidance_interval=(0.8, 0.3))):
        with pytest.raises(ValueError):
            m.sample(**kw, **bad)
    lib, eng = _lib.load(), m.net.engine()
    tab = pack_table(solver_table(SIG, "ab2"))
    sc = np.full((T, B), 2.0, dtype=np.float32)
    ctx = [c.contiguous() for c in cond["channels"]]
    nws = int(lib.sf_vsample_gx_workspace_bytes(eng.handle, B, L0, 1, T))
    assert nws > int(lib.sf_vsample_gx_workspace_bytes(eng.handle, B, L0, 0, T)) > 0 and lib.sf_vsample_gx_workspace_bytes(eng.handle, B, L0, 1, 0) < 0
    ws = torch.empty(nws, dtype=torch.uint8, device=cuda)
    x = x0.clone()

    def call(scales, phi, nbytes):
        return lib.sf_vsample_gx(eng.handle, x.data_ptr(), _lib.ptr_array(ctx), cond["embedding"].data_ptr(), B, L0, T, SIG.ctypes.data, tab.ctypes.data,
                                 scales.ctypes.data, phi, None, 0, ws.data_ptr(), nbytes, _lib.stream_ptr(cuda))

    assert call(sc, 0.0, nws - 1) != 0 and "workspace" in lib.sf_last_error().decode()
    assert call(sc, 1.5, nws) == 1 and call(sc, -0.5, nws) == 1                                         # SF_ERR_INVALID
    bad = sc.copy()
    bad[3, 1] = np.inf
    assert call(bad, 0.0, nws) == 1
    assert torch.equal(x, x0), "a refused call leaves x alone"
    assert call(sc, 0.0, nws) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, m.sample(embedding_scale=2.0, solver="ab2", **kw))


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. generation API
# ---------------------------------------------------------------------------------------------------------------------------------
def test_generate_batch_takes_the_guidance_arguments(cuda):
    from syncfusion_amd import Model, RandomEmbedder, generate_batch
    from helpers import small_encoder_module

    model = Model(1e-4, 0.95, 0.999, 1e-6, 1e-3, _small_diffusion(cuda), small_encoder_module().to(cuda), RandomEmbedder(SMALL_UNET["embedding_features"]),
                  None).to(cuda)
    g = torch.Generator().manual_seed(4)
    y = torch.zeros(B, 1, L0)
    for b in range(B):
        y[b, 0, torch.randint(0, L0, (6,), generator=g)] = 1.0
    z = torch.randn(B, 1, 2048, generator=g) * 0.1
    noise = torch.randn(B, 1, L0, generator=torch.Generator().manual_seed(7)).to(cuda)
    cond = dict(channels=model.onsets_encoder(y.to(cuda), with_info=True)[1]["xs"][2:-1], embedding=model.clap_encode_audio(z.to(cuda)))
    kw = dict(num_steps=4, length=L0, noise=noise, solver="ab2")
    per_clip = torch.tensor([2.0, 5.0])
    a = generate_batch(model, y, z, embedding_scale=per_clip, guidance_rescale=0.7, guidance_interval=(0.3, 0.9), **kw)
    assert model.model.sampler.last_segments == [(0, 1, False), (1, 3, True), (3, 4, False)]
    assert torch.equal(a, model.model.sample(x_noisy=noise, num_steps=4, solver="ab2", embedding_scale=per_clip, guidance_rescale=0.7,
                                             guidance_interval=(0.3, 0.9), **cond))
    plain = generate_batch(model, y, z, embedding_scale=2.0, **kw)
    assert torch.equal(plain, model.model.sample(x_noisy=noise, num_steps=4, solver="ab2", embedding_scale=2.0, **cond))
    assert not torch.equal(a, plain) and bool(torch.isfinite(a).all())
