"""Multistep v-sampler on the MI355X: the update launch element by element against fp64, ``sample(..., solver=)`` against the fp64
restatement of the loop (tests/solver_ref.py) around the oracle U-Net, the untouched default path, graph replay against eager (cached
graphs with a new table included), guard bands around one ``sf_vsample_ms`` call, and the generation API on top."""
import functools

import numpy as np
import pytest
import torch

import solver_ref
from helpers import SMALL_UNET, oracle_params, rel_l2, small_encoder_module, synth_inputs
from test_gpu_guards import _G, _bytes, _unet_args
from test_gpu_models import FP32_TOL, _small_diffusion

pytestmark = pytest.mark.gpu

B, L0 = 2, 16 * 44


@functools.lru_cache(maxsize=None)
def _model(dtype="fp32"):
    return _small_diffusion(torch.device("cuda:0"), dtype)


@functools.lru_cache(maxsize=None)
def _inputs(batch=B, seed=31):
    x0, _, emb, chans = synth_inputs(SMALL_UNET, batch, L0, seed=seed)
    return x0, emb, chans


def _case(cuda, batch=B, seed=31):
    x0, emb, chans = _inputs(batch, seed)
    return x0.to(cuda), dict(channels=[c.to(cuda) for c in chans], embedding=emb.to(cuda))


def _schedule(name):
    from syncfusion_amd.diffusion import LinearSchedule, PowerSchedule

    return {"default": LinearSchedule(), "linear_0.6_0.1": LinearSchedule(0.6, 0.1), "power": PowerSchedule()}[name]


@functools.lru_cache(maxsize=None)
def _oracle(solver, T, batch, scale, sched="default"):
    """The restated loop around the oracle U-Net (fp64 update, fp32 net): once per case, shared by the engines and by graph / eager."""
    from oracle import unet_ref

    m = _model("fp32")
    x0, emb, chans = _inputs(batch)
    P, cfg = oracle_params(m.net, "net."), dict(m.net.hparams)

    def net(x, sig):
        return unet_ref.unet_forward(P, cfg, x, sig, embedding=emb, channels=chans, embedding_scale=scale)

    with torch.no_grad():
        return solver_ref.multistep_sample(net, x0, _schedule(sched)(T + 1).numpy(), solver)


def _sample(m, graph, *a, **k):
    m.sampler.use_graph = graph
    try:
        return m.sample(*a, **k)
    finally:
        m.sampler.use_graph = True


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the update launch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [False, True], ids=["no_vu", "scale2"])
def test_update_launch_is_independent_of_range_split_and_alignment(cuda, guided):
    """One sf_op_vsampler_update_ms over [0, n), n = 4099: the 16-byte path with its element-wise ends.  Cut into ranges off the group
    boundaries and run from pointers one element off the 16-byte boundary (element-wise throughout) it must give the same bits in x and
    in the history; against fp64 both are held to the roundings of their fp32 operations."""
    from syncfusion_amd import _lib
    from syncfusion_amd.solvers import pack_table, solver_table

    lib = _lib.load()
    n, k, scale = 4099, 3, 2.0
    g = torch.Generator().manual_seed(23)
    x0, v, vu, h0 = (torch.randn(n, generator=g) for _ in range(4))
    tab = pack_table(solver_table(np.linspace(1.0, 0.0, 9, dtype=np.float32), "ab2"))
    assert tab[k, 4] != 0.0
    tab_d = torch.from_numpy(tab).to(cuda)
    step = torch.tensor([k], dtype=torch.int32, device=cuda)

    def run(ranges, shift):
        def dev(t):                                    # the tensor at an offset of `shift` elements from a fresh allocation
            buf = torch.zeros(n + 4, dtype=t.dtype, device=cuda)
            buf[shift:shift + n] = t.to(cuda)
            return buf[shift:shift + n]
        xd, vd, ud, hd = (dev(t) for t in (x0, v, vu, h0))
        for e0, e1 in ranges:
            _lib.check(lib.sf_op_vsampler_update_ms(xd.data_ptr(), vd.data_ptr(), ud.data_ptr() if guided else None, scale, hd.data_ptr(),
                                                    tab_d.data_ptr(), step.data_ptr(), e0, e1, _lib.stream_ptr(cuda)), "sf_op_vsampler_update_ms")
        return xd.cpu(), hd.cpu()

    wx, wh = run([(0, n)], 0)
    cx_, ch_ = run([(0, 1027), (1027, 2050), (2050, 2051), (2051, n)], 0)
    assert torch.equal(wx, cx_) and torch.equal(wh, ch_), "ranges cut off the group boundaries"
    sx, sh = run([(0, n)], 1)
    assert torch.equal(wx, sx) and torch.equal(wh, sh), "pointers off the 16-byte boundary"
    al, be, cx, c0, c1 = (float(c) for c in tab[k, :5].astype(np.float64))
    xx, hh = x0.double(), h0.double()
    vg = vu.double() + (v.double() - vu.double()) * scale if guided else v.double()
    X = al * xx - be * vg
    ref = cx * xx + c0 * X + c1 * hh
    # at most 8 fp32 roundings on the way to an element, each below 2**-24 of the largest intermediate magnitude
    gate = 8 * 2.0 ** -24 * (2.0 * float(torch.stack([xx.abs(), vg.abs(), hh.abs()]).max()) * float(np.abs(tab[k, :5]).max()))
    ex, eh = float((wx.double() - ref).abs().max()), float((wh.double() - X).abs().max())
    print(f"sf_op_vsampler_update_ms vs fp64: x {ex:.3e}, hist {eh:.3e} (gate {gate:.3e})")
    assert ex < gate and eh < gate


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. loop parity
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp32x"])
@pytest.mark.parametrize("solver", ["ab2", "dpmpp_2m"])
@pytest.mark.parametrize("graph", [True, False], ids=["graphed", "eager"])
@pytest.mark.parametrize("batch,scale", [(2, 1.0), (2, 2.0), (4, 1.0)], ids=["unguided", "guided", "branches"])
def test_multistep_parity(cuda, batch, scale, graph, solver, dtype):
    m = _model(dtype)
    x0, cond = _case(cuda, batch)
    ref = _oracle(solver, 5, batch, scale)
    out = _sample(m, graph, x_noisy=x0, num_steps=5, embedding_scale=scale, solver=solver, **cond)
    e = rel_l2(out.cpu().double(), ref)
    print(f"multistep parity {solver} B={batch} scale {scale} {'graph' if graph else 'eager'} {dtype}: rel-L2 {e:.3e}")
    assert out.shape == x0.shape and out.dtype == torch.float32 and e < FP32_TOL


@pytest.mark.parametrize("dtype", ["fp32", "fp32x"])
@pytest.mark.parametrize("solver", ["ab2", "dpmpp_2m"])
@pytest.mark.parametrize("T", [1, 2])
def test_multistep_parity_short_loops(cuda, T, solver, dtype):
    m = _model(dtype)
    x0, cond = _case(cuda)
    out = _sample(m, False, x_noisy=x0, num_steps=T, embedding_scale=2.0, solver=solver, **cond)
    e = rel_l2(out.cpu().double(), _oracle(solver, T, B, 2.0))
    print(f"multistep parity {solver} T={T} eager {dtype}: rel-L2 {e:.3e}")
    assert e < FP32_TOL


@pytest.mark.parametrize("dtype", ["fp32", "fp32x"])
@pytest.mark.parametrize("solver,sched", [("ab2", "linear_0.6_0.1"), ("dpmpp_2m", "power"), ("ddim", "linear_0.6_0.1")])
def test_multistep_parity_other_schedules(cuda, solver, sched, dtype):
    m = _model(dtype)
    x0, cond = _case(cuda)
    out = m.sample(x_noisy=x0, num_steps=5, embedding_scale=2.0, solver=solver, schedule=_schedule(sched), **cond)
    e = rel_l2(out.cpu().double(), _oracle(solver, 5, B, 2.0, sched))
    print(f"multistep parity {solver} on {sched} {dtype}: rel-L2 {e:.3e}")
    assert e < FP32_TOL
    # the constructor's schedule and explicit sigmas are the same call
    from syncfusion_amd.diffusion import VSampler

    s2 = VSampler(m.net, schedule=_schedule(sched), solver=solver)
    assert torch.equal(out, s2(x0, 5, embedding_scale=2.0, **cond))
    assert torch.equal(out, m.sample(x_noisy=x0, num_steps=5, embedding_scale=2.0, solver=solver, sigmas=_schedule(sched)(6), **cond))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the default path
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,scale", [(2, 2.0), (4, 1.0)], ids=["guided", "branches"])
def test_default_path_is_untouched(cuda, batch, scale):
    from syncfusion_amd.diffusion import LinearSchedule

    m = _model()
    x0, cond = _case(cuda, batch)
    kw = dict(x_noisy=x0, num_steps=6, embedding_scale=scale, **cond)
    want = m.sample(**kw)
    eng = m.net.engine()
    c0 = eng.graph_captures()
    assert torch.equal(want, m.sample(solver="ddim", **kw))
    assert torch.equal(want, m.sample(solver="ddim", schedule=LinearSchedule(1.0, 0.0), **kw))
    assert eng.graph_captures() == c0, "solver='ddim' on the default schedule replays sf_vsample's cached graph"
    # the first-order table through sf_vsample_ms is the same rule with other roundings: close, and on its own graph
    via_ms = m.sample(solver="ddim", sigmas=LinearSchedule()(7), **kw)
    assert eng.graph_captures() > c0
    assert rel_l2(via_ms.cpu(), want.cpu()) < FP32_TOL


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. graph replay against eager (bit-equal), cached graphs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,scale", [(2, 2.0), (4, 1.0)], ids=["guided", "branches"])
def test_graph_equals_eager_and_cached_graph_takes_new_table(cuda, batch, scale):
    """Three calls of one shape: the second and third replay the first call's graph with another solver's table, another schedule and
    another x_noisy, and must use THEIR arguments.  batch 4 without guidance is the independent-branch path: each branch updates its
    slice of x and of the history."""
    m = _small_diffusion(cuda)
    eng = m.net.engine()
    x0, cond = _case(cuda, batch)
    kw = dict(num_steps=4, embedding_scale=scale, **cond)
    calls = [(x0, "ab2", "default"), (x0.flip(0) * 0.5, "dpmpp_2m", "power"), (-x0, "ab2", "linear_0.6_0.1")]
    c0 = eng.graph_captures()
    got = []
    for i, (x_, solver, sched) in enumerate(calls):
        got.append(m.sample(x_noisy=x_, solver=solver, schedule=_schedule(sched), **kw))
        if i == 0:
            c1 = eng.graph_captures()
            assert c1 > c0, "the graphed call did not capture a step graph"
            if batch == 4:
                assert c1 - c0 == 2, "batch 4 without guidance: one single-stream graph per branch"
    assert eng.graph_captures() == c1, "a later call of the same shape must replay the cached graph"
    for (x_, solver, sched), g_ in zip(calls, got):
        assert torch.equal(g_, _sample(m, False, x_noisy=x_, solver=solver, schedule=_schedule(sched), **kw)), (solver, sched)
    assert not torch.equal(got[0], got[1])


def test_sample_inpaint_and_multistep_alternate_on_their_own_graphs(cuda):
    m = _small_diffusion(cuda)
    eng = m.net.engine()
    x0, cond = _case(cuda)
    src = x0.flip(-1) * 0.3
    mask = torch.zeros_like(x0, dtype=torch.bool)
    mask[:, :, 37:401] = True
    kw = dict(embedding_scale=2.0, **cond)
    first, caps = [], []
    for rnd in range(3):
        s = m.sample(x_noisy=x0, num_steps=6, **kw)
        i = m.inpaint(src, mask, 3, 2, x_noisy=x0, seed=5, **kw)             # 6 iterations: the same table size
        a = m.sample(x_noisy=x0, num_steps=6, solver="ab2", **kw)
        caps.append(eng.graph_captures())
        if rnd == 0:
            first = [s, i, a]
        else:
            assert torch.equal(s, first[0]) and torch.equal(i, first[1]) and torch.equal(a, first[2])
    # (the first round grows the engine's workspace twice, so the second round captures once more on the final buffer)
    assert caps[2] == caps[1], "once the workspace has its size, the three loops replay their cached graphs"
    assert not torch.equal(first[0], first[2])
    assert torch.equal(first[0], _sample(m, False, x_noisy=x0, num_steps=6, **kw))
    assert torch.equal(first[2], _sample(m, False, x_noisy=x0, num_steps=6, solver="ab2", **kw))
    m.inpainter.use_graph = False
    assert torch.equal(first[1], m.inpaint(src, mask, 3, 2, x_noisy=x0, seed=5, **kw))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. guard bands
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graphed"])
def test_vsample_ms_guard_bands(cuda, use_graph):
    from syncfusion_amd import _lib as _l
    from syncfusion_amd.solvers import pack_table, solver_table

    lib = _l.load()
    m = _small_diffusion(cuda)
    eng = m.net.engine()
    Bg, Lg, steps, scale = 3, 16 * 7, 4, 2.0
    x, _, emb, chans = synth_inputs(SMALL_UNET, Bg, Lg, seed=4)
    sig = np.linspace(1.0, 0.0, steps + 1, dtype=np.float32)
    tab = pack_table(solver_table(sig, "ab2"))
    plain = eng.sample_ms(x.to(cuda), sig, tab, [c.to(cuda) for c in chans], emb.to(cuda), scale, use_graph=use_graph)
    torch.cuda.synchronize()
    nws = int(lib.sf_vsample_ms_workspace_bytes(eng.handle, Bg, Lg, 1, steps))
    assert nws > 0
    g = _G(cuda)
    _, _, es, cs, arr = _unet_args(g, x, None, emb, chans)
    g.items.pop(0)                      # (x is the in/out buffer below, not an input)
    xio = g.inout(x, "x_inout")
    wk = g.ws(nws, "ws")
    rc = lib.sf_vsample_ms(eng.handle, xio.ptr, arr, es.ptr, Bg, Lg, steps, scale, sig.ctypes.data, tab.ctypes.data, int(use_graph), wk.ptr, nws,
                           _l.stream_ptr(cuda))
    assert rc == 0, lib.sf_last_error().decode()
    g.verify_all()
    assert bool(torch.isfinite(xio.payload).all())
    assert torch.equal(_bytes(xio.payload), _bytes(plain))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. inputs and bad arguments
# ---------------------------------------------------------------------------------------------------------------------------------
def test_inputs_unchanged_and_repeatable(cuda):
    m = _model()
    x0, cond = _case(cuda)
    keep = x0.clone()
    a = m.sample(x_noisy=x0, num_steps=4, embedding_scale=2.0, solver="ab2", **cond)
    assert torch.equal(x0, keep)
    assert torch.equal(a, m.sample(x_noisy=x0, num_steps=4, embedding_scale=2.0, solver="ab2", **cond))
    assert bool(torch.isfinite(a).all())
    assert not torch.equal(a, m.sample(x_noisy=x0, num_steps=4, embedding_scale=2.0, solver="dpmpp_2m", schedule=_schedule("power"), **cond))


def test_bad_arguments_raise(cuda):
    from syncfusion_amd import _lib
    from syncfusion_amd.diffusion import VSampler
    from syncfusion_amd.solvers import pack_table, solver_table

    m = _model()
    x0, cond = _case(cuda)
    with pytest.raises(ValueError):
        m.sample(x_noisy=x0, num_steps=4, solver="heun", **cond)
    with pytest.raises(ValueError):
        VSampler(m.net, solver="heun")
    with pytest.raises(ValueError):
        m.sample(x_noisy=x0, num_steps=4, solver="ab2", sigmas=torch.linspace(1, 0, 4), **cond)        # 4 values for 4 steps
    with pytest.raises(ValueError):
        m.sample(x_noisy=x0, num_steps=3, solver="ab2", sigmas=torch.tensor([1.0, 0.5, 0.5, 0.0]), **cond)
    lib, eng = _lib.load(), m.net.engine()
    sig = np.linspace(1.0, 0.0, 5, dtype=np.float32)
    tab = pack_table(solver_table(sig, "ab2"))
    ctx = [c.contiguous() for c in cond["channels"]]
    nws = int(lib.sf_vsample_ms_workspace_bytes(eng.handle, B, L0, 0, 4))
    assert nws > 0 and lib.sf_vsample_ms_workspace_bytes(eng.handle, B, L0, 0, 0) < 0
    ws = torch.empty(nws, dtype=torch.uint8, device=cuda)
    x = x0.clone()

    def call(sigmas, table, nbytes):
        return lib.sf_vsample_ms(eng.handle, x.data_ptr(), _lib.ptr_array(ctx), cond["embedding"].data_ptr(), B, L0, 4, 1.0, sigmas.ctypes.data,
                                 table.ctypes.data, 0, ws.data_ptr(), nbytes, _lib.stream_ptr(cuda))

    assert call(sig, tab, nws - 1) != 0 and "workspace" in lib.sf_last_error().decode()               # one byte short
    assert torch.equal(x, x0), "a refused call leaves x alone"
    assert call(sig[::-1].copy(), tab, nws) == 1                                                        # SF_ERR_INVALID: increasing sigmas
    bad = tab.copy()
    bad[2, 3] = np.nan
    assert call(sig, bad, nws) == 1
    assert call(sig, tab, nws) == 0
    torch.cuda.synchronize()
    # the multistep loop leaves sf_vsample's workspace as it was: its own is larger by the history and the table
    ns = lib.sf_vsample_workspace_bytes(eng.handle, B, L0, 0, 4)
    assert 0 < ns < nws <= ns + B * L0 * 4 + 1024 * 32 + 2 * 256


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. generation API
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_small_model(cuda):
    from syncfusion_amd import Model, RandomEmbedder

    return Model(1e-4, 0.95, 0.999, 1e-6, 1e-3, _small_diffusion(cuda), small_encoder_module().to(cuda), RandomEmbedder(SMALL_UNET["embedding_features"]),
                 None).to(cuda)


def _track(batch, total, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.zeros(batch, 1, total)
    for b in range(batch):
        y[b, 0, torch.randint(0, total, (6,), generator=g)] = 1.0
    return y, torch.randn(batch, 1, 2048, generator=g) * 0.1


def _conditioning(model, y, z, cuda):
    chans = model.onsets_encoder(y.to(cuda), with_info=True)[1]["xs"][2:-1]
    return dict(channels=chans, embedding=model.clap_encode_audio(z.to(cuda)))


def test_vary_batch_is_the_hand_composition(cuda, full_small_model):
    import math

    from syncfusion_amd import LinearSchedule, vary_batch
    from syncfusion_amd.diffusion import philox_normal

    model = full_small_model
    y, z = _track(B, L0, 5)
    audio = (torch.randn(B, 1, L0, generator=torch.Generator().manual_seed(6)) * 0.3).to(cuda)
    kw = dict(strength=0.4, num_steps=4, embedding_scale=2.0)
    out = vary_batch(model, audio, y, z, seed=11, **kw)
    assert out.shape == audio.shape and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    angle = 0.4 * math.pi / 2
    x_noisy = math.cos(angle) * audio + math.sin(angle) * philox_normal(tuple(audio.shape), 11, 0, cuda)
    hand = model.model.sample(x_noisy=x_noisy, num_steps=4, embedding_scale=2.0, solver="ab2", schedule=LinearSchedule(0.4, 0.0),
                              **_conditioning(model, y, z, cuda))
    assert torch.equal(out, hand)
    assert not torch.equal(out, vary_batch(model, audio, y, z, seed=12, **kw))
    assert torch.equal(out, vary_batch(model, audio.cpu(), y, z, seed=11, **kw))
    with pytest.raises(ValueError):
        vary_batch(model, audio, y, z, strength=0.0)


def test_generate_batch_takes_solver_and_schedule(cuda, full_small_model):
    from syncfusion_amd import PowerSchedule, generate_batch

    model = full_small_model
    y, z = _track(B, L0, 4)
    noise = torch.randn(B, 1, L0, generator=torch.Generator().manual_seed(7)).to(cuda)
    cond = _conditioning(model, y, z, cuda)
    kw = dict(num_steps=3, length=L0, embedding_scale=2.0, noise=noise)
    a = generate_batch(model, y, z, solver="ab2", **kw)
    assert torch.equal(a, model.model.sample(x_noisy=noise, num_steps=3, embedding_scale=2.0, solver="ab2", **cond))
    b = generate_batch(model, y, z, solver="dpmpp_2m", schedule=PowerSchedule(), **kw)
    assert torch.equal(b, model.model.sample(x_noisy=noise, num_steps=3, embedding_scale=2.0, solver="dpmpp_2m", schedule=PowerSchedule(), **cond))
    plain = generate_batch(model, y, z, **kw)
    assert torch.equal(plain, model.model.sample(x_noisy=noise, num_steps=3, embedding_scale=2.0, **cond))
    assert not torch.equal(a, plain)
