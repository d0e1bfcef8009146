"""Inpainting sampler on the MI355X: device noise against the fp64 restatement, ``DiffusionModel.inpaint`` against the oracle loop
(tests/inpaint_ref.py) fed the device's own draws, the bit-exact identities of the loop, graph replay against eager (cached graphs with
new seed / source / mask included), guard bands around one ``sf_vinpaint`` call, and the generation API on top."""
import functools

import numpy as np
import pytest
import torch

import inpaint_ref
from helpers import SMALL_UNET, oracle_params, rel_l2, small_encoder_module, synth_inputs
from test_gpu_guards import _G, _bytes, _unet_args
from test_gpu_models import FP32_TOL, _small_diffusion

pytestmark = pytest.mark.gpu

B, L0 = 2, 16 * 44
SEED = (3 << 32) | 12345
# Largest |device - fp64 restatement| over the draws of test_noise_matches_restatement, measured on the MI355X: 3.52e-7 (logf, sqrtf and
# sincospif of this ROCm at radii up to 5.8).  The gate is 4x that -- the margin covers other seeds -- and stays far below 2e-5, above which
# something other than rounding is wrong.
NOISE_MEASURED = 3.52e-7
NOISE_GATE = 4 * NOISE_MEASURED
assert NOISE_GATE <= 2e-5


@functools.lru_cache(maxsize=None)
def _model(dtype="fp32"):
    return _small_diffusion(torch.device("cuda:0"), dtype)


def _case(cuda, batch=B, seed=31):
    """(source, keep mask, start noise, conditioning kwargs) on the device; the mask edges are off every multiple of 4."""
    x0, _, emb, chans = synth_inputs(SMALL_UNET, batch, L0, seed=seed)
    src = torch.randn(batch, 1, L0, generator=torch.Generator().manual_seed(seed + 1)) * 0.5
    mask = torch.zeros(batch, 1, L0, dtype=torch.bool)
    for b in range(batch):
        for lo, hi in (((0, 37), (401, 530)), ((5, 111), (333, 702)))[b % 2]:
            mask[b, 0, lo + b // 2:hi + b // 2] = True
    cond = dict(channels=[c.to(cuda) for c in chans], embedding=emb.to(cuda))
    return src.to(cuda), mask.to(cuda), x0.to(cuda), cond


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. noise
# ---------------------------------------------------------------------------------------------------------------------------------
def test_noise_matches_restatement(cuda):
    from syncfusion_amd.diffusion import philox_normal

    worst = 0.0
    for seed, k, off, n in [(SEED, 0, 0, 4099), (SEED, 1000, 0, 4099), (SEED, 1, 1027, 1001), (77, 3, 2, 5), (SEED, 2, (1 << 34) + 5, 67)]:
        dev = philox_normal((n,), seed, k, cuda, elem_offset=off)
        assert torch.equal(dev, philox_normal((n,), seed, k, cuda, elem_offset=off)), "two calls must give the same bits"
        ref = inpaint_ref.philox_normal(seed, k, off, n)
        worst = max(worst, float(np.abs(dev.cpu().double().numpy() - ref).max()))
    print(f"philox_normal: largest |device - fp64| = {worst:.3e} (gate {NOISE_GATE:.3e})")
    assert worst < NOISE_GATE
    big = philox_normal((B, 1, 4099), SEED, 1000, cuda).reshape(-1)
    assert torch.equal(philox_normal((1001,), SEED, 1000, cuda, elem_offset=1027), big[1027:2028]), "a draw at an offset is a slice of the larger draw"
    assert not torch.equal(big[:4099], philox_normal((4099,), SEED, 999, cuda)) and not torch.equal(big[:4099], philox_normal((4099,), SEED + 1, 1000, cuda))


def test_noise_statistics(cuda):
    from syncfusion_amd.diffusion import philox_normal

    z = philox_normal((inpaint_ref.STAT_N,), inpaint_ref.STAT_SEED, 0, cuda).double()
    mean, var = float(z.mean()), float(z.var(unbiased=False))
    print(f"philox_normal over 2**20 draws: mean {mean:.3e}, var - 1 {var - 1:.3e}")
    assert bool(torch.isfinite(z).all())
    assert abs(mean) < inpaint_ref.MEAN_GATE and abs(var - 1.0) < inpaint_ref.VAR_GATE


def test_update_launch_is_independent_of_range_split_and_alignment(cuda):
    """One sf_op_vinpaint_update over [0, n), n = 4099: the 16-byte path with its element-wise ends.  Cut into ranges that start and end
    off the group boundaries (what a branch slice could do) and run from pointers that are not 16-byte aligned (element-wise throughout)
    it must give the same bits; against fp64 it is held to the roundings of its fp32 operations."""
    from syncfusion_amd import _lib

    lib = _lib.load()
    n, k, scale, seed = 4099, 3, 2.0, SEED
    g = torch.Generator().manual_seed(17)
    x0, v, vu, src = (torch.randn(n, generator=g) for _ in range(4))
    mask = torch.rand(n, generator=g) < 0.4
    ang = torch.rand(8, generator=g) * (np.pi / 2)
    sched = torch.stack([torch.cos(ang[:4]), torch.sin(ang[:4]), torch.cos(ang[4:]), torch.sin(ang[4:])], dim=1).contiguous()     # rows (a0, b0, a1, b1)
    step = torch.tensor([k], dtype=torch.int32, device=cuda)
    words = torch.from_numpy(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32).view(np.int32)).to(cuda)
    sched_d = sched.to(cuda)

    def run(ranges, shift):
        def dev(t):                                    # the tensor at an offset of `shift` elements from a fresh allocation
            buf = torch.zeros(n + 4, dtype=t.dtype, device=cuda)
            buf[shift:shift + n] = t.to(cuda)
            return buf, buf[shift:shift + n]
        (_, xd), (_, vd), (_, ud), (_, sd), (_, md) = (dev(t) for t in (x0, v, vu, src, mask.to(torch.uint8)))
        for e0, e1 in ranges:
            _lib.check(lib.sf_op_vinpaint_update(xd.data_ptr(), vd.data_ptr(), ud.data_ptr(), scale, sd.data_ptr(), md.data_ptr(), sched_d.data_ptr(),
                                                 step.data_ptr(), words.data_ptr(), e0, e1, _lib.stream_ptr(cuda)), "sf_op_vinpaint_update")
        return xd.cpu()

    whole = run([(0, n)], 0)
    assert torch.equal(whole, run([(0, 1027), (1027, 2050), (2050, 2051), (2051, n)], 0)), "ranges cut off the group boundaries"
    assert torch.equal(whole, run([(0, n)], 1)), "pointers off the 16-byte boundary"
    a0, b0, a1, b1 = (float(c) for c in sched[k].double())
    xx, vv = x0.double(), vu.double() + (v.double() - vu.double()) * scale
    z = torch.from_numpy(inpaint_ref.philox_normal(seed, k, 0, n))
    ref = torch.where(mask, a1 * src.double() + b1 * z, a1 * (a0 * xx - b0 * vv) + b1 * (b0 * xx + a0 * vv))
    # at most 8 fp32 roundings on the way to an element, each below 2**-24 of the largest intermediate magnitude, plus the noise gate
    big = float(torch.stack([xx.abs(), vv.abs(), src.double().abs(), z.abs()]).max()) * 2.0
    gate = 8 * 2.0 ** -24 * big + NOISE_GATE
    err = float((whole.double() - ref).abs().max())
    print(f"sf_op_vinpaint_update vs fp64: max abs {err:.3e} (gate {gate:.3e})")
    assert err < gate


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. loop parity
# ---------------------------------------------------------------------------------------------------------------------------------
T, R = 5, 3


@functools.lru_cache(maxsize=None)
def _oracle_inpaint(scale):
    """The oracle loop on the device's own draws (they do not depend on the engine's dtype or on graph use): once per guidance scale."""
    from oracle import unet_ref
    from syncfusion_amd.diffusion import philox_normal

    cuda = torch.device("cuda:0")
    m = _model("fp32")
    src, mask, x0, cond = _case(cuda)
    P, cfg = oracle_params(m.net, "net."), dict(m.net.hparams)
    emb, chans = cond["embedding"].cpu(), [c.cpu() for c in cond["channels"]]

    def net(x, sig):
        return unet_ref.unet_forward(P, cfg, x, sig, embedding=emb, channels=chans, embedding_scale=scale)

    return inpaint_ref.vinpaint(net, src.cpu(), mask.cpu(), T, R, x0.cpu(), lambda k: philox_normal((B, 1, L0), SEED, k, cuda).cpu())


@pytest.mark.parametrize("dtype", ["fp32", "fp32x"])
@pytest.mark.parametrize("graph", [True, False], ids=["graphed", "eager"])
@pytest.mark.parametrize("scale", [1.0, 2.0])
def test_inpaint_parity(cuda, scale, graph, dtype):
    m = _model(dtype)
    src, mask, x0, cond = _case(cuda)
    ref = _oracle_inpaint(scale)
    m.inpainter.use_graph = graph
    out = m.inpaint(src, mask, T, R, x_noisy=x0, seed=SEED, embedding_scale=scale, **cond)
    m.inpainter.use_graph = True
    e = rel_l2(out.cpu(), ref)
    print(f"inpaint parity scale {scale} {'graph' if graph else 'eager'} {dtype}: rel-L2 {e:.3e}")
    assert out.shape == src.shape and e < FP32_TOL


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. identities (bit-exact)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,scale", [(2, 2.0), (2, 1.0), (4, 1.0)], ids=["guided", "unguided", "branches"])
def test_one_resample_without_mask_is_sample(cuda, batch, scale):
    m = _model()
    src, _, x0, cond = _case(cuda, batch)
    none = torch.zeros_like(src, dtype=torch.bool)
    for graph in (True, False):
        m.sampler.use_graph = graph
        want = m.sample(x_noisy=x0, num_steps=6, embedding_scale=scale, **cond)
        m.inpainter.use_graph = graph
        got = m.inpaint(src, none, 6, 1, x_noisy=x0, seed=SEED, embedding_scale=scale, **cond)
        m.sampler.use_graph = m.inpainter.use_graph = True
        assert torch.equal(got, want), f"graph={graph}"


def test_full_mask_returns_source(cuda):
    m = _small_diffusion(cuda)
    src, _, x0, cond = _case(cuda)
    full = torch.ones(B, 1, 1, dtype=torch.bool, device=cuda)               # broadcast over the samples
    assert torch.equal(m.inpaint(src, full, 4, 2, x_noisy=x0, seed=SEED, embedding_scale=2.0, **cond), src)
    params = dict(m.net.named_parameters())
    params["blocks.0.up.weight"].zero_()                                    # the output convolution: v == 0 everywhere
    params["blocks.0.up.bias"].zero_()
    assert torch.equal(m.inpaint(src, full, 4, 2, x_noisy=x0, seed=SEED, embedding_scale=2.0, **cond), src)


def test_partial_mask_keeps_source_bits(cuda):
    m = _model()
    src, mask, x0, cond = _case(cuda)
    out = m.inpaint(src, mask, 4, 2, x_noisy=x0, seed=SEED, embedding_scale=2.0, **cond)
    assert torch.equal(out[mask], src[mask])
    assert not torch.equal(out[~mask], src[~mask]) and bool(torch.isfinite(out).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. graph replay against eager (bit-equal)
# ---------------------------------------------------------------------------------------------------------------------------------
def _eager(m, *a, **k):
    m.inpainter.use_graph = False
    try:
        return m.inpaint(*a, **k)
    finally:
        m.inpainter.use_graph = True


@pytest.mark.parametrize("batch,scale", [(2, 2.0), (4, 1.0)], ids=["guided", "branches"])
def test_graph_equals_eager_and_cached_graph_takes_new_arguments(cuda, batch, scale):
    """Three calls of one shape with different seed, source and mask: the second and third replay the first call's graph, and must use
    THEIR arguments (nothing that changes between calls may be baked into the captured launch).  batch 4 without guidance is the
    independent-branch path: each branch updates its slice with the global element index."""
    m = _small_diffusion(cuda)
    eng = m.net.engine()
    src, mask, x0, cond = _case(cuda, batch)
    kw = dict(embedding_scale=scale, **cond)
    c0 = eng.graph_captures()
    calls = [(src, mask, x0, SEED), (src.flip(-1) * 0.7, mask.flip(-1), x0.flip(0), SEED + (1 << 33)), (src * -1.0, ~mask, x0 * 0.5, 5)]
    got = []
    for i, (s_, m_, x_, seed) in enumerate(calls):
        got.append(m.inpaint(s_, m_, 3, 2, x_noisy=x_, seed=seed, **kw))
        if i == 0:
            c1 = eng.graph_captures()
            assert c1 > c0, "the graphed call did not capture a step graph"
            if batch == 4:
                assert c1 - c0 == 2, "batch 4 without guidance: one single-stream graph per branch"
    assert eng.graph_captures() == c1, "a later call of the same shape must replay the cached graph"
    for (s_, m_, x_, seed), g_ in zip(calls, got):
        assert torch.equal(g_, _eager(m, s_, m_, 3, 2, x_noisy=x_, seed=seed, **kw))
        assert torch.equal(g_[m_], s_[m_])
    assert not torch.equal(got[0], got[1])


def test_sample_and_inpaint_alternate_on_their_own_graphs(cuda):
    m = _small_diffusion(cuda)
    eng = m.net.engine()
    src, mask, x0, cond = _case(cuda)
    kw = dict(embedding_scale=2.0, **cond)
    first, caps = [], []
    for rnd in range(3):
        s = m.sample(x_noisy=x0, num_steps=6, **kw)
        i = m.inpaint(src, mask, 3, 2, x_noisy=x0, seed=SEED, **kw)           # 6 iterations: the same table size as sample()'s
        caps.append(eng.graph_captures())
        if rnd == 0:
            first = [s, i]
        else:
            assert torch.equal(s, first[0]) and torch.equal(i, first[1])
    # (the first inpaint() grows the engine's workspace, so the second sample() captures once more on the new buffer)
    assert caps[2] == caps[1], "once the workspace has its size, both loops replay their cached graphs"
    m.sampler.use_graph = False
    assert torch.equal(first[0], m.sample(x_noisy=x0, num_steps=6, **kw))
    assert torch.equal(first[1], _eager(m, src, mask, 3, 2, x_noisy=x0, seed=SEED, **kw))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def test_inputs_unchanged_seed_decides(cuda):
    m = _model()
    src, mask, x0, cond = _case(cuda)
    keep = [t.clone() for t in (src, mask, x0)]
    kw = dict(x_noisy=x0, embedding_scale=2.0, **cond)
    a = m.inpaint(src, mask, 3, 2, seed=SEED, **kw)
    assert all(torch.equal(t, k) for t, k in zip((src, mask, x0), keep))
    assert torch.equal(a, m.inpaint(src, mask, 3, 2, seed=SEED, **kw))
    assert not torch.equal(a, m.inpaint(src, mask, 3, 2, seed=SEED + 1, **kw))
    torch.manual_seed(11)                                                     # seed=None: drawn from torch's CPU generator
    b = m.inpaint(src, mask, 3, 2, **kw)
    torch.manual_seed(11)
    assert torch.equal(b, m.inpaint(src, mask, 3, 2, **kw))
    assert m.inpaint(src, mask, 3, 2, seed=SEED, embedding_scale=2.0, **cond).shape == src.shape      # x_noisy=None: drawn on the device


def test_bad_arguments_raise(cuda):
    m = _model()
    src, mask, x0, cond = _case(cuda)
    with pytest.raises(ValueError):
        m.inpaint(src, mask, 3, 0, x_noisy=x0, seed=1, **cond)
    with pytest.raises(ValueError):
        m.inpaint(src, mask[:, :, :-1], 3, 2, x_noisy=x0, seed=1, **cond)
    with pytest.raises(TypeError):
        m.inpaint(src, mask.float(), 3, 2, x_noisy=x0, seed=1, **cond)
    from syncfusion_amd import _lib

    lib, eng = _lib.load(), m.net.engine()
    assert lib.sf_vinpaint_workspace_bytes(eng.handle, B, L0, 1, 3, 0) < 0 and lib.sf_vinpaint_workspace_bytes(eng.handle, B, L0, 1, 0, 2) < 0
    assert lib.sf_vinpaint(eng.handle, x0.data_ptr(), None, mask.data_ptr(), None, None, B, L0, 3, 2, 1, 1.0, 1, None, 0, None) == 1       # SF_ERR_INVALID
    # the inpainting loop leaves sf_vsample's workspace as it was: its own is larger by the source, the mask and the seed slot
    ns, ni = lib.sf_vsample_workspace_bytes(eng.handle, B, L0, 1, 6), lib.sf_vinpaint_workspace_bytes(eng.handle, B, L0, 1, 3, 2)
    assert 0 < ns < ni <= ns + B * L0 * 5 + 3 * 256


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. guard bands
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graphed"])
def test_vinpaint_guard_bands(cuda, use_graph):
    from syncfusion_amd import _lib as _l

    lib = _l.load()
    m = _small_diffusion(cuda)
    eng = m.net.engine()
    Bg, Lg, steps, res, scale = 3, 16 * 7, 2, 2, 2.0
    x, _, emb, chans = synth_inputs(SMALL_UNET, Bg, Lg, seed=4)
    g0 = torch.Generator().manual_seed(9)
    src = torch.randn(Bg, 1, Lg, generator=g0)
    mask = torch.rand(Bg, 1, Lg, generator=g0) < 0.4
    plain = eng.inpaint(src.to(cuda), mask.to(cuda), steps, res, [c.to(cuda) for c in chans], emb.to(cuda), scale, x_noisy=x.to(cuda), seed=SEED,
                        use_graph=use_graph)
    torch.cuda.synchronize()
    nws = int(lib.sf_vinpaint_workspace_bytes(eng.handle, Bg, Lg, 1, steps, res))
    assert nws > 0
    g = _G(cuda)
    _, _, es, cs, arr = _unet_args(g, x, None, emb, chans)
    g.items.pop(0)                      # (x is the in/out buffer below, not an input)
    xio = g.inout(x, "x_inout")
    ss, ms = g.inp(src, "source"), g.inp(mask.to(torch.uint8), "mask")
    wk = g.ws(nws, "ws")
    rc = lib.sf_vinpaint(eng.handle, xio.ptr, ss.ptr, ms.ptr, arr, es.ptr, Bg, Lg, steps, res, SEED, scale, int(use_graph), wk.ptr, nws,
                         _l.stream_ptr(cuda))
    assert rc == 0, lib.sf_last_error().decode()
    g.verify_all()
    assert bool(torch.isfinite(xio.payload).all())
    assert torch.equal(_bytes(xio.payload), _bytes(plain))


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


def test_generate_long_joins_windows_exactly(cuda, full_small_model):
    from syncfusion_amd import generate_long, long_windows

    model = full_small_model
    length, overlap = L0, 96
    total = 2 * length - 100
    y, z = _track(B, total, 3)
    kw = dict(num_steps=3, embedding_scale=2.0)
    out = generate_long(model, y, z, length=length, overlap=overlap, num_resamples=2, seed=100, generator=torch.Generator(device=cuda).manual_seed(8), **kw)
    assert out.shape == (B, 1, total) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    # the same windows composed by hand from sample() and inpaint()
    gen = torch.Generator(device=cuda).manual_seed(8)
    emb = model.clap_encode_audio(z.to(cuda))
    windows = long_windows(total, length, overlap)
    assert windows == [(0, 0), (length - 100, 100)]
    hand, yd = [], y.to(cuda)
    for w, (start, kept) in enumerate(windows):
        chans = model.onsets_encoder(yd[:, :, start:start + length].contiguous(), with_info=True)[1]["xs"][2:-1]
        noise = torch.randn((B, 1, length), device=cuda, generator=gen)
        if w == 0:
            hand.append(model.model.sample(x_noisy=noise, channels=chans, embedding=emb, **kw))
        else:
            prev_tail = hand[-1][:, :, length - kept:]
            src = torch.zeros(B, 1, length, device=cuda)
            src[:, :, :kept] = prev_tail
            mask = torch.zeros(B, 1, length, dtype=torch.bool, device=cuda)
            mask[:, :, :kept] = True
            hand.append(model.model.inpaint(src, mask, 3, 2, x_noisy=noise, seed=100 + w, channels=chans, embedding=emb, embedding_scale=2.0))
            assert torch.equal(hand[-1][:, :, :kept], prev_tail), "a window's kept prefix is the previous window's tail"
    assert torch.equal(out[:, :, :length], torch.cat([hand[0][:, :, :length - 100], hand[1][:, :, :100]], dim=-1))
    assert torch.equal(out[:, :, length - 100:], hand[1])
    assert torch.equal(out[:, :, length - 100:length], hand[0][:, :, length - 100:])


def test_inpaint_batch_regions_and_mask_agree(cuda, full_small_model):
    from syncfusion_amd import inpaint_batch, regions_to_keep_mask

    model = full_small_model
    y, z = _track(B, L0, 4)
    audio = torch.randn(B, 1, L0, generator=torch.Generator().manual_seed(6)) * 0.3
    noise = torch.randn(B, 1, L0, generator=torch.Generator().manual_seed(7))
    regions = [[(37, 401), (530, 530)], [(0, 5), (111, 333), (333, 350)]]
    keep = regions_to_keep_mask(regions, B, L0)
    kw = dict(num_steps=3, num_resamples=2, embedding_scale=2.0, seed=9, noise=noise)
    a = inpaint_batch(model, audio, y, z, regions=regions, **kw)
    b = inpaint_batch(model, audio, y, z, keep_mask=keep, **kw)
    assert a.shape == audio.shape and torch.equal(a, b)
    assert torch.equal(a.cpu()[keep], audio[keep]) and not torch.equal(a.cpu()[~keep], audio[~keep])
