"""FAD evaluation on the device (MI355X) against the fp64 reference of tests/fad_ref.py: the front end, the network (narrow and
full-size configurations, every pool output), the moments and the directory-level call."""
import functools

import numpy as np
import pytest
import torch

import fad_ref
from numerics import check_close

pytestmark = pytest.mark.gpu

FRONT_GATE = 2e-6            # of the plane's maximum: the figure tests/test_gpu_audio_features.py holds the fp32 FFT pipeline to against fp64
FP32_GATE = 1e-4             # the project's fp32 rel-L2 figure (check_close adds the max-error bound)
# end to end against the all-fp64 pipeline: measured relative error of the FAD on MI355X (see test_end_to_end_*), gated at 10 x that
# because summation orders differ between boxes through 9 layers, and never above 1e-3
E2E_MEASURED = {16000: 2.5e-7, 22050: 6.2e-6}
E2E_CEILING = 1e-3


def narrow_model(device=None, seed=11):
    from syncfusion_amd.fad import VGGish, VGGishConfig

    m = VGGish(VGGishConfig(layout=fad_ref.NARROW_LAYOUT, fc=fad_ref.NARROW_FC))
    m.load_state_dict(fad_ref.seeded_weights(fad_ref.NARROW_LAYOUT, fad_ref.NARROW_FC, seed))
    return m.to(device) if device is not None else m


# ---- front end ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def front_reference(B, L):
    wav = fad_ref.clip_signal(B, L, 100 + B)
    ex, mel = fad_ref.examples(wav.double().numpy())
    return wav, ex, mel


@pytest.mark.parametrize("L", [15600, 30959, 31000])
@pytest.mark.parametrize("B", [1, 3])
def test_front_end_against_fp64(cuda, B, L):
    model = narrow_model()
    wav, ex_ref, mel_ref = front_reference(B, L)
    E = fad_ref.example_count(L)
    x = wav.to(cuda)
    mel = model.mel_magnitude(x).double().cpu().numpy()
    rows = model.example_rows(x)
    ex = model.examples(x).double().cpu().numpy()
    assert mel.shape == (B, E * 96, 64) == mel_ref.shape and ex.shape == (B, E, 96, 64) == ex_ref.shape
    assert rows.shape == (B * E * 96 * 64, 4) and bool((rows[:, 1:] == 0).all()), "columns 1 .. 3 of the example rows must be exactly zero"
    assert np.array_equal(rows[:, 0].double().cpu().numpy().reshape(ex.shape), ex)
    for b in range(B):
        peak = mel_ref[b].max()
        err = np.abs(mel[b] - mel_ref[b]).max()
        log_ref = ex_ref[b].reshape(-1, 64)
        bound = FRONT_GATE * peak / (mel_ref[b] + fad_ref.LOG_OFFSET) + 4 * 2.0 ** -24 * np.abs(log_ref)
        lerr = np.abs(ex[b].reshape(-1, 64) - log_ref)
        worst = float((lerr / bound).max())
        print(f"B {B} L {L} clip {b}: mel max err / plane max {err / peak:.3e} (gate {FRONT_GATE:.0e}); log plane worst err / bound {worst:.3f}")
        assert np.isfinite(mel[b]).all() and err <= FRONT_GATE * peak
        assert np.isfinite(ex[b]).all() and worst <= 1.0


def test_front_end_short_clip_is_empty_without_a_launch(cuda):
    from syncfusion_amd import _lib

    model = narrow_model()
    calls = []
    lib = _lib.load()
    real = lib.sf_logmel_examples_forward
    x = fad_ref.clip_signal(2, 15599, 5).to(cuda)
    try:
        lib.sf_logmel_examples_forward = lambda *a: calls.append(a) or real(*a)
        ex = model.examples(x)
        emb = model(x)
    finally:
        lib.sf_logmel_examples_forward = real
    assert tuple(ex.shape) == (2, 0, 96, 64) and tuple(emb.shape) == (0, 24) and not calls


# ---- network --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def five_examples():
    """Five examples of one clip from the reference front end, rounded to fp32: (5, 96, 64)."""
    L = 400 + (5 * 96 - 1) * 160
    ex, _ = fad_ref.examples(fad_ref.clip_signal(1, L, 42).double().numpy())
    assert ex.shape == (1, 5, 96, 64)
    return torch.from_numpy(ex[0]).float()


@functools.lru_cache(maxsize=None)
def network_reference(kind, seed):
    layout, fc = (fad_ref.NARROW_LAYOUT, fad_ref.NARROW_FC) if kind == "narrow" else (fad_ref.FULL_LAYOUT, fad_ref.FULL_FC)
    state = fad_ref.seeded_weights(layout, fc, seed)
    ex = five_examples() if kind == "narrow" else five_examples()[:2]
    emb, pools = fad_ref.network(state, layout, fc, ex)          # examples are independent: the first N rows are the reference of N examples
    return state, emb, pools


def rows_of(ex, device):
    rows = torch.zeros((ex.numel(), 4), dtype=torch.float32)
    rows[:, 0] = ex.reshape(-1)
    return rows.to(device)


def run_network(cuda, kind, N):
    from syncfusion_amd.fad import VGGish, VGGishConfig

    state, emb_ref, pools_ref = network_reference(kind, 11)
    cfg = VGGishConfig(layout=fad_ref.NARROW_LAYOUT, fc=fad_ref.NARROW_FC) if kind == "narrow" else VGGishConfig()
    model = VGGish(cfg)
    model.load_state_dict(state)
    model = model.to(cuda)
    emb, pools = model.embed_rows(rows_of(five_examples()[:N], cuda), pool_taps=True)
    assert len(pools) == len(pools_ref) == 4
    for i, (p, r) in enumerate(zip(pools, pools_ref)):       # a layout slip shows here before the FC layers hide it
        check_close(p, r[:N], FP32_GATE, f"{kind} N={N} pool {i} {tuple(p.shape)}", dims=("example", "h", "w", "channel"))
    check_close(emb, emb_ref[:N], FP32_GATE, f"{kind} N={N} embeddings", dims=("example", "dim"))
    assert float(emb_ref.min()) < 0, "without the final ReLU the embeddings take both signs"


@pytest.mark.parametrize("N", [1, 3, 5])
def test_network_narrow_against_fp64(cuda, N):
    run_network(cuda, "narrow", N)


def test_network_full_size_against_fp64(cuda):
    run_network(cuda, "full", 2)


def test_network_final_relu_switch(cuda):
    from syncfusion_amd.fad import VGGish, VGGishConfig

    state, emb_ref, _ = network_reference("narrow", 11)
    model = VGGish(VGGishConfig(layout=fad_ref.NARROW_LAYOUT, fc=fad_ref.NARROW_FC, final_relu=True))
    model.load_state_dict(state)
    emb = model.to(cuda).embed_rows(rows_of(five_examples()[:3], cuda))
    check_close(emb, emb_ref[:3].clamp_min(0), FP32_GATE, "narrow, final ReLU on", dims=("example", "dim"))


# ---- moments --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [24, 128])
@pytest.mark.parametrize("N", [2, 97, 1000])
def test_moments_against_numpy_fp64(cuda, N, D):
    from syncfusion_amd.fad import embedding_moments, embedding_statistics

    g = torch.Generator().manual_seed(N * 131 + D)
    x = torch.randn(N, D, generator=g)
    x[:, ::5] += 30.0                                             # offsets of 30 sigma in some columns: a one-pass variance would lose digits
    x[:, 3] -= 30.0
    xd = x.to(cuda)
    mu, sigma, n = embedding_statistics(xd)
    ref = x.double().numpy()
    mu_ref, sigma_ref = ref.mean(axis=0), np.cov(ref, rowvar=False)
    e_mu, e_sig = np.abs(mu - mu_ref).max() / np.abs(mu_ref).max(), np.abs(sigma - sigma_ref).max() / np.abs(sigma_ref).max()
    print(f"N {N} D {D}: mu err {e_mu:.2e}, sigma err {e_sig:.2e} (gates 1e-10)")
    assert n == N and mu.dtype == np.float64 and sigma.dtype == np.float64
    assert e_mu <= 1e-10 and e_sig <= 1e-10
    assert np.array_equal(sigma, sigma.T)
    a, b = embedding_moments(xd), embedding_moments(xd)          # identical input, identical bits
    assert np.array_equal(a.sum, b.sum) and np.array_equal(a.scatter, b.scatter)
    cut = max(1, N // 3)
    mu2, sigma2, n2 = embedding_moments(xd[:cut]).merge(embedding_moments(xd[cut:])).statistics()
    assert n2 == N
    assert np.abs(mu2 - mu_ref).max() <= 1e-10 * np.abs(mu_ref).max() and np.abs(sigma2 - sigma_ref).max() <= 1e-10 * np.abs(sigma_ref).max()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def make_clips(sr):
    """Eight generated clips (decaying sinusoid bursts) and eight background clips (enveloped white noise) of 1.5 s, fp32 (8, n)."""
    n = int(1.5 * sr)
    g = torch.Generator().manual_seed(77)
    t = torch.arange(n, dtype=torch.float64) / sr
    gen, gt = [], []
    for i in range(8):
        x = torch.zeros(n, dtype=torch.float64)
        for k in range(3):
            t0 = 0.1 + 0.4 * k + 0.03 * i
            m = (t >= t0).double()
            x += 0.6 * m * torch.exp(-(9.0 + i) * (t - t0).clamp_min(0)) * torch.sin(2 * np.pi * (300.0 + 170.0 * i + 90.0 * k) * (t - t0))
        gen.append(x)
        env = 0.15 + 0.35 * torch.sin(np.pi * t / 1.5 * (1 + i % 3)) ** 2
        gt.append(env * torch.randn(n, generator=g, dtype=torch.float64) * 0.5)
    return torch.stack(gen).float().clamp(-1, 1), torch.stack(gt).float().clamp(-1, 1)


def run_end_to_end(cuda, tmp_path, sr):
    from syncfusion_amd import resample
    from syncfusion_amd.fad import embed_clips, evaluate_fad, load_dir
    from syncfusion_amd.generation import save_wav

    gen, gt = make_clips(sr)
    dirs = {"gen": tmp_path / "gen", "gt": tmp_path / "gt"}
    for name, clips in (("gen", gen), ("gt", gt)):
        dirs[name].mkdir()
        for i, c in enumerate(clips):
            save_wav(dirs[name] / f"clip{i}.wav", c[None], sr)
    model = narrow_model(cuda)
    out = evaluate_fad(dirs["gen"], dirs["gt"], model=model)
    assert out["n_gen"] == 8 and out["n_gt"] == 8
    # (a) the plumbing: the reference's statistics and distance on the device's own embeddings
    stats = {}
    for name in ("gen", "gt"):
        embs = embed_clips(load_dir(dirs[name], model.config, cuda), model, cuda)[1]
        stats[name] = fad_ref.statistics(torch.cat(embs).double().cpu().numpy())
    plumb = fad_ref.frechet(*stats["gt"], *stats["gen"])
    rel_a = abs(out["FAD"] - plumb) / abs(plumb)
    # (b) the all-fp64 pipeline; at another rate both sides read this package's resampler output
    state = fad_ref.seeded_weights(fad_ref.NARROW_LAYOUT, fad_ref.NARROW_FC, 11)
    ref_stats = {}
    for name, clips in (("gen", gen), ("gt", gt)):
        w = clips if sr == fad_ref.SR else resample(clips.to(cuda), sr, fad_ref.SR).cpu()
        ex, _ = fad_ref.examples(w.double().numpy())
        emb, _ = fad_ref.network(state, fad_ref.NARROW_LAYOUT, fad_ref.NARROW_FC, torch.from_numpy(ex.reshape(-1, 96, 64)))
        ref_stats[name] = fad_ref.statistics(emb.numpy())
    full = fad_ref.frechet(*ref_stats["gt"], *ref_stats["gen"])
    rel_b = abs(out["FAD"] - full) / abs(full)
    scale = np.trace(ref_stats["gt"][1]) + np.trace(ref_stats["gen"][1])
    print(f"sr {sr}: FAD {out['FAD']:.9g}; on the device's embeddings {plumb:.9g} (rel {rel_a:.2e}, gate 1e-9); all-fp64 pipeline {full:.9g} "
          f"(rel {rel_b:.2e}, gate {min(10 * E2E_MEASURED[sr], E2E_CEILING):.1e}); trace sum {scale:.6g}")
    assert full > 0.05 * scale, "the two sets must be far apart: the distance is no cancellation"
    assert rel_a <= 1e-9
    assert rel_b <= min(10 * E2E_MEASURED[sr], E2E_CEILING)


def test_end_to_end_16k(cuda, tmp_path):
    """evaluate_fad on two directories of eight 1.5 s clips at 16 kHz, narrow network.  Measured on MI355X: relative error of the FAD
    against the all-fp64 pipeline 2.5e-7 (FAD 1.69533631e-06 vs 1.69533588e-06); the gate is 10 x that, capped at 1e-3.  Against
    the reference's statistics and distance on the device's own embeddings: 0 (gate 1e-9)."""
    run_end_to_end(cuda, tmp_path, 16000)


def test_end_to_end_22050(cuda, tmp_path):
    """The same clips stored at 22050 Hz: both sides feed the network this package's resampler output, so only the plumbing differs.
    Measured on MI355X: relative error against the all-fp64 pipeline 6.2e-6 (FAD 1.85897959e-06 vs 1.85899108e-06), gated at 10 x that;
    on the device's own embeddings 1.1e-16 (gate 1e-9)."""
    run_end_to_end(cuda, tmp_path, 22050)
