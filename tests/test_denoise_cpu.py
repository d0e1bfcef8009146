"""CPU suite of the spectral-gating denoiser (no GPU): the fp64 restatement of tests/denoise_ref.py against the scipy composition it
restates (scipy.signal.stft / filtfilt / fftconvolve / istft) to 1e-10 at every test shape, the chunking host functions, the C ABI's
symbols and refusals (all before any device call) and the command-line tool's --device cpu round trip."""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import scipy.signal
import torch

import denoise_ref as R
from syncfusion_amd import _lib, denoise
from syncfusion_amd.generation import load_wav, save_wav

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE_SYMBOLS = ("sf_spectral_gate_create", "sf_spectral_gate_destroy", "sf_spectral_gate_frames", "sf_spectral_gate_workspace_bytes",
                "sf_stft_forward", "sf_istft_forward", "sf_spectral_gate_noise_threshold", "sf_spectral_gate")
TOL = 1e-10


def scipy_gate(x, sr, n_fft, hop, stationary=False, thresh=None, prop=1.0):
    """noisereduce's composition of scipy calls, as the issue restates it"""
    _, _, S = scipy.signal.stft(x, nfft=n_fft, nperseg=n_fft, noverlap=n_fft - hop, padded=False)
    A = np.abs(S)
    n_f, n_t = int(500 / (sr / (n_fft / 2))), int(50 / (hop / sr * 1000))
    v = np.outer(R.triangle(n_f), R.triangle(n_t))
    v = v / v.sum()
    if stationary:
        db = 20 * np.log10(np.maximum(A, 1e-20))
        db = np.maximum(db, db.max() - 80)
        raw = (db > thresh[:, None]).astype(np.float64)
        m = scipy.signal.fftconvolve(raw * prop + (1 - prop), v, mode="same")
    else:
        t = 2.0 * sr / hop
        b = (np.sqrt(1 + 4 * t ** 2) - 1) / (2 * t ** 2)
        sm = scipy.signal.filtfilt([b], [1, b - 1], A, axis=-1, padtype=None)
        raw = 1 / (1 + np.exp(-(((A - sm) / sm - 2) * 10)))
        m = scipy.signal.fftconvolve(raw, v, mode="same") * prop + (1 - prop)
    _, y = scipy.signal.istft(S * m, nfft=n_fft, nperseg=n_fft, noverlap=n_fft - hop)
    return S, raw, m, y


@pytest.mark.parametrize("n_fft,hop,L", R.SHAPES)
def test_restatement_equals_scipy(n_fft, hop, L):
    rows = R.make_rows(L, 5).astype(np.float64)
    for r in (0, 2, 3):                                   # row 1 is all zero: 0 / 0 in scipy, the documented deviation
        x = rows[r]
        for prop in (1.0, 0.8):
            S, raw, m, y = scipy_gate(x, R.SR, n_fft, hop, prop=prop)
            ref = R.gate_ref(x, R.SR, n_fft, hop, prop_decrease=prop)
            assert ref["spec"].shape == S.shape == (n_fft // 2 + 1, L // hop + 1)
            scale = np.abs(x).max()
            assert np.abs(ref["spec"] - S).max() <= TOL * scale
            assert np.abs(ref["mask_raw"] - raw).max() <= TOL
            assert np.abs(ref["mask_smooth"] - m).max() <= TOL
            n = (S.shape[1] - 1) * hop
            assert y.shape[0] == n
            assert np.abs(ref["out"][:n] - y).max() <= TOL * scale
            assert not ref["out"][n:].any()               # the tail behind the last frame stays zero
        # stationary, the row as its own noise clip
        th = R.stationary_threshold(R.stft_ref(x, n_fft, hop))
        db = 20 * np.log10(np.maximum(np.abs(S), 1e-20))
        db = np.maximum(db, db.max() - 80)
        assert np.abs(th - (db.mean(axis=1) + 1.5 * db.std(axis=1))).max() <= 1e-9
        S, raw, m, y = scipy_gate(x, R.SR, n_fft, hop, stationary=True, thresh=th, prop=0.9)
        ref = R.gate_ref(x, R.SR, n_fft, hop, stationary=True, thresh=th, prop_decrease=0.9, mask_raw=raw)
        assert np.abs(ref["mask_smooth"] - m).max() <= TOL
        assert np.abs(ref["out"][:y.shape[0]] - y).max() <= TOL * np.abs(x).max()
    zero = R.gate_ref(rows[1], R.SR, n_fft, hop)
    assert not zero["out"].any() and not zero["mask_raw"].any()


def test_stft_pair_alone_equals_scipy_with_short_window():
    x = R.make_rows(3000, 1)[0].astype(np.float64)
    _, _, S = scipy.signal.stft(x, nfft=256, nperseg=200, noverlap=200 - 50, padded=False)
    ref = R.stft_ref(x, 256, 50, 200)
    assert ref.shape == S.shape and np.abs(ref - S).max() <= TOL
    _, y = scipy.signal.istft(S, nfft=256, nperseg=200, noverlap=150)
    assert np.abs(R.istft_ref(ref, 256, 50, 200) - y).max() <= TOL


def test_package_host_pieces_match_the_restatement():
    for n_fft, hop, _ in R.SHAPES:
        vf, vt = denoise.smoothing_taps(R.SR, n_fft, hop, 500.0, 50.0)
        n_f, n_t = R.smoothing_counts(R.SR, n_fft, hop)
        assert (vf.size, vt.size) == (2 * n_f + 1, 2 * n_t + 1)
        full = np.outer(R.triangle(n_f), R.triangle(n_t))
        assert np.abs(np.outer(vf, vt) - full / full.sum()).max() <= 1e-15
        assert denoise.smoothing_coefficient(2.0, R.SR, hop) == pytest.approx(R.smoothing_coefficient(2.0, R.SR, hop), rel=1e-15)
    assert (denoise.smoothing_taps(R.SR, 256, 64, 500.0, 50.0)[0].size, denoise.smoothing_taps(R.SR, 256, 64, 500.0, 50.0)[1].size) == (3, 75)
    assert [v.size for v in denoise.smoothing_taps(R.SR, 1024, 256, 500.0, 50.0)] == [11, 19]
    cfg = denoise.SpectralGateConfig()
    assert (cfg.hop, cfg.win, cfg.chunk_size, cfg.padding, cfg.stationary) == (256, 1024, 600000, 30000, False)


@pytest.mark.parametrize("L", [1000, 4096, 8192, 10000])     # below, equal to, a multiple of and not a multiple of chunk_size
def test_chunk_rows_then_merge_rows_is_the_identity(L):
    chunk, pad = 4096, 512
    y = np.random.default_rng(L).standard_normal((2, L)).astype(np.float32)
    chunks = denoise.chunk_rows(L, chunk, pad)
    assert len(chunks) == -(-L // chunk) and sum(c.count for c in chunks) == L
    for data in (y, torch.from_numpy(y)):
        rows = denoise.split_rows(data, chunks)
        assert tuple(rows.shape) == (2 * len(chunks), chunk + 2 * pad)
        back = denoise.merge_rows(rows, chunks, 2, L)
        assert np.array_equal(np.asarray(back), y)
    rows = denoise.split_rows(y, chunks)
    n = len(chunks)
    for k, c in enumerate(chunks):                           # zeros outside the clip, the clip's own samples inside
        for i in (0, c.keep - 1, c.keep, c.length - 1):
            s = c.start + i
            assert rows[n + k, i] == (y[1, s] if 0 <= s < L else 0.0)


def test_chunked_path_equals_the_per_chunk_restatement():
    L, chunk, pad, n_fft, hop = 2500, 1024, 256, 256, 64
    y = R.make_rows(L, 2).astype(np.float64)
    chunks = denoise.chunk_rows(L, chunk, pad)
    rows = denoise.split_rows(y, chunks)
    out = np.stack([R.gate_ref(r, R.SR, n_fft, hop)["out"] for r in rows])
    merged = denoise.merge_rows(out, chunks, 2, L)
    ref = R.reduce_noise_ref(y, R.SR, n_fft=n_fft, hop=hop, chunk_size=chunk, padding=pad)
    assert np.array_equal(merged, ref)
    whole = R.gate_ref(y[0], R.SR, n_fft, hop)["out"]
    assert not np.array_equal(whole, ref[0])                 # chunking is not a no-op: the recurrence restarts in every chunk


def test_symbols_declared_bound_and_exported():
    import syncfusion_amd

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "syncfusion_amd.h")).read()
    declared = set(re.findall(r"\b(sf_[a-z0-9_]+)\s*\(", header))
    for name in GATE_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/syncfusion_amd.h"
        assert name in _lib.SYMBOLS, f"{name} is not bound in _lib.py"
        assert hasattr(lib, name), f"{name} is not exported"
    for name in ("denoise", "SpectralGateConfig", "reduce_noise", "stft", "istft", "chunk_rows", "merge_rows"):
        assert name in syncfusion_amd.__all__ and hasattr(syncfusion_amd, name)


def _create(n_fft=256, win=256, hop=64, center=1, pad_mode=0, taps=(1.0,)):
    t = np.asarray(taps, dtype=np.float32)
    h = C.c_void_p()
    rc = _lib.load().sf_spectral_gate_create(n_fft, win, hop, center, pad_mode, 1, t.ctypes.data, t.size, t.ctypes.data, t.size, C.byref(h))
    return rc, h.value


def test_python_refusals_happen_without_a_device():
    x = torch.zeros(4000)
    for bad in (1000, 128, 8192):
        with pytest.raises(ValueError, match="n_fft"):
            denoise.stft(x, bad, 64)
        with pytest.raises(ValueError, match="n_fft"):
            denoise.reduce_noise(x.numpy(), 48000, n_fft=bad)
    with pytest.raises(ValueError, match="shorter than the window"):
        denoise.stft(torch.zeros(100), 256, 64)
    with pytest.raises(ValueError, match="shorter than the window"):
        denoise.reduce_noise(np.zeros(100, dtype=np.float32), 48000, n_fft=256, padding=0)
    spec = torch.zeros(129, 10, dtype=torch.complex64)
    with pytest.raises(ValueError, match="NOLA"):
        denoise.istft(spec, 256, 256)
    with pytest.raises(ValueError, match="NOLA"):
        denoise.istft(spec, 256, 300)
    with pytest.raises(ValueError, match="NOLA"):
        denoise.reduce_noise(x.numpy(), 48000, n_fft=256, hop_length=256)
    assert denoise.nola_min(256, 64) == pytest.approx(1.5, rel=1e-12)    # hann^2 at four equally spaced phases: 4 * 3/8
    assert denoise.nola_min(256, 96) > 0.5
    with pytest.raises(_lib.SyncFusionAmdError, match="no CPU execution path"):       # valid arguments, no device: an error, not a fallback
        denoise.reduce_noise(x.numpy(), 48000, n_fft=256, device="cpu")


def test_c_abi_refusals_happen_without_a_device():
    lib = _lib.load()
    for n_fft in (1000, 128, 8192):
        rc, h = _create(n_fft=n_fft, win=n_fft)
        assert rc != 0 and not h and b"n_fft" in lib.sf_last_error()
    assert _create(win=300)[0] != 0 and _create(hop=0)[0] != 0 and _create(pad_mode=2)[0] != 0 and _create(taps=(0.5, 0.5))[0] != 0
    rc, h = _create()
    assert rc == 0 and h
    fake = C.c_void_p(4096)          # never dereferenced: every call below is refused before the first HIP call
    try:
        assert lib.sf_spectral_gate_frames(h, 3000) == 47 and lib.sf_spectral_gate_frames(h, 255) == -1
        assert lib.sf_spectral_gate_workspace_bytes(h, 1, 255) == -1 and lib.sf_spectral_gate_workspace_bytes(h, 0, 3000) == -1
        need = lib.sf_spectral_gate_workspace_bytes(h, 2, 3000)
        r256 = lambda n: (n + 255) // 256 * 256      # a real plane, a complex plane, the windowed frames, one float per row
        assert need == r256(2 * 47 * 129 * 4) + r256(2 * 47 * 129 * 8) + r256(2 * 47 * 256 * 4) + r256(2 * 4)
        assert lib.sf_stft_forward(h, fake, 1, 255, fake, None) != 0 and b"shorter than the window" in lib.sf_last_error()
        assert lib.sf_stft_forward(h, None, 1, 3000, fake, None) != 0
        assert lib.sf_stft_forward(h, fake, 70000, 3000, fake, None) != 0
        assert lib.sf_spectral_gate(h, fake, 2, 3000, 0, 0.1, 2.0, 10.0, 1.0, 0, None, fake, fake, fake, fake, fake, need - 1, None) != 0
        assert b"workspace" in lib.sf_last_error()
        assert lib.sf_spectral_gate(h, fake, 2, 3000, 1, 0.1, 2.0, 10.0, 1.0, 0, None, fake, fake, fake, fake, fake, need, None) != 0   # no thresholds
        assert lib.sf_spectral_gate(h, fake, 2, 3000, 0, 0.0, 2.0, 10.0, 1.0, 0, None, fake, fake, fake, fake, fake, need, None) != 0   # b = 0
        assert lib.sf_spectral_gate(h, fake, 2, 3000, 0, 0.1, 2.0, 10.0, 1.5, 0, None, fake, fake, fake, fake, fake, need, None) != 0   # prop > 1
        assert lib.sf_istft_forward(h, fake, 1, 47, fake, 3000, fake, 16, None) != 0 and b"workspace" in lib.sf_last_error()
        assert lib.sf_spectral_gate_noise_threshold(h, fake, 1, 3000, -1.0, fake, fake, need, None) != 0
    finally:
        lib.sf_spectral_gate_destroy(h)
    rc, h = _create(hop=256)         # hop = window: w[0] = 0 is never covered
    assert rc == 0
    try:
        assert lib.sf_stft_forward(h, None, 1, 3000, fake, None) != 0
        assert lib.sf_istft_forward(h, fake, 1, 12, fake, 3000, fake, 1 << 30, None) != 0 and b"NOLA" in lib.sf_last_error()
        assert lib.sf_spectral_gate(h, fake, 1, 3000, 0, 0.1, 2.0, 10.0, 1.0, 0, None, fake, fake, fake, fake, fake, 1 << 30, None) != 0
        assert b"NOLA" in lib.sf_last_error()
    finally:
        lib.sf_spectral_gate_destroy(h)


def _tool():
    spec = importlib.util.spec_from_file_location("preprocess_audio", os.path.join(ROOT, "tools", "preprocess_audio.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_round_trip_on_the_host(tmp_path):
    sr, n = 16000, 3200                                      # 0.2 s
    x = torch.from_numpy(R.make_rows(n, 1)[:1] * 0.5)
    save_wav(tmp_path / "clip.resampled.wav", x, sr)
    save_wav(tmp_path / "other.wav", x, sr)                  # not a *.resampled.wav: left alone
    tool = _tool()
    ref = R.reduce_noise_ref(x.numpy(), sr, n_fft=1024, hop=256)
    assert tool.main(["--input_dir", str(tmp_path), "--device", "cpu"]) == 0
    out, rate = load_wav(tmp_path / "clip.resampled_denoised.wav")
    assert rate == sr and tuple(out.shape) == (1, n)
    assert np.array_equal(out.numpy(), ref.astype(np.float32))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["clip.resampled.wav", "clip.resampled_denoised.wav", "other.wav"]
    assert tool.main(["--input_dir", str(tmp_path), "--device", "cpu", "--audio_bitdepth", "16", "--stationary"]) == 0
    out16, _ = load_wav(tmp_path / "clip.resampled_denoised.wav")
    ref_s = R.reduce_noise_ref(x.numpy(), sr, n_fft=1024, hop=256, stationary=True)
    assert np.abs(out16.numpy() - ref_s).max() <= 0.5 / 32768 + 1e-7
    with pytest.raises(SystemExit, match="24-bit"):
        tool.main(["--input_dir", str(tmp_path), "--audio_bitdepth", "24"])
    with pytest.raises(SystemExit, match="no \\*.resampled.wav"):
        tool.main(["--input_dir", str(tmp_path / "nowhere")])
