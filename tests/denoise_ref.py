"""fp64 restatement of the spectral-gating denoiser (syncfusion_amd/denoise.py), stage by stage, as plain numpy loops: framing with the
padding spelled out, one rfft per frame, the two passes of the one-pole recurrence, the separable mask filter with zeros outside the plane
and the overlap-add with its squared-window envelope.  tests/test_denoise_cpu.py pins every stage to scipy.signal (stft, istft, filtfilt,
fftconvolve); the GPU tests compare the device with it.  Each stage takes its input as an argument, so a test can feed one stage the
device's result of the stage before (for instance the device's binary mask).

Plain module (not a conftest); spectra are (F, T) complex128, masks (F, T) float64.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np


def hann(win: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win, dtype=np.float64) / win)


def n_frames(L: int, win: int, hop: int, center: bool = True) -> int:
    pad = win // 2 if center else 0
    return (L + 2 * pad - win) // hop + 1


def stft_ref(x, n_fft: int, hop: int, win: Optional[int] = None, center: bool = True, pad_mode: str = "constant",
             scaling: Optional[str] = "spectrum") -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    win = n_fft if win is None else win
    L, pad = x.shape[0], (win // 2 if center else 0)
    w = hann(win)
    T = n_frames(L, win, hop, center)
    S = np.zeros((n_fft // 2 + 1, T), dtype=np.complex128)
    for t in range(T):
        frame = np.zeros(n_fft)
        for i in range(win):
            s = t * hop - pad + i
            if pad_mode == "reflect":
                s = -s if s < 0 else s
                s = 2 * (L - 1) - s if s >= L else s
                frame[i] = x[s]
            elif 0 <= s < L:
                frame[i] = x[s]
        frame[:win] *= w
        S[:, t] = np.fft.rfft(frame)
    return S / w.sum() if scaling == "spectrum" else S


def istft_ref(S, n_fft: int, hop: int, win: Optional[int] = None, center: bool = True, scaling: Optional[str] = "spectrum",
              length: Optional[int] = None) -> np.ndarray:
    S = np.asarray(S, dtype=np.complex128)
    win = n_fft if win is None else win
    T, pad = S.shape[1], (win // 2 if center else 0)
    w = hann(win)
    total = win + (T - 1) * hop
    acc, env = np.zeros(total), np.zeros(total)
    for t in range(T):
        frame = np.fft.irfft(S[:, t], n_fft)[:win] * (w.sum() if scaling == "spectrum" else 1.0)
        acc[t * hop:t * hop + win] += frame * w
        env[t * hop:t * hop + win] += w * w
    y = (acc / np.where(env > 1e-10, env, 1.0))[pad:total - pad]
    if length is None:
        return y
    out = np.zeros(length)
    out[:min(length, y.shape[0])] = y[:length]
    return out


def smoothing_coefficient(time_constant_s: float, sr: float, hop: int) -> float:
    t = time_constant_s * sr / hop
    return (math.sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t)


def smooth_time(A: np.ndarray, b: float) -> np.ndarray:
    """forward, then backward, y = b x + (1 - b) y_prev over the last axis, each pass started from y_prev = its first input"""
    A = np.asarray(A, dtype=np.float64)
    T = A.shape[-1]
    fwd, out = np.empty_like(A), np.empty_like(A)
    prev = A[..., 0].copy()
    for t in range(T):
        prev = b * A[..., t] + (1.0 - b) * prev
        fwd[..., t] = prev
    prev = fwd[..., T - 1].copy()
    for t in range(T - 1, -1, -1):
        prev = b * fwd[..., t] + (1.0 - b) * prev
        out[..., t] = prev
    return out


def ns_mask(A: np.ndarray, b: float, mult: float = 2.0, slope: float = 10.0) -> np.ndarray:
    sm = smooth_time(A, b)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = 1.0 / (1.0 + np.exp(-(((A - sm) / sm - mult) * slope)))
    return np.where(sm == 0.0, 0.0, m)      # the documented deviation: a bin silent in every frame


def amp_db(S: np.ndarray) -> np.ndarray:
    db = 20.0 * np.log10(np.maximum(np.abs(S), 1e-20))
    return np.maximum(db, db.max() - 80.0)


def stationary_threshold(S_noise: np.ndarray, n_std: float = 1.5) -> np.ndarray:
    db = amp_db(S_noise)
    F, T = db.shape
    th = np.empty(F)
    for f in range(F):
        mean = db[f].sum() / T
        th[f] = mean + n_std * math.sqrt(((db[f] - mean) ** 2).sum() / T)
    return th


def triangle(n: int) -> np.ndarray:
    return np.concatenate([np.linspace(0.0, 1.0, n + 1, endpoint=False), np.linspace(1.0, 0.0, n + 2)])[1:-1]


def smoothing_counts(sr: float, n_fft: int, hop: int, freq_hz: float = 500.0, time_ms: float = 50.0):
    return int(freq_hz / (sr / (n_fft / 2))), int(time_ms / (hop / sr * 1000.0))


def smooth_mask(mask: np.ndarray, n_f: int, n_t: int) -> np.ndarray:
    """(2 n_f + 1) taps over bins, then (2 n_t + 1) taps over frames, zeros outside the plane"""
    mask = np.asarray(mask, dtype=np.float64)
    F, T = mask.shape
    vf, vt = triangle(n_f), triangle(n_t)
    vf, vt = vf / vf.sum(), vt / vt.sum()
    tmp = np.zeros_like(mask)
    for i in range(2 * n_f + 1):
        d = i - n_f                      # tmp[f] += vf[i] mask[f - d]
        lo, hi = max(0, d), min(F, F + d)
        if hi > lo:
            tmp[lo:hi] += vf[i] * mask[lo - d:hi - d]
    out = np.zeros_like(mask)
    for j in range(2 * n_t + 1):
        d = j - n_t
        lo, hi = max(0, d), min(T, T + d)
        if hi > lo:
            out[:, lo:hi] += vt[j] * tmp[:, lo - d:hi - d]
    return out


def gate_ref(x, sr: float, n_fft: int, hop: int, win: Optional[int] = None, stationary: bool = False, prop_decrease: float = 1.0,
             time_constant_s: float = 2.0, freq_hz: float = 500.0, time_ms: float = 50.0, mult: float = 2.0, slope: float = 10.0,
             thresh: Optional[np.ndarray] = None, spec: Optional[np.ndarray] = None, mask_raw: Optional[np.ndarray] = None,
             prop_before_smoothing: Optional[bool] = None) -> Dict[str, np.ndarray]:
    """One row through the whole denoiser.  Overrides: `spec` (F, T) replaces the STFT of x, `mask_raw` (F, T) the unsmoothed mask;
    `thresh` (F,) dB is the stationary threshold (needed when stationary and no mask_raw is given).  prop_decrease enters before the
    smoothing filter in the stationary mode and behind it otherwise; `prop_before_smoothing` overrides that."""
    x = np.asarray(x, dtype=np.float64)
    win = n_fft if win is None else win
    S = stft_ref(x, n_fft, hop, win) if spec is None else np.asarray(spec, dtype=np.complex128)
    res = {"spec": S}
    if mask_raw is None:
        if stationary:
            res["db"] = amp_db(S)
            mask_raw = (res["db"] > np.asarray(thresh, dtype=np.float64)[:, None]).astype(np.float64)
        else:
            mask_raw = ns_mask(np.abs(S), smoothing_coefficient(time_constant_s, sr, hop), mult, slope)
    mask_raw = np.asarray(mask_raw, dtype=np.float64)
    n_f, n_t = smoothing_counts(sr, n_fft, hop, freq_hz, time_ms)
    if stationary if prop_before_smoothing is None else prop_before_smoothing:
        m = smooth_mask(mask_raw * prop_decrease + (1.0 - prop_decrease), n_f, n_t)
    else:
        m = smooth_mask(mask_raw, n_f, n_t) * prop_decrease + (1.0 - prop_decrease)
    res.update(mask_raw=mask_raw, mask_smooth=m, out=istft_ref(S * m, n_fft, hop, win, length=x.shape[0]))
    return res


def reduce_noise_ref(y, sr: float, n_fft: int = 1024, hop: Optional[int] = None, stationary: bool = False, y_noise=None, chunk_size: int = 600000,
                     padding: int = 30000, n_std: float = 1.5, **kw) -> np.ndarray:
    """(L,) or (C, L) -> the same shape: chunks at multiples of chunk_size (clamped to the clip), each filtered with `padding` samples on
    each side (zeros outside the clip), only the chunk's own samples kept."""
    y = np.asarray(y, dtype=np.float64)
    y2 = y.reshape(1, -1) if y.ndim == 1 else y
    hop = n_fft // 4 if hop is None else hop
    Cn, L = y2.shape
    size = min(chunk_size, L)
    out = np.zeros_like(y2)
    for c in range(Cn):
        thresh = None
        if stationary:
            noise = y2[c] if y_noise is None else np.asarray(y_noise, dtype=np.float64).reshape(-1, np.shape(y_noise)[-1])[c if np.ndim(y_noise) == 2 else 0]
            thresh = stationary_threshold(stft_ref(noise[:chunk_size], n_fft, hop), n_std)
        for s in range(0, L, size):
            row = np.zeros(size + 2 * padding)
            lo, hi = max(s - padding, 0), min(s + size + padding, L)
            row[lo - (s - padding):hi - (s - padding)] = y2[c, lo:hi]
            n = min(size, L - s)
            out[c, s:s + n] = gate_ref(row, sr, n_fft, hop, stationary=stationary, thresh=thresh, **kw)["out"][padding:padding + n]
    return out.reshape(y.shape)


# ---- the shapes and inputs shared by the CPU and the GPU tests ----------------------------------------------------------------------------------
SR = 48000
# (n_fft, hop, L): the smallest shapes at which each mechanism can go wrong
SHAPES = [
    (256, 64, 3000),      # T = 47; 75 time taps > T, 3 bin taps
    (256, 96, 3000),      # hop does not divide the window, overlap 3
    (256, 64, 256),       # L = window, T = 5
    (1024, 256, 10000),   # tail behind the last frame not covered
    (1024, 256, 10240),   # a multiple of hop; 11 x 19 taps
    (2048, 512, 5000),    # T = 10, every frame holds padding
]


def make_rows(L: int, B: int = 5, seed: int = 0) -> np.ndarray:
    """(B, L) float32: decaying tones on noise; with B >= 3 row 1 is all zero and row 2 is row 0's kind scaled by 1e-4."""
    rng = np.random.default_rng(seed + 1000 * L + B)
    n = np.arange(L, dtype=np.float64)
    rows = np.zeros((B, L))
    for r in range(B):
        x = 0.05 * rng.standard_normal(L)
        for _ in range(3):
            f0, start, tau = rng.uniform(200.0, 9000.0), rng.integers(0, max(1, L - L // 4)), rng.uniform(0.02, 0.15) * SR
            env = np.where(n >= start, np.exp(-(n - start) / tau), 0.0)
            x += rng.uniform(0.2, 0.6) * env * np.sin(2.0 * np.pi * f0 * n / SR + rng.uniform(0, 2 * np.pi))
        rows[r] = x
    if B >= 3:
        rows[1] = 0.0
        rows[2] *= 1e-4
    return rows.astype(np.float32)


# ---- the same stages in plain fp32 on the host: the rounding floor the device gates are taken from ------------------------------------------------
def _istft_f32(S, n_fft: int, hop: int, length: int) -> np.ndarray:
    import torch

    f = np.float32
    win, T = n_fft, S.shape[1]
    w = hann(win).astype(f)
    fr = torch.fft.irfft(torch.from_numpy(np.ascontiguousarray(S.T.astype(np.complex64))), n=n_fft, dim=1).numpy()[:, :win] * f(hann(win).sum()) * w
    total = win + (T - 1) * hop
    acc, env = np.zeros(total, dtype=f), np.zeros(total, dtype=f)
    for t in range(T):
        acc[t * hop:t * hop + win] += fr[t]
        env[t * hop:t * hop + win] += w * w
    y = (acc / np.where(env > f(1e-10), env, f(1.0)))[win // 2:total - win // 2]
    out = np.zeros(length, dtype=f)
    out[:min(length, y.shape[0])] = y[:length]
    return out


def gate_f32(x, sr: float, n_fft: int, hop: int, mask_raw: Optional[np.ndarray] = None, stationary: bool = False, prop_decrease: float = 1.0) -> Dict[str, np.ndarray]:
    """gate_ref with every value and every operation in float32 (torch's fp32 FFT): what rounding alone costs at these shapes.  The
    stationary path needs mask_raw (the comparison of dB with the threshold is tested cell by cell, not by a norm)."""
    import torch

    f = np.float32
    x = np.asarray(x, dtype=f)
    win, pad, L = n_fft, n_fft // 2, x.shape[0]
    w, wsum = hann(win).astype(f), f(hann(win).sum())
    xp = np.concatenate([np.zeros(pad, dtype=f), x, np.zeros(pad, dtype=f)])
    T = n_frames(L, win, hop)
    frames = xp[np.arange(T)[:, None] * hop + np.arange(win)[None, :]] * w
    S = np.ascontiguousarray((torch.fft.rfft(torch.from_numpy(frames), n=n_fft, dim=1).numpy() / wsum).T)
    res = {"spec": S, "roundtrip": _istft_f32(S, n_fft, hop, L)}
    if mask_raw is None:
        A, b = np.abs(S).astype(f), f(smoothing_coefficient(2.0, sr, hop))
        c = f(1.0) - b
        fwd, sm = np.empty_like(A), np.empty_like(A)
        prev = A[:, 0].copy()
        for t in range(T):
            prev = b * A[:, t] + c * prev
            fwd[:, t] = prev
        prev = fwd[:, T - 1].copy()
        for t in range(T - 1, -1, -1):
            prev = b * fwd[:, t] + c * prev
            sm[:, t] = prev
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            mask_raw = np.where(sm == 0, f(0), f(1) / (f(1) + np.exp(-(((A - sm) / sm - f(2)) * f(10))))).astype(f)
    mask_raw = np.asarray(mask_raw, dtype=f)
    n_f, n_t = smoothing_counts(sr, n_fft, hop)
    vf, vt = (triangle(n_f) / triangle(n_f).sum()).astype(f), (triangle(n_t) / triangle(n_t).sum()).astype(f)
    p, F = f(prop_decrease), mask_raw.shape[0]
    src = mask_raw * p + (f(1) - p) if stationary else mask_raw
    tmp, m = np.zeros_like(src), np.zeros_like(src)
    for i in range(2 * n_f + 1):
        d = i - n_f
        lo, hi = max(0, d), min(F, F + d)
        if hi > lo:
            tmp[lo:hi] += vf[i] * src[lo - d:hi - d]
    for j in range(2 * n_t + 1):
        d = j - n_t
        lo, hi = max(0, d), min(T, T + d)
        if hi > lo:
            m[:, lo:hi] += vt[j] * tmp[:, lo - d:hi - d]
    if not stationary:
        m = m * p + (f(1) - p)
    res.update(mask_raw=mask_raw, mask_smooth=m, out=_istft_f32(S * m, n_fft, hop, L))
    return res


def errors(got: Dict[str, np.ndarray], ref: Dict[str, np.ndarray], x: np.ndarray, hop: int) -> Dict[str, float]:
    """The figures every gate is stated in: spectra and waveforms as the largest absolute error over the row's largest reference magnitude,
    masks (values in [0, 1]) as the largest absolute error.  `got` holds (F, T) planes and (L,) waveforms like `ref`."""
    n = (ref["spec"].shape[1] - 1) * hop
    xmax = float(np.abs(x).max())
    e = {"spec": float(np.abs(got["spec"] - ref["spec"]).max() / np.abs(ref["spec"]).max()),
         "mask_raw": float(np.abs(got["mask_raw"] - ref["mask_raw"]).max()),
         "mask_smooth": float(np.abs(got["mask_smooth"] - ref["mask_smooth"]).max()),
         "out": float(np.abs(got["out"].astype(np.float64) - ref["out"]).max() / xmax)}
    if "roundtrip" in got:
        e["roundtrip"] = float(np.abs(got["roundtrip"][:n].astype(np.float64) - np.asarray(x, dtype=np.float64)[:n]).max() / xmax)
    return e


def fp32_floors(B: int = 5) -> Dict[str, float]:
    """Largest fp32-restatement error per figure over every shape and every non-zero row of make_rows()."""
    worst: Dict[str, float] = {}
    for n_fft, hop, L in SHAPES:
        rows = make_rows(L, B)
        for r in range(B):
            if not rows[r].any():
                continue
            ref = gate_ref(rows[r], SR, n_fft, hop)
            for k, v in errors(gate_f32(rows[r], SR, n_fft, hop), ref, rows[r], hop).items():
                worst[k] = max(worst.get(k, 0.0), v)
            th = stationary_threshold(ref["spec"])
            raw = (amp_db(ref["spec"]) > th[:, None]).astype(np.float64)
            ref_s = gate_ref(rows[r], SR, n_fft, hop, stationary=True, thresh=th, prop_decrease=0.9, mask_raw=raw)
            for k, v in errors(gate_f32(rows[r], SR, n_fft, hop, mask_raw=raw, stationary=True, prop_decrease=0.9), ref_s, rows[r], hop).items():
                if k in ("mask_smooth", "out"):
                    worst["stationary_" + k] = max(worst.get("stationary_" + k, 0.0), v)
    return worst


if __name__ == "__main__":
    for name, value in sorted(fp32_floors().items()):
        print(f"{name:24s} {value:.3e}")
