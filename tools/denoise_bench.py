"""Seconds per clip of the spectral-gating denoiser on one MI355X against its scipy composition on the host: one mono clip of 30 s at
48 kHz (1 440 000 samples, fp32), n_fft 1024, hop 256, chunk_size 600000, padding 30000 -- three padded chunks, one device batch of three rows.

  (a) device, tensor in / tensor out   syncfusion_amd.reduce_noise on a clip already on the device (chunking, 7 launches, merge)
  (b) device, numpy in / numpy out     the same with the host-to-device and device-to-host copies of the clip
  (c) host, scipy composition          scipy.signal.stft / filtfilt / fftconvolve / istft per padded chunk in fp64 (what noisereduce runs)

Timing: a host clock around calls that end in a device synchronise, `--iters` calls per window for the device legs, one call per window for
the host leg; the device legs alternate window by window; min / median / max over `--windows` windows after `--warmup` calls.  The outputs
of (a) and (c) are compared before anything is timed (largest absolute difference over the clip's largest sample).

    python tools/denoise_bench.py [--seconds 30] [--sr 48000] [--iters 5] [--windows 7] [--host_windows 3] [--warmup 2] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.signal
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import denoise_ref as R  # noqa: E402
from syncfusion_amd import denoise  # noqa: E402


def scipy_reduce_noise(y, sr, n_fft, hop, chunk_size, padding):
    """the non-stationary composition, chunk by chunk, fp64"""
    L = y.shape[0]
    out = np.zeros(L)
    t = 2.0 * sr / hop
    b = (np.sqrt(1 + 4 * t ** 2) - 1) / (2 * t ** 2)
    n_f, n_t = R.smoothing_counts(sr, n_fft, hop)
    v = np.outer(R.triangle(n_f), R.triangle(n_t))
    v /= v.sum()
    for ch in denoise.chunk_rows(L, min(chunk_size, L), padding):
        row = np.zeros(ch.length)
        lo, hi = max(ch.start, 0), min(ch.start + ch.length, L)
        row[lo - ch.start:hi - ch.start] = y[lo:hi]
        _, _, S = scipy.signal.stft(row, nfft=n_fft, nperseg=n_fft, noverlap=n_fft - hop, padded=False)
        A = np.abs(S)
        sm = scipy.signal.filtfilt([b], [1, b - 1], A, axis=-1, padtype=None)
        with np.errstate(divide="ignore", invalid="ignore"):
            mask = np.nan_to_num(1 / (1 + np.exp(-(((A - sm) / sm - 2) * 10))))
        mask = scipy.signal.fftconvolve(mask, v, mode="same")
        _, z = scipy.signal.istft(S * mask, nfft=n_fft, nperseg=n_fft, noverlap=n_fft - hop)
        kept = z[ch.keep:ch.keep + ch.count]
        out[ch.dest:ch.dest + kept.shape[0]] = kept
    return out


def window_s(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--sr", type=int, default=48000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--host_windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("denoise_bench: no GPU visible (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    sr, L = a.sr, int(a.seconds * a.sr)
    n_fft, hop, chunk, pad = 1024, 256, 600000, 30000
    y = np.tile(R.make_rows(sr, 1)[0], -(-L // sr))[:L].copy()       # one second of decaying tones on noise, repeated
    y_dev = torch.from_numpy(y).to(dev)
    legs = [("a device, tensor in / tensor out", lambda: denoise.reduce_noise(y_dev, sr, n_fft=n_fft, hop_length=hop, chunk_size=chunk, padding=pad)),
            ("b device, numpy in / numpy out", lambda: denoise.reduce_noise(y, sr, n_fft=n_fft, hop_length=hop, chunk_size=chunk, padding=pad))]
    got = legs[0][1]().cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    ref = scipy_reduce_noise(y.astype(np.float64), sr, n_fft, hop, chunk, pad)
    host = [time.perf_counter() - t0]
    n = min(got.shape[0], ref.shape[0])
    err = float(np.abs(got[:n] - ref[:n]).max() / np.abs(y).max())
    for _, fn in legs:
        for _ in range(a.warmup):
            fn()
    ms = {name: [] for name, _ in legs}
    for _ in range(a.windows):
        for name, fn in legs:
            ms[name].append(window_s(fn, a.iters))
    for _ in range(a.host_windows - 1):
        t0 = time.perf_counter()
        scipy_reduce_noise(y.astype(np.float64), sr, n_fft, hop, chunk, pad)
        host.append(time.perf_counter() - t0)
    ms["c host, scipy composition (fp64)"] = host
    rows = len(denoise.chunk_rows(L, min(chunk, L), pad))
    lines = [f"# tools/denoise_bench.py on one MI355X: one mono clip of {L} fp32 samples ({a.seconds:g} s at {sr} Hz), n_fft {n_fft}, hop {hop}, "
             f"chunk_size {chunk}, padding {pad} ({rows} rows in one batch); {a.windows} alternating windows of {a.iters} calls per device leg after "
             f"{a.warmup} warm-up calls, {a.host_windows} single calls of the host leg; seconds per clip min / median / max; x real time on the median",
             f"# device output against the scipy composition: largest difference {err:.3e} of the clip's largest sample"]
    out = {"samples": L, "sr": sr, "max_err": err, "legs": {}}
    for name, v in ms.items():
        lo, med, hi = min(v), statistics.median(v), max(v)
        out["legs"][name] = {"s_min": round(lo, 6), "s_median": round(med, 6), "s_max": round(hi, 6), "x_real_time": round(a.seconds / med, 1)}
        lines.append(f"{name:36s}: {lo:10.6f} / {med:10.6f} / {hi:10.6f} s   {a.seconds / med:10.1f} x real time")
        print(lines[-1], flush=True)
    lines.append(json.dumps(out))
    print(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
