"""Milliseconds per batch of the audio front end on one MI355X: 256 clips x 44100 samples (2 s at 22050 Hz, fp32, already on the device) through
  (a) log-mel, SampleLogger's configuration    n_fft 1024, hop 512, 80 mels, reflect, dB            (sf_logmel_forward, 2 launches)
  (b) log-mel, the detector's configuration    n_fft 2048, hop 512, 128 mels, zero padding, dB      (sf_logmel_forward, 2 launches)
  (c) onset_detect, delta 0.3                  (b)'s mel power -> envelope -> peaks, confidences    (sf_onset_detect, 3 launches)
Nothing else runs beside them; the legs alternate window by window, so a drift of the clock falls on all of them.

Timing: device events on the launch stream around `--iters` calls per window, `--windows` windows per leg after `--warmup` calls; min / median /
max over the windows.  GB/s is on the ALGORITHMIC bytes: the waveform read once plus every output written once (the mel-power scratch of
(c) and the overlap of the frames -- each sample lies in n_fft / hop of them -- are implementation traffic and are not counted).  The shader
clock is read by the library's clock probe (one wave on a side stream) during one extra window per leg, outside the timed ones.

    python tools/audio_features_bench.py [--clips 256] [--samples 44100] [--iters 50] [--windows 7] [--warmup 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import audio_features_ref as R  # noqa: E402
from syncfusion_amd import _lib  # noqa: E402
from syncfusion_amd.audio_features import front_end, peak_pick_defaults  # noqa: E402


def window_ms(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--samples", type=int, default=44100)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("audio_features_bench: no GPU visible (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    B, L, sr = a.clips, a.samples, 22050
    wav = torch.from_numpy(R.make_input("bursts", 8, L)).repeat((B + 7) // 8, 1)[:B].contiguous().to(dev)
    logger = front_end(dev, sr, 1024, 512, 80, mel_scale="htk", norm="slaney", pad_mode="reflect")
    det = front_end(dev, sr, 2048, 512, 128)
    win = peak_pick_defaults(sr, 512)
    T = 1 + L // 512
    legs = [
        ("a log-mel 1024/512/80 reflect, dB", lambda: logger.logmel(wav, to_db=True), 4.0 * B * (L + 80 * T)),
        ("b log-mel 2048/512/128 constant, dB", lambda: det.logmel(wav, to_db=True), 4.0 * B * (L + 128 * T)),
        ("c onset_detect delta 0.3", lambda: det.detect(wav, 0.3, **win), 4.0 * B * (2 * L + T + 1 + 3 * T)),   # the waveform is read twice: frames, confidences
    ]
    for _, fn, _ in legs:
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in legs}
    for _ in range(a.windows):
        for name, fn, _ in legs:
            ms[name].append(window_ms(fn, a.iters))
    lib = _lib.load()
    side = torch.cuda.Stream(dev)
    lines = [f"# tools/audio_features_bench.py on one MI355X: {B} clips x {L} fp32 samples; {a.windows} alternating windows of {a.iters} calls per leg "
             f"after {a.warmup} warm-up calls; ms per batch min / median / max; GB/s on the algorithmic bytes; shader clock from the clock probe "
             f"during one extra window"]
    out = {"shape": [B, L], "legs": {}}
    for name, fn, nbytes in legs:
        lo, med, hi = min(ms[name]), statistics.median(ms[name]), max(ms[name])
        _lib.check(lib.sf_clock_probe_start(0.8 * 1e3 * med * a.iters, int(side.cuda_stream)), "sf_clock_probe_start")
        window_ms(fn, a.iters)
        mhz = ctypes.c_double()
        _lib.check(lib.sf_clock_probe_read(ctypes.byref(mhz)), "sf_clock_probe_read")
        gbs = nbytes / med / 1e6
        out["legs"][name] = {"ms_min": round(lo, 4), "ms_median": round(med, 4), "ms_max": round(hi, 4), "algorithmic_mb": round(nbytes / 1e6, 2),
                             "gb_per_s": round(gbs, 1), "clips_per_s": round(B / med * 1e3, 1), "shader_mhz": round(mhz.value, 1)}
        lines.append(f"{name:38s}: {lo:8.4f} / {med:8.4f} / {hi:8.4f} ms   {nbytes / 1e6:7.2f} MB  {gbs:7.1f} GB/s  {B / med * 1e3:10.0f} clips/s   "
                     f"shader clock {mhz.value:6.0f} MHz")
        print(lines[-1], flush=True)
    lines.append(json.dumps(out))
    print(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
