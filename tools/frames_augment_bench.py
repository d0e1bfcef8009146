"""Milliseconds per batch of the onset data's frame transforms on one MI355X: 16 clips x 30 decoded frames of 240 x 320 (uint8, already on the
device) through
  (a) frames_to_clip                      the evaluation chain, Resize((112, 112)) -> Normalize            (sf_frames_preprocess)
  (b) Resize(128) -> RandomCrop(112) -> Normalize                                                          (sf_frames_augment, one pass)
  (c) (b) + ColorJitter(0.4, 0.2, 0.4, 0.1)     the reference's training chain: contrast => two passes    (sf_frames_augment)
  (d) (c) with contrast = 0                     one pass                                                   (sf_frames_augment)
and, beside them, the restated oracle (tests/frames_augment_ref.py, fp32 torch CPU ops) on `--host-threads` host threads in clips/s -- a
PORT of the transform to torch ops, not the reference's DataLoader (torchvision on 8 worker processes), which this image cannot run.

Timing: device events on the launch stream around `--iters` calls per window, `--windows` windows after `--warmup` calls; min / median / max
over the windows.  GB/s is on the ALGORITHMIC bytes: the source pixels under the filter footprint of the surviving crop plus the fp32 output
(the fp32 intermediate the two-pass form rereads is implementation traffic and is not counted).  The parameter table is drawn once, outside
the timed region; its upload (48 bytes per clip) and the host-side validation are inside, as in use.

    python tools/frames_augment_bench.py [--clips 16] [--frames 30] [--iters 200] [--windows 7] [--warmup 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import frames_augment_ref as R  # noqa: E402
from syncfusion_amd import frame_transforms as ft  # noqa: E402
from syncfusion_amd.input_pipeline import frames_to_clip  # noqa: E402

NORM = dict(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])


def footprint(in_size: int, resized: int, start: int, count: int) -> int:
    """source rows (columns) the antialiased filter reads for resized indices start .. start + count - 1"""
    scale = in_size / resized
    support = max(scale, 1.0)
    lo = max(int(scale * (start + 0.5) - support + 0.5), 0)
    hi = min(int(scale * (start + count - 0.5) + support + 0.5), in_size)
    return hi - lo


def algorithmic_bytes(T, H, W, params) -> float:
    rh, rw = params.resized_hw
    oh, ow = params.out_hw
    src = sum(footprint(H, rh, int(t), oh) * footprint(W, rw, int(l), ow) * 3 for t, l in zip(params.top.tolist(), params.left.tolist()))
    return float(T) * src + float(len(params)) * T * 3 * oh * ow * 4


def time_windows(fn, iters, windows, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1) / iters)
    return min(ms), statistics.median(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--train-step-ms", type=float, default=284.76, help="profiles/onset_train_step_bench.txt, HIP path")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frames_augment_bench: no GPU visible (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    N, T, H, W = a.clips, a.frames, a.height, a.width
    u8 = R.make_frames(N, T, H, W, seed=0)
    x = u8.to(dev)
    g = torch.Generator().manual_seed(0)
    chains = {
        "b resize+crop": ft.Compose([ft.Resize(128, antialias=True), ft.RandomCrop(112), ft.Normalize(**NORM)]),
        "c full chain (contrast: 2 passes)": ft.Compose([ft.Resize(128, antialias=True), ft.RandomCrop(112), ft.ColorJitter(0.4, 0.2, 0.4, 0.1),
                                                         ft.Normalize(**NORM)]),
        "d full chain, contrast=0 (1 pass)": ft.Compose([ft.Resize(128, antialias=True), ft.RandomCrop(112), ft.ColorJitter(0.4, 0, 0.4, 0.1),
                                                         ft.Normalize(**NORM)]),
    }
    lines = [f"# tools/frames_augment_bench.py on one MI355X: {N} clips x {T} frames of {H} x {W} uint8 -> ({N}, 3, {T}, 112, 112) fp32; "
             f"{a.windows} windows of {a.iters} calls after {a.warmup} warm-up calls; ms per batch min / median / max; GB/s on the algorithmic bytes"]
    out = {"shape": [N, T, H, W], "legs": {}}
    eval_params = ft.default_chain().sample(N, (H, W))
    legs = [("a frames_to_clip (evaluation chain)", lambda: frames_to_clip(x), algorithmic_bytes(T, H, W, eval_params))]
    for name, chain in chains.items():
        params = chain.sample(N, (H, W), g)
        legs.append((name, (lambda c=chain, p=params: c(x, params=p)), algorithmic_bytes(T, H, W, params)))
    for name, fn, nbytes in legs:
        lo, med, hi = time_windows(fn, a.iters, a.windows, a.warmup)
        gbs = nbytes / med / 1e6
        out["legs"][name] = {"ms_min": round(lo, 4), "ms_median": round(med, 4), "ms_max": round(hi, 4), "algorithmic_mb": round(nbytes / 1e6, 2),
                             "gb_per_s": round(gbs, 1), "share_of_train_step": round(med / a.train_step_ms, 5)}
        lines.append(f"{name:36s}: {lo:8.4f} / {med:8.4f} / {hi:8.4f} ms   {nbytes / 1e6:7.2f} MB  {gbs:7.1f} GB/s   "
                     f"{100.0 * med / a.train_step_ms:5.2f} % of the {a.train_step_ms:.0f} ms training step")
        print(lines[-1], flush=True)
    # the oracle restatement on the host (a port to torch ops, fp32)
    torch.set_num_threads(a.host_threads)
    chain = chains["c full chain (contrast: 2 passes)"]
    params = chain.sample(N, (H, W), torch.Generator().manual_seed(1))
    R.transform_batch(u8[:2], params.select([0, 1]), dtype=torch.float32)
    best = float("inf")
    for _ in range(a.host_repeats):
        t0 = time.perf_counter()
        R.transform_batch(u8, params, dtype=torch.float32)
        best = min(best, time.perf_counter() - t0)
    out["host_port"] = {"threads": a.host_threads, "s_per_batch": round(best, 4), "clips_per_s": round(N / best, 2)}
    lines.append(f"host port of the full chain (torch CPU ops, fp32, {a.host_threads} threads; NOT the reference's DataLoader): "
                 f"{best * 1e3:8.1f} ms per batch, {N / best:7.2f} clips/s")
    print(lines[-1], flush=True)
    lines.append(json.dumps(out))
    print(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
