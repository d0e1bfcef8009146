"""Examples per second of ``VGGish.forward`` (front end + network, HIP) at 256 examples of the full-size configuration and, in the same run
and in alternation, the same layers as torch modules on the same device (nn.Conv2d / nn.MaxPool2d / nn.Linear: MIOpen and rocBLAS),
fed the same examples.

Device events around `--steps` calls after `--warmup` calls, `--rounds` alternating rounds (A B A B ...), the median per leg.  No throughput
is gated anywhere: this is where the number gets written down (profiles/fad_bench.txt).

    python tools/fad_bench.py [--examples 256] [--steps 3] [--warmup 1] [--rounds 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from syncfusion_amd.fad import VGGish, VGGishConfig  # noqa: E402


def time_loop(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--examples", type=int, default=256)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = VGGishConfig()
    model = VGGish(cfg).to(dev).eval()            # nn defaults: the timing does not depend on the values
    per = cfg.window_length + (cfg.example_frames - 1) * cfg.hop_length
    L = per + (8 - 1) * cfg.example_frames * cfg.hop_length          # 8 examples per clip
    B = max(1, a.examples // 8)
    n = B * cfg.examples(L)
    wav = (0.1 * torch.randn(B, L, device=dev)).clamp(-1, 1)

    def torch_modules(x):                          # (N, 1, 96, 64) -> (N, D), torchvggish's forward without the post-processor
        h = model.features(x)
        return model.embeddings(h.permute(0, 2, 3, 1).reshape(h.shape[0], -1))

    with torch.no_grad():
        ex = model.examples(wav).reshape(n, 1, cfg.example_frames, cfg.n_mels).contiguous()
        rows = model.example_rows(wav)
        err = float((model.embed_rows(rows) - torch_modules(ex)).norm() / torch_modules(ex).norm())
        legs = {"hip_forward": lambda: model(wav), "hip_network_only": lambda: model.embed_rows(rows), "torch_modules_network_only": lambda: torch_modules(ex)}
        runs = {k: [] for k in legs}
        for _ in range(max(1, a.rounds)):
            for name, step in legs.items():
                runs[name].append(time_loop(step, a.steps, a.warmup))
    out = {"examples": n, "clips": B, "samples_per_clip": L, "rel_l2_hip_vs_torch_modules": err}
    for name, ms_all in runs.items():
        med = sorted(ms_all)[len(ms_all) // 2]
        out[name] = {"ms": round(med, 2), "examples_per_s": round(n / med * 1e3, 1), "rounds_ms": [round(v, 2) for v in ms_all]}
        print(f"{name:28s}: {med:9.2f} ms  {n / med * 1e3:9.1f} examples/s  (rounds {', '.join(f'{v:.2f}' for v in ms_all)})", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
