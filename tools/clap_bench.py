"""Milliseconds per ``get_audio_embedding_from_data`` call of ``ClapAudioEmbedder`` (HIP) on 2^18-sample clips at the training batch (4) and
the evaluation batch (10), eager and replayed from a captured graph, and, in the same run and in alternation, the same network composed
from torch operations in fp32 on the same device (tests/clap_ref.py with ``dtype=torch.float32``: torch.stft, F.interpolate, F.layer_norm,
F.linear, torch.roll + window partition: rocFFT / rocBLAS / ATen), fed the same clips and weights.

Device events around `--steps` calls after `--warmup` calls, `--rounds` alternating rounds (A B C A B C ...), the median per leg.  No speed
is gated anywhere: this is where the number gets written down (profiles/clap_bench.txt).

    python tools/clap_bench.py [--batches 4 10] [--steps 10] [--warmup 3] [--rounds 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import clap_ref  # noqa: E402
from syncfusion_amd.clap import ClapAudioConfig, ClapAudioEmbedder  # noqa: E402

TRAIN_STEP_MS = 41.5          # the batch-4 training step of profiles/HISTORY.md (41-42 ms), for the share of the step


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


def engine_launches(cfg: ClapAudioConfig) -> int:
    """Kernel launches of sf_clap_audio_forward: patch embed, 7 per block (LayerNorm, qkv, attention, proj, LayerNorm, fc1, fc2), 2 per
    PatchMerging (gather + LayerNorm, reduction), 4 for the tail (pool, two Linears, normalisation)."""
    return 1 + 7 * sum(cfg.depths) + 2 * (len(cfg.depths) - 1) + 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 10])
    ap.add_argument("--samples", type=int, default=1 << 18)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = ClapAudioConfig()
    sd = clap_ref.seeded_weights(cfg, 1)
    model = ClapAudioEmbedder(cfg)
    model.load_state_dict(sd)
    model = model.to(dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    out = {"samples_per_clip": a.samples, "engine_launches_per_call": engine_launches(cfg), "image_launches": 1,
           "params_M": round(sum(p.numel() for p in model.parameters()) / 1e6, 2)}
    print(f"engine launches per call: {out['engine_launches_per_call']} (+ 1 image launch, the mel front end and the repeat-pad copies)", flush=True)
    with torch.no_grad():
        for B in a.batches:
            wav = clap_ref.chirp(cfg, a.samples, B, 3).to(dev)
            static = wav.clone()
            torch_modules = lambda: clap_ref.embed(wav, sd_dev, cfg, dtype=torch.float32)      # noqa: E731
            eager = lambda: model.get_audio_embedding_from_data(static)                        # noqa: E731
            err = float((eager() - torch_modules()).norm() / torch_modules().norm())
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                eager()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                captured = eager()
            graph.replay()
            assert torch.equal(captured, eager())
            legs = {"hip_eager": eager, "hip_graph_replay": graph.replay, "torch_modules_fp32": torch_modules}
            runs = {k: [] for k in legs}
            for _ in range(max(1, a.rounds)):
                for name, step in legs.items():
                    runs[name].append(time_loop(step, a.steps, a.warmup))
            res = {"rel_l2_hip_vs_torch_modules": err}
            for name, ms_all in runs.items():
                med = sorted(ms_all)[len(ms_all) // 2]
                res[name] = {"ms": round(med, 3), "share_of_train_step": round(med / TRAIN_STEP_MS, 4), "rounds_ms": [round(v, 3) for v in ms_all]}
                print(f"B {B:2d} {name:20s}: {med:8.3f} ms  {100 * med / TRAIN_STEP_MS:5.1f} % of a {TRAIN_STEP_MS} ms training step  "
                      f"(rounds {', '.join(f'{v:.3f}' for v in ms_all)})", flush=True)
            out[f"B{B}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
