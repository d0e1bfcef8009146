#!/usr/bin/env python3
"""Time the optimizer stage alone on the reference model's full parameter set (215 M fp32 parameters, ~900 tensors): gradient clipping at
0.5 by global norm + AdamW, as `torch.nn.utils.clip_grad_norm_` + `torch.optim.AdamW(fused=True)` (what the trainer ran so far) and as
`syncfusion_amd.optim.AdamW(max_grad_norm=0.5)` (one `sf_optim_adamw_step`), eager and -- for the HIP class -- replayed from a graph.

    python tools/optim_bench.py [--rounds 3] [--steps 20] [--warmup 3]
The legs alternate (torch, hip, hip-graph, torch, ...); prints one JSON line with min / median / max ms per step over the rounds and GB/s
counted as (7 * 4 + 4) bytes per parameter: read p, g, m, v and write p, m, v for the update, read g once more for the norm.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLIP = 0.5


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    import syncfusion_amd as sa
    from syncfusion_amd.optim import AdamW
    from syncfusion_amd.reference_config import model_config

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = sa.instantiate(model_config())
    shapes = [tuple(p.shape) for p in list(model.model.parameters()) + list(model.onsets_encoder.parameters())]
    hyper = dict(lr=model.lr, betas=(model.lr_beta1, model.lr_beta2), eps=model.lr_eps, weight_decay=model.lr_weight_decay)
    del model
    n_params = sum(int(torch.Size(s).numel()) for s in shapes)

    def params():
        ps = [torch.nn.Parameter(torch.randn(s, device=dev) * 0.02) for s in shapes]
        for p in ps:
            p.grad = torch.randn_like(p) * 1e-3
        return ps

    pt, ph, pg = params(), params(), params()
    ot = torch.optim.AdamW(pt, fused=True, **hyper)
    oh = AdamW(ph, max_grad_norm=CLIP, **hyper)
    og = AdamW(pg, max_grad_norm=CLIP, **hyper)

    def torch_stage():
        torch.nn.utils.clip_grad_norm_(pt, CLIP)
        ot.step()

    og.step()                      # moments, table and workspace exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og.step()
    og.sync_device_state()

    legs = {"torch_clip_fused_adamw": torch_stage, "hip": oh.step, "hip_graph_replay": graph.replay}
    times = {k: [] for k in legs}
    for fn in legs.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    nbytes = (7 * 4 + 4) * n_params
    out = {"workload": f"optimizer stage: clip {CLIP} + AdamW, {n_params} fp32 parameters in {len(shapes)} tensors", "steps_per_round": args.steps}
    for name, ts in times.items():
        med = statistics.median(ts)
        out[name] = {"ms_min": min(ts), "ms_median": med, "ms_max": max(ts), "gb_per_s_at_median": nbytes / med / 1e6}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
