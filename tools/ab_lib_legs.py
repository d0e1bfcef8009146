#!/usr/bin/env python3
"""The denoise-loop legs of an A/B of library builds, for the library SF_LIB_PATH names, each timed several times in ONE process:
    SF_LIB_PATH=<lib> python tools/ab_lib_legs.py <tag> [reps] [legs: cfg1,cfg2,cfg3,x3]
cfg1 = configs[1] (batch 8, bf16), cfg2 = configs[2] (batch 32, guidance 2.0), cfg3 = one GPU's share of configs[3] (batch 32, no guidance),
x3 = configs[1] with the fp32x engine.  One line per leg: min / median / max steps/s of `reps` timed sample() calls of 50 steps and every
sample (the method of tools/ab_tree_legs.py, which alternates source trees; this one alternates libraries of one tree)."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402

tag = sys.argv[1]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
legs = (sys.argv[3] if len(sys.argv) > 3 else "cfg1,cfg2,cfg3,x3").split(",")
dev = torch.device("cuda", 0)
SHAPES = {"cfg1": ("bf16", 8, 1.0), "cfg2": ("bf16", 32, 2.0), "cfg3": ("bf16", 32, 1.0), "x3": ("fp32x", 8, 1.0)}
models = {}
with torch.no_grad():
    for leg in legs:
        dtype, B, scale = SHAPES[leg]
        if dtype not in models:
            models[dtype] = bench.build_model(dtype, dev)
        model = models[dtype]
        nz = torch.randn(B, 1, bench.L0, generator=torch.Generator().manual_seed(1000)).to(dev)
        ch, e = bench.synthetic_conditioning(model, B, bench.L0, dev, real=True)
        run = lambda n: model.model.sample(x_noisy=nz, num_steps=n, channels=ch, embedding=e, embedding_scale=scale)  # noqa: E731
        run(2)
        run(2)
        rates = []
        for _ in range(reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            run(50)
            torch.cuda.synchronize(dev)
            rates.append(50 / (time.perf_counter() - t0))
        print(f"{tag:7s} {leg:5s} {dtype:5s} min {min(rates):8.3f}  median {statistics.median(rates):8.3f}  max {max(rates):8.3f} steps/s   samples "
              + " ".join(f"{r:.2f}" for r in rates), flush=True)
