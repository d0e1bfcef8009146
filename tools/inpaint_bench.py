#!/usr/bin/env python3
"""ms per iteration of DiffusionModel.inpaint() beside ms per step of DiffusionModel.sample(), graph replay, alternating within one process.

Shapes: bench.py's headline (batch 8, 2 s @ 22.05 kHz -> L0 = 45056, bf16, no guidance) and the reference's evaluation shape (batch 10,
length 2**18, embedding_scale 2.0, bf16).  sample() is the yardstick: an inpaint() iteration is a sample() step whose update launch also
reads the source and the mask and, where the mask keeps the source, draws the noise.  Each round times sample(N), inpaint(N steps, R = 1)
and inpaint(N / R steps, R resamples) -- N iterations each -- in that order; the medians over the rounds are reported.

    python tools/inpaint_bench.py [--iters 20] [--rounds 5] [--resamples 4] [--keep 0.5] [--out profiles/inpaint_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="U-Net evaluations per timed call")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--resamples", type=int, default=4, help="the larger R (must divide --iters)")
    ap.add_argument("--keep", type=float, default=0.5, help="fraction of every clip (its head) the mask keeps")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.iters % args.resamples:
        ap.error("--resamples must divide --iters")
    import torch

    import bench

    device = torch.device("cuda:0")
    model = bench.build_model(args.dtype, device)
    lines = [f"# tools/inpaint_bench.py --iters {args.iters} --rounds {args.rounds} --resamples {args.resamples} --keep {args.keep} --dtype {args.dtype}",
             "# ms per U-Net evaluation (median of the rounds; min .. max), graph replay, one process, calls alternating sample / inpaint R=1 / inpaint R"]
    for name, B, L, scale in (("bench.py headline: batch 8 x 45056, no guidance", 8, 45056, 1.0),
                              ("reference evaluation shape: batch 10 x 2**18, embedding_scale 2.0", 10, 2 ** 18, 2.0)):
        chans, emb = bench.synthetic_conditioning(model, B, L, device, real=True)
        g = torch.Generator().manual_seed(1)
        noise = torch.randn(B, 1, L, generator=g).to(device)
        source = (torch.randn(B, 1, L, generator=g) * 0.3).to(device)
        mask = torch.zeros(B, 1, L, dtype=torch.bool, device=device)
        mask[:, :, : int(L * args.keep)] = True
        kw = dict(channels=chans, embedding=emb, embedding_scale=scale)
        N, R = args.iters, args.resamples
        legs = {
            "sample()": lambda: model.model.sample(x_noisy=noise, num_steps=N, **kw),
            "inpaint(R=1)": lambda: model.model.inpaint(source, mask, N, 1, x_noisy=noise, seed=7, **kw),
            f"inpaint(R={R})": lambda: model.model.inpaint(source, mask, N // R, R, x_noisy=noise, seed=7, **kw),
        }
        with torch.no_grad():
            for _ in range(2):                      # capture + one replay of every leg before anything is timed
                for f in legs.values():
                    f()
            ms = {k: [] for k in legs}
            for _ in range(args.rounds):
                for k, f in legs.items():
                    torch.cuda.synchronize(device)
                    t0 = time.perf_counter()
                    f()
                    torch.cuda.synchronize(device)
                    ms[k].append((time.perf_counter() - t0) * 1e3 / N)
        base = statistics.median(ms["sample()"])
        lines.append(f"{name} ({args.dtype}, mask keeps {args.keep:.0%})")
        for k, v in ms.items():
            med = statistics.median(v)
            lines.append(f"  {k:<14} {med:8.3f} ms  ({min(v):.3f} .. {max(v):.3f})  {100.0 * (med / base - 1.0):+6.2f} % vs sample()")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
