#!/usr/bin/env python3
"""Solver error and step time of the multistep v-sampler on the full random-initialised model (one MI355X).

Error: rel-L2 of sample(solver, T steps) against sample("ddim", --ref-steps steps) on the same noise and conditioning, for every solver at
every T of --steps; batch 8 at bench.py's headline length, fp32x.  The weights are random, so this says how fast each rule approaches the
ODE solution of THIS network, not how a trained checkpoint sounds.

Time: ms per step of sample(solver="ab2") beside sample() (the first-order loop, sf_vsample) in alternating windows of one process, graph
replay.  The multistep update moves one more read and one more write of B * L0 floats per step; the condition is that ab2's median lies
within the spread (min .. max) of the ddim windows of the same run.

    python tools/solver_bench.py [--steps 25,50,100,150] [--ref-steps 600] [--iters 50] [--rounds 7] [--out profiles/solver_bench.txt]
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
    ap.add_argument("--steps", default="25,50,100,150")
    ap.add_argument("--ref-steps", type=int, default=600)
    ap.add_argument("--iters", type=int, default=50, help="steps per timed call")
    ap.add_argument("--rounds", type=int, default=7, help="alternating windows per leg")
    ap.add_argument("--dtype", default="fp32x")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import bench

    if not torch.cuda.is_available():
        print("solver_bench.py needs the GPU: nothing measured", file=sys.stderr)
        return 1
    device = torch.device("cuda:0")
    model = bench.build_model(args.dtype, device)
    B, L = args.batch, bench.L0
    chans, emb = bench.synthetic_conditioning(model, B, L, device, real=True)
    noise = torch.randn(B, 1, L, generator=torch.Generator().manual_seed(1)).to(device)
    kw = dict(x_noisy=noise, channels=chans, embedding=emb, embedding_scale=1.0)
    legs = ["ddim", "ab2"]
    lines = [f"# tools/solver_bench.py --steps {args.steps} --ref-steps {args.ref_steps} --iters {args.iters} --rounds {args.rounds} --dtype {args.dtype} "
             f"--batch {args.batch}",
             f"# full model, random weights, batch {B} x {L}, no guidance, {args.dtype}"]

    def rel_l2(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm())

    with torch.no_grad():
        ref = model.model.sample(num_steps=args.ref_steps, **kw)
        lines.append(f"rel-L2 against {args.ref_steps} first-order steps")
        lines.append(f"  {'steps':>6} " + " ".join(f"{s:>12}" for s in ("ddim", "ab2", "dpmpp_2m")))
        for T in (int(t) for t in args.steps.split(",")):
            errs = [rel_l2(model.model.sample(num_steps=T, solver=s, **kw), ref) for s in ("ddim", "ab2", "dpmpp_2m")]
            lines.append(f"  {T:>6} " + " ".join(f"{e:>12.4e}" for e in errs))
        N = args.iters
        calls = {s: (lambda s=s: model.model.sample(num_steps=N, solver=s, **kw)) for s in legs}
        for _ in range(2):                          # capture + one replay of every leg before anything is timed
            for f in calls.values():
                f()
        ms = {s: [] for s in legs}
        for _ in range(args.rounds):
            for s, f in calls.items():
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize(device)
                ms[s].append((time.perf_counter() - t0) * 1e3 / N)
    lines.append(f"ms per step, {N}-step calls, {args.rounds} alternating windows per leg (median; min .. max), graph replay")
    for s, v in ms.items():
        lines.append(f"  {s:<8} {statistics.median(v):8.4f} ms  ({min(v):.4f} .. {max(v):.4f})")
    med, lo, hi = statistics.median(ms["ab2"]), min(ms["ddim"]), max(ms["ddim"])
    base = statistics.median(ms["ddim"])
    lines.append(f"  ab2 median {100.0 * (med / base - 1.0):+.2f} % vs ddim median; inside the ddim windows' spread [{lo:.4f}, {hi:.4f}]: "
                 f"{'yes' if lo <= med <= hi else 'NO'}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
