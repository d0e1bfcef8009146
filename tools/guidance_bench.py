#!/usr/bin/env python3
"""Step time of the v-sampler under guidance schedules on the full random-initialised model (one MI355X).

Four runs of one shape in alternating windows of one process, graph replay, solver "ab2" on explicit LinearSchedule(1, 0) sigmas (every
run goes through sf_vsample_ms / sf_vsample_gx, so they differ in guidance only):

    full      a float scale at every step                       (2 B rows per step)
    interval  the same scale inside --interval, 1 outside       (2 B rows inside, B outside; one sf_vsample_gx per segment)
    unguided  scale 1                                           (B rows per step)
    rescale   the float scale with guidance_rescale = --phi     (full + one statistics launch per step)

Reported: median and spread (min .. max) of the ms per call; the interval run against  n_two * t_full + n_single * t_unguided  taken from
the same windows' per-step times; the rescale run against the full run.  The weights are random: this measures time, not audio quality.

    python tools/guidance_bench.py [--shapes 8x45056,10x262144] [--dtypes bf16,fp32x] [--steps 50] [--rounds 5] [--out profiles/guidance_bench.txt]
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
    ap.add_argument("--shapes", default="8x45056,10x262144", help="BxL: the headline shape and the reference's evaluation shape")
    ap.add_argument("--dtypes", default="bf16,fp32x")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--scale", type=float, default=2.0)
    ap.add_argument("--interval", default="0.3,0.8")
    ap.add_argument("--phi", type=float, default=0.7)
    ap.add_argument("--rounds", type=int, default=5, help="alternating windows per run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import bench
    from syncfusion_amd.guidance import evaluation_rows, plan_segments, scale_table

    if not torch.cuda.is_available():
        print("guidance_bench.py needs the GPU: nothing measured", file=sys.stderr)
        return 1
    device = torch.device("cuda:0")
    T = args.steps
    interval = tuple(float(v) for v in args.interval.split(","))
    sig = np.linspace(1.0, 0.0, T + 1, dtype=np.float32)
    lines = [f"# tools/guidance_bench.py --shapes {args.shapes} --dtypes {args.dtypes} --steps {T} --scale {args.scale} --interval {args.interval} "
             f"--phi {args.phi} --rounds {args.rounds}",
             "# full model, random weights, real conditioning, solver ab2 on explicit sigmas, graph replay; ms per call: median (min .. max)"]

    def flush():
        text = "\n".join(lines) + "\n"
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text)
        return text

    for dtype in args.dtypes.split(","):
        model = bench.build_model(dtype, device)
        for shape in args.shapes.split(","):
            B, L = (int(v) for v in shape.split("x"))
            chans, emb = bench.synthetic_conditioning(model, B, L, device, real=True)
            noise = torch.randn(B, 1, L, generator=torch.Generator().manual_seed(1)).to(device)
            kw = dict(x_noisy=noise, num_steps=T, channels=chans, embedding=emb, solver="ab2", sigmas=sig)
            plan = plan_segments(scale_table(args.scale, sig, B, interval))
            n_two = sum(i1 - i0 for i0, i1, two in plan if two)
            runs = {
                "full": lambda: model.model.sample(embedding_scale=args.scale, **kw),
                "interval": lambda: model.model.sample(embedding_scale=args.scale, guidance_interval=interval, **kw),
                "unguided": lambda: model.model.sample(embedding_scale=1.0, **kw),
                "rescale": lambda: model.model.sample(embedding_scale=args.scale, guidance_rescale=args.phi, **kw),
            }
            ms = {k: [] for k in runs}
            with torch.no_grad():
                for _ in range(2):                      # capture + one replay of every run before anything is timed
                    for f in runs.values():
                        f()
                for _ in range(args.rounds):
                    for k, f in runs.items():
                        torch.cuda.synchronize(device)
                        t0 = time.perf_counter()
                        f()
                        torch.cuda.synchronize(device)
                        ms[k].append((time.perf_counter() - t0) * 1e3)
            med = {k: statistics.median(v) for k, v in ms.items()}
            lines.append(f"{dtype}, batch {B} x {L}, {T} steps, scale {args.scale}: plan {plan} ({n_two} guided steps, "
                         f"{evaluation_rows(plan, B)} of {2 * T * B} rows)")
            for k, v in ms.items():
                lines.append(f"  {k:<9} {med[k]:10.3f} ms  ({min(v):.3f} .. {max(v):.3f})   {med[k] / T:8.4f} ms/step")
            model_ms = (n_two * med["full"] + (T - n_two) * med["unguided"]) / T
            lines.append(f"  interval vs n_two * t_full + n_single * t_unguided = {model_ms:.3f} ms: {med['interval'] - model_ms:+.3f} ms "
                         f"({100.0 * (med['interval'] / model_ms - 1.0):+.2f} %), {len(plan)} segments; saves "
                         f"{100.0 * (1.0 - med['interval'] / med['full']):.1f} % of the full-guidance call")
            lines.append(f"  rescale vs full: {med['rescale'] - med['full']:+.3f} ms per call ({(med['rescale'] - med['full']) / T * 1e3:+.1f} us per step, "
                         f"{100.0 * (med['rescale'] / med['full'] - 1.0):+.2f} %); full windows' spread "
                         f"{100.0 * (min(ms['full']) / med['full'] - 1.0):+.2f} .. {100.0 * (max(ms['full']) / med['full'] - 1.0):+.2f} %")
            flush()
            del chans, emb, noise
        del model
        torch.cuda.empty_cache()
    sys.stdout.write(flush())
    return 0


if __name__ == "__main__":
    sys.exit(main())
