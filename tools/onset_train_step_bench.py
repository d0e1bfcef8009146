"""Milliseconds per VideoOnsetNet training step at the reference's configuration: batch 16 x (3, 30, 112, 112) (cfg/data/
data-onset-greatesthit.yaml: 2 s chunks at 15 fps), forward + BCLoss + backward + fused AdamW -- the HIP path (VideoOnsetNet.train(),
syncfusion_amd/onset_training.py) and, in the same run, the same step on torch's own nn.Conv3d / nn.BatchNorm3d modules (MIOpen).

Device events around `--steps` steps after `--warmup` steps; FLOPs per step = 3 x the forward's convolutions (forward, data and weight
gradients; the stem has no data gradient, so this slightly overstates the work); peak memory from torch.cuda.max_memory_allocated.

    python tools/onset_train_step_bench.py [--batch 16] [--steps 5] [--warmup 2] [--skip-torch] [--split-phase [--rccl]] [--loss hip [--graph]]

`--split-phase` adds a leg that sends every BatchNorm through the cross-rank kernels (sf_op_bn_sync_*) at world size 1: the price of the extra
launches of data-parallel training with no link cost in it.  With `--rccl` a one-rank nccl process group carries the 2 x 37 gathers (RCCL
on device tensors); without it the "gather" is a reshape.

`--loss hip` adds the step as a trainer runs it, `Model.training_step` (forward, loss AND the step metrics) + backward + AdamW, twice: with the
default `BCLoss` (ATen loss, metrics on the host: three device-to-host copies per step) and with `loss="hip"` (loss and metrics in the HIP
library, nothing read back).  `--graph` (with `--loss hip`) adds the same step replayed from one HIP graph, the HIP AdamW captured with it
(`GraphedOnsetTrainStep`).  `--rounds R` repeats these legs R times in alternation (A B C A B C ...) and reports each leg's median.  The first row
("HIP path": forward + loss + backward + AdamW, no metrics) is unchanged; the leg `hip_no_metrics` is that step again, inside the alternation.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.onsetnet_ref import onsetnet_flops  # noqa: E402
from syncfusion_amd import OnsetModel, VideoOnsetNet  # noqa: E402


def torch_modules_forward(net, x):
    """main/onset_net.py:57-63 on the nn modules that hold the parameters (train-mode BatchNorm, MIOpen convolutions)."""
    m = net.net.model
    h = m.stem(x)
    for name in ("layer1", "layer2", "layer3", "layer4"):
        for blk in getattr(m, name):
            res = h if blk.downsample is None else blk.downsample(h)
            h = F.relu(blk.conv2(blk.conv1(h)) + res)
    return net.fc(h.mean(dim=(3, 4)).transpose(-1, -2)).squeeze(-1)


def time_steps(model, forward, batch, steps, warmup):
    opt = model.configure_optimizers()

    def step():
        opt.zero_grad(set_to_none=True)
        loss = model.loss(forward(batch["frames"]), batch["label"])
        loss.backward()
        opt.step()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps, torch.cuda.max_memory_allocated() / 2**30


def time_loop(step, steps, warmup):
    """ms per call of `step` over `steps` calls after `warmup` calls (device events)."""
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


def loss_legs(dev, batch, graph: bool):
    """name -> step(): Model.training_step (loss + metrics) + backward + AdamW on fresh models; the graphed leg is built first, before any eager
    backward of the process touches its parameters."""
    from syncfusion_amd import GraphedOnsetTrainStep

    legs = {}
    if graph:
        model = OnsetModel(1e-4, 0.9, 0.999, 1e-8, 1e-2, VideoOnsetNet(False).to(dev).train(), optimizer="hip", loss="hip").to(dev)
        gs = GraphedOnsetTrainStep(model, batch, optimizer=model.configure_optimizers())
        legs["training_step_hip_loss_graph"] = lambda: gs.step(batch)
    for name, kw, metrics in (("hip_no_metrics", {}, False), ("training_step_torch_loss", {}, True), ("training_step_hip_loss", {"loss": "hip"}, True)):
        model = OnsetModel(1e-4, 0.9, 0.999, 1e-8, 1e-2, VideoOnsetNet(False).to(dev).train(), **kw).to(dev)
        opt = model.configure_optimizers()

        def step(model=model, opt=opt, metrics=metrics):
            opt.zero_grad(set_to_none=True)
            # hip_no_metrics: the first row's step (loss only) again, inside the alternation
            loss = model.training_step(batch, 0) if metrics else model.loss(model.model(batch["frames"]), batch["label"])
            loss.backward()
            opt.step()

        legs[name] = step
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--split-phase", action="store_true", help="also time the step with every BatchNorm on the split-phase (cross-rank) kernels")
    ap.add_argument("--rccl", action="store_true", help="with --split-phase: a one-rank nccl group carries the gathers")
    ap.add_argument("--master-port", type=int, default=29671)
    ap.add_argument("--loss", choices=("torch", "hip"), default="torch", help="hip: also time Model.training_step with the host and the device loss / metrics")
    ap.add_argument("--graph", action="store_true", help="with --loss hip: also time the step replayed from one HIP graph (GraphedOnsetTrainStep)")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds of the --loss hip legs (the median is reported)")
    a = ap.parse_args()
    if a.graph and a.loss != "hip":
        ap.error("--graph needs --loss hip")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    N, T, S = a.batch, a.frames, a.size
    batch = {"frames": torch.randn(N, 3, T, S, S, device=dev), "label": (torch.rand(N, T, device=dev) < 0.2).float()}
    batch["label"][0, 0] = 1.0
    fwd_flop = N * (onsetnet_flops(T, S, S) - 2.0 * T * (512 * 128 + 128))   # the convolutions
    step_flop = 3 * fwd_flop
    out = {"shape": [N, 3, T, S, S], "tflop_per_step": step_flop / 1e12}
    net = VideoOnsetNet(False).to(dev).train()
    model = OnsetModel(1e-4, 0.9, 0.999, 1e-8, 1e-2, net).to(dev)
    ms, gib = time_steps(model, net, batch, a.steps, a.warmup)
    out["hip"] = {"ms_per_step": round(ms, 2), "tflops": round(step_flop / ms / 1e9, 2), "peak_gib": round(gib, 2)}
    print(f"HIP path    : {ms:8.2f} ms/step  {step_flop / ms / 1e9:6.2f} TFLOP/s  peak {gib:6.2f} GiB", flush=True)
    if a.loss == "hip":
        legs = loss_legs(dev, batch, a.graph)
        runs = {name: [] for name in legs}
        for _ in range(max(1, a.rounds)):
            for name, step in legs.items():
                runs[name].append(time_loop(step, a.steps, a.warmup))
        for name, ms_all in runs.items():
            med = sorted(ms_all)[len(ms_all) // 2]
            out[name] = {"ms_per_step": round(med, 2), "rounds": [round(v, 2) for v in ms_all]}
            print(f"{name:30s}: {med:8.2f} ms/step  (rounds {', '.join(f'{v:.2f}' for v in ms_all)})", flush=True)
        del legs
        torch.cuda.empty_cache()
    if a.split_phase:
        from syncfusion_amd.onset_training import onset_train_forward

        if a.rccl:
            import torch.distributed as dist

            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(a.master_port))
            dist.init_process_group("nccl", rank=0, world_size=1)
        del model, net
        torch.cuda.empty_cache()
        net = torch.nn.SyncBatchNorm.convert_sync_batchnorm(VideoOnsetNet(False)).to(dev).train()
        model = OnsetModel(1e-4, 0.9, 0.999, 1e-8, 1e-2, net).to(dev)
        ms_s, gib_s = time_steps(model, lambda x: onset_train_forward(net, x, _force_sync=True), batch, a.steps, a.warmup)
        out["hip_split_phase"] = {"ms_per_step": round(ms_s, 2), "tflops": round(step_flop / ms_s / 1e9, 2), "peak_gib": round(gib_s, 2),
                                  "gathers": "rccl, one rank" if a.rccl else "none (reshape)"}
        print(f"HIP split-phase ({out['hip_split_phase']['gathers']}): {ms_s:8.2f} ms/step  {step_flop / ms_s / 1e9:6.2f} TFLOP/s  peak {gib_s:6.2f} GiB",
              flush=True)
        if a.rccl:
            dist.destroy_process_group()
    if not a.skip_torch:
        del model, net
        torch.cuda.empty_cache()
        net = VideoOnsetNet(False).to(dev).train()
        model = OnsetModel(1e-4, 0.9, 0.999, 1e-8, 1e-2, net).to(dev)
        ms_t, gib_t = time_steps(model, lambda x: torch_modules_forward(net, x), batch, a.steps, a.warmup)
        out["torch_modules"] = {"ms_per_step": round(ms_t, 2), "tflops": round(step_flop / ms_t / 1e9, 2), "peak_gib": round(gib_t, 2)}
        print(f"torch (MIOpen): {ms_t:8.2f} ms/step  {step_flop / ms_t / 1e9:6.2f} TFLOP/s  peak {gib_t:6.2f} GiB", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
