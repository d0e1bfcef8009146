"""The onset net's test stage on one MI355X: milliseconds per test batch of ``OnsetTestStage.step`` beside the path the package offered
before it, and the whole stage over a frame directory.

  (a) the net at ``--clips`` x (3, ``--frames``, 112, 112), frames already on the device:
        stage          ``OnsetTestStage.step``: one eval forward + one ``sf_op_onset_test_step``; nothing is read back per step
        parent api     ``OnsetModel(loss="hip").test_step`` (forward, device loss and metrics), then -- ``test_step`` returns the loss only -- a
                       second forward for the logits as the reference's ``log_annotations`` does, ``.cpu()`` of logits and labels, numpy threshold
        parent 1 fwd   the same by hand with ONE forward: net, ``DeviceBCLoss`` forward / evaluate, ``.cpu()`` of logits and labels, numpy threshold
  (b) synthetic logits alone (no net): ``step_logits`` against ``DeviceBCLoss`` forward / evaluate + ``.cpu()`` + numpy threshold
  (c) ``test_onset_model`` over a generated frame directory (``--videos`` videos of ``--seconds`` s at 15 frames per second, 240 x 320 JPEG,
      the size script/gh_preprocess_videos.py extracts) with ``num_workers`` 0 and ``--workers``; beside it the time of decoding the same
      frames alone (one host thread / the same thread pool) and its share of the stage's time.

Timing: a host clock around ``--iters`` steps that end in a device synchronise; ``--windows`` windows per leg after ``--warmup`` steps, the legs
of a group ALTERNATING window by window in this one process; min / median / max over the windows.  (c): wall time of whole runs, alternating,
``--runs`` each, after one untimed run (first-use set-up, page cache).

    python tools/onset_test_stage_bench.py [--clips 16] [--frames 30] [--iters 20] [--windows 7] [--warmup 3] [--videos 8] [--seconds 10]
                                           [--workers 8] [--runs 3] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows(legs, iters, n_windows, warmup):
    """legs: {name: fn}; -> {name: (min, median, max) ms per call}, the legs alternating window by window."""
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(n_windows):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / iters)
    return {k: (min(v), statistics.median(v), max(v)) for k, v in ms.items()}


def make_frame_directory(root, videos, seconds, rate=15, hw=(240, 320)):
    from PIL import Image

    rs = np.random.RandomState(0)
    names = []
    for v in range(videos):
        name = f"video{v:03d}"
        d = os.path.join(root, name, "frames")
        os.makedirs(d)
        base = rs.randint(0, 256, size=(hw[0] // 8, hw[1] // 8, 3))
        for i in range(int(seconds * rate)):
            img = np.kron(np.roll(base, i, axis=1), np.ones((8, 8, 1))).astype(np.uint8)
            img[::3] //= 2                                              # some texture for the JPEG coder
            Image.fromarray(img).save(os.path.join(d, f"{i + 1}.jpg"), quality=90)
        with open(os.path.join(root, name, f"{name}.metadata.json"), "w") as f:
            json.dump({"processed": {"video_frame_rate": float(rate), "video_duration": float(seconds) + 0.05}}, f)
        with open(os.path.join(root, name, f"{name}.times.csv"), "w") as f:
            f.write("".join(f"{t:.3f},hit\n" for t in np.arange(0.4, seconds, 0.9)))
        names.append(name)
    return names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("onset_test_stage_bench: no GPU visible (nothing here is measured on a CPU)")
    torch.set_grad_enabled(False)
    from syncfusion_amd import OnsetModel, OnsetTestStage, VideoOnsetNet, onset_test, video_chunks
    from syncfusion_amd.onset_loss import DeviceBCLoss

    dev = torch.device("cuda:0")
    N, T = a.clips, a.frames
    torch.manual_seed(0)
    net = VideoOnsetNet(False).to(dev).eval()
    model = OnsetModel(1e-4, 0.9, 0.999, 1e-8, 1e-2, net, loss="hip").to(dev)
    frames = torch.randn(N, 3, T, 112, 112, device=dev)
    labels = (torch.rand(N, T, device=dev) < 0.1).float()
    labels[0, 0], labels[0, 1] = 1.0, 0.0
    chunks = [dict(video_name="v", start_frame=i * T, end_frame=(i + 1) * T, frame_rate=15.0) for i in range(N)]
    batch = {"frames": frames, "label": labels}
    crit = DeviceBCLoss()
    lines, result = [], {"clips": N, "frames": T, "device": torch.cuda.get_device_name(0)}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def host_threshold(logits, lab):
        p, t = logits.cpu().numpy(), lab.cpu().numpy()                  # the read-back of every step
        return [np.nonzero(r > 0.5)[0] for r in p], [np.nonzero(r)[0] for r in t]

    stage = OnsetTestStage(net, capacity=N * (a.iters * (a.windows + 1) + a.warmup + 1))

    def leg_stage():
        if stage.capacity and stage.clips + N > stage.capacity:                   # keep the tables at one size: growth is not what is timed
            stage.reset()
        stage.step(frames, labels, chunks)

    def leg_parent_api():
        model.test_step(batch, 0)
        return host_threshold(model.model(frames), labels)

    def leg_parent_one_forward():
        pred = net(frames)
        crit(pred, labels)
        crit.evaluate(pred, labels)
        return host_threshold(pred, labels)

    say(f"# onset test stage, {result['device']}, {N} x (3, {T}, 112, 112); ms per step: min / median / max over {a.windows} alternating windows of {a.iters} steps")
    r = windows({"stage": leg_stage, "parent_api": leg_parent_api, "parent_one_forward": leg_parent_one_forward}, a.iters, a.windows, a.warmup)
    for k, (lo, med, hi) in r.items():
        say(f"(a) net   {k:20s} {lo:8.3f} / {med:8.3f} / {hi:8.3f} ms   {N / med * 1e3:8.1f} clips/s")
    result["net"] = {k: {"ms_min": v[0], "ms_median": v[1], "ms_max": v[2]} for k, v in r.items()}

    logits = torch.randn(N, T, device=dev)
    lstage = OnsetTestStage(net, capacity=N * 4096)

    def leg_logits_stage():
        if lstage.capacity and lstage.clips + N > lstage.capacity:
            lstage.reset()
        lstage.step_logits(logits, labels, chunks)

    def leg_logits_parent():
        crit(logits, labels)
        crit.evaluate(logits, labels)
        return host_threshold(logits, labels)

    it = a.iters * 10
    r = windows({"stage": leg_logits_stage, "parent": leg_logits_parent}, it, a.windows, a.warmup)
    for k, (lo, med, hi) in r.items():
        say(f"(b) logits {k:19s} {lo:8.3f} / {med:8.3f} / {hi:8.3f} ms   ({it} steps per window)")
    result["logits"] = {k: {"ms_min": v[0], "ms_median": v[1], "ms_max": v[2]} for k, v in r.items()}

    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        names = make_frame_directory(tmp, a.videos, a.seconds)
        table = video_chunks.chunk_table(tmp, names)
        n_frames = sum(c["end_frame"] - c["start_frame"] for c in table)
        say(f"(c) frame directory: {a.videos} videos, {len(table)} clips, {n_frames} frames of 240 x 320 (written in {time.perf_counter() - t0:.1f} s)")

        def decode(workers):
            t0 = time.perf_counter()
            if workers:
                with ThreadPoolExecutor(workers) as pool:
                    list(pool.map(lambda c: video_chunks.chunk_frames_u8(c, ".jpg", False), table))
            else:
                for c in table:
                    video_chunks.chunk_frames_u8(c, ".jpg", False)
            return time.perf_counter() - t0

        def full(workers):
            t0 = time.perf_counter()
            onset_test.test_onset_model(model, tmp, names, os.path.join(tmp, f"out{workers}"), batch_size=N, num_workers=workers)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        full(0)
        times = {("decode", 0): [], ("decode", a.workers): [], ("stage", 0): [], ("stage", a.workers): []}
        for _ in range(a.runs):
            for what, w in times:
                times[(what, w)].append(decode(w) if what == "decode" else full(w))
        result["directory"] = {"clips": len(table), "frames": n_frames}
        for w in (0, a.workers):
            d, s = statistics.median(times[("decode", w)]), statistics.median(times[("stage", w)])
            say(f"(c) num_workers {w}: stage {s:7.3f} s ({len(table) / s:7.1f} clips/s; min {min(times[('stage', w)]):.3f} max {max(times[('stage', w)]):.3f})   "
                f"decoding alone {d:7.3f} s = {100 * d / s:5.1f} % of the stage")
            result["directory"][f"workers_{w}"] = {"stage_s": s, "decode_alone_s": d, "decode_share": d / s}
    say(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
