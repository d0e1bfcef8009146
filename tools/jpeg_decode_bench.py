"""JPEG decoding for the onset path on one MI355X: Pillow on the host against the device decoder (syncfusion_amd/jpeg.py), over the frame
directory of tools/onset_test_stage_bench.py leg (c) (``--videos`` videos of ``--seconds`` s at 15 frames per second, 240 x 320 JPEG written by
Pillow at 4:2:0), and the whole test stage with either decoder.

  (a) pil, 0 threads    ``read_frames_u8`` chunk after chunk on one host thread (uint8 frames on the host; no upload)
  (b) pil, N threads    the same chunks over a pool of ``--workers`` threads
  (c) hip               per batch of ``--clips`` chunks: read the files, parse, one pinned upload, ``sf_jpeg_decode``; frames on the device
  (d) kernels alone     ``sf_jpeg_decode`` on a staged batch that is already on the device (memsets + entropy + IDCT + colour kernels)
  stage                 ``video_chunks.run_onset_test`` over the directory: decoder pil (= ``test_onset_model``) / hip, num_workers 0 /
                        ``--workers`` (with hip the threads only read files)

(a) - (c) decode every frame of the directory once per window and end in a device synchronise; (d) is one batch per call, ``--iters`` calls
per window.  ``--windows`` windows per leg after one untimed pass, the legs ALTERNATING window by window in this one process; min / median /
max over the windows.  Verdict: (c) counts as faster than (b) when the medians differ by more than (b)'s own min-max spread.

    python tools/jpeg_decode_bench.py [--videos 8] [--seconds 10] [--clips 16] [--workers 8] [--windows 5] [--iters 20] [--runs 3] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_decode_bench: no GPU visible (nothing here is measured on a CPU)")
    torch.set_grad_enabled(False)
    from onset_test_stage_bench import make_frame_directory
    from syncfusion_amd import OnsetModel, VideoOnsetNet, _lib, jpeg, video_chunks

    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines, result = [], {"device": torch.cuda.get_device_name(0)}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as tmp:
        names = make_frame_directory(tmp, a.videos, a.seconds)
        table = video_chunks.chunk_table(tmp, names)
        paths = [video_chunks.chunk_frame_paths(c) for c in table]
        n_frames = sum(len(p) for p in paths)
        n_bytes = sum(os.path.getsize(f) for p in paths for f in p)
        say(f"# JPEG decode, {result['device']}: {len(table)} clips, {n_frames} frames of 240 x 320 (4:2:0, {n_bytes / n_frames / 1024:.1f} KiB per file); "
            f"min / median / max over {a.windows} alternating windows")
        batches = [paths[i: i + a.clips] for i in range(0, len(paths), a.clips)]

        def leg_pil0():
            for p in paths:
                video_chunks.read_frames_u8(p, False)

        def leg_pil_threads():
            with ThreadPoolExecutor(a.workers) as pool:
                list(pool.map(lambda p: video_chunks.read_frames_u8(p, False), paths))

        def leg_hip():
            for b in batches:
                video_chunks.batch_frames_device(b, dev)
            torch.cuda.synchronize()

        # (d): one batch staged on the device once
        blobs = [x for p in batches[0] for x in jpeg.read_files(p)]
        st = jpeg._Staged(blobs, pin=True)
        staged = st.host[: st.used].to(dev)
        H, W = st.desc[0].height, st.desc[0].width
        ws_bytes = int(lib.sf_jpeg_decode_workspace_bytes(C.addressof(st.desc), st.n))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty((st.n, H, W, 3), dtype=torch.uint8, device=dev)
        status = torch.empty(st.n, dtype=torch.int32, device=dev)
        stream = _lib.stream_ptr(dev)

        def kernels():
            base = staged.data_ptr()
            _lib.check(lib.sf_jpeg_decode(base, st.n_bytes, C.addressof(st.desc), base + st.desc_at, base + st.seg_at, st.n_segs, st.n, H, W, out.data_ptr(),
                                          status.data_ptr(), ws.data_ptr(), ws_bytes, stream), "sf_jpeg_decode")

        def leg_kernels():
            for _ in range(a.iters):
                kernels()
            torch.cuda.synchronize()

        legs = {"(a) pil, 0 threads": leg_pil0, f"(b) pil, {a.workers} threads": leg_pil_threads, "(c) hip": leg_hip, "(d) kernels alone": leg_kernels}
        for fn in legs.values():
            fn()
        assert int(status.count_nonzero()) == 0
        ms = {k: [] for k in legs}
        for _ in range(a.windows):
            for k, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        stats = {k: (min(v), statistics.median(v), max(v)) for k, v in ms.items()}
        for k, (lo, med, hi) in stats.items():
            if k.startswith("(d)"):
                per = med / a.iters
                say(f"{k:22s} {lo / a.iters:9.3f} / {per:9.3f} / {hi / a.iters:9.3f} ms per batch of {st.n} frames   {st.n / per * 1e3:10.0f} frames/s   "
                    f"(workspace {ws_bytes / 2**20:.1f} MiB, {st.n_bytes / 2**20:.1f} MiB of files)")
            else:
                say(f"{k:22s} {lo:9.1f} / {med:9.1f} / {hi:9.1f} ms per {n_frames} frames   {n_frames / med * 1e3:10.0f} frames/s")
        kb, kc = f"(b) pil, {a.workers} threads", "(c) hip"
        spread = stats[kb][2] - stats[kb][0]
        gain = stats[kb][1] - stats[kc][1]
        faster = gain > spread
        say(f"(c) against (b): {stats[kb][1] / stats[kc][1]:.2f}x (median {stats[kb][1]:.1f} ms -> {stats[kc][1]:.1f} ms; (b)'s min-max spread {spread:.1f} ms): "
            f"{'FASTER by more than the spread' if faster else 'NOT faster by more than the spread'}")
        per_call = {k: (a.iters if k.startswith("(d)") else 1) for k in stats}          # (d): ms per batch, as in the text line
        result["legs"] = {k: {"ms_min": v[0] / per_call[k], "ms_median": v[1] / per_call[k], "ms_max": v[2] / per_call[k]} for k, v in stats.items()}
        result["hip_over_pil_threads"] = stats[kb][1] / stats[kc][1]
        result["hip_faster_than_spread"] = bool(faster)

        torch.manual_seed(0)
        model = OnsetModel(1e-4, 0.9, 0.999, 1e-8, 1e-2, VideoOnsetNet(False).to(dev).eval(), loss="hip").to(dev)

        def full(decoder, workers):
            t0 = time.perf_counter()
            video_chunks.run_onset_test(model, tmp, names, None, batch_size=a.clips, num_workers=workers, decoder=decoder)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        full("pil", 0)
        full("hip", 0)
        keys = [("pil", 0), ("pil", a.workers), ("hip", 0), ("hip", a.workers)]
        times = {k: [] for k in keys}
        for _ in range(a.runs):
            for k in keys:
                times[k].append(full(*k))
        result["stage"] = {}
        for (decoder, w), v in times.items():
            s = statistics.median(v)
            say(f"stage decoder={decoder:3s} num_workers {w}: {s:7.3f} s   {len(table) / s:8.1f} clips/s   (min {min(v):.3f} max {max(v):.3f}, {a.runs} alternating runs)")
            result["stage"][f"{decoder}_workers_{w}"] = {"s_median": s, "clips_per_s": len(table) / s}
    say(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
