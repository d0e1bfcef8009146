"""numpy restatement of the onset net's test-stage annotations (main/module_onset.py:142-229) that goes the reference's FILE ROUTE: one
csv per chunk and per kind written with ``np.savetxt``, then per video the chunk files in natural order read back with ``np.loadtxt``,
merged, written again, and the chunk files deleted.  ``syncfusion_amd.onset_test`` takes an in-memory shortcut; the tests check it against
this.  Written from the description of the stage, not from the kernels: element-wise loops for the rows, real files for the merge."""
from __future__ import annotations

import glob
import os
import re
import warnings
from typing import Dict, List, Sequence, Tuple

import numpy as np


def rows_ref(logits: np.ndarray, labels: np.ndarray, threshold: float = 0.5) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(pred_count, pred_frames, target_count, target_frames): per clip the frames whose fp32 logit is > threshold (NaN: never), resp. whose
    label is non-zero, in ascending order, the rest of the row -1."""
    z = np.asarray(logits, dtype=np.float32)
    t = np.asarray(labels)
    N, T = z.shape
    thr = np.float32(threshold)
    pc, tc = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    pf, tf = np.full((N, T), -1, dtype=np.int32), np.full((N, T), -1, dtype=np.int32)
    for n in range(N):
        for j in range(T):
            v = z[n, j]
            if not np.isnan(v) and v > thr:
                pf[n, pc[n]] = j
                pc[n] += 1
            if t[n, j] != 0:
                tf[n, tc[n]] = j
                tc[n] += 1
    return pc, pf, tc, tf


def _natural_key(path: str):
    return [int(p) if p.isdigit() else p for p in re.split(r"(\d+)", os.path.basename(path))]


def _load(path: str) -> List[float]:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # np.loadtxt warns about an empty file
        v = np.loadtxt(path, delimiter=",").tolist()
    return [v] if isinstance(v, float) else v


def write_chunk_files(run_dir: str, clips: Sequence[dict], pred_idx: Sequence[np.ndarray], target_idx: Sequence[np.ndarray]) -> None:
    """One batch (or many) of ``log_annotations``: clip i has ``video_name``, ``start_frame``, ``end_frame``, ``frame_rate`` and the onset
    frame indices ``pred_idx[i]`` / ``target_idx[i]``."""
    for kind, idx in (("target", target_idx), ("pred", pred_idx)):
        d = os.path.join(run_dir, "media", "annotations", kind)
        os.makedirs(d, exist_ok=True)
        for c, ix in zip(clips, idx):
            times = (np.asarray(ix, dtype=np.int64) + np.int64(c["start_frame"])) / np.asarray(c["frame_rate"])
            np.savetxt(os.path.join(d, f"{c['video_name']}.{c['start_frame']}-{c['end_frame']}.times.csv"), times, fmt="%.4f", delimiter=",")


def concat_chunk_files(run_dir: str) -> Dict[str, Dict[str, bytes]]:
    """``concat_annotations``: -> {kind: {video: bytes of the merged file}}; afterwards the directories hold the merged files only."""
    out: Dict[str, Dict[str, bytes]] = {}
    tdir = os.path.join(run_dir, "media", "annotations", "target")
    videos = {os.path.basename(p).split(".")[0] for p in glob.glob(os.path.join(tdir, "*.times.csv"))}
    for kind in ("target", "pred"):
        d = os.path.join(run_dir, "media", "annotations", kind)
        out[kind] = {}
        for video in videos:
            merged: List[float] = []
            for p in sorted(glob.glob(os.path.join(d, f"{video}.*.times.csv")), key=_natural_key):
                merged += _load(p)
            np.savetxt(os.path.join(d, f"{video}.times.csv"), merged, fmt="%.4f", delimiter="\n")
        for p in glob.glob(os.path.join(d, "*.*.times.csv")):
            os.remove(p)
        for video in videos:
            with open(os.path.join(d, f"{video}.times.csv"), "rb") as f:
                out[kind][video] = f.read()
    return out


def file_route(run_dir: str, batches: Sequence[Tuple[np.ndarray, np.ndarray, Sequence[dict]]]) -> Dict[str, Dict[str, bytes]]:
    """Batches of (logits (N, T), labels (N, T), clip records) -> the merged files' bytes, through the per-chunk files."""
    for logits, labels, clips in batches:
        pc, pf, tc, tf = rows_ref(logits, labels)
        write_chunk_files(run_dir, clips, [pf[i, : pc[i]] for i in range(len(clips))], [tf[i, : tc[i]] for i in range(len(clips))])
    return concat_chunk_files(run_dir)


def read_dir(run_dir: str) -> Dict[str, Dict[str, bytes]]:
    """{kind: {video: bytes}} of EVERY file under media/annotations/{target,pred} (names minus ``.times.csv``)."""
    out: Dict[str, Dict[str, bytes]] = {}
    for kind in ("target", "pred"):
        d = os.path.join(run_dir, "media", "annotations", kind)
        out[kind] = {}
        for name in sorted(os.listdir(d)):
            assert name.endswith(".times.csv"), name
            with open(os.path.join(d, name), "rb") as f:
                out[kind][name[: -len(".times.csv")]] = f.read()
    return out


def special_rows(z: np.ndarray) -> np.ndarray:
    """Overwrite rows 1 .. min(N - 1, 7) of grid logits with the threshold's edge cases -- all below, all above, exactly 0.5,
    nextafter(0.5, 1), NaN, +inf, -inf, starting at entry T % 7 of that list so that small batches of different T cover different cases --
    and, when there is a row 8, mix NaN and +inf into it.  Row 0 and the rows behind stay grid values."""
    z = z.copy()
    N, T = z.shape
    fills = [-3.0, 3.0, 0.5, np.nextafter(np.float32(0.5), np.float32(1.0)), np.nan, np.inf, -np.inf]
    for n in range(1, min(N, 8)):
        z[n, :] = fills[(n - 1 + T) % 7]
    if N > 8:
        z[8, ::3] = np.nan
        z[8, 1::3] = np.inf
    return z
