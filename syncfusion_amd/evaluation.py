"""The reference's onset-sync evaluation, ``script/evaluate_onset.py --gen_dir ... --tar_dir ...``, as one call: ``evaluate_onsets``.

The reference loads every wav of the two directories with librosa at 22050 Hz, runs ``librosa.onset.onset_detect(delta=0.3)`` on each
(script/evaluate_onset.py:20-33), and scores every generated file against the target of the same name (:35-93, :159-191): onset-count
match, detection accuracy and detection average precision, averaged over the files.  Here the detector is the device front end of
``audio_features.py`` (clips of equal length run as one batch; counts, positions and confidences come back in one copy per batch); the
scoring works on a handful of integers per file and stays on the host, restated in plain Python / numpy.

What is kept, including what the reference does by accident:

* non-maximum suppression (:35-48): generated onsets in descending confidence (equal confidences: the later onset first, numpy's stable
  ``argsort`` reversed); a surviving onset drops the remaining ones closer than ``0.05 s`` -- but the reference deletes from the list it
  is walking, so the onset right after a dropped one is not examined in that pass.  Reproduced.
* matching (:51-93): targets in order; of the free generated onsets closer than ``delta`` seconds the one with the largest ``w[o]`` wins
  (a tie: the later one); a target without candidate scores 0 as a positive; once no generated onset is free the remaining targets are
  not scored at all (the early ``break``); free generated onsets left over are negatives scored with their confidence.
* per file (:159-191): no onsets on either side -> count match False, acc 0, AP 0; ``remove_head`` filters both sides AFTER that test;
  ``multi_delta`` averages over ``arange(0.1, delta + 0.05, 0.05)``.

What is defined where the reference is not:

* the confidence window ``w[o - ci : o + ci]`` is clipped to the clip (``max(0, o - ci) : min(L, o + ci)``): for an onset in the first
  0.05 s the reference's negative start index wraps around and its ``np.max`` of an empty slice raises; ``w[o]`` for ``o == L`` is 0;
* average precision is the step-wise definition (sklearn's ``average_precision_score``; tied scores are one threshold).  A file that is
  left with one class only after ``remove_head`` -- no target onset, so no positive: the AP is NaN, and with nothing to score at all the
  reference's call raises -- counts as AP 0, the value the reference gives a file with an empty side.  (All positives is defined: AP 1.)
* a file whose sample rate is not 22050 goes through ``syncfusion_amd.resample`` -- the windowed-sinc resampler of this package (torchaudio's
  algorithm), NOT librosa's resampler (soxr): onsets of such files can differ from the reference's by the resamplers' difference;
* multi-channel files are averaged to mono, as ``librosa.load`` does.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .audio_features import onset_detect_batch
from .generation import load_wav
from .resample import resample

EVAL_SR = 22050
DETECT_DELTA = 0.3        # script/evaluate_onset.py:30


def average_precision(y: Sequence[int], s: Sequence[float]) -> float:
    """Step-wise AP: sum over the thresholds (distinct scores, descending) of (recall - previous recall) * precision.  NaN without positives."""
    y, s = np.asarray(y, dtype=np.int64), np.asarray(s, dtype=np.float64)
    n_pos = int(y.sum())
    if n_pos == 0:
        return float("nan")
    order = np.argsort(-s, kind="stable")
    y, s = y[order], s[order]
    tp = np.cumsum(y)
    last = np.nonzero(np.append(s[1:] != s[:-1], True))[0]      # the last element of every run of equal scores
    recall = tp[last] / n_pos
    precision = tp[last] / (last + 1)
    return float(np.sum(np.diff(np.concatenate([[0.0], recall])) * precision))


def onset_nms(onsets: Sequence[int], confidence: Sequence[float], window: float = 0.05, sr: int = EVAL_SR) -> List[int]:
    remaining = [int(o) for o in onsets]
    kept = []
    for idx in np.argsort(np.asarray(confidence, dtype=np.float64), kind="stable")[::-1]:
        cur = int(onsets[idx])
        if cur not in remaining:
            continue
        kept.append(cur)
        survivors, spared = [], False
        for o in remaining:
            if o == cur:
                continue
            if spared or not abs(cur - o) < window * sr:   # the neighbour right after a dropped onset is spared in this pass
                survivors.append(o)
                spared = False
            else:
                spared = True
        remaining = survivors
    return sorted(kept)


def match_onsets(tar: Sequence[int], gen: Sequence[int], confidence: Sequence[float], strength: Sequence[float], delta: float = 0.1,
                 sr: int = EVAL_SR) -> Tuple[float, float, List[int]]:
    """``eval_osnets`` (:51-93): -> (accuracy, average precision, hit flag per generated onset that survived the NMS)."""
    conf = {int(o): float(c) for o, c in zip(gen, confidence)}
    stren = {int(o): float(c) for o, c in zip(gen, strength)}
    kept = onset_nms(gen, confidence, sr=sr)
    free = list(kept)
    flags = {g: 0 for g in kept}
    labels, scores, hits = [], [], 0
    for o in tar:
        best = None
        for g in free:                                          # ascending; `>=` lets a later onset take a tie
            if abs(g - o) < delta * sr and (best is None or stren[g] >= stren[best]):
                best = g
        labels.append(1)
        if best is None:
            scores.append(0.0)
            continue
        hits += 1
        scores.append(conf[best])
        flags[best] = 1
        free.remove(best)
        if not free:
            break
    labels += [0] * len(free)
    scores += [conf[g] for g in free]
    acc = hits / len(tar) if len(tar) else 0.0
    ap = average_precision(labels, scores) if labels else float("nan")
    return acc, ap, [flags[g] for g in kept]


def score_file(tar: Optional[Dict[str, np.ndarray]], gen: Dict[str, np.ndarray], delta: float = 0.1, remove_head: Optional[float] = None,
               multi_delta: bool = False, sr: int = EVAL_SR) -> Dict[str, object]:
    """One iteration of the reference's loop over the generated files (:159-191).  tar / gen: {"onsets", "confidence", "strength"}."""
    o1 = [int(o) for o in tar["onsets"]] if tar is not None else []
    o2 = [int(o) for o in gen["onsets"]]
    if not o1 or not o2:
        return {"count_match": False, "acc": 0.0, "ap": 0.0, "n_tar": len(o1), "n_gen": len(o2)}
    conf, stren = list(gen["confidence"]), list(gen["strength"])
    if remove_head is not None:
        keep = [i for i, o in enumerate(o2) if o >= remove_head * sr]
        o1 = [o for o in o1 if o >= remove_head * sr]
        o2, conf, stren = [o2[i] for i in keep], [conf[i] for i in keep], [stren[i] for i in keep]
    deltas = [float(d) for d in np.arange(0.1, delta + 0.05, 0.05)] if multi_delta else [float(delta)]
    acc = ap = 0.0
    for d in deltas:
        a, p, _ = match_onsets(o1, o2, conf, stren, d, sr)
        acc += a
        ap += 0.0 if np.isnan(p) else p
    return {"count_match": len(o1) == len(o2), "acc": acc / len(deltas), "ap": ap / len(deltas), "n_tar": len(o1), "n_gen": len(o2)}


def detect_dir(audio_dir, device, batch_size: int = 64, delta: float = DETECT_DELTA) -> Dict[str, Dict[str, object]]:
    """``detect_onset`` (:20-33) for every ``*.wav`` of a directory: file name -> {"onsets", "confidence", "strength", "resampled_from"}."""
    paths = sorted(Path(audio_dir).glob("*.wav"))
    clips: Dict[str, torch.Tensor] = {}
    rates: Dict[str, Optional[int]] = {}
    for p in paths:
        a, rate = load_wav(p)
        a = a.mean(dim=0)
        rates[p.name] = None
        if rate != EVAL_SR:
            a = resample(a.to(device), rate, EVAL_SR).cpu()
            rates[p.name] = rate
        clips[p.name] = a
    by_length: Dict[int, List[str]] = {}
    for name, a in clips.items():
        by_length.setdefault(int(a.numel()), []).append(name)
    out: Dict[str, Dict[str, object]] = {}
    for L, names in by_length.items():
        for i in range(0, len(names), batch_size):
            chunk = names[i:i + batch_size]
            if L < 1:
                rows = [{"onsets": np.zeros(0, np.int64), "confidence": np.zeros(0, np.float32), "strength": np.zeros(0, np.float32)} for _ in chunk]
            else:
                wav = torch.stack([clips[n] for n in chunk]).to(device)
                rows = onset_detect_batch(wav, sr=EVAL_SR, delta=delta).to_host()      # one copy per batch
            for n, r in zip(chunk, rows):
                r["resampled_from"] = rates[n]
                out[n] = r
    return {p.name: out[p.name] for p in paths}


def evaluate_onsets(gen_dir, tar_dir, delta: float = 0.1, remove_head: Optional[float] = None, multi_delta: bool = False, batch_size: int = 64,
                    device=None) -> Dict[str, object]:
    """``script/evaluate_onset.py`` for two directories of wav files -> ``{"onset_num_acc", "detection_acc", "detection_ap", "per_file"}``:
    the means over the generated files of the count match, the detection accuracy and the detection AP, and the per-file rows (with
    ``resampled_from``: the original rate of a generated file that went through the resampler, else None)."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    _lib.require_gpu_tensor(torch.empty(0, device=device), "evaluate_onsets")
    tar = detect_dir(tar_dir, device, batch_size)
    gen = detect_dir(gen_dir, device, batch_size)
    if not gen:
        raise ValueError(f"{gen_dir}: no wav files")
    per_file = {}
    for name, g in gen.items():
        row = score_file(tar.get(Path(name).stem + ".wav"), g, delta, remove_head, multi_delta)
        row["resampled_from"] = g["resampled_from"]
        per_file[name] = row
    rows = list(per_file.values())
    return {"onset_num_acc": float(np.mean([r["count_match"] for r in rows])), "detection_acc": float(np.mean([r["acc"] for r in rows])),
            "detection_ap": float(np.mean([r["ap"] for r in rows])), "per_file": per_file}


def summary_line(result: Dict[str, object]) -> str:
    """The reference's closing line (:191), same format."""
    return f"#onset acc: {result['onset_num_acc']:.4f}, detection acc: {result['detection_acc']:.4f}, detection ap: {result['detection_ap']:.4f}"
