"""fp64 / numpy restatement of the onset step metrics (main/module_onset.py:288-354, BCLoss.evaluate) and the inputs the loss / metrics tests
share.  Written from the definitions -- average precision by a sort over the distinct scores, the consecutive-onset removal as the
reference's sequential loop -- not from the kernels' counting form, so the two check each other.

Scores: the fp32 sigmoid, computed ONCE per distinct logit value (in fp64, rounded to fp32): equal logits then have equal scores whatever
their position.  (torch.sigmoid on the CPU is not position-independent: its vector body and its scalar tail round differently.)"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np

LN3 = math.log(3.0)     # sigmoid(ln 3) = 0.75, the threshold


def sigmoid32(z: np.ndarray) -> np.ndarray:
    z = np.asarray(z, dtype=np.float32)
    vals, inv = np.unique(z.reshape(-1), return_inverse=True)
    s = (1.0 / (1.0 + np.exp(-vals.astype(np.float64)))).astype(np.float32)
    return s[inv].reshape(z.shape)


def balanced_subset(t: np.ndarray) -> Tuple[np.ndarray, int]:
    """Flat indices of the first b positives followed by the first b negatives (row-major), b = min(#pos, #neg)."""
    flat = np.asarray(t).reshape(-1)
    pos, neg = np.nonzero(flat == 1)[0], np.nonzero(flat == 0)[0]
    b = min(pos.size, neg.size)
    return np.concatenate([pos[:b], neg[:b]]), b


def average_precision(t: np.ndarray, s: np.ndarray) -> float:
    """Step-wise AP: over the distinct scores v, descending, (recall(v) - recall(previous)) * precision(v); ties are one threshold."""
    P = int(np.sum(t == 1))
    if P == 0:
        return float("nan")
    ap, prev = 0.0, 0.0
    for v in np.unique(s)[::-1]:
        sel = s >= v
        tp = int(np.sum(t[sel] == 1))
        recall = tp / P
        ap += (recall - prev) * (tp / int(np.sum(sel)))
        prev = recall
    return ap


def onset_num_acc(s: np.ndarray, t: np.ndarray, thr: np.float32) -> float:
    p = (s > thr).astype(int)
    hits = 0
    for i in range(p.shape[0]):
        row = p[i].copy()
        for j in range(row.shape[0] - 1):      # the later frame of an adjacent pair goes, left to right, on the updated row
            if row[j] == 1 and row[j + 1] == 1:
                row[j + 1] = 0
        hits += int(row.sum() == int(np.asarray(t[i]).astype(int).sum()))
    return hits / p.shape[0]


def step_metrics_ref(z: np.ndarray, t: np.ndarray, threshold: float = 0.75) -> Dict[str, float]:
    z, t = np.asarray(z, dtype=np.float32), np.asarray(t, dtype=np.float64)
    assert z.ndim == 2 and z.shape == t.shape
    thr = np.float32(threshold)
    s = sigmoid32(z)
    idx, b = balanced_subset(t)
    ss, ts = s.reshape(-1)[idx], t.reshape(-1)[idx]
    if b == 0:
        ap = acc = float("nan")
    else:
        ap = average_precision(ts, ss)
        acc = int(np.sum((ss > thr).astype(np.float64) == ts)) / (2 * b)
    return {"AP": ap, "Acc": acc, "OnsNumAcc": onset_num_acc(s, t, thr), "b": b}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def grid_logits(rng: np.random.Generator, shape) -> np.ndarray:
    """fp32 logits k / 64, |k| <= 512 (|z| <= 8), none within 1e-2 of ln 3: distinct values have distinct fp32 scores, equal values are ties,
    and no score is near the 0.75 threshold -- ordering, ties and threshold decisions do not depend on the last bits of a sigmoid."""
    k = rng.integers(-512, 513, size=shape)
    z = k / 64.0
    z = np.where(np.abs(z - LN3) < 1e-2, z + 1.0 / 64.0 * 2, z)      # 70 / 64 is 4.9e-3 from ln 3: move it to 72 / 64
    assert not np.any(np.abs(z - LN3) < 1e-2) and np.max(np.abs(z)) <= 8.0 + 1e-9
    return z.astype(np.float32)


def random_labels(rng: np.random.Generator, shape, density: float) -> np.ndarray:
    return (rng.random(shape) < density).astype(np.float32)
