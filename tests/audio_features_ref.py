"""fp64 / numpy restatement of the audio front end (syncfusion_amd/csrc/audio_features.hip) and of the onset-sync evaluation
(syncfusion_amd/evaluation.py), with the inputs their tests share.  Written from the definitions -- an explicit loop over frames and
``numpy.fft.rfft``, filters evaluated triangle by triangle, the reference's list handling simulated step by step -- not from the kernels'
or the product's form, so the two check each other.  No torch op takes part in the arithmetic.

The specification restated here (script/evaluate_onset.py:30 -> librosa.onset.onset_detect) is UNPINNED: librosa is not available, see
syncfusion_amd/audio_features.py.  What pins the framing, padding and window is ``torch.stft`` in fp64 (tests/test_audio_features_cpu.py).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from onset_metrics_ref import average_precision

FLT_MIN = float(np.finfo(np.float32).tiny)


# ---- STFT power ----------------------------------------------------------------------------------------------------------------------------
def pad_center(x: np.ndarray, n_fft: int, pad_mode: str) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    p = n_fft // 2
    if pad_mode == "constant":
        return np.concatenate([np.zeros(p), x, np.zeros(p)])
    if pad_mode == "reflect":
        assert x.size > p, "reflect padding needs more than n_fft / 2 samples"
        return np.concatenate([x[1:p + 1][::-1], x, x[-p - 1:-1][::-1]])
    raise ValueError(pad_mode)


def hann_periodic(n: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def stft_power(x: np.ndarray, n_fft: int, hop: int, pad_mode: str) -> np.ndarray:
    """(L,) -> (n_fft // 2 + 1, T) fp64, T = 1 + L // hop."""
    xp = pad_center(x, n_fft, pad_mode)
    T = 1 + len(x) // hop
    w = hann_periodic(n_fft)
    out = np.empty((n_fft // 2 + 1, T))
    for t in range(T):
        out[:, t] = np.abs(np.fft.rfft(xp[t * hop:t * hop + n_fft] * w)) ** 2
    return out


# ---- mel filterbank, triangle by triangle --------------------------------------------------------------------------------------------------
def hz_to_mel_ref(f: float, scale: str) -> float:
    if scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return f / (200.0 / 3.0) if f < 1000.0 else 15.0 + np.log(f / 1000.0) / (np.log(6.4) / 27.0)


def mel_to_hz_ref(m: float, scale: str) -> float:
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return m * (200.0 / 3.0) if m < 15.0 else 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0))


def mel_filterbank_ref(sr: float, n_fft: int, n_mels: int, fmin: float, fmax: float, scale: str, norm: Optional[str]) -> np.ndarray:
    lo, hi = hz_to_mel_ref(fmin, scale), hz_to_mel_ref(fmax, scale)
    f = [mel_to_hz_ref(lo + (hi - lo) * i / (n_mels + 1), scale) for i in range(n_mels + 2)]
    fb = np.zeros((n_mels, n_fft // 2 + 1))
    for m in range(n_mels):
        for k in range(n_fft // 2 + 1):
            fk = k * sr / n_fft
            if f[m] < fk <= f[m + 1]:
                fb[m, k] = (fk - f[m]) / (f[m + 1] - f[m])
            elif f[m + 1] < fk < f[m + 2]:
                fb[m, k] = (f[m + 2] - fk) / (f[m + 2] - f[m + 1])
        if norm == "slaney":
            fb[m] *= 2.0 / (f[m + 2] - f[m])
    return fb


# ---- dB, envelope, peaks -------------------------------------------------------------------------------------------------------------------
def power_to_db(P: np.ndarray, amin: float = 1e-10, top_db: float = 80.0) -> np.ndarray:
    db = 10.0 * np.log10(np.maximum(amin, P))
    return np.maximum(db, db.max() - top_db)


def onset_envelope(db: np.ndarray, n_fft: int, hop: int, lag: int = 1) -> np.ndarray:
    """(n_mels, T) dB -> (T,): lag + n_fft // (2 hop) zero frames, then mean_m max(0, dB[m, t] - dB[m, t - lag]) for t = lag ..., cut to T."""
    T = db.shape[1]
    d = np.maximum(0.0, db[:, lag:] - db[:, :-lag]).mean(axis=0) if T > lag else np.zeros(0)
    return np.concatenate([np.zeros(lag + n_fft // (2 * hop)), d])[:T]


def normalise(e: np.ndarray) -> np.ndarray:
    e = e - e.min()
    return e / (e.max() + FLT_MIN)


def peak_pick(e: np.ndarray, pre_max: int, post_max: int, pre_avg: int, post_avg: int, wait: int, delta: float) -> Tuple[List[int], float]:
    """-> (onset frames, the smallest decision margin in normalised-envelope units).  A frame's decision is `window maximum AND above
    mean + delta`; its margin is how far x would have to move for that decision to flip: a = distance to the largest OTHER value of the max
    window, b = |x[n] - mean - delta|;  maximum and above: min(a, b);  maximum, not above: b;  above, not maximum: a;  neither: max(a, b)."""
    e = np.asarray(e, dtype=np.float64)
    T = e.size
    if not e.any():
        return [], float("inf")
    x = normalise(e)
    flags, margin = [], float("inf")
    for n in range(T):
        lo, hi = max(0, n - pre_max), min(T, n + post_max)
        others = np.delete(x[lo:hi], n - lo)
        is_max = bool(x[n] == x[lo:hi].max())
        a = abs(x[n] - others.max()) if others.size else float("inf")
        mean = x[max(0, n - pre_avg):min(T, n + post_avg)].mean()
        above = bool(x[n] >= mean + delta)
        b = abs(x[n] - mean - delta)
        margin = min(margin, (min(a, b) if above else b) if is_max else (a if above else max(a, b)))
        flags.append(is_max and above)
    onsets, last = [], None
    for n in range(T):
        if flags[n] and (last is None or n - last > wait):
            onsets.append(n)
            last = n
    return onsets, margin


def confidences(wav: np.ndarray, onsets: Sequence[int], ci: int) -> Tuple[np.ndarray, np.ndarray]:
    """w = (|wav| - min) / (max - min);  -> (max of w over [o - ci, o + ci) clipped to the clip, w[o] (0 where o == len(wav)))."""
    a = np.abs(np.asarray(wav, dtype=np.float64))
    w = (a - a.min()) / (a.max() - a.min())
    L = a.size
    conf = np.array([w[max(0, o - ci):min(L, o + ci)].max() for o in onsets], dtype=np.float64)
    strength = np.array([w[o] if o < L else 0.0 for o in onsets], dtype=np.float64)
    return conf, strength


def detect(wav: np.ndarray, fb: np.ndarray, n_fft: int, hop: int, pad_mode: str, delta: float, pre_max: int, post_max: int, pre_avg: int,
           post_avg: int, wait: int, lag: int = 1, ci: int = 1102, amin: float = 1e-10, top_db: float = 80.0) -> Dict[str, object]:
    """The whole detector on one fp32 clip, in fp64."""
    P = fb @ stft_power(wav, n_fft, hop, pad_mode)
    db = power_to_db(P, amin, top_db)
    env = onset_envelope(db, n_fft, hop, lag)
    frames, margin = peak_pick(env, pre_max, post_max, pre_avg, post_avg, wait, delta)
    onsets = [n * hop for n in frames]
    conf, strength = confidences(wav, onsets, ci) if onsets else (np.zeros(0), np.zeros(0))
    return {"mel": P, "db": db, "env": env, "onsets": np.asarray(onsets, dtype=np.int64), "margin": margin, "confidence": conf, "strength": strength}


# ---- evaluation (script/evaluate_onset.py:35-93, 159-191) ----------------------------------------------------------------------------------
def nms_ref(onsets: Sequence[int], conf: Sequence[float], window: float = 0.05, sr: int = 22050) -> List[int]:
    """The reference walks its list of remaining onsets with a running index while deleting from it: after a deletion the element that
    slides into the freed slot is never looked at in that pass.  Simulated with the index spelled out."""
    remaining = [int(o) for o in onsets]
    order = np.argsort(np.asarray(conf, dtype=np.float64), kind="stable")[::-1]
    out = []
    for idx in order:
        cur = int(onsets[idx])
        if cur not in remaining:
            continue
        out.append(cur)
        del remaining[remaining.index(cur)]
        i = 0
        while i < len(remaining):
            o = remaining[i]
            i += 1                                   # the running index moves on before the deletion ...
            if abs(cur - o) < window * sr:
                del remaining[i - 1]                 # ... so what slides into slot i - 1 is skipped
    return sorted(out)


def match_ref(tar: Sequence[int], gen: Sequence[int], conf: Dict[int, float], strength: Dict[int, float], delta: float,
              sr: int = 22050) -> Tuple[float, float, List[int]]:
    """-> (acc, ap, hit flag per generated onset after NMS).  conf / strength: by onset position.  AP NaN (no positive) stays NaN here."""
    kept = nms_ref(gen, [conf[int(o)] for o in gen], sr=sr)
    free = list(kept)
    res = [0] * len(kept)
    hits, y, s = 0, [], []
    for o in tar:
        cand = [g for g in free if abs(g - o) < delta * sr]
        if not cand:
            y.append(1)
            s.append(0.0)
            continue
        best = max(range(len(cand)), key=lambda i: (strength[cand[i]], i))      # the highest strength, the later one on a tie
        g = cand[best]
        hits += 1
        y.append(1)
        s.append(conf[g])
        res[kept.index(g)] = 1
        free.remove(g)
        if not free:
            break
    for g in free:
        y.append(0)
        s.append(conf[g])
    acc = hits / len(tar) if len(tar) else 0.0
    ap = average_precision(np.asarray(y), np.asarray(s, dtype=np.float64)) if y else float("nan")
    return acc, ap, res


def evaluate_ref(gen: Dict[str, Dict[str, np.ndarray]], tar: Dict[str, Dict[str, np.ndarray]], delta: float = 0.1,
                 remove_head: Optional[float] = None, multi_delta: bool = False, sr: int = 22050) -> Dict[str, object]:
    """gen / tar: file name -> {"onsets", "confidence", "strength"} (arrays by onset).  The per-file rules of :159-191; a file whose AP is
    undefined (no positive / nothing to score, where the reference would raise) counts 0."""
    counts, accs, aps, per_file = [], [], [], {}
    for name, g in gen.items():
        t = tar.get(name)
        o1 = [int(o) for o in t["onsets"]] if t is not None else []
        o2 = [int(o) for o in g["onsets"]]
        if not o1 or not o2:
            row = (False, 0.0, 0.0)
        else:
            conf = {int(o): float(c) for o, c in zip(g["onsets"], g["confidence"])}
            strength = {int(o): float(c) for o, c in zip(g["onsets"], g["strength"])}
            if remove_head is not None:
                o1 = [o for o in o1 if o >= remove_head * sr]
                o2 = [o for o in o2 if o >= remove_head * sr]
            deltas = list(np.arange(0.1, delta + 0.05, 0.05)) if multi_delta else [delta]
            acc = ap = 0.0
            for d in deltas:
                a, p, _ = match_ref(o1, o2, conf, strength, d, sr)
                acc += a
                ap += 0.0 if np.isnan(p) else p
            row = (len(o1) == len(o2), acc / len(deltas), ap / len(deltas))
        counts.append(row[0]), accs.append(row[1]), aps.append(row[2])
        per_file[name] = {"count_match": row[0], "acc": row[1], "ap": row[2], "n_tar": len(o1), "n_gen": len(o2)}
    return {"onset_num_acc": float(np.mean(counts)), "detection_acc": float(np.mean(accs)), "detection_ap": float(np.mean(aps)), "per_file": per_file}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
SR = 22050
KINDS = ("bursts", "tone", "gated", "quiet_bursts", "clicks", "zeros")


def burst_clip(rng: np.random.Generator, L: int, positions: Optional[Sequence[int]] = None, floor: float = 1e-3) -> np.ndarray:
    """a noise floor plus exponentially decaying noise bursts: 1-5 at random positions (or at `positions`), amplitude 0.2-1.0, decay 200-800"""
    x = floor * rng.standard_normal(L)
    if positions is None:
        positions = rng.integers(0, max(1, L - 1), size=int(rng.integers(1, 6)))
    for p in positions:
        n = np.arange(L - int(p))
        x[int(p):] += rng.uniform(0.2, 1.0) * np.exp(-n / rng.uniform(200.0, 800.0)) * rng.standard_normal(n.size)
    return x


def make_input(kind: str, B: int, L: int, seed: int = 0) -> np.ndarray:
    """(B, L) fp32.  Clip i is the same whatever B is (one generator per clip)."""
    out = np.zeros((B, L), dtype=np.float64)
    t = np.arange(L) / SR
    for i in range(B):
        rng = np.random.default_rng([seed, KINDS.index(kind), i, L])
        if kind == "bursts":
            out[i] = burst_clip(rng, L)
        elif kind == "quiet_bursts":                 # the amin floor (-100 dB) lies inside the 80 dB range below the maximum
            out[i] = 1e-4 * burst_clip(rng, L)
        elif kind == "tone":                         # 440 Hz switched on at 0.3 s over a 1e-4 floor
            out[i] = 1e-4 * rng.standard_normal(L) + np.where(t >= 0.3, 0.5 * np.sin(2 * np.pi * 440.0 * t), 0.0)
        elif kind == "gated":                        # 3 kHz and 7000.5 Hz, gated at 3 Hz, over a 1e-5 floor
            gate = (np.sin(2 * np.pi * 3.0 * t + 0.3 * i) > 0).astype(np.float64)
            out[i] = 1e-5 * rng.standard_normal(L) + gate * (0.4 * np.sin(2 * np.pi * 3000.0 * t) + 0.3 * np.sin(2 * np.pi * 7000.5 * t))
        elif kind == "clicks":                       # digital silence with two single-sample clicks
            for p in rng.choice(L, size=2, replace=False):
                out[i, p] = rng.uniform(0.3, 1.0)
        elif kind != "zeros":
            raise ValueError(kind)
    return out.astype(np.float32)
