"""fp64 reference of the FAD evaluation for the tests: numpy / torch only, no import of the product.

Restates the pipeline of syncfusion_amd/fad.py independently: uncentred framing + ``np.fft.rfft`` + the mel matrix + log, the layer stack
with ``torch.nn.functional.conv2d / max_pool2d / linear`` in fp64, ``np.cov`` and the Fréchet distance (``scipy.linalg.sqrtm`` when scipy
imports, as the upstream package computes it, on covariances of full rank; the nuclear-norm form of the same trace otherwise).
Plain module, not a conftest: the tests import it like numerics.py.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

SR, WIN, HOP, N_FFT, N_MELS, FRAMES = 16000, 400, 160, 512, 64, 96
MEL_LO, MEL_HI, LOG_OFFSET = 125.0, 7500.0, 0.01
FULL_LAYOUT = (64, "M", 128, "M", 256, 256, "M", 512, 512, "M")
FULL_FC = (4096, 4096, 128)
NARROW_LAYOUT = (8, "M", 12, "M", 20, 20, "M", 36, 36, "M")      # channel counts that are no multiples of 8: the padded-column paths
NARROW_FC = (96, 64, 24)


def hz_to_mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_matrix() -> np.ndarray:
    """(257, 64) fp64, written as loops over the bands (the product vectorises)."""
    bins = N_FFT // 2 + 1
    m = hz_to_mel(np.arange(bins) * (SR / 2.0) / (bins - 1))
    edges = np.linspace(hz_to_mel(MEL_LO), hz_to_mel(MEL_HI), N_MELS + 2)
    w = np.zeros((bins, N_MELS))
    for i in range(N_MELS):
        lo, c, up = edges[i], edges[i + 1], edges[i + 2]
        w[:, i] = np.maximum(0.0, np.minimum((m - lo) / (c - lo), (up - m) / (up - c)))
    w[0, :] = 0.0
    return w


def frame_count(L: int) -> int:
    return 0 if L < WIN else 1 + (L - WIN) // HOP


def example_count(L: int) -> int:
    return frame_count(L) // FRAMES


def mel_magnitude(wav: np.ndarray) -> np.ndarray:
    """(B, L) -> (B, F, 64) fp64: every frame of the clip (the caller cuts the examples)."""
    wav = np.asarray(wav, dtype=np.float64)
    B, L = wav.shape
    nf = frame_count(L)
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WIN) / WIN)
    idx = HOP * np.arange(nf)[:, None] + np.arange(WIN)[None, :]
    frames = wav[:, idx] * window                                        # (B, F, 400)
    spec = np.abs(np.fft.rfft(frames, n=N_FFT, axis=-1))                 # zero-padded at the end to 512
    return spec @ mel_matrix()


def examples(wav: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(B, L) -> ((B, E, 96, 64) log-mel examples, (B, E * 96, 64) mel magnitudes of the frames they hold), fp64."""
    mel = mel_magnitude(wav)
    E = mel.shape[1] // FRAMES
    mel = mel[:, :E * FRAMES]
    return np.log(mel + LOG_OFFSET).reshape(mel.shape[0], E, FRAMES, N_MELS), mel


def seeded_weights(layout: Sequence, fc: Sequence[int], seed: int) -> Dict[str, torch.Tensor]:
    """fp32 state dict with torchvggish's names from a seeded CPU generator: Kaiming-uniform weights as nn.Conv2d / nn.Linear draw them
    (bound 1 / sqrt(fan_in)), biases uniform in +-0.1 so that the bias path is visible."""
    g = torch.Generator().manual_seed(seed)
    state: Dict[str, torch.Tensor] = {}
    idx, c, h, w = 0, 1, FRAMES, N_MELS
    for v in layout:
        if v == "M":
            idx += 1
            h, w = h // 2, w // 2
            continue
        bound = 1.0 / np.sqrt(c * 9)
        state[f"features.{idx}.weight"] = (torch.rand((int(v), c, 3, 3), generator=g) * 2 - 1) * bound
        state[f"features.{idx}.bias"] = (torch.rand((int(v),), generator=g) * 2 - 1) * 0.1
        idx += 2
        c = int(v)
    k = h * w * c
    for i, n in enumerate(fc):
        bound = 1.0 / np.sqrt(k)
        state[f"embeddings.{2 * i}.weight"] = (torch.rand((int(n), k), generator=g) * 2 - 1) * bound
        state[f"embeddings.{2 * i}.bias"] = (torch.rand((int(n),), generator=g) * 2 - 1) * 0.1
        k = int(n)
    return state


def network(state: Dict[str, torch.Tensor], layout: Sequence, fc: Sequence[int], ex: torch.Tensor, final_relu: bool = False):
    """(N, 96, 64) examples -> ((N, D) embeddings, [the tensor after each pool as (N, h, w, C)]) in fp64."""
    P = {k: v.double() for k, v in state.items()}
    x = ex.double()[:, None]                                              # (N, 1, 96, 64)
    pools: List[torch.Tensor] = []
    idx = 0
    for v in layout:
        if v == "M":
            x = F.max_pool2d(x, 2, 2)
            pools.append(x.permute(0, 2, 3, 1).contiguous())
            idx += 1
        else:
            x = F.relu(F.conv2d(x, P[f"features.{idx}.weight"], P[f"features.{idx}.bias"], padding=1))
            idx += 2
    x = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)                     # torchvggish: NCHW -> NHWC, then flatten
    for i in range(len(fc)):
        x = F.linear(x, P[f"embeddings.{2 * i}.weight"], P[f"embeddings.{2 * i}.bias"])
        if i + 1 < len(fc) or final_relu:
            x = F.relu(x)
    return x, pools


def statistics(emb) -> Tuple[np.ndarray, np.ndarray]:
    e = np.asarray(emb, dtype=np.float64)
    return e.mean(axis=0), np.cov(e, rowvar=False)


def frechet_sqrtm(mu1, s1, mu2, s2) -> float:
    """The upstream formula: tr sqrtm(s1 s2) by scipy (ImportError without scipy: the caller skips)."""
    from scipy import linalg

    root = linalg.sqrtm(np.asarray(s1, dtype=np.float64) @ np.asarray(s2, dtype=np.float64))
    d = np.asarray(mu1, dtype=np.float64) - np.asarray(mu2, dtype=np.float64)
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * np.trace(np.real(root)))


def _factor(s: np.ndarray) -> np.ndarray:
    lam, q = np.linalg.eigh(0.5 * (s + s.T))
    keep = lam > lam.max() * lam.size * np.finfo(np.float64).eps
    return q[:, keep] * np.sqrt(lam[keep])


def frechet(mu1, s1, mu2, s2) -> float:
    """The Fréchet distance of two Gaussians.  With scipy and two covariances of full numerical rank: ``frechet_sqrtm``, the upstream
    formula.  Otherwise (fewer samples than dimensions, where sqrtm of the singular product is only good to ~8e-9 of the traces: its
    zero eigenvalues come back as sqrt(1e-16)) the same trace as a nuclear norm: tr sqrtm(s1 s2) = sum of the singular values of
    R1^T R2 with Ri Ri^T = si, which an SVD gives to machine precision.  Not the product's route (eigenvalues of a symmetrised
    product)."""
    s1, s2 = np.asarray(s1, dtype=np.float64), np.asarray(s2, dtype=np.float64)
    r1, r2 = _factor(s1), _factor(s2)
    if r1.shape[1] == s1.shape[0] and r2.shape[1] == s2.shape[0]:
        try:
            return frechet_sqrtm(mu1, s1, mu2, s2)
        except ImportError:
            pass
    d = np.asarray(mu1, dtype=np.float64) - np.asarray(mu2, dtype=np.float64)
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * np.linalg.svd(r1.T @ r2, compute_uv=False).sum())


def clip_signal(B: int, L: int, seed: int) -> torch.Tensor:
    """Noise plus two decaying sinusoids, amplitude <= 1, fp32 (B, L)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(L, dtype=torch.float64) / SR
    rows = []
    for b in range(B):
        x = 0.1 * torch.randn(L, generator=g, dtype=torch.float64)
        x += 0.5 * torch.exp(-3.0 * t) * torch.sin(2 * np.pi * (440.0 + 60.0 * b) * t)
        x += 0.3 * torch.exp(-1.0 * t) * torch.sin(2 * np.pi * (2500.0 + 310.0 * b) * t + 0.7)
        rows.append(x / max(1.0, float(x.abs().max())))
    return torch.stack(rows).float()

