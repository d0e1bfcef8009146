"""CPU restatement of the inpainting sampler (syncfusion_amd/csrc/sampler.hip, sf_vinpaint): the counter-based normals in numpy --
Philox4x32-10 on integers, then Box-Muller in fp64 -- and ``VInpainter``'s loop ([RECALLED, UNPINNED]) over the oracle
U-Net, written the way upstream writes it: two nested Python loops, ``torch.where``.  It shares no code with the product.

The loop takes ``noise_fn(k)`` for the draw of virtual iteration k = i * num_resamples + r, so that a parity test can feed it the very
normals the device used (``syncfusion_amd.diffusion.philox_normal``) and the transcendental rounding is tested once, on its own.
"""
from __future__ import annotations

import math
from typing import Callable

import numpy as np
import torch

Tensor = torch.Tensor

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

# Philox4x32-10 known answers (counter, key, output)
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((MASK32,) * 4, (MASK32,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


# the 2**20 draws whose mean and variance the GPU test gates (tests/test_inpaint_cpu.py checks that this seed's fp64 draws lie inside)
STAT_SEED = (0x5EED << 32) | 0x1234ABCD
STAT_N = 1 << 20
MEAN_GATE, VAR_GATE = 3.9e-3, 5.5e-3      # four standard errors: 4 / sqrt(n) and 4 * sqrt(2 / n)


def philox4x32_10(counter, key):
    """counter: four uint64 arrays (values < 2**32) of one shape, key: two ints -> four uint64 arrays (values < 2**32)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in counter)
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    m32 = np.uint64(MASK32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0           # < 2**64: both factors are below 2**32
        p1 = np.uint64(PHILOX_M1) * c2
        hi0, lo0 = p0 >> s32, p0 & m32
        hi1, lo1 = p1 >> s32, p1 & m32
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return c0, c1, c2, c3


def philox_words(seed: int, k: int, elem_offset: int, n: int) -> np.ndarray:
    """The integer draws behind elements [elem_offset, elem_offset + n): (groups, 4) uint64 and the first group's index."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    g_lo, g_hi = elem_offset >> 2, (elem_offset + n + 3) >> 2
    g = np.arange(g_lo, g_hi, dtype=np.uint64)
    zero = np.zeros_like(g)
    r = philox4x32_10((g & np.uint64(MASK32), g >> np.uint64(32), zero + np.uint64(k), zero), (seed & MASK32, seed >> 32))
    return np.stack(r, axis=1)


def unit_open(w: np.ndarray) -> np.ndarray:
    """u(w) = ((w >> 9) + 0.5) * 2**-23 in fp64 (exact, and exact in fp32 too)."""
    return ((w >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def philox_normal(seed: int, k: int, elem_offset: int, n: int) -> np.ndarray:
    """fp64 normals of elements [elem_offset, elem_offset + n) at virtual iteration k."""
    r = philox_words(seed, k, elem_offset, n)
    z = np.empty((r.shape[0], 4), dtype=np.float64)
    for a in (0, 2):
        rho = np.sqrt(-2.0 * np.log(unit_open(r[:, a])))
        th = 2.0 * math.pi * unit_open(r[:, a + 1])
        z[:, a], z[:, a + 1] = rho * np.cos(th), rho * np.sin(th)
    first = elem_offset - ((elem_offset >> 2) << 2)
    return z.reshape(-1)[first:first + n]


def vinpaint(net: Callable[[Tensor, Tensor], Tensor], source: Tensor, mask: Tensor, num_steps: int, num_resamples: int, x_noisy: Tensor,
             noise_fn: Callable[[int], Tensor]) -> Tensor:
    """VInpainter.forward.  ``net(x, sigma_b)`` -> v; ``mask`` bool, True = keep the source; ``noise_fn(k)``: the
    ``randn_like(source)`` of virtual iteration k."""
    B = source.shape[0]
    sigmas = torch.linspace(1.0, 0.0, num_steps + 1, dtype=torch.float32)
    angle = sigmas * (math.pi / 2.0)
    alphas, betas = torch.cos(angle), torch.sin(angle)
    mask = torch.broadcast_to(mask, source.shape)
    x = x_noisy
    for i in range(num_steps):
        for r in range(num_resamples):
            v = net(x, sigmas[i].expand(B))
            x_pred = alphas[i] * x - betas[i] * v
            noise_pred = betas[i] * x + alphas[i] * v
            j = 1 if r == num_resamples - 1 else 0          # re-noise to the SAME level while resampling
            x = alphas[i + j] * x_pred + betas[i + j] * noise_pred
            s_noisy = alphas[i + j] * source + betas[i + j] * noise_fn(i * num_resamples + r)
            x = torch.where(mask, s_noisy, x)
    return x
