"""Restated oracle of the onset data's training transforms -- TEST INFRASTRUCTURE, torch CPU ops, dtype-generic (fp32 and fp64).

    Resize((rh, rw), antialias=True) -> crop -> ColorJitter -> Normalize -> (C, T, H, W)
    (cfg/data/data-onset-greatesthit-augment.yaml:8-28 applied by main/dataset_onset.py:152-165 to the (T, C, H, W) stack of one clip)

What is pinned and what is not:
  * resize + crop + normalize: PINNED.  ``F.interpolate(mode="bilinear", antialias=True, align_corners=False)`` is the ATen kernel
    torchvision's ``Resize`` calls for tensors (see oracle/frames_ref.py); the crop is a slice, Normalize ``(x - mean) / std``.
  * the colour operations and the order in which random numbers are consumed: UNPINNED.  They are restated from torchvision 0.14.1
    (``transforms/functional_tensor.py``: ``_blend``, ``rgb_to_grayscale``, ``adjust_brightness / contrast / saturation / hue``,
    ``_rgb2hsv``, ``_hsv2rgb``; ``transforms/transforms.py``: ``ColorJitter.forward / get_params``, ``RandomCrop.get_params``), which is
    not installed where this was written.  ``tests/test_frame_transforms_cpu.py::test_oracle_matches_torchvision`` pins it the day it is.

``probe`` (a dict) receives the intermediates the fixture conditions of the GPU tests are asserted on: the hue sector of every pixel
entering ``_hsv2rgb`` and the pre-clamp values of every blend.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def gray(x: torch.Tensor) -> torch.Tensor:
    """rgb_to_grayscale, (..., 3, H, W) -> (..., 1, H, W)"""
    r, g, b = x.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(-3)


def blend(a: torch.Tensor, b: torch.Tensor, f: float, probe: Optional[dict] = None, name: str = "") -> torch.Tensor:
    v = f * a + (1.0 - f) * b
    if probe is not None:
        probe.setdefault("preclamp_" + name, []).append(v)
    return v.clamp(0.0, 1.0)


def rgb2hsv(img: torch.Tensor) -> torch.Tensor:
    r, g, b = img.unbind(dim=-3)
    maxc = torch.max(img, dim=-3).values
    minc = torch.min(img, dim=-3).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    cr_divisor = torch.where(eqc, ones, cr)
    rc = (maxc - r) / cr_divisor
    gc = (maxc - g) / cr_divisor
    bc = (maxc - b) / cr_divisor
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = hr + hg + hb
    h = torch.fmod((h / 6.0 + 1.0), 1.0)
    return torch.stack((h, s, maxc), dim=-3)


def hsv2rgb(img: torch.Tensor, probe: Optional[dict] = None) -> torch.Tensor:
    h, s, v = img.unbind(dim=-3)
    i = torch.floor(h * 6.0)
    f = (h * 6.0) - i
    i = i.to(dtype=torch.int32)
    p = torch.clamp((v * (1.0 - s)), 0.0, 1.0)
    q = torch.clamp((v * (1.0 - s * f)), 0.0, 1.0)
    t = torch.clamp((v * (1.0 - (s * (1.0 - f)))), 0.0, 1.0)
    i = i % 6
    if probe is not None:
        probe.setdefault("hue_sector", []).append(i)
    mask = i.unsqueeze(dim=-3) == torch.arange(6).view(-1, 1, 1)
    a1 = torch.stack((v, q, p, p, t, v), dim=-3)
    a2 = torch.stack((t, v, v, q, p, p), dim=-3)
    a3 = torch.stack((p, p, t, v, v, q), dim=-3)
    a4 = torch.stack((a1, a2, a3), dim=-4)
    return torch.einsum("...ijk, ...xijk -> ...xjk", mask.to(dtype=img.dtype), a4)


def adjust_brightness(x, f, probe=None):
    return blend(x, torch.zeros_like(x), f, probe, "brightness")


def adjust_contrast(x, f, probe=None):
    """x: (T, 3, H, W); the mean runs over the last three dimensions: one value per FRAME"""
    m = torch.mean(gray(x), dim=(-3, -2, -1), keepdim=True)
    return blend(x, m, f, probe, "contrast")


def adjust_saturation(x, f, probe=None):
    return blend(x, gray(x), f, probe, "saturation")


def adjust_hue(x, f, probe=None):
    hsv = rgb2hsv(x)
    h, s, v = hsv.unbind(dim=-3)
    h = (h + f) % 1.0
    return hsv2rgb(torch.stack((h, s, v), dim=-3), probe)


ADJUST = (adjust_brightness, adjust_contrast, adjust_saturation, adjust_hue)


def transform_clip(frames_u8: torch.Tensor, resized_hw: Sequence[int], out_hw: Sequence[int], top: int, left: int, order: Sequence[int],
                   factor: Sequence[float], mask: int, mean=MEAN, std=STD, dtype=torch.float64, probe: Optional[dict] = None) -> torch.Tensor:
    """frames_u8: (T, H, W, 3) uint8 -> (3, T, oh, ow) ``dtype``"""
    x = frames_u8.permute(0, 3, 1, 2).to(dtype) / 255.0                                                        # ToTensor, stacked
    x = F.interpolate(x, size=tuple(resized_hw), mode="bilinear", antialias=True, align_corners=False)         # Resize(antialias=True)
    x = x[..., top: top + out_hw[0], left: left + out_hw[1]]                                                   # crop
    for op in order:                                                                                           # ColorJitter.forward
        if (mask >> int(op)) & 1:
            x = ADJUST[int(op)](x, float(factor[int(op)]), probe)
    m = torch.tensor(mean, dtype=dtype).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=dtype).view(1, 3, 1, 1)
    x = (x - m) / s                                                                                            # Normalize
    return x.permute(1, 0, 2, 3).contiguous()


def transform_batch(frames_u8: torch.Tensor, params, mean=MEAN, std=STD, dtype=torch.float64, probe: Optional[dict] = None) -> torch.Tensor:
    """frames_u8: (N, T, H, W, 3) uint8, params: ``frame_transforms.ClipParams`` -> (N, 3, T, oh, ow)"""
    return torch.stack([transform_clip(frames_u8[n], params.resized_hw, params.out_hw, int(params.top[n]), int(params.left[n]),
                                       params.order[n].tolist(), params.factor[n].tolist(), int(params.mask[n]), mean, std, dtype, probe)
                        for n in range(frames_u8.shape[0])])


def make_frames(N: int, T: int, H: int, W: int, seed: int = 0) -> torch.Tensor:
    """Test frames (N, T, H, W, 3) uint8 that exercise the colour operations (uniform noise would not: the antialiased resize turns it
    into mid-gray).  Four horizontal bands: a full-saturation hue sweep (all six hue sectors), saturated colour blocks with pure black
    and white among them, a black-to-white gradient with mild texture, and a black | white split.  Every frame is shifted along x."""
    g = torch.Generator().manual_seed(seed)
    xs = torch.arange(W, dtype=torch.float64) / W
    h6 = xs * 6.0
    sweep = torch.stack([(h6 - 3.0).abs() - 1.0, 2.0 - (h6 - 2.0).abs(), 2.0 - (h6 - 4.0).abs()], dim=-1).clamp(0.0, 1.0)   # HSV(h, 1, 1)
    blocks = torch.tensor([[255, 0, 0], [0, 0, 0], [0, 255, 0], [255, 255, 255], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]],
                          dtype=torch.float64)
    out = torch.zeros(N, T, H, W, 3, dtype=torch.uint8)
    b0, b1, b2 = H // 4, H // 2, 3 * H // 4
    for n in range(N):
        for t in range(T):
            img = torch.zeros(H, W, 3, dtype=torch.float64)
            img[:b0] = sweep[None] * 255.0
            img[:b0] *= 0.75 + 0.25 * torch.rand(b0, W, 1, generator=g, dtype=torch.float64)
            img[b0:b1] = blocks[(torch.arange(W) * 8 // W)][None]
            img[b1:b2] = (xs * 255.0)[None, :, None] + 24.0 * (torch.rand(b2 - b1, W, 3, generator=g, dtype=torch.float64) - 0.5)
            img[b2:, : W // 2] = 0.0
            img[b2:, W // 2:] = 255.0
            shift = (13 * t + 29 * n + seed) % W
            out[n, t] = torch.roll(img, shifts=shift, dims=1).round().clamp(0, 255).to(torch.uint8)
    return out
