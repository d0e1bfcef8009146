"""The onset data's frame transforms on the device: what ``cfg/data/data-onset-greatesthit-augment.yaml:8-52`` configures for training
(``Resize(128, antialias) -> RandomCrop(112) -> ColorJitter(0.4, 0.2, 0.4, 0.1) -> Normalize``; variants in
main/datamodule_onset.py:138-156) and main/dataset_onset.py:152-165 applies to the ``(T, C, H, W)`` stack of one clip.

The classes carry torchvision 0.14.1's names and constructor arguments so that the reference's YAML instantiates unchanged
(``config.instantiate`` maps ``torchvision.transforms.*`` here), but they are *descriptions*: only ``Compose`` computes, and it does so
for a whole batch of decoded uint8 frames in one launch sequence of the HIP library (``sf_frames_augment``: resize + crop as one gather,
the colour operations per clip in its own random order, Normalize, ``(C, T, H, W)`` layout).  The random draws stay on the host:
``Compose.sample`` consumes a ``torch.Generator`` in the order torchvision does for one clip after the other (``RandomCrop.get_params``:
two ``randint``; ``ColorJitter.get_params``: ``randperm(4)``, then one ``uniform_`` per operation that is present).

There is no CPU execution path: calling a ``Compose`` on a CPU tensor raises, like every other entry point of the package.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import _lib
from ._lib import SyncFusionAmdError

Tensor = torch.Tensor
OPS = ("brightness", "contrast", "saturation", "hue")   # ColorJitter.forward's fn_id 0..3


def _pair(size, what: str) -> Tuple[int, int]:
    """torchvision's ``_setup_size``: an int or a 1-sequence is a square, a 2-sequence is (h, w)."""
    if isinstance(size, numbers.Integral) and not isinstance(size, bool):
        return int(size), int(size)
    if isinstance(size, (list, tuple)) and len(size) == 1:
        return int(size[0]), int(size[0])
    if isinstance(size, (list, tuple)) and len(size) == 2:
        return int(size[0]), int(size[1])
    raise ValueError(f"{what}: size must be an int or a sequence of one or two ints, got {size!r}")


class Resize:
    """``Resize(size, interpolation, max_size, antialias)``.  An int (or 1-sequence) sets the SHORTER edge and keeps the aspect ratio
    (the longer edge becomes ``int(size * long / short)``); a pair is ``(h, w)``."""

    def __init__(self, size, interpolation="bilinear", max_size=None, antialias=None):
        if isinstance(size, numbers.Integral) and not isinstance(size, bool):
            self.size: Union[int, Tuple[int, int]] = int(size)
        elif isinstance(size, (list, tuple)) and len(size) == 1:
            self.size = int(size[0])
        elif isinstance(size, (list, tuple)) and len(size) == 2:
            self.size = (int(size[0]), int(size[1]))
        else:
            raise TypeError(f"Resize: size must be an int or a sequence of one or two ints, got {size!r}")
        if min(self.size if isinstance(self.size, tuple) else (self.size,)) < 1:
            raise ValueError(f"Resize: size must be positive, got {size!r}")
        self.interpolation = getattr(interpolation, "value", interpolation)
        self.max_size = max_size
        self.antialias = antialias

    def output_size(self, in_hw: Sequence[int]) -> Tuple[int, int]:
        h, w = int(in_hw[0]), int(in_hw[1])
        if isinstance(self.size, tuple):
            return self.size
        short, long = (w, h) if w <= h else (h, w)
        new_short, new_long = self.size, int(self.size * long / short)
        return (new_long, new_short) if w <= h else (new_short, new_long)

    def __repr__(self):
        return f"Resize(size={self.size}, interpolation={self.interpolation}, max_size={self.max_size}, antialias={self.antialias})"


class RandomCrop:
    def __init__(self, size, padding=None, pad_if_needed=False, fill=0, padding_mode="constant"):
        self.size = _pair(size, "RandomCrop")
        self.padding, self.pad_if_needed, self.fill, self.padding_mode = padding, pad_if_needed, fill, padding_mode

    def __repr__(self):
        return f"RandomCrop(size={self.size}, padding={self.padding}, pad_if_needed={self.pad_if_needed})"


class CenterCrop:
    def __init__(self, size):
        self.size = _pair(size, "CenterCrop")

    def __repr__(self):
        return f"CenterCrop(size={self.size})"


class ColorJitter:
    """Strengths as torchvision reads them (``ColorJitter._check_input``): a number ``v`` means ``[center - v, center + v]`` (floored at 0
    for brightness, contrast and saturation), a pair is the range itself; hue lies within ``[-0.5, 0.5]``.  A range that collapses to the
    neutral value makes the operation ABSENT (``None``): it is not applied and draws no random number."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        self.brightness = self._check(brightness, "brightness")
        self.contrast = self._check(contrast, "contrast")
        self.saturation = self._check(saturation, "saturation")
        self.hue = self._check(hue, "hue", center=0.0, bound=(-0.5, 0.5), clip_first_on_zero=False)

    @staticmethod
    def _check(value, name, center=1.0, bound=(0.0, float("inf")), clip_first_on_zero=True) -> Optional[Tuple[float, float]]:
        if isinstance(value, numbers.Number) and not isinstance(value, bool):
            if value < 0:
                raise ValueError(f"If {name} is a single number, it must be non negative.")
            value = [center - float(value), center + float(value)]
            if clip_first_on_zero:
                value[0] = max(value[0], 0.0)
        elif isinstance(value, (tuple, list)) and len(value) == 2:
            value = [float(value[0]), float(value[1])]
        else:
            raise TypeError(f"{name} should be a single number or a list/tuple with length 2.")
        if not (bound[0] <= value[0] <= value[1] <= bound[1]):   # (false for NaN as well)
            raise ValueError(f"{name} values should be between {bound}, got {value}")
        if value[0] == value[1] == center:
            return None
        return (value[0], value[1])

    def ranges(self) -> List[Optional[Tuple[float, float]]]:
        return [self.brightness, self.contrast, self.saturation, self.hue]

    def __repr__(self):
        return f"ColorJitter(brightness={self.brightness}, contrast={self.contrast}, saturation={self.saturation}, hue={self.hue})"


class Normalize:
    def __init__(self, mean, std, inplace=False):
        self.mean = tuple(float(v) for v in mean)
        self.std = tuple(float(v) for v in std)
        if len(self.mean) != 3 or len(self.std) != 3:
            raise ValueError(f"Normalize: mean and std must have 3 entries (RGB), got {mean!r} / {std!r}")
        if not all(math.isfinite(v) for v in self.mean) or not all(math.isfinite(v) and v > 0 for v in self.std):
            raise ValueError(f"Normalize: mean must be finite and std positive, got {mean!r} / {std!r}")
        self.inplace = inplace

    def __repr__(self):
        return f"Normalize(mean={self.mean}, std={self.std})"


@dataclass
class ClipParams:
    """Per-clip parameters of one batch (host tensors): what ``Compose.sample`` draws and ``sf_frames_augment`` reads."""
    resized_hw: Tuple[int, int]
    out_hw: Tuple[int, int]
    top: Tensor       # (N) int32, crop origin in the resized frame
    left: Tensor      # (N) int32
    order: Tensor     # (N, 4) int32, a permutation of 0..3 per clip (OPS)
    factor: Tensor    # (N, 4) float32, indexed by operation
    mask: Tensor      # (N) int32, bit op set: the operation is applied

    def __len__(self) -> int:
        return int(self.top.numel())

    def table(self) -> Tensor:
        """``(N, 12)`` int32 host tensor laid out as ``sf_augment_clip`` (the factors as their bit patterns)."""
        n = len(self)
        t = torch.zeros(n, 12, dtype=torch.int32)
        t[:, 0] = self.top.to(torch.int32)
        t[:, 1] = self.left.to(torch.int32)
        t[:, 2:6] = self.order.to(torch.int32).reshape(n, 4)
        t[:, 6:10] = self.factor.to(torch.float32).reshape(n, 4).contiguous().view(torch.int32)
        t[:, 10] = self.mask.to(torch.int32)
        return t

    def select(self, idx) -> "ClipParams":
        idx = torch.as_tensor(idx, dtype=torch.long).reshape(-1)
        return ClipParams(self.resized_hw, self.out_hw, self.top[idx].clone(), self.left[idx].clone(), self.order[idx].clone(),
                          self.factor[idx].clone(), self.mask[idx].clone())


class Compose:
    """``Resize -> [RandomCrop | CenterCrop] -> [ColorJitter] -> Normalize`` (the evaluation chain ``Resize -> Normalize`` included):
    the only shapes the reference's onset configurations use, and the only ones the kernel implements."""

    def __init__(self, transforms: Sequence):
        ts = list(transforms)
        known = (Resize, RandomCrop, CenterCrop, ColorJitter, Normalize)
        for i, t in enumerate(ts):
            if not isinstance(t, known):
                raise SyncFusionAmdError(f"Compose: entry {i} ({t!r}) is not one of Resize, RandomCrop, CenterCrop, ColorJitter, Normalize")
        shape = "Resize -> [RandomCrop | CenterCrop] -> [ColorJitter] -> Normalize"
        rest = list(enumerate(ts))
        if not rest or not isinstance(rest[0][1], Resize):
            raise SyncFusionAmdError(f"Compose: entry 0 ({ts[0]!r}) must be a Resize; supported chain: {shape}" if ts else f"Compose: empty list; supported chain: {shape}")
        self.resize: Resize = rest.pop(0)[1]
        self.crop: Union[RandomCrop, CenterCrop, None] = rest.pop(0)[1] if rest and isinstance(rest[0][1], (RandomCrop, CenterCrop)) else None
        self.jitter: Optional[ColorJitter] = rest.pop(0)[1] if rest and isinstance(rest[0][1], ColorJitter) else None
        if not rest:
            raise SyncFusionAmdError(f"Compose: the chain must end with a Normalize; supported chain: {shape}")
        if not isinstance(rest[0][1], Normalize) or len(rest) > 1:
            i, t = rest[0] if not isinstance(rest[0][1], Normalize) else rest[1]
            raise SyncFusionAmdError(f"Compose: entry {i} ({t!r}) is out of place; supported chain: {shape}")
        self.normalize: Normalize = rest[0][1]
        r = self.resize
        if r.antialias is not True:
            raise SyncFusionAmdError(f"Compose: entry 0 ({r!r}): only antialias=True is implemented (torchvision 0.14.1 resizes tensors without "
                                     "antialiasing otherwise)")
        if r.max_size is not None:
            raise SyncFusionAmdError(f"Compose: entry 0 ({r!r}): max_size is not implemented")
        if str(r.interpolation).lower() != "bilinear":
            raise SyncFusionAmdError(f"Compose: entry 0 ({r!r}): only bilinear interpolation is implemented")
        c = self.crop
        if isinstance(c, RandomCrop) and (c.padding is not None or c.pad_if_needed):
            raise SyncFusionAmdError(f"Compose: entry 1 ({c!r}): padding is not implemented")
        self.transforms = ts

    def __repr__(self):
        return "Compose([" + ", ".join(repr(t) for t in self.transforms) + "])"

    # ---- geometry ---------------------------------------------------------------------------------------------------------------------
    def resized_hw(self, in_hw: Sequence[int]) -> Tuple[int, int]:
        return self.resize.output_size(in_hw)

    def out_hw(self, in_hw: Sequence[int]) -> Tuple[int, int]:
        return self.crop.size if self.crop is not None else self.resized_hw(in_hw)

    # ---- random parameters (host) -----------------------------------------------------------------------------------------------------
    def sample(self, n_clips: int, in_hw: Sequence[int], generator: Optional[torch.Generator] = None) -> ClipParams:
        """Draw the parameters of ``n_clips`` clips of ``in_hw`` frames, clip after clip, in torchvision's order of consumption."""
        rh, rw = self.resized_hw(in_hw)
        th, tw = self.out_hw(in_hw)
        if th > rh or tw > rw:
            raise SyncFusionAmdError(f"{self.crop!r}: crop {(th, tw)} larger than the resized frame {(rh, rw)} (padding is not implemented)")
        n = int(n_clips)
        top, left = torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
        order = torch.arange(4, dtype=torch.int32).repeat(n, 1)
        factor = torch.tensor([1.0, 1.0, 1.0, 0.0]).repeat(n, 1)
        ranges = self.jitter.ranges() if self.jitter is not None else [None] * 4
        mask = torch.full((n,), sum(1 << i for i, r in enumerate(ranges) if r is not None), dtype=torch.int32)
        for k in range(n):
            if isinstance(self.crop, RandomCrop):
                if not (rh == th and rw == tw):     # RandomCrop.get_params: no draw when the crop is the whole frame
                    top[k] = int(torch.randint(0, rh - th + 1, size=(1,), generator=generator))
                    left[k] = int(torch.randint(0, rw - tw + 1, size=(1,), generator=generator))
            elif isinstance(self.crop, CenterCrop):
                top[k] = int(round((rh - th) / 2.0))
                left[k] = int(round((rw - tw) / 2.0))
            if self.jitter is not None:             # ColorJitter.get_params
                order[k] = torch.randperm(4, generator=generator).to(torch.int32)
                for i, r in enumerate(ranges):
                    if r is not None:
                        factor[k, i] = float(torch.empty(1).uniform_(r[0], r[1], generator=generator))
        return ClipParams((rh, rw), (th, tw), top, left, order, factor, mask)

    # ---- the device pass --------------------------------------------------------------------------------------------------------------
    def __call__(self, frames_u8: Tensor, params: Optional[ClipParams] = None, generator: Optional[torch.Generator] = None) -> Tensor:
        """``(N, T, H, W, 3)`` uint8 on the device -> ``(N, 3, T, oh, ow)`` float32; ``params`` from ``sample`` (drawn here when None)."""
        _lib.require_gpu_tensor(frames_u8, "frame_transforms.Compose")
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 5 or frames_u8.shape[-1] != 3:
            raise SyncFusionAmdError(f"frame_transforms.Compose: expected uint8 frames of shape (N, T, H, W, 3), got {frames_u8.dtype} "
                                     f"{tuple(frames_u8.shape)}")
        N, T, H, W, _ = frames_u8.shape
        if params is None:
            params = self.sample(N, (H, W), generator)
        rh, rw = self.resized_hw((H, W))
        oh, ow = self.out_hw((H, W))
        if len(params) != N or tuple(params.resized_hw) != (rh, rw) or tuple(params.out_hw) != (oh, ow):
            raise SyncFusionAmdError(f"frame_transforms.Compose: parameters for {len(params)} clips resized to {tuple(params.resized_hw)} / cropped "
                                     f"to {tuple(params.out_hw)}, frames are {N} clips -> {(rh, rw)} -> {(oh, ow)}")
        lib = _lib.load()
        fr = frames_u8.contiguous()
        host = params.table().contiguous()
        m = (C.c_float * 3)(*self.normalize.mean)
        s = (C.c_float * 3)(*self.normalize.std)
        with torch.cuda.device(fr.device):
            dev = host.to(fr.device)
            out = torch.empty(N, 3, T, oh, ow, dtype=torch.float32, device=fr.device)
            ws_bytes = int(lib.sf_frames_augment_workspace_bytes(N, T, oh, ow))
            ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=fr.device)
            _lib.check(lib.sf_frames_augment(fr.data_ptr(), N, T, H, W, rh, rw, oh, ow, host.data_ptr(), dev.data_ptr(), m, s, out.data_ptr(),
                                             ws.data_ptr(), ws_bytes, _lib.stream_ptr(fr.device)), "sf_frames_augment")
        return out


def default_chain(size: Tuple[int, int] = (112, 112)) -> Compose:
    """The transform a ``null`` ``*_frames_transforms`` block selects (main/dataset_onset.py:47-50)."""
    from .input_pipeline import IMAGENET_MEAN, IMAGENET_STD

    return Compose([Resize(tuple(size), antialias=True), Normalize(IMAGENET_MEAN, IMAGENET_STD)])
