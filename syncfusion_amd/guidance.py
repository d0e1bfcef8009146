"""Guidance schedules of the v-sampler ("Guidance schedules"); host side, numpy only.

``s[i, b]`` is the classifier-free guidance scale of clip ``b`` at step ``i`` (the step that evaluates the net at ``sigmas[i]``).  A step all
of whose scales are exactly 1 is a *single-pass step*: its guided direction is the conditional output itself, so the unconditional half of
the batch is not evaluated.  ``plan_segments`` cuts a table into maximal runs of one kind; the sampler runs one ``sf_vsample_gx`` per run and
threads the multistep history through the cuts.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from .solvers import check_sigmas

Segment = Tuple[int, int, bool]


def _host_array(a) -> np.ndarray:
    if hasattr(a, "detach"):                                     # a torch tensor, on any device
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def is_plain_scale(embedding_scale) -> bool:
    """True for a Python / numpy scalar: the one-float-per-call form the sampler has always taken."""
    return isinstance(embedding_scale, (int, float, np.integer, np.floating)) and not isinstance(embedding_scale, bool)


def scale_table(embedding_scale, sigmas, B: int, guidance_interval: Optional[Sequence[float]] = None) -> np.ndarray:
    """The ``(T, B)`` fp32 table ``s[i, b]`` for the ``T + 1`` schedule values ``sigmas`` and ``B`` clips.

    ``embedding_scale``: a float (every clip, every step), a ``(B,)`` array or tensor (one scale per clip), a ``(T,)`` array (one per
    step; where ``T == B`` a 1-D array is read per clip) or a ``(T, B)`` array.  ``guidance_interval=(lo, hi)``: the scale is 1 at every
    step whose ``sigmas[i]`` lies outside ``lo <= sigmas[i] <= hi``.  ``ValueError`` for non-finite values, shapes that are none of the
    above, or ``lo > hi``."""
    sig = check_sigmas(sigmas)
    T, B = sig.size - 1, int(B)
    if B < 1:
        raise ValueError(f"B must be >= 1, got {B}")
    s = _host_array(embedding_scale)
    if s.dtype == object or not (np.issubdtype(s.dtype, np.floating) or np.issubdtype(s.dtype, np.integer)):
        raise ValueError(f"embedding_scale must be real numbers, got dtype {s.dtype}")
    s = s.astype(np.float64)
    if s.ndim == 0:
        table = np.full((T, B), float(s))
    elif s.shape == (B,):
        table = np.broadcast_to(s[None, :], (T, B))
    elif s.shape == (T,):
        table = np.broadcast_to(s[:, None], (T, B))
    elif s.shape == (T, B):
        table = s
    else:
        raise ValueError(f"embedding_scale of shape {s.shape} is none of (), ({B},), ({T},), ({T}, {B})")
    table = np.array(table, dtype=np.float32)
    if not np.all(np.isfinite(table)):
        raise ValueError("guidance scales must be finite")
    if guidance_interval is not None:
        iv = _host_array(guidance_interval).astype(np.float64)
        if iv.shape != (2,) or not np.all(np.isfinite(iv)):
            raise ValueError(f"guidance_interval must be two finite values (lo, hi), got {guidance_interval!r}")
        lo, hi = float(iv[0]), float(iv[1])
        if lo > hi:
            raise ValueError(f"guidance_interval: lo = {lo} > hi = {hi}")
        level = sig[:T].astype(np.float64)
        table[(level < lo) | (level > hi), :] = 1.0
    return table


def check_rescale(guidance_rescale) -> float:
    phi = float(guidance_rescale)
    if not 0.0 <= phi <= 1.0:                                   # (NaN fails both comparisons)
        raise ValueError(f"guidance_rescale must lie inside [0, 1], got {guidance_rescale!r}")
    return phi


def plan_segments(table) -> List[Segment]:
    """``[(i0, i1, two)]``: the maximal runs ``i0 <= i < i1`` of consecutive steps that are all single-pass (``two=False``: every scale of
    the step is exactly 1) or all not (``two=True``), in order; they cover ``0 .. T``."""
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"a scale table is (T, B), got {t.shape}")
    two = np.any(t != 1.0, axis=1)
    cuts = [0] + [i for i in range(1, t.shape[0]) if two[i] != two[i - 1]] + [t.shape[0]]
    return [(i0, i1, bool(two[i0])) for i0, i1 in zip(cuts[:-1], cuts[1:])]


def evaluation_rows(segments: Sequence[Segment], B: int) -> int:
    """U-Net batch rows of the whole call: ``2 B`` per step of a ``two`` segment, ``B`` per single-pass step."""
    return sum((i1 - i0) * (2 * int(B) if two else int(B)) for i0, i1, two in segments)
