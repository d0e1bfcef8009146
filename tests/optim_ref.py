"""fp64 numpy statement of the optimizer stage (syncfusion_amd/optim.py, csrc/optim.hip): ``torch.nn.utils.clip_grad_norm_``'s global norm and
coefficient, and AdamW with decoupled weight decay (``amsgrad=False``, ``maximize=False``) in torch's order of operations.  No torch in
here: the tests compare both torch and the HIP kernels against it."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np


def grad_norm(grads: Sequence[Optional[np.ndarray]], present: Optional[Sequence[bool]] = None) -> float:
    """Global L2 norm of the gradients that are present."""
    total = 0.0
    for i, g in enumerate(grads):
        if g is None or (present is not None and not present[i]):
            continue
        g = np.asarray(g, dtype=np.float64)
        total += float(np.sum(g * g))
    return float(np.sqrt(total))


def clip_coef(total_norm: float, max_norm: float) -> float:
    """``clip_grad_norm_``: max_norm / (total_norm + 1e-6), clamped to 1 (a NaN stays a NaN)."""
    c = max_norm / (total_norm + 1e-6)
    return 1.0 if c > 1.0 else c


class AdamWRef:
    """``params``: arrays (copied to fp64); ``groups``: dicts with lr, betas, eps, weight_decay; ``group_of[i]``: the group of tensor i."""

    def __init__(self, params: Sequence[np.ndarray], groups: Sequence[Dict], group_of: Sequence[int]):
        self.p: List[np.ndarray] = [np.array(p, dtype=np.float64) for p in params]
        self.groups = [dict(g) for g in groups]
        self.group_of = list(group_of)
        self.m: List[Optional[np.ndarray]] = [None] * len(self.p)      # None until the tensor's first step, as torch's lazy state
        self.v: List[Optional[np.ndarray]] = [None] * len(self.p)
        self.steps = [0] * len(self.p)

    def load_state(self, i: int, step: float, exp_avg: np.ndarray, exp_avg_sq: np.ndarray) -> None:
        self.steps[i] = int(step)
        self.m[i] = np.array(exp_avg, dtype=np.float64)
        self.v[i] = np.array(exp_avg_sq, dtype=np.float64)

    def step(self, grads: Sequence[Optional[np.ndarray]], present: Optional[Sequence[bool]] = None,
             max_norm: Optional[float] = None) -> Tuple[Optional[float], float]:
        """One optimizer step; a tensor whose gradient is absent is skipped whole (no decay, no step increment).  Returns
        (total_norm or None without clipping, clip_coef)."""
        present = [g is not None and (present is None or bool(present[i])) for i, g in enumerate(grads)]
        norm, coef = None, 1.0
        if max_norm is not None:
            norm = grad_norm(grads, present)
            coef = clip_coef(norm, max_norm)
        for i, g in enumerate(grads):
            if not present[i]:
                continue
            h = self.groups[self.group_of[i]]
            lr, (b1, b2), eps, wd = h["lr"], h["betas"], h["eps"], h["weight_decay"]
            if self.m[i] is None:
                self.m[i] = np.zeros_like(self.p[i])
                self.v[i] = np.zeros_like(self.p[i])
            self.steps[i] += 1
            t = self.steps[i]
            bc1 = 1.0 - b1 ** t
            bc2 = 1.0 - b2 ** t
            gc = np.asarray(g, dtype=np.float64) * coef
            p, m, v = self.p[i], self.m[i], self.v[i]
            p -= lr * wd * p
            m += (1.0 - b1) * (gc - m)
            v *= b2
            v += (1.0 - b2) * gc * gc
            p -= (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
        return norm, coef
