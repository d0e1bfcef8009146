"""fp64 restatement of the v-sampler under a guidance schedule ("Guidance schedules"; sf_vsample_gx), sharing no code with the
product: the solver rows are solver_ref's, the update is fp64, the net is fp32.

Step i, clip b, with v_c the conditional and v_u the unconditional output of the net:

    g = v_u + s[i, b] * (v_c - v_u)                        (v_c itself where s[i, b] == 1)
    v = g * (1 + phi * (std(v_c) / std(g) - 1))            (std over all (C, L) elements of the clip; factor 1 where std(g) == 0 or phi == 0)
    X = a x - b v,   x <- cx x + c0 X + c1 X_prev,   X_prev <- X

A step all of whose scales are 1 never asks for v_u.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch

import solver_ref

Tensor = torch.Tensor


def scales(embedding_scale, sigmas, B: int, interval=None) -> np.ndarray:
    """(T, B) float64 table of scales, written out case by case."""
    T = len(sigmas) - 1
    s = np.asarray(embedding_scale, dtype=np.float64)
    out = np.empty((T, B), dtype=np.float64)
    for i in range(T):
        for b in range(B):
            if s.ndim == 0:
                out[i, b] = float(s)
            elif s.ndim == 2:
                out[i, b] = s[i, b]
            elif s.shape[0] == B:
                out[i, b] = s[b]
            else:
                out[i, b] = s[i]
            if interval is not None and not (interval[0] <= float(np.float32(sigmas[i])) <= interval[1]):
                out[i, b] = 1.0
    return out


def guided(v_c: Tensor, v_u: Optional[Tensor], s_row, phi: float) -> Tensor:
    """The direction v of one step from fp64 v_c, v_u (B, C, L) and the step's B scales."""
    out = torch.empty_like(v_c)
    for b in range(v_c.shape[0]):
        s = float(s_row[b])
        g = v_c[b] if s == 1.0 else v_u[b] + s * (v_c[b] - v_u[b])
        sg = float(g.std(unbiased=False))
        factor = 1.0
        if phi != 0.0 and sg != 0.0:
            factor = 1.0 + phi * (float(v_c[b].std(unbiased=False)) / sg - 1.0)
        out[b] = g * factor
    return out


def sample(net_c: Callable[[Tensor, Tensor], Tensor], net_u: Callable[[Tensor, Tensor], Tensor], x: Tensor, sigmas, solver: str, table,
           phi: float = 0.0, restart_at=()) -> Tensor:
    """The whole loop.  ``net_c(x_fp32, sigma_b)`` / ``net_u(...)``: conditional / unconditional v; ``table``: (T, B) scales.
    ``restart_at``: steps at which the history is dropped and the solver restarts at first order (what a cut WITHOUT the history would
    do: rows of the schedule that begins there)."""
    sig = list(sigmas)
    rows = solver_ref.TABLES[solver](sig)
    for r in restart_at:
        rows[r:] = solver_ref.TABLES[solver](sig[r:])
    sig32 = torch.as_tensor(np.asarray(sig, dtype=np.float32))
    B = x.shape[0]
    x = x.double()
    prev = torch.zeros_like(x)
    for i, (a, b, cx, c0, c1) in enumerate(rows):
        if i in restart_at:
            prev = torch.zeros_like(x)
        s_row = np.asarray(table[i], dtype=np.float64)
        v_c = net_c(x.float(), sig32[i].expand(B)).double()
        v_u = net_u(x.float(), sig32[i].expand(B)).double() if np.any(s_row != 1.0) else None
        v = guided(v_c, v_u, s_row, phi)
        X = a * x - b * v
        x = cx * x + c0 * X + c1 * prev
        prev = X
    return x


def unet_nets(P, cfg, emb: Tensor, chans):
    """(net_c, net_u) around the oracle U-Net: v_u is the same forward with the fixed embedding in place of the clip's."""
    from oracle import unet_ref

    B, n = emb.shape[:2]
    fixed = P["net.cfg.fixed_embedding.weight"][:n][None].expand(B, -1, -1)

    def net_c(x, s):
        return unet_ref.unet_forward(P, cfg, x, s, embedding=emb, channels=chans, embedding_scale=1.0)

    def net_u(x, s):
        return unet_ref.unet_forward(P, cfg, x, s, embedding=fixed, channels=chans, embedding_scale=1.0)

    return net_c, net_u
