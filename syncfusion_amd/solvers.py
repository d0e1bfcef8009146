"""Coefficient tables of the multistep v-sampler ("Multistep sampler"); host side, numpy only.

In angle form, ``t = sigma * pi / 2``, ``alpha = cos t``, ``beta = sin t``, the probability-flow ODE of the v-objective is
``d(x / beta)/dt = -x0_hat / beta**2`` with ``x0_hat = alpha * x - beta * v``.  Every solver here is a linear rule on ``x0_hat`` that needs
one U-Net evaluation per step; the step a table row describes is

    X_i = alpha_i * x - beta_i * v          x <- c_x * x + c_0 * X_i + c_1 * X_{i-1}

These solvers are additions: the reference's sampler is the first-order rule (``"ddim"``).
"""
from __future__ import annotations

import numpy as np

SOLVERS = ("ddim", "ab2", "dpmpp_2m")


def check_sigmas(sigmas, num_steps=None) -> np.ndarray:
    """The schedule as a 1-D fp32 array of ``T + 1 >= 2`` finite, strictly decreasing values inside [0, 1]; ``ValueError`` otherwise."""
    s = np.asarray(sigmas)
    if s.ndim != 1 or s.size < 2:
        raise ValueError(f"sigmas must be a 1-D array of num_steps + 1 >= 2 values, got shape {s.shape}")
    if num_steps is not None and s.size != int(num_steps) + 1:
        raise ValueError(f"sigmas must hold num_steps + 1 = {int(num_steps) + 1} values, got {s.size}")
    s = s.astype(np.float32)
    if not np.all(np.isfinite(s)):
        raise ValueError("sigmas must be finite")
    if s.max() > 1.0 or s.min() < 0.0:
        raise ValueError(f"sigmas must lie inside [0, 1], got [{s.min()}, {s.max()}]")
    if not np.all(s[1:] < s[:-1]):
        raise ValueError("sigmas must be strictly decreasing")
    return s


def solver_table(sigmas, solver: str = "ab2") -> np.ndarray:
    """``(T, 5)`` float64 rows ``(alpha_i, beta_i, c_x, c_0, c_1)`` for the ``T + 1`` schedule values ``sigmas``; all arithmetic in fp64 on
    the fp32 sigmas.  In every row ``c_0 + c_1`` is the first-order ``c_0``, and row 0 is the first-order row.

    ``"ddim"``: the exact step for constant ``x0_hat``, ``c_x = beta_{i+1} / beta_i``, ``c_0 = alpha_{i+1} - beta_{i+1} alpha_i / beta_i``.
    ``"ab2"``: second-order Adams-Bashforth in the angle, ``x0_hat`` linear in ``t`` through ``X_{i-1}`` and ``X_i`` with the integral of
    ``x0_hat / sin**2`` in closed form; finite at both ends of ``1 -> 0``.
    ``"dpmpp_2m"``: DPM-Solver++(2M) (Lu et al., 2022) in ``lambda = ln(alpha / beta)``; a row whose three lambdas are not all finite
    (``sigma_{i-1} = 1`` or ``sigma_{i+1} = 0``) is the first-order row."""
    if solver not in SOLVERS:
        raise ValueError(f"unknown solver {solver!r}: expected one of {SOLVERS}")
    sig = check_sigmas(sigmas)
    t = sig.astype(np.float64) * (np.pi / 2.0)
    al, be = np.cos(t), np.sin(t)
    al[sig == 1.0], be[sig == 0.0] = 0.0, 0.0          # the exact ends (cos(pi/2) in floating point is 6e-17)
    T = sig.size - 1
    a0, b0, a1, b1 = al[:-1], be[:-1], al[1:], be[1:]          # rows i = 0 .. T - 1: this level and the next (b0 > 0: sigma_i > 0)
    cx = b1 / b0
    c0 = a1 - b1 * a0 / b0
    w = np.zeros(T, dtype=np.float64)                          # second-order weight: c_0 += w, c_1 = -w
    if solver == "ab2" and T > 1:
        ratio = np.where(b1[1:] > 0.0, b1[1:] / b0[1:], 1.0)   # beta ln beta is 0 at beta_{i+1} = 0
        w[1:] = ((t[1:-1] - t[2:]) * a1[1:] + b1[1:] * np.log(ratio)) / (t[:-2] - t[1:-1])
    elif solver == "dpmpp_2m" and T > 1:
        ok = (sig[:-2] < 1.0) & (sig[2:] > 0.0)                # all three lambdas of row i finite
        with np.errstate(divide="ignore", invalid="ignore"):
            lam = np.log(al / be)
            inv_2r = 0.5 * (lam[2:] - lam[1:-1]) / (lam[1:-1] - lam[:-2])
            w[1:] = np.where(ok, c0[1:] * inv_2r, 0.0)
    return np.stack([a0, b0, cx, c0 + w, 0.0 - w], axis=1)


def pack_table(table: np.ndarray) -> np.ndarray:
    """The ``(T, 8)`` fp32 rows ``sf_vsample_ms`` reads: the five coefficients and three unused floats (one aligned load per row)."""
    t = np.asarray(table, dtype=np.float64)
    if t.ndim != 2 or t.shape[1] != 5:
        raise ValueError(f"a solver table is (T, 5), got {t.shape}")
    out = np.zeros((t.shape[0], 8), dtype=np.float32)
    out[:, :5] = t
    return out
