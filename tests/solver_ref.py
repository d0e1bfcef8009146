"""fp64 restatement of the multistep v-sampler (syncfusion_amd/solvers.py, sf_vsample_ms), written from the ODE and sharing no code with
the product.

With t = sigma * pi / 2 the probability-flow ODE of the v-objective is  d(x / sin t)/dt = -X(t) / sin(t)**2,  X = cos t * x - sin t * v,
so a step from t_i down to t_n is

    x_n = sin t_n * ( x_i / sin t_i + integral_{t_n}^{t_i} X(s) / sin(s)**2 ds ).

Antiderivatives used below:  int 1/sin**2 = -cot,   int s/sin**2 = -s cot s + ln sin s.
"""
from __future__ import annotations

import math
from typing import Callable

import numpy as np
import torch

Tensor = torch.Tensor


def _angles(sigmas):
    return [float(np.float64(np.float32(s))) * math.pi / 2.0 for s in sigmas]


def _first_order(t_i: float, t_n: float):
    """(c_x, c_0) of the exact step for constant X:  sin t_n / sin t_i  and  sin t_n * (cot t_n - cot t_i) = sin(t_i - t_n) / sin t_i."""
    return math.sin(t_n) / math.sin(t_i), math.sin(t_i - t_n) / math.sin(t_i)


def ddim_rows(sigmas):
    t = _angles(sigmas)
    return [(math.cos(t[i]), math.sin(t[i])) + _first_order(t[i], t[i + 1]) + (0.0,) for i in range(len(t) - 1)]


def ab2_rows(sigmas):
    """X(s) = X_i + (s - t_i) * (X_i - X_p) / (t_i - t_p) through the last two evaluations; the integral of (s - t_i) / sin**2 over
    [t_n, t_i] is  ln sin t_i - ln sin t_n - (t_i - t_n) cot t_n,  and sin t_n times it tends to 0 - 0 - t_i as t_n -> 0."""
    t = _angles(sigmas)
    rows = ddim_rows(sigmas)
    for i in range(1, len(t) - 1):
        t_p, t_i, t_n = t[i - 1], t[i], t[i + 1]
        if t_n > 0.0:
            moment = math.sin(t_n) * (math.log(math.sin(t_i)) - math.log(math.sin(t_n))) - (t_i - t_n) * math.cos(t_n)
        else:
            moment = -t_i
        slope_w = moment / (t_i - t_p)          # multiplies (X_i - X_p)
        a, b, cx, c0, _ = rows[i]
        rows[i] = (a, b, cx, c0 + slope_w, -slope_w)
    return rows


def dpmpp_2m_rows(sigmas):
    """DPM-Solver++(2M), Lu et al. 2022, algorithm 2 with data prediction:  x_n = (b_n / b_i) x - a_n (exp(-h) - 1) D,
    D = (1 + 1/(2r)) X_i - (1/(2r)) X_p,  lambda = ln(a / b),  h = lambda_n - lambda_i,  r = (lambda_i - lambda_p) / h;  first order
    where a lambda is infinite."""
    t = _angles(sigmas)
    rows = ddim_rows(sigmas)
    lam = [math.log(math.cos(s) / math.sin(s)) if 0.0 < s < math.pi / 2.0 and math.cos(s) > 1e-15 else None for s in t]
    for i in range(1, len(t) - 1):
        if lam[i - 1] is None or lam[i + 1] is None or float(np.float32(sigmas[i - 1])) >= 1.0:
            continue
        h = lam[i + 1] - lam[i]
        r = (lam[i] - lam[i - 1]) / h
        a, b, cx, _, _ = rows[i]
        first = -math.cos(t[i + 1]) * math.expm1(-h)
        rows[i] = (a, b, cx, first * (1.0 + 1.0 / (2.0 * r)), -first / (2.0 * r))
    return rows


TABLES = {"ddim": ddim_rows, "ab2": ab2_rows, "dpmpp_2m": dpmpp_2m_rows}


def table(sigmas, solver: str) -> np.ndarray:
    return np.array(TABLES[solver](list(sigmas)), dtype=np.float64)


def multistep_sample(net: Callable[[Tensor, Tensor], Tensor], x: Tensor, sigmas, solver: str) -> Tensor:
    """The loop of sf_vsample_ms with the update in fp64 around an fp32 net: ``net(x_fp32, sigma_b)`` -> v.  Returns fp64."""
    rows = TABLES[solver](list(sigmas))
    sig32 = torch.as_tensor(np.asarray(sigmas, dtype=np.float32))
    B = x.shape[0]
    x = x.double()
    prev = torch.zeros_like(x)
    for i, (a, b, cx, c0, c1) in enumerate(rows):
        v = net(x.float(), sig32[i].expand(B)).double()
        X = a * x - b * v
        x = cx * x + c0 * X + c1 * prev
        prev = X
    return x
