"""fp64 references, per-element gates and an fp32 CPU emulation for the shared back half of the small-batch implicit-GEMM kernels
(csrc/gemm_epilogue.h: conv_gemm_sk / _v2 / _fast / _wp / _rs), reached through the op-level entries sf_op_conv1d_epi and sf_op_conv1d_ln.

conv1d_ref.py gates bias and residual.  Here the whole epilogue is armed -- bscale, badd, act 1 / 2 / 3, out_f32, a second source -- and the
three statistics contracts the header calls its own: rowpart_out, gnpart_out and the LayerNorm consumer (accumulator side: ln_colsum;
operand side: ln_ss / res_ln).  U, U24, C_ACC, gamma and the fp64 convolution come from conv1d_ref.py; nothing is copied and no constant below
is fitted to a device run, with ONE exception that the text of the header cannot give: C_ACT, the error of the device's erff / expf / division
(no ULP figure for them is documented in the ROCm installation), measured as described under "Values".  u = 2^-24 throughout, u_T = U[T].

VALUES (epi_values).   y = (v + bias) * bscale[b] + res + badd[b],  out = T(act(y)),   v = the fp32 accumulator.
  conv1d_ref's gate u_T |ref| + gamma(K) A covers K + 2 roundings (accumulation, + bias, + res) with A = conv(|x|, |w|) + |bias| + |res|.  The
  product with bscale and the sum with badd are two more roundings on the path of every term, so gamma(K + 2), and
      A = (conv(|x|, |w|) + |bias|) |bscale| + |res| + |badd|                   (a contraction of * and + into one fmaf only removes a rounding).
  act = 1 (relu): 1-Lipschitz and exact: no new term.
  act = 2, 3: |act(y_dev) - act(y)| <= Lip(act) gamma A + (error of the activation's own arithmetic).
      Lip(gelu) = max Phi(x) + x phi(x) = Phi(sqrt 2) + sqrt 2 phi(sqrt 2) = 1.12896.. <= 1.13;  Lip(silu) = max |s + x s (1 - s)| = 1.0998.. <= 1.10;
      act 3 = silu(gelu(.)): 1.13 * 1.10 <= 1.25.
      The activation's own arithmetic (common.h apply_act): gelu = 0.5 y (1 + erff(y fl(1 / sqrt 2))).  For y < 0 the sum 1 + erf CANCELS: erf is
      stored with an absolute error of at least 2^-25 near -1 however good erff is, so the error of gelu is proportional to |y|, not to
      |gelu(y)| (at y = -3 a correctly rounded erff already gives 185 u |gelu(y)|).  The term is therefore C_ACT u |y| -- |act(y)| <= |y| for
      both activations, so this is the issue's "c_act u |act(y)|" with the one normaliser that also holds on the negative tail.  Pieces, in u |y|:
      argument rounding 2 u |t| erf'(t) <= 0.97, erff E_erf ulp -> E_erf, the sum 1 + erf: 1, the two products: <= 2;  silu(g) = g / (1 + expf(-g)):
      expf E_exp ulp -> 2 E_exp, the sum 1, the division (v_div sequence, correctly rounded) 1, times Lip(silu).  E_erf and E_exp are what is
      not documented here; C_ACT is measured ONCE on the device (test_gpu_gemm_epilogue.py, test_c_act: the fp32 launch with act 0 gives the
      device's own y bit for bit, so |dev - act64(y_dev)| / (u |y_dev|) isolates the library functions) and fixed at 4 x the measured maximum:
      profiles/gemm_epilogue_test.txt holds the measurement.
  The stored rounding is u_T |ref| (u for out_f32).  fp16 subnormal outputs: as conv1d_ref.py.

ROWPART (row32_stats).  Compared with the fp64 (mean, M2) of each row's 32 STORED values x_i, read back from the launch's own output, so the
  GEMM error drops out.  a = mean |x_i|.
      mean = fl(sum / 32): (x0 + x1) + (x2 + x3) per lane, then a three-level butterfly over the row's eight lanes: depth 5, the product with
      1 / 32 is exact:   |d mean| <= 6 u a  =: e                                (5 first-order units + 1 for (1 + u)^5)
      M2: d_i = fl(x_i - mean) (u), a chain of four fmaf(d, d, q) (4), the butterfly (3); sum (x_i - mean_dev)^2 = M2 + 32 (d mean)^2:
                         |d M2| <= 10 u M2 + 33 e^2                             (2 + 7 units + 1;  32 (1 + 10 u) <= 33)
  The macro tiles (the one mt_ln row) keep statistics of their own, eight values per lane: an ordered sum of 8 (7 roundings) and two quad
  permutes: 9 + 1 = 10 u a for the mean; 2 + 8 + 2 + 1 = 13 u M2 (ROW_UNITS).

GNPART (gn_tile_stats).  Compared with the fp64 (mean, M2) of the stored values over (rows of the segment) x 32 columns.  Segment 0: the tile's
  rows in the clip of its first row; segment 1: the tile's rows of the next clip, below M.  An empty segment is EXACTLY (0, 0).  M2 >= 0 exactly
  (the final fmaxf: a consumer takes rsqrt(M2 / n + eps)).
  k rows with fp64 row statistics (m_r, q_r), a_r = mean |x| of row r, e_r = 6 u a_r;  p = m_first,  m = the segment's mean,
  S = sum_r (q_r + 32 (m_r - p)^2),  P = 32 k (m - p)^2 <= S,  a = the segment's mean |x|.
  The device forms d_r = fl(mean_r - p') about p' = its own first row mean,
  t1 = sum d_r in row order, dk = fl(t1 / k), mean = fl(p' + dk).  The identities mean = p + sum (m_r - p) / k and M2 = S - P hold for ANY
  pivot, so the pivot's own error does not enter to first order.
      mean: the row means' errors average to mean_r e_r <= 6 u a;  d_r one rounding, the ordered sum k - 1, the division 1: (k + 1) u, + 1 for
      the second order, on mean_r |m_r - p|;  the last sum u |mean| <= u a;  what e_r adds inside (k + 2) u mean |d_r| is (k + 2) 12 u^2 a << u a:
                         |d mean| <= 8 u a + (k + 2) u mean_r |m_r - p|                        (the issue's candidate had k + 3)
      M2: the issue's candidate, kept as it stands:
                         |d M2| <= (k + 12) u S + 40 k (8 u a)^2 + 512 u a sum_r |m_r - m|
      Where its terms come from: t2 = sum_r fmaf(32 d_r, d_r, M2_r), one fmaf and at most k - 1 sums per term, all terms >= 0: k u S; M2_r
      carries 10 u q_r (above) and d_r^2 2 u from d_r's rounding: (k + 12) u S.  The row means' errors eps_r enter d_r^2 as 2 (m_r - p) eps_r
      and the subtracted 32 t1 dk = 32 t1^2 / k as 2 (sum (m_r - p)) (sum eps_r) / k: to first order the two leave 64 sum_r (m_r - m) eps_r,
      which is why m and not p stands in the last term (64 * 6 u a = 384 u a <= 512 u a); the squares of eps_r are the middle term.
      A worst-case count would add (2 k + 2) u P for the roundings of t1 itself (2 (k - 1) + 2 units on t1^2 / k), which cancel against
      nothing.  That count is not reachable: a rounding of the partial sum j d is relative to THAT sum, so k - 1 roundings of a sum of
      like terms cost about k / 2 units, and where one term dominates t1, P is S / k.  A greedy adversarial search on the fp32 emulation
      (constant rows, every row mean chosen among 24 neighbours to push both sums the wrong way, P ~ S) reached 0.61 of the candidate and
      random segments 0.48, so the candidate is not loosened (test_gemm_epilogue_cpu.py keeps the adversarial segment as a case).
      The clamp cannot bite on finite data: d_first = 0 gives M2 = S - P >= P / (k - 1) >= S' / k for the mean part S' of S, orders of
      magnitude above the rounding error of S.  So the planted fault "clamp removed" changes no bit on any case and no gate can catch it;
      the CPU test asserts exactly that (bit identity) instead of a 10 x miss.

LAYERNORM CONSUMER (ln_pool_row, ln_fold; conv_gemm_fast's operand transform).  ref = Linear(LN(src)) (+ modulation, + res_ln) + bias in fp64
  from the T-rounded source;  mu, var = fp64 row statistics, r = 1 / sqrt(var + eps).
  Inputs: ln_part (mean_j, M2_j) per 32 channels, with |d mean_j| <= e_in_j and |d M2_j| <= q_in M2_j + 33 e_in_j^2.  Computed by the test in fp64
  and rounded to fp32: e_in_j = u |mean_j|, q_in = u.  Chained behind a producer: the ROWPART bound, e_in_j = 6 u a_j, q_in = 10 u.
      mean = fl(sum8(sm) / nt), sm = the lane's <= 4 partials: conv_gemm_fast adds them in sequence (3 roundings: 0 + mp[0] is exact),
      conv_gemm_wp / _rs pairwise (2); the butterfly 3; the division 1: 7 (6) units + 1 on mean_j |mean_j|, + mean_j e_in_j:
                         dmean = N_SUM u mean_j |mean_j| + mean_j e_in_j,     N_SUM = 8 (fast, macro tiles) / 7 (wp, rs)
      m2 = sum (M2_j + 32 d_j^2): d_j = fl(mean_j - mean) (2 u on d^2), the fmaf 1, the lane's ordered sum <= 4, the butterfly 3, / cin 1, + eps 1:
      12 u + q_in relative on var + eps, + what the means' errors add: sum 32 (mean_j - mean_dev)^2 / cin = var_means + dmean^2 exactly, and
      each e_in_j enters 32 d_j^2 as 64 |d_j| e_in_j + 33 e_in_j^2 (+ 33 from M2_j): with v_e = sum_j (64 |mean_j - mu| e_in_j + 66 e_in_j^2) / cin
      rsqrtf: v_rsq_f32, 1 ulp in the CDNA ISA's own table; 2 ulp = 4 u allowed for the library's wrapper:
                         e_rstd = (12 u + q_in) / 2 + 4 u + (dmean^2 + v_e) / (2 (var + eps))      (relative)
  Accumulator side:  v = rstd (acc - mean cu),  cu = launch_row_sums' fp32 sum of the PACKED weight row (K terms in an order of its own:
  (K - 1) u Wabs, Wabs = sum_k |w_k|);  mean cu, the difference and the product with rstd: 3 roundings
      bound(v) = r [gamma(K) A_raw + |mu| (K - 1) u Wabs + dmean |colsum| + 3 u (|acc| + |mu colsum|)] + e_rstd |ref_v|
  with A_raw = sum |src_k| |w_k|.  Operand side (conv_gemm_fast): a_k = T(fmaf(x_k, A_k, fmaf(-mean, A_k, sh_k))), A_k = fl(rstd fl(1 + ss_k));
  the difference x_k A_k - mean A_k cancels, so its error is proportional to (|x_k| + |mu|), not to |a_k| -- the price of the one-fmaf form at
  a large row offset:
      |d a_k| <= (e_rstd + 4 u) (|x_k| + |mu|) r |1 + ss_k| + r dmean |1 + ss_k| + u |sh_k| + u_T |a_k|          (u_T: 16-bit operands only)
      bound(v) = sum_k |w_k| |d a_k| + gamma(K) sum_k |a_k| |w_k|
  res_ln: the residual fmaf((res - mean) rstd, 1 + ss, sh) in fp32: (e_rstd + 4 u) |res_n - mu| r |1 + ss_n| + r dmean |1 + ss_n| + u |sh_n|.
  Then the epilogue: + bias (and + residual): gamma's K + 3 already holds those units; stored rounding u_T |ref|.

Plain module (not a conftest): the tests import it like conv1d_ref.py.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

import conv1d_ref as R
import numerics as nx
from conv1d_ref import C_ACC, U, U24, gamma, round_to   # noqa: F401

u = U24
TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
LN_EPS = 1e-5
LIP = {0: 1.0, 1: 1.0, 2: 1.13, 3: 1.25}
# Measured on the device (profiles/gemm_epilogue_test.txt): max |dev - act64(y_dev)| / (u |y_dev|) over the fp32 sk case of the table, times 4.
C_ACT_MEASURED = {2: 1.574, 3: 2.942}
C_ACT = {0: 0.0, 1: 0.0, 2: 4.0 * C_ACT_MEASURED[2], 3: 4.0 * C_ACT_MEASURED[3]}
N_SUM = {"fast": 8, "mt": 8, "wp": 7, "rs": 7}
FAULTS = ("seg_plus", "seg_minus", "rows_past_M", "transposed", "swapped", "no_32d2", "no_clamp", "mean_div_32", "cu_first_column", "bscale_after_res",
          "badd_by_row")


class EpiCase(NamedTuple):
    """One launch of sf_op_conv1d_epi.  ops: which of bias / bscale / res / badd are armed, e.g. "b", "bsra" (bias, scale, res, add).
    regime: "" (unit inputs, clip b: mean 0.5 b (-1)^b, scale 1 + 0.3 b) or a statistics regime of the STORED output ("offset:<ratio>", "const",
    "first50"): the output is then the residual (weights 1e-2 / K^0.5; "const": zero), row by row in that regime."""
    name: str
    dtype: str
    B: int
    L: int
    C: int
    C2: int
    N: int
    taps: int
    stride: int
    pad: int
    up: int
    ops: str
    act: int
    out_f32: bool
    want_row: bool
    want_gn: bool
    mt_ln: bool
    regime: str
    label: str
    row: bool
    gn: bool

    @property
    def K(self) -> int:
        return self.taps * self.C + self.C2

    @property
    def Lout(self) -> int:
        return (self.L * self.up + 2 * self.pad - self.taps) // self.stride + 1

    @property
    def M(self) -> int:
        return self.B * self.Lout


class LnCase(NamedTuple):
    """One launch of sf_op_conv1d_ln on (B, L, C) -> N.  form: "acc" (accumulator side), "ss" (operand side with modulation), "ss_res" (and the
    residual transformed, N == C), "plain" (operand side, no modulation).  ratio: source rows at mean / std = ratio (0: the clip regime)."""
    name: str
    dtype: str
    B: int
    L: int
    C: int
    N: int
    form: str
    ratio: float
    label: str
    producer: str      # label of the chained 1x1 producer (C -> C) that writes the source and its partials

    @property
    def M(self) -> int:
        return self.B * self.L


def family(label: str) -> str:
    return label.split("<")[0].replace("conv_gemm_", "") if label.startswith("conv_gemm_") else "classic"


# ---------------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------------
def clip_input(B: int, L: int, C: int, gen: torch.Generator, T: str) -> torch.Tensor:
    """(B, L, C) rounded to T: clip b has mean 0.5 b (-1)^b and scale 1 + 0.3 b, so that a row attributed to the wrong clip moves a statistic
    by orders of magnitude more than its bound."""
    b = torch.arange(B, dtype=torch.float32).reshape(B, 1, 1)
    return round_to(torch.randn(B, L, C, generator=gen) * (1 + 0.3 * b) + 0.5 * b * (-1.0) ** b, T)


def regime_rows(B: int, L: int, N: int, regime: str, gen: torch.Generator, T: str) -> torch.Tensor:
    if regime == "first50":
        r = clip_input(B, L, N, gen, T)
        m = torch.arange(B * L).reshape(B, L)
        first = (m % 32 == 0) | (torch.arange(L).reshape(1, L) == 0)         # the first row of every tile segment
        return round_to(r + 50.0 * first[:, :, None], T)
    return nx.row_input(B, L, N, regime, gen, TORCH_DT[T])


def epi_operands(c: EpiCase, seed: int = 0) -> dict:
    """Seeded operands in the values the op reads (fp32 tensors holding T-rounded values where the op reads T).  w is the GEMM matrix (N, K),
    column tap * C + c, then the C2 columns of the second source; w_op what the kernel multiplies by."""
    g = torch.Generator().manual_seed(seed)
    T = R.STORE[c.dtype]
    o = {"x": clip_input(c.B, c.L, c.C, g, T)}
    o["x2"] = clip_input(c.B, c.Lout, c.C2, g, T) if c.C2 else None
    w = torch.randn(c.N, c.K, generator=g) / math.sqrt(c.K)
    if c.regime:
        w = w * (0.0 if c.regime == "const" else 1e-2)
    o["w"] = w.contiguous()
    o["w_op"] = round_to(w, T)
    o["bias"] = torch.randn(c.N, generator=g) * 0.1 if "b" in c.ops and c.regime != "const" else (torch.zeros(c.N) if "b" in c.ops else None)
    o["bscale"] = 1.0 + 0.3 * torch.randn(c.B, c.N, generator=g) if "s" in c.ops else None
    if "r" in c.ops:
        o["res"] = regime_rows(c.B, c.Lout, c.N, c.regime, g, T) if c.regime else round_to(torch.randn(c.B, c.Lout, c.N, generator=g), T)
    else:
        o["res"] = None
    bb = torch.arange(c.B, dtype=torch.float32).reshape(c.B, 1)
    o["badd"] = 0.5 * torch.randn(c.B, c.N, generator=g) + bb * (-1.0) ** bb if "a" in c.ops else None
    return o


def _split(c, label: Optional[str] = None) -> bool:
    return c.dtype == "fp32x" and R.is_split(label or c.label)


def act64(y: torch.Tensor, act: int) -> torch.Tensor:
    if act == 0:
        return y
    if act == 1:
        return y.clamp_min(0.0)
    g = 0.5 * y * (1.0 + torch.erf(y * math.sqrt(0.5)))
    return g if act == 2 else g * torch.sigmoid(g)


def linear64(c, o, floor: float = 0.0):
    """(lin, Alin) in fp64: the accumulator's exact value and sum |a| |w| (operand magnitudes raised to `floor` for the split families)."""
    K1 = c.taps * c.C
    w = o["w_op"].double()
    w1 = w[:, :K1].reshape(c.N, c.taps, c.C).permute(0, 2, 1)                  # (N, C, taps): conv1d_ref's layout
    lin, A = R.conv1d_ref(o["x"], w1, None, None, c.taps, c.stride, c.pad, c.up, floor)
    if c.C2:
        w2 = w[:, K1:]
        lin = lin + o["x2"].double() @ w2.T
        A = A + o["x2"].double().abs().clamp_min(floor) @ w2.abs().clamp_min(floor).T
    return lin, A


def epi_ref(c: EpiCase, o: dict):
    """(ref, bound) in fp64, (B, Lout, N): the module docstring's VALUES gate."""
    lin, A = linear64(c, o, R.X3_FLOOR if _split(c) else 0.0)
    y = lin
    if o["bias"] is not None:
        y = y + o["bias"].double()
        A = A + o["bias"].double().abs()
    if o["bscale"] is not None:
        y = y * o["bscale"].double()[:, None, :]
        A = A * o["bscale"].double().abs()[:, None, :]
    if o["res"] is not None:
        y = y + o["res"].double()
        A = A + o["res"].double().abs()
    if o["badd"] is not None:
        y = y + o["badd"].double()[:, None, :]
        A = A + o["badd"].double().abs()[:, None, :]
    ref = act64(y, c.act)
    uT = U["fp32"] if c.out_f32 else U[R.STORE[c.dtype]]
    bound = uT * ref.abs() + LIP[c.act] * gamma(c.K + 2, c.dtype, c.label) * A + C_ACT[c.act] * u * y.abs()
    return ref, bound, y


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 statistics of stored values and their bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def row_stats64(stored: torch.Tensor):
    """stored (M, N) -> (mean, M2, a), each (M, N / 32) fp64, of every row's 32 values per column tile."""
    M, N = stored.shape
    x = stored.double().reshape(M, N // 32, 32)
    mean = x.mean(-1)
    return mean, ((x - mean[..., None]) ** 2).sum(-1), x.abs().mean(-1)


ROW_UNITS = {"mt": (10, 13)}        # (mean, M2) units of a family's own row statistics; every other family calls row32_stats: (6, 10)


def rowpart_bound(m2: torch.Tensor, a: torch.Tensor, fam: str = ""):
    cm, cq = ROW_UNITS.get(fam, (6, 10))
    e = cm * u * a
    return e, cq * u * m2 + 33 * e * e


def segments(M: int, Lout: int, mt: int):
    """The two row ranges [lo, hi) (tile-local) of row tile mt: gn_tile_stats' own rule, restated."""
    m0 = mt * 32
    rb = min((m0 // Lout + 1) * Lout - m0, 32)
    return (0, rb), (rb, max(rb, min(32, M - m0)))


def gnpart64(stored: torch.Tensor, Lout: int):
    """stored (M, N) -> ref (mt, nt, 2, 2) fp64 and bound (mt, nt, 2, 2): the module docstring's GNPART gate.  Empty segments: ref 0, bound 0."""
    M, N = stored.shape
    mean_r, q_r, a_r = row_stats64(stored)
    mtiles, nt = (M + 31) // 32, N // 32
    ref = torch.zeros(mtiles, nt, 2, 2, dtype=torch.float64)
    bound = torch.zeros_like(ref)
    for mt in range(mtiles):
        for seg, (lo, hi) in enumerate(segments(M, Lout, mt)):
            k = hi - lo
            if k <= 0:
                continue
            rows = slice(mt * 32 + lo, mt * 32 + hi)
            mr, qr, ar = mean_r[rows], q_r[rows], a_r[rows]
            m = mr.mean(0)
            p = mr[0]
            S = (qr + 32 * (mr - p) ** 2).sum(0)
            ref[mt, :, seg, 0] = m
            ref[mt, :, seg, 1] = (qr + 32 * (mr - m) ** 2).sum(0)
            bound[mt, :, seg, 0] = 8 * u * ar.mean(0) + (k + 2) * u * (mr - p).abs().mean(0)
            bound[mt, :, seg, 1] = (k + 12) * u * S + 40 * k * (8 * u * ar.mean(0)) ** 2 + 512 * u * ar.mean(0) * (mr - m).abs().sum(0)
    return ref, bound


def check(dev: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, what: str, quiet: bool = True) -> float:
    """Assert |dev - ref| <= bound for EVERY element (dev finite everywhere); returns max err / bound (0 / 0 = 0, x / 0 = inf)."""
    d = dev.detach().double().cpu()
    assert d.shape == ref.shape == bound.shape, f"{what}: shapes {tuple(d.shape)} / {tuple(ref.shape)} / {tuple(bound.shape)}"
    bad = ~torch.isfinite(d)
    if bool(bad.any()):
        raise AssertionError(f"{what}: {int(bad.sum())} non-finite values of {d.numel()}, first at {nx._unravel(int(bad.flatten().nonzero()[0]), d.shape)}")
    err = (d - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = int(ratio.flatten().argmax()) if ratio.numel() else 0
    r = float(ratio.flatten()[worst]) if ratio.numel() else 0.0
    if not quiet:
        print(f"{what}: err/bound {r:.3f}")
    idx = nx._unravel(worst, d.shape)
    assert r <= 1.0, (f"{what}: err/bound {r:.3g} > 1 at {idx}: got {float(d[idx]):.9g}, ref {float(ref[idx]):.9g}, bound {float(bound[idx]):.3g}; "
                      f"{int((ratio > 1).sum())} of {d.numel()} over the bound")
    return r


def ratio_of(dev, ref, bound) -> float:
    """max err / bound without asserting (the CPU tests measure headroom and planted faults with it); non-finite -> inf."""
    d = dev.detach().double().cpu()
    if not bool(torch.isfinite(d).all()):
        return float("inf")
    err = (d - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max()) if ratio.numel() else 0.0


def check_stats(stored: torch.Tensor, rowpart: Optional[torch.Tensor], gnpart: Optional[torch.Tensor], Lout: int, what: str, assert_: bool = True,
                fam: str = ""):
    """The ROWPART and GNPART gates of one launch against its own stored output (M, N).  Returns {gate: err / bound}."""
    f = check if assert_ else (lambda d, r, b, w: ratio_of(d, r, b))
    out = {}
    if rowpart is not None:
        mean, m2, a = row_stats64(stored)
        e, bq = rowpart_bound(m2, a, fam)
        rp = rowpart.double().cpu()
        out["rowpart.mean"] = f(rp[..., 0], mean, e, what + " rowpart mean")
        out["rowpart.M2"] = f(rp[..., 1], m2, bq, what + " rowpart M2")
    if gnpart is not None:
        ref, bound = gnpart64(stored, Lout)
        gp = gnpart.double().cpu()
        out["gnpart.mean"] = f(gp[..., 0], ref[..., 0], bound[..., 0], what + " gnpart mean")
        out["gnpart.M2"] = f(gp[..., 1], ref[..., 1], bound[..., 1], what + " gnpart M2")
        neg = float(gp[..., 1].min()) if gp.numel() else 0.0
        if assert_:
            assert neg >= 0.0, f"{what}: gnpart M2 {neg} < 0"
        elif neg < 0.0:
            out["gnpart.M2"] = float("inf")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 emulation of gemm_epilogue.h (what a correct kernel computes, in its own order), with planted faults
# ---------------------------------------------------------------------------------------------------------------------------------
def _fma(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """fmaf on fp32 tensors: the product of two fp32 values is exact in fp64; the sum is rounded to fp64 and then to fp32 (a double rounding
    differs from fmaf in ~2^-29 of the cases, by one ulp: far inside every bound)."""
    return (a.double() * b.double() + c.double()).float()


def _sum8(v: torch.Tensor) -> torch.Tensor:
    """sum8_dpp over the last axis (8 lanes): quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror."""
    a = v[..., 0::2] + v[..., 1::2]
    b = a[..., 0::2] + a[..., 1::2]
    return b[..., 0] + b[..., 1]


def emulate_values(c: EpiCase, o: dict, fault: str = "", stored: bool = True) -> torch.Tensor:
    """epi_values in fp32 on the fp32 accumulator of conv1d_ref.emulate (split families: their three products): (B, Lout, N)."""
    K1 = c.taps * c.C
    w = o["w_op"]
    w1 = w[:, :K1].reshape(c.N, c.taps, c.C).permute(0, 2, 1)
    v = R.emulate(o["x"], w1, None, None, c.taps, c.stride, c.pad, c.up, c.dtype, c.label, stored=False)
    if c.C2:
        if _split(c):
            ah, al = R.x3_split(o["x2"])
            wh, wl = R.x3_split(w[:, K1:].T.contiguous())
            v = v + (ah @ wh + (ah @ wl + al @ wh) * (1.0 / 2048.0))
        else:
            v = v + o["x2"].float() @ w[:, K1:].T.float()
    one, zero = torch.ones(1), torch.zeros(1)
    bi = o["bias"] if o["bias"] is not None else zero
    sv = o["bscale"][:, None, :] if o["bscale"] is not None else one
    rv = o["res"] if o["res"] is not None else zero
    if o["badd"] is not None:
        if fault == "badd_by_row":
            m = torch.arange(c.M).reshape(c.B, c.Lout) % c.B
            av = o["badd"][m]
        else:
            av = o["badd"][:, None, :]
    else:
        av = zero
    y = ((v + bi) + rv) * sv + av if fault == "bscale_after_res" else (v + bi) * sv + rv + av
    y = y.float()
    if c.act == 1:
        y = y.clamp_min(0.0)
    elif c.act >= 2:
        yd = y.double()                                                         # the library functions: exact here, C_ACT on the device
        y = act64(yd, c.act).float()
    if not stored:
        return y
    return y if c.out_f32 else round_to(y, R.STORE[c.dtype])


def emulate_row32(stored: torch.Tensor):
    """row32_stats on (M, N) fp32 stored values -> (mean, M2), each (M, N / 32) fp32."""
    M, N = stored.shape
    x = stored.float().reshape(M, N // 32, 8, 4)
    mean = _sum8((x[..., 0] + x[..., 1]) + (x[..., 2] + x[..., 3])) * (1.0 / 32.0)
    q = torch.zeros(M, N // 32, 8)
    for e in range(4):
        d = x[..., e] - mean[..., None]
        q = _fma(d, d, q)
    return mean, _sum8(q)


def emulate_gnpart(stored: torch.Tensor, Lout: int, fault: str = "") -> torch.Tensor:
    """gn_tile_stats on the rows' row32_stats -> (mt, nt, 2, 2) fp32.  Rows >= M repeat row M - 1 here (the kernel computes them from loads
    clamped to the last row: they are no zeros, which a segment of them would hide behind its (0, 0))."""
    M, N = stored.shape
    mtiles, nt = (M + 31) // 32, N // 32
    mean, m2 = emulate_row32(stored)
    pad = mtiles * 32 - M
    mean = torch.cat([mean, mean[-1:].expand(pad, nt)]).numpy().astype(np.float32)
    m2 = torch.cat([m2, m2[-1:].expand(pad, nt)]).numpy().astype(np.float32)
    out = np.zeros((mtiles * nt, 2, 2), dtype=np.float32)
    f32 = np.float32
    for mt in range(mtiles):
        m0 = mt * 32
        rb = min((m0 // Lout + 1) * Lout - m0, 32)
        if fault == "seg_plus":
            rb = min(rb + 1, 32)
        elif fault == "seg_minus":
            rb = max(rb - 1, 1)
        top = 32 if fault == "rows_past_M" else min(32, M - m0)
        for seg in range(2):
            lo, hi = (0, rb) if seg == 0 else (rb, max(rb, top))
            k = hi - lo
            t1, t2 = np.zeros(nt, f32), np.zeros(nt, f32)
            p = mean[m0 + lo] if k > 0 else np.zeros(nt, f32)
            for r in range(lo, hi):
                d = mean[m0 + r] - p
                t1 = t1 + d
                term = m2[m0 + r] if fault == "no_32d2" else (f32(32.0) * d).astype(np.float64) * d.astype(np.float64) + m2[m0 + r].astype(np.float64)
                t2 = t2 + term.astype(f32)
            dk = t1 / f32(k) if k > 0 else np.zeros(nt, f32)
            t2 = ((f32(-32.0) * t1).astype(np.float64) * dk.astype(np.float64) + t2.astype(np.float64)).astype(f32)
            if fault != "no_clamp":
                t2 = np.maximum(t2, f32(0.0))
            t1 = p + dk
            s = 1 - seg if fault == "swapped" else seg
            for n in range(nt):
                idx = n * mtiles + mt if fault == "transposed" else mt * nt + n
                out[idx, s, 0] = t1[n]
                out[idx, s, 1] = t2[n]
    return torch.from_numpy(out.reshape(mtiles, nt, 2, 2))


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm consumer
# ---------------------------------------------------------------------------------------------------------------------------------
def ln_operands(c: LnCase, seed: int = 0) -> dict:
    g = torch.Generator().manual_seed(seed)
    T = R.STORE[c.dtype]
    o = {"x": nx.row_input(c.B, c.L, c.C, f"offset:{c.ratio}", g, TORCH_DT[T]) if c.ratio else clip_input(c.B, c.L, c.C, g, T)}
    w = torch.randn(c.N, c.C, generator=g) / math.sqrt(c.C)
    o["w"] = w.contiguous()
    o["w_op"] = round_to(w, T)
    o["bias"] = torch.randn(c.N, generator=g) * 0.1
    o["ss"] = 0.3 * torch.randn(c.B, 2 * c.C, generator=g) if c.form in ("ss", "ss_res") else None
    return o


def ln_part64(x: torch.Tensor):
    """The fp64 partials (mean_j, M2_j, a_j) of the source rows, (M, C / 32) each."""
    return row_stats64(x.reshape(-1, x.shape[-1]))


def ln_ref(c: LnCase, o: dict, src: torch.Tensor, e_in: torch.Tensor, q_in: float, label: str):
    """(ref, bound) in fp64, (M, N): the module docstring's LAYERNORM CONSUMER gate for the source `src` (B, L, C) as the launch reads it.
    e_in (M, C / 32): the absolute error bound of each partial mean handed to the launch; q_in: the relative one of each partial M2."""
    Mr, Cc, N = c.M, c.C, c.N
    x = src.double().reshape(Mr, Cc)
    w = o["w_op"].double()
    mean_j, _, _ = row_stats64(x)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    eps = LN_EPS
    r = 1.0 / torch.sqrt(var + eps)
    dmean = N_SUM[family(label)] * u * mean_j.abs().mean(-1, keepdim=True) + e_in.mean(-1, keepdim=True)
    v_e = (64 * (mean_j - mu).abs() * e_in + 66 * e_in * e_in).sum(-1, keepdim=True) / Cc
    e_rstd = (12 * u + q_in) / 2 + 4 * u + (dmean ** 2 + v_e) / (2 * (var + eps))
    bias = o["bias"].double()
    split = c.dtype == "fp32x" and R.is_split(label)
    fl = R.X3_FLOOR if split else 0.0
    gK = gamma(Cc, c.dtype, label)
    T = R.STORE[c.dtype]
    b_of = torch.arange(Mr) // c.L
    if c.form == "acc":
        acc = x @ w.T
        colsum = w.sum(-1)[None, :]
        Wabs = w.abs().sum(-1)[None, :]
        A_raw = x.abs().clamp_min(fl) @ w.abs().clamp_min(fl).T
        ref_v = r * (acc - mu * colsum)
        bound_v = r * (gK * A_raw + mu.abs() * (Cc - 1) * u * Wabs + dmean * colsum.abs() + 3 * u * (acc.abs() + (mu * colsum).abs())) + e_rstd * ref_v.abs()
        ref = ref_v + bias
        bound = U[T] * ref.abs() + bound_v + gK * bias.abs()
        return ref, bound
    if o["ss"] is not None:
        sc1 = 1.0 + o["ss"].double()[b_of, :Cc]
        sh = o["ss"].double()[b_of, Cc:]
    else:
        sc1, sh = torch.ones(Mr, Cc, dtype=torch.float64), torch.zeros(Mr, Cc, dtype=torch.float64)
    a = (x - mu) * r * sc1 + sh
    uop = U[T] if T != "fp32" else 0.0
    da = (e_rstd + 4 * u) * (x.abs() + mu.abs()) * r * sc1.abs() + r * dmean * sc1.abs() + u * sh.abs() + uop * a.abs()
    ref_v = a @ w.T
    bound_v = da @ w.abs().T + gK * (a.abs().clamp_min(fl) @ w.abs().clamp_min(fl).T)
    ref = ref_v + bias
    bound = bound_v + gK * bias.abs()
    if c.form == "ss_res":
        ref = ref + a
        bound = bound + (e_rstd + 4 * u) * (x - mu).abs() * r * sc1.abs() + r * dmean * sc1.abs() + u * sh.abs() + gK * a.abs()
    return ref, U[T] * ref.abs() + bound


def ln_inputs_direct(src: torch.Tensor):
    """ln_part computed in fp64 from the source and rounded to fp32: (part (M, C / 32, 2) fp32, e_in, q_in)."""
    mean, m2, _ = ln_part64(src)
    part = torch.stack([mean, m2], -1).float()
    return part, u * mean.abs(), u


def ln_inputs_chained(src: torch.Tensor):
    """The error bounds of partials a producer's row32_stats wrote for `src` (its stored output): the ROWPART gate."""
    _, _, a = ln_part64(src)
    return 6 * u * a, 10 * u


def emulate_ln(c: LnCase, o: dict, src: torch.Tensor, part: torch.Tensor, label: str, fault: str = "") -> torch.Tensor:
    """ln_pool_row + ln_fold (accumulator side) or conv_gemm_fast's operand transform, then + bias and one rounding: (M, N) fp32."""
    Mr, Cc, N, nt = c.M, c.C, c.N, c.C // 32
    T = R.STORE[c.dtype]
    x = src.float().reshape(Mr, Cc)
    mp = torch.zeros(Mr, 32)
    qp = torch.zeros(Mr, 32)
    mp[:, :nt] = part[..., 0]
    qp[:, :nt] = part[..., 1]
    mp, qp = mp.reshape(Mr, 4, 8), qp.reshape(Mr, 4, 8)                          # [j][t8]: partial t8 + 8 j
    on = (torch.arange(32).reshape(4, 8) < nt)[None]
    if family(label) in ("wp", "rs"):
        sm = (mp[:, 0] + mp[:, 1]) + (mp[:, 2] + mp[:, 3])
    else:
        sm = ((mp[:, 0] + mp[:, 1]) + mp[:, 2]) + mp[:, 3]
    mean = _sum8(sm) / (32.0 if fault == "mean_div_32" else float(nt))
    dq = torch.zeros(Mr, 8)
    for j in range(4):
        d = mp[:, j] - mean[:, None]
        dq = torch.where(on[:, j], dq + _fma(32.0 * d, d, qp[:, j]), dq)
    rstd = (1.0 / torch.sqrt((_sum8(dq) / float(Cc) + LN_EPS).double())).float()
    mean, rstd = mean[:, None], rstd[:, None]
    w = o["w_op"].float()
    split = c.dtype == "fp32x" and R.is_split(label)

    def mm(a):
        if split:
            ah, al = R.x3_split(a)
            wh, wl = R.x3_split(w.T.contiguous())
            return ah @ wh + (ah @ wl + al @ wh) * (1.0 / 2048.0)
        return a @ w.T

    if c.form == "acc":
        cu = w.sum(-1)[None, :]
        if fault == "cu_first_column":
            cu = cu.reshape(1, N // 4, 4)[..., :1].expand(1, N // 4, 4).reshape(1, N)
        v = rstd * (mm(x) - mean * cu)
        return round_to(v + o["bias"], T)
    b_of = torch.arange(Mr) // c.L
    if o["ss"] is not None:
        A = rstd * (1.0 + o["ss"][b_of, :Cc])
        sh = o["ss"][b_of, Cc:]
        a = _fma(x, A, _fma(-mean.expand_as(A), A, sh))
    else:
        a = _fma(x, rstd.expand_as(x), (-mean * rstd).expand_as(x))
    a_op = round_to(a, T)
    v = mm(a_op) + o["bias"]
    if c.form == "ss_res":
        v = v + (_fma((x - mean) * rstd, 1.0 + o["ss"][b_of, :Cc], o["ss"][b_of, Cc:]) if o["ss"] is not None else (x - mean) * rstd)
    return round_to(v, T)


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI: descriptor and queries (no device needed for the queries)
# ---------------------------------------------------------------------------------------------------------------------------------
PROBE = 256          # an aligned non-null pointer: only whether an optional pointer is set enters a plan


def desc_of(dtype: str, B: int, L: int, C: int, C2: int, N: int, taps: int = 1, stride: int = 1, pad: int = 0, up: int = 1, act: int = 0,
            out_f32: bool = False, mt_ln: bool = False, res_ln: bool = False, ln_operand: bool = False, solo: bool = True, ln_eps: float = LN_EPS, **ptrs):
    """An sf_conv1d_epi_desc; ptrs: x, x2, w, bias, bscale, badd, residual, out, rowpart, gnpart, ln_part, ln_ss as integers (or None)."""
    from syncfusion_amd import _lib as _l

    d = _l.Conv1dEpiDesc()
    d.dtype = _l.DTYPES[dtype]
    d.B, d.L, d.C, d.C2, d.N, d.taps, d.stride, d.pad, d.upsample, d.act = B, L, C, C2, N, taps, stride, pad, up, act
    d.out_f32, d.mt_ln, d.res_ln, d.ln_operand, d.solo, d.ln_eps = int(out_f32), int(mt_ln), int(res_ln), int(ln_operand), int(solo), ln_eps
    for k, v in ptrs.items():
        setattr(d, k, v)
    return d


def epi_desc(c: EpiCase, **ptrs):
    return desc_of(c.dtype, c.B, c.L, c.C, c.C2, c.N, c.taps, c.stride, c.pad, c.up, c.act, c.out_f32, c.mt_ln, **ptrs)


def epi_probe_ptrs(c: EpiCase) -> dict:
    p = dict(x=PROBE, w=PROBE, out=PROBE)
    for key, flag in (("x2", c.C2 > 0), ("bias", "b" in c.ops), ("bscale", "s" in c.ops), ("residual", "r" in c.ops), ("badd", "a" in c.ops),
                      ("rowpart", c.want_row), ("gnpart", c.want_gn)):
        if flag:
            p[key] = PROBE
    return p


def query_epi(d):
    """(rc, label, rowpart, gnpart) of sf_op_conv1d_epi_variant."""
    import ctypes as C

    from syncfusion_amd import _lib as _l

    buf, row, gn = C.create_string_buffer(96), C.c_int(-1), C.c_int(-1)
    rc = _l.load().sf_op_conv1d_epi_variant(C.byref(d), buf, 96, C.byref(row), C.byref(gn))
    return rc, buf.value.decode(), bool(row.value == 1), bool(gn.value == 1)


def ln_desc(c: LnCase, **ptrs):
    return desc_of(c.dtype, c.B, c.L, c.C, 0, c.N, ln_operand=c.form != "acc", res_ln=c.form == "ss_res", **ptrs)


def ln_probe_ptrs(c: LnCase) -> dict:
    p = dict(x=PROBE, w=PROBE, out=PROBE, bias=PROBE, ln_part=PROBE)
    if c.form in ("ss", "ss_res"):
        p["ln_ss"] = PROBE
    if c.form == "ss_res":
        p["residual"] = PROBE
    return p


def query_ln(d):
    """(rc, label, rowpart) of sf_op_conv1d_ln_variant."""
    import ctypes as C

    from syncfusion_amd import _lib as _l

    buf, row = C.create_string_buffer(96), C.c_int(-1)
    rc = _l.load().sf_op_conv1d_ln_variant(C.byref(d), buf, 96, C.byref(row))
    return rc, buf.value.decode(), bool(row.value == 1)
