"""fp64 reference, per-element gate and CPU emulation for the op-level 1-D convolution (sf_op_conv1d_cl, groups = 0): the MFMA implicit-GEMM
families (conv_gemm_mt / rs / wp / fast / sk / v2 and the classic conv_gemm tiles) and conv_direct.

The kernel-level tests (test_gpu_ops.py) compare whole tensors by rel-L2; one wrong 32x32 tile of 10^6 outputs passes them.  Here every
output element of one launch is held to a bound derived from the arithmetic, by the method of onset_layers_ref.py (whose U, C_ACC, U24,
round_to and round_once are imported, not copied).

Operands, restated from csrc/capi_misc.cpp conv1d_cl_impl (T = the storage type of `dtype`; fp32x stores fp32):
  * x (B, L, C) and the residual (B, Lout, N) are GIVEN in T (channels-last): operands() rounds them once and both sides read those values;
  * the weight arrives as fp32 (N, C, taps).  GEMM path (C % 32 == 0): launch_pack_conv(wdt = T, ..., scale = nullptr) stores (T)w, a plain
    conversion -- no scale is multiplied in, so there is no one-or-two-roundings ambiguity and no flip term (onset_layers_ref.py needs one only
    because it folds a BatchNorm scale).  fp32 / fp32x: the fp32 weight itself (fp32x splits it on the device, below).
    conv_direct path (C % 32 != 0): wdt = F32 whatever T is, the kernel multiplies T activations by fp32 weights;
  * the bias stays fp32 and is added to the fp32 accumulator.
Geometry: nearest upsample of the source by `up` (source row = p >> log2(up)), then Conv1d(taps, stride, pad) with zero padding per clip,
Lout = (L * up + 2 * pad - taps) / stride + 1.

Gate, per element, no element exempt, no sampled subset, dev finite everywhere (the output buffer is NaN-filled before the launch):
    |dev_i - ref_i| <= u_T |ref_i| + gamma A_i,     ref = conv(x, w) + bias + res,   A = conv(|x|, |w|) + |bias| + |res|     (fp64)
  * u_T |ref|: the ONE rounding of the stored output.  Every family keeps its accumulators in fp32 up to the store: the macro tiles park the
    fp32 tile in LDS, the split-K kernels (sk / fast / wp / rs) reduce fp32 partials, and each kernel has one from_f<T> at its store.  So no
    launch path stores through an intermediate 16-bit rounding and SECOND_ROUNDING is empty; a path listed there would get 2 u_T.
  * gamma A: fp32 accumulation of K = taps * C products, then + bias, then + residual: K + 2 roundings on the path of any term, in ANY
    order (tile shape, K split and MFMA operand order need no allowance); the (K + 3)rd unit covers the second-order terms of (1 + u)^(K+2)
    for K + 2 <= 2^12 (the case tables keep K <= 3072).
      - fp32 GEMMs and conv_direct: gamma = (K + 3) 2^-24.  v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain (one rounding per product, with
        its add); conv_direct accumulates with explicit fmaf.  Every add is round-to-nearest: c = 1.
      - 16-bit GEMMs: gamma = 2 (K + 3) 2^-24.  Products of two 16-bit values are exact in fp32; how the 16-bit-input MFMA rounds the sum of
        its 16 products into the fp32 accumulator is not documented, so truncation is taken as possible: c = 2, the same choice and the same
        reasoning as onset_layers_ref.py (C_ACC), not a measurement.
      - fp32x, on the families that honour the split image (label "<x3"; the others multiply in fp32 and get the fp32 gamma):
            gamma = (K + 3) 2^-24 + X3_MULT(K) 2^-22,      X3_MULT(K) = (K + 3) / 4 + 3 + 1 / 64 + (K + 3) / 512
        Derivation, from common.h x3_split1<X3_F16> and the accumulation "accM += hi_a hi_b; accL += hi_a lo'_b + lo'_a hi_b;
        result = accM + accL / 2048" (the lo lo product is dropped).  For an fp32 operand a:  hi = fp16(a),  r = a - hi is exact in fp32 (hi
        keeps the leading bits of a), 2048 r is exact, lo' = fp16(2048 r), lo = lo' / 2048.  Write m(a) = max(|a|, 2^-14).
          |a| >= 2^-14 (hi normal): |r| <= 2^-11 |a|.  If 2048 |r| >= 2^-14, lo' is a normal fp16 and |lo - r| <= 2^-11 |r| <= 2^-22 |a|; if
          not, lo' is SUBNORMAL, rounded to a multiple of 2^-24 with error <= 2^-25, so |lo - r| <= 2^-36 <= 2^-22 |a|.
          |a| < 2^-14 (hi itself subnormal): |r| <= 2^-25, 2048 |r| <= 2^-14, |lo - r| <= 2^-36 = 2^-22 2^-14.
        So a = hi + lo + d_a with |d_a| <= 2^-22 m(a) and |lo| <= (2^-11 + 2^-22) m(a).  The product the kernel forms differs from a b by
            a b - (hi_a hi_b + hi_a lo_b + lo_a hi_b) = a d_b + b d_a - d_a d_b + lo_a lo_b,
        at most (2^-22 + 2^-22 + 2^-44 + 2^-22 (1 + 2^-11)^2) m(a) m(b) <= (3 + 2^-9) 2^-22 m(a) m(b).  That is the "3".
        Accumulation.  hi hi (22 bits) is exact in fp32 and accM is a sum of K such products through 16-bit-input MFMAs: c = 2 as above, on
        terms of magnitude |hi_a hi_b| <= (1 + 2^-11)^2 |a b|:  2 (K + 3) 2^-24 (1 + 2^-10 + 2^-22) sum m m
            <= [(K + 3) 2^-24 + ((K + 3) / 4 + (K + 3) / 2048) 2^-22] sum m m  -- the fp32 gamma plus "(K + 3) / 4" plus a sliver.
        accL sums 2 K exact products of total magnitude <= 2 (2^-11 + 2^-22) 2048 sum m m = 2 (1 + 2^-11) sum m m; its accumulation error,
        c = 2 over 2 K terms, then divided by 2048 (exact), is <= 2 (2 K + 1) 2^-24 2 (1 + 2^-11) 2^-11 sum m m <= ((K + 3) / 1024) 2^-22 sum m m.
        The combination accM + accL / 2048, the bias and the residual are three of the K + 3 units already counted.  Altogether
            X3_MULT(K) = (K + 3) / 4 + 3 + 1 / 64 + (K + 3) / 512       (1 / 64 >= 2^-9;  1 / 512 >= 1 / 1024 + 1 / 2048),
        which is what x3_mult() returns, and sum m m <= A with A formed from m(x), m(w).
        Input range over which this holds: |a| < 65520 for every activation and weight, so that hi = fp16(a) does not overflow (the kernel's
        own limit, common.h); operands below 2^-14 in magnitude, zeros included, count as 2^-14 in A -- conv1d_ref(floor = 2^-14) forms A from
        m(x), m(w), which is what gate() is given for fp32x.  operands() draws |x| < 10 and |w| < 6.
  * fp16 outputs below 2^-14 are subnormal and round with error up to 2^-25 rather than u |ref|; as in onset_layers_ref.py no term is added:
    gamma A covers it wherever A >= 2^-25 / (2 (K + 3) 2^-24), at most 0.0625 for K >= 1 here, and A is of order 1 for the operands drawn.

No constant above is fitted to a device measurement.  Plain module (not a conftest): the tests import it like helpers.py and numerics.py.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Tuple

import torch

from onset_layers_ref import C_ACC, U, U24, round_once, round_to   # noqa: F401  (round_once: for callers that round fp64 values)

STORE = {"fp32": "fp32", "fp32x": "fp32", "bf16": "bf16", "fp16": "fp16"}      # the storage type T of a dtype name
SECOND_ROUNDING: Tuple[str, ...] = ()      # kernel labels that store through an intermediate 16-bit rounding: none (module docstring)
X3_FLOOR = 2.0 ** -14                       # m(a) = max(|a|, 2^-14) in A for the split families
K_MAX = 4094                                # (K + 3) 2^-24 covers the second-order terms up to here


class Case(NamedTuple):
    """One row of a case table: the arguments of sf_op_conv1d_cl (groups = 0) and the kernel the dispatcher must pick for them."""
    dtype: str
    B: int
    L: int
    C: int
    N: int
    taps: int
    stride: int
    pad: int
    up: int
    residual: bool
    expected_label: str

    @property
    def K(self) -> int:
        return self.taps * self.C

    @property
    def Lout(self) -> int:
        return (self.L * self.up + 2 * self.pad - self.taps) // self.stride + 1

    @property
    def M(self) -> int:
        return self.B * self.Lout

    def ref_gflop(self) -> float:
        """fp64 work of conv1d_ref (ref and A)."""
        return 2 * 2.0 * self.M * self.N * self.K / 1e9


def is_split(label: str) -> bool:
    return "<x3" in label


def x3_mult(K: int) -> float:
    return (K + 3) / 4.0 + 3.0 + 1.0 / 64.0 + (K + 3) / 512.0


def gamma(K: int, dtype: str, label: str) -> float:
    """The accumulation coefficient of the gate for a launch of `label` in `dtype` (module docstring)."""
    assert K <= K_MAX, f"K = {K}: the first-order bound is written for K <= {K_MAX}"
    if dtype == "fp32x":
        return (K + 3) * U24 + (x3_mult(K) * 2.0 ** -22 if is_split(label) else 0.0)
    return (1 if label == "conv_direct" else C_ACC[dtype]) * (K + 3) * U24      # conv_direct: fmaf in fp32 whatever the storage type


def source_rows(Lout: int, L: int, taps: int, stride: int, pad: int, up: int):
    """(idx, ok), each (taps, Lout): the source row tap t of output position l reads, and whether it is inside the (upsampled) clip."""
    l = torch.arange(Lout).reshape(1, -1)
    p = l * stride - pad + torch.arange(taps).reshape(-1, 1)
    ok = (p >= 0) & (p < L * up)
    return torch.div(p.clamp(0, L * up - 1), up, rounding_mode="floor"), ok


def gathered(x: torch.Tensor, taps: int, stride: int, pad: int, up: int) -> torch.Tensor:
    """The implicit GEMM's A operand made explicit: (B, L, C) -> (B, Lout, taps * C), k = tap * C + c, zeros where padding is read."""
    B, L, C = x.shape
    Lout = (L * up + 2 * pad - taps) // stride + 1
    idx, ok = source_rows(Lout, L, taps, stride, pad, up)
    g = x[:, idx.reshape(-1)].reshape(B, taps, Lout, C) * ok.reshape(1, taps, Lout, 1).to(x.dtype)
    return g.permute(0, 2, 1, 3).reshape(B, Lout, taps * C)


def weight_matrix(w: torch.Tensor) -> torch.Tensor:
    """(N, C, taps) PyTorch layout -> (taps * C, N), k = tap * C + c."""
    return w.permute(2, 1, 0).reshape(-1, w.shape[0])


def conv1d_ref(x, w, bias, res, taps: int, stride: int, pad: int, up: int, floor: float = 0.0):
    """(ref, A) in fp64, channels-last: x (B, L, C), w (N, C, taps), bias (N) or None, res (B, Lout, N) or None -> (B, Lout, N).
    ref = conv(nearest_up(x), w) + bias + res;  A = conv(|x|, |w|) + |bias| + |res|, with operand magnitudes raised to `floor` first
    (fp32x: X3_FLOOR; padding rows stay zero).  The operands are taken as they are: round them first (operands())."""
    assert w.shape[2] == taps and w.shape[1] == x.shape[2]
    xd, wd = x.double(), w.double()
    ref = gathered(xd, taps, stride, pad, up) @ weight_matrix(wd)
    A = gathered(xd.abs().clamp_min(floor), taps, stride, pad, up) @ weight_matrix(wd.abs().clamp_min(floor))
    if bias is not None:
        ref += bias.double()
        A += bias.double().abs()
    if res is not None:
        ref += res.double()
        A += res.double().abs()
    return ref, A


def operands(case: Case, seed: int = 0):
    """Seeded operands as test_gpu_ops._conv_case draws them (x ~ 1.5 randn + 0.3, w ~ randn / sqrt(K), bias ~ 0.1 randn, res ~ randn), in the
    values the op reads: x and res rounded to T; `w` is the fp32 weight handed to the C ABI and `w_op` what the kernel multiplies by -- (T)w
    on the GEMM path, w itself on the conv_direct path (C % 32 != 0) and for fp32 / fp32x.  All fp32, channels-last."""
    g = torch.Generator().manual_seed(seed)
    T = STORE[case.dtype]
    x = round_to(torch.randn(case.B, case.L, case.C, generator=g) * 1.5 + 0.3, T)
    w = torch.randn(case.N, case.C, case.taps, generator=g) / math.sqrt(case.K)
    bias = torch.randn(case.N, generator=g) * 0.1
    res = round_to(torch.randn(case.B, case.Lout, case.N, generator=g), T) if case.residual else None
    w_op = round_to(w, T) if case.C % 32 == 0 else w
    return x, w, w_op, bias, res


def case_ref(case: Case, ops):
    x, _, w_op, bias, res = ops
    return conv1d_ref(x, w_op, bias, res, case.taps, case.stride, case.pad, case.up, X3_FLOOR if case.dtype == "fp32x" and is_split(case.expected_label) else 0.0)


def x3_split(a: torch.Tensor):
    """common.h x3_split1<X3_F16> in fp32: (hi, lo') with hi = fp16(a), lo' = fp16((a - hi) * 2048), both carried in fp32."""
    hi = a.float().half().float()
    return hi, ((a.float() - hi) * 2048.0).half().float()


def emulate(x, w_op, bias, res, taps: int, stride: int, pad: int, up: int, dtype: str, label: str, stored: bool = True, parts: bool = False):
    """What a correct kernel computes, channels-last fp32: the same rounded operands, fp32 accumulation, bias and residual added in fp32,
    ONE output rounding (stored = False: the fp32 value before it).  Split families of fp32x: the three products of the split operands in
    two fp32 accumulators, accM + accL / 2048, as coded (parts = True returns (accM, accL) instead, for the tests that take one away)."""
    g, wm = gathered(x.float(), taps, stride, pad, up), weight_matrix(w_op.float())
    if dtype == "fp32x" and is_split(label):
        gh, gl = x3_split(g)
        wh, wl = x3_split(wm)
        accM, accL = gh @ wh, gh @ wl + gl @ wh
        if parts:
            return accM, accL
        y = accM + accL * (1.0 / 2048.0)
    else:
        y = g @ wm
    if bias is not None:
        y = y + bias.float()
    if res is not None:
        y = y + res.float()
    return round_to(y, STORE[dtype]) if stored else y


def case_emulate(case: Case, ops, stored: bool = True):
    x, _, w_op, bias, res = ops
    return emulate(x, w_op, bias, res, case.taps, case.stride, case.pad, case.up, case.dtype, case.expected_label, stored)


def bound_of(ref, A, K: int, dtype: str, label: str):
    return ((2 if label in SECOND_ROUNDING else 1) * U[STORE[dtype]]) * ref.abs() + gamma(K, dtype, label) * A


def rel_l2(d, ref) -> float:
    return float((d.double() - ref).norm() / ref.norm().clamp_min(1e-300))


def gate(dev, ref, A, K: int, dtype: str, label: str, what: str, quiet: bool = False) -> Tuple[float, float]:
    """Assert |dev - ref| <= u_T |ref| + gamma A for EVERY element of (B, Lout, N) tensors, dev finite everywhere.  Prints and returns
    (max err / bound, whole-tensor rel-L2); the failure names the worst element as (clip, position, channel) with got / ref / A, the number
    of elements over the bound, the rel-L2 and the kernel label."""
    d = dev.detach().double().cpu()
    assert d.shape == ref.shape == A.shape, f"{what}: shapes {tuple(d.shape)} / {tuple(ref.shape)} / {tuple(A.shape)}"
    _, Lo, N = d.shape

    def where(i: int) -> str:
        b, l, n = i // (Lo * N), (i // N) % Lo, i % N
        return f"(clip {b}, position {l}, channel {n}): got {float(d[b, l, n]):.9g}, ref {float(ref[b, l, n]):.9g}, A {float(A[b, l, n]):.4g}"

    bad = ~torch.isfinite(d)
    if bool(bad.any()):
        raise AssertionError(f"{what} [{label}]: {int(bad.sum())} non-finite outputs of {d.numel()}, first at {where(int(bad.flatten().nonzero()[0]))}")
    err = (d - ref).abs_()
    rel = float(err.norm() / ref.norm().clamp_min(1e-300))
    bound = bound_of(ref, A, K, dtype, label)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)        # 0 / 0 = 0, x / 0 = inf
    worst = int(ratio.flatten().argmax())
    r = float(ratio.flatten()[worst])
    if not quiet:
        print(f"{what} [{label}]: err/bound {r:.3f}, rel-L2 {rel:.3e}, K {K}, {d.numel()} elements")
    assert r <= 1.0, (f"{what} [{label}]: err/bound {r:.3f} > 1 at {where(worst)}; {int((ratio > 1).sum())} of {d.numel()} elements over the bound, "
                      f"rel-L2 {rel:.3e}, kernel {label}")
    return r, rel
