"""fp64 references, two per-element gates and a CPU emulation for the training backward of the op-level 1-D convolution
(sf_op_conv1d_bwd_cl_x, groups = 0): the data gradient (the forward GEMM families on the flipped / transposed weight written by
pack_dgrad_kernel, or conv_direct), the weight gradient (conv_wgrad_kernel, conv_wgrad_lds_kernel, conv_wgrad_x3_kernel, their row splits and
the two reducers) and the bias gradient (the column-sum kernels and their slice reduction, alone or riding on the weight gradient's reducer).

test_gpu_train.py holds these to a whole-tensor rel-L2 of 2e-5 against fp32 autograd on shapes that reach a few of the launch paths.  Here
every element of dx, dw and db of one call is checked, the call's launch plan (sf_op_conv1d_bwd_variant) is asserted first, and the case
tables of test_gpu_conv1d_bwd_elementwise.py reach every path.  U24, C_ACC, round_to and gathered come from conv1d_ref.py.

References, channels-last, fp64, from the fp32 operands x (B, L, C), w (N, C, taps), dy (B, L, N); "same" padding, 2 pad = taps - 1:
    dw[n, c, t] = sum_{b, l} dy[b, l, n] x[b, l + t - pad, c]        (terms whose row leaves the clip are dropped)
    db[n]       = sum_{b, l} dy[b, l, n]
    dx[b, l, c] = sum_{n, t} dy[b, l - t + pad, n] w[n, c, t]
and A, the same sums over absolute values.

EXACT GATE (exact_operands, exact_gate).  x, w and dy are drawn from {-3, -2, -1, 1, 2, 3}: no operand is zero, and the only zeros a kernel
may meet are the ones it must put in itself -- padding rows, rows past a slice's end, columns past a ragged tile -- whose place depends on the
position.  Every product and every partial sum is an integer below 2^24 in magnitude (asserted per case: max A < 2^24), hence exact in fp32
in any order; the bf16 split of such an operand is hi = a, lo = 0, so the split kernels are exact as well.  The device must equal the fp64
reference BIT FOR BIT.  Since no operand is zero, a dropped, doubled or misplaced term changes the element it belongs to.  This is the gate
that gives the 16 K-row, 64-slice cases their meaning: a rounding bound at that length would let whole rows go missing.

ROUNDING GATE (operands, rounding_gate).  x ~ 1.5 randn + 0.3, w ~ randn / sqrt(taps C), dy ~ scale randn.  |dev - ref| <= gamma A for every
element, dev finite everywhere.  gamma, from the code (u = 2^-24; nothing is fitted to a device run):
  * fp32 weight gradient (wgrad_thin, wgrad_lds, and every kernel of the fp32 mode): v_mfma_f32_32x32x2f32 is a k-ordered fmaf chain, one
    rounding per accumulated product (c = 1), over at most R = B L rows; conv_wgrad_kernel then sums its four waves through LDS (at most 3
    more roundings) and the reducer adds at most S slices.  gamma = (R + S + 6) u; the spare units cover the second-order terms of
    (1 + u)^(R + S + 3) for R + S + 6 <= K_MAX.
  * bias gradient: a sum of R terms in fp32.  The slices, the per-thread strides and the LDS merges only change the shape of the summation
    tree, and accumulators start from an exact zero: no term passes more than R - 1 roundings.  gamma = (R + 1) u.
  * fp32 data gradient: as the forward convolution with K = taps N and neither bias nor residual kept apart: gamma = (K + 3) u, for
    conv_direct (explicit fmaf) and for every fp32 GEMM label.
  * split bf16 launches -- wgrad_x3<TW> and data-gradient labels with "<x3" in them (common.h x3_split1<X3_BF16>, x3_mfma1_bf16):
        hi = bf16(a),  r = a - hi (exact in fp32: hi keeps the leading 8 bits of a),  lo = bf16(r),  acc += lo_a hi_b + hi_a lo_b + hi_a hi_b.
    bf16 has unit roundoff 2^-9: |r| <= 2^-9 |a|, |lo - r| <= 2^-9 |r|, so a = hi + lo + d with |d| <= 2^-18 |a| and
    |lo| <= 2^-9 (1 + 2^-9) |a|.  What the kernel forms differs from a b by
        a b - (hi_a hi_b + hi_a lo_b + lo_a hi_b) = a d_b + b d_a - d_a d_b + lo_a lo_b,
    at most (2^-18 + 2^-18 + 2^-36 + 2^-18 (1 + 2^-9)^2) |a b| <= (3 + 2^-7) 2^-18 |a b|.
    Accumulation: a product of two bf16 values has 16 significant bits and is exact in fp32; ONE accumulator takes all 3 n of them (n = the
    chain length: R rows for the weight gradient, K = taps N for the data gradient).  How the 16-bit-input MFMA rounds its 16 products into
    the fp32 accumulator is not documented, so truncation is taken as possible: c = 2 per term, as in conv1d_ref.py.  The terms' magnitudes
    sum to at most (1 + 2^-9)^2 (1 + 2^-8) |a b| <= (1 + 2^-7 + 2^-15) |a b|, so the accumulation costs at most 2 * 3 n u (1 + 2^-7 + 2^-15)
    sum |a b| to first order, and 6 n (1 + 2^-6) u with the second-order terms for 6 n u <= 2^-8 (n <= K_MAX).  The kernels of the data
    gradient that keep two accumulators add them once: one more unit.  Altogether
        gamma_x3(n, extra) = (3 + 2^-7) 2^-18 + (6 n (1 + 2^-6) + extra) u,     extra = S + 6 (weight gradient), 3 (data gradient).
    Operand range: |a| below the largest bf16 (3.39e38), and a - hi a NORMAL fp32 / bf16 number or zero, i.e. |a| >= 2^-117 or a = 0 (a
    zero splits into two zeros: no floor on A is needed, unlike the fp16 split of the forward pass).  The gradient scales 1e-9 ... 1e6 of
    the tests keep |dy| between 2^-60 and 2^30.  The bound is relative to A, so it does not move with the scale of dy.
  * The thin kernel has no split form (conv_wgrad_plan: x3 only with an LDS-staged family) and a data gradient whose label lacks "<x3"
    multiplies in fp32: both get the fp32 gamma in the fp32x mode.

The emulation (emulate_wgrad_partials, reduce_partials, emulate_dx, emulate_db) computes in fp32 what a correct kernel computes, slice by
slice as the label's S says, with the three split products in one fp32 sum for the split launches.  test_conv1d_bwd_elementwise_cpu.py runs
it through both gates and plants faults in it.

plan() restates the dispatch (family, S, rows per slice, reducer) in Python.  It serves only to describe the case table (how many trailing
slices own no rows); what a test EXPECTS is the literal label in its row, compared with sf_op_conv1d_bwd_variant.
Plain module (not a conftest): the tests import it like helpers.py and numerics.py.
"""
from __future__ import annotations

import math
import re
from typing import NamedTuple, Optional, Tuple

import torch

from conv1d_ref import C_ACC, K_MAX, U24, gathered, round_to   # noqa: F401  (C_ACC, round_to: re-exported for the tests)

X3_PRODUCT = (3.0 + 2.0 ** -7) * 2.0 ** -18     # |a b - (hi hi + hi lo + lo hi)| / |a b| for the bf16 split
OLD_REL_L2 = 2e-5                               # the whole-tensor gate of test_gpu_train.py (reported next to every planted fault)


class Case(NamedTuple):
    """One call of sf_op_conv1d_bwd_cl_x (groups = 0) and the launch plan the dispatcher must pick for it."""
    mode: str             # "fp32" | "fp32x"
    B: int
    L: int
    C: int
    N: int
    taps: int
    outs: str             # which of dx / dw / db are asked for: a subset of "xwb" (the others are passed as NULL)
    expected_label: str
    dy_scale: float = 1.0

    @property
    def pad(self) -> int:
        return (self.taps - 1) // 2

    @property
    def rows(self) -> int:
        return self.B * self.L

    @property
    def shape(self) -> Tuple[int, int, int, int, int]:
        return (self.B, self.L, self.C, self.N, self.taps)


def case_id(c: Case) -> str:
    return f"{c.mode}-B{c.B}-L{c.L}-C{c.C}-N{c.N}-k{c.taps}-{c.outs}" + (f"-dy{c.dy_scale:g}" if c.dy_scale != 1.0 else "")


_LABEL = re.compile(r"^dgrad (\S+) \| (\S+) S=(\d+) (direct|vec|scalar) \| db (vec4|vec1|generic) Sb=(\d+)$")


class Plan(NamedTuple):
    dgrad: str
    wgrad: str
    S: int
    reducer: str
    colsums: str
    Sb: int

    @property
    def wgrad_key(self) -> str:
        """wgrad kernel / staging, reducer and column-sum kernel: what the coverage sweep pins."""
        return f"{self.wgrad} {self.reducer} | db {self.colsums}"


def parse(label: str) -> Plan:
    m = _LABEL.match(label)
    assert m, f"not a backward label: {label!r}"
    return Plan(m.group(1), m.group(2), int(m.group(3)), m.group(4), m.group(5), int(m.group(6)))


def wgrad_split(plan: Plan) -> bool:
    return plan.wgrad.startswith("wgrad_x3")


def dgrad_split(plan: Plan) -> bool:
    return "<x3" in plan.dgrad


# ---------------------------------------------------------------------------------------------------------------------------------
# the dispatch restated (train.hip wgrad_family / conv_wgrad_splits / conv_wgrad_plan) -- describes the table, decides nothing
# ---------------------------------------------------------------------------------------------------------------------------------
def wgrad_family(C: int, N: int, taps: int) -> int:
    Q = taps * C
    if N < 64 or Q < 64 or C % 32 or N % 4 or taps > 9:
        return 0
    TW = 2 if (N >= 128 and Q >= 128) else 1
    T = 64 * TW
    if not (taps == 1 or C % T == 0 or C <= T):
        return 1 if TW == 2 and (C % 64 == 0 or C <= 64) else 0
    return TW


def plan(B: int, L: int, C: int, N: int, taps: int):
    """(family, S, rows per slice, trailing slices without rows, reducer) for the default split target."""
    rows, Q, fam = B * L, taps * C, wgrad_family(C, N, taps)
    T = 64 * fam if fam else 32
    tiles = ((N + T - 1) // T) * ((Q + T - 1) // T)
    S = max(1, (512 if fam else 2048) // max(tiles, 1))
    S = min(S, max(1, rows // 256), 512)
    rps = rows_per_slice(rows, S)
    empty = sum(1 for s in range(S) if s * rps >= rows)
    reducer = "direct" if S == 1 else ("vec" if C % 4 == 0 and (S < 64 or N * Q > 65536) else "scalar")
    return fam, S, rps, empty, reducer


def rows_per_slice(rows: int, S: int) -> int:
    return ((rows + S - 1) // S + 31) // 32 * 32


# ---------------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------------
def exact_operands(c: Case, seed: int = 0):
    """x, w, dy drawn from the non-zero integers -3 ... 3 (fp32)."""
    g = torch.Generator().manual_seed(seed)

    def draw(*shape):
        v = torch.randint(1, 4, shape, generator=g).float()
        return torch.where(torch.rand(shape, generator=g) < 0.5, -v, v)

    return draw(c.B, c.L, c.C), draw(c.N, c.C, c.taps), draw(c.B, c.L, c.N)


def operands(c: Case, seed: int = 0):
    """Real-valued operands as conv1d_ref.operands draws them: x ~ 1.5 randn + 0.3, w ~ randn / sqrt(taps C), dy ~ dy_scale randn (fp32)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(c.B, c.L, c.C, generator=g) * 1.5 + 0.3
    w = torch.randn(c.N, c.C, c.taps, generator=g) / math.sqrt(c.taps * c.C)
    dy = torch.randn(c.B, c.L, c.N, generator=g) * c.dy_scale
    return x, w, dy


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 references
# ---------------------------------------------------------------------------------------------------------------------------------
def dw_layout(m: torch.Tensor, C: int, taps: int) -> torch.Tensor:
    """(N, taps * C) with q = t * C + c  ->  PyTorch's (N, C, taps)."""
    return m.reshape(m.shape[0], taps, C).permute(0, 2, 1).contiguous()


def dgrad_matrix(w: torch.Tensor, flip: bool = True) -> torch.Tensor:
    """(N, C, taps) -> the data-gradient GEMM's weight (taps * N, C), k = t' * N + n, holding w[n, c, taps - 1 - t'] (pack_dgrad_kernel)."""
    wf = w.flip(2) if flip else w
    return wf.permute(2, 0, 1).reshape(-1, w.shape[1])


def wgrad_ref(x, dy, taps: int, pad: int):
    """(dw, A) in fp64, (N, C, taps)."""
    B, L, C = x.shape
    xd, dd = x.double(), dy.double().reshape(B * L, -1)
    dw = dd.t() @ gathered(xd, taps, 1, pad, 1).reshape(B * L, taps * C)
    A = dd.abs().t() @ gathered(xd.abs(), taps, 1, pad, 1).reshape(B * L, taps * C)
    return dw_layout(dw, C, taps), dw_layout(A, C, taps)


def db_ref(dy):
    d = dy.double().reshape(-1, dy.shape[2])
    return d.sum(0), d.abs().sum(0)


def dgrad_ref(dy, w, taps: int, pad: int):
    """(dx, A) in fp64, (B, L, C)."""
    dd, wd = dy.double(), w.double()
    dx = gathered(dd, taps, 1, taps - 1 - pad, 1) @ dgrad_matrix(wd)
    A = gathered(dd.abs(), taps, 1, taps - 1 - pad, 1) @ dgrad_matrix(wd.abs())
    return dx, A


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 emulation of a correct kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def bf16_split(a: torch.Tensor):
    """common.h x3_split1<X3_BF16>: hi = bf16(a), lo = bf16(a - hi), both carried in fp32."""
    hi = a.float().bfloat16().float()
    return hi, (a.float() - hi).bfloat16().float()


def x3_matmul(a: torch.Tensor, b: torch.Tensor, drop_lo_hi: bool = False) -> torch.Tensor:
    """a @ b as x3_mfma1_bf16 forms it: lo_a hi_b + hi_a lo_b + hi_a hi_b in one fp32 sum (drop_lo_hi: the first product lost -- a fault)."""
    ah, al = bf16_split(a)
    bh, bl = bf16_split(b)
    small = ah @ bl if drop_lo_hi else al @ bh + ah @ bl
    return small + ah @ bh


def emulate_wgrad_partials(x, dy, taps: int, pad: int, S: int, split: bool, drop_lo_hi: bool = False) -> torch.Tensor:
    """partial[s][n][q], q = t * C + c: the weight gradient of the rows of slice s (rows_per_slice rows each; trailing slices may own none
    and then hold zeros), fp32.  S = 1: the kernel writes dw itself (reduce_partials of one slice changes nothing)."""
    B, L, C = x.shape
    rows, rps = B * L, rows_per_slice(B * L, S)
    g = gathered(x.float(), taps, 1, pad, 1).reshape(rows, taps * C)
    d = dy.float().reshape(rows, -1)
    out = torch.zeros(S, d.shape[1], taps * C)
    for s in range(S):
        r0, r1 = s * rps, min(rows, (s + 1) * rps)
        if r0 < r1:
            out[s] = x3_matmul(d[r0:r1].t(), g[r0:r1], drop_lo_hi) if split else d[r0:r1].t() @ g[r0:r1]
    return out


def reduce_partials(partial: torch.Tensor, C: int, taps: int) -> torch.Tensor:
    """The reducers: slices added in index order in fp32, then PyTorch's (N, C, taps) layout."""
    acc = partial[0].clone()
    for s in range(1, partial.shape[0]):
        acc = acc + partial[s]
    return dw_layout(acc, C, taps)


def emulate_dw(x, dy, taps: int, pad: int, S: int, split: bool) -> torch.Tensor:
    return reduce_partials(emulate_wgrad_partials(x, dy, taps, pad, S, split), x.shape[2], taps)


def emulate_db(dy, Sb: int) -> torch.Tensor:
    d = dy.float().reshape(-1, dy.shape[2])
    rps = (d.shape[0] + Sb - 1) // Sb
    acc = torch.zeros(d.shape[1])
    for s in range(Sb):
        acc = acc + d[s * rps:(s + 1) * rps].sum(0)
    return acc


def emulate_dx(dy, w, taps: int, pad: int, split: bool, flip: bool = True) -> torch.Tensor:
    g = gathered(dy.float(), taps, 1, taps - 1 - pad, 1)
    wm = dgrad_matrix(w.float(), flip)
    return x3_matmul(g, wm) if split else g @ wm


# ---------------------------------------------------------------------------------------------------------------------------------
# gates
# ---------------------------------------------------------------------------------------------------------------------------------
def gamma_x3(n: int, extra: int) -> float:
    assert n <= K_MAX
    return X3_PRODUCT + (6.0 * n * (1.0 + 2.0 ** -6) + extra) * U24


def gamma_dw(c: Case, p: Plan) -> float:
    R = c.rows
    assert R + p.S + 6 <= K_MAX, f"{case_id(c)}: R + S + 6 = {R + p.S + 6} > {K_MAX}: the first-order bound is not written for it"
    return gamma_x3(R, p.S + 6) if c.mode == "fp32x" and wgrad_split(p) else (R + p.S + 6) * U24


def gamma_db(c: Case, p: Plan) -> float:
    assert c.rows + 1 <= K_MAX
    return (c.rows + 1) * U24


def gamma_dx(c: Case, p: Plan) -> float:
    K = c.taps * c.N
    return gamma_x3(K, 3) if c.mode == "fp32x" and dgrad_split(p) else (K + 3) * U24


def _where(d, ref, A, i: int, dims) -> str:
    idx, rest = [], i
    for s in reversed(d.shape):
        idx.append(rest % s)
        rest //= s
    idx = tuple(reversed(idx))
    name = ", ".join(f"{n} {j}" for n, j in zip(dims, idx))
    return f"({name}): got {float(d[idx]):.9g}, ref {float(ref[idx]):.9g}, A {float(A[idx]):.4g}"


def _finite(d, ref, A, what, label, dims):
    assert d.shape == ref.shape == A.shape, f"{what}: shapes {tuple(d.shape)} / {tuple(ref.shape)} / {tuple(A.shape)}"
    bad = ~torch.isfinite(d)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what} [{label}]: {int(bad.sum())} non-finite outputs of {d.numel()}, first at {_where(d, ref, A, i, dims)}")


DIMS = {"dx": ("clip", "position", "channel"), "dw": ("out channel", "in channel", "tap"), "db": ("out channel",)}


def rel_l2(d, ref) -> float:
    return float((d.double() - ref).norm() / ref.norm().clamp_min(1e-300))


def exact_gate(dev, ref, A, which: str, what: str, label: str) -> None:
    """Every element of dev finite and EQUAL to the fp64 reference (integer operands: max A < 2^24 makes every partial sum exact in fp32)."""
    d = dev.detach().double().cpu()
    assert float(A.max()) < 2.0 ** 24, f"{what}: max A {float(A.max()):.4g}: the partial sums of this case are not exact in fp32"
    _finite(d, ref, A, f"{what} {which}", label, DIMS[which])
    bad = d != ref
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what} {which} [{label}]: {int(bad.sum())} of {d.numel()} elements differ from the exact result, first at "
                             f"{_where(d, ref, A, i, DIMS[which])}; rel-L2 {rel_l2(d, ref):.3e}")


def rounding_gate(dev, ref, A, gamma: float, which: str, what: str, label: str) -> float:
    """|dev - ref| <= gamma A for EVERY element, dev finite everywhere.  Returns max err / bound."""
    d = dev.detach().double().cpu()
    _finite(d, ref, A, f"{what} {which}", label, DIMS[which])
    err = (d - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / (gamma * A))        # 0 / 0 = 0, x / 0 = inf
    worst = int(ratio.flatten().argmax())
    r = float(ratio.flatten()[worst])
    assert r <= 1.0, (f"{what} {which} [{label}]: err/bound {r:.3f} > 1 at {_where(d, ref, A, worst, DIMS[which])}; {int((ratio > 1).sum())} of "
                      f"{d.numel()} elements over the bound, gamma {gamma:.3e}, rel-L2 {rel_l2(d, ref):.3e}")
    return r


def references(c: Case, ops):
    """{which: (ref, A)} for the outputs the case asks for."""
    x, w, dy = ops
    out = {}
    if "x" in c.outs:
        out["dx"] = dgrad_ref(dy, w, c.taps, c.pad)
    if "w" in c.outs:
        out["dw"] = wgrad_ref(x, dy, c.taps, c.pad)
    if "b" in c.outs:
        out["db"] = db_ref(dy)
    return out


def emulate(c: Case, ops, p: Optional[Plan] = None):
    """{which: fp32 tensor} of a correct kernel for the outputs the case asks for."""
    x, w, dy = ops
    p = p or parse(c.expected_label)
    x3 = c.mode == "fp32x"
    out = {}
    if "x" in c.outs:
        out["dx"] = emulate_dx(dy, w, c.taps, c.pad, x3 and dgrad_split(p))
    if "w" in c.outs:
        out["dw"] = emulate_dw(x, dy, c.taps, c.pad, p.S, x3 and wgrad_split(p))
    if "b" in c.outs:
        out["db"] = emulate_db(dy, p.Sb)
    return out


def gammas(c: Case, p: Plan):
    return {"dx": gamma_dx(c, p), "dw": gamma_dw(c, p) if "w" in c.outs else None, "db": gamma_db(c, p) if "b" in c.outs else None}
