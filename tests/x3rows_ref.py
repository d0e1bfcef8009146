"""The fp32x engine's pre-split activation rows: the layout in torch, seeded faults of its writers and its reader, the dispatch rules that
decide which kernel writes or reads it, and the fp32 error bounds of the three producers for the chained tests.

LAYOUT (csrc/common.h st4_x3, read by the AX branch of conv_gemm_mt's split K step).  A row of C fp32 channels (C % 32 == 0) occupies the same
C * 4 bytes as C / 32 chunks of 128 bytes, chunk j = [hi of channels 32 j .. 32 j + 31 | lo' of the same channels], 32 fp16 each, with
    hi = fp16(v),   lo' = fp16((v - hi) * 2048)          (conv1d_ref.x3_split; both conversions round to nearest even, as the device's cast)
encode() / decode() carry rows as fp16 tensors (..., 2 C): the bytes of the device buffer (little endian), reinterpreted.

ROUND TRIP.  decode(encode(v)) = hi + lo' / 2048 =: hi + lo, so the round-trip error is lo - r with r = v - hi the residual the second
conversion rounds.  r is exact in fp32 (hi keeps the leading 11 bits of v) and so is 2048 r.  Two roundings enter:
  1. hi = fp16(v).  |v| >= 2^-14 (hi normal): |r| <= 2^-11 |v|.  |v| < 2^-14 (hi subnormal, a multiple of 2^-24): |r| <= 2^-25.
  2. lo' = fp16(2048 r).  If 2048 |r| >= 2^-14, lo' is normal: |lo' - 2048 r| <= 2^-11 * 2048 |r|, i.e. |lo - r| <= 2^-11 |r| <= 2^-22 |v|.
     If 2048 |r| < 2^-14, lo' is subnormal: |lo' - 2048 r| <= 2^-25, i.e. |lo - r| <= 2^-36.  For |v| < 2^-14 that is the only case
     (2048 |r| <= 2^-14; at equality lo' is exact).
  So |decode(encode(v)) - v| <= max(2^-22 |v|, 2^-36) for |v| < 65520 (beyond, fp16(v) is inf): round_trip_bound().  This is the d_a of
  conv1d_ref.py's fp32x gate, which therefore covers a GEMM that reads encode(x) exactly as it covers one that splits x itself.

FAULTS.  Each name is a wrong writer (encode(v, fault)), a wrong reader (halves(rows, fault)), or both:
  lo_unscaled      writer: lo' = fp16(v - hi);  reader: the second half taken as lo (2048 x too large after the common / 2048)
  halves_swapped   [lo' | hi] per chunk, on either side
  pitch_64         chunk j at byte 64 j instead of 128 j (a chunk's lo' is overwritten by the next chunk's hi; the row's second half is
                   never written and keeps what the buffer held), on either side
  head_local_chunk the chunk index taken from the channel inside its 64-channel head, (c % 64) >> 5, instead of from the row channel: every
                   head lands on chunks 0 and 1, on either side
  hi_truncated     writer only: hi = fp16 truncation of v (lo' follows from that hi).  The pair still decodes to v within 2^-21 |v|, so no
                   accuracy gate on a consumer can see it: only the producers' byte comparison does (test_x3rows_cpu.py asserts both halves
                   of that sentence)

DISPATCH, restated from the launchers (the tests name the kernel a shape reaches in their ids; test_x3rows_cpu.py pins the restatements):
  gn_silu_kernel_name   norms.hip gn_silu_go             ln_kernel_name        norms.hip ln_go
  attention_kernel_name attention.hip launch_attention, attention_mfma.hip attention_mfma_go, attention_bwd.hip launch_attention_f32_mfma
  mt_x3_prefers / mt_x3_variant / mt_x3_min_cols        conv_gemm_mt.hip conv_gemm_prefers_mt_x3, conv_gemm_mt_x3_variant

PRODUCER ERROR BOUNDS (fp64 reference a and a per-element bound da on the fp32 value the device forms BEFORE it is split), for the chained
tests: |GEMM_dev(a_dev) - GEMM(a)| <= gate(a_dev) + sum_k |w_k| da_k, and the gate's A is formed from |a| + da (chain_gate).  u = 2^-24; every
count is first order plus one unit for the second-order terms, as in conv1d_ref.py.  rsqrtf: 4 u (gemm_epilogue_ref.py).
  ln_modulate (ln_modulate_kernel).  s_abs = mean_j |x_j - x_0| over the row, mu, var, r = 1 / sqrt(var + eps) its fp64 statistics.
      mean = x_0 + fl(sum (x_j - x_0)) / C: the difference 1, a lane's ordered sum of <= 16 terms and a butterfly of <= 6 levels 21, the
      division 1, the last sum 1 (on |mu|):                    dmean = 24 u s_abs + u |mu|
      var: d = x - mean (2 u on d^2), the fmaf chain and the butterfly 22, / C and + eps 2; sum (x - mean_dev)^2 / C = var + dmean^2 exactly:
                                                                e_rstd = 13 u + 4 u + dmean^2 / (2 (var + eps))      (relative)
      y = (x - mean) rstd (difference 1, product 1), out = fmaf(y, fl(1 + sc), sh) (the sum 1, the fmaf 1 on |out|):
                                                                da = r |1 + sc| ((e_rstd + 4 u) |x - mu| + dmean) + u |a|
  gn_silu (gn_silu_reg_kernel, both passes in registers).  Per (clip, group) of n = L C / G values, pivot = the slab's first:
      mean: the difference 1, a thread's ordered sum of <= 64 terms, six DPP levels, an ordered sum of eight waves: 77; / n and + pivot:
                                                                dmean = 80 u s_abs + u |mu|
      var about that mean: 2 + 64 + 6 + 8 + 2 = 82 u:           e_rstd = 41 u + 4 u + dmean^2 / (2 (var + eps))
      (gn_silu_kernel, the strided form for slabs beyond the registers, forms its variance in one pass about the pivot and is not bounded here:
      the chained test's shape takes the register form, and gn_silu_ref asserts that.)
      t = fmaf(x - mean, fl(rstd gamma), beta):                 dt = r |gamma| ((e_rstd + 4 u) |x - mu| + dmean) + u |t|
      silu(t) = t / (1 + expf(-t)): Lipschitz 1.10 (gemm_epilogue_ref.py) and its own arithmetic, for which that module's measured
      C_ACT[3] u |t| (silu(gelu(.)): a superset of these operations) is reused:         da = 1.10 dt + C_ACT[3] u |t|
  attention (attn_fwd_x3_kernel).  q' = fl(q scale log2 e), s = q' . k through the split products of 64 terms: the GEMM coefficient of
      conv1d_ref.gamma(64, "fp32x", split) on A_s = sum_d m(q'_d) m(k_d), m(.) = max(|.|, 2^-14), plus the rounding of q' (u A_s) and the
      combination fmaf(sl, 1 / 2048, sm) (inside gamma's K + 3):         e_s = (gamma(64) + u) A_s
      p = exp2f(s - m): the difference u |s - m|, the constant fl(log2 e) and its product with 1 / 8 2 u |s - m| (what they add to every score
      alike cancels in the ratio), exp2f 4 u (2 ulp allowed for the library function):          rho = ln 2 (e_s + 3 u |s - m|) + 4 u
      (relative; with ph = 2^(s - m_final), the value of p after the later rescales -- errors made under an earlier, smaller maximum are scaled
      down with their terms, so the operand floor of the split may be applied to ph: m(ph) = max(ph, 2^-14)).
      numerator: the split products over L keys, gamma(L) on A_o = sum_j m(ph_j) m(v_j); the rescale of every one of the nkt = ceil(L / 32)
      key tiles one rounding each; denominator l = sum ph: a lane's ordered sum of 16, one sum per tile, the half-wave exchange: 18 + nkt.
      out = fmaf(ol, 1 / 2048, o) / l: 3 more.  With w_j = ph_j / l:
          da = gamma(min(L, 4094)) A_o / l + sum_j rho_j w_j |v_j| + nkt u sum_j w_j |v_j| + |a| (sum_j rho_j w_j + (21 + nkt) u)
Nothing here is fitted to a device run.  Plain module (not a conftest): the tests import it like conv1d_ref.py.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Tuple

import torch

import conv1d_ref as R
import gemm_epilogue_ref as E
import numerics as nx

u = R.U24
HEAD = 64                                     # channels per attention head (the only head size the kernels take)
SPLIT_LABEL = "conv_gemm_mt<x3>"              # the one kernel that reads pre-split rows (one label for every tile variant)
FAULTS = ("lo_unscaled", "halves_swapped", "pitch_64", "head_local_chunk", "hi_truncated")
WRITER_ONLY = ("hi_truncated",)


# ---------------------------------------------------------------------------------------------------------------------------------
# the layout
# ---------------------------------------------------------------------------------------------------------------------------------
def _nan_rows(shape, C: int) -> torch.Tensor:
    """An fp16 view (..., 2 C) of an fp32 buffer (..., C) filled with NaN, as numerics.nan_like leaves it."""
    return torch.full(tuple(shape) + (C,), float("nan"), dtype=torch.float32).view(torch.float16)


def trunc16(v: torch.Tensor) -> torch.Tensor:
    """fp16 truncation (round toward zero) of fp32 values, carried in fp32."""
    h = v.float().half()
    over = h.float().abs() > v.float().abs()
    bits = h.view(torch.int16) - over.to(torch.int16)          # sign-magnitude: one step toward zero in either sign
    return bits.view(torch.float16).float()


def _chunk_slot(j: int, fault: str) -> Tuple[int, int]:
    """fp16 offsets of (hi, lo') of chunk j inside a row."""
    if fault == "pitch_64":
        base = 32 * j
    elif fault == "head_local_chunk":
        base = 64 * (j % (HEAD // 32))
    else:
        base = 64 * j
    return (base + 32, base) if fault == "halves_swapped" else (base, base + 32)


def encode(v: torch.Tensor, fault: str = "") -> torch.Tensor:
    """fp32 (..., C) -> the pre-split rows as fp16 (..., 2 C).  fault: one of FAULTS (a wrong writer; bytes it never writes stay NaN-fp32)."""
    assert fault == "" or fault in FAULTS, fault
    v = v.detach().float().cpu()
    C = v.shape[-1]
    assert C % 32 == 0, "pre-split rows need C % 32 == 0"
    if fault == "hi_truncated":
        hi = trunc16(v)
        lo = ((v - hi) * 2048.0).half().float()
    else:
        hi, lo = R.x3_split(v)
        if fault == "lo_unscaled":
            lo = (v - hi).half().float()
    rows = _nan_rows(v.shape[:-1], C)
    for j in range(C // 32):                                    # where a fault makes chunks overlap, the later channel wins here (a race on the device)
        oh, ol = _chunk_slot(j, fault)
        rows[..., oh:oh + 32] = hi[..., 32 * j:32 * j + 32].half()
        rows[..., ol:ol + 32] = lo[..., 32 * j:32 * j + 32].half()
    return rows


def halves(rows: torch.Tensor, fault: str = "") -> Tuple[torch.Tensor, torch.Tensor]:
    """(hi, lo') in fp32, (..., C) each, as a reader takes them from fp16 rows (..., 2 C).  fault: a wrong reader."""
    assert fault == "" or (fault in FAULTS and fault not in WRITER_ONLY), fault
    C = rows.shape[-1] // 2
    r = rows.detach().cpu().float()
    hi, lo = torch.empty(r.shape[:-1] + (C,)), torch.empty(r.shape[:-1] + (C,))
    for j in range(C // 32):
        oh, ol = _chunk_slot(j, fault)
        hi[..., 32 * j:32 * j + 32] = r[..., oh:oh + 32]
        lo[..., 32 * j:32 * j + 32] = r[..., ol:ol + 32]
    return hi, (lo * 2048.0 if fault == "lo_unscaled" else lo)


def decode(rows: torch.Tensor) -> torch.Tensor:
    """fp16 rows (..., 2 C) -> the value they stand for, hi + lo' / 2048, exact in fp64: (..., C)."""
    hi, lo = halves(rows)
    return hi.double() + lo.double() / 2048.0


def round_trip_bound(v: torch.Tensor) -> torch.Tensor:
    return torch.maximum(2.0 ** -22 * v.double().abs(), torch.full_like(v, 2.0 ** -36, dtype=torch.float64))


def rows_of(buf: torch.Tensor) -> torch.Tensor:
    """A device (or host) fp32 buffer (..., C) reinterpreted as the fp16 rows (..., 2 C) a producer with xfmt wrote into it."""
    return buf.detach().cpu().contiguous().view(torch.float16)


def as_f32(rows: torch.Tensor) -> torch.Tensor:
    """fp16 rows (..., 2 C) reinterpreted as the fp32 buffer (..., C) handed to a consumer."""
    return rows.contiguous().view(torch.float32)


def same_bytes(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)))


def byte_diff(got: torch.Tensor, want: torch.Tensor, what: str) -> str:
    """'' when the two fp16 row tensors hold the same bytes, else a message naming the first differing (row..., chunk, half, channel)."""
    if same_bytes(got, want):
        return ""
    g, w = got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)
    bad = (g != w)
    i = int(bad.flatten().nonzero()[0])
    idx = nx._unravel(i, g.shape)
    e = idx[-1]
    return (f"{what}: {int(bad.sum())} of {g.numel()} fp16 words differ, first at row {idx[:-1]}, chunk {e // 64}, {'lo' if (e % 64) >= 32 else 'hi'} half, "
            f"channel {32 * (e // 64) + e % 32}: got 0x{int(g.flatten()[i]) & 0xFFFF:04x}, want 0x{int(w.flatten()[i]) & 0xFFFF:04x}")


def emulate_src_x3(rows: torch.Tensor, w_op: torch.Tensor, bias, res, taps: int, stride: int, pad: int, up: int, fault: str = "") -> torch.Tensor:
    """What conv_gemm_mt computes from pre-split rows (B, L, 2 C) and the fp32 weight (N, C, taps), in fp32 (conv1d_ref.emulate's split branch
    with the activation halves taken from the rows instead of formed): accM + accL / 2048 + bias + res.  fault: a wrong reader."""
    hi, lo = halves(rows, fault)
    gh, gl = R.gathered(hi, taps, stride, pad, up), R.gathered(lo, taps, stride, pad, up)
    wh, wl = R.x3_split(R.weight_matrix(w_op.float()))
    y = gh @ wh + (gh @ wl + gl @ wh) * (1.0 / 2048.0)
    if bias is not None:
        y = y + bias.float()
    if res is not None:
        y = y + res.float()
    return y


# ---------------------------------------------------------------------------------------------------------------------------------
# dispatch rules, restated
# ---------------------------------------------------------------------------------------------------------------------------------
GN_REG_MAX_RV = 16                            # norms.hip gn_reg_max_rv() of the product build


def gn_silu_kernel_name(L: int, C: int, G: int, dtype: str = "fp32") -> str:
    """gn_silu_go for contiguous rows (ld = out_ld = C)."""
    V = 4 if dtype == "fp32" else 8
    cpg = C // G
    al = C % V == 0
    if al and cpg % V == 0 and 512 % (cpg // V) == 0 and L * (cpg // V) <= GN_REG_MAX_RV * 512:
        nv = L * (cpg // V)
        return f"gn_silu_reg_kernel<{dtype},{2 if nv <= 1024 else 4 if nv <= 2048 else 8 if nv <= 4096 else 16}>"
    if al and cpg % V == 0:
        return f"gn_silu_kernel<{dtype},{V}>"
    for vw in (4, 2):
        if C % vw == 0 and cpg % vw == 0:
            return f"gn_silu_kernel<{dtype},{vw}>"
    return f"gn_silu_kernel<{dtype},1>"


def ln_plan(C: int, dtype: str = "fp32") -> Tuple[int, int]:
    """(tpr, vpt) of ln_go: threads per row and 16-byte vectors per thread."""
    V = 4 if dtype == "fp32" else 8
    vpr, tpr = C // V, 1
    while tpr < 64 and tpr * 2 <= vpr:
        tpr *= 2
    assert C % V == 0 and vpr % tpr == 0 and vpr // tpr in (1, 2, 4, 8), f"ln_go refuses C = {C}"
    return tpr, vpr // tpr


def ln_kernel_name(C: int, dtype: str = "fp32") -> str:
    tpr, vpt = ln_plan(C, dtype)
    return f"ln_modulate_kernel<{dtype},{vpt}>/tpr{tpr}"


def attention_kernel_name(dtype: str, B: int, H: int, L: int) -> str:
    """launch_attention at strides that are multiples of 8 elements (contiguous and packed rows alike), head dim 64."""
    if dtype == "fp32":
        return "attn_fwd_f32_mfma_kernel"
    if dtype == "fp32x":
        return "attn_fwd_x3_kernel"
    t = "bf16" if dtype == "bf16" else "f16"
    waves_plain = -(-L // 64) * H * B * 2                        # the 2-wave kernel: 64 queries per workgroup
    long_kernel = L >= 256 and -(-L // 128) * H * B >= 128
    if not long_kernel and waves_plain < 1024 and L <= 4096:
        return f"attention_ksplit_kernel<{t}>"
    return f"attention_mfma4_kernel<{t}>" if L >= 256 else f"attention_mfma_kernel<{t}>"


def mt_x3_prefers(M: int, N: int, K: int) -> bool:
    return K >= 256 and -(-M // 128) * -(-N // 64) >= 128


def mt_x3_min_cols(M: int) -> int:
    """The fewest output columns (a multiple of 64) at which M rows still take the macro tiles."""
    return 64 * -(-128 // -(-M // 128))


def mt_x3_variant(M: int, N: int, solo: bool) -> int:
    """conv_gemm_mt_x3_variant: 0 = 256x128, 5 = 128x128 two slots, 7 = 128x64."""
    if N <= 64 or ((N % 128) and (N % 128) <= 64 and N % 64 == 0 and N <= 192):
        return 7
    if -(-M // 256) * -(-N // 128) >= 512:
        return 0
    if solo and -(-M // 128) * -(-N // 128) < 256 and N % 64 == 0:
        return 7
    return 5


# ---------------------------------------------------------------------------------------------------------------------------------
# producers: fp64 references and the bounds of their fp32 error (module docstring)
# ---------------------------------------------------------------------------------------------------------------------------------
def ln_modulate_ref(x: torch.Tensor, ss, eps: float):
    """(a, da) fp64 (B, L, C): LayerNorm(x; eps) * (1 + ss[:, :C]) + ss[:, C:] (ss None: plain) and the bound of ln_modulate_kernel's error."""
    xd = x.double()
    C = xd.shape[-1]
    mu = xd.mean(-1, keepdim=True)
    var = ((xd - mu) ** 2).mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    sc1 = 1.0 + ss.double()[:, None, :C] if ss is not None else torch.ones(1, 1, C, dtype=torch.float64)
    sh = ss.double()[:, None, C:] if ss is not None else torch.zeros(1, 1, C, dtype=torch.float64)
    a = (xd - mu) * r * sc1 + sh
    s_abs = (xd - xd[..., :1]).abs().mean(-1, keepdim=True)
    dmean = 24 * u * s_abs + u * mu.abs()
    e_rstd = 17 * u + dmean ** 2 / (2 * (var + eps))
    da = r * sc1.abs() * ((e_rstd + 4 * u) * (xd - mu).abs() + dmean) + u * a.abs()
    return a, da


def gn_silu_ref(x: torch.Tensor, G: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float):
    """(a, da) fp64 (B, L, C): SiLU(GroupNorm(x)) channels-last and the bound of the GroupNorm + SiLU kernels' error."""
    xd = x.double()
    B, L, C = xd.shape
    cpg = C // G
    xg = xd.reshape(B, L, G, cpg)
    mu = xg.mean((1, 3), keepdim=True)
    var = ((xg - mu) ** 2).mean((1, 3), keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    pivot = xg[:, :1, :, :1]
    s_abs = (xg - pivot).abs().mean((1, 3), keepdim=True)
    assert gn_silu_kernel_name(L, C, G).startswith("gn_silu_reg_kernel"), "the bound is written for the register form"
    dmean = 80 * u * s_abs + u * mu.abs()
    e_rstd = 45 * u + dmean ** 2 / (2 * (var + eps))
    ga, be = gamma.double().reshape(1, 1, G, cpg), beta.double().reshape(1, 1, G, cpg)
    t = (xg - mu) * r * ga + be
    dt = r * ga.abs() * ((e_rstd + 4 * u) * (xg - mu).abs() + dmean) + u * t.abs()
    a = t * torch.sigmoid(t)
    da = 1.10 * dt + E.C_ACT[3] * u * t.abs()
    return a.reshape(B, L, C), da.reshape(B, L, C)


def attention_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, H: int):
    """(a, da) fp64 (B, L, H * 64): softmax(q k^T / 8) v per head and the bound of attn_fwd_x3_kernel's error."""
    B, L, HD = q.shape
    D = HD // H
    assert D == HEAD
    sh = lambda t: t.double().reshape(B, L, H, D).transpose(1, 2)   # noqa: E731
    fl = R.X3_FLOOR
    c = 1.4426950408889634 / math.sqrt(D)
    qs, kd, vd = sh(q) * c, sh(k), sh(v)
    s = qs @ kd.transpose(-1, -2)                                    # log2 domain
    A_s = qs.abs().clamp_min(fl) @ kd.abs().clamp_min(fl).transpose(-1, -2)
    g64 = R.gamma(D, "fp32x", SPLIT_LABEL)
    m = s.max(-1, keepdim=True).values
    ph = torch.exp2(s - m)
    l = ph.sum(-1, keepdim=True)
    w = ph / l
    a = w @ vd
    rho = math.log(2.0) * ((g64 + u) * A_s + 3 * u * (s - m).abs()) + 4 * u
    nkt = -(-L // 32)
    gL = R.gamma(min(L, R.K_MAX), "fp32x", SPLIT_LABEL)
    A_o = ph.clamp_min(fl) @ vd.abs().clamp_min(fl)
    wv = w @ vd.abs()
    da = gL * A_o / l + (rho * w) @ vd.abs() + nkt * u * wv + a.abs() * ((rho * w).sum(-1, keepdim=True) + (21 + nkt) * u)
    back = lambda t: t.transpose(1, 2).reshape(B, L, HD)            # noqa: E731
    return back(a), back(da)


def chain_gate(dev: torch.Tensor, a: torch.Tensor, da: torch.Tensor, w: torch.Tensor, bias, res, badd, taps: int, pad: int, label: str, what: str):
    """The fp32x GEMM gate of conv1d_ref.py on a producer -> consumer pair: ref = conv(a, w) + bias + res + badd[b] in fp64 from the producer's
    fp64 output a (B, L, C); the consumer read a_dev with |a_dev - a| <= da, so A is formed from |a| + da and the term sum |w| da is folded
    into it (A += conv(da, |w|) / gamma).  w (N, C, taps) fp32 as the kernel multiplies by it.  One more unit of K where badd adds a rounding."""
    K = taps * a.shape[-1] + (1 if badd is not None else 0)
    ref, _ = R.conv1d_ref(a, w, bias, res, taps, 1, pad, 1)
    _, A = R.conv1d_ref(a.abs() + da, w, bias, res, taps, 1, pad, 1, R.X3_FLOOR)
    if badd is not None:
        ref = ref + badd.double()[:, None, :]
        A = A + badd.double().abs()[:, None, :]
    wda, _ = R.conv1d_ref(da, w.abs(), None, None, taps, 1, pad, 1)
    A = A + wda / R.gamma(K, "fp32x", label)
    return R.gate(dev, ref, A, K, "fp32x", label, what)


# ---------------------------------------------------------------------------------------------------------------------------------
# test inputs (shared by test_x3rows_cpu.py and test_gpu_x3rows.py)
# ---------------------------------------------------------------------------------------------------------------------------------
REGIMES = ("offset:0.3", "offset:30", "dead:4", "offset:300", "const")     # numerics.py: ordinary, offset, dead, far offset, constant


def spread(n: int, gen: torch.Generator, lo: float, hi: float) -> torch.Tensor:
    """n values +-2^U(lo, hi): magnitudes spread over many binades, so that hi and lo' are exercised away from unit scale (and below 2^-14)."""
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    return sign * torch.exp2(lo + (hi - lo) * torch.rand(n, generator=gen))


def gn_inputs(B: int, L: int, C: int, G: int, seed: int = 0):
    """(x (B, L, C), gamma, beta): group g of every clip follows REGIMES[g % 5]; gamma and beta spread over 2^-12 .. 2^10 (outputs < 2^13)."""
    g = torch.Generator().manual_seed(seed + L)
    xs = [nx.grouped_input(B, L, C, G, r, g) for r in REGIMES]
    cpg = C // G
    x = torch.cat([xs[i % len(REGIMES)][:, :, i * cpg:(i + 1) * cpg] for i in range(G)], dim=-1)
    return x.contiguous(), spread(C, g, -12.0, 10.0), spread(C, g, -12.0, 10.0)


def ln_inputs(B: int, L: int, C: int, mod: bool, seed: int = 0):
    """(x (B, L, C), ss (B, 2 C) or None): row l follows REGIMES[l % 5]; 1 + scale and shift spread over 2^-12 .. 2^10."""
    g = torch.Generator().manual_seed(seed + C)
    xs = [nx.row_input(B, L, C, r, g) for r in REGIMES]
    x = torch.stack([xs[l % len(REGIMES)][:, l] for l in range(L)], dim=1)
    ss = torch.cat([spread(B * C, g, -12.0, 8.0).reshape(B, C) - 1.0, spread(B * C, g, -12.0, 10.0).reshape(B, C)], dim=-1) if mod else None
    return x.contiguous(), ss


def attn_inputs(B: int, H: int, L: int, seed: int = 0, v_spread: bool = True) -> torch.Tensor:
    """The engine's packed rows (B, L, 3 H 64) = q | k | v; every value channel scaled by +-2^U(-14, 10) (v_spread), so that the outputs
    -- averages of a channel's values -- spread the same way."""
    g = torch.Generator().manual_seed(seed + 7 * L + H)
    hd = H * HEAD
    qkv = torch.randn(B, L, 3 * hd, generator=g)
    if v_spread:
        qkv[..., 2 * hd:] *= spread(hd, g, -14.0, 10.0)
    return qkv.contiguous()


class ConsCase(NamedTuple):
    """One sf_op_conv1d_epi launch on pre-split rows.  ops as gemm_epilogue_ref.EpiCase ("b" bias, "r" residual, "a" badd); variant: the tile
    variant conv_gemm_mt_x3_variant picks (asserted against mt_x3_variant); sub: the fp64 gate reads a subset of the rows."""
    name: str
    B: int
    L: int
    C: int
    N: int
    taps: int
    pad: int
    ops: str
    solo: bool
    variant: int
    sub: bool = False

    @property
    def K(self) -> int:
        return self.taps * self.C

    @property
    def M(self) -> int:
        return self.B * self.L


CONS_CASES = (
    ConsCase("qkv", 2, 1024, 256, 512, 1, 0, "", False, 5),
    # M = 2000 is still 16 row tiles of 128, so the threshold of 128 tiles of 128x64 needs 8 column tiles: mt_x3_min_cols(2000) = 512
    ConsCase("qkv-ragged-solo", 2, 1000, 256, 512, 1, 0, "", True, 7),
    # three clips of 1323 rows: clip boundaries (zero-padding rows of the 3-tap window) inside row tiles 10 and 20, one row in the last tile
    ConsCase("conv1", 3, 1323, 256, 256, 3, 1, "br", False, 5),
    ConsCase("attn_out", 2, 1024, 512, 512, 1, 0, "ra", False, 5),
    ConsCase("narrow", 2, 8129, 256, 64, 1, 0, "b", False, 7),
    ConsCase("wide", 2, 8192, 256, 1024, 1, 0, "b", False, 0, True),
)


def cons_id(c: ConsCase) -> str:
    return f"{c.name}-B{c.B}-L{c.L}-C{c.C}-N{c.N}-k{c.taps}-{c.ops or 'plain'}{'-solo' if c.solo else ''}-variant{c.variant}"


def cons_epi(c: ConsCase, dtype: str = "fp32x") -> E.EpiCase:
    return E.EpiCase(c.name, dtype, c.B, c.L, c.C, 0, c.N, c.taps, 1, c.pad, 1, c.ops, 0, False, False, False, False, "", SPLIT_LABEL, False, False)


def cons_operands(c: ConsCase) -> dict:
    """gemm_epilogue_ref.epi_operands of the case, plus w3 = the weight in conv1d_ref's (N, C, taps) layout."""
    o = E.epi_operands(cons_epi(c), seed=3)
    o["w3"] = o["w"].reshape(c.N, c.taps, c.C).permute(0, 2, 1).contiguous()
    return o


def cons_desc(c: ConsCase, src_x3: int, dtype: str = "fp32x", C2: int = 0, **ptrs):
    d = E.desc_of(dtype, c.B, c.L, c.C, C2, c.N, c.taps, 1, c.pad, 1, solo=c.solo, **ptrs)
    d.src_x3 = src_x3
    return d


def cons_probe_ptrs(c: ConsCase) -> dict:
    return E.epi_probe_ptrs(cons_epi(c))


def cons_rows(c: ConsCase):
    """The rows of a case the fp64 gate reads: all of them, or (sub) the first 256, the last 256 and every 8th in between."""
    if not c.sub:
        return None
    return torch.cat([torch.arange(256), torch.arange(256, c.M - 256, 8), torch.arange(c.M - 256, c.M)])


def cons_ref(c: ConsCase, o: dict, rows=None):
    """(ref, A, K) of conv1d_ref.py's gate for the case: bias and residual as there, badd one more term of A and one more unit of K.
    rows (taps == 1 only): the gate's subset, returned as one clip (1, len(rows), N)."""
    x, res, badd = o["x"], o["res"], o["badd"]
    if rows is not None:
        assert c.taps == 1
        b_of = rows // c.L
        x = x.reshape(c.M, c.C)[rows][None]
        res = res.reshape(c.M, c.N)[rows][None] if res is not None else None
    ref, A = R.conv1d_ref(x, o["w3"], o["bias"], res, c.taps, 1, c.pad, 1, R.X3_FLOOR)
    K = c.K
    if badd is not None:
        add = badd.double()[b_of][None] if rows is not None else badd.double()[:, None, :]
        ref, A, K = ref + add, A + add.abs(), K + 1
    return ref, A, K
