"""Input regimes and checks for the statistics inside the normalisation and attention kernels.

The usual test inputs (randn * 1.3..1.5 + 0.2..0.4) have a mean/std ratio of about 0.3, where every way of computing a variance
agrees.  The regimes here are where they do not:
  * offset groups / rows  x = mu + sigma z  with mu / sigma in OFFSET_RATIOS: a one-pass M2 = sum x^2 - sum x * mean in fp32 loses
    about log2(ratio^2) bits, a pivot-shifted or two-pass M2 does not;
  * near-constant ("dead") groups, sigma = 1e-3 |mu|, mu in DEAD_MEANS, and exactly constant groups (variance 0: rstd = 1 / sqrt(eps));
  * peaked attention scores (std of q.k / sqrt(D) in PEAK_STDS) with one dominant key per query in the first, a middle or the last
    (ragged) key block: the running-max rescale of an online softmax and the merge of key-split partials.

check_close() is the gate: the suite's whole-tensor rel-L2 plus a max-error bound that names the worst (clip, row, channel), so that
one bad group or chunk cannot hide in the average.  Plain module (not a conftest): the tests import it like helpers.py.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

OFFSET_RATIOS = (3.0, 30.0, 300.0)
DEAD_MEANS = (1.0, 4.0)
PEAK_STDS = (8.0, 30.0)
U24 = 2.0 ** -24           # fp32 unit roundoff
MAX_K = 8.0                # max|err| / rms(ref) may reach MAX_K times the rel-L2 tolerance
MAX_K16 = 16.0             # ... for 16-bit outputs: one output rounding of a value 10-20x the rms (dead groups, peaked softmax) is 2^-9 of it


def offset_gate(tol: float, ratio: float) -> float:
    """The gate of an fp32 statistics test at mean/std = ratio: the existing tolerance, or what an exact-but-fp32 mean reaches
    (the mean itself is rounded to 2^-24 |mu|, i.e. 2^-24 ratio in units of sigma), whichever is larger."""
    return max(tol, 8.0 * U24 * ratio)


def regime_stats(B: int, G: int, regime: str, gen: torch.Generator):
    """(mu, sigma) per (clip, group), shape (B, G) each.  regime: 'offset:<ratio>', 'dead:<mu>' or 'const'."""
    kind, _, val = regime.partition(":")
    sign = torch.where(torch.rand(B, G, generator=gen) < 0.5, -1.0, 1.0)
    if kind == "offset":
        sigma = torch.exp(0.3 * torch.randn(B, G, generator=gen))
        return sign * float(val) * sigma, sigma
    if kind == "dead":
        mu = sign * float(val) * (1 + 0.1 * torch.rand(B, G, generator=gen))
        return mu, 1e-3 * mu.abs()
    if kind == "const":
        return sign * (0.1 + torch.rand(B, G, generator=gen)), torch.zeros(B, G)
    raise ValueError(regime)


def grouped_input(B: int, L: int, C: int, G: int, regime: str, gen: torch.Generator, dtype=torch.float32) -> torch.Tensor:
    """Channels-last (B, L, C) input whose (clip, group) slabs follow `regime`; rounded to `dtype` and returned in fp32, so that
    the reference and the kernel see the same values.  G = C gives per-channel regimes, G = 1 per-clip ones."""
    mu, sigma = regime_stats(B, G, regime, gen)
    cpg = C // G
    z = torch.randn(B, L, C, generator=gen)
    x = mu.repeat_interleave(cpg, dim=1)[:, None, :] + sigma.repeat_interleave(cpg, dim=1)[:, None, :] * z
    return x.to(dtype).float()


def row_input(B: int, L: int, C: int, regime: str, gen: torch.Generator, dtype=torch.float32) -> torch.Tensor:
    """Channels-last (B, L, C) input whose ROWS follow `regime` (LayerNorm statistics): one (mu, sigma) per (clip, row)."""
    mu, sigma = regime_stats(B, L, regime, gen)
    x = mu[:, :, None] + sigma[:, :, None] * torch.randn(B, L, C, generator=gen)
    return x.to(dtype).float()


def group_ratio(x: torch.Tensor, G: int) -> float:
    """max over (clip, group) of |mean| / std of a channels-last (B, L, C) tensor, in fp64 (asserts that a regime was reached)."""
    B, L, C = x.shape
    xg = x.double().reshape(B, L, G, C // G).permute(0, 2, 1, 3).reshape(B, G, -1)
    return float((xg.mean(-1).abs() / xg.std(-1).clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 references, from the (already dtype-rounded) fp32 inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def group_norm_cl64(x: torch.Tensor, G: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> torch.Tensor:
    """GroupNorm of a channels-last (B, L, C) tensor in fp64 -> (B, L, C) fp64."""
    return torch.nn.functional.group_norm(x.double().transpose(1, 2), G, gamma.double(), beta.double(), eps=eps).transpose(1, 2)


def gn_silu_cl64(x, G, gamma, beta, eps):
    return torch.nn.functional.silu(group_norm_cl64(x, G, gamma, beta, eps))


def peaked_qk(B: int, L: int, H: int, D: int, peak_std: float, where: str, gen: torch.Generator):
    """q (B, L, H*D), k (B, L, H*D) whose scores q.k / sqrt(D) have standard deviation ~peak_std, plus one key per (clip, head) whose
    score is ~8 peak_std for every query (the rest reach ~3-4 peak_std).  where: 'first' (key 0), 'middle' (key L // 2) or 'last'
    (key L - 1: the ragged last key block)."""
    a = math.sqrt(peak_std)                     # std(q.k / sqrt(D)) = a^2 for q, k ~ a N(0, 1)
    q = a * torch.randn(B, L, H, D, generator=gen)
    k = a * torch.randn(B, L, H, D, generator=gen)
    j = {"first": 0, "middle": L // 2, "last": L - 1}[where]
    u = torch.randn(B, 1, H, D, generator=gen)
    u = u / u.norm(dim=-1, keepdim=True)
    # key j = 2 a sqrt(D) u (twice a typical key's length); every query gets 4 a u: its score with key j is 8 a^2 (+- 2 a^2), and the
    # other keys' scores widen to ~1.1 a^2
    q = q + 4.0 * a * u
    k[:, j] = 2.0 * a * math.sqrt(D) * u[:, 0]
    return q.reshape(B, L, H * D), k.reshape(B, L, H * D)


def attention64(q, k, v, H: int) -> torch.Tensor:
    """softmax(q k^T / sqrt(D)) v per head in fp64; q, k, v (B, L, H*D) -> (B, L, H*D)."""
    B, L, HD = q.shape
    D = HD // H
    sh = lambda t: t.double().reshape(B, -1, H, D).transpose(1, 2)   # noqa: E731
    sim = sh(q) @ sh(k).transpose(-1, -2) * D ** -0.5
    return (sim.softmax(-1) @ sh(v)).transpose(1, 2).reshape(B, L, HD)


# ---------------------------------------------------------------------------------------------------------------------------------
# gates and poisoned buffers
# ---------------------------------------------------------------------------------------------------------------------------------
def check_close(got: torch.Tensor, ref: torch.Tensor, tol: float, what: str, k: float = MAX_K,
                dims: Sequence[str] = ("clip", "row", "channel")) -> float:
    """Assert rel-L2(got, ref) <= tol AND max|got - ref| / rms(ref) <= k tol (and that got is finite); returns the rel-L2.
    The failure message names the worst element by `dims` (channels-last (B, L, C) by default)."""
    g = got.detach().double().cpu()
    r = ref.detach().double().cpu()
    assert g.shape == r.shape, f"{what}: shape {tuple(g.shape)} != {tuple(r.shape)}"
    bad = ~torch.isfinite(g)
    if bool(bad.any()):
        idx = _unravel(int(bad.flatten().nonzero()[0]), g.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} non-finite outputs, first at {_name(idx, dims)}")
    err = (g - r).abs()
    rms = float(r.pow(2).mean().sqrt().clamp_min(1e-300))
    rel = float((g - r).norm() / r.norm().clamp_min(1e-300))
    worst = int(err.flatten().argmax())
    mx = float(err.flatten()[worst]) / rms
    idx = _unravel(worst, g.shape)
    where = f"worst at {_name(idx, dims)}: got {float(g[idx]):.6g}, ref {float(r[idx]):.6g}"
    print(f"{what}: rel-L2 {rel:.3e} (gate {tol:.1e}), max/rms {mx:.3e} (gate {k * tol:.1e}); {where}")
    assert rel <= tol, f"{what}: rel-L2 {rel:.3e} > {tol:.1e}; {where}"
    assert mx <= k * tol, f"{what}: max|err| / rms(ref) {mx:.3e} > {k * tol:.1e} (rel-L2 {rel:.3e}); {where}"
    return rel


def nan_like(shape, dtype, device) -> torch.Tensor:
    """An output buffer pre-filled with NaN: a skipped write fails the test instead of passing by luck."""
    return torch.full(shape, float("nan"), dtype=dtype, device=device)


def poisoned_workspace(nbytes: int, device, dtype=torch.uint8) -> torch.Tensor:
    """A workspace filled with 0xFF bytes (NaN as fp32): a read of stale workspace fails instead of passing by luck."""
    n = (nbytes + torch.tensor([], dtype=dtype).element_size() - 1) // torch.tensor([], dtype=dtype).element_size()
    t = torch.empty(n, dtype=dtype, device=device)
    t.view(torch.uint8).fill_(0xFF)
    return t


def _unravel(i: int, shape) -> tuple:
    out = []
    for s in reversed(shape):
        out.append(i % s)
        i //= s
    return tuple(reversed(out))


def _name(idx: tuple, dims: Optional[Sequence[str]]) -> str:
    if dims and len(dims) == len(idx):
        return "(" + ", ".join(f"{d} {i}" for d, i in zip(dims, idx)) + ")"
    return str(idx)


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 emulations of the two ways of computing chunk statistics (test_numerics_cpu.py: the regimes must tell them apart)
# ---------------------------------------------------------------------------------------------------------------------------------
def chunk_stats_fp32(x: torch.Tensor, G: int, chunk_rows: int, shifted: bool, nthreads: int = 256):
    """(mean, var) per (clip, group) the way the chunked GroupNorm statistics are formed, in fp32: every chunk of `chunk_rows` rows
    is spread over `nthreads` per-thread partials, merged serially; one-pass (mean, M2 = sum x^2 - sum x * mean) per chunk, or the
    same sums about a pivot (the chunk's first value of the group); chunks merged with Chan's formula.  x: (B, L, C) fp32."""
    B, L, C = x.shape
    cpg = C // G
    mean_out = torch.empty(B, G, dtype=torch.float64)
    var_out = torch.empty(B, G, dtype=torch.float64)
    for b in range(B):
        for g in range(G):
            n_t = torch.zeros((), dtype=torch.float32)
            m_t = torch.zeros((), dtype=torch.float32)
            q_t = torch.zeros((), dtype=torch.float32)
            for r0 in range(0, L, chunk_rows):
                blk = x[b, r0:r0 + chunk_rows, g * cpg:(g + 1) * cpg].float().flatten()
                piv = blk[0] if shifted else torch.zeros((), dtype=torch.float32)
                d = blk - piv
                n = blk.numel()
                pad = (-n) % nthreads
                dp = torch.cat([d, torch.zeros(pad)]).reshape(-1, nthreads)
                s = torch.zeros(nthreads, dtype=torch.float32)
                q = torch.zeros(nthreads, dtype=torch.float32)
                for row in dp:                                   # per-thread fp32 accumulation
                    s = s + row
                    q = q + row * row
                a = torch.zeros((), dtype=torch.float32)
                c = torch.zeros((), dtype=torch.float32)
                for t in range(nthreads):                        # serial merge of the partials
                    a = a + s[t]
                    c = c + q[t]
                nf = torch.tensor(float(n), dtype=torch.float32)
                md = a / nf
                m2 = torch.clamp(c - a * md, min=0.0)
                mean = piv + md
                tot = n_t + nf                                   # Chan merge of (n, mean, M2)
                delta = mean - m_t
                m_t = m_t + delta * (nf / tot)
                q_t = q_t + m2 + delta * delta * (n_t * nf / tot)
                n_t = tot
            mean_out[b, g] = float(m_t)
            var_out[b, g] = float(q_t / n_t)
    return mean_out, var_out
