// Training kernels of the VideoOnsetNet (R(2+1)D-18) in fp32, channels-last video activations: rows = ((n * T + t) * H + h) * W + w, channel
// counts padded to `ld` columns that hold zeros (the engine's cin_ld / cout_ld).  The forward convolutions and the stride-1 data gradients run
// on the implicit-GEMM kernels (launch_conv_gemm, geom 1); this file holds what those cannot do:
//
//   wgrad     dW[co][tap][ci] = sum_rows dY[row][co] X[src(row, tap)][ci]       -> vwgrad_kernel: a "TN" GEMM reducing over the output rows,
//             v_mfma_f32_32x32x2_f32 with both operands straight from their row-major layout (the reduction index across the half-waves), split
//             over row ranges and summed in a fixed order by vwgrad_reduce_kernel, which also writes PyTorch's (Cout, Cin, kt, kh, kw) layout
//   dgrad s2  dX[pix][ci] = sum_{taps reaching pix} sum_co dY[dst(pix, tap)][co] W[co][ci][tap]   (stride (1, s, s), kt == 1)
//             -> vdgrad_gather_kernel: input pixels grouped by (h % s, w % s) so that every 32-row tile has one tap set; no zero-dilated dY
//   BatchNorm3d (train): per-channel slice statistics (mean, M2) with a shift inside each slice, merged about the first slice's mean in order;
//             apply (+ residual, ReLU); backward sums  sum dz, sum dz xhat  per slice, merged in order, then dx (+ the residual's dz) in one pass
//   BatchNorm3d (train) across the ranks of a data-parallel group: the same slice kernels, a per-rank merge, and a rank-order merge of the gathered
//             (world, C, 2) table on either side of the caller's all-gather (statistics forward, sum dz / sum dz xhat backward)
//   spatial mean pool backward: a broadcast of dP / (H W)
// No atomics: two identical passes give bit-identical results.
#include "common.h"
#include "gemm_args.h"
#include "kernels.h"

namespace sf {
namespace {

constexpr int kTPB = 256;

inline dim3 grid1d(int64_t n) { return dim3((unsigned)std::min<int64_t>((n + kTPB - 1) / kTPB, 65536)); }

// ---- weight images --------------------------------------------------------------------------------------------------------------------
// stride-1 data gradient (the forward GEMM on flipped taps, channels transposed): out[ci][tap' * cout_ld + co] = w[co][ci][taps - 1 - tap'], zero
// for co >= cout and in the row padding [taps * cout_ld, K)
__global__ void pack_dgrad_flip_kernel(const float *__restrict__ w, int cout, int cin, int taps, int cout_ld, int K, float *__restrict__ out) {
  const int64_t total = (int64_t)cin * K;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % K), ci = (int)(i / K);
    const int t = k / cout_ld, co = k - t * cout_ld;
    out[i] = (t < taps && co < cout) ? w[((int64_t)co * cin + ci) * taps + (taps - 1 - t)] : 0.f;
  }
}

// gather data gradient: out[tap][co][ci] = w[co][ci][tap], zero for co >= cout or ci >= cin
__global__ void pack_dgrad_gather_kernel(const float *__restrict__ w, int cout, int cin, int taps, int cout_ld, int cin_ld, float *__restrict__ out) {
  const int64_t total = (int64_t)taps * cout_ld * cin_ld;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int ci = (int)(i % cin_ld);
    const int64_t r = i / cin_ld;
    const int co = (int)(r % cout_ld), t = (int)(r / cout_ld);
    out[i] = (co < cout && ci < cin) ? w[((int64_t)co * cin + ci) * taps + t] : 0.f;
  }
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------------------
// One workgroup (4 waves) owns a (32 TN) x (32 TQ) tile of dW -- rows co, columns q = tap * cin_ld + ci -- over one row range; wave w takes the
// row pairs w, w + 4, ... (the half-wave picks the row of the pair: the k index of the 32x32x2 MFMA) and the four waves' accumulators are
// added in LDS in a fixed order.  Every lane walks its output row's (t, ho, wo) incrementally and reads the source row of each of its columns'
// taps (zero outside the frame / clip).
template <int TN, int TQ>
__global__ __launch_bounds__(256) void vwgrad_kernel(const float *__restrict__ dy, int ldy, const float *__restrict__ x, int ldx, VConvGeom g,
                                                      int64_t rows, int64_t rows_per_split, float *__restrict__ partial) {
  __shared__ float red[4][32][33];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 31, fh = lane >> 5;
  const int Q = g.taps() * ldx;
  int co[TN], ci[TQ], dt[TQ], dh[TQ], dw[TQ];
  bool nok[TN], qok[TQ];
#pragma unroll
  for (int i = 0; i < TN; ++i) {
    co[i] = (blockIdx.x * TN + i) * 32 + fr;
    nok[i] = co[i] < g.cout;
  }
#pragma unroll
  for (int j = 0; j < TQ; ++j) {
    const int q = (blockIdx.y * TQ + j) * 32 + fr;
    qok[j] = q < Q;
    const int t = qok[j] ? q / ldx : 0;
    ci[j] = qok[j] ? q - t * ldx : 0;
    const int khw = g.kh * g.kw;
    dt[j] = t / khw - g.pt;
    dh[j] = (t % khw) / g.kw - g.ph;
    dw[j] = t % g.kw - g.pw;
  }
  const int64_t r_begin = (int64_t)blockIdx.z * rows_per_split, r_end = min(rows, r_begin + rows_per_split);
  f32x16 acc[TN][TQ];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TQ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  // this lane's row r walks r_begin + 2 wave + fh, +8, ...: (nt, t, ho, wo) advance incrementally
  int64_t r = r_begin + 2 * wave + fh;
  const int64_t HWo = (int64_t)g.Ho * g.Wo;
  int64_t nt = r / HWo;
  int rem = (int)(r - nt * HWo);
  int ho = rem / g.Wo, wo = rem - ho * g.Wo;
  int t = (int)(nt % g.T);
  constexpr int UNR = 4;
  for (int64_t r0 = r_begin + 2 * wave; r0 < r_end; r0 += 8 * UNR) {
    float av[UNR][TN], bv[UNR][TQ];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const bool rv = r < r_end;
#pragma unroll
      for (int i = 0; i < TN; ++i) av[u][i] = (rv && nok[i]) ? dy[r * ldy + co[i]] : 0.f;
#pragma unroll
      for (int j = 0; j < TQ; ++j) {
        const int ts = t + dt[j], hs = ho * g.sh + dh[j], ws = wo * g.sw + dw[j];
        const bool ok = rv && qok[j] && (unsigned)ts < (unsigned)g.T && (unsigned)hs < (unsigned)g.Hi && (unsigned)ws < (unsigned)g.Wi;
        const int64_t src = ((nt + dt[j]) * g.Hi + hs) * (int64_t)g.Wi + ws;
        bv[u][j] = ok ? x[src * ldx + ci[j]] : 0.f;
      }
      r += 8;
      wo += 8;
      while (wo >= g.Wo) {
        wo -= g.Wo;
        if (++ho == g.Ho) {
          ho = 0;
          ++nt;
          if (++t == g.T) t = 0;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
      for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TQ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][i], bv[u][j], acc[i][j], 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TQ; ++j) {
      if (i + j) __syncthreads();
#pragma unroll
      for (int e = 0; e < 16; ++e) red[wave][(e & 3) + 8 * (e >> 2) + 4 * fh][fr] = acc[i][j][e];
      __syncthreads();
      for (int idx = threadIdx.x; idx < 32 * 32; idx += 256) {
        const int a = idx >> 5, b = idx & 31;
        const float v = (red[0][a][b] + red[1][a][b]) + (red[2][a][b] + red[3][a][b]);
        const int nn = (blockIdx.x * TN + i) * 32 + a, qq = (blockIdx.y * TQ + j) * 32 + b;
        if (nn < g.cout && qq < Q) partial[((size_t)blockIdx.z * g.cout + nn) * Q + qq] = v;
      }
    }
}

// dw[co][ci][tap] = sum_s partial[s][co][tap * ldx + ci]   (slice order fixed; PyTorch's weight layout)
__global__ void vwgrad_reduce_kernel(const float *__restrict__ partial, int S, int cout, int cin, int taps, int ldx, float *__restrict__ dw) {
  const int64_t total = (int64_t)cout * cin * taps, Q = (int64_t)taps * ldx, slab = (int64_t)cout * Q;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int t = (int)(i % taps);
    const int64_t r = i / taps;
    const int c = (int)(r % cin), n = (int)(r / cin);
    const float *p = partial + n * Q + (int64_t)t * ldx + c;
    float v = 0.f;
    for (int s = 0; s < S; ++s) v += p[s * slab];
    dw[i] = v;
  }
}

// ---- strided data gradient ------------------------------------------------------------------------------------------------------------
// Input pixels of one phase class (h % sh, w % sw) = (py, px) are reached by the same taps: kh with (py + ph - kh) % sh == 0 (likewise kw).
// A wave owns 32 pixels of a class and 32 TJ input channels; K runs over (reaching tap, output channel) in steps of 8 channels: the half-wave
// fh reads channels [4 fh, 4 fh + 4) of its pixel's dY row as one 16-byte load and the four MFMAs of the step take them in turn (the B operand
// -- packed weights [tap][co][ci] -- is read in the same channel order).
template <int TJ>
__global__ __launch_bounds__(256) void vdgrad_gather_kernel(const float *__restrict__ dy, int ldy, const float *__restrict__ wg, int ldx, VConvGeom g,
                                                             int64_t NT, float *__restrict__ dx) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 31, fh = lane >> 5;
  const int py = blockIdx.z / g.sw, px = blockIdx.z % g.sw;
  const int Hc = (g.Hi - py + g.sh - 1) / g.sh, Wc = (g.Wi - px + g.sw - 1) / g.sw;
  const int64_t crow = NT * Hc * Wc;   // pixels of this class
  const int64_t m0 = ((int64_t)blockIdx.x * 4 + wave) * 32;
  if (Hc <= 0 || Wc <= 0 || m0 >= crow) return;   // (wave-uniform; no barrier below)
  // this lane's A row: pixel m0 + fr of the class
  const int64_t m = m0 + fr;
  const bool mok = m < crow;
  int64_t nt = 0;
  int hi = 0, wi = 0;
  if (mok) {
    nt = m / ((int64_t)Hc * Wc);
    const int rem = (int)(m - nt * Hc * Wc);
    hi = (rem / Wc) * g.sh + py;
    wi = (rem % Wc) * g.sw + px;
  }
  const int c0 = blockIdx.y * 32 * TJ;
  f32x16 acc[TJ];
#pragma unroll
  for (int j = 0; j < TJ; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
  const int khr = (py + g.ph) % g.sh, kwr = (px + g.pw) % g.sw;   // first reaching kh / kw
  for (int kh = khr; kh < g.kh; kh += g.sh) {
    const int ho = (hi + g.ph - kh) / g.sh;   // exact: hi + ph - kh is a multiple of sh (and >= 0 checked below)
    const bool hok = mok && hi + g.ph - kh >= 0 && ho < g.Ho;
    for (int kw = kwr; kw < g.kw; kw += g.sw) {
      const int wo = (wi + g.pw - kw) / g.sw;
      const bool ok = hok && wi + g.pw - kw >= 0 && wo < g.Wo;
      const float *arow = dy + ((nt * g.Ho + (ok ? ho : 0)) * (int64_t)g.Wo + (ok ? wo : 0)) * ldy + 4 * fh;
      const float *brow = wg + ((int64_t)(kh * g.kw + kw) * ldy + 4 * fh) * ldx + c0 + fr;
#pragma unroll 2
      for (int k0 = 0; k0 < ldy; k0 += 8) {
        const f32x4 a = ok ? *reinterpret_cast<const f32x4 *>(arow + k0) : f32x4{0.f, 0.f, 0.f, 0.f};
        float b[4][TJ];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int j = 0; j < TJ; ++j) b[s][j] = (c0 + 32 * j + fr < ldx) ? brow[(int64_t)(k0 + s) * ldx + 32 * j] : 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int j = 0; j < TJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s][j], acc[j], 0, 0, 0);
      }
    }
  }
  // accumulator row i of this lane -> the destination row of pixel m0 + i (its source lane's A row, fetched by shuffle)
  const int64_t myrow = mok ? (nt * g.Hi + hi) * (int64_t)g.Wi + wi : -1;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int i = (e & 3) + 8 * (e >> 2) + 4 * fh;
    const int64_t row = __shfl(myrow, i);
    if (row < 0) continue;
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      const int c = c0 + 32 * j + fr;
      if (c < ldx) dx[row * ldx + c] = acc[j][e];
    }
  }
}

// ---- BatchNorm3d, train mode ----------------------------------------------------------------------------------------------------------
// slice statistics: part[s][c] = (mean, M2) of rows [s * rps, min(rows, (s + 1) * rps)); inside the slice the sums are taken about the
// slice's first value of the channel (a shifted one-pass form: no E[x^2] - E[x]^2 cancellation at offset inputs)
__global__ __launch_bounds__(256) void bn_stats_part_kernel(const float *__restrict__ x, int ld, int C, int64_t rows, int64_t rps,
                                                            float2 *__restrict__ part) {
  __shared__ float sh1[4][64], sh2[4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cx;
  const int64_t r0 = (int64_t)blockIdx.y * rps, r1 = min(rows, r0 + rps);
  float s1 = 0.f, s2 = 0.f;
  if (c < C && r0 < r1) {
    const float k = x[r0 * ld + c];
    for (int64_t r = r0 + ry; r < r1; r += 4) {
      const float d = x[r * ld + c] - k;
      s1 += d;
      s2 = fmaf(d, d, s2);
    }
  }
  sh1[ry][cx] = s1;
  sh2[ry][cx] = s2;
  __syncthreads();
  if (ry == 0 && c < C && r0 < r1) {
    const float t1 = (sh1[0][cx] + sh1[1][cx]) + (sh1[2][cx] + sh1[3][cx]);
    const float t2 = (sh2[0][cx] + sh2[1][cx]) + (sh2[2][cx] + sh2[3][cx]);
    const float n = (float)(r1 - r0), d = t1 / n;
    part[(int64_t)blockIdx.y * C + c] = make_float2(x[r0 * ld + c] + d, fmaxf(t2 - t1 * d, 0.f));
  }
}

// merge the slices in order, save (mean, 1/std), update the running statistics, and leave gamma / std for the apply pass
__global__ void bn_stats_final_kernel(const float2 *__restrict__ part, int S, int64_t rows, int64_t rps, int C, const float *__restrict__ gamma,
                                      const float *__restrict__ beta, float eps, float momentum, float *__restrict__ run_mean,
                                      float *__restrict__ run_var, int64_t *__restrict__ nbt, float *__restrict__ save_mean,
                                      float *__restrict__ save_invstd, float *__restrict__ scale) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0 && nbt) *nbt += 1;
  if (c >= C) return;
  // two passes over the slices: the mean about the first slice's mean m0 (the sum of n_s (mean_s - m0) stays small next to an offset mean and
  // the mean is rounded once), then M2 = sum M2_s + n_s (mean_s - mean)^2
  const float m0 = part[c].x;
  float dsum = 0.f;
  for (int s = 0; s < S; ++s) {
    const int64_t r0 = (int64_t)s * rps;
    if (r0 >= rows) break;
    dsum += (float)(min(rows, r0 + rps) - r0) * (part[(int64_t)s * C + c].x - m0);
  }
  const float mean = m0 + dsum / (float)rows;
  float m2 = 0.f;
  for (int s = 0; s < S; ++s) {
    const int64_t r0 = (int64_t)s * rps;
    if (r0 >= rows) break;
    const float2 p = part[(int64_t)s * C + c];
    const float d = p.x - mean;
    m2 += p.y + (float)(min(rows, r0 + rps) - r0) * d * d;
  }
  const float var = m2 / (float)rows;
  const float inv = 1.f / sqrtf(var + eps);
  save_mean[c] = mean;
  save_invstd[c] = inv;
  if (run_mean) run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * mean;
  if (run_var) run_var[c] = (1.f - momentum) * run_var[c] + momentum * (m2 / (float)(rows - 1));
  scale[c] = gamma[c] * inv;
}

// y = act((x - mean) * scale + beta (+ res)); columns [C, ld) are written as zeros.  (x - mean first: x * scale + (beta - mean * scale) would
// lose beta next to a large offset mean times a large scale -- a constant channel has scale gamma / sqrt(eps))
__global__ void bn_apply_kernel(const float *__restrict__ x, const float *__restrict__ res, int ld, int C, int64_t rows, const float *__restrict__ mean,
                                const float *__restrict__ scale, const float *__restrict__ beta, int relu, float *__restrict__ y) {
  const int64_t total = rows * (ld / 4);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(i % (ld / 4)) * 4;
    const f32x4 v = reinterpret_cast<const f32x4 *>(x)[i];
    f32x4 r = res ? reinterpret_cast<const f32x4 *>(res)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = c0 + e;
      float z = c < C ? fmaf(v[e] - mean[c], scale[c], beta[c]) + r[e] : 0.f;
      o[e] = relu ? fmaxf(z, 0.f) : z;
    }
    reinterpret_cast<f32x4 *>(y)[i] = o;
  }
}

// backward slice sums: part[s][0][c] = sum dz, part[s][1][c] = sum dz * xhat,  dz = relu ? dy * (y > 0) : dy
__global__ __launch_bounds__(256) void bn_bwd_part_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ dy, int ld,
                                                          int C, int64_t rows, int64_t rps, const float *__restrict__ mean,
                                                          const float *__restrict__ invstd, float *__restrict__ part) {
  __shared__ float sh1[4][64], sh2[4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cx;
  const int64_t r0 = (int64_t)blockIdx.y * rps, r1 = min(rows, r0 + rps);
  float s1 = 0.f, s2 = 0.f;
  if (c < C) {
    const float mu = mean[c], is = invstd[c];
    for (int64_t r = r0 + ry; r < r1; r += 4) {
      const int64_t o = r * ld + c;
      const float dz = (y && !(y[o] > 0.f)) ? 0.f : dy[o];
      s1 += dz;
      s2 = fmaf(dz, (x[o] - mu) * is, s2);
    }
  }
  sh1[ry][cx] = s1;
  sh2[ry][cx] = s2;
  __syncthreads();
  if (ry == 0 && c < C) {
    part[((int64_t)blockIdx.y * 2) * C + c] = (sh1[0][cx] + sh1[1][cx]) + (sh1[2][cx] + sh1[3][cx]);
    part[((int64_t)blockIdx.y * 2 + 1) * C + c] = (sh2[0][cx] + sh2[1][cx]) + (sh2[2][cx] + sh2[3][cx]);
  }
}

// dbeta = sum dz, dgamma = sum dz xhat (slices in order); coef = (gamma invstd, mean(dz), mean(dz xhat))
__global__ void bn_bwd_final_kernel(const float *__restrict__ part, int S, int64_t rows, int C, const float *__restrict__ gamma,
                                    const float *__restrict__ invstd, float *__restrict__ dgamma, float *__restrict__ dbeta, float *__restrict__ coef) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float a = 0.f, b = 0.f;
  for (int s = 0; s < S; ++s) {
    a += part[((int64_t)s * 2) * C + c];
    b += part[((int64_t)s * 2 + 1) * C + c];
  }
  if (dbeta) dbeta[c] = a;
  if (dgamma) dgamma[c] = b;
  coef[c] = gamma[c] * invstd[c];
  coef[C + c] = a / (float)rows;
  coef[2 * C + c] = b / (float)rows;
}

// dx = gamma invstd (dz - mean(dz) - xhat mean(dz xhat));  dres = dz (the residual branch's gradient);  columns [C, ld) -> 0
__global__ void bn_bwd_apply_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ dy, int ld, int C, int64_t rows,
                                    const float *__restrict__ mean, const float *__restrict__ invstd, const float *__restrict__ coef,
                                    float *__restrict__ dx, float *__restrict__ dres) {
  const int64_t total = rows * (ld / 4);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(i % (ld / 4)) * 4;
    const f32x4 xv = reinterpret_cast<const f32x4 *>(x)[i], dv = reinterpret_cast<const f32x4 *>(dy)[i];
    const f32x4 yv = y ? reinterpret_cast<const f32x4 *>(y)[i] : f32x4{1.f, 1.f, 1.f, 1.f};
    f32x4 o, z;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = c0 + e;
      if (c < C) {
        const float dz = yv[e] > 0.f ? dv[e] : 0.f;
        z[e] = dz;
        o[e] = coef[c] * (dz - coef[C + c] - (xv[e] - mean[c]) * invstd[c] * coef[2 * C + c]);
      } else {
        z[e] = 0.f;
        o[e] = 0.f;
      }
    }
    if (dx) reinterpret_cast<f32x4 *>(dx)[i] = o;
    if (dres) reinterpret_cast<f32x4 *>(dres)[i] = z;
  }
}

// ---- BatchNorm3d, train mode, statistics shared by the ranks of a data-parallel group ---------------------------------------------------------
// Each direction is cut where the per-channel numbers are small: a rank reduces its own rows to one pair per channel, the caller gathers the
// (world, C, 2) table of all ranks, and every rank merges that table in rank order: identical input, identical order, identical bits on every rank.
// The row counts travel beside the table as exact int64 values.

// local statistics: out[c] = (mean, M2) of this rank's rows; the slices in order, in bn_stats_final_kernel's two-pass form
__global__ void bn_stats_merge_kernel(const float2 *__restrict__ part, int S, int64_t rows, int64_t rps, int C, float2 *__restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float m0 = part[c].x;
  float dsum = 0.f;
  for (int s = 0; s < S; ++s) {
    const int64_t r0 = (int64_t)s * rps;
    if (r0 >= rows) break;
    dsum += (float)(min(rows, r0 + rps) - r0) * (part[(int64_t)s * C + c].x - m0);
  }
  const float mean = m0 + dsum / (float)rows;
  float m2 = 0.f;
  for (int s = 0; s < S; ++s) {
    const int64_t r0 = (int64_t)s * rps;
    if (r0 >= rows) break;
    const float2 p = part[(int64_t)s * C + c];
    const float d = p.x - mean;
    m2 += p.y + (float)(min(rows, r0 + rps) - r0) * d * d;
  }
  out[c] = make_float2(mean, m2);
}

// merge the ranks' (mean, M2) in rank order (the mean about rank 0's mean, then M2 = sum M2_r + n_r (mean_r - mean)^2), save (mean, 1/std), update
// the running statistics with the unbiased variance over the total row count, and leave gamma / std for the apply pass
__global__ void bn_sync_final_kernel(const float2 *__restrict__ tab, const int64_t *__restrict__ counts, int world, int C, const float *__restrict__ gamma,
                                     float eps, float momentum, float *__restrict__ run_mean, float *__restrict__ run_var, int64_t *__restrict__ nbt,
                                     float *__restrict__ save_mean, float *__restrict__ save_invstd, float *__restrict__ scale) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0 && nbt) *nbt += 1;
  if (c >= C) return;
  const float m0 = tab[c].x;
  int64_t total = 0;
  float dsum = 0.f;
  for (int r = 0; r < world; ++r) {
    const int64_t n = counts[r];
    total += n;
    dsum += (float)n * (tab[(int64_t)r * C + c].x - m0);
  }
  const float mean = m0 + dsum / (float)total;
  float m2 = 0.f;
  for (int r = 0; r < world; ++r) {
    const float2 p = tab[(int64_t)r * C + c];
    const float d = p.x - mean;
    m2 += p.y + (float)counts[r] * d * d;
  }
  const float var = m2 / (float)total;
  const float inv = 1.f / sqrtf(var + eps);
  save_mean[c] = mean;
  save_invstd[c] = inv;
  if (run_mean) run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * mean;
  if (run_var) run_var[c] = (1.f - momentum) * run_var[c] + momentum * (m2 / (float)(total - 1));
  scale[c] = gamma[c] * inv;
}

// local backward sums: out[c] = (sum dz, sum dz xhat) over this rank's rows (slices in order); dbeta / dgamma are these LOCAL sums, as in
// torch.nn.SyncBatchNorm (the gradient all-reduce averages them afterwards)
__global__ void bn_bwd_merge_kernel(const float *__restrict__ part, int S, int C, float2 *__restrict__ out, float *__restrict__ dgamma,
                                    float *__restrict__ dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float a = 0.f, b = 0.f;
  for (int s = 0; s < S; ++s) {
    a += part[((int64_t)s * 2) * C + c];
    b += part[((int64_t)s * 2 + 1) * C + c];
  }
  out[c] = make_float2(a, b);
  if (dbeta) dbeta[c] = a;
  if (dgamma) dgamma[c] = b;
}

// the ranks' sums added in rank order, over the total row count: coef = (gamma invstd, mean(dz), mean(dz xhat)) for bn_bwd_apply_kernel
__global__ void bn_sync_bwd_coef_kernel(const float2 *__restrict__ tab, const int64_t *__restrict__ counts, int world, int C,
                                        const float *__restrict__ gamma, const float *__restrict__ invstd, float *__restrict__ coef) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  int64_t total = 0;
  float a = 0.f, b = 0.f;
  for (int r = 0; r < world; ++r) {
    const float2 p = tab[(int64_t)r * C + c];
    total += counts[r];
    a += p.x;
    b += p.y;
  }
  coef[c] = gamma[c] * invstd[c];
  coef[C + c] = a / (float)total;
  coef[2 * C + c] = b / (float)total;
}

// spatial mean pool backward: dx[(nt * HW + p) * ld + c] = c < C ? dp[nt * C + c] / HW : 0
__global__ void pool_bwd_kernel(const float *__restrict__ dp, int64_t NT, int HW, int C, int ld, float *__restrict__ dx) {
  const int64_t total = NT * HW * ld;
  const float inv = 1.f / (float)HW;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % ld);
    const int64_t nt = i / ld / HW;
    dx[i] = c < C ? dp[nt * C + c] * inv : 0.f;
  }
}

}  // namespace

// ---- launchers --------------------------------------------------------------------------------------------------------------------------
int vconv_k(int taps, int ld) { return (taps * ld + 31) / 32 * 32; }

hipError_t launch_vconv_pack_fwd(const float *w, const VConvGeom &g, int cin_ld, float *out, hipStream_t s) {
  const int K = vconv_k(g.taps(), cin_ld);   // rows padded to a multiple of 32 with zeros, as the engine packs them
  if (K != g.taps() * cin_ld) {
    hipError_t e = hipMemsetAsync(out, 0, (size_t)g.cout * K * sizeof(float), s);
    if (e != hipSuccess) return e;
  }
  return launch_pack_conv(F32, w, g.cout, g.cin, 0, g.cin, g.taps(), cin_ld, nullptr, out, K, 0, s);
}

hipError_t launch_vconv_fwd(const float *x, int cin_ld, const float *wpk, const VConvGeom &g, int64_t NT, float *y, int cout_ld, hipStream_t s) {
  ConvGemmArgs a = vconv_args(g, NT, x, cin_ld, wpk, vconv_k(g.taps(), cin_ld), y, cout_ld);
  a.n_store = cout_ld;
  a.solo = 1;
  return launch_conv_gemm(F32, a, s);
}

hipError_t launch_vconv_dgrad_s1(const float *dy, int cout_ld, const float *w, const VConvGeom &g, int64_t NT, float *wflip, float *dx, int cin_ld,
                                 hipStream_t s) {
  const int K = vconv_k(g.taps(), cout_ld);
  hipLaunchKernelGGL(pack_dgrad_flip_kernel, grid1d((int64_t)g.cin * K), dim3(kTPB), 0, s, w, g.cout, g.cin, g.taps(), cout_ld, K, wflip);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // the transposed convolution of a stride-1 'same' convolution: the same geometry with the output and input roles swapped
  VConvGeom t = g;
  t.cin = g.cout;
  t.cout = g.cin;
  t.Hi = g.Ho;
  t.Wi = g.Wo;
  t.Ho = g.Hi;
  t.Wo = g.Wi;
  t.pt = g.kt - 1 - g.pt;
  t.ph = g.kh - 1 - g.ph;
  t.pw = g.kw - 1 - g.pw;
  return launch_vconv_fwd(dy, cout_ld, wflip, t, NT, dx, cin_ld, s);
}

hipError_t launch_vconv_dgrad_gather(const float *dy, int cout_ld, const float *w, const VConvGeom &g, int64_t NT, float *wg, float *dx, int cin_ld,
                                     hipStream_t s) {
  if (g.kt != 1 || g.pt != 0 || cout_ld % 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pack_dgrad_gather_kernel, grid1d((int64_t)g.taps() * cout_ld * cin_ld), dim3(kTPB), 0, s, w, g.cout, g.cin, g.taps(), cout_ld,
                     cin_ld, wg);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  int64_t maxc = 0;   // pixels of the largest phase class
  for (int py = 0; py < g.sh; ++py)
    for (int px = 0; px < g.sw; ++px)
      maxc = std::max<int64_t>(maxc, NT * ((g.Hi - py + g.sh - 1) / g.sh) * ((g.Wi - px + g.sw - 1) / g.sw));
  const int TJ = cin_ld > 32 ? 2 : 1;
  dim3 grid((unsigned)((maxc + 127) / 128), (unsigned)((cin_ld + 32 * TJ - 1) / (32 * TJ)), (unsigned)(g.sh * g.sw));
  if (TJ == 2) hipLaunchKernelGGL(vdgrad_gather_kernel<2>, grid, dim3(256), 0, s, dy, cout_ld, wg, cin_ld, g, NT, dx);
  else hipLaunchKernelGGL(vdgrad_gather_kernel<1>, grid, dim3(256), 0, s, dy, cout_ld, wg, cin_ld, g, NT, dx);
  return hipGetLastError();
}

int vwgrad_splits(int64_t rows, const VConvGeom &g, int cin_ld) {
  const int64_t tiles = (int64_t)((g.cout + 63) / 64) * ((g.taps() * cin_ld + 63) / 64);
  int64_t S = (2048 + tiles - 1) / tiles;                            // ~2048 workgroups
  S = std::min<int64_t>(S, std::max<int64_t>(1, rows / 512));        // >= 512 rows per slice
  const int64_t slab = (int64_t)g.cout * g.taps() * cin_ld;
  S = std::min<int64_t>(S, std::max<int64_t>(1, (int64_t(64) << 20) / slab));   // partials <= 256 MB
  return (int)std::max<int64_t>(1, S);
}

hipError_t launch_vconv_wgrad(const float *dy, int cout_ld, const float *x, int cin_ld, const VConvGeom &g, int64_t NT, float *partial, int S, float *dw,
                              hipStream_t s) {
  const int64_t rows = NT * g.Ho * g.Wo;
  const int64_t rps = ((rows + S - 1) / S + 7) / 8 * 8;   // whole row octets per slice (a wave's row walk)
  const int Q = g.taps() * cin_ld;
  dim3 grid((unsigned)((g.cout + 63) / 64), (unsigned)((Q + 63) / 64), (unsigned)((rows + rps - 1) / rps));
  hipLaunchKernelGGL((vwgrad_kernel<2, 2>), grid, dim3(256), 0, s, dy, cout_ld, x, cin_ld, g, rows, rps, partial);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(vwgrad_reduce_kernel, grid1d((int64_t)g.cout * g.cin * g.taps()), dim3(kTPB), 0, s, partial, (int)grid.z, g.cout, g.cin, g.taps(),
                     cin_ld, dw);
  return hipGetLastError();
}

int bn_train_slices(int64_t rows, int C) {
  const int64_t cb = (C + 63) / 64;
  int64_t S = (1024 + cb - 1) / cb;
  S = std::min<int64_t>(S, std::max<int64_t>(1, rows / 256));
  return (int)std::max<int64_t>(1, S);
}

hipError_t launch_bn_train_fwd(const float *x, const float *res, int ld, int C, int64_t rows, const float *gamma, const float *beta, float eps,
                               float momentum, float *run_mean, float *run_var, int64_t *nbt, int relu, float *y, float *save_mean, float *save_invstd,
                               float *ws, hipStream_t s) {
  const int S = bn_train_slices(rows, C);
  const int64_t rps = (rows + S - 1) / S;
  float2 *part = reinterpret_cast<float2 *>(ws);
  float *ss = ws + 2 * (int64_t)S * C;
  hipLaunchKernelGGL(bn_stats_part_kernel, dim3((C + 63) / 64, S), dim3(256), 0, s, x, ld, C, rows, rps, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3((C + 255) / 256), dim3(256), 0, s, part, S, rows, rps, C, gamma, beta, eps, momentum, run_mean, run_var,
                     nbt, save_mean, save_invstd, ss);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(bn_apply_kernel, grid1d(rows * (ld / 4)), dim3(kTPB), 0, s, x, res, ld, C, rows, save_mean, ss, beta, relu, y);
  return hipGetLastError();
}

hipError_t launch_bn_train_bwd(const float *x, const float *y, const float *dy, int ld, int C, int64_t rows, const float *gamma, const float *mean,
                               const float *invstd, float *dx, float *dres, float *dgamma, float *dbeta, float *ws, hipStream_t s) {
  const int S = bn_train_slices(rows, C);
  const int64_t rps = (rows + S - 1) / S;
  float *part = ws, *coef = ws + 2 * (int64_t)S * C;
  hipLaunchKernelGGL(bn_bwd_part_kernel, dim3((C + 63) / 64, S), dim3(256), 0, s, x, y, dy, ld, C, rows, rps, mean, invstd, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((C + 255) / 256), dim3(256), 0, s, part, S, rows, C, gamma, invstd, dgamma, dbeta, coef);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(bn_bwd_apply_kernel, grid1d(rows * (ld / 4)), dim3(kTPB), 0, s, x, y, dy, ld, C, rows, mean, invstd, coef, dx, dres);
  return hipGetLastError();
}

hipError_t launch_bn_sync_stats(const float *x, int ld, int C, int64_t rows, float *local, float *ws, hipStream_t s) {
  const int S = bn_train_slices(rows, C);
  const int64_t rps = (rows + S - 1) / S;
  float2 *part = reinterpret_cast<float2 *>(ws);
  hipLaunchKernelGGL(bn_stats_part_kernel, dim3((C + 63) / 64, S), dim3(256), 0, s, x, ld, C, rows, rps, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(bn_stats_merge_kernel, dim3((C + 255) / 256), dim3(256), 0, s, part, S, rows, rps, C, reinterpret_cast<float2 *>(local));
  return hipGetLastError();
}

hipError_t launch_bn_sync_fwd_apply(const float *x, const float *res, int ld, int C, int64_t rows, const float *gathered, const int64_t *counts, int world,
                                    const float *gamma, const float *beta, float eps, float momentum, float *run_mean, float *run_var, int64_t *nbt,
                                    int relu, float *y, float *save_mean, float *save_invstd, float *ws, hipStream_t s) {
  float *ss = ws;   // gamma / std: C floats
  hipLaunchKernelGGL(bn_sync_final_kernel, dim3((C + 255) / 256), dim3(256), 0, s, reinterpret_cast<const float2 *>(gathered), counts, world, C, gamma, eps,
                     momentum, run_mean, run_var, nbt, save_mean, save_invstd, ss);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(bn_apply_kernel, grid1d(rows * (ld / 4)), dim3(kTPB), 0, s, x, res, ld, C, rows, save_mean, ss, beta, relu, y);
  return hipGetLastError();
}

hipError_t launch_bn_sync_bwd_sums(const float *x, const float *y, const float *dy, int ld, int C, int64_t rows, const float *mean, const float *invstd,
                                   float *local, float *dgamma, float *dbeta, float *ws, hipStream_t s) {
  const int S = bn_train_slices(rows, C);
  const int64_t rps = (rows + S - 1) / S;
  hipLaunchKernelGGL(bn_bwd_part_kernel, dim3((C + 63) / 64, S), dim3(256), 0, s, x, y, dy, ld, C, rows, rps, mean, invstd, ws);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(bn_bwd_merge_kernel, dim3((C + 255) / 256), dim3(256), 0, s, ws, S, C, reinterpret_cast<float2 *>(local), dgamma, dbeta);
  return hipGetLastError();
}

hipError_t launch_bn_sync_bwd_apply(const float *x, const float *y, const float *dy, int ld, int C, int64_t rows, const float *gathered,
                                    const int64_t *counts, int world, const float *gamma, const float *mean, const float *invstd, float *dx, float *dres,
                                    float *ws, hipStream_t s) {
  float *coef = ws;   // 3 * C floats
  hipLaunchKernelGGL(bn_sync_bwd_coef_kernel, dim3((C + 255) / 256), dim3(256), 0, s, reinterpret_cast<const float2 *>(gathered), counts, world, C, gamma,
                     invstd, coef);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(bn_bwd_apply_kernel, grid1d(rows * (ld / 4)), dim3(kTPB), 0, s, x, y, dy, ld, C, rows, mean, invstd, coef, dx, dres);
  return hipGetLastError();
}

hipError_t launch_pool_bwd(const float *dp, int64_t NT, int HW, int C, int ld, float *dx, hipStream_t s) {
  hipLaunchKernelGGL(pool_bwd_kernel, grid1d(NT * HW * ld), dim3(kTPB), 0, s, dp, NT, HW, C, ld, dx);
  return hipGetLastError();
}

}  // namespace sf
