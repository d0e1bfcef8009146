// Swin transformer pieces of the CLAP audio embedder (HTSAT), fp32.
//
//   window_attention_kernel<D>  one wave per (clip, window, head), one lane per query token of the 8 x 8 window.  The window partition, the
//                               cyclic shift and their inverses are index arithmetic on the loads and the store: lane (y, x) of window
//                               (wy, wx) reads and writes the token at ((8 wy + y + shift) mod H, (8 wx + x + shift) mod W).  k and v of the
//                               window-head sit in LDS (2 * 64 * D floats) and are read as broadcasts; q, the 64 scores and the D outputs
//                               of a query stay in its lane's registers, so the softmax needs no cross-lane step and every sum runs in
//                               key order.  The two contractions are vector FMAs: with a lane per query the operands of q k^T and P v are
//                               one register and one LDS broadcast, no fragment shuffles, and the attention is ~4 % of the network's
//                               FLOPs (the fp32 MFMA rate is only twice the vector rate).  The relative-position bias of the head (225
//                               floats) sits in LDS; the shift mask is recomputed from the rolled-frame coordinates (no mask tensor).
//   swin_layernorm_kernel       row LayerNorm without affine, one wave per row, two passes over registers; optionally gathers the 2 x 2
//                               PatchMerging neighbourhood as its source (4 C columns), so no merged copy is ever written un-normalised.
#include "clap.h"
#include "common.h"

namespace sf {

namespace {

constexpr int WS = SWIN_WINDOW, WT = WS * WS;       // window side, tokens per window
constexpr int NB = (2 * WS - 1) * (2 * WS - 1);     // relative-position bias entries per head

// region of a rolled-frame coordinate for the shift mask: [0, n - 8), [n - 8, n - 4), [n - 4, n)
__device__ __forceinline__ int shift_region(int p, int n) { return p < n - WS ? 0 : (p < n - WS / 2 ? 1 : 2); }

template <int D>
__global__ __launch_bounds__(WT) void window_attention_kernel(const float *__restrict__ qkv, int H, int W, int C, int heads, int shift,
                                                              const float *__restrict__ table, float mask_value, float scale,
                                                              float *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) float ks[WT * D];
  __shared__ __attribute__((aligned(16))) float vs[WT * D];
  __shared__ float tb[NB];
  const int lane = threadIdx.x;
  const int nwx = W / WS, nwy = H / WS;
  int t = blockIdx.x;
  const int head = t % heads;
  t /= heads;
  const int wx = t % nwx;
  t /= nwx;
  const int wy = t % nwy;
  const int b = t / nwy;
  const int yi = lane >> 3, xi = lane & 7;
  const int hp = wy * WS + yi, wp = wx * WS + xi;   // rolled-frame coordinates
  int h = hp + shift, w = wp + shift;               // the token they hold
  if (h >= H) h -= H;
  if (w >= W) w -= W;
  const int64_t row = ((int64_t)b * H + h) * W + w;
  const float *p = qkv + row * (3 * (int64_t)C) + head * D;

  float q[D];
#pragma unroll
  for (int c = 0; c < D / 4; ++c) {
    const float4 a = *reinterpret_cast<const float4 *>(p + 4 * c);
    const float4 kk = *reinterpret_cast<const float4 *>(p + C + 4 * c);
    const float4 vv = *reinterpret_cast<const float4 *>(p + 2 * C + 4 * c);
    q[4 * c] = a.x * scale, q[4 * c + 1] = a.y * scale, q[4 * c + 2] = a.z * scale, q[4 * c + 3] = a.w * scale;
    *reinterpret_cast<float4 *>(&ks[lane * D + 4 * c]) = kk;
    *reinterpret_cast<float4 *>(&vs[lane * D + 4 * c]) = vv;
  }
  for (int i = lane; i < NB; i += WT) tb[i] = table[(int64_t)i * heads + head];
  __syncthreads();

  float sc[WT];
#pragma unroll
  for (int j = 0; j < WT; ++j) {
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < D / 4; ++c) {
      const float4 kk = *reinterpret_cast<const float4 *>(&ks[j * D + 4 * c]);
      a = fmaf(q[4 * c], kk.x, a);
      a = fmaf(q[4 * c + 1], kk.y, a);
      a = fmaf(q[4 * c + 2], kk.z, a);
      a = fmaf(q[4 * c + 3], kk.w, a);
    }
    sc[j] = a;
  }
  // relative-position bias: entry (yi - yj + 7) * 15 + (xi - xj + 7), query minus key
  const int base = (yi + WS - 1) * (2 * WS - 1) + xi + WS - 1;
#pragma unroll
  for (int j = 0; j < WT; ++j) sc[j] += tb[base - ((j >> 3) * (2 * WS - 1) + (j & 7))];
  if (shift) {
    const int reg = shift_region(hp, H) * 3 + shift_region(wp, W);
#pragma unroll
    for (int j = 0; j < WT; ++j) {
      const int rj = shift_region(wy * WS + (j >> 3), H) * 3 + shift_region(wx * WS + (j & 7), W);
      sc[j] += rj != reg ? mask_value : 0.f;
    }
  }
  float m = sc[0];
#pragma unroll
  for (int j = 1; j < WT; ++j) m = fmaxf(m, sc[j]);
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < WT; ++j) {
    sc[j] = expf(sc[j] - m);
    sum += sc[j];
  }
  float o[D];
#pragma unroll
  for (int d = 0; d < D; ++d) o[d] = 0.f;
#pragma unroll
  for (int j = 0; j < WT; ++j) {
#pragma unroll
    for (int c = 0; c < D / 4; ++c) {
      const float4 vv = *reinterpret_cast<const float4 *>(&vs[j * D + 4 * c]);
      o[4 * c] = fmaf(sc[j], vv.x, o[4 * c]);
      o[4 * c + 1] = fmaf(sc[j], vv.y, o[4 * c + 1]);
      o[4 * c + 2] = fmaf(sc[j], vv.z, o[4 * c + 2]);
      o[4 * c + 3] = fmaf(sc[j], vv.w, o[4 * c + 3]);
    }
  }
  const float inv = 1.0f / sum;
  float *dst = out + row * C + head * D;
#pragma unroll
  for (int c = 0; c < D / 4; ++c)
    *reinterpret_cast<float4 *>(dst + 4 * c) = make_float4(o[4 * c] * inv, o[4 * c + 1] * inv, o[4 * c + 2] * inv, o[4 * c + 3] * inv);
}

template <int D>
hipError_t attn_go(const float *qkv, int B, int H, int W, int C, int heads, int shift, const float *table, float mask_value, float *out,
                   hipStream_t s) {
  const int64_t grid = (int64_t)B * (H / WS) * (W / WS) * heads;
  hipLaunchKernelGGL((window_attention_kernel<D>), dim3((unsigned)grid), dim3(WT), 0, s, qkv, H, W, C, heads, shift, table, mask_value,
                     1.0f / sqrtf((float)D), out);
  return hipGetLastError();
}

constexpr int LN_ROWS = 4;        // rows (waves) per workgroup
constexpr int LN_MAXV = 32;       // values per lane: C <= 2048

__global__ __launch_bounds__(LN_ROWS *WAVE) void swin_layernorm_kernel(const float *__restrict__ x, int64_t rows_out, int C, float eps, int merge,
                                                                       int H, int W, float *__restrict__ y) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t m = (int64_t)blockIdx.x * LN_ROWS + (threadIdx.x >> 6);
  if (m >= rows_out) return;
  const float *src = x + m * C;   // merge: the (2 h2, 2 w2) token; segment q sits ((q & 1) W + (q >> 1)) tokens further
  int cin = C;
  if (merge) {
    cin = C / 4;
    const int W2 = W / 2, H2 = H / 2;
    const int w2 = (int)(m % W2);
    const int64_t r = m / W2;
    const int h2 = (int)(r % H2);
    const int64_t b = r / H2;
    src = x + (((b * H + 2 * h2) * W) + 2 * w2) * cin;
  }
  float v[LN_MAXV];
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < LN_MAXV; ++k) {
    const int c = k * WAVE + lane;
    v[k] = 0.f;
    if (c < C) {
      const int qd = c / cin;   // 0 without merge
      v[k] = src[(int64_t)((qd & 1) * W + (qd >> 1)) * cin + (c - qd * cin)];
      sum += v[k];
    }
  }
  const float mean = wave_sum(sum) / (float)C;
  float dev = 0.f;
#pragma unroll
  for (int k = 0; k < LN_MAXV; ++k) {
    const int c = k * WAVE + lane;
    if (c < C) {
      const float d = v[k] - mean;
      dev = fmaf(d, d, dev);
    }
  }
  const float rstd = rsqrtf(wave_sum(dev) / (float)C + eps);
  float *dst = y + m * C;
#pragma unroll
  for (int k = 0; k < LN_MAXV; ++k) {
    const int c = k * WAVE + lane;
    if (c < C) dst[c] = (v[k] - mean) * rstd;
  }
}

}  // namespace

hipError_t launch_window_attention(const float *qkv, int B, int H, int W, int C, int heads, int shift, const float *bias_table, float mask_value,
                                   float *out, hipStream_t s) {
  if (B < 1 || heads < 1 || C % heads || H % WS || W % WS || H < WS || W < WS || (shift != 0 && shift != WS / 2)) return hipErrorInvalidValue;
  if (shift && (H == WS || W == WS)) return hipErrorInvalidValue;
  switch (C / heads) {
    case 4: return attn_go<4>(qkv, B, H, W, C, heads, shift, bias_table, mask_value, out, s);
    case 8: return attn_go<8>(qkv, B, H, W, C, heads, shift, bias_table, mask_value, out, s);
    case 12: return attn_go<12>(qkv, B, H, W, C, heads, shift, bias_table, mask_value, out, s);
    case 16: return attn_go<16>(qkv, B, H, W, C, heads, shift, bias_table, mask_value, out, s);
    case 20: return attn_go<20>(qkv, B, H, W, C, heads, shift, bias_table, mask_value, out, s);
    case 24: return attn_go<24>(qkv, B, H, W, C, heads, shift, bias_table, mask_value, out, s);
    case 28: return attn_go<28>(qkv, B, H, W, C, heads, shift, bias_table, mask_value, out, s);
    case 32: return attn_go<32>(qkv, B, H, W, C, heads, shift, bias_table, mask_value, out, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_swin_layernorm(const float *x, int64_t rows_out, int C, float eps, int merge, int H, int W, float *y, hipStream_t s) {
  if (rows_out < 1 || C < 1 || C > LN_MAXV * WAVE) return hipErrorInvalidValue;
  if (merge && ((C % 4) || (H % 2) || (W % 2) || H < 2 || W < 2)) return hipErrorInvalidValue;
  const int64_t grid = (rows_out + LN_ROWS - 1) / LN_ROWS;
  if (grid > 0x7FFFFFFFll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(swin_layernorm_kernel, dim3((unsigned)grid), dim3(LN_ROWS * WAVE), 0, s, x, rows_out, C, eps, merge, H, W, y);
  return hipGetLastError();
}

}  // namespace sf
