// Front and tail of the CLAP audio embedder (HTSAT), fp32: everything between the mel power of the audio front end (audio_features.hip)
// and the first transformer block, and everything behind the last one.
//
//   logmel_image_kernel   mel power (B, n_mels, T) -> the S x S "image" the patch embed reads, one thread per pixel: 10 log10(max(P, amin)),
//                         the folded BatchNorm (one fma per value), bicubic interpolation along time (PyTorch's kernel, A = -0.75,
//                         align_corners, clamped borders) and the fold of the time axis into `ratio` bands of rows, in one pass.  The source
//                         position is exact integer arithmetic (t (T - 1) divided by (T' - 1) with remainder); the four taps are combined
//                         as v1 + sum w_i (v_i - v1), so a constant stretch (the zero padding of a short clip) comes out bit-exact.
//   patch_embed_kernel    Conv2d(1, E, 4, 4) + bias + LayerNorm(E): one wave per token, the 16-tap weights transposed in LDS, the E
//                         outputs of a token in its wave's registers (two-pass statistics).  K = 16 is too short for the GEMM launcher.
//   clap_pool_kernel, clap_linear_kernel, clap_l2norm_kernel   the tail, four launches: LayerNorm(C) and the mean over the tokens (one
//                         workgroup per clip), the two Linears (one wave per output, its weight row read once for every clip), the L2
//                         normalisation; every sum in a fixed order.  (One workgroup per clip for the whole tail measured 245 us at
//                         batch 4: a single CU streaming 2.5 MB of weights.)
#include "clap.h"
#include "common.h"

namespace sf {

namespace {

constexpr float CUBIC_A = -0.75f;
__device__ __forceinline__ float cubic_near(float t) { return ((CUBIC_A + 2.f) * t - (CUBIC_A + 3.f)) * t * t + 1.f; }                    // |t| <= 1
__device__ __forceinline__ float cubic_far(float t) { return ((CUBIC_A * t - 5.f * CUBIC_A) * t + 8.f * CUBIC_A) * t - 4.f * CUBIC_A; }   // 1 < |t| < 2

__global__ __launch_bounds__(256) void logmel_image_kernel(const float *__restrict__ mel, int64_t total, int n_mels, int T, int ratio,
                                                           const float *__restrict__ scale, const float *__restrict__ shift, float amin,
                                                           float db_floor, float *__restrict__ image) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int S = n_mels * ratio, Tt = S * ratio;
  const int tp = (int)(i % S);
  const int64_t rr = i / S;
  const int R = (int)(rr % S);
  const int64_t b = rr / S;
  const int r = R / n_mels, f = R - r * n_mels;
  const int to = r * S + tp;
  const float *row = mel + (b * n_mels + f) * T;
  const float sc = scale[f], sh = shift[f];
  auto val = [&](int t) {
    const float p = row[t];
    return fmaf(p <= amin ? db_floor : 10.f * log10f(p), sc, sh);
  };
  if (T == Tt) {
    image[i] = val(to);
    return;
  }
  const int num = to * (T - 1), den = Tt - 1;   // align_corners: source position to (T - 1) / (Tt - 1)
  const int i0 = num / den;
  const float fr = (float)(num - i0 * den) / (float)den;
  const float v0 = val(max(i0 - 1, 0)), v1 = val(i0), v2 = val(min(i0 + 1, T - 1)), v3 = val(min(i0 + 2, T - 1));
  float o = v1;
  o = fmaf(cubic_far(fr + 1.f), v0 - v1, o);
  o = fmaf(cubic_near(1.f - fr), v2 - v1, o);
  o = fmaf(cubic_far(2.f - fr), v3 - v1, o);
  image[i] = o;
}

constexpr int PE_WAVES = 4, PE_TOK = 4;   // waves per workgroup, tokens per wave
constexpr int PE_MAXV = 4;                // E <= 256

__global__ __launch_bounds__(PE_WAVES *WAVE) void patch_embed_kernel(const float *__restrict__ image, int64_t ntok, int S, int E,
                                                                     const float *__restrict__ w, const float *__restrict__ bias,
                                                                     const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
                                                                     float *__restrict__ tokens) {
  __shared__ float wt[16 * PE_MAXV * WAVE];   // [tap][e]
  __shared__ float aff[3 * PE_MAXV * WAVE];   // bias | gamma | beta
  for (int i = threadIdx.x; i < 16 * E; i += blockDim.x) wt[(i % 16) * E + i / 16] = w[i];
  for (int i = threadIdx.x; i < E; i += blockDim.x) aff[i] = bias[i], aff[E + i] = gamma[i], aff[2 * E + i] = beta[i];
  __syncthreads();
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
  const int P = S / 4;
  for (int k = 0; k < PE_TOK; ++k) {
    const int64_t tok = ((int64_t)blockIdx.x * PE_WAVES + wave) * PE_TOK + k;
    if (tok >= ntok) break;                   // (per wave: the reductions below stay whole)
    const int pw = (int)(tok % P);
    const int64_t r = tok / P;
    const int ph = (int)(r % P);
    const int64_t b = r / P;
    const float *src = image + (b * S + 4 * ph) * S + 4 * pw;
    float px[16];
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) {
      const float4 a = *reinterpret_cast<const float4 *>(src + (int64_t)ky * S);
      px[4 * ky] = a.x, px[4 * ky + 1] = a.y, px[4 * ky + 2] = a.z, px[4 * ky + 3] = a.w;
    }
    float v[PE_MAXV];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < PE_MAXV; ++j) {
      const int e = j * WAVE + lane;
      v[j] = 0.f;
      if (e < E) {
        float a = aff[e];
#pragma unroll
        for (int tp = 0; tp < 16; ++tp) a = fmaf(px[tp], wt[tp * E + e], a);
        v[j] = a;
        sum += a;
      }
    }
    const float mean = wave_sum(sum) / (float)E;
    float dev = 0.f;
#pragma unroll
    for (int j = 0; j < PE_MAXV; ++j)
      if (j * WAVE + lane < E) dev = fmaf(v[j] - mean, v[j] - mean, dev);
    const float rstd = rsqrtf(wave_sum(dev) / (float)E + eps);
#pragma unroll
    for (int j = 0; j < PE_MAXV; ++j) {
      const int e = j * WAVE + lane;
      if (e < E) tokens[tok * E + e] = fmaf((v[j] - mean) * rstd, aff[E + e], aff[2 * E + e]);
    }
  }
}

constexpr int TAIL_THREADS = 1024, TAIL_MAXC = 1024, TAIL_MAXJ = 1024, TAIL_MAXTOK = 256;
constexpr int LIN_WAVES = 4, LIN_MAXV = TAIL_MAXC / WAVE;   // waves (outputs) per workgroup of the tail's Linears; weights per lane

// x (B, ntok, C) -> pooled (B, C) = mean over the tokens of LayerNorm_C(x; gamma, beta): one workgroup per clip, a wave per token for the
// statistics, a lane per channel for the token sum (token order)
__global__ __launch_bounds__(TAIL_THREADS) void clap_pool_kernel(const float *__restrict__ x, int ntok, int C, const float *__restrict__ gamma,
                                                                 const float *__restrict__ beta, float eps, float *__restrict__ pooled) {
  __shared__ float st[TAIL_MAXTOK][2];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const float *xb = x + (int64_t)blockIdx.x * ntok * C;
  for (int t = wave; t < ntok; t += nw) {
    const float *r = xb + (int64_t)t * C;
    float s = 0.f;
    for (int c = lane; c < C; c += WAVE) s += r[c];
    const float mean = wave_sum(s) / (float)C;
    float d = 0.f;
    for (int c = lane; c < C; c += WAVE) d = fmaf(r[c] - mean, r[c] - mean, d);
    const float rstd = rsqrtf(wave_sum(d) / (float)C + eps);
    if (lane == 0) st[t][0] = mean, st[t][1] = rstd;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float a = 0.f;
    for (int t = 0; t < ntok; ++t) a += (xb[(int64_t)t * C + c] - st[t][0]) * st[t][1];
    pooled[(int64_t)blockIdx.x * C + c] = fmaf(a / (float)ntok, gamma[c], beta[c]);
  }
}

// y[b][n] = act(sum_k w[n][k] x[b x_ld + k] + bias[n]) for a handful of rows b: one wave per output n, its weight row in the lanes'
// registers (read once for every clip), wave-level sums in a fixed order: a clip's outputs do not depend on the batch.  K <= 1024.
// act: CLAP_ACT_NONE, CLAP_ACT_RELU, CLAP_ACT_TANH
__global__ __launch_bounds__(LIN_WAVES *WAVE) void clap_linear_kernel(const float *__restrict__ x, int64_t x_ld, int B, int K, int N,
                                                                      const float *__restrict__ w, const float *__restrict__ bias, int act,
                                                                      float *__restrict__ y) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int n = blockIdx.x * LIN_WAVES + (threadIdx.x >> 6);
  if (n >= N) return;
  const float *wr = w + (int64_t)n * K;
  float wv[LIN_MAXV];
#pragma unroll
  for (int j = 0; j < LIN_MAXV; ++j) wv[j] = j * WAVE + lane < K ? wr[j * WAVE + lane] : 0.f;
  const float bn = bias[n];
  for (int b = 0; b < B; ++b) {
    const float *xr = x + (int64_t)b * x_ld;
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < LIN_MAXV; ++j)
      if (j * WAVE + lane < K) a = fmaf(wv[j], xr[j * WAVE + lane], a);
    a = wave_sum(a) + bn;
    if (lane == 0) y[(int64_t)b * N + n] = act == CLAP_ACT_RELU ? fmaxf(a, 0.f) : act == CLAP_ACT_TANH ? tanhf(a) : a;
  }
}

// out[b][:] = x[b][:] / max(|x[b]|, 1e-12) (normalize) or a copy: one wave per clip
__global__ __launch_bounds__(WAVE) void clap_l2norm_kernel(const float *__restrict__ x, int J, int normalize, float *__restrict__ out) {
  const int lane = threadIdx.x;
  const float *xr = x + (int64_t)blockIdx.x * J;
  float s = 0.f;
  for (int n = lane; n < J; n += WAVE) s = fmaf(xr[n], xr[n], s);
  const float scale = normalize ? 1.0f / fmaxf(sqrtf(wave_sum(s)), 1e-12f) : 1.0f;
  for (int n = lane; n < J; n += WAVE) out[(int64_t)blockIdx.x * J + n] = xr[n] * scale;
}

}  // namespace

hipError_t launch_logmel_image(const float *mel, int B, int n_mels, int T, int ratio, const float *scale, const float *shift, float amin,
                               float db_floor, float *image, hipStream_t s) {
  if (B < 1 || n_mels < 1 || ratio < 1 || T < 2) return hipErrorInvalidValue;
  const int64_t S = (int64_t)n_mels * ratio, Tt = S * ratio;
  if (S > 4096 || T > Tt) return hipErrorInvalidValue;   // (to (T - 1) stays far below 2^31)
  const int64_t total = (int64_t)B * S * S;
  if (total >= (1ll << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(logmel_image_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, mel, total, n_mels, T, ratio, scale, shift, amin,
                     db_floor, image);
  return hipGetLastError();
}

hipError_t launch_patch_embed(const float *image, int B, int S, int E, const float *w, const float *bias, const float *gamma, const float *beta,
                              float eps, float *tokens, hipStream_t s) {
  if (B < 1 || S < 4 || (S % 4) || E < 1 || E > PE_MAXV * WAVE) return hipErrorInvalidValue;
  const int64_t ntok = (int64_t)B * (S / 4) * (S / 4);
  const int64_t grid = (ntok + PE_WAVES * PE_TOK - 1) / (PE_WAVES * PE_TOK);
  if (grid > 0x7FFFFFFFll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(patch_embed_kernel, dim3((unsigned)grid), dim3(PE_WAVES * WAVE), 0, s, image, ntok, S, E, w, bias, gamma, beta, eps, tokens);
  return hipGetLastError();
}

hipError_t launch_clap_tail(const float *x, int B, int ntok, int C, int J, const float *gamma, const float *beta, float eps, const float *w1,
                            const float *b1, const float *w2, const float *b2, int relu, int normalize, float *scratch, float *out, hipStream_t s) {
  if (B < 1 || ntok < 1 || ntok > TAIL_MAXTOK || C < 1 || C > TAIL_MAXC || J < 1 || J > TAIL_MAXJ || !scratch) return hipErrorInvalidValue;
  float *pooled = scratch, *hid = pooled + (int64_t)B * C, *emb = hid + (int64_t)B * J;
  hipLaunchKernelGGL(clap_pool_kernel, dim3(B), dim3(TAIL_THREADS), 0, s, x, ntok, C, gamma, beta, eps, pooled);
  return launch_clap_projection(pooled, B, C, J, w1, b1, relu, w2, b2, normalize, hid, emb, out, s);
}

hipError_t launch_clap_linear(const float *x, int64_t x_ld, int B, int K, int N, const float *w, const float *bias, int act, float *y, hipStream_t s) {
  if (B < 1 || K < 1 || K > LIN_MAXV * WAVE || N < 1 || x_ld < K) return hipErrorInvalidValue;
  hipLaunchKernelGGL(clap_linear_kernel, dim3((N + LIN_WAVES - 1) / LIN_WAVES), dim3(LIN_WAVES * WAVE), 0, s, x, x_ld, B, K, N, w, bias, act, y);
  return hipGetLastError();
}

hipError_t launch_clap_projection(const float *pooled, int B, int C, int J, const float *w1, const float *b1, int relu, const float *w2,
                                  const float *b2, int normalize, float *hid, float *emb, float *out, hipStream_t s) {
  if (B < 1 || C < 1 || C > TAIL_MAXC || J < 1 || J > TAIL_MAXJ) return hipErrorInvalidValue;
  hipError_t e = launch_clap_linear(pooled, C, B, C, J, w1, b1, relu ? CLAP_ACT_RELU : CLAP_ACT_NONE, hid, s);
  if (e != hipSuccess) return e;
  e = launch_clap_linear(hid, J, B, J, J, w2, b2, CLAP_ACT_NONE, emb, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(clap_l2norm_kernel, dim3(B), dim3(WAVE), 0, s, emb, J, normalize, out);
  return hipGetLastError();
}

}  // namespace sf
