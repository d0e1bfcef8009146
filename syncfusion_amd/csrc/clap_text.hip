// Device pieces of the CLAP text embedder (RoBERTa, post-LN) beside the implicit-GEMM launcher, fp32.
//
//   text_embed_kernel         ids -> LayerNorm(word[id] + position[p] + type[0]) with its affine, one wave per token row.  The position id is
//                             RoBERTa's pad-aware count: every lane tests one or two columns of the row (S <= 128) and the wave adds them up.
//   layernorm_affine_kernel   y = LN_C(x) gamma + beta, one wave per row, the row in the wave's registers, two-pass statistics.  RoBERTa is
//                             post-LN: the normalised rows feed the next Linear AND the next residual, so the affine cannot be folded into
//                             weights as the Swin path does; the residual add is the GEMM epilogue's.
//   masked_attention_kernel   one workgroup per (text, head), K and V of the head in LDS (2 S 64 floats, 64 KB at S = 128), four waves that
//                             take the query rows in turn.  Scores: a lane per key (two at S > 64), the query element broadcast from its
//                             lane; K rows are stored rotated by their row number (element d of row j at column (d + j) & 63), so the 32
//                             lanes of a half-wave read 32 different banks where a plain 64-float stride would put them on one.  PV: a lane
//                             per output dimension (head dim 64 = the wave), the weight of key j broadcast from its lane; V rows are read
//                             row-wise, one bank per lane.  Keys the mask leaves out are skipped by a wave-uniform branch on the ballot of
//                             the mask: their weight is exactly 0 and their K / V values (whatever they hold) never reach an accumulator.
//   the tail                  pooler / projection / L2 normalisation on the wave-per-output Linear of clap_front.hip.
// Every sum runs in a fixed order and no kernel looks beyond its own text: a text's rows do not depend on the rest of the batch.
#include "clap.h"
#include "common.h"

namespace sf {

namespace {

constexpr int ROW_WAVES = 4;                       // rows (waves) per workgroup of the two row kernels
constexpr int ROW_MAXV = TEXT_MAX_C / WAVE;        // values per lane
constexpr int ATT_WAVES = 4;

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// v[k] holds column k * 64 + lane of one row (C = 64 nv columns): normalise over C, apply the affine, store
__device__ __forceinline__ void ln_affine_store(float (&v)[ROW_MAXV], int nv, int lane, int C, const float *__restrict__ gamma,
                                                const float *__restrict__ beta, float eps, float *__restrict__ dst) {
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < ROW_MAXV; ++k)
    if (k < nv) sum += v[k];
  const float mean = wave_sum(sum) / (float)C;
  float dev = 0.f;
#pragma unroll
  for (int k = 0; k < ROW_MAXV; ++k)
    if (k < nv) {
      const float d = v[k] - mean;
      dev = fmaf(d, d, dev);
    }
  const float rstd = rsqrtf(wave_sum(dev) / (float)C + eps);
#pragma unroll
  for (int k = 0; k < ROW_MAXV; ++k)
    if (k < nv) {
      const int c = k * WAVE + lane;
      dst[c] = fmaf((v[k] - mean) * rstd, gamma[c], beta[c]);
    }
}

__global__ __launch_bounds__(ROW_WAVES *WAVE) void text_embed_kernel(const int32_t *__restrict__ ids, int64_t rows, int S, int C, int vocab, int n_pos,
                                                                     int pad_id, const float *__restrict__ word, const float *__restrict__ pos,
                                                                     const float *__restrict__ type, const float *__restrict__ gamma,
                                                                     const float *__restrict__ beta, float eps, float *__restrict__ out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t m = (int64_t)blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
  if (m >= rows) return;                               // (per wave: the reductions below stay whole)
  const int64_t b = m / S;
  const int col = (int)(m - b * S);
  const int32_t *row = ids + b * S;
  int real = 0;
  for (int j = lane; j <= col; j += WAVE) real += row[j] != pad_id;
  real = wave_sum_int(real);
  const int id = row[col];
  int p = id != pad_id ? pad_id + real : pad_id;
  p = min(max(p, 0), n_pos - 1);
  const float *wr = word + (int64_t)min(max(id, 0), vocab - 1) * C;
  const float *pr = pos + (int64_t)p * C;
  const int nv = C / WAVE;
  float v[ROW_MAXV];
#pragma unroll
  for (int k = 0; k < ROW_MAXV; ++k) {
    v[k] = 0.f;
    if (k < nv) {
      const int c = k * WAVE + lane;
      v[k] = wr[c] + type[c] + pr[c];
    }
  }
  ln_affine_store(v, nv, lane, C, gamma, beta, eps, out + m * C);
}

__global__ __launch_bounds__(ROW_WAVES *WAVE) void layernorm_affine_kernel(const float *__restrict__ x, int64_t rows, int C,
                                                                           const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                           float eps, float *__restrict__ y) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t m = (int64_t)blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
  if (m >= rows) return;
  const float *src = x + m * C;
  const int nv = C / WAVE;
  float v[ROW_MAXV];
#pragma unroll
  for (int k = 0; k < ROW_MAXV; ++k) {
    v[k] = 0.f;
    if (k < nv) v[k] = src[k * WAVE + lane];
  }
  ln_affine_store(v, nv, lane, C, gamma, beta, eps, y + m * C);
}

__global__ __launch_bounds__(ATT_WAVES *WAVE) void masked_attention_kernel(const float *__restrict__ qkv, const int32_t *__restrict__ mask, int S,
                                                                           int heads, float *__restrict__ out) {
  extern __shared__ float smem[];                      // K (S, 64), row j rotated by j | V (S, 64)
  constexpr int D = TEXT_HEAD_DIM;
  float *Ks = smem, *Vs = smem + S * D;
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const int C = heads * D;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
  const float *base = qkv + (int64_t)b * S * 3 * C + h * D;
  for (int i = threadIdx.x; i < S * D; i += blockDim.x) {
    const int j = i >> 6, d = i & (D - 1);
    const float *r = base + (int64_t)j * 3 * C;
    Ks[j * D + ((d + j) & (D - 1))] = r[C + d];
    Vs[i] = r[2 * C + d];
  }
  __syncthreads();
  // the two keys of this lane and whether the mask admits them
  const int j0 = lane, j1 = lane + WAVE;
  const bool ok0 = j0 < S && mask[(int64_t)b * S + j0] != 0;
  const bool ok1 = j1 < S && mask[(int64_t)b * S + j1] != 0;
  const unsigned long long m0 = __ballot(ok0), m1 = __ballot(ok1);
  const int r0 = min(j0, S - 1), r1 = min(j1, S - 1);   // (a lane without a key reads the last row and drops the result)
  const float *k0 = Ks + r0 * D, *k1 = Ks + r1 * D;
  const int n0 = min(S, WAVE), n1 = S - n0;
  for (int i = wave; i < S; i += ATT_WAVES) {
    float *dst = out + ((int64_t)b * S + i) * C + h * D;
    if ((m0 | m1) == 0ull) {                             // no key admitted: zeros (wave-uniform)
      dst[lane] = 0.f;
      continue;
    }
    const float q = base[(int64_t)i * 3 * C + lane] * 0.125f;   // 64^-1/2, exact
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const float qd = __shfl(q, d, WAVE);
      s0 = fmaf(qd, k0[(d + r0) & (D - 1)], s0);
      s1 = fmaf(qd, k1[(d + r1) & (D - 1)], s1);
    }
    const float neg = -__builtin_huge_valf();
    s0 = ok0 ? s0 : neg;                                 // a select: a masked key's score (NaN, for all we know) goes no further
    s1 = ok1 ? s1 : neg;
    const float mx = wave_max(fmaxf(s0, s1));
    const float p0 = ok0 ? expf(s0 - mx) : 0.f, p1 = ok1 ? expf(s1 - mx) : 0.f;
    const float denom = wave_sum(p0 + p1);
    float acc = 0.f;
    for (int j = 0; j < n0; ++j)
      if ((m0 >> j) & 1ull) acc = fmaf(__shfl(p0, j, WAVE), Vs[j * D + lane], acc);
    for (int j = 0; j < n1; ++j)
      if ((m1 >> j) & 1ull) acc = fmaf(__shfl(p1, j, WAVE), Vs[(WAVE + j) * D + lane], acc);
    dst[lane] = acc / denom;
  }
}

}  // namespace

hipError_t launch_text_embed(const int32_t *ids, int B, int S, int C, int vocab, int n_pos, int pad_id, const float *word, const float *pos,
                             const float *type, const float *gamma, const float *beta, float eps, float *out, hipStream_t s) {
  if (B < 1 || S < 1 || C < WAVE || C > TEXT_MAX_C || (C % WAVE) || vocab < 1 || n_pos < 1) return hipErrorInvalidValue;
  const int64_t rows = (int64_t)B * S;
  const int64_t grid = (rows + ROW_WAVES - 1) / ROW_WAVES;
  if (grid > 0x7FFFFFFFll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(text_embed_kernel, dim3((unsigned)grid), dim3(ROW_WAVES * WAVE), 0, s, ids, rows, S, C, vocab, n_pos, pad_id, word, pos, type,
                     gamma, beta, eps, out);
  return hipGetLastError();
}

hipError_t launch_layernorm_affine(const float *x, int64_t rows, int C, const float *gamma, const float *beta, float eps, float *y, hipStream_t s) {
  if (rows < 1 || C < WAVE || C > TEXT_MAX_C || (C % WAVE)) return hipErrorInvalidValue;
  const int64_t grid = (rows + ROW_WAVES - 1) / ROW_WAVES;
  if (grid > 0x7FFFFFFFll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(layernorm_affine_kernel, dim3((unsigned)grid), dim3(ROW_WAVES * WAVE), 0, s, x, rows, C, gamma, beta, eps, y);
  return hipGetLastError();
}

hipError_t launch_masked_attention(const float *qkv, const int32_t *mask, int B, int S, int heads, float *out, hipStream_t s) {
  if (B < 1 || S < 1 || S > TEXT_MAX_S || heads < 1 || (int64_t)B * heads > 0x7FFFFFFFll) return hipErrorInvalidValue;
  const size_t lds = (size_t)2 * S * TEXT_HEAD_DIM * sizeof(float);
  hipLaunchKernelGGL(masked_attention_kernel, dim3((unsigned)(B * heads)), dim3(ATT_WAVES * WAVE), lds, s, qkv, mask, S, heads, out);
  return hipGetLastError();
}

hipError_t launch_text_tail(const float *x, int B, int S, int C, int J, int pooler, const float *pool_w, const float *pool_b, const float *w1,
                            const float *b1, int relu, const float *w2, const float *b2, int normalize, float *scratch, float *out, hipStream_t s) {
  if (B < 1 || S < 1 || C < 1 || C > TEXT_MAX_C || J < 1 || J > 1024 || !scratch) return hipErrorInvalidValue;
  float *pooled = scratch, *hid = pooled + (int64_t)B * C, *emb = hid + (int64_t)B * J;
  hipError_t e;
  if (pooler)
    e = launch_clap_linear(x, (int64_t)S * C, B, C, C, pool_w, pool_b, CLAP_ACT_TANH, pooled, s);
  else
    e = hipMemcpy2DAsync(pooled, (size_t)C * 4, x, (size_t)S * C * 4, (size_t)C * 4, (size_t)B, hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return e;
  return launch_clap_projection(pooled, B, C, J, w1, b1, relu, w2, b2, normalize, hid, emb, out, s);
}

}  // namespace sf
