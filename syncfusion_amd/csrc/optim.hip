// The optimizer stage of a training step (exp/train_diffusion_gh.yaml:84-96: gradient_clip_val 0.5 by global norm, then AdamW as
// main/module_diffusion.py:53-62 configures it) as three launches over ONE device-resident descriptor table: no per-tensor launch
// sequence, no scaling pass over the gradients, nothing that changes per step in a kernel argument (so a captured graph replays it).
//
//   table   n_tensors records of OPTIM_DESC_WORDS 64-bit words, sorted by first_chunk:
//             [0] p  [1] g  [2] exp_avg  [3] exp_avg_sq  [4] step (fp32 device scalar)  [5] element count
//             [6] hyper-parameter group | first_chunk << 32                             [7] unused
//   chunks  a tensor of n elements is cut into ceil(n / OPTIM_CHUNK) chunks of OPTIM_CHUNK = 16384 elements (64 KB per stream); one
//           workgroup of 256 lanes owns one chunk (16 sixteen-byte accesses per lane and stream) and finds its tensor by a binary search
//           of the first_chunk column.  No chunk spans two tensors.
//   hyper   fp64 device array: [0] max_norm, then per group g at 8 + 8 g: lr, beta1, beta2, eps, weight_decay
//   ws      [0] clip_coef (fp64) | 256: (1 - beta1^step, sqrt(1 - beta2^step)) fp64 per tensor | then one fp32 sum of squares per chunk
//
// Arithmetic of the update: the multiply-adds of the recurrence run in fp64 on the fp32 operands (v_fma_f64 is full rate on this part and
// the kernel is bound by its 28 bytes per element), so p, exp_avg and exp_avg_sq each round ONCE per step; sqrt and the division of the
// update term run in fp32 (their error is scaled by lr before it meets p).
#include "common.h"

namespace sf {

namespace {

typedef unsigned long long u64;
// the table holds addresses as integers: tell the compiler they are global memory (global_load / global_store, not flat accesses)
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
typedef __attribute__((address_space(1))) const float cgf32;
typedef __attribute__((address_space(1))) const f32x4 cgf32x4;

constexpr int OPTIM_DESC_WORDS = 8;
constexpr int OPTIM_HYPER_STRIDE = 8;
constexpr int OPTIM_THREADS = 256;

// the last record whose first_chunk <= blk (uniform over the workgroup: scalar loads)
__device__ __forceinline__ int optim_find(const u64 *__restrict__ desc, int n_tensors, unsigned blk) {
  int lo = 0, hi = n_tensors - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((unsigned)(desc[(size_t)mid * OPTIM_DESC_WORDS + 6] >> 32) <= blk) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// elements in front of the first 16-byte boundary of `ptr` (fp32 elements), at most len
__device__ __forceinline__ int optim_head(cgf32 *ptr, int len) {
  const int h = (int)((4u - (unsigned)(((uintptr_t)ptr >> 2) & 3u)) & 3u);
  return h < len ? h : len;
}

// partial[chunk] = sum of g^2 over the chunk, fp32.  Per lane: four accumulators over <= 16 float4 (depth 16), combined pairwise (+2), the
// scalar head / tail elements (+2); then a 64-lane butterfly (6 levels) and the 4 waves pairwise through LDS (2 levels).  Fixed order,
// no atomics: the same bits on every run.
__global__ __launch_bounds__(OPTIM_THREADS) void optim_sumsq_kernel(const u64 *__restrict__ desc, int n_tensors, float *__restrict__ partial) {
  __shared__ float red[OPTIM_THREADS / WAVE];
  const unsigned blk = blockIdx.x;
  const u64 *d = desc + (size_t)optim_find(desc, n_tensors, blk) * OPTIM_DESC_WORDS;
  const int64_t n = (int64_t)d[5];
  const int64_t off = (int64_t)(blk - (unsigned)(d[6] >> 32)) * OPTIM_CHUNK;
  const int tid = threadIdx.x;
  float a = 0.f;
  if (off < n) {   // (a table whose chunk count overstates a tensor leaves the surplus workgroups without work)
    const int len = (int)(n - off < OPTIM_CHUNK ? n - off : OPTIM_CHUNK);
    cgf32 *g = (cgf32 *)d[1] + off;
    const int head = optim_head(g, len), body4 = (len - head) >> 2, tail = len - head - 4 * body4;
    cgf32x4 *g4 = (cgf32x4 *)(g + head);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int i = tid; i < body4; i += OPTIM_THREADS) {
      const f32x4 x = g4[i];
      a0 = fmaf(x[0], x[0], a0);
      a1 = fmaf(x[1], x[1], a1);
      a2 = fmaf(x[2], x[2], a2);
      a3 = fmaf(x[3], x[3], a3);
    }
    a = (a0 + a1) + (a2 + a3);
    if (tid < head) a = fmaf(g[tid], g[tid], a);
    if (tid < tail) {
      const float x = g[head + 4 * body4 + tid];
      a = fmaf(x, x, a);
    }
  }
  a = wave_sum(a);
  if ((tid & (WAVE - 1)) == 0) red[tid / WAVE] = a;
  __syncthreads();
  if (tid == 0) partial[blk] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup: the chunk partials summed in a fixed order in fp64 -> total_norm, clip_coef (torch.nn.utils.clip_grad_norm_'s formula;
// a NaN norm gives a NaN coefficient, as there); every listed step += 1 and the two bias-correction terms of the NEW step per tensor.
__global__ __launch_bounds__(OPTIM_THREADS) void optim_prepare_kernel(const u64 *__restrict__ desc, int n_tensors, int total_chunks,
                                                                      const double *__restrict__ hyper, int n_groups, int clip,
                                                                      const float *__restrict__ partial, double *__restrict__ coef_out,
                                                                      double *__restrict__ bc, float *__restrict__ result) {
  __shared__ double red[OPTIM_THREADS];
  const int tid = threadIdx.x;
  if (clip) {
    double s = 0.0;
    for (int i = tid; i < total_chunks; i += OPTIM_THREADS) s += (double)partial[i];
    red[tid] = s;
    __syncthreads();
    for (int o = OPTIM_THREADS / 2; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) {
      const double norm = sqrt(red[0]);
      const double c = hyper[0] / (norm + 1e-6);
      const double coef = c > 1.0 ? 1.0 : c;   // (not fmin: a NaN stays a NaN)
      result[0] = (float)norm;
      result[1] = (float)coef;
      *coef_out = coef;
    }
  } else if (tid == 0) {
    result[1] = 1.f;
    *coef_out = 1.0;
  }
  for (int t = tid; t < n_tensors; t += OPTIM_THREADS) {
    const u64 *d = desc + (size_t)t * OPTIM_DESC_WORDS;
    gf32 *step = (gf32 *)d[4];
    const float s = *step + 1.f;
    *step = s;
    int grp = (int)(d[6] & 0xffffffffu);
    grp = grp < n_groups ? grp : n_groups - 1;
    const double *h = hyper + OPTIM_HYPER_STRIDE * (1 + grp);
    bc[2 * t] = 1.0 - pow(h[1], (double)s);
    bc[2 * t + 1] = sqrt(1.0 - pow(h[2], (double)s));
  }
}

struct AdamConst {
  double coef, lr_wd, omb1, beta2, omb2, step_size;
  float bc2_sqrt, eps;
};

// torch's order of operations for AdamW (decoupled weight decay, amsgrad = False, maximize = False) on one element
__device__ __forceinline__ void adamw_element(const AdamConst &k, float &p, float g, float &m, float &v) {
  const double gd = (double)g * k.coef;
  double pd = (double)p;
  pd -= k.lr_wd * pd;
  const double md = (double)m + k.omb1 * (gd - (double)m);
  const double vd = k.beta2 * (double)v + k.omb2 * gd * gd;
  m = (float)md;
  v = (float)vd;
  const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
  pd -= k.step_size * (double)(m / denom);
  p = (float)pd;
}

__global__ __launch_bounds__(OPTIM_THREADS) void optim_adamw_kernel(const u64 *__restrict__ desc, int n_tensors, const double *__restrict__ hyper,
                                                                    int n_groups, const double *__restrict__ coef_in,
                                                                    const double *__restrict__ bc) {
  const unsigned blk = blockIdx.x;
  const int t = optim_find(desc, n_tensors, blk);
  const u64 *d = desc + (size_t)t * OPTIM_DESC_WORDS;
  const int64_t n = (int64_t)d[5];
  const int64_t off = (int64_t)(blk - (unsigned)(d[6] >> 32)) * OPTIM_CHUNK;
  if (off >= n) return;
  const int len = (int)(n - off < OPTIM_CHUNK ? n - off : OPTIM_CHUNK);
  int grp = (int)(d[6] & 0xffffffffu);
  grp = grp < n_groups ? grp : n_groups - 1;
  const double *h = hyper + OPTIM_HYPER_STRIDE * (1 + grp);
  const double lr = h[0], beta1 = h[1], beta2 = h[2];
  AdamConst k;
  k.coef = *coef_in;
  k.lr_wd = lr * h[4];
  k.omb1 = 1.0 - beta1;
  k.beta2 = beta2;
  k.omb2 = 1.0 - beta2;
  k.step_size = lr / bc[2 * t];
  k.bc2_sqrt = (float)bc[2 * t + 1];
  k.eps = (float)h[3];
  gf32 *p = (gf32 *)d[0] + off;
  cgf32 *g = (cgf32 *)d[1] + off;
  gf32 *m = (gf32 *)d[2] + off;
  gf32 *v = (gf32 *)d[3] + off;
  const int tid = threadIdx.x;
  // 16-byte accesses need the four streams at the same offset from a 16-byte boundary (a parameter that is a view at an odd offset has
  // freshly allocated, aligned, gradient and moments: then the chunk runs element by element)
  const unsigned ap = (unsigned)((uintptr_t)p & 15u);
  const bool same = ap == (unsigned)((uintptr_t)g & 15u) && ap == (unsigned)((uintptr_t)m & 15u) && ap == (unsigned)((uintptr_t)v & 15u);
  const int head = same ? optim_head(p, len) : len;
  const int body4 = (len - head) >> 2, tail0 = head + 4 * body4;
  gf32x4 *p4 = (gf32x4 *)(p + head);
  cgf32x4 *g4 = (cgf32x4 *)(g + head);
  gf32x4 *m4 = (gf32x4 *)(m + head);
  gf32x4 *v4 = (gf32x4 *)(v + head);
  for (int i = tid; i < body4; i += OPTIM_THREADS) {
    f32x4 pp = p4[i], mm = m4[i], vv = v4[i];
    const f32x4 gg = g4[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pj = pp[j], mj = mm[j], vj = vv[j];
      adamw_element(k, pj, gg[j], mj, vj);
      pp[j] = pj;
      mm[j] = mj;
      vv[j] = vj;
    }
    p4[i] = pp;
    m4[i] = mm;
    v4[i] = vv;
  }
  for (int i = tid; i < len - 4 * body4; i += OPTIM_THREADS) {   // the elements in front of and behind the 16-byte body
    const int e = i < head ? i : tail0 + (i - head);
    float pe = p[e], me = m[e], ve = v[e];
    adamw_element(k, pe, g[e], me, ve);
    p[e] = pe;
    m[e] = me;
    v[e] = ve;
  }
}

}  // namespace

int64_t optim_ws_bytes(int64_t total_chunks) { return 256 + total_chunks * (int64_t)(2 * sizeof(double) + sizeof(float)); }

hipError_t launch_optim_adamw_step(const void *desc_dev, int n_tensors, int total_chunks, const double *hyper_dev, int n_groups, int clip,
                                   float *result_dev, void *ws, hipStream_t s) {
  if (!desc_dev || !hyper_dev || !result_dev || !ws || n_tensors < 1 || total_chunks < n_tensors || n_groups < 1) return hipErrorInvalidValue;
  const u64 *desc = static_cast<const u64 *>(desc_dev);
  double *coef = static_cast<double *>(ws);
  double *bc = reinterpret_cast<double *>(static_cast<char *>(ws) + 256);
  float *partial = reinterpret_cast<float *>(bc + 2 * (int64_t)total_chunks);
  if (clip) {
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3((unsigned)total_chunks), dim3(OPTIM_THREADS), 0, s, desc, n_tensors, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(optim_prepare_kernel, dim3(1), dim3(OPTIM_THREADS), 0, s, desc, n_tensors, total_chunks, hyper_dev, n_groups, clip, partial, coef, bc,
                     result_dev);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(optim_adamw_kernel, dim3((unsigned)total_chunks), dim3(OPTIM_THREADS), 0, s, desc, n_tensors, hyper_dev, n_groups, coef, bc);
  return hipGetLastError();
}

}  // namespace sf
