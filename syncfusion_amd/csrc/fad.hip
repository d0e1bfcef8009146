// FAD evaluation (replaces the frechet_audio_distance package behind main/evaluation.py:7-28): what the VGGish network needs beside the
// implicit-GEMM convolution, and the statistics of its embeddings.
//
//   maxpool2x2_cl_kernel  channels-last 2x2 / stride 2 max-pool, one thread per output vector of 4 columns (or per element when the row
//                         length is not a multiple of 4)
//   pack_fc_kernel        Linear weight with (position, channel) columns -> rows of padded channel groups, as the pooled rows lie
//   moments_sum_kernel    column sums of the (N, D) embeddings in fp64: 8 row groups per column, added in group order
//   moments_scatter_kernel one workgroup per row i of the centred scatter matrix: sum_r (x[r][i] - mean_i)(x[r][j] - mean_j) in fp64, the same
//                         8 row groups.  Two passes about the mean; no atomics, so identical input gives identical bits.
#include "fad.h"

namespace sf {

namespace {

constexpr int MOM_D = 128;     // columns at most
constexpr int MOM_G = 8;       // row groups per workgroup

template <typename V> __device__ __forceinline__ V vmax(V a, V b);
template <> __device__ __forceinline__ float vmax<float>(float a, float b) { return fmaxf(a, b); }
template <> __device__ __forceinline__ float4 vmax<float4>(float4 a, float4 b) {
  return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}

// ldv: row length in units of V
template <typename V> __global__ void maxpool2x2_cl_kernel(const V *__restrict__ x, int64_t n, int H, int W, int ldv, V *__restrict__ y) {
  const int Ho = H >> 1, Wo = W >> 1;
  const int64_t total = n * Ho * Wo * ldv;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % ldv);
    int64_t r = i / ldv;
    const int wo = (int)(r % Wo);
    r /= Wo;
    const int ho = (int)(r % Ho);
    const int64_t b = r / Ho;
    const V *p = x + ((b * H + 2 * ho) * W + 2 * wo) * ldv + c;     // 2 ho + 1 < H and 2 wo + 1 < W by the floor division
    y[i] = vmax<V>(vmax<V>(p[0], p[ldv]), vmax<V>(p[(int64_t)W * ldv], p[(int64_t)(W + 1) * ldv]));
  }
}

__global__ void pack_fc_kernel(const float *__restrict__ w, int N, int P, int C, int ld, int K, float *__restrict__ out) {
  const int64_t total = (int64_t)N * K;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % K);
    const int64_t nn = i / K;
    const int p = k / ld, c = k - p * ld;
    out[i] = (p < P && c < C) ? w[(nn * P + p) * C + c] : 0.f;
  }
}

__global__ __launch_bounds__(MOM_D *MOM_G) void moments_sum_kernel(const float *__restrict__ x, int64_t N, int D, double *__restrict__ sum) {
  __shared__ double part[MOM_G][MOM_D];
  const int d = threadIdx.x % MOM_D, g = threadIdx.x / MOM_D;
  double acc = 0.0;
  if (d < D)
    for (int64_t r = g; r < N; r += MOM_G) acc += (double)x[r * D + d];
  part[g][d] = acc;
  __syncthreads();
  if (g == 0 && d < D) {
    double t = part[0][d];
    for (int k = 1; k < MOM_G; ++k) t += part[k][d];
    sum[d] = t;
  }
}

__global__ __launch_bounds__(MOM_D *MOM_G) void moments_scatter_kernel(const float *__restrict__ x, int64_t N, int D, const double *__restrict__ sum,
                                                                       double *__restrict__ scatter) {
  __shared__ double part[MOM_G][MOM_D];
  const int i = blockIdx.x, j = threadIdx.x % MOM_D, g = threadIdx.x / MOM_D;
  double acc = 0.0;
  if (j < D) {
    const double mi = sum[i] / (double)N, mj = sum[j] / (double)N;
    for (int64_t r = g; r < N; r += MOM_G) acc += ((double)x[r * D + i] - mi) * ((double)x[r * D + j] - mj);
  }
  part[g][j] = acc;
  __syncthreads();
  if (g == 0 && j < D) {
    double t = part[0][j];
    for (int k = 1; k < MOM_G; ++k) t += part[k][j];
    scatter[(int64_t)i * D + j] = t;
  }
}

unsigned grid_for(int64_t total) { return (unsigned)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535); }

}  // namespace

hipError_t launch_maxpool2x2_cl(const float *x, int64_t n, int H, int W, int ld, float *y, hipStream_t s) {
  if (n < 1 || H < 2 || W < 2 || ld < 1) return hipErrorInvalidValue;
  const int64_t total = n * (H / 2) * (W / 2) * ld;
  const bool vec = (ld % 4) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(maxpool2x2_cl_kernel<float4>, dim3(grid_for(total / 4)), dim3(256), 0, s, reinterpret_cast<const float4 *>(x), n, H, W, ld / 4,
                       reinterpret_cast<float4 *>(y));
  else
    hipLaunchKernelGGL(maxpool2x2_cl_kernel<float>, dim3(grid_for(total)), dim3(256), 0, s, x, n, H, W, ld, y);
  return hipGetLastError();
}

hipError_t launch_pack_fc(const float *w, int N, int P, int C, int ld, int K, float *out, hipStream_t s) {
  if (N < 1 || P < 1 || C < 1 || ld < C || K < P * ld) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pack_fc_kernel, dim3(grid_for((int64_t)N * K)), dim3(256), 0, s, w, N, P, C, ld, K, out);
  return hipGetLastError();
}

hipError_t launch_moments(const float *x, int64_t N, int D, double *sum, double *scatter, hipStream_t s) {
  if (N < 1 || D < 1 || D > MOM_D) return hipErrorInvalidValue;
  hipLaunchKernelGGL(moments_sum_kernel, dim3(1), dim3(MOM_D * MOM_G), 0, s, x, N, D, sum);
  hipLaunchKernelGGL(moments_scatter_kernel, dim3(D), dim3(MOM_D * MOM_G), 0, s, x, N, D, sum, scatter);
  return hipGetLastError();
}

}  // namespace sf
