// Inpainting sampler kernels: counter-based device noise (Philox4x32-10 + Box-Muller) and the fused VInpainter update
// (v-sampler step + re-noised source blend); the linear multistep update of sf_vsample_ms.  HBM-bound streaming, one Philox group (four
// consecutive elements) per thread.
#include "common.h"
#include "kernels.h"

namespace sf {
namespace {

constexpr int TPB = 256;
inline dim3 grid_for(int64_t n) {
  int64_t b = (n + TPB - 1) / TPB;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

// Philox4x32-10 (Salmon et al., SC'11): ten rounds of two 32x32 -> 64 multiplies, the key bumped by the Weyl constants between rounds
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t r[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0;
    c1 = lo1;
    c2 = n2;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r[0] = c0;
  r[1] = c1;
  r[2] = c2;
  r[3] = c3;
}

// 32 random bits -> u in [2^-24, 1 - 2^-24]: ((w >> 9) + 0.5) * 2^-23, exact in fp32 (24 significant bits), never 0 or 1
__device__ __forceinline__ float unit_open(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-7f; }

// Box-Muller pair: rho = sqrt(-2 ln u0), (rho cos 2 pi u1, rho sin 2 pi u1).  sincospif takes 2 * u1 (exact), so the angle carries no
// rounding of its own.
__device__ __forceinline__ void box_muller(uint32_t w0, uint32_t w1, float &z0, float &z1) {
  const float rho = sqrtf(-2.0f * logf(unit_open(w0)));
  float sn, cs;
  sincospif(2.0f * unit_open(w1), &sn, &cs);
  z0 = rho * cs;
  z1 = rho * sn;
}

// the four normals of Philox group g at virtual iteration k: counter (g lo, g hi, k, 0), key (seed lo, seed hi)
__device__ __forceinline__ void normal4(int64_t g, uint32_t k, uint32_t seed_lo, uint32_t seed_hi, float z[4]) {
  uint32_t r[4];
  philox4x32_10((uint32_t)((uint64_t)g & 0xffffffffu), (uint32_t)((uint64_t)g >> 32), k, 0u, seed_lo, seed_hi, r);
  box_muller(r[0], r[1], z[0], z[1]);
  box_muller(r[2], r[3], z[2], z[3]);
}

// out[i] = normal of element (e0 + i), i in [0, n)
__global__ void philox_normal_kernel(uint32_t seed_lo, uint32_t seed_hi, uint32_t k, int64_t e0, int64_t n, float *__restrict__ out) {
  const int64_t e1 = e0 + n, g_lo = e0 >> 2, ng = ((e1 + 3) >> 2) - g_lo;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < ng; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = g_lo + t;
    float z[4];
    normal4(g, k, seed_lo, seed_hi, z);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int64_t e = 4 * g + l;
      if (e >= e0 && e < e1) out[e - e0] = z[l];
    }
  }
}

// The v-sampler step of one element with the roundings vsampler_update_kernel (misc.hip) compiles to, spelled out -- left to the compiler,
// the same expressions contract differently inside the 16-byte path below, and R = 1 with an empty mask must be sample() bit for bit
// (tests/test_gpu_inpaint.py holds the two kernels together):
//   x_pred = fma(a0, x, -(b0 * v)),  n_pred = fma(b0, x, a0 * v),  out = (a1 * x_pred) + (b1 * n_pred);  guidance: fma(v_c - v_u, scale, v_u)
__device__ __forceinline__ float vstep(float xx, float vv, float a0, float b0, float a1, float b1) {
#pragma clang fp contract(off)
  const float x_pred = __builtin_fmaf(a0, xx, -(b0 * vv));
  const float n_pred = __builtin_fmaf(b0, xx, a0 * vv);
  const float p = a1 * x_pred, q = b1 * n_pred;
  return p + q;
}
__device__ __forceinline__ float guide(float vc, float m, float scale) {
#pragma clang fp contract(off)
  const float d = vc - m;
  return __builtin_fmaf(d, scale, m);
}
// the kept source at the iteration's target level
__device__ __forceinline__ float renoise(float src, float z, float a1, float b1) {
#pragma clang fp contract(off)
  const float p = a1 * src, q = b1 * z;
  return p + q;
}

// VInpainter iteration, in place on x, for the elements [e0, e1) of the whole (B, C, L) tensor (every pointer is the base of the WHOLE
// tensor: a clip-parallel branch passes its slice as the range, so the generator sees the global element index whatever the split):
//   x <- mask ? a1 * source + b1 * z : vstep(x, v)      z = normal(seed, k, element),  k = *step_idx + step_bias
// Nothing that changes between calls is an argument: the seed and the iteration are read from device memory (graph replay).
// A thread takes one Philox group; groups that lie wholly inside the range go through 16-byte accesses (vec: all bases 16-byte aligned),
// the at most two partial groups at the ends of the range element by element.  Groups with no kept element skip the generator.
__global__ void vinpaint_update_kernel(float *__restrict__ x, const float *__restrict__ v, const float *__restrict__ vu, float scale,
                                       const float *__restrict__ src, const uint8_t *__restrict__ mask, const float *__restrict__ sched,
                                       const int *__restrict__ step_idx, int step_bias, const uint32_t *__restrict__ seed, int64_t e0, int64_t e1,
                                       int vec) {
  const int k = *step_idx + step_bias;
  const float *sc = sched + 4 * k;
  const float a0 = sc[0], b0 = sc[1], a1 = sc[2], b1 = sc[3];
  const uint32_t seed_lo = seed[0], seed_hi = seed[1];
  const int64_t g_lo = e0 >> 2, ng = ((e1 + 3) >> 2) - g_lo;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < ng; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = g_lo + t, e = 4 * g;
    if (vec && e >= e0 && e + 4 <= e1) {
      const float4 xx = *reinterpret_cast<const float4 *>(x + e);
      float4 vv = *reinterpret_cast<const float4 *>(v + e);
      if (vu) {
        const float4 m = *reinterpret_cast<const float4 *>(vu + e);
        vv.x = guide(vv.x, m.x, scale);
        vv.y = guide(vv.y, m.y, scale);
        vv.z = guide(vv.z, m.z, scale);
        vv.w = guide(vv.w, m.w, scale);
      }
      const uchar4 mk = *reinterpret_cast<const uchar4 *>(mask + e);
      float4 o;
      o.x = vstep(xx.x, vv.x, a0, b0, a1, b1);
      o.y = vstep(xx.y, vv.y, a0, b0, a1, b1);
      o.z = vstep(xx.z, vv.z, a0, b0, a1, b1);
      o.w = vstep(xx.w, vv.w, a0, b0, a1, b1);
      if (mk.x | mk.y | mk.z | mk.w) {
        const float4 ss = *reinterpret_cast<const float4 *>(src + e);
        float z[4];
        normal4(g, (uint32_t)k, seed_lo, seed_hi, z);
        if (mk.x) o.x = renoise(ss.x, z[0], a1, b1);
        if (mk.y) o.y = renoise(ss.y, z[1], a1, b1);
        if (mk.z) o.z = renoise(ss.z, z[2], a1, b1);
        if (mk.w) o.w = renoise(ss.w, z[3], a1, b1);
      }
      *reinterpret_cast<float4 *>(x + e) = o;
    } else {
      float z[4];
      bool have = false;
      for (int l = 0; l < 4; ++l) {
        const int64_t i = e + l;
        if (i < e0 || i >= e1) continue;
        float o;
        if (mask[i]) {
          if (!have) {
            normal4(g, (uint32_t)k, seed_lo, seed_hi, z);
            have = true;
          }
          o = renoise(src[i], z[l], a1, b1);
        } else {
          float vv = v[i];
          if (vu) {
            const float m = vu[i];
            vv = guide(vv, m, scale);
          }
          o = vstep(x[i], vv, a0, b0, a1, b1);
        }
        x[i] = o;
      }
    }
  }
}

// One element of the multistep update with its roundings spelled out (the 16-byte path and the element-wise ends must agree bit for bit):
//   X = fma(al, x, -(be * v)),  x <- fma(c1, hist, fma(c0, X, cx * x)),  hist <- X
__device__ __forceinline__ float ms_x0(float xx, float vv, float al, float be) {
#pragma clang fp contract(off)
  return __builtin_fmaf(al, xx, -(be * vv));
}
__device__ __forceinline__ float ms_next(float xx, float X, float hh, float cx, float c0, float c1) {
#pragma clang fp contract(off)
  const float p = cx * xx;
  return __builtin_fmaf(c1, hh, __builtin_fmaf(c0, X, p));
}

// Linear multistep step of the v-sampler ("Multistep sampler"), in place on x and on the history, for the elements [e0, e1) of the
// whole tensor (range convention of vinpaint_update_kernel: every pointer is the base of the WHOLE tensor, a branch passes its slice as the range):
//   X = al * x - be * v,   x <- cx * x + c0 * X + c1 * hist,   hist <- X,    (al, be, cx, c0, c1) = table[8 k .. 8 k + 4],  k = *step_idx + step_bias
// The row is 8 floats (three unused) at a 32-byte aligned address that is the same for every lane: one scalar load.  Nothing that changes
// between calls is an argument (graph replay): the coefficients are read from device memory.
__global__ void vsampler_update_ms_kernel(float *__restrict__ x, const float *__restrict__ v, const float *__restrict__ vu, float scale,
                                          float *__restrict__ hist, const float *__restrict__ table, const int *__restrict__ step_idx, int step_bias,
                                          int64_t e0, int64_t e1, int vec) {
  const int k = *step_idx + step_bias;
  const float *row = table + 8 * (int64_t)k;
  const float al = row[0], be = row[1], cx = row[2], c0 = row[3], c1 = row[4];
  const int64_t g_lo = e0 >> 2, ng = ((e1 + 3) >> 2) - g_lo;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < ng; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = 4 * (g_lo + t);
    if (vec && e >= e0 && e + 4 <= e1) {
      const float4 xx = *reinterpret_cast<const float4 *>(x + e);
      const float4 hh = *reinterpret_cast<const float4 *>(hist + e);
      float4 vv = *reinterpret_cast<const float4 *>(v + e);
      if (vu) {
        const float4 m = *reinterpret_cast<const float4 *>(vu + e);
        vv.x = guide(vv.x, m.x, scale);
        vv.y = guide(vv.y, m.y, scale);
        vv.z = guide(vv.z, m.z, scale);
        vv.w = guide(vv.w, m.w, scale);
      }
      float4 X, o;
      X.x = ms_x0(xx.x, vv.x, al, be);
      X.y = ms_x0(xx.y, vv.y, al, be);
      X.z = ms_x0(xx.z, vv.z, al, be);
      X.w = ms_x0(xx.w, vv.w, al, be);
      o.x = ms_next(xx.x, X.x, hh.x, cx, c0, c1);
      o.y = ms_next(xx.y, X.y, hh.y, cx, c0, c1);
      o.z = ms_next(xx.z, X.z, hh.z, cx, c0, c1);
      o.w = ms_next(xx.w, X.w, hh.w, cx, c0, c1);
      *reinterpret_cast<float4 *>(x + e) = o;
      *reinterpret_cast<float4 *>(hist + e) = X;
    } else {
      for (int l = 0; l < 4; ++l) {
        const int64_t i = e + l;
        if (i < e0 || i >= e1) continue;
        float vv = v[i];
        if (vu) {
          const float m = vu[i];
          vv = guide(vv, m, scale);
        }
        const float xx = x[i];
        const float X = ms_x0(xx, vv, al, be);
        x[i] = ms_next(xx, X, hist[i], cx, c0, c1);
        hist[i] = X;
      }
    }
  }
}

}  // namespace

hipError_t launch_vsampler_update_ms(float *x, const float *v, const float *v_uncond, float scale, float *hist, const float *table,
                                     const int *step_idx, int step_bias, int64_t e0, int64_t e1, hipStream_t s) {
  if (e1 <= e0) return hipSuccess;
  auto al16 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const int vec = al16(x) && al16(v) && (!v_uncond || al16(v_uncond)) && al16(hist);
  hipLaunchKernelGGL(vsampler_update_ms_kernel, grid_for((e1 - e0 + 3) / 4 + 1), dim3(TPB), 0, s, x, v, v_uncond, scale, hist, table, step_idx,
                     step_bias, e0, e1, vec);
  return hipGetLastError();
}

hipError_t launch_philox_normal(uint64_t seed, uint32_t k, int64_t elem_offset, int64_t n, float *out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(philox_normal_kernel, grid_for((n + 3) / 4 + 1), dim3(TPB), 0, s, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), k,
                     elem_offset, n, out);
  return hipGetLastError();
}

hipError_t launch_vinpaint_update(float *x, const float *v, const float *v_uncond, float scale, const float *source, const uint8_t *mask,
                                  const float *sched, const int *step_idx, int step_bias, const uint32_t *seed, int64_t e0, int64_t e1,
                                  hipStream_t s) {
  if (e1 <= e0) return hipSuccess;
  auto al16 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const int vec = al16(x) && al16(v) && (!v_uncond || al16(v_uncond)) && al16(source) && (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
  hipLaunchKernelGGL(vinpaint_update_kernel, grid_for((e1 - e0 + 3) / 4 + 1), dim3(TPB), 0, s, x, v, v_uncond, scale, source, mask, sched, step_idx,
                     step_bias, seed, e0, e1, vec);
  return hipGetLastError();
}

}  // namespace sf
