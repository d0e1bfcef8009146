// Inpainting sampler kernels: counter-based device noise (Philox4x32-10 + Box-Muller) and the fused VInpainter update
// (v-sampler step + re-noised source blend); the linear multistep update of sf_vsample_ms; the per-clip statistics and the guided update of
// sf_vsample_gx (guidance schedules).  HBM-bound streaming, one Philox group (four consecutive elements) per thread.
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

// ---------------------------------------------------------------------------------------------------
// Guidance schedules ("Guidance schedules"): the scale of clip b at step k is gtab[k * B + b]; an optional per-clip rescale of the
// guided direction to the level of v_c (Lin et al. 2023, section 3.4).
// ---------------------------------------------------------------------------------------------------
// the guided direction of one element: v_c itself where the scale is exactly 1 (or there is no unconditional half), else guide()
__device__ __forceinline__ float guide_s(float vc, const float *__restrict__ vu, int64_t i, float sc) {
  if (!vu || sc == 1.0f) return vc;
  return guide(vc, vu[i], sc);
}
__device__ __forceinline__ float rescaled(float g, float fac) {
#pragma clang fp contract(off)
  return g * fac;
}

constexpr int kStatsPart = 6;   // doubles per partial: count, mean(v_c), M2(v_c), mean(g), M2(g), unused

// sum of the TPB per-thread values in a fixed order (LDS tree); every thread gets the result
__device__ __forceinline__ double block_sum(double val, double *sh) {
  __syncthreads();
  sh[threadIdx.x] = val;
  __syncthreads();
  for (int w = TPB / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  return sh[0];
}

// Statistics of v_c and of the guided direction g over one clip, for the rescale: grid (blocks per clip, B).  A block takes a contiguous share of
// its clip and leaves (count, mean, M2) of both in fp64 -- two passes over its share (the mean first, then the squared deviations from it, with
// the first-order correction), the second one from cache -- in part[(b * gridDim.x + block) * kStatsPart ..].  No atomics, a fixed order of
// additions: a replay gives the same bits, and so does a launch from pointers with another alignment (a thread adds the same elements in
// the same order on the 16-byte path and element by element).  v, vu: bases of the WHOLE (B, C, L) tensors; vu may be null (g = v_c).
__global__ void guidance_stats_kernel(const float *__restrict__ v, const float *__restrict__ vu, const float *__restrict__ gtab,
                                      const int *__restrict__ step_idx, int step_bias, int B, int64_t clip_len, double *__restrict__ part, int vec) {
  __shared__ double sh[TPB];
  const int b = blockIdx.y, nb = gridDim.x;
  const int k = *step_idx + step_bias;
  const float sc = gtab[(int64_t)k * B + b];
  const int64_t per = (clip_len + nb - 1) / nb;
  const int64_t base = (int64_t)b * clip_len;
  int64_t lo = base + (int64_t)blockIdx.x * per, hi = lo + per;
  if (hi > base + clip_len) hi = base + clip_len;
  if (lo > hi) lo = hi;
  const int64_t g_lo = lo >> 2, ng = hi > lo ? ((hi + 3) >> 2) - g_lo : 0;
  double mc = 0.0, mg = 0.0, m2c = 0.0, m2g = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    double a_c = 0.0, a_g = 0.0, q_c = 0.0, q_g = 0.0;
    auto add = [&](float c, float g) {   // one element, in the element order of the thread's groups on either path
      if (pass == 0) {
        a_c += (double)c;
        a_g += (double)g;
      } else {
        const double dc = (double)c - mc, dg = (double)g - mg;
        a_c += dc;
        a_g += dg;
        q_c += dc * dc;
        q_g += dg * dg;
      }
    };
    for (int64_t t = threadIdx.x; t < ng; t += TPB) {
      const int64_t e = 4 * (g_lo + t);
      if (vec && e >= lo && e + 4 <= hi) {
        const float4 vv = *reinterpret_cast<const float4 *>(v + e);
        if (vu && sc != 1.0f) {
          const float4 m = *reinterpret_cast<const float4 *>(vu + e);
          add(vv.x, guide(vv.x, m.x, sc));
          add(vv.y, guide(vv.y, m.y, sc));
          add(vv.z, guide(vv.z, m.z, sc));
          add(vv.w, guide(vv.w, m.w, sc));
        } else {
          add(vv.x, vv.x);
          add(vv.y, vv.y);
          add(vv.z, vv.z);
          add(vv.w, vv.w);
        }
      } else {
        for (int l = 0; l < 4; ++l) {
          const int64_t i = e + l;
          if (i < lo || i >= hi) continue;
          const float c = v[i];
          add(c, guide_s(c, vu, i, sc));
        }
      }
    }
    const double cntd = (double)(hi - lo);
    if (pass == 0) {
      const double s_c = block_sum(a_c, sh), s_g = block_sum(a_g, sh);
      if (hi > lo) mc = s_c / cntd, mg = s_g / cntd;
    } else {
      const double s_c = block_sum(a_c, sh), s_g = block_sum(a_g, sh), t_c = block_sum(q_c, sh), t_g = block_sum(q_g, sh);
      if (hi > lo) {
        m2c = t_c - s_c * s_c / cntd;   // (the sum of the deviations from the rounded mean is ~0: the textbook correction)
        m2g = t_g - s_g * s_g / cntd;
        if (m2c < 0.0) m2c = 0.0;
        if (m2g < 0.0) m2g = 0.0;
      }
    }
  }
  if (threadIdx.x == 0) {
    double *o = part + ((int64_t)b * nb + blockIdx.x) * kStatsPart;
    o[0] = (double)(hi - lo);
    o[1] = mc;
    o[2] = m2c;
    o[3] = mg;
    o[4] = m2g;
    o[5] = 0.0;
  }
}

// The rescale factor of clip b from its npart partials: Chan's pairwise update in fp64, partial after partial in index order, then
//   r = sqrt(M2(v_c) / M2(g)),  factor = 1 + phi (r - 1), rounded once to fp32;  exactly 1 where M2(g) == 0.
__device__ float rescale_factor(const double *__restrict__ part, int npart, int b, float phi) {
  const double *p = part + (int64_t)b * npart * kStatsPart;
  double n = 0.0, mc = 0.0, m2c = 0.0, mg = 0.0, m2g = 0.0;
  for (int j = 0; j < npart; ++j, p += kStatsPart) {
    const double nj = p[0];
    if (!(nj > 0.0)) continue;
    const double nn = n + nj, w = nj / nn, dc = p[1] - mc, dg = p[3] - mg;
    mc += dc * w;
    mg += dg * w;
    m2c += p[2] + dc * dc * (n * w);
    m2g += p[4] + dg * dg * (n * w);
    n = nn;
  }
  if (!(m2g > 0.0)) return 1.0f;
  return (float)(1.0 + (double)phi * (sqrt(m2c / m2g) - 1.0));
}

constexpr int kFacCache = 32;   // clips whose factor a workgroup keeps in LDS (its contiguous share of the range rarely touches more than two)

// The multistep update with a guidance schedule (range convention of vsampler_update_ms_kernel: whole-tensor bases, elements [e0, e1)):
//   g = s == 1 ? v_c : guide(v_c, v_u, s),   v = phi > 0 ? g * factor(clip) : g,   then the solver row exactly as vsampler_update_ms_kernel,
//   s = gtab[k * B + clip],  clip = element / clip_len,  row = table + 8 k,  k = *step_idx + step_bias.
// Each workgroup takes a CONTIGUOUS share of the range's 4-groups, so it needs the factors of few clips: it combines their partials once, into
// LDS (rescale_factor; element by element where a share touches more than kFacCache clips -- the same function, the same bits).  A 4-group takes
// the 16-byte path only where it lies inside the range and inside one clip.  Nothing that changes between calls is an argument except phi and B.
__global__ void vsampler_update_g_kernel(float *__restrict__ x, const float *__restrict__ v, const float *__restrict__ vu, float *__restrict__ hist,
                                         const float *__restrict__ table, const float *__restrict__ gtab, const int *__restrict__ step_idx,
                                         int step_bias, const double *__restrict__ part, int npart, float phi, int B, int64_t clip_len,
                                         float *__restrict__ fac_out, int64_t e0, int64_t e1, int vec) {
  __shared__ float fac_sh[kFacCache];
  const int k = *step_idx + step_bias;
  const float *row = table + 8 * (int64_t)k;
  const float al = row[0], be = row[1], cx = row[2], c0 = row[3], c1 = row[4];
  const float *srow = gtab + (int64_t)k * B;
  const bool resc = phi > 0.0f;
  const int64_t g_lo = e0 >> 2, ng = ((e1 + 3) >> 2) - g_lo;
  const int64_t per = (ng + gridDim.x - 1) / gridDim.x;
  int64_t t_lo = (int64_t)blockIdx.x * per, t_hi = t_lo + per;
  if (t_hi > ng) t_hi = ng;
  if (fac_out && blockIdx.x == 0)
    for (int b = threadIdx.x; b < B; b += blockDim.x) fac_out[b] = resc ? rescale_factor(part, npart, b, phi) : 1.0f;
  if (t_lo >= t_hi) return;
  // clips of the first and the last element of this workgroup's share
  int64_t f_lo = 4 * (g_lo + t_lo), f_hi = 4 * (g_lo + t_hi);
  if (f_lo < e0) f_lo = e0;
  if (f_hi > e1) f_hi = e1;
  const int64_t c_first = f_lo / clip_len, c_last = (f_hi - 1) / clip_len;
  const bool cached = resc && c_last - c_first < kFacCache;
  if (cached) {
    for (int64_t c = c_first + threadIdx.x; c <= c_last; c += blockDim.x) fac_sh[c - c_first] = rescale_factor(part, npart, (int)c, phi);
    __syncthreads();
  }
  const bool narrow = e1 <= (int64_t)0x7fffffff && clip_len <= (int64_t)0x7fffffff;   // 32-bit division for the clip index where both fit
  for (int64_t t = t_lo + threadIdx.x; t < t_hi; t += blockDim.x) {
    const int64_t e = 4 * (g_lo + t);
    const int64_t c = narrow ? (int64_t)((uint32_t)e / (uint32_t)clip_len) : e / clip_len;
    const bool one_clip = e - c * clip_len + 4 <= clip_len;
    if (vec && one_clip && e >= e0 && e + 4 <= e1) {
      const float sc = srow[c];
      const float4 xx = *reinterpret_cast<const float4 *>(x + e);
      const float4 hh = *reinterpret_cast<const float4 *>(hist + e);
      float4 vv = *reinterpret_cast<const float4 *>(v + e);
      if (vu && sc != 1.0f) {
        const float4 m = *reinterpret_cast<const float4 *>(vu + e);
        vv.x = guide(vv.x, m.x, sc);
        vv.y = guide(vv.y, m.y, sc);
        vv.z = guide(vv.z, m.z, sc);
        vv.w = guide(vv.w, m.w, sc);
      }
      if (resc) {
        const float fac = cached ? fac_sh[c - c_first] : rescale_factor(part, npart, (int)c, phi);
        vv.x = rescaled(vv.x, fac);
        vv.y = rescaled(vv.y, fac);
        vv.z = rescaled(vv.z, fac);
        vv.w = rescaled(vv.w, fac);
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
        const int64_t ci = (i - c * clip_len >= clip_len) ? i / clip_len : c;   // (a clip shorter than a group: past the next one too)
        float vv = guide_s(v[i], vu, i, srow[ci]);
        if (resc) vv = rescaled(vv, cached ? fac_sh[ci - c_first] : rescale_factor(part, npart, (int)ci, phi));
        const float xx = x[i];
        const float X = ms_x0(xx, vv, al, be);
        x[i] = ms_next(xx, X, hist[i], cx, c0, c1);
        hist[i] = X;
      }
    }
  }
}

}  // namespace

int guidance_stats_blocks(int64_t clip_len) {
  int64_t nb = (clip_len + 4095) / 4096;   // 16 elements per thread and pass
  return (int)(nb < 1 ? 1 : (nb > 64 ? 64 : nb));
}

hipError_t launch_guidance_stats(const float *v, const float *v_uncond, const float *gtab, const int *step_idx, int step_bias, int B,
                                 int64_t clip_len, double *part, hipStream_t s) {
  if (B < 1 || clip_len < 1) return hipSuccess;
  auto al16 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const int vec = al16(v) && (!v_uncond || al16(v_uncond));
  hipLaunchKernelGGL(guidance_stats_kernel, dim3((unsigned)guidance_stats_blocks(clip_len), (unsigned)B), dim3(TPB), 0, s, v, v_uncond, gtab, step_idx,
                     step_bias, B, clip_len, part, vec);
  return hipGetLastError();
}

hipError_t launch_vsampler_update_g(float *x, const float *v, const float *v_uncond, float *hist, const float *table, const float *gtab,
                                    const int *step_idx, int step_bias, const double *part, float phi, int B, int64_t clip_len, float *fac_out,
                                    int64_t e0, int64_t e1, hipStream_t s) {
  if (e1 <= e0) return hipSuccess;
  auto al16 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const int vec = al16(x) && al16(v) && (!v_uncond || al16(v_uncond)) && al16(hist);
  hipLaunchKernelGGL(vsampler_update_g_kernel, grid_for((e1 - e0 + 3) / 4 + 1), dim3(TPB), 0, s, x, v, v_uncond, hist, table, gtab, step_idx, step_bias,
                     part, guidance_stats_blocks(clip_len), phi, B, clip_len, fac_out, e0, e1, vec);
  return hipGetLastError();
}

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
