// Implicit-GEMM convolution on the CDNA4 matrix cores (wave64 MFMA 32x32).
//
//   out[m][n] = epi( sum_k A(m,k) * W[n][k] ),  m = output row (channels-last), n = output channel.
//
// One 256-thread workgroup (4 waves) owns a BM x BN output tile; the K loop walks 32-wide
// slices of the (tap, channel) axis.  Because activations are channels-last, a K slice of one
// tap is a contiguous 128-byte (fp32) / 64-byte (bf16) run of one source row, so the A tile is
// gathered with 16-byte loads, transformed in registers (GroupNorm+SiLU prologue: one fma and
// one SiLU per element from a per-(clip,channel) table in LDS) and staged in LDS; the W tile is
// K-contiguous too.  Global loads of slice t+1 are issued before the MFMAs of slice t and
// written to LDS after them (issue-early / write-late).
//
//   fp32 path : v_mfma_f32_32x32x2_f32  (exact fp32 fma chain; K order permuted {s, 16+s})
//   bf16 path : v_mfma_f32_32x32x16_bf16 (fp32 accumulate)
#include <cstring>
#include <set>
#include <string>

#include "common.h"
#include "kernels.h"

namespace sf {

namespace {

constexpr int BK = 32;

template <typename T> struct Lds {
  // row stride of an LDS tile in elements: 32 + one 16-byte pad
  static constexpr int LD = BK + 16 / (int)sizeof(T);
};

struct RowState {  // per staged A row held by a thread
  int valid_m;     // m < M
  int b_rel;       // clip index relative to the tile's first clip (GN table)
  int p0;          // 1-D: l*stride - pad ;  video: unused
  int base;        // 1-D: b*Lsrc ; video: n
  int t, h, w;     // video coordinates (already multiplied by stride, minus pad)
};

template <typename T, int BM, int BN, int WM_, int WN_, bool SCALAR_A>
__global__ __launch_bounds__(256) void conv_gemm_kernel(const ConvGemmArgs a) {
  constexpr int VEC = Vec16<T>::N;
  constexpr int VPR = BK / VEC;        // 16-byte vectors per tile row
  constexpr int RPP = 256 / VPR;       // rows staged per pass
  constexpr int PA = BM / RPP;
  constexpr int PB = (BN + RPP - 1) / RPP;   // BN < RPP: only the first BN*VPR threads stage W
  static_assert(PA >= 1 && BM % RPP == 0, "tile too small for the staging pattern");
  constexpr int LD = Lds<T>::LD;
  constexpr int WTM = BM / WM_, WTN = BN / WN_;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr bool FAST = sizeof(T) == 2;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T *As = reinterpret_cast<T *>(smem);
  T *Bs = As + BM * LD;
  float2 *tab = reinterpret_cast<float2 *>(Bs + BN * LD);  // GN: (scale, shift) per (clip, channel)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave / WN_, wc = wave % WN_;
  const int m0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;

  const T *src = static_cast<const T *>(a.src);
  const T *src2 = static_cast<const T *>(a.src2);
  const T *wgt = static_cast<const T *>(a.w);

  const int srow = tid / VPR;   // row within a pass
  const int svec = tid % VPR;   // vector within the row

  // ---- per-row state of the A rows this thread stages -------------------------------------
  RowState rs[PA];
  const int b_first = (a.geom == 0) ? (m0 / a.Lout) : 0;
#pragma unroll
  for (int i = 0; i < PA; ++i) {
    int m = m0 + i * RPP + srow;
    rs[i].valid_m = m < a.M;
    int mm = rs[i].valid_m ? m : 0;
    if (a.geom == 0) {
      int b = mm / a.Lout;
      int l = mm - b * a.Lout;
      rs[i].b_rel = b - b_first;
      rs[i].p0 = l * a.stride - a.pad;
      rs[i].base = b * a.Lsrc;
      rs[i].t = rs[i].h = rs[i].w = 0;
    } else {
      int w_ = mm % a.Wo;
      int r = mm / a.Wo;
      int h_ = r % a.Ho;
      r /= a.Ho;
      int t_ = r % a.To;
      int n_ = r / a.To;
      rs[i].b_rel = 0;
      rs[i].p0 = 0;
      rs[i].base = n_;
      rs[i].t = t_ * a.st - a.pt;
      rs[i].h = h_ * a.sh - a.ph;
      rs[i].w = w_ * a.sw - a.pw;
    }
  }

  // ---- GroupNorm+SiLU prologue table ----------------------------------------------------------
  if (a.pro == 1) {
    const int b_last = min(a.M - 1, m0 + BM - 1) / a.Lout;
    const int nb = b_last - b_first + 1;
    float2 *mr = tab + (size_t)a.cin * nb;  // (mean, rstd) per (clip, group), behind the table
    const int cpg = a.cin / a.G;
    for (int idx = tid >> 5; idx < nb * a.G; idx += 8) {   // one half-wave per (clip, group)
      const int bl = idx / a.G, g = idx - bl * a.G;
      const float *sl = a.stats + ((size_t)(b_first + bl) * a.nch) * a.G * 2 + g * 2;
      const float2 r = gn_merge32(sl, a.G, a.nch, a.chunk_rows, a.Lsrc, cpg, a.eps, tid & 31);
      if ((tid & 31) == 0) mr[idx] = r;
    }
    __syncthreads();
    for (int idx = tid; idx < nb * a.cin; idx += 256) {
      int bl = idx / a.cin, c = idx - bl * a.cin;
      float2 s = mr[bl * a.G + c / cpg];
      float sc = s.y * a.gamma[c];
      tab[idx] = make_float2(sc, a.beta[c] - s.x * sc);
    }
    __syncthreads();
  }

  // ---- accumulators ---------------------------------------------------------------------------
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  Vec16<T> ra[PA], rb[PB];
  int bvalid[PB];
  int rvalid[PA];  // source row in range (bit) for the prefetched slice
  int rci0 = 0;    // first channel of the prefetched slice (GN table index)
  int rsecond = 0; // slice comes from src2

  const int nkt = (a.K + BK - 1) / BK;
  const int k_taps = a.taps * a.cin;

  auto prefetch = [&](int kt) {
    const int k0 = kt * BK;
    // ---- W tile ----
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      int n = n0 + i * RPP + srow;
      int k = k0 + svec * VEC;
      if (i * RPP + srow >= BN) n = a.N;  // outside the tile
      // unconditional load from a clamped address (K is a multiple of 8 on every path); zeroed at stage time
      bvalid[i] = (n < a.N) && (k + VEC <= a.K);
      rb[i] = ld16<T>(wgt + (size_t)min(n, a.N - 1) * a.K + min(k, a.K - VEC));
    }
    // ---- A tile ----
    if constexpr (!SCALAR_A) {
      if (k0 < k_taps) {
        const int tap = k0 / a.cin;
        const int ci0 = k0 - tap * a.cin;
        rci0 = ci0 + svec * VEC;
        rsecond = 0;
        int dt = 0, dh = 0, dw = 0;
        if (a.geom == 1) {
          dw = tap % a.kw;
          int r = tap / a.kw;
          dh = r % a.kh;
          dt = r / a.kh;
        }
#pragma unroll
        for (int i = 0; i < PA; ++i) {
          int ok = rs[i].valid_m;
          size_t row;
          if (a.geom == 0) {
            int p = rs[i].p0 + tap;
            const int pmax = (a.Lsrc << a.up_shift) - 1;
            ok = ok && p >= 0 && p <= pmax;
            row = (size_t)(rs[i].base + (min(max(p, 0), pmax) >> a.up_shift));
          } else {
            int ti = rs[i].t + dt, hi = rs[i].h + dh, wi = rs[i].w + dw;
            ok = ok && ti >= 0 && ti < a.Ti && hi >= 0 && hi < a.Hi && wi >= 0 && wi < a.Wi;
            row = ((size_t)(rs[i].base * a.Ti + min(max(ti, 0), a.Ti - 1)) * a.Hi + min(max(hi, 0), a.Hi - 1)) * a.Wi + min(max(wi, 0), a.Wi - 1);
          }
          rvalid[i] = ok;
          ra[i] = ld16<T>(src + row * a.src_ld + rci0);  // unconditional (clamped row); zeroed at stage time
        }
      } else {
        const int ci0 = k0 - k_taps + svec * VEC;
        rsecond = 1;
#pragma unroll
        for (int i = 0; i < PA; ++i) {
          const int m = min(m0 + i * RPP + srow, a.M - 1);
          rvalid[i] = rs[i].valid_m;
          ra[i] = ld16<T>(src2 + (size_t)m * a.src2_ld + ci0);
        }
      }
    } else {
      // per-element (tap, channel) decode: thin-channel layers such as the RGB stem
      rsecond = 0;
#pragma unroll
      for (int i = 0; i < PA; ++i) {
        Vec16<T> v = zero16<T>();
        rvalid[i] = 0;
        if (rs[i].valid_m) {
          for (int j = 0; j < VEC; ++j) {
            int k = k0 + svec * VEC + j;
            if (k >= k_taps) break;
            int tap = k / a.cin, ci = k - tap * a.cin;
            int ok;
            size_t row;
            if (a.geom == 0) {
              int p = rs[i].p0 + tap;
              ok = p >= 0 && p < (a.Lsrc << a.up_shift);
              row = (size_t)(rs[i].base + (max(p, 0) >> a.up_shift));
            } else {
              int dw = tap % a.kw;
              int r = tap / a.kw;
              int dh = r % a.kh;
              int dt = r / a.kh;
              int ti = rs[i].t + dt, hi = rs[i].h + dh, wi = rs[i].w + dw;
              ok = ti >= 0 && ti < a.Ti && hi >= 0 && hi < a.Hi && wi >= 0 && wi < a.Wi;
              row = ((size_t)(rs[i].base * a.Ti + max(ti, 0)) * a.Hi + max(hi, 0)) * a.Wi + max(wi, 0);
            }
            if (ok) v.set(j, to_f(src[row * a.src_ld + ci]));
          }
        }
        ra[i] = v;
      }
    }
  };

  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < PB; ++i)
      if (i * RPP + srow < BN) st16<T>(Bs + (i * RPP + srow) * LD + svec * VEC, bvalid[i] ? rb[i] : zero16<T>());
#pragma unroll
    for (int i = 0; i < PA; ++i) {
      Vec16<T> v = (SCALAR_A || rvalid[i]) ? ra[i] : zero16<T>();
      if (a.pro == 1 && !rsecond && rvalid[i]) {
        const float2 *tb = tab + (size_t)rs[i].b_rel * a.cin + rci0;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          float2 sd = tb[j];
          float y = fmaf(v.get(j), sd.x, sd.y);
          v.set(j, silu_t<FAST>(y));
        }
      }
      st16<T>(As + (i * RPP + srow) * LD + svec * VEC, v);
    }
  };

  const int fr = lane & 31, fh = lane >> 5;

  auto compute = [&]() {
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        using frag = typename Frag16<T>::type;
        frag af[TM], bfr[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
          af[i] = *reinterpret_cast<const frag *>(As + (wr * WTM + i * 32 + fr) * LD + 16 * s + 8 * fh);
#pragma unroll
        for (int j = 0; j < TN; ++j)
          bfr[j] = *reinterpret_cast<const frag *>(Bs + (wc * WTN + j * 32 + fr) * LD + 16 * s + 8 * fh);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = mfma32x16(af[i], bfr[j], acc[i][j]);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 af[TM], bfr[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
          af[i] = *reinterpret_cast<const f32x4 *>(As + (wr * WTM + i * 32 + fr) * LD + 16 * fh + 4 * q);
#pragma unroll
        for (int j = 0; j < TN; ++j)
          bfr[j] = *reinterpret_cast<const f32x4 *>(Bs + (wc * WTN + j * 32 + fr) * LD + 16 * fh + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bfr[j][e], acc[i][j], 0, 0, 0);
      }
    }
  };

  // ---- main loop ------------------------------------------------------------------------------
  prefetch(0);
  stage();
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const bool more = kt + 1 < nkt;
    if (more) prefetch(kt + 1);
    compute();
    __syncthreads();
    if (more) {
      stage();
      __syncthreads();
    }
  }

  // ---- epilogue -------------------------------------------------------------------------------
  // Every operand load is UNCONDITIONAL (indices clamped into range) and batched per 32x32 tile, so the 16
  // residual / per-clip loads of a lane are all in flight together; only the stores are predicated.
  T *out = static_cast<T *>(a.out);
  const T *res = static_cast<const T *>(a.res);
  const bool has_res = res != nullptr, has_bs = a.bscale != nullptr, has_ba = a.badd != nullptr, has_b = has_bs || has_ba;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + wc * WTN + j * 32 + fr;
    const int nc = min(n, a.N - 1);
    const bool real = n < a.N;
    const float bias = a.bias ? a.bias[nc] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      float rv[16], sv[16], av[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = min(m0 + wr * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh, a.M - 1);
        rv[r] = has_res ? to_f(res[(size_t)m * a.res_ld + nc]) : 0.f;
        const int b = has_b ? m / a.Lout : 0;
        sv[r] = has_bs ? a.bscale[(size_t)b * a.bscale_ld + nc] : 1.f;
        av[r] = has_ba ? a.badd[(size_t)b * a.badd_ld + nc] : 0.f;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wr * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
        float v = (acc[i][j][r] + bias) * sv[r] + rv[r] + av[r];
        v = real ? apply_act(v, a.act) : 0.f;
        if (m < a.M && n < a.n_store) {
          if (a.out_f32) static_cast<float *>(a.out)[(size_t)m * a.out_ld + n] = v;
          else out[(size_t)m * a.out_ld + n] = from_f<T>(v);
        }
      }
    }
  }
}

template <typename T, int BM, int BN, int WM_, int WN_, bool SC>
hipError_t launch_cfg(const ConvGemmArgs &a, hipStream_t s) {
  constexpr int LD = Lds<T>::LD;
  size_t lds = (size_t)(BM + BN) * LD * sizeof(T);
  if (a.pro == 1) {
    int nb = min(a.M / a.Lout + (a.M % a.Lout ? 1 : 0), BM / a.Lout + 2);
    lds += (size_t)nb * (a.cin + a.G) * sizeof(float2);
  }
  dim3 grid((a.M + BM - 1) / BM, (a.n_store + BN - 1) / BN);
  auto kern = conv_gemm_kernel<T, BM, BN, WM_, WN_, SC>;
  static bool big_lds_enabled = false;  // one-time opt-in to > 48 KiB of dynamic LDS (never inside graph capture)
  if (!big_lds_enabled) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    if (e != hipSuccess) return e;
    big_lds_enabled = true;
  }
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a);
  return hipGetLastError();
}

// tile variants: 0 scalar-A 64x64, 1 128x32, 2 128x64, 3 64x64, 4 128x128
template <typename T> hipError_t launch_classic(const ConvGemmArgs &a, int tile, hipStream_t s) {
  switch (tile) {
    case 0: return launch_cfg<T, 64, 64, 2, 2, true>(a, s);
    case 1: return launch_cfg<T, 128, 32, 4, 1, false>(a, s);
    case 2: return launch_cfg<T, 128, 64, 2, 2, false>(a, s);
    case 3: return launch_cfg<T, 64, 64, 2, 2, false>(a, s);
    case 4: return launch_cfg<T, 128, 128, 2, 2, false>(a, s);
    default: return hipErrorInvalidValue;
  }
}

// One name table per family: labels are profiling keys and test keys, built once from (family, tile, operand type) and kept by pointer.
struct Labels {
  static constexpr int NT = CG_MT_TILES;
  const char *at[CG_MT + 1][NT + 1][4] = {};   // [family][tile; NT = no tile in the name][f32, x3, bf16, f16]
  std::set<std::string> pool;
  Labels() {
    static const char *const stem[CG_MT + 1] = {nullptr, "conv_gemm", "conv_gemm_v2", "conv_gemm_sk", "conv_gemm_fast", "conv_gemm_wp", "conv_gemm_rs", "conv_gemm_mt"};
    static const char *const tiles[CG_MT + 1][NT] = {
        {},
        {"64x64,scalarA", "128x32", "128x64", "64x64", "128x128"},
        {"128x128", "128x64", "64x64"},
        {"64x64", "64x32", "32x32"},
        {"64x64", "64x32", "32x32"},
        {"64x64", "64x32", "32x32"},
        {"32x32"},
        {"256x128", "128x128", "128x192", "192x128", "256x64", "128x128,2wg", "128x192,2wg", "128x64,2wg", "192x128,2wg", "256x64,2wg", "256x256"}};
    static const char *const type[3] = {"f32", "x3", "bf16"};
    for (int f = CG_CLASSIC; f <= CG_MT; ++f)
      for (int t = 0; t <= NT; ++t)
        for (int ty = 0; ty < 3; ++ty) {
          if (t < NT && !tiles[f][t]) continue;
          const std::string name = std::string(stem[f]) + "<" + type[ty] + (t < NT ? std::string(",") + tiles[f][t] : std::string()) + ">";
          at[f][t][ty] = pool.insert(name).first->c_str();
          if (ty == 2) at[f][t][3] = label_for_dtype(F16, at[f][t][2]);
        }
  }
};
const char *plan_label(int dt, const ConvGemmPlan &p) {
  static const Labels l;
  if (p.family == CG_INVALID) return "conv_gemm<invalid>";
  const bool no_tile = p.family == CG_MT && dt == F32;   // conv_gemm_mt<f32> / conv_gemm_mt<x3>: one label for every tile
  const char *name = l.at[p.family][no_tile ? Labels::NT : p.tile][dt == F32 ? (p.split ? 1 : 0) : dt == BF16 ? 2 : 3];
  return name ? name : "conv_gemm<invalid>";
}

// tuning hook: below this many 64x64 tiles a GEMM goes to the wave-split-K / wave-private kernels
long short_act_tiles() {
  static const long v = [] {
    const char *e = tune_env("SF_SHORT_TILES");
    const long t = e ? atol(e) : 0;
    return t > 0 ? t : 500L;
  }();
  return v;
}

// classic tile: 0 scalar-A 64x64, 1 128x32, 2 128x64, 3 64x64, 4 128x128; -1: no classic kernel takes the shape
int classic_tile(const ConvGemmArgs &a) {
  if (g_conv_gemm_force.path == 1 && g_conv_gemm_force.tile >= 1 && g_conv_gemm_force.tile <= 4) return g_conv_gemm_force.tile;
  const bool scalar_a = (a.cin % BK) != 0 || (a.cin2 % BK) != 0;
  if (scalar_a) return (a.cin2 != 0 || a.pro != 0) ? -1 : 0;
  const long M = a.M, N = a.n_store;
  auto blocks = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((N + bn - 1) / bn); };
  if (N <= 32) return 1;
  if (N <= 64) return blocks(128, 64) >= 512 ? 2 : 3;
  if (blocks(128, 128) >= 512) return 4;
  if (blocks(128, 64) >= 384) return 2;
  return 3;
}

bool mt_wanted(int dt, const ConvGemmArgs &a) { return conv_gemm_mt_ok(dt, a) && conv_gemm_mt_prefers(dt, a); }

ConvGemmPlan mt_plan(int dt, const ConvGemmArgs &a) {
  ConvGemmPlan p;
  p.family = CG_MT;
  p.tile = conv_gemm_mt_tile(dt, a);
  p.split = dt == F32 && a.wx ? (a.wx_mode == X3_BF16 ? X3_BF16 : X3_F16) : 0;
  return p;
}

ConvGemmArgs without_rowpart(ConvGemmArgs a) {
  a.rowpart_out = nullptr;
  return a;
}

alignas(16) float g_armed[4];   // what a query arms its copy of the arguments with: only whether a pointer is set enters a plan

}  // namespace

ConvGemmForce g_conv_gemm_force;

bool conv_gemm_supported(int dt, const ConvGemmArgs &a) {
  (void)dt;
  if (a.M <= 0 || a.N <= 0 || a.K <= 0) return false;
  if (a.pro == 1) {
    if (a.geom != 0 || a.cin % BK || a.cin % a.G) return false;
    int nb = min(a.M / a.Lout + 1, 128 / a.Lout + 2);
    if ((size_t)nb * (a.cin + a.G) * 8 > 96 * 1024) return false;
  }
  return true;
}

// profiling label of a 16-bit kernel in the f16 build: the bf16 label with the type renamed (interned: labels are kept by pointer)
const char *label_for_dtype(int dt, const char *bf16_label) {
  if (dt != F16) return bf16_label;
  static std::set<std::string> pool;
  std::string s(bf16_label);
  const size_t at = s.find("bf16");
  if (at != std::string::npos) s.replace(at, 4, "f16");
  return pool.insert(s).first->c_str();
}

// The decision of launch_conv_gemm.  Automatic (ConvGemmForce::path == 0):
//   macro tiles where eligible and preferred; otherwise long activations take v2 and short ones (fewer than short_act_tiles() tiles of
//   64x64, or a classic tiling that would leave most CUs idle) the small-batch cascade rs -> wp -> fast -> sk; the classic tiles take the rest.
// Forced (sf_bench_conv1d): 1 classic, 2 the cascade without rs / wp, 4 v2, 5 the cascade with wp preferred, 6 macro tiles; a forced launch
// carries no fused epilogue statistics and no pre-split source.
ConvGemmPlan conv_gemm_plan(int dt, const ConvGemmArgs &a) {
  const ConvGemmForce &f = g_conv_gemm_force;
  ConvGemmPlan p;
  const bool automatic = f.path == 0;
  if (!conv_gemm_supported(dt, a) || (a.src_x3 && !automatic)) return p;
  if (f.path == 6 ? conv_gemm_mt_ok(dt, a) : (automatic && mt_wanted(dt, a))) {
    p = mt_plan(dt, a);
    p.src_x3 = automatic && a.src_x3;                                   // (conv_gemm_mt_ok has checked what the pre-split form needs)
    p.rowpart = automatic && a.rowpart_out != nullptr && a.mt_ln != 0;   // the caller allows the row-LayerNorm fusion on the macro tiles
  } else if (f.path == 6 || a.src_x3) {
    return p;   // only the macro tiles read pre-split rows
  } else {
    // Macro tiles pay from ~80 tiles of 256x128 per launch (conv_gemm_mt.hip); below short_act_tiles() tiles of 64x64 the small-batch
    // kernels win.  K >= 256: their pipelines need a few steps to reach steady state.
    const long t64 = (long)((a.M + 63) / 64) * ((a.n_store + 63) / 64);
    const bool short_act = t64 < short_act_tiles() && a.K >= (a.short_k ? 128 : 256) && (a.K % 32) == 0 && (a.cin % 32) == 0 && (a.cin2 % 32) == 0;
    const int ct = classic_tile(a);
    // the classic tiling would leave most CUs idle: the wave-split-K kernels
    auto use_sk = [&] {
      static const int bm[5] = {64, 128, 128, 64, 128}, bn[5] = {64, 32, 64, 64, 128};
      return ct > 0 && (a.K % 32) == 0 && a.K >= 256 && (long)((a.M + bm[ct] - 1) / bm[ct]) * ((a.n_store + bn[ct] - 1) / bn[ct]) < 256;
    };
    if ((f.path == 4 || (automatic && !short_act)) && conv_gemm_v2_plan(dt, a, p.tile)) {
      p.family = CG_V2;   // long activations: 2x2-wave tiles, channel counts that are multiples of 64, no prologue
    } else if (f.path == 4) {
      return p;
    } else if (f.path == 2 || f.path == 5 || (automatic && (short_act || use_sk()))) {
      if ((a.cin % 32) || (a.cin2 % 32) || (a.K % 32)) return p;
      const int v = conv_gemm_sk_variant(a);
      // barrier-free wave-private pipelines where few tiles exist (conv_gemm_prefers_wp); with many tiles the staged kernels win because
      // their loads are shared by more MFMA work per byte
      const bool wp_prefers = f.path == 5 || (automatic && conv_gemm_prefers_wp(a));
      const bool wp = wp_prefers && conv_gemm_wp_ok(dt, a);
      const int x3 = dt == F32 && a.wx ? (a.wx_mode == X3_BF16 ? X3_BF16 : X3_F16) : 0;
      if (automatic && wp_prefers && v == 2 && conv_gemm_rs_ok(dt, a)) {
        p.family = CG_RS;   // few 32x32 tiles and fragment-ordered weights at hand: all loads of a wave up front
        p.tile = 0;
        p.split = dt == F32 ? X3_F16 : 0;
      } else if (wp && !(x3 == X3_BF16 && a.cin2)) {   // (the split bf16 form has one source: gradient GEMMs)
        p.family = CG_WP;
        p.tile = dt == F32 ? 2 : v;   // fp32 launches take the 32x32 tile
        p.split = x3;
      } else if (conv_gemm_fast_ok(dt, a)) {
        p.family = CG_FAST;
        p.tile = v;
        p.split = dt == F32 && a.wx && (a.wx_mode == X3_F16 || (a.wx_mode == X3_BF16 && !a.cin2)) ? a.wx_mode : 0;
        p.wide = !p.split && (a.cin % 256) == 0 && f.sk == 64;   // measured: no gain over 128-wide chunks
      } else {
        p.family = CG_SK;
        p.tile = v;
      }
      // Epilogue statistics (32x32 tiles that hold whole 32-column groups).  A launch that the macro tiles would take without the row
      // partials stays there: arming them must not move it.  (rs launches keep the rule of the kernels they took over from.)
      const bool epi = automatic && v == 2 && p.family != CG_SK && (a.n_store % 32) == 0 && a.n_store == a.N && (wp || conv_gemm_fast_ok(dt, a)) &&
                       !(a.rowpart_out && mt_wanted(dt, without_rowpart(a)));
      p.rowpart = epi;
      p.gnpart = epi && wp && p.family != CG_FAST && a.Lout >= 32;   // wp / rs write them: a tile touches at most two clips
    } else if (ct >= 0) {
      p.family = CG_CLASSIC;
      p.tile = ct;
    }
  }
  p.label = plan_label(dt, p);
  return p;
}

// The decision of launch_conv_gemm_ln: the first source (cin channels, one tap) is LayerNorm-modulated on the fly from row partials.
ConvGemmPlan conv_gemm_ln_plan(int dt, const ConvGemmArgs &a) {
  ConvGemmPlan p;
  p.ln = true;
  ConvGemmArgs plain = a;
  plain.ln_part = nullptr;
  plain.ln_colsum = nullptr;
  plain.ln_ss = nullptr;
  plain.rowpart_out = nullptr;
  plain.res_ln = 0;
  const bool acc_side = a.ln_colsum && !a.ln_ss && !a.res_ln;   // LayerNorm applied to the accumulator: raw rows through the matrix cores
  if (mt_wanted(dt, plain)) {
    // long activations: the macro-tile GEMM beats the LayerNorm-fused 32x32 kernel; it carries the accumulator-side LayerNorm but no
    // operand transform (Modulation + InjectChannels keep their ln_modulate launch there), and only where the caller allows it
    if (a.mt_ln == 0 || !a.ln_part || !acc_side || !conv_gemm_mt_ok(dt, a)) return p;
    const bool rowpart = a.rowpart_out != nullptr;
    p = mt_plan(dt, a);
    p.ln = true;
    p.rowpart = rowpart;
  } else {
    if (!conv_gemm_fast_ok(dt, a)) return p;
    // the operand-transform form runs on the 32x32 staged kernel: short activations only (with the macro-tile row partials a long
    // producer can offer them too -- depth 3 at batch 32: 8 launches of 13 us more than ln_modulate + the 64x64 kernel)
    if (!acc_side && (long)((a.M + 63) / 64) * ((a.n_store + 63) / 64) >= 500) return p;
    if (a.taps != 1 || a.stride != 1 || a.up_shift != 0 || a.Lout != a.Lsrc || a.Lout < 32) return p;
    if (!a.ln_part || a.ln_nt * 32 != a.cin || a.ln_nt > 32) return p;
    if (a.res_ln && (a.N != a.cin || !a.res)) return p;
    if (a.ln_colsum && (a.cin2 || a.ln_ss || a.res_ln)) return p;
    if (a.rowpart_out && ((a.n_store % 32) || a.rowpart_nt * 32 != a.n_store)) return p;
    static const long rs_max_tiles = [] {   // tuning hook: most 32x32 tiles a LayerNorm-folded projection may have and still take the register-staged kernel
      const char *e = tune_env("SF_RS_LN_TILES");
      return e ? atol(e) : 512L;
    }();
    // tuning hook: the wave-private kernel also carries the epilogue fold, but on the qkv projections of this model (288 tiles,
    // K = 1024) the staged kernel measured 1.2 % faster over a whole step (460 vs 455 steps/s), so it stays opt-in
    static const bool use_wp = tune_env("SF_LN_WP") != nullptr;
    const long tiles = (long)((a.M + 31) / 32) * ((a.n_store + 31) / 32);
    const int x3 = dt == F32 && a.wx ? (a.wx_mode == X3_BF16 ? X3_BF16 : X3_F16) : 0;
    p.tile = 2;
    p.rowpart = a.rowpart_out != nullptr;
    if (acc_side && g_conv_gemm_force.path == 0 && tiles <= rs_max_tiles && a.K >= 256 && conv_gemm_rs_ok(dt, a)) {
      p.family = CG_RS;   // fragment-ordered weights at hand and few tiles
      p.tile = 0;
      p.split = dt == F32 ? X3_F16 : 0;
    } else if (use_wp && acc_side && !a.rowpart_out && conv_gemm_wp_ok(dt, a)) {
      p.family = CG_WP;
      p.split = x3;
    } else {
      p.family = CG_FAST;
      p.split = x3 == X3_F16 ? X3_F16 : 0;
    }
  }
  p.label = plan_label(dt, p);
  return p;
}

hipError_t launch_conv_gemm_planned(int dt, const ConvGemmArgs &a, const ConvGemmPlan &p, hipStream_t s) {
  switch (p.family) {
    case CG_CLASSIC: return SF_DISPATCH_T(dt, launch_classic<T>(a, p.tile, s));
    case CG_V2: return launch_conv_gemm_v2(dt, a, p.tile, s);
    case CG_SK: return launch_conv_gemm_sk(dt, a, p.tile, s);
    case CG_FAST: return launch_conv_gemm_fast(dt, a, p, s);
    case CG_WP: return launch_conv_gemm_wp(dt, a, p.tile, p.split, s);
    case CG_RS: return launch_conv_gemm_rs(dt, a, s);
    case CG_MT: return launch_conv_gemm_mt(dt, a, p.tile, p.split, s);
    default: return hipErrorInvalidValue;
  }
}
hipError_t launch_conv_gemm(int dt, const ConvGemmArgs &a, hipStream_t s) { return launch_conv_gemm_planned(dt, a, conv_gemm_plan(dt, a), s); }
hipError_t launch_conv_gemm_ln(int dt, const ConvGemmArgs &a, hipStream_t s) { return launch_conv_gemm_planned(dt, a, conv_gemm_ln_plan(dt, a), s); }

const char *conv_gemm_variant_name(int dt, const ConvGemmArgs &a) { return conv_gemm_plan(dt, a).label; }
const char *conv_gemm_ln_variant_name(int dt, const ConvGemmArgs &a) { return conv_gemm_ln_plan(dt, a).label; }
bool conv_gemm_ln_ok(int dt, const ConvGemmArgs &a) { return conv_gemm_ln_plan(dt, a).family != CG_INVALID; }

// The queries below are asked before the caller sets the pointer or flag in question: each arms its copy and reads the plan.
// (A wrong answer of conv_gemm_reads_split_only is a memory fault, not a wrong number: the training step then packs no fp32 image and
// passes a null `w`.)
bool conv_gemm_reads_split_only(int dt, const ConvGemmArgs &a_in) {
  ConvGemmArgs a = a_in;
  if (!a.wx) a.wx = g_armed;
  return conv_gemm_plan(dt, a).split != 0;
}
bool conv_gemm_emits_rowpart(int dt, const ConvGemmArgs &a_in) {
  ConvGemmArgs a = a_in;
  if (!a.rowpart_out) {
    a.rowpart_out = g_armed;
    a.rowpart_nt = a.n_store / 32;
  }
  return conv_gemm_plan(dt, a).rowpart;
}
bool conv_gemm_emits_gnpart(int dt, const ConvGemmArgs &a_in) {
  ConvGemmArgs a = a_in;
  if (!a.gnpart_out) a.gnpart_out = g_armed;
  return conv_gemm_plan(dt, a).gnpart;
}
bool conv_gemm_src_x3_ok(const ConvGemmArgs &a_in) {
  ConvGemmArgs a = a_in;
  a.src_x3 = 1;
  return conv_gemm_plan(F32, a).src_x3;
}

}  // namespace sf
