// Channel-block split-K convolution ("cb") for the DEEP U-Net levels at small batch, and the two launches that consume it.
//
// What the wave-private 32x32 kernel (conv_gemm_wp.hip) pays at depths 5-7: a tile streams (32 + 32) * K * 2 B = 393 KB at
// K = 3072 through ONE CU, 192 such workgroups move 75 MB through the vector caches for 6.3 MB of weights (a 12-fold operand
// amplification at the chip's ~14 TB/s L2 -> CU ceiling), and its output feeds a launch that reads the whole tensor anyway
// (GroupNorm+SiLU, or LayerNorm+Modulation).  Here the reduction is split over WORKGROUPS along the input channels:
//
//   conv_cb        one workgroup = BM rows (32 * MT, flat over the clips) x 128 output columns x ONE 128-channel block of the
//                  input, all three taps of it (K slice = 3 * 128).  The activation panel ((BM + 2) rows x 128 channels) is read
//                  ONCE for the three taps, optionally GroupNorm+SiLU'd on the way into LDS (23-35 elements per thread: the
//                  prologue that cost +11 us on full-K tiles is 0.3 us here); the weight slice arrives in MFMA FRAGMENT ORDER
//                  (packed once per weight version: a wave's 16-byte-per-lane load is 1 KB contiguous), straight into registers,
//                  all 24 loads of a wave issued up front behind the panel loads -- they do not depend on the producer kernel.
//                  A workgroup streams 107-131 KB instead of 393 KB; d7 (M = 176): 192 workgroups x 115 KB = 22 MB.
//                  Output: fp32 partial slabs  slab[cb][m][n]  (no bias), written through (sc1) in whole 128-byte lines.
//   cb_reduce_gn   the launch that already followed conv1 (gn_silu) becomes the reducer: sum of the slabs + bias -> h (16-bit)
//                  and the GroupNorm chunk partials of h; >= 176 workgroups instead of 32.  The second convolution applies
//                  GroupNorm+SiLU from those partials in its panel prologue.
//   cb_reduce_ln   the launch that already followed conv2 (ln_modulate): sum of the slabs + bias + residual x -> y (never stored),
//                  LayerNorm over the row in fp32, Modulation -> m (16-bit).
// No tickets, no last-arriver, no extra kernel boundary: the reduction rides with launches the chain already had.
//
// Reference arithmetic: a-unet ResnetItem / ModulationItem (exp/model/diffusion.yaml:17-19).
#include <cstdlib>

#include "common.h"
#include "kernels.h"

namespace sf {
namespace {

constexpr int KC = 128;         // input channels per workgroup (one K block = 3 taps x 128)
constexpr int KC_LOG2 = 7;
constexpr int NSLOT = 4;        // clips a (BM + 2 <= 130)-row panel may touch: L >= 44 (host guarantees it)

// Partial-slab stores of one wave's 32 x 32 fp32 tile: rows m0 .. m0 + 31 of the workgroup's own slab behind resource rB, col_b = byte offset of
// the wave's first column; lane (fr, fh) holds v[g] = columns 8 g + 4 fh + 0..3 of row fr.  The NEXT launch reads the slabs on other XCDs, so
// every byte has to leave this XCD's L2 before the kernel boundary.  sc1 (aux 16) writes it through while the kernel still runs instead of
// leaving it to the write-back behind the kernel -- but a write-through store is one fabric write per contiguous piece, and in the
// accumulator layout a store instruction touches 32 rows x 32 B.  So the tile passes through `stage` (SLAB_STAGE floats per wave: 16 rows at
// a time, pitch 36 floats -- the 8 lanes of a row write 8 distinct 16-byte slots, a row is read back as 128 contiguous bytes) and every store
// instruction writes 8 whole 128-byte lines (8 lanes x 16 B = one row), 4 instructions per tile as before.  Rows m >= M get the out-of-range
// offset: the resource drops them.  Measured (profiles/HISTORY.md, "conv_cb slab stores"): whole lines + sc1 +1.4 .. 3.2 % on configs[1];
// sc1 on the accumulator layout -3.5 %; whole lines with plain stores +0.5 .. 1.2 %.
constexpr int SLAB_PITCH = 36, SLAB_STAGE = 16 * SLAB_PITCH;
__device__ __forceinline__ void slab_store_tile(const __amdgpu_buffer_rsrc_t rB, float *const stage, const f32x4 (&v)[4], const int m0, const int M,
                                                const unsigned row_b, const unsigned col_b, const int lane) {
  const int fr = lane & 31, fh = lane >> 5, rr = lane >> 3, q = lane & 7;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if ((fr >> 4) == h) {
#pragma unroll
      for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4 *>(stage + (fr & 15) * SLAB_PITCH + 8 * g + 4 * fh) = v[g];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the staging rows are the wave's own: LDS operations of a wave complete in order
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const f32x4 o = *reinterpret_cast<const f32x4 *>(stage + (8 * i + rr) * SLAB_PITCH + 4 * q);
      const int m = m0 + 16 * h + 8 * i + rr;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rB, m < M ? (unsigned)m * row_b + col_b + 16u * q : OOB, 0, /*sc1*/ 16);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// GroupNorm partials of one (clip, group) for the panel prologue are (mean, M2) pairs: pro 1, per statistics chunk of cb_reduce_gn
// (chunk_rows rows x 2^log2cpg channels); pro 2, per 32 x 32 tile segment of the producing GEMM (the tile's rows inside the clip x 32).
// Elements behind partial kc (pro 1) / behind the tile segment of row tile `mtile` (pro 2):
__device__ __forceinline__ float part_count(bool tiles, int clip, int kc, int mtile, int L, int chunk_rows, int log2cpg) {
  const int c0 = clip * L;
  const int rows = tiles ? min((mtile + 1) * 32, c0 + L) - max(mtile * 32, c0) : min(chunk_rows, L - kc * chunk_rows);
  return (float)(rows << (tiles ? 5 : log2cpg));
}

// Chan merge of the partials of one (clip, group): 8 consecutive lanes hold 4 each (partial sub + 8 k, live below lim).  Pooled mean
// first, then M2 = sum (M2_k + n_k (mean_k - mean)^2): no raw sum of squares, so no cancellation at a large mean.  -> (mean, rstd)
__device__ __forceinline__ float2 merge_parts(const float2 (&cs)[4], const float (&cn)[4], int sub, int lim, float rn, float eps) {
  float s1 = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (sub + 8 * k < lim) s1 = fmaf(cn[k], cs[k].x, s1);
  const float mean = sum8_dpp(s1) * rn;
  float s2 = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (sub + 8 * k < lim) {
      const float d = cs[k].x - mean;
      s2 += fmaf(cn[k] * d, d, cs[k].y);
    }
  return make_float2(mean, rsqrtf(sum8_dpp(s2) * rn + eps));
}

// MT = 32-row MFMA tiles per workgroup.  256 threads: wave w owns output columns [32 w, 32 w + 32) of the 128-column block.
// PRO: the GroupNorm+SiLU panel prologue, a compile-time switch (as a run-time branch its loaded values meet "undefined" at the join
// and the compiler's copies put a wait in front of the weight loads).
// Grid: x = weight slice (column block, channel block), y = row tile (rows y >= mtiles: hosted prefetch).  Every division of the index
// arithmetic is a shift (S, channels per group, groups per block are powers of two) or a multiply-high by ceil(2^32 / L) (exact for
// x * L < 2^32): the weight loads are issued ~100 instructions into the kernel, not ~400.
// KB = 128-channel blocks per workgroup (1 or 2): two blocks halve the number of partial slabs (their traffic is what limits the chain at
// 8-16 clips per branch) for twice the weight stream per workgroup (48 fragments per wave).
// EPI = what becomes of the accumulators (kernels.h, ConvCbArgs::epi).  0: fp32 partial slab.  With ONE channel slice (C = N = 128, KB = 1) the
// workgroup holds the full reduction of whole rows, L % 32 == 0 makes every 32-row MFMA tile one statistics chunk of one clip, and the reducer
// launches have nothing left to sum:
//   1 (direct_gn): h = acc + bias -> 16-bit, and the (mean, M2) GroupNorm chunk statistics of the STORED values in the layout pro 1 reads,
//                  chunked and summed exactly as cb_reduce_gn does it (the rounded tile goes through LDS: the panel is free by then).
//   2 (direct_ln): y = acc + bias + residual; row mean, then squares about it, over the four waves through LDS (the panel is free after the
//                  MFMA loop) in cb_reduce_ln's summation order; LayerNorm + Modulation -> 16-bit, the chain's m bit for bit.
// Their operands (bias, residual rows, scale / shift of the tile's clip) are requested behind the weight loads.
template <typename T, int MT, bool PRO, int KB, int EPI = 0>
__global__ __launch_bounds__(256) void conv_cb_kernel(const void *const src, const void *const wimg, const unsigned bytes_src, const int mtiles, const int M,
                                                      const int L, const unsigned magicL, const int src_ld, const int N, const unsigned lg,
                                                      const ConvCbArgs a) {
  // argument head (12 dwords, preloaded into SGPRs with the wave: kernels.h, "argument heads"): what the prefetch test, the tile index, the
  // panel loads and the weight-fragment loads need (lg = log2S | log2cpg << 8).  `a` arrives through scalar loads behind them; the head
  // fields are NOT read from it here.
  const int log2S = (int)(lg & 255u), log2cpg = (int)(lg >> 8);
  using frag = typename Frag16<T>::type;
  using v4 = T __attribute__((ext_vector_type(4)));
  static_assert(EPI == 0 || (KB == 1 && MT <= 2), "direct epilogues: one channel block, at most two row tiles");
  constexpr int KCW = KC * KB, PITCHW = KCW + 8, TPR = KCW / 8, RPP = 256 / TPR;   // channels per workgroup, LDS pitch, threads per row, rows per pass
  constexpr int BM = 32 * MT, PR = BM + 2, NV = (PR + RPP - 1) / RPP;
  __shared__ __attribute__((aligned(16))) T panel[PR * PITCHW];
  __shared__ float2 gstat[NSLOT][8];   // (mean, rstd) per (clip slot, group inside the channel block)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nws = (int)gridDim.x;
  if ((int)blockIdx.y >= mtiles) {   // hosted weight prefetch for the next GEMM of the chain (kernels.h, Prefetch)
    prefetch_slice(a.pf, ((int)blockIdx.y - mtiles) * nws + (int)blockIdx.x, 256);
    return;
  }
  // workgroups that share a weight slice (same x) are nws apart in dispatch order: with nws % 8 == 0 they land on the same XCD
  const int mt = (int)blockIdx.y, ws = (int)blockIdx.x;
  const int nt = ws >> log2S, cb = ws & ((1 << log2S) - 1);
  const int r0 = mt * BM;
  auto divL = [&](int x) { return (int)__umulhi((unsigned)x, magicL); };

  // ---- 1. activation panel: rows r0 - 1 .. r0 + BM of channel block cb (16 threads per row, 16 rows per pass) ----------------
  const __amdgpu_buffer_rsrc_t rS = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(src), 0, bytes_src, 0x00020000);
  const int cv = tid % TPR, pr = tid / TPR;
  Vec16<T> pv[NV];
  const unsigned col_b = (unsigned)((cb * KCW + cv * 8) * sizeof(T)), row_b = (unsigned)(src_ld * sizeof(T));
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int j = pr + RPP * i, r = r0 - 1 + j;
    const bool ok = j < PR && r >= 0 && r < M;
    pv[i] = buf_ld16<T>(rS, ok ? (unsigned)r * row_b + col_b : OOB);
  }
  // ---- 2. GroupNorm operands: gamma / beta of this thread's channel octet, chunk statistics of the clips the panel touches ----------
  //         (8 lanes per (clip, group) pair, 4 chunks each; every address is clamped so that the loads are branch-free and all in
  //         flight together, behind the panel loads and in front of the weight loads: the first wait must not cover the weights)
  const int gshift = KC_LOG2 + (KB == 2 ? 1 : 0) - log2cpg;   // log2(groups inside the workgroup's channel range)
  const int clip0 = divL(max(r0 - 1, 0));
  const int nclip = PRO ? (divL(min(r0 + BM, M - 1)) - clip0 + 1) : 0;
  const int npair = nclip << gshift;                           // <= NSLOT * 8 = 32: one pair per 8 lanes
  f32x4 ga[2], be[2];
  constexpr int NRD = 1;
  float2 cs[NRD][4];
  float cn[NRD][4];   // elements behind each partial (Chan merge weights)
  int lim[NRD] = {0};
  const int sub = tid & 7;
  if constexpr (PRO) {
    const int G = a.C >> log2cpg;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      ga[q] = *reinterpret_cast<const f32x4 *>(a.gamma + cb * KCW + cv * 8 + 4 * q);
      be[q] = *reinterpret_cast<const f32x4 *>(a.beta + cb * KCW + cv * 8 + 4 * q);
    }
    // pro 1: chunk (mean, M2) [clip][nch][G]; pro 2: tile (mean, M2) [m tile][C / 32][segment] of the producing GEMM (kernels.h).  One address
    // select per load instead of two code paths: loaded values that meet at a join cost a wait in front of the weight loads.
    const bool tiles = a.pro == 2;
    const int ltpg = log2cpg - 5, ct = a.C >> 5;               // log2(32-column tiles per group), tiles per row
#pragma unroll
    for (int rd = 0; rd < NRD; ++rd) {
      const int p = min((tid >> 3) + 32 * rd, npair - 1);
      const int slot = p >> gshift, gi = p & ((1 << gshift) - 1);
      const int clip = clip0 + slot;
      const int mt_lo = (clip * L) >> 5, nmt = ((clip * L + L - 1) >> 5) - mt_lo + 1;
      lim[rd] = tiles ? (nmt << max(ltpg, 0)) : a.nch;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int kc = min(sub + 8 * k, lim[rd] - 1);
        const int mtile = mt_lo + (kc >> max(ltpg, 0));
        const int tile = (((cb << gshift) + gi) << max(ltpg, 0)) + (kc & ((1 << max(ltpg, 0)) - 1));
        const unsigned off2 = (unsigned)(((mtile * ct + tile) * 2 + (clip - divL(mtile << 5))) * 2);
        const unsigned off1 = (unsigned)((((clip * a.nch + kc) * G) + (cb << gshift) + gi) * 2);
        cs[rd][k] = *reinterpret_cast<const float2 *>(a.stats + (tiles ? off2 : off1));
        cn[rd][k] = part_count(tiles, clip, kc, mtile, L, a.chunk_rows, log2cpg);
      }
    }
  }
  // ---- 3. the wave's weight slice, fragment order: 24 x 1 KB contiguous, independent of the producer kernel -----------------
  __builtin_amdgcn_sched_barrier(0);   // issue order = wait order (vmcnt counts in issue order): panel, GroupNorm operands, THEN weights
  frag wf[24 * KB];
#pragma unroll
  for (int blk = 0; blk < KB; ++blk) {
    const frag *wp = reinterpret_cast<const frag *>(wimg) + ((size_t)((cb * KB + blk) * (N >> 5) + (nt * 4 + wave)) * 24) * 64;   // uniform
#pragma unroll
    for (int s = 0; s < 24; ++s) wf[blk * 24 + s] = wp[s * 64 + lane];
  }
  __builtin_amdgcn_sched_barrier(0);
  // ---- 3b. operands of the direct epilogues, behind the weights: a lane ends up with columns 32 wave + 8 g + 4 fh + 0..3 (g = 0..3) of row fr
  //          of each tile.  Every address is valid whatever the tile (rows clamped, no Modulation: the bias vector stands in), no branch ----
  const int fr = lane & 31, fh = lane >> 5;
  const int ec0 = wave * 32 + 4 * fh;
  f32x4 eb[4], esc[MT][4], esh[MT][4];
  v4 er[MT][4];
  if constexpr (EPI != 0) {
#pragma unroll
    for (int g = 0; g < 4; ++g) eb[g] = *reinterpret_cast<const f32x4 *>(a.bias + ec0 + 8 * g);
  }
  if constexpr (EPI == 2) {
    const float *ssp = a.ss ? a.ss : a.bias;
    const int sh_off = a.ss ? N : 0;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int m = min(r0 + t * 32 + fr, M - 1);
      const T *rp = static_cast<const T *>(a.res) + (size_t)m * a.res_ld + ec0;
      const float *sp = ssp + (a.ss ? (size_t)divL(min(r0 + t * 32, M - 1)) * a.ss_ld : 0) + ec0;   // the tile lies inside one clip
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        er[t][g] = *reinterpret_cast<const v4 *>(rp + 8 * g);
        esc[t][g] = *reinterpret_cast<const f32x4 *>(sp + 8 * g);
        esh[t][g] = *reinterpret_cast<const f32x4 *>(sp + sh_off + 8 * g);
      }
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  // (the compiler otherwise hoists the first use of a chunk sum in front of the weight loads, and its wait with it)
  if constexpr (PRO) {
#pragma unroll
    for (int rd = 0; rd < NRD; ++rd)
#pragma unroll
      for (int k = 0; k < 4; ++k) asm volatile("" : "+v"(cs[rd][k].x), "+v"(cs[rd][k].y));
  }
  // ---- 4. statistics of the touched (clip, group) pairs -> LDS ----------------------------------------------------------------
  if constexpr (PRO) {
    const float rn = 1.0f / ((float)L * (float)(1 << log2cpg));
#pragma unroll
    for (int rd = 0; rd < NRD; ++rd) {
      const float2 st = merge_parts(cs[rd], cn[rd], sub, lim[rd], rn, a.eps);
      const int p = (tid >> 3) + 32 * rd;
      if (sub == 0 && p < npair) gstat[p >> gshift][p & ((1 << gshift) - 1)] = st;
    }
    __syncthreads();
  }
  // ---- 5. panel -> LDS, GroupNorm + SiLU applied on the way -------------------------------------------------------------------
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int j = pr + RPP * i, r = r0 - 1 + j;
    if (j < PR) {
      Vec16<T> o = pv[i];
      if (PRO && r >= 0 && r < M) {
        const float2 st = gstat[divL(r) - clip0][(cv * 8) >> log2cpg];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float sc = st.y * ga[e >> 2][e & 3];
          const float sh = fmaf(-st.x, sc, be[e >> 2][e & 3]);
          o.set(e, silu_t<true>(fmaf(pv[i].get(e), sc, sh)));
        }
      }
      st16<T>(panel + j * PITCHW + cv * 8, o);
    }
  }
  __syncthreads();
  // ---- 6. D^T[n][m] += W[n][k] * act[m + tap - 1][k]: the weight fragment is the MFMA's A operand, so a lane ends up with four
  //         consecutive output COLUMNS of one row (16-byte slab stores) ---------------------------------------------------------
  bool ok0[MT], ok2[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = r0 + t * 32 + fr, l = m - divL(m) * L;
    ok0[t] = l > 0;              // tap 0 reads position l - 1 of the same clip
    ok2[t] = l < L - 1;        // tap 2 reads position l + 1
  }
  f32x16 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  const frag zf = __builtin_bit_cast(frag, u32x4{0u, 0u, 0u, 0u});
#pragma unroll
  for (int blk = 0; blk < KB; ++blk)
#pragma unroll
    for (int tap = 0; tap < 3; ++tap)
#pragma unroll
      for (int ks = 0; ks < 8; ++ks)
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          frag af = *reinterpret_cast<const frag *>(panel + (t * 32 + fr + tap) * PITCHW + blk * KC + ks * 16 + fh * 8);
          if (tap == 0) af = ok0[t] ? af : zf;
          if (tap == 2) af = ok2[t] ? af : zf;
          acc[t] = mfma32x16(wf[blk * 24 + tap * 8 + ks], af, acc[t]);
        }
  if constexpr (EPI == 0) {
  // ---- 7. partial slab ---------------------------------------------------------------------------------------------------------
  // one resource per workgroup: its own slab (M * N * 4 < 2^31, conv_cb_shape_ok; the S slabs together need not fit 32 bits)
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(a.slab + (size_t)cb * M * N, 0, (unsigned)(M * N) * 4u, 0x00020000);
  static_assert(4 * SLAB_STAGE * sizeof(float) <= PR * PITCHW * sizeof(T), "the four waves' staging rows fit the panel");
  __syncthreads();   // every wave has read its last panel fragment
  float *stage = reinterpret_cast<float *>(panel) + wave * SLAB_STAGE;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    f32x4 v[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) v[g] = f32x4{acc[t][4 * g], acc[t][4 * g + 1], acc[t][4 * g + 2], acc[t][4 * g + 3]};
    slab_store_tile(rB, stage, v, r0 + t * 32, M, (unsigned)N * 4u, (unsigned)(nt * 128 + wave * 32) * 4u, lane);
  }
  } else if constexpr (EPI == 1) {
  // ---- 7a. direct_gn: h = acc + bias -> 16-bit; chunk statistics of the stored values.  M % 32 == 0: a tile is whole or absent.  The rounded
  //          tile goes through LDS (the panel is free) and the statistics are formed by cb_reduce_gn's threads in cb_reduce_gn's order, per chunk
  //          of a.chunk_rows = 8 P rows (cb_gn_plan: 8, 16 or 32, whole chunks per tile): the same bits as the chain's, so the convolution
  //          that merges them sees the same (mean, rstd) ----------------------------------------------------------------------------------
  __syncthreads();   // every wave has read its last panel fragment
  T *tile = panel;                                                  // [BM][128]
  float *red = reinterpret_cast<float *>(panel + BM * 128);         // [4 waves][8 groups][2 passes], then the group means [8]
  float *gmean = red + 64;
  static_assert(BM * 128 * sizeof(T) + 72 * sizeof(float) <= PR * PITCHW * sizeof(T), "tile + reduction scratch fit the panel");
  T *outp = static_cast<T *>(a.out) + ec0;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = r0 + t * 32 + fr;
    const bool live = r0 + t * 32 < M;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      v4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = from_f<T>(acc[t][4 * g + e] + eb[g][e]);
      if (live) *reinterpret_cast<v4 *>(outp + (size_t)m * a.out_ld + 8 * g) = o;
      *reinterpret_cast<v4 *>(tile + (t * 32 + fr) * 128 + ec0 + 8 * g) = o;
    }
  }
  __syncthreads();
  {
    const int R = a.chunk_rows, P = R >> 3;
    const int cq = tid & 31, rr = tid >> 5;            // thread = 4 consecutive columns of one row per pass, as in cb_reduce_gn
    const int cpg = 1 << log2cpg, span = cpg >> 2, gpb = KC >> log2cpg;
    auto group_total = [&](float tt, int k) {
      for (int off = 1; off < span; off <<= 1) tt += __shfl_xor(tt, off, 64);
      tt += __shfl_xor(tt, 32, 64);
      if (lane < 32 && (cq % span) == 0) red[(wave * 8 + cq / span) * 2 + k] = tt;
      __syncthreads();
      float x = 0.f;
      if (tid < gpb) {
#pragma unroll
        for (int w = 0; w < 4; ++w) x += red[(w * 8 + tid) * 2 + k];
      }
      return x;
    };
    for (int ch = 0; ch < BM / R; ++ch) {
      const int m0 = r0 + ch * R;
      float xs[4][4];
      float s1 = 0.f;
#pragma unroll
      for (int pp = 0; pp < 4; ++pp)
        if (pp < P) {
          const v4 v = *reinterpret_cast<const v4 *>(tile + (ch * R + pp * 8 + rr) * 128 + cq * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            xs[pp][e] = to_f(v[e]);
            s1 += xs[pp][e];
          }
        }
      const float a1 = group_total(s1, 0);
      if (tid < gpb) gmean[tid] = a1 / ((float)R * (float)cpg);
      __syncthreads();
      const float mu = gmean[cq / span];
      float s2 = 0.f;
#pragma unroll
      for (int pp = 0; pp < 4; ++pp)
        if (pp < P) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float d = xs[pp][e] - mu;
            s2 = fmaf(d, d, s2);
          }
        }
      const float a2 = group_total(s2, 1);
      if (tid < gpb && m0 < M) {
        const int clip = divL(m0), kc = (m0 - clip * L) / R;
        float *o = a.stats_out + ((size_t)(clip * a.nch + kc) * gpb + tid) * 2;
        o[0] = gmean[tid];
        o[1] = a2;
      }
      __syncthreads();   // red / gmean serve the next chunk
    }
  }
  } else {
  // ---- 7b. direct_ln: y = acc + bias + residual; LayerNorm over the 128 columns of the row (four waves, through LDS), Modulation ------------
  //          The row sums take cb_reduce_ln's order -- a column quad's (y0 + y1) + (y2 + y3), then the 32 quads paired by the bits of the
  //          quad index from the top (wave, then g, then fh) -- so that m is the chain's m bit for bit.  Every lane of a row adds the row's 32
  //          quad sums itself: LDS [pass][row][16-byte slot fh * 4 + wave, XOR row % 8 against bank conflicts][g].
  __syncthreads();   // every wave has read its last panel fragment: the panel's memory carries the quad sums
  float *red = reinterpret_cast<float *>(panel);
  static_assert(2 * BM * 32 * sizeof(float) <= PR * PITCHW * sizeof(T), "the quad sums of both passes fit the panel");
  T *outp = static_cast<T *>(a.out) + ec0;
  const int myslot = (fh * 4 + wave) ^ (fr & 7);
  auto row_total = [&](const float *rowp) {
    float tot[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x4 v[4];
#pragma unroll
      for (int w = 0; w < 4; ++w) v[w] = *reinterpret_cast<const f32x4 *>(rowp + (((h * 4 + w) ^ (fr & 7)) << 2));
      float u[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) u[g] = (v[0][g] + v[2][g]) + (v[1][g] + v[3][g]);
      tot[h] = (u[0] + u[2]) + (u[1] + u[3]);
    }
    return tot[0] + tot[1];
  };
  float y[MT][16];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    f32x4 p;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int e = 0; e < 4; ++e) y[t][4 * g + e] = (acc[t][4 * g + e] + eb[g][e]) + to_f(er[t][g][e]);
      p[g] = (y[t][4 * g] + y[t][4 * g + 1]) + (y[t][4 * g + 2] + y[t][4 * g + 3]);
    }
    *reinterpret_cast<f32x4 *>(red + (t * 32 + fr) * 32 + (myslot << 2)) = p;
  }
  __syncthreads();
  float mean[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    mean[t] = row_total(red + (t * 32 + fr) * 32) / 128.0f;
    f32x4 q;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      q[g] = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = y[t][4 * g + e] - mean[t];
        q[g] = fmaf(d, d, q[g]);
      }
    }
    *reinterpret_cast<f32x4 *>(red + (BM + t * 32 + fr) * 32 + (myslot << 2)) = q;
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = r0 + t * 32 + fr;
    const float rstd = rsqrtf(row_total(red + (BM + t * 32 + fr) * 32) / 128.0f + a.eps_ln);
    if (m < M) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        v4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float z = (y[t][4 * g + e] - mean[t]) * rstd;
          if (a.ss) z = fmaf(z, 1.0f + esc[t][g][e], esh[t][g][e]);
          o[e] = from_f<T>(z);
        }
        *reinterpret_cast<v4 *>(outp + (size_t)m * a.out_ld + 8 * g) = o;
      }
    }
  }
  }
}

// The same workgroup on split fp16 operands (the fp32x engine: fp32 activations in HBM, fp32 partial slabs out).  The panel is fetched as
// fp32 (32 threads per row), GroupNorm+SiLU'd in fp32 and SPLIT ONCE per element on the way into two fp16 LDS images (hi, lo'): every
// fragment the three taps and the four waves read afterwards is a plain 16-byte row read, no vector instruction in the MFMA loop.  The
// weight slice arrives as (hi, lo') fragment pairs, 48 x 1 KB contiguous per wave; three MFMAs per product into two accumulators.
// One 128-channel block per workgroup (the two LDS images of a two-block panel would not fit the static 64 KB).
template <int MT, bool PRO>
__global__ __launch_bounds__(256) void conv_cb_x3_kernel(const void *const src, const void *const wimg, const unsigned bytes_src, const int mtiles, const int M,
                                                         const int L, const unsigned magicL, const int src_ld, const int N, const unsigned lg,
                                                         const ConvCbArgs a) {
  // argument head (12 dwords, preloaded into SGPRs with the wave: kernels.h, "argument heads"): what the prefetch test, the tile index, the
  // panel loads and the weight-fragment loads need (lg = log2S | log2cpg << 8).  `a` arrives through scalar loads behind them; the head
  // fields are NOT read from it here.
  const int log2S = (int)(lg & 255u), log2cpg = (int)(lg >> 8);
  using frag = f16x8;
  constexpr int PITCHW = KC + 8, TPR = KC / 4, RPP = 256 / TPR;   // LDS pitch (fp16 elements), threads per panel row (16 B of fp32 each), rows per pass
  constexpr int BM = 32 * MT, PR = BM + 2, NV = (PR + RPP - 1) / RPP;
  __shared__ __attribute__((aligned(16))) f16 panelH[PR * PITCHW], panelL[PR * PITCHW];
  __shared__ float2 gstat[NSLOT][8];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nws = (int)gridDim.x;
  if ((int)blockIdx.y >= mtiles) {
    prefetch_slice(a.pf, ((int)blockIdx.y - mtiles) * nws + (int)blockIdx.x, 256);
    return;
  }
  const int mt = (int)blockIdx.y, ws = (int)blockIdx.x;
  const int nt = ws >> log2S, cb = ws & ((1 << log2S) - 1);
  const int r0 = mt * BM;
  auto divL = [&](int x) { return (int)__umulhi((unsigned)x, magicL); };

  // ---- 1. activation panel (fp32): rows r0 - 1 .. r0 + BM of channel block cb ----------------------------------------------------------
  const __amdgpu_buffer_rsrc_t rS = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(src), 0, bytes_src, 0x00020000);
  const int cv = tid % TPR, pr = tid / TPR;
  f32x4 pv[NV];
  const unsigned col_b = (unsigned)((cb * KC + cv * 4) * 4), row_b = (unsigned)(src_ld * 4);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int j = pr + RPP * i, r = r0 - 1 + j;
    const bool ok = j < PR && r >= 0 && r < M;
    pv[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rS, ok ? (unsigned)r * row_b + col_b : OOB, 0, 0));
  }
  // ---- 2. GroupNorm operands (as in conv_cb_kernel; this thread owns a channel QUAD) ----------------------------------------------------
  const int gshift = KC_LOG2 - log2cpg;
  const int clip0 = divL(max(r0 - 1, 0));
  const int nclip = PRO ? (divL(min(r0 + BM, M - 1)) - clip0 + 1) : 0;
  const int npair = nclip << gshift;
  f32x4 ga = {1.f, 1.f, 1.f, 1.f}, be = {0.f, 0.f, 0.f, 0.f};
  float2 cs[4];
  float cn[4];
  int lim = 0;
  const int sub = tid & 7;
  if constexpr (PRO) {
    const int G = a.C >> log2cpg;
    ga = *reinterpret_cast<const f32x4 *>(a.gamma + cb * KC + cv * 4);
    be = *reinterpret_cast<const f32x4 *>(a.beta + cb * KC + cv * 4);
    const bool tiles = a.pro == 2;
    const int ltpg = log2cpg - 5, ct = a.C >> 5;
    const int p = min(tid >> 3, npair - 1);
    const int slot = p >> gshift, gi = p & ((1 << gshift) - 1);
    const int clip = clip0 + slot;
    const int mt_lo = (clip * L) >> 5, nmt = ((clip * L + L - 1) >> 5) - mt_lo + 1;
    lim = tiles ? (nmt << max(ltpg, 0)) : a.nch;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int kc = min(sub + 8 * k, lim - 1);
      const int mtile = mt_lo + (kc >> max(ltpg, 0));
      const int tile = (((cb << gshift) + gi) << max(ltpg, 0)) + (kc & ((1 << max(ltpg, 0)) - 1));
      const unsigned off2 = (unsigned)(((mtile * ct + tile) * 2 + (clip - divL(mtile << 5))) * 2);
      const unsigned off1 = (unsigned)((((clip * a.nch + kc) * G) + (cb << gshift) + gi) * 2);
      cs[k] = *reinterpret_cast<const float2 *>(a.stats + (tiles ? off2 : off1));
      cn[k] = part_count(tiles, clip, kc, mtile, L, a.chunk_rows, log2cpg);
    }
  }
  // ---- 3. the wave's weight slice: 24 (hi, lo') fragment pairs, 48 KB contiguous per wave, independent of the producer kernel -----------
  __builtin_amdgcn_sched_barrier(0);
  frag wh[24], wl[24];
  {
    const frag *wp = reinterpret_cast<const frag *>(wimg) + ((size_t)(cb * (N >> 5) + (nt * 4 + wave)) * 48) * 64;   // uniform
#pragma unroll
    for (int s = 0; s < 24; ++s) {
      wh[s] = wp[(2 * s) * 64 + lane];
      wl[s] = wp[(2 * s + 1) * 64 + lane];
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (PRO) {
#pragma unroll
    for (int k = 0; k < 4; ++k) asm volatile("" : "+v"(cs[k].x), "+v"(cs[k].y));
  }
  // ---- 4. statistics of the touched (clip, group) pairs -> LDS ---------------------------------------------------------------------------
  if constexpr (PRO) {
    const float rn = 1.0f / ((float)L * (float)(1 << log2cpg));
    const float2 st = merge_parts(cs, cn, sub, lim, rn, a.eps);
    const int p = tid >> 3;
    if (sub == 0 && p < npair) gstat[p >> gshift][p & ((1 << gshift) - 1)] = st;
    __syncthreads();
  }
  // ---- 5. panel -> LDS: GroupNorm + SiLU in fp32, then split into the two fp16 images ----------------------------------------------------
  typedef f16 f16x4_c __attribute__((ext_vector_type(4)));
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int j = pr + RPP * i, r = r0 - 1 + j;
    if (j < PR) {
      f32x4 o = pv[i];
      if (PRO && r >= 0 && r < M) {
        const float2 st = gstat[divL(r) - clip0][(cv * 4) >> log2cpg];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float sc = st.y * ga[e];
          const float sh = fmaf(-st.x, sc, be[e]);
          o[e] = silu_t<false>(fmaf(pv[i][e], sc, sh));
        }
      }
      f16x4_c h, l;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        f16 x, y;
        x3_split1<X3_F16>(o[e], x, y);
        h[e] = x;
        l[e] = y;
      }
      *reinterpret_cast<f16x4_c *>(panelH + j * PITCHW + cv * 4) = h;
      *reinterpret_cast<f16x4_c *>(panelL + j * PITCHW + cv * 4) = l;
    }
  }
  __syncthreads();
  // ---- 6. D^T[n][m] += W[n][k] * act[m + tap - 1][k] -------------------------------------------------------------------------------------
  const int fr = lane & 31, fh = lane >> 5;
  bool ok0[MT], ok2[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = r0 + t * 32 + fr, l = m - divL(m) * L;
    ok0[t] = l > 0;
    ok2[t] = l < L - 1;
  }
  f32x16 acc[MT], accL[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = accL[t][r] = 0.f;
  const frag zf = __builtin_bit_cast(frag, u32x4{0u, 0u, 0u, 0u});
#pragma unroll
  for (int tap = 0; tap < 3; ++tap)
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const int o = (t * 32 + fr + tap) * PITCHW + ks * 16 + fh * 8;
        frag ah = *reinterpret_cast<const frag *>(panelH + o), al = *reinterpret_cast<const frag *>(panelL + o);
        if (tap == 0) {
          ah = ok0[t] ? ah : zf;
          al = ok0[t] ? al : zf;
        }
        if (tap == 2) {
          ah = ok2[t] ? ah : zf;
          al = ok2[t] ? al : zf;
        }
        x3_mfma<X3_F16>(wh[tap * 8 + ks], wl[tap * 8 + ks], ah, al, acc[t], accL[t]);
      }
  // ---- 7. partial slab --------------------------------------------------------------------------------------------------------------------
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(a.slab + (size_t)cb * M * N, 0, (unsigned)(M * N) * 4u, 0x00020000);
  static_assert(4 * SLAB_STAGE * sizeof(float) <= PR * PITCHW * sizeof(f16), "the four waves' staging rows fit the hi image");
  __syncthreads();   // every wave has read its last panel fragment
  float *stage = reinterpret_cast<float *>(panelH) + wave * SLAB_STAGE;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    f32x4 v[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[g][e] = fmaf(accL[t][4 * g + e], X3P<X3_F16>::INV, acc[t][4 * g + e]);
    slab_store_tile(rB, stage, v, r0 + t * 32, M, (unsigned)N * 4u, (unsigned)(nt * 128 + wave * 32) * 4u, lane);
  }
}

// the same weights as (hi, lo') fragment pairs for conv_cb_x3_kernel: [cb][n / 32][tap][ks][part][lane][8]
__global__ void pack_conv_cb_x3_kernel(const float *__restrict__ w, int N, int C, f16 *__restrict__ out) {
  const size_t total = (size_t)N * C * 3;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int q = (int)(e & 7), lane = (int)((e >> 3) & 63);
    size_t t = e >> 9;
    const int ks = (int)(t & 7);
    t >>= 3;
    const int tap = (int)(t % 3);
    t /= 3;
    const int nt32 = (int)(t % (N / 32)), cb = (int)(t / (N / 32));
    const int n = nt32 * 32 + (lane & 31), c = cb * KC + ks * 16 + (lane >> 5) * 8 + q;
    const size_t pair = (e >> 9) * 1024;   // 512 hi then 512 lo' per (cb, n / 32, tap, ks)
    x3_split1<X3_F16>(w[((size_t)n * C + c) * 3 + tap], out[pair + (e & 511)], out[pair + 512 + (e & 511)]);
  }
}

// Conv1d weight (N, C, 3) fp32 -> fragment order [cb][n / 32][tap][ks][lane][8]:
//   lane holds W[n = 32 * (n / 32) + lane % 32][tap][c = 128 cb + 16 ks + 8 (lane / 32) + 0..7]
template <typename T>
__global__ void pack_conv_cb_kernel(const float *__restrict__ w, int N, int C, T *__restrict__ out) {
  const size_t total = (size_t)N * C * 3;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int q = (int)(e & 7), lane = (int)((e >> 3) & 63);
    size_t t = e >> 9;
    const int ks = (int)(t & 7);
    t >>= 3;
    const int tap = (int)(t % 3);
    t /= 3;
    const int nt32 = (int)(t % (N / 32)), cb = (int)(t / (N / 32));
    const int n = nt32 * 32 + (lane & 31), c = cb * KC + ks * 16 + (lane >> 5) * 8 + q;
    out[e] = from_f<T>(w[((size_t)n * C + c) * 3 + tap]);
  }
}

// slabs -> h = sum + bias (16-bit) and GroupNorm chunk statistics (mean, M2 per (clip, chunk, group)) of the STORED h, in two passes over the
// values the threads keep in registers (raw sums of squares cancel once a group's mean is large next to its spread).  Workgroup = (clip,
// chunk of 8 P rows, 128-column block); thread = 4 consecutive columns of one row per pass.
template <typename T, int S, int P>
__global__ __launch_bounds__(256) void cb_reduce_gn_kernel(const float *__restrict__ slab, const int M, const int N, const int L,
                                                           const float *__restrict__ bias, T *__restrict__ out, const int out_ld, const int G,
                                                           float *__restrict__ stats, const int nch, const int nreal, const Prefetch pf) {
  __shared__ float red[4][8][2];
  __shared__ float gmean[8];
  if ((int)blockIdx.x >= nreal) {
    prefetch_slice(pf, (int)blockIdx.x - nreal, 256);
    return;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ncb = N / 128;
  const int cblk = (int)blockIdx.x % ncb, bc = (int)blockIdx.x / ncb;
  const int b = bc / nch, ch = bc - b * nch;
  const int cq = tid & 31, rr = tid >> 5;
  const int c = cblk * 128 + cq * 4;
  const int l0 = ch * 8 * P, rows = min(8 * P, L - l0);
  f32x4 v[P][S];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int lr = p * 8 + rr;
    const size_t m = (size_t)b * L + l0 + min(lr, rows - 1);
#pragma unroll
    for (int s = 0; s < S; ++s) v[p][s] = *reinterpret_cast<const f32x4 *>(slab + ((size_t)s * M + m) * N + c);
  }
  const f32x4 bi = *reinterpret_cast<const f32x4 *>(bias + c);
  float xs[P][4];   // the stored values (rows past the chunk: 0, and left out of both passes)
  float s1 = 0.f;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int lr = p * 8 + rr;
    f32x4 x = v[p][0];
#pragma unroll
    for (int s = 1; s < S; ++s) x += v[p][s];   // fixed order: deterministic
    x += bi;
    T o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[e] = from_f<T>(x[e]);
      xs[p][e] = lr < rows ? to_f(o[e]) : 0.f;
      s1 += xs[p][e];
    }
    if (lr < rows) __builtin_memcpy(__builtin_assume_aligned(out + ((size_t)b * L + l0 + lr) * out_ld + c, 4 * sizeof(T)), o, 4 * sizeof(T));
  }
  // group totals: lanes of one group are `span` consecutive channel quads; lane ^ 32 is the same quad one row further.  Fixed shapes: deterministic
  const int cpg = N / G, span = cpg / 4;   // 4 .. 32
  const int gpb = 128 / cpg;
  auto group_total = [&](float t, int k) {
    for (int off = 1; off < span; off <<= 1) t += __shfl_xor(t, off, 64);
    t += __shfl_xor(t, 32, 64);
    if (lane < 32 && (cq % span) == 0) red[wave][cq / span][k] = t;
    __syncthreads();
    float a = 0.f;
    if (tid < gpb) {
#pragma unroll
      for (int w = 0; w < 4; ++w) a += red[w][tid][k];
    }
    return a;
  };
  // pass 1: the chunk's group means
  const float a1 = group_total(s1, 0);
  if (tid < gpb) gmean[tid] = a1 / ((float)rows * (float)cpg);
  __syncthreads();
  // pass 2: squares about them
  const float mu = gmean[cq / span];
  float s2 = 0.f;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const bool live = p * 8 + rr < rows;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = live ? xs[p][e] - mu : 0.f;
      s2 = fmaf(d, d, s2);
    }
  }
  const float a2 = group_total(s2, 1);
  if (tid < gpb) {
    float *o = stats + (((size_t)b * nch + ch) * G + cblk * gpb + tid) * 2;   // (mean, M2) of the chunk: the consumer merges the chunks (Chan)
    o[0] = gmean[tid];
    o[1] = a2;
  }
}

// slabs + bias + residual -> y (fp32, never stored);  m = LayerNorm_C(y; eps) * (1 + ss[b][c]) + ss[b][C + c]  -> out (16-bit).
// TPR = C / 4 threads per row (32 .. 256), 256 / TPR rows per workgroup.
template <typename T, int S, int TPR>
__global__ __launch_bounds__(256) void cb_reduce_ln_kernel(const float *__restrict__ slab, const int M, const int C, const int L,
                                                           const float *__restrict__ bias, const T *__restrict__ res, const int res_ld,
                                                           const float *__restrict__ ss, const int ss_ld, const float eps, T *__restrict__ out,
                                                           const int out_ld, const int nreal, const Prefetch pf) {
  constexpr int RPB = 256 / TPR, WPR = TPR >= 64 ? TPR / 64 : 1;   // rows per workgroup, waves per row
  __shared__ float red[2][4];
  if ((int)blockIdx.x >= nreal) {
    prefetch_slice(pf, (int)blockIdx.x - nreal, 256);
    return;
  }
  const int tid = threadIdx.x, wave = tid >> 6;
  const int row = (int)blockIdx.x * RPB + tid / TPR, sub = tid % TPR;
  const bool active = row < M;
  const size_t m = active ? row : 0;
  const int c = sub * 4, b = (int)(m / L);
  f32x4 v[S];
#pragma unroll
  for (int s = 0; s < S; ++s) v[s] = *reinterpret_cast<const f32x4 *>(slab + ((size_t)s * M + m) * C + c);
  T rv[4];
  __builtin_memcpy(rv, __builtin_assume_aligned(res + m * res_ld + c, 4 * sizeof(T)), 4 * sizeof(T));
  const f32x4 bi = *reinterpret_cast<const f32x4 *>(bias + c);
  f32x4 sc = {0.f, 0.f, 0.f, 0.f}, sh = {0.f, 0.f, 0.f, 0.f};
  if (ss) {
    sc = *reinterpret_cast<const f32x4 *>(ss + (size_t)b * ss_ld + c);
    sh = *reinterpret_cast<const f32x4 *>(ss + (size_t)b * ss_ld + C + c);
  }
  f32x4 y = v[0];
#pragma unroll
  for (int s = 1; s < S; ++s) y += v[s];
  y += bi;
#pragma unroll
  for (int e = 0; e < 4; ++e) y[e] += to_f(rv[e]);
  auto row_sum = [&](float x, int slot) {
    constexpr int W = TPR < 64 ? TPR : 64;
#pragma unroll
    for (int o = W >> 1; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if constexpr (WPR > 1) {
      if ((tid & 63) == 0) red[slot][wave] = x;
      __syncthreads();
      const int w0 = (wave / WPR) * WPR;
      x = 0.f;
#pragma unroll
      for (int w = 0; w < WPR; ++w) x += red[slot][w0 + w];
    }
    return x;
  };
  const float mean = row_sum((y[0] + y[1]) + (y[2] + y[3]), 0) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float d = y[e] - mean;
    q = fmaf(d, d, q);
  }
  const float rstd = rsqrtf(row_sum(q, 1) / (float)C + eps);
  if (!active) return;
  T o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float z = (y[e] - mean) * rstd;
    if (ss) z = fmaf(z, 1.0f + sc[e], sh[e]);
    o[e] = from_f<T>(z);
  }
  __builtin_memcpy(__builtin_assume_aligned(out + (size_t)row * out_ld + c, 4 * sizeof(T)), o, 4 * sizeof(T));
}

int cb_min_wgs() {
  static const int v = [] {   // tuning hook: fewest workgroups a launch should have when choosing the rows per workgroup
    const char *e = tune_env("SF_CB_MIN_WGS");
    return e && atoi(e) > 0 ? atoi(e) : 160;
  }();
  return v;
}

}  // namespace

size_t conv_cb_weight_elems(int N, int C) { return (size_t)N * C * 3; }

bool conv_cb_shape_ok(int dt, int B, int L, int C, int N, int G) {
  if (dt == F32) return false;   // (F32X: the split-operand form)
  if (C < KC || (C % KC) || (N % 128) || C / KC > 8 || ((C / KC) & (C / KC - 1))) return false;
  if (L < 44 || (int64_t)B * L * (int64_t)(C > N ? C : N) * 4 >= 0x7FFFFFF0ll) return false;   // a 130-row panel touches <= NSLOT clips
  if ((uint64_t)B * L * (uint64_t)L >= (1ull << 32)) return false;   // row / L by multiply-high (magicL) is exact only while row * L < 2^32
  if (G > 0) {
    if (C % G) return false;
    const int cpg = C / G;
    if (cpg < 16 || cpg > KC || (cpg & (cpg - 1))) return false;
  }
  return true;
}

// pro 2 (GroupNorm statistics per 32 x 32 tile of the producing GEMM): a group must be whole tiles, a (clip, group) at most 32 of them
bool conv_cb_tile_stats_ok(int L, int C, int G) {
  if (G < 1 || C % G) return false;
  const int cpg = C / G;
  if (cpg < 32 || (cpg & (cpg - 1)) || L < 32) return false;
  return ((L + 30) / 32 + 1) * (cpg / 32) <= 32;
}

// the direct epilogues (ConvCbArgs::epi): one channel slice and whole rows per workgroup, a 32-row MFMA tile = one statistics chunk inside one clip
bool conv_cb_direct_ok(int dt, int B, int L, int C, int N, int G) {
  if (dt != BF16 && dt != F16) return false;
  if (C != KC || N != KC || (L % 32) || L / 32 > 32) return false;
  return conv_cb_shape_ok(dt, B, L, C, N, G);
}

// Measured alone on the chip (tools/cb_bench.py, profiles/r4_a_cb_bench.txt; HBM-cold weights, us per launch, MT = 1 / 2 / 3 / 4):
//   d7 (176 rows, C 1024): 6.7 / 6.4 / 8.2 / 8.6     d6 (352 rows): 8.9 / 8.5 / 9.2 / 9.3     d5 (704 rows, C 512): 6.0 / 6.1 / 7.8 / 8.2
//   d4 (1408 rows, C 256): 4.0 / 5.1 / 6.8 / 7.1   (88 workgroups at MT = 2)
// 96- and 128-row panels hold 1 wave per SIMD (184-258 registers) and serialise a longer prologue: two tiles where that still
// gives >= 160 workgroups, else one.
int conv_cb_mt(int M, int N, int C) {
  static const int forced = [] {
    const char *e = tune_env("SF_CB_MT");
    return e ? atoi(e) : 0;
  }();
  if (forced >= 1 && forced <= 4) return forced;
  const int nws = (N / 128) * (C / KC);
  return ((M + 63) / 64) * nws >= cb_min_wgs() ? 2 : 1;
}

hipError_t launch_pack_conv_cb(int dt, const float *w, int N, int C, void *out, hipStream_t s) {
  if (dt == F32 || (C % KC) || (N % 32)) return hipErrorInvalidValue;
  const size_t total = (size_t)N * C * 3;
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
  if (dt == F32X) hipLaunchKernelGGL(pack_conv_cb_x3_kernel, dim3(blocks), dim3(256), 0, s, w, N, C, static_cast<f16 *>(out));
  else if (dt == BF16) hipLaunchKernelGGL((pack_conv_cb_kernel<bf16>), dim3(blocks), dim3(256), 0, s, w, N, C, static_cast<bf16 *>(out));
  else hipLaunchKernelGGL((pack_conv_cb_kernel<f16>), dim3(blocks), dim3(256), 0, s, w, N, C, static_cast<f16 *>(out));
  return hipGetLastError();
}

namespace {
// The one launch site of the conv_cb kernels: the argument head (kernels.h, "argument heads") is built here, in the kernels' parameter order
template <typename Kern> void launch_cb_head(Kern kern, const ConvCbArgs &a, dim3 grid, int mtiles, unsigned bytes_src, hipStream_t s) {
  const void *const src = a.src, *const wimg = a.wp;
  const int M = a.B * a.L, L = a.L, src_ld = a.src_ld, N = a.N;
  const unsigned magicL = a.magicL, lg = (unsigned)a.log2S | ((unsigned)a.log2cpg << 8);
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, src, wimg, bytes_src, mtiles, M, L, magicL, src_ld, N, lg, a);
}
}  // namespace

hipError_t launch_conv_cb(int dt, const ConvCbArgs &a0, hipStream_t s) {
  if (!conv_cb_shape_ok(dt, a0.B, a0.L, a0.C, a0.N, a0.pro ? a0.G : 0)) return hipErrorInvalidValue;
  if (a0.pro == 1 && a0.nch > 32) return hipErrorInvalidValue;
  if (a0.pro == 2 && !conv_cb_tile_stats_ok(a0.L, a0.C, a0.G)) return hipErrorInvalidValue;
  ConvCbArgs a = a0;
  if (dt == F32X && a.kb == 2) return hipErrorInvalidValue;   // one channel block per workgroup in the split-operand form
  if (a.epi) {
    // direct_gn after a materialised GroupNorm+SiLU (pro 0), direct_ln behind the chunk statistics it left (pro 1): the two instantiated forms
    if (!((a.epi == 1 && a.pro == 0) || (a.epi == 2 && a.pro == 1)) || a.kb == 2) return hipErrorInvalidValue;
    if (!conv_cb_direct_ok(dt, a.B, a.L, a.C, a.N, a.G) || a.G < 1) return hipErrorInvalidValue;
    if (!a.out || !a.bias || (a.out_ld % 4) || a.out_ld < a.N) return hipErrorInvalidValue;
    if (a.epi == 1 && !a.stats_out) return hipErrorInvalidValue;
    if (a.epi == 2 && (!a.res || (a.res_ld % 4) || a.res_ld < a.N)) return hipErrorInvalidValue;
    if (a.epi == 2 && a.ss && ((a.ss_ld % 4) || (reinterpret_cast<uintptr_t>(a.ss) % 16))) return hipErrorInvalidValue;
    // statistics chunks (written by epi 1, read by pro 1): whole chunks of 8, 16 or 32 rows per tile, cb_gn_plan's choice
    if ((a.chunk_rows != 8 && a.chunk_rows != 16 && a.chunk_rows != 32) || a.nch * a.chunk_rows != a.L || a.nch > 32) return hipErrorInvalidValue;
  }
  const int kb = a.kb == 2 ? 2 : 1;
  const int M = a.B * a.L, S = a.C / KC / kb;   // partial slabs = workgroups along the input channels
  if (kb == 2 && ((a.C / KC) % 2 || (a.pro && a.C / a.G < 32))) return hipErrorInvalidValue;   // <= 8 groups inside a 256-channel range
  a.log2S = 0;
  while ((1 << a.log2S) < S) ++a.log2S;
  const int cpg = (a.pro || a.epi == 1) ? a.C / a.G : KC;   // (direct_gn without prologue: the groups of its OUTPUT, N = C)
  a.log2cpg = 0;
  while ((1 << a.log2cpg) < cpg) ++a.log2cpg;
  if ((1 << a.log2S) != S || (1 << a.log2cpg) != cpg) return hipErrorInvalidValue;
  a.magicL = (unsigned)((0x100000000ull + (unsigned)a.L - 1) / (unsigned)a.L);   // x / L == mulhi(x, magicL) while x * L < 2^32
  int mt = kb == 2 ? std::min(2, conv_cb_mt(M, a.N, a.C / 2)) : conv_cb_mt(M, a.N, a.C);
  if (dt == F32X || a.epi) mt = std::min(mt, 2);
  const int mtiles = (M + 32 * mt - 1) / (32 * mt), nws = (a.N / 128) * S;
  const int pf_rows = (a.pf.ptr && a.pf.bytes >= 16 && a.pf.wgs > 0) ? (a.pf.wgs + nws - 1) / nws : 0;
  a.pf.wgs = pf_rows * nws;
  const dim3 grid(nws, mtiles + pf_rows);
  const unsigned bytes_src = (unsigned)((size_t)M * a.src_ld * dsize(dt));
  if (dt == F32X) {
    if (a.pro) {
      if (mt == 1) launch_cb_head(conv_cb_x3_kernel<1, true>, a, grid, mtiles, bytes_src, s);
      else launch_cb_head(conv_cb_x3_kernel<2, true>, a, grid, mtiles, bytes_src, s);
    } else {
      if (mt == 1) launch_cb_head(conv_cb_x3_kernel<1, false>, a, grid, mtiles, bytes_src, s);
      else launch_cb_head(conv_cb_x3_kernel<2, false>, a, grid, mtiles, bytes_src, s);
    }
    return hipGetLastError();
  }
  if (a.epi) {
#define SF_CBD(T, MT)                                                                                                          \
  do {                                                                                                                         \
    if (a.epi == 1) launch_cb_head(conv_cb_kernel<T, MT, false, 1, 1>, a, grid, mtiles, bytes_src, s);     \
    else launch_cb_head(conv_cb_kernel<T, MT, true, 1, 2>, a, grid, mtiles, bytes_src, s);                 \
  } while (0)
    if (dt == BF16) {
      if (mt == 1) SF_CBD(bf16, 1);
      else SF_CBD(bf16, 2);
    } else {
      if (mt == 1) SF_CBD(f16, 1);
      else SF_CBD(f16, 2);
    }
#undef SF_CBD
    return hipGetLastError();
  }
#define SF_CB2(T, MT, KB_)                                                                                                \
  do {                                                                                                                    \
    if (a.pro) launch_cb_head(conv_cb_kernel<T, MT, true, KB_>, a, grid, mtiles, bytes_src, s);       \
    else launch_cb_head(conv_cb_kernel<T, MT, false, KB_>, a, grid, mtiles, bytes_src, s);            \
  } while (0)
#define SF_CB(T, MT)                 \
  do {                               \
    if (kb == 2) SF_CB2(T, MT, 2);   \
    else SF_CB2(T, MT, 1);           \
  } while (0)
#define SF_CB_T(T)            \
  switch (mt) {               \
    case 1: SF_CB(T, 1); break; \
    case 2: SF_CB(T, 2); break; \
    case 3: if (kb == 2) { SF_CB2(T, 2, 2); } else { SF_CB2(T, 3, 1); } break; \
    default: if (kb == 2) { SF_CB2(T, 2, 2); } else { SF_CB2(T, 4, 1); } break; \
  }
  if (dt == BF16) { SF_CB_T(bf16) } else { SF_CB_T(f16) }
#undef SF_CB_T
#undef SF_CB
#undef SF_CB2
  return hipGetLastError();
}

// rows per statistics chunk of cb_reduce_gn: 8 P with the fewest passes that keep the chunk count within the 32 the consumers merge
CbGnPlan cb_gn_plan(int L) {
  CbGnPlan p;
  int P = 1;
  while (P < 4 && (L + 8 * P - 1) / (8 * P) > 32) P *= 2;
  p.chunk_rows = 8 * P;
  p.nch = (L + p.chunk_rows - 1) / p.chunk_rows;
  return p;
}

hipError_t launch_cb_reduce_gn(int dt, const float *slab, int S, int B, int L, int N, const float *bias, void *out, int out_ld, int G, float *stats,
                               const CbGnPlan &gp, hipStream_t s, Prefetch pf) {
  if ((N % 128) || N % G || (N / G) < 16 || (N / G) > 128 || (128 % (N / G)) || gp.nch > 32 || (out_ld % 4)) return hipErrorInvalidValue;
  const int P = gp.chunk_rows / 8, M = B * L;
  const int nreal = B * gp.nch * (N / 128);
  const dim3 grid(nreal + (pf.ptr && pf.bytes >= 16 ? pf.wgs : 0));
#define SF_RG(T, S_, P_)                                                                                                                          \
  hipLaunchKernelGGL((cb_reduce_gn_kernel<T, S_, P_>), grid, dim3(256), 0, s, slab, M, N, L, bias, static_cast<T *>(out), out_ld, G, stats, gp.nch, \
                     nreal, pf)
#define SF_RG_P(T, S_)            \
  switch (P) {                    \
    case 1: SF_RG(T, S_, 1); break; \
    case 2: SF_RG(T, S_, 2); break; \
    case 4: SF_RG(T, S_, 4); break; \
    default: return hipErrorInvalidValue; \
  }
#define SF_RG_S(T)                \
  switch (S) {                    \
    case 1: SF_RG_P(T, 1) break;  \
    case 2: SF_RG_P(T, 2) break;  \
    case 4: SF_RG_P(T, 4) break;  \
    case 8: SF_RG_P(T, 8) break;  \
    default: return hipErrorInvalidValue; \
  }
  if (dt == BF16) { SF_RG_S(bf16) } else if (dt == F16) { SF_RG_S(f16) } else { SF_RG_S(float) }   // float: the fp32x engine's chain
#undef SF_RG_S
#undef SF_RG_P
#undef SF_RG
  return hipGetLastError();
}

hipError_t launch_cb_reduce_ln(int dt, const float *slab, int S, int B, int L, int C, const float *bias, const void *res, int res_ld, const float *ss,
                               int ss_ld, float eps, void *out, int out_ld, hipStream_t s, Prefetch pf) {
  const int tpr = C / 4;
  if ((C % 128) || (tpr != 32 && tpr != 64 && tpr != 128 && tpr != 256) || (res_ld % 4) || (out_ld % 4)) return hipErrorInvalidValue;
  if (ss && ((ss_ld % 4) || (reinterpret_cast<uintptr_t>(ss) % 16))) return hipErrorInvalidValue;
  const int M = B * L, rpb = 256 / tpr;
  const int nreal = (M + rpb - 1) / rpb;
  const dim3 grid(nreal + (pf.ptr && pf.bytes >= 16 ? pf.wgs : 0));
#define SF_RL(T, S_, TPR_)                                                                                                                     \
  hipLaunchKernelGGL((cb_reduce_ln_kernel<T, S_, TPR_>), grid, dim3(256), 0, s, slab, M, C, L, bias, static_cast<const T *>(res), res_ld, ss, ss_ld, \
                     eps, static_cast<T *>(out), out_ld, nreal, pf)
#define SF_RL_T(T, S_)               \
  switch (tpr) {                     \
    case 32: SF_RL(T, S_, 32); break;  \
    case 64: SF_RL(T, S_, 64); break;  \
    case 128: SF_RL(T, S_, 128); break; \
    default: SF_RL(T, S_, 256); break; \
  }
#define SF_RL_S(T)                 \
  switch (S) {                     \
    case 1: SF_RL_T(T, 1) break;   \
    case 2: SF_RL_T(T, 2) break;   \
    case 4: SF_RL_T(T, 4) break;   \
    case 8: SF_RL_T(T, 8) break;   \
    default: return hipErrorInvalidValue; \
  }
  if (dt == BF16) { SF_RL_S(bf16) } else if (dt == F16) { SF_RL_S(f16) } else { SF_RL_S(float) }
#undef SF_RL_S
#undef SF_RL_T
#undef SF_RL
  return hipGetLastError();
}

}  // namespace sf
