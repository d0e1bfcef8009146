// The back half of the small-batch implicit-GEMM kernels (conv_gemm_sk / _fast / _wp / _rs, and conv_gemm_v2's single-tile form), in pieces:
// a kernel calls the pieces it uses, in its own order, and keeps what is its own (operand loaders, K loops, where its epilogue operands and
// LayerNorm partials are loaded, its output stores).  Nothing here branches on its caller.
//
// THE ONE PLACE that defines the bits of ConvGemmArgs::rowpart_out, gnpart_out and of the accumulator-side LayerNorm (ln_colsum): every
// summation order, fmaf and clamp below is a contract with the consumers named in kernels.h (conv_cb prologue 2, the LayerNorm-consumer
// GEMMs) -- a change here changes all producers together, which is the point.
#pragma once
#include "common.h"
#include "kernels.h"

namespace sf {

// ---- block id -> (row tile, column tile) ----------------------------------------------------------------------------------------------
// swz (ntiles % 8 == 0): XCD x (= bid % 8 under round-robin dispatch) owns the column tiles == x (mod 8), so all row tiles of one W panel
// share an L2.  (conv_gemm_rs computes the same map with one division and no branch in front of its first loads.)
__device__ __forceinline__ void tile_of_block(int bid, int mtiles, int swz, int &mt, int &nt) {
  if (swz) {
    const int xcd = bid & 7, j = bid >> 3;
    nt = xcd + 8 * (j / mtiles);
    mt = j % mtiles;
  } else {
    nt = bid / mtiles;
    mt = bid % mtiles;
  }
}

// ---- one staged K chunk: fragment reads + MFMAs ----------------------------------------------------------------------------------------
// As / Bs: LDS rows of LD elements; this wave multiplies the KW-deep slice that starts at element kw0 into its TM x TN tiles of 32x32.
// 16-bit: v_mfma_f32_32x32x16 on 8 consecutive k per lane; fp32: v_mfma_f32_32x32x2_f32, the two k of a step are {s, KW / 2 + s} of the
// slice (the same permutation for A and W).
template <typename T, int TM, int TN, int KW>
__device__ __forceinline__ void mma_chunk(const T *As, const T *Bs, int LD, int kw0, int fr, int fh, f32x16 (&acc)[TM][TN]) {
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int s = 0; s < KW / 16; ++s) {
      using frag = typename Frag16<T>::type;
      frag af[TM], bfr[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const frag *>(As + (i * 32 + fr) * LD + kw0 + 16 * s + 8 * fh);
#pragma unroll
      for (int j = 0; j < TN; ++j) bfr[j] = *reinterpret_cast<const frag *>(Bs + (j * 32 + fr) * LD + kw0 + 16 * s + 8 * fh);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mfma32x16(af[i], bfr[j], acc[i][j]);
    }
  } else {
#pragma unroll
    for (int q = 0; q < KW / 8; ++q) {
      f32x4 af[TM], bfr[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const f32x4 *>(As + (i * 32 + fr) * LD + kw0 + (KW / 2) * fh + 4 * q);
#pragma unroll
      for (int j = 0; j < TN; ++j) bfr[j] = *reinterpret_cast<const f32x4 *>(Bs + (j * 32 + fr) * LD + kw0 + (KW / 2) * fh + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bfr[j][e], acc[i][j], 0, 0, 0);
    }
  }
}

// ---- accumulators -> a row-major fp32 tile in LDS --------------------------------------------------------------------------------------
// Register r of lane (fr, fh) of a 32x32 accumulator is row (r & 3) + 8 (r >> 2) + 4 fh, column fr.  `tile` points at the tile's first
// float (a wave's partial tile, or conv_gemm_v2's wave offset inside the block tile); LDR = row pitch in floats.
// (conv_gemm_rs writes the same mapping out for its one tile: through this function its split forms allocate 2-4 registers more)
template <int LDR> __device__ __forceinline__ void acc32_to_lds(float *tile, int fr, int fh, const f32x16 acc) {
#pragma unroll
  for (int r = 0; r < 16; ++r) tile[((r & 3) + 8 * (r >> 2) + 4 * fh) * LDR + fr] = acc[r];
}
template <int LDR, int TM, int TN> __device__ __forceinline__ void acc_to_lds(float *tile, int fr, int fh, const f32x16 (&acc)[TM][TN]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc32_to_lds<LDR>(tile + i * 32 * LDR + j * 32, fr, fh, acc[i][j]);
}
// split mode X3 (common.h): the stored value is acc + accL / SCALE
template <int LDR, int X3, int TM, int TN>
__device__ __forceinline__ void acc_split_to_lds(float *tile, int fr, int fh, const f32x16 (&acc)[TM][TN], const f32x16 (&accL)[TM][TN]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      f32x16 t;
#pragma unroll
      for (int r = 0; r < 16; ++r) t[r] = fmaf(accL[i][j][r], X3P<X3>::INV, acc[i][j][r]);
      acc32_to_lds<LDR>(tile + i * 32 * LDR + j * 32, fr, fh, t);
    }
}

// ---- the four wave partials of one row quad, summed in the fixed order w = 0, 1, 2, 3 (deterministic) -----------------------------------
// red: four partial tiles of BM rows, LDR floats apart; row ml (< BM), column quad nq
template <int BM, int LDR> __device__ __forceinline__ f32x4 sum4_partials(const float *red, int ml, int nq) {
  f32x4 v = *reinterpret_cast<const f32x4 *>(red + (size_t)ml * LDR + nq * 4);
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const f32x4 t = *reinterpret_cast<const f32x4 *>(red + ((size_t)w * BM + ml) * LDR + nq * 4);
    v[0] += t[0];
    v[1] += t[1];
    v[2] += t[2];
    v[3] += t[3];
  }
  return v;
}

// ---- epilogue operands of one row quad (row m, columns nb .. nb + 3) -------------------------------------------------------------------
// Loads are unconditional from clamped (always mapped) addresses, so that all of them are in flight together; an absent operand is its
// neutral value.  cu = ln_colsum (accumulator-side LayerNorm), read only when the caller's launch can carry it.
// (conv_gemm_rs loads the same operands with branch-free buffer loads behind its operand stream and feeds the pieces below from them.)
struct EpiOps {
  float bi[4], rv[4], sv[4], av[4], cu[4];
};
template <typename T> __device__ __forceinline__ EpiOps epi_load(const ConvGemmArgs &a, int m, int nb, bool ln_epi) {
  EpiOps o;
  const T *res = static_cast<const T *>(a.res);
  const bool has_res = res != nullptr, has_bs = a.bscale != nullptr, has_ba = a.badd != nullptr;
  const int mc = min(m, a.M - 1);
  const int b = (has_bs || has_ba) ? mc / a.Lout : 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int nc = min(nb + e, a.N - 1);
    o.bi[e] = a.bias ? a.bias[nc] : 0.f;
    o.rv[e] = has_res ? to_f(res[(size_t)mc * a.res_ld + nc]) : 0.f;
    o.sv[e] = has_bs ? a.bscale[(size_t)b * a.bscale_ld + nc] : 1.f;
    o.av[e] = has_ba ? a.badd[(size_t)b * a.badd_ld + nc] : 0.f;
    o.cu[e] = ln_epi ? a.ln_colsum[nc] : 0.f;
  }
  return o;
}

// ---- accumulator-side LayerNorm (ConvGemmArgs::ln_colsum) -------------------------------------------------------------------------------
// Row statistics pooled from the producer's per-tile partials (rowpart_out of the launch before: (mean, M2) per 32 channels).  Eight
// consecutive lanes t8 = 0 .. 7 serve one row; lane t8 holds partials t8 + 8 j (zeros past ln_nt) and passes `sm`, the sum of its mp[] --
// the ORDER of that sum is the caller's (conv_gemm_fast adds 0 + mp[0] + mp[1] + mp[2] + mp[3] in sequence, conv_gemm_wp and conv_gemm_rs
// add (mp[0] + mp[1]) + (mp[2] + mp[3]); the two round differently and each kernel keeps its own).  Returns (mean, rstd) in every lane.
__device__ __forceinline__ float2 ln_pool_row(float sm, const float (&mp)[4], const float (&qp)[4], int t8, int ln_nt, int cin, float eps) {
  const float mean = sum8_dpp(sm) / (float)ln_nt;   // every partial covers 32 channels
  float dq = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (t8 + 8 * j < ln_nt) {
      const float d = mp[j] - mean;
      dq += fmaf(32.f * d, d, qp[j]);
    }
  const float m2 = sum8_dpp(dq);
  return make_float2(mean, rsqrtf(m2 / (float)cin + eps));
}
// LayerNorm of the raw source folded into the accumulator: rstd_m * (acc[m][n] - mean_m * colsum(W)_n)
__device__ __forceinline__ void ln_fold(f32x4 &v, float mu, float rstd, const float (&cu)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = rstd * (v[e] - mu * cu[e]);
}

// ---- the value of one row quad ----------------------------------------------------------------------------------------------------------
// x = act((v + bias) * bscale + res + badd), zero beyond N; xo = x as the output will hold it (rounded to T unless out_f32): what the
// statistics below are taken of
template <typename T>
__device__ __forceinline__ void epi_values(const ConvGemmArgs &a, const f32x4 v, const float *bi, const float *sv, const float *rv, const float *av, int nb,
                                           float (&x)[4], float (&xo)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float y = (v[e] + bi[e]) * sv[e] + rv[e] + av[e];
    x[e] = nb + e < a.N ? apply_act(y, a.act) : 0.f;
    xo[e] = a.out_f32 ? x[e] : to_f(from_f<T>(x[e]));
  }
}
// element-wise store of the quad (row m < M and quad inside n_store: `live`)
template <typename T> __device__ __forceinline__ void epi_store(const ConvGemmArgs &a, int m, int nb, bool live, const float (&x)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int n = nb + e;
    if (live && n < a.n_store) {
      if (a.out_f32) static_cast<float *>(a.out)[(size_t)m * a.out_ld + n] = x[e];
      else static_cast<T *>(a.out)[(size_t)m * a.out_ld + n] = from_f<T>(x[e]);
    }
  }
}

// ---- statistics of the stored values (32-column tiles, one row = 8 consecutive lanes with 4 values each) ---------------------------------
// (mean, M2) of a row's 32 stored values, in every lane of the row: rowpart_out's entry, and the rows gnpart_out is pooled from
__device__ __forceinline__ float2 row32_stats(const float (&xo)[4]) {
  const float mean = sum8_dpp((xo[0] + xo[1]) + (xo[2] + xo[3])) * (1.0f / 32.0f);
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float d = xo[e] - mean;
    q = fmaf(d, d, q);
  }
  return make_float2(mean, sum8_dpp(q));
}
// gnpart_out of one 32-row x 32-column tile (mt, nt) of `ntiles` column tiles: every thread of the workgroup calls it with its row's
// statistics `rs` (row ml of the tile, lane nq of the row's eight); gsum = 64 floats of LDS.  Segment 0: the rows of the first row's clip;
// segment 1: the rows of the next clip (Lout >= 32: a tile touches at most two).  Fixed order: deterministic.
__device__ __forceinline__ void gn_tile_stats(const ConvGemmArgs &a, float *gsum, const float2 rs, int tid, int ml, int nq, int m0, int mt, int nt, int ntiles) {
  if (nq == 0) {
    gsum[2 * ml] = rs.x;
    gsum[2 * ml + 1] = rs.y;
  }
  __syncthreads();
  if (tid < 2) {
    const int rb = min((m0 / a.Lout + 1) * a.Lout - m0, 32);
    const int lo = tid == 0 ? 0 : rb, hi = tid == 0 ? rb : min(32, a.M - m0);   // rows past M belong to no clip
    // the segment's (mean, M2) from its rows' (32 values each, row order), in one pass about the first row's mean p:
    // d_r = mean_r - p,  mean = p + sum d / k,  M2 = sum (M2_r + 32 d_r^2) - 32 (sum d)^2 / k.  (0, 0) when empty
    const float p = hi > lo ? gsum[2 * lo] : 0.f;
    float t1 = 0.f, t2 = 0.f;
    for (int r = lo; r < hi; ++r) {
      const float d = gsum[2 * r] - p;
      t1 += d;
      t2 += fmaf(32.f * d, d, gsum[2 * r + 1]);
    }
    const float dk = hi > lo ? t1 / (float)(hi - lo) : 0.f;
    t2 = fmaxf(fmaf(-32.f * t1, dk, t2), 0.f);
    t1 = p + dk;
    *reinterpret_cast<float2 *>(a.gnpart_out + (((size_t)mt * ntiles + nt) * 2 + tid) * 2) = make_float2(t1, t2);
  }
}

}  // namespace sf
