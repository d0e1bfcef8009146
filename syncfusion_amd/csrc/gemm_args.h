// Builders for the argument block of the implicit-GEMM launcher (ConvGemmArgs, kernels.h).  A builder sets the fields every site of its
// kind shares and nothing else: what differs between sites (residual, act, solo, rows per item, padded row lengths) is a parameter or an
// assignment behind the call, where the reader of the site sees it.  solo, Lout and Lsrc feed conv_gemm_plan, so they choose the kernel.
#pragma once
#include "kernels.h"

namespace sf {
#pragma GCC visibility push(hidden)   // internal to the library: no new exported symbols

// A Linear on rows: out[rows][N] = src[rows][K] * w[N][K]^T (+ bias).  Dense rows on both sides (src_ld = K, out_ld = n_store = N).
inline ConvGemmArgs linear_args(const void *src, int rows, int K, int N, const void *w, const float *bias, void *out) {
  ConvGemmArgs a;
  a.src = src;
  a.src_ld = K;
  a.w = w;
  a.bias = bias;
  a.N = N;
  a.K = K;
  a.cin = K;
  a.M = rows;
  a.out = out;
  a.out_ld = N;
  a.n_store = N;
  return a;
}

// The Linear of the token engines (CLAP audio and text): B items of `tokens` rows each, an optional residual of the output's shape, and
// nothing running beside the launch.
inline ConvGemmArgs token_linear_args(const void *src, int B, int tokens, int K, int N, const void *w, const float *bias, const void *res, int act,
                                      void *out) {
  ConvGemmArgs a = linear_args(src, B * tokens, K, N, w, bias, out);
  a.Lout = a.Lsrc = tokens;
  a.res = res;
  a.res_ld = N;
  a.act = act;
  a.solo = 1;
  return a;
}

// A video convolution on channels-last rows ((n * T + t) * H + h) * W + w: NT * Ho * Wo output rows of g.cout channels from rows of cin_ld
// columns, K = the packed weights' row length.  Temporal stride 1.  Bias, residual, act, n_store and solo stay with the caller.
inline ConvGemmArgs vconv_args(const VConvGeom &g, int64_t NT, const void *src, int cin_ld, const void *w, int K, void *out, int cout_ld) {
  ConvGemmArgs a;
  a.geom = 1;
  a.src = src;
  a.src_ld = cin_ld;
  a.w = w;
  a.N = g.cout;
  a.K = K;
  a.cin = cin_ld;
  a.taps = g.taps();
  a.M = (int)(NT * g.Ho * g.Wo);
  a.To = a.Ti = g.T;
  a.Ho = g.Ho, a.Wo = g.Wo, a.Hi = g.Hi, a.Wi = g.Wi;
  a.kt = g.kt, a.kh = g.kh, a.kw = g.kw;
  a.st = 1, a.sh = g.sh, a.sw = g.sw;
  a.pt = g.pt, a.ph = g.ph, a.pw = g.pw;
  a.out = out;
  a.out_ld = cout_ld;
  a.Lout = a.Lsrc = 1;
  return a;
}

// The launch geometry the wave-split-K kernels share (conv_gemm_sk / _fast / _wp / _rs, 1-D rows): BM x BN tiles over M x n_store, the XCD
// swizzle of the block -> tile map (gemm_epilogue.h, tile_of_block), the byte lengths of the three buffer descriptors (es = bytes per
// element, cat = a second source is read) and the grid with the hosted prefetch workgroups behind the tiles (kernels.h, Prefetch; a kernel
// that hosts none launches tiles() workgroups).
struct GemmTiling {
  int mtiles, ntiles, swz;
  unsigned bytesA, bytesA2, bytesW, grid;
  unsigned tiles() const { return (unsigned)(mtiles * ntiles); }
};
inline GemmTiling gemm_tiling(const ConvGemmArgs &a, int BM, int BN, size_t es, bool cat) {
  GemmTiling t;
  t.mtiles = (a.M + BM - 1) / BM;
  t.ntiles = (a.n_store + BN - 1) / BN;
  t.swz = (t.ntiles % 8 == 0) ? 1 : 0;
  t.bytesA = (unsigned)((size_t)(a.M / a.Lout + (a.M % a.Lout ? 1 : 0)) * a.Lsrc * a.src_ld * es);
  t.bytesA2 = cat ? (unsigned)((size_t)a.M * a.src2_ld * es) : 0u;
  t.bytesW = (unsigned)((size_t)a.N * a.K * es);
  t.grid = t.tiles() + (a.pf.ptr && a.pf.bytes >= 16 ? a.pf.wgs : 0);
  return t;
}
// every buffer a 1-D launch reads through a 32-bit descriptor offset stays below 2 GiB (the OOB bit of common.h lies beyond it)
inline bool gemm_buffers_below_2g(int dt, const ConvGemmArgs &a) {
  const size_t es = dsize(dt), lim = 0x7FFFFFF0ull;
  if ((size_t)(a.M / a.Lout + 1) * a.Lsrc * a.src_ld * es >= lim) return false;
  if ((size_t)a.M * (a.src2_ld > 0 ? a.src2_ld : 1) * es >= lim) return false;
  if ((size_t)a.N * a.K * es >= lim) return false;
  return true;
}

#pragma GCC visibility pop
}  // namespace sf
