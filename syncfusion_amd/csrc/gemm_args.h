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

#pragma GCC visibility pop
}  // namespace sf
