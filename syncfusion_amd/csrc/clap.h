// Device pieces of the CLAP audio embedder (HTSAT: a Swin transformer on a log-mel "image") beside the implicit-GEMM launcher: shifted-window
// attention and the row LayerNorm of widths 3 * 2^k (swin.hip), the spectrogram -> image -> patch-token front and the embedding tail
// (clap_front.hip); and of the text embedder (RoBERTa: embedding gather, affine LayerNorm, masked attention, pooler tail; clap_text.hip).
// Shared by the kernels and the engines / C ABI (clap_engine.cpp, clap_text_engine.cpp).  fp32 data, on the caller's stream, no allocation,
// fixed-order reductions (no atomics): a clip's or a text's rows never depend on the rest of the batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sf {

constexpr int SWIN_WINDOW = 8;      // the only window the attention kernel implements (64 tokens = one wave, one lane per query)
constexpr int SWIN_MAX_HEAD_DIM = 32;

// qkv (B H W, 3 C) rows in raster order, columns [q | k | v] each (heads, D) -> out (B H W, C): softmax(q k^T D^-1/2 + bias + mask) v inside
// 8 x 8 windows of the map rolled by (-shift, -shift); window partition, roll and their inverses are index arithmetic.  bias_table
// ((2 * 8 - 1)^2, heads).  D = C / heads in {4, 8, ..., 32}; H, W multiples of 8; shift 0 or 4 (0 when H or W is 8) -- the caller checks.
hipError_t launch_window_attention(const float *qkv, int B, int H, int W, int C, int heads, int shift, const float *bias_table, float mask_value,
                                   float *out, hipStream_t s);
// y[m][:] = (x[src(m)][:] - mean) * rstd over C columns, two passes, one wave per row; no affine (the engine folds it into the next weights).
// merge == 0: rows in, rows out (src(m) = m).  merge == 1 (PatchMerging): the output row (b, h2, w2) of a (B, H / 2, W / 2) map has 4 C
// columns, segment q = tokens (2 h2 + (q & 1), 2 w2 + (q >> 1)) of the (B, H, W) input, normalised over all 4 C.
hipError_t launch_swin_layernorm(const float *x, int64_t rows_out, int C, float eps, int merge, int H, int W, float *y, hipStream_t s);

// mel power (B, n_mels, T) -> image (B, S, S), S = n_mels * ratio: v[f][t] = fma(10 log10(max(P, amin)), scale[f], shift[f]) (P <= amin gives
// db_floor, the host's 10 log10(amin)), bicubic along time to S * ratio frames when T is shorter (A = -0.75, align_corners, clamped
// borders; T == S * ratio copies), folded: image[r n_mels + f][t'] = v[f][r S + t'].
hipError_t launch_logmel_image(const float *mel, int B, int n_mels, int T, int ratio, const float *scale, const float *shift, float amin,
                               float db_floor, float *image, hipStream_t s);
// image (B, S, S) -> tokens (B (S / 4)^2, E) in raster order: Conv2d(1, E, 4, 4) + bias, then LayerNorm(E) with its affine.  w (E, 16), E <= 256
hipError_t launch_patch_embed(const float *image, int B, int S, int E, const float *w, const float *bias, const float *gamma, const float *beta,
                              float eps, float *tokens, hipStream_t s);
// x (B, ntok, C) -> embedding (B, J): LayerNorm(C; gamma, beta), mean over the tokens, Linear(C, J) [ReLU] Linear(J, J) [L2 normalise]; four
// launches.  scratch: B (C + 2 J) floats.  C <= 1024, J <= 1024, ntok <= 256
hipError_t launch_clap_tail(const float *x, int B, int ntok, int C, int J, const float *gamma, const float *beta, float eps, const float *w1,
                            const float *b1, const float *w2, const float *b2, int relu, int normalize, float *scratch, float *out, hipStream_t s);
// the pieces of that tail the text embedder shares.  y[b][:] = act(W x[b x_ld + :] + bias) for a handful of rows: one wave per output, K <= 1024
enum { CLAP_ACT_NONE = 0, CLAP_ACT_RELU = 1, CLAP_ACT_TANH = 2 };
hipError_t launch_clap_linear(const float *x, int64_t x_ld, int B, int K, int N, const float *w, const float *bias, int act, float *y, hipStream_t s);
// pooled (B, C) -> Linear(C, J) [ReLU] -> hid (B, J) -> Linear(J, J) -> emb (B, J) -> [L2 normalise] -> out (B, J); three launches
hipError_t launch_clap_projection(const float *pooled, int B, int C, int J, const float *w1, const float *b1, int relu, const float *w2,
                                  const float *b2, int normalize, float *hid, float *emb, float *out, hipStream_t s);

// ---- the text branch (RoBERTa; clap_text.hip, clap_text_engine.cpp) -------------------------------------------------------------------------
constexpr int TEXT_HEAD_DIM = 64;     // the only head dim the attention kernel implements (one output dimension per lane)
constexpr int TEXT_MAX_S = 128;       // K and V of one (text, head) in LDS: 2 * 128 * 64 floats = 64 KB
constexpr int TEXT_MAX_C = 1024;      // row kernels keep a row in one wave's registers: C a multiple of 64 up to here

// ids (B, S) int32 -> out (B S, C): LayerNorm_C(word[id] + pos[p] + type[0]; gamma, beta), one wave per token row, two-pass statistics.
// p = pad_id + (count of ids != pad_id in the row up to and including this column) for a real token, pad_id for a pad.  id and p are clamped
// into their tables (vocab, n_pos rows): memory safety only, the caller has validated them.
hipError_t launch_text_embed(const int32_t *ids, int B, int S, int C, int vocab, int n_pos, int pad_id, const float *word, const float *pos,
                             const float *type, const float *gamma, const float *beta, float eps, float *out, hipStream_t s);
// y[m][:] = (x[m][:] - mean) * rstd * gamma + beta over C columns, two passes, one wave per row
hipError_t launch_layernorm_affine(const float *x, int64_t rows, int C, const float *gamma, const float *beta, float eps, float *y, hipStream_t s);
// qkv (B S, 3 C) rows, columns [q | k | v] each (heads, 64), C = 64 heads; mask (B, S) int32, non-zero = a real token -> out (B S, C):
// softmax(q k^T / 8) v over the keys the mask admits.  A masked key carries weight exactly 0 and its K / V rows never enter the arithmetic;
// masked QUERY rows are computed like any other; a text whose mask admits no key gives zeros.  1 <= S <= 128.
hipError_t launch_masked_attention(const float *qkv, const int32_t *mask, int B, int S, int heads, float *out, hipStream_t s);
// x (B S, C) -> embedding (B, J): pooler (tanh(Linear(C, C)) of row b S; pooler == 0: that row as it is), Linear(C, J) [ReLU], Linear(J, J),
// [L2 normalise].  scratch: B (C + 2 J) floats; its first B C floats hold the pooled rows afterwards.  C, J <= 1024
hipError_t launch_text_tail(const float *x, int B, int S, int C, int J, int pooler, const float *pool_w, const float *pool_b, const float *w1,
                            const float *b1, int relu, const float *w2, const float *b2, int normalize, float *scratch, float *out, hipStream_t s);

}  // namespace sf
