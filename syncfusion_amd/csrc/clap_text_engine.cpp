// CLAP text embedder behind the C ABI (replaces laion_clap.CLAP_Module(...).get_text_embedding, main/module_diffusion.py:69-71): RoBERTa's
// embeddings, its post-LN encoder layers, the pooler and the two-layer projection on token ids.  fp32 throughout.  The fused q/k/v projection,
// the attention output (+ residual), the intermediate Linear (+ GELU) and the output Linear (+ residual) run on the implicit-GEMM launcher;
// the LayerNorms behind the two residual adds keep their affine (clap_text.hip).  Weights are copied once at create time; the forward call
// allocates nothing.  Also the C entry points of the stand-alone pieces.
#include <algorithm>
#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "clap.h"
#include "engine_common.h"

using namespace sf;

namespace {

struct LayerW {
  float *qkv_w = nullptr, *qkv_b = nullptr, *ao_w = nullptr, *ao_b = nullptr, *ln1_g = nullptr, *ln1_b = nullptr;
  float *fc1_w = nullptr, *fc1_b = nullptr, *fc2_w = nullptr, *fc2_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
};

void check_config(const sf_clap_text_config &c) {
  if (c.layers < 1 || c.layers > 64) fail(SF_ERR_INVALID, "layers %d outside 1 .. 64", c.layers);
  if (c.vocab_size < 1 || c.max_positions < 1 || c.heads < 1 || c.intermediate < 1) fail(SF_ERR_INVALID, "vocab_size, max_positions, heads, intermediate >= 1 expected");
  if (c.pad_id < 0 || c.pad_id >= c.vocab_size) fail(SF_ERR_INVALID, "pad_id %d outside the vocabulary", c.pad_id);
  if (c.max_length < 1) fail(SF_ERR_INVALID, "max_length must be at least 1");
  if (!(c.ln_eps > 0.f)) fail(SF_ERR_INVALID, "ln_eps must be positive");
  if (c.pooling != 0 && c.pooling != 1) fail(SF_ERR_INVALID, "pooling %d: 0 (pooler) or 1 (cls)", c.pooling);
  if (c.hidden != TEXT_HEAD_DIM * c.heads) fail(SF_ERR_UNSUPPORTED, "head dim %d / %d: only %d is built", c.hidden, c.heads, TEXT_HEAD_DIM);
  if (c.hidden > TEXT_MAX_C) fail(SF_ERR_UNSUPPORTED, "hidden %d: a multiple of 64 up to %d is built", c.hidden, TEXT_MAX_C);
  if (c.max_length > TEXT_MAX_S) fail(SF_ERR_UNSUPPORTED, "max_length %d: at most %d tokens are built", c.max_length, TEXT_MAX_S);
  if (c.max_length + c.pad_id + 1 > c.max_positions)
    fail(SF_ERR_SHAPE, "max_length %d needs %d position rows, the table has %d", c.max_length, c.max_length + c.pad_id + 1, c.max_positions);
  if (c.joint_dim < 1 || c.joint_dim > 1024) fail(SF_ERR_SHAPE, "joint_dim %d outside 1 .. 1024", c.joint_dim);
  if (c.intermediate > 16384) fail(SF_ERR_SHAPE, "intermediate %d above 16384", c.intermediate);
}

// S against the engine's limits (the config has been checked)
void check_length(const sf_clap_text_config &c, int S) {
  if (S > TEXT_MAX_S) fail(SF_ERR_UNSUPPORTED, "S = %d: at most %d tokens are built", S, TEXT_MAX_S);
  if (S > c.max_length) fail(SF_ERR_SHAPE, "S = %d exceeds max_length %d", S, c.max_length);
  if (S + c.pad_id + 1 > c.max_positions) fail(SF_ERR_SHAPE, "S = %d needs %d position rows, the table has %d", S, S + c.pad_id + 1, c.max_positions);
}

// the GEMMs of one layer at B texts of S tokens
std::vector<LinearDesc> gemms_of(const sf_clap_text_config &c, int B, int S) {
  const int C = c.hidden, I = c.intermediate;
  return {{"qkv", B, S, C, 3 * C, 0, false}, {"attention output", B, S, C, C, 0, true}, {"intermediate", B, S, C, I, 2, false},
          {"output", B, S, I, C, 0, true}};
}

// the widest activation (the intermediate rows, or q | k | v) stays below 2^31 bytes: the GEMM kernels' 32-bit offsets
int64_t max_rows(const sf_clap_text_config &c) { return 0x7FFFFFF0ll / ((int64_t)std::max(c.intermediate, 3 * c.hidden) * 4); }

// X | X1 (normalised rows: each layer's input and the rows between its halves) | T (rows before a LayerNorm) | A (attention output) | QKV |
// HID | the tail's pooled, hidden and raw rows
int64_t ws_bytes_for(const sf_clap_text_config &c, int B, int S) {
  const int64_t unit = (int64_t)B * S * c.hidden * 4;
  return 4 * align_up(unit, 256) + align_up(3 * unit, 256) + align_up((int64_t)B * S * c.intermediate * 4, 256) +
         align_up((int64_t)B * (c.hidden + 2 * c.joint_dim) * 4, 256);
}

}  // namespace

struct sf_clap_text {
  sf_clap_text_config cfg;
  DeviceArena arena;
  std::vector<LayerW> layers;
  float *word = nullptr, *pos = nullptr, *type = nullptr, *emb_g = nullptr, *emb_b = nullptr;
  float *pool_w = nullptr, *pool_b = nullptr, *p0_w = nullptr, *p0_b = nullptr, *p2_w = nullptr, *p2_b = nullptr;
};

extern "C" {

int sf_clap_text_create(const sf_clap_text_config *cfg, const sf_tensor *weights, int n_weights, void *stream, sf_clap_text **out) {
  SF_API_BEGIN
  if (!cfg || !weights || !out) fail(SF_ERR_INVALID, "null argument");
  *out = nullptr;
  if (n_weights < 1) fail(SF_ERR_INVALID, "no weights");
  const sf_clap_text_config c = *cfg;
  check_config(c);
  const WeightMap wm(weights, n_weights);
  WeightWants ww;
  auto eng = std::unique_ptr<sf_clap_text>(new sf_clap_text());
  eng->cfg = c;
  const int64_t C = c.hidden, I = c.intermediate, J = c.joint_dim;
  ww.want("emb.word", (int64_t)c.vocab_size * C, &eng->word);
  ww.want("emb.pos", (int64_t)c.max_positions * C, &eng->pos);
  ww.want("emb.type", C, &eng->type);
  ww.want("emb.g", C, &eng->emb_g);
  ww.want("emb.beta", C, &eng->emb_b);
  eng->layers.resize(c.layers);
  for (int i = 0; i < c.layers; ++i) {
    LayerW &l = eng->layers[i];
    const std::string p = "l" + std::to_string(i) + ".";
    ww.want(p + "qkv.w", 3 * C * C, &l.qkv_w);
    ww.want(p + "qkv.b", 3 * C, &l.qkv_b);
    ww.want(p + "ao.w", C * C, &l.ao_w);
    ww.want(p + "ao.b", C, &l.ao_b);
    ww.want(p + "ln1.g", C, &l.ln1_g);
    ww.want(p + "ln1.beta", C, &l.ln1_b);
    ww.want(p + "fc1.w", I * C, &l.fc1_w);
    ww.want(p + "fc1.b", I, &l.fc1_b);
    ww.want(p + "fc2.w", C * I, &l.fc2_w);
    ww.want(p + "fc2.b", C, &l.fc2_b);
    ww.want(p + "ln2.g", C, &l.ln2_g);
    ww.want(p + "ln2.beta", C, &l.ln2_b);
  }
  if (c.pooling == 0) {
    ww.want("pool.w", C * C, &eng->pool_w);
    ww.want("pool.b", C, &eng->pool_b);
  }
  ww.want("proj0.w", J * C, &eng->p0_w);
  ww.want("proj0.b", J, &eng->p0_b);
  ww.want("proj2.w", J * J, &eng->p2_w);
  ww.want("proj2.b", J, &eng->p2_b);
  hipStream_t s = static_cast<hipStream_t>(stream);
  ww.load(wm, eng->arena, s);   // refuses a missing or mis-sized name before the first HIP call
  SF_HIP(hipStreamSynchronize(s));
  *out = eng.release();
  return SF_OK;
  SF_API_END
}

void sf_clap_text_destroy(sf_clap_text *h) { delete h; }

int64_t sf_clap_text_workspace_bytes(const sf_clap_text *h, int B, int S) {
  if (!h || B < 1 || S < 1 || S > TEXT_MAX_S || S > h->cfg.max_length || (int64_t)B * S > max_rows(h->cfg)) return -1;
  return ws_bytes_for(h->cfg, B, S);
}

int sf_clap_text_describe(const sf_clap_text_config *cfg, int B, int S, char *text, int64_t capacity) {
  SF_API_BEGIN
  if (!cfg || !text || capacity < 1) fail(SF_ERR_INVALID, "null argument");
  if (B < 1 || S < 1) fail(SF_ERR_INVALID, "B and S must be at least 1");
  check_config(*cfg);
  check_length(*cfg, S);
  if ((int64_t)B * S > max_rows(*cfg)) fail(SF_ERR_SHAPE, "at most %lld token rows per call", (long long)max_rows(*cfg));
  describe_gemms(gemms_of(*cfg, B, S), " (x " + std::to_string(cfg->layers) + " layers)", text, capacity);
  return SF_OK;
  SF_API_END
}

int sf_clap_text_forward(sf_clap_text *h, const int32_t *ids, const int32_t *mask, int B, int S, float *embedding, float *const *taps, void *ws,
                         int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!h || !ids || !mask || !embedding) fail(SF_ERR_INVALID, "null argument");
  if (B < 1 || S < 1) fail(SF_ERR_INVALID, "B and S must be at least 1");
  const sf_clap_text_config &c = h->cfg;
  check_length(c, S);
  if ((int64_t)B * S > max_rows(c)) fail(SF_ERR_SHAPE, "at most %lld token rows per call", (long long)max_rows(c));
  require_workspace(ws, ws_bytes, ws_bytes_for(c, B, S));
  require_gemm_kernels(gemms_of(c, B, S));
  hipStream_t s = static_cast<hipStream_t>(stream);
  Workspace wsp(ws, ws_bytes);
  const int C = c.hidden, I = c.intermediate;
  const int64_t M = (int64_t)B * S, unit = M * C;
  float *x = wsp.alloc_n<float>(unit), *x1 = wsp.alloc_n<float>(unit), *t = wsp.alloc_n<float>(unit), *att = wsp.alloc_n<float>(unit);
  float *qkv = wsp.alloc_n<float>(3 * unit), *hid = wsp.alloc_n<float>(M * I);
  float *tail = wsp.alloc_n<float>((int64_t)B * (C + 2 * c.joint_dim));
  SF_HIP(launch_text_embed(ids, B, S, C, c.vocab_size, c.max_positions, c.pad_id, h->word, h->pos, h->type, h->emb_g, h->emb_b, c.ln_eps, x, s));
  copy_tap(taps, 0, x, unit, s);
  for (int i = 0; i < c.layers; ++i) {
    const LayerW &l = h->layers[i];
    SF_HIP(launch_conv_gemm(F32, token_linear_args(x, B, S, C, 3 * C, l.qkv_w, l.qkv_b, nullptr, 0, qkv), s));
    SF_HIP(launch_masked_attention(qkv, mask, B, S, c.heads, att, s));
    SF_HIP(launch_conv_gemm(F32, token_linear_args(att, B, S, C, C, l.ao_w, l.ao_b, x, 0, t), s));
    SF_HIP(launch_layernorm_affine(t, M, C, l.ln1_g, l.ln1_b, c.ln_eps, x1, s));
    SF_HIP(launch_conv_gemm(F32, token_linear_args(x1, B, S, C, I, l.fc1_w, l.fc1_b, nullptr, 2, hid), s));
    SF_HIP(launch_conv_gemm(F32, token_linear_args(hid, B, S, I, C, l.fc2_w, l.fc2_b, x1, 0, t), s));
    SF_HIP(launch_layernorm_affine(t, M, C, l.ln2_g, l.ln2_b, c.ln_eps, x, s));
    copy_tap(taps, i + 1, x, unit, s);
  }
  SF_HIP(launch_text_tail(x, B, S, C, c.joint_dim, c.pooling == 0, h->pool_w, h->pool_b, h->p0_w, h->p0_b, c.projection_relu, h->p2_w, h->p2_b,
                          c.normalize, tail, embedding, s));
  copy_tap(taps, c.layers + 1, tail, (int64_t)B * C, s);
  return SF_OK;
  SF_API_END
}

int sf_op_text_embed(const int32_t *ids, int B, int S, int C, int vocab, int n_pos, int pad_id, const float *word, const float *pos, const float *type,
                     const float *gamma, const float *beta, float eps, float *out, void *stream) {
  SF_API_BEGIN
  if (!ids || !word || !pos || !type || !gamma || !beta || !out) fail(SF_ERR_INVALID, "null argument");
  if (B < 1 || S < 1 || vocab < 1 || n_pos < 1) fail(SF_ERR_INVALID, "B, S, vocab, n_pos >= 1 expected");
  if (!(eps > 0.f)) fail(SF_ERR_INVALID, "eps must be positive");
  if (C < 64 || (C % 64) || C > TEXT_MAX_C) fail(SF_ERR_UNSUPPORTED, "C = %d: a multiple of 64 up to %d is built", C, TEXT_MAX_C);
  if ((int64_t)B * S * C >= (1ll << 31)) fail(SF_ERR_SHAPE, "tensor too large");
  SF_HIP(launch_text_embed(ids, B, S, C, vocab, n_pos, pad_id, word, pos, type, gamma, beta, eps, out, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_layernorm_affine(const float *x, int64_t rows, int C, const float *gamma, const float *beta, float eps, float *y, void *stream) {
  SF_API_BEGIN
  if (!x || !gamma || !beta || !y) fail(SF_ERR_INVALID, "null argument");
  if (rows < 1) fail(SF_ERR_INVALID, "rows must be at least 1");
  if (!(eps > 0.f)) fail(SF_ERR_INVALID, "eps must be positive");
  if (C < 64 || (C % 64) || C > TEXT_MAX_C) fail(SF_ERR_UNSUPPORTED, "C = %d: a multiple of 64 up to %d is built", C, TEXT_MAX_C);
  if (rows * C >= (1ll << 31)) fail(SF_ERR_SHAPE, "tensor too large");
  SF_HIP(launch_layernorm_affine(x, rows, C, gamma, beta, eps, y, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_masked_attention(const float *qkv, const int32_t *mask, int B, int S, int heads, float *out, void *stream) {
  SF_API_BEGIN
  if (!qkv || !mask || !out) fail(SF_ERR_INVALID, "null argument");
  if (B < 1 || S < 1 || heads < 1) fail(SF_ERR_INVALID, "B, S, heads >= 1 expected");
  if (S > TEXT_MAX_S) fail(SF_ERR_UNSUPPORTED, "S = %d: at most %d tokens are built", S, TEXT_MAX_S);
  if ((int64_t)B * S * 3 * heads * TEXT_HEAD_DIM >= (1ll << 31) || (int64_t)B * heads >= (1ll << 31)) fail(SF_ERR_SHAPE, "tensor too large");
  SF_HIP(launch_masked_attention(qkv, mask, B, S, heads, out, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

}  // extern "C"
