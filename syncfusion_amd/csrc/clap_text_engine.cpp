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

#define SF_API_BEGIN try {
#define SF_API_END                  \
  }                                 \
  catch (const EngineError &e) {    \
    return e.code;                  \
  }                                 \
  catch (const std::exception &e) { \
    set_error("%s", e.what());      \
    return SF_ERR_INVALID;          \
  }

namespace {

struct LayerW {
  float *qkv_w = nullptr, *qkv_b = nullptr, *ao_w = nullptr, *ao_b = nullptr, *ln1_g = nullptr, *ln1_b = nullptr;
  float *fc1_w = nullptr, *fc1_b = nullptr, *fc2_w = nullptr, *fc2_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
};

// one GEMM of a layer on S rows per text
struct Gemm {
  const char *name;
  int K, N, act;
  bool res;
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

std::vector<Gemm> gemms_of(const sf_clap_text_config &c) {
  const int C = c.hidden, I = c.intermediate;
  return {{"qkv", C, 3 * C, 0, false}, {"attention output", C, C, 0, true}, {"intermediate", C, I, 2, false}, {"output", I, C, 0, true}};
}

ConvGemmArgs lin(const float *src, int B, int S, int K, int N, const float *w, const float *bias, const float *res, int act, float *out) {
  ConvGemmArgs a;
  a.src = src;
  a.src_ld = K;
  a.w = w;
  a.bias = bias;
  a.N = N;
  a.K = K;
  a.cin = K;
  a.taps = 1;
  a.M = B * S;
  a.Lout = a.Lsrc = S;
  a.out = out;
  a.out_ld = N;
  a.n_store = N;
  a.res = res;
  a.res_ld = N;
  a.act = act;
  a.solo = 1;
  return a;
}

// what the plan needs is whether a pointer is set, not where it points
alignas(16) float g_some[4];
ConvGemmPlan plan_of(const Gemm &g, int B, int S) {
  return conv_gemm_plan(F32, lin(g_some, B, S, g.K, g.N, g_some, g_some, g.res ? g_some : nullptr, g.act, g_some));
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
  // every name and size is looked up before anything is allocated or copied: refusals come before the first HIP call
  struct Want {
    std::string name;
    int64_t n;
    float **dst;
  };
  std::vector<Want> want;
  auto eng = std::unique_ptr<sf_clap_text>(new sf_clap_text());
  eng->cfg = c;
  const int64_t C = c.hidden, I = c.intermediate, J = c.joint_dim;
  want.push_back({"emb.word", (int64_t)c.vocab_size * C, &eng->word});
  want.push_back({"emb.pos", (int64_t)c.max_positions * C, &eng->pos});
  want.push_back({"emb.type", C, &eng->type});
  want.push_back({"emb.g", C, &eng->emb_g});
  want.push_back({"emb.beta", C, &eng->emb_b});
  eng->layers.resize(c.layers);
  for (int i = 0; i < c.layers; ++i) {
    LayerW &l = eng->layers[i];
    const std::string p = "l" + std::to_string(i) + ".";
    want.push_back({p + "qkv.w", 3 * C * C, &l.qkv_w});
    want.push_back({p + "qkv.b", 3 * C, &l.qkv_b});
    want.push_back({p + "ao.w", C * C, &l.ao_w});
    want.push_back({p + "ao.b", C, &l.ao_b});
    want.push_back({p + "ln1.g", C, &l.ln1_g});
    want.push_back({p + "ln1.beta", C, &l.ln1_b});
    want.push_back({p + "fc1.w", I * C, &l.fc1_w});
    want.push_back({p + "fc1.b", I, &l.fc1_b});
    want.push_back({p + "fc2.w", C * I, &l.fc2_w});
    want.push_back({p + "fc2.b", C, &l.fc2_b});
    want.push_back({p + "ln2.g", C, &l.ln2_g});
    want.push_back({p + "ln2.beta", C, &l.ln2_b});
  }
  if (c.pooling == 0) {
    want.push_back({"pool.w", C * C, &eng->pool_w});
    want.push_back({"pool.b", C, &eng->pool_b});
  }
  want.push_back({"proj0.w", J * C, &eng->p0_w});
  want.push_back({"proj0.b", J, &eng->p0_b});
  want.push_back({"proj2.w", J * J, &eng->p2_w});
  want.push_back({"proj2.b", J, &eng->p2_b});
  for (const Want &w : want) (void)wm.get(w.name, w.n);

  hipStream_t s = static_cast<hipStream_t>(stream);
  for (const Want &w : want) {
    *w.dst = eng->arena.alloc_n<float>(w.n);
    SF_HIP(hipMemcpyAsync(*w.dst, wm.get(w.name, w.n), (size_t)w.n * 4, hipMemcpyDeviceToDevice, s));
  }
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
  std::string s;
  for (const Gemm &g : gemms_of(*cfg)) {
    char line[256];
    snprintf(line, sizeof line, "%s (x %d layers): M %lld N %d K %d -> %s\n", g.name, cfg->layers, (long long)B * S, g.N, g.K, plan_of(g, B, S).label);
    s += line;
  }
  if ((int64_t)s.size() + 1 > capacity) fail(SF_ERR_INVALID, "text capacity %lld below %lld", (long long)capacity, (long long)s.size() + 1);
  memcpy(text, s.c_str(), s.size() + 1);
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
  const int64_t need = ws_bytes_for(c, B, S);
  if (!ws || ws_bytes < need) fail(SF_ERR_WORKSPACE, "workspace too small: need %lld bytes", (long long)need);
  for (const Gemm &g : gemms_of(c))
    if (plan_of(g, B, S).family == CG_INVALID)
      fail(SF_ERR_UNSUPPORTED, "%s (M %lld, N %d, K %d): no GEMM kernel takes the shape", g.name, (long long)B * S, g.N, g.K);
  hipStream_t s = static_cast<hipStream_t>(stream);
  Workspace wsp(ws, ws_bytes);
  const int C = c.hidden, I = c.intermediate;
  const int64_t M = (int64_t)B * S, unit = M * C;
  float *x = wsp.alloc_n<float>(unit), *x1 = wsp.alloc_n<float>(unit), *t = wsp.alloc_n<float>(unit), *att = wsp.alloc_n<float>(unit);
  float *qkv = wsp.alloc_n<float>(3 * unit), *hid = wsp.alloc_n<float>(M * I);
  float *tail = wsp.alloc_n<float>((int64_t)B * (C + 2 * c.joint_dim));
  auto tap = [&](int i, const float *src, int64_t floats) {
    if (taps && taps[i]) SF_HIP(hipMemcpyAsync(taps[i], src, (size_t)floats * 4, hipMemcpyDeviceToDevice, s));
  };
  SF_HIP(launch_text_embed(ids, B, S, C, c.vocab_size, c.max_positions, c.pad_id, h->word, h->pos, h->type, h->emb_g, h->emb_b, c.ln_eps, x, s));
  tap(0, x, unit);
  for (int i = 0; i < c.layers; ++i) {
    const LayerW &l = h->layers[i];
    SF_HIP(launch_conv_gemm(F32, lin(x, B, S, C, 3 * C, l.qkv_w, l.qkv_b, nullptr, 0, qkv), s));
    SF_HIP(launch_masked_attention(qkv, mask, B, S, c.heads, att, s));
    SF_HIP(launch_conv_gemm(F32, lin(att, B, S, C, C, l.ao_w, l.ao_b, x, 0, t), s));
    SF_HIP(launch_layernorm_affine(t, M, C, l.ln1_g, l.ln1_b, c.ln_eps, x1, s));
    SF_HIP(launch_conv_gemm(F32, lin(x1, B, S, C, I, l.fc1_w, l.fc1_b, nullptr, 2, hid), s));
    SF_HIP(launch_conv_gemm(F32, lin(hid, B, S, I, C, l.fc2_w, l.fc2_b, x1, 0, t), s));
    SF_HIP(launch_layernorm_affine(t, M, C, l.ln2_g, l.ln2_b, c.ln_eps, x, s));
    tap(i + 1, x, unit);
  }
  SF_HIP(launch_text_tail(x, B, S, C, c.joint_dim, c.pooling == 0, h->pool_w, h->pool_b, h->p0_w, h->p0_b, c.projection_relu, h->p2_w, h->p2_b,
                          c.normalize, tail, embedding, s));
  tap(c.layers + 1, tail, (int64_t)B * C);
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
