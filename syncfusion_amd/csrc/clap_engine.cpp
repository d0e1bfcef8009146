// CLAP audio embedder behind the C ABI (replaces laion_clap.CLAP_Module(enable_fusion=False, amodel='HTSAT-tiny').get_audio_embedding_from_data,
// main/module_diffusion.py:64-67): patch embed, the Swin stages (window attention, MLP, PatchMerging) and the embedding tail on the log-mel
// image of clap_front.hip.  fp32 throughout.  qkv, proj, fc1 (+ GELU), fc2 (+ residual) and the merge reduction run on the implicit-GEMM
// launcher; the caller has folded every LayerNorm affine into the weights that follow it, so the LayerNorm launches only normalise.
// Weights are copied once at create time; the forward call allocates nothing.  Also the C entry points of the stand-alone pieces.
#include <algorithm>
#include <cmath>
#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "clap.h"
#include "engine_common.h"

using namespace sf;

namespace {

constexpr int PATCH = 4;

struct BlockW {
  float *qkv_w = nullptr, *qkv_b = nullptr, *rpb = nullptr, *proj_w = nullptr, *proj_b = nullptr;
  float *fc1_w = nullptr, *fc1_b = nullptr, *fc2_w = nullptr, *fc2_b = nullptr;
  int shift = 0;
};
struct StageW {
  int res = 0, C = 0, heads = 0;       // tokens per side, width
  std::vector<BlockW> blocks;
  float *merge_w = nullptr, *merge_b = nullptr;
};

void check_config(const sf_clap_audio_config &c) {
  if (c.n_stages < 1 || c.n_stages > SF_CLAP_MAX_STAGES) fail(SF_ERR_INVALID, "1 .. %d stages expected", SF_CLAP_MAX_STAGES);
  if (c.window != SWIN_WINDOW) fail(SF_ERR_UNSUPPORTED, "window %d: only %d is built", c.window, SWIN_WINDOW);
  if (c.spec_size < PATCH * SWIN_WINDOW || c.spec_size > 4096 || c.spec_size % (PATCH * SWIN_WINDOW << (c.n_stages - 1)))
    fail(SF_ERR_SHAPE, "spec_size %d: a multiple of %d expected (every stage a whole number of windows)", c.spec_size,
         PATCH * SWIN_WINDOW << (c.n_stages - 1));
  if (c.embed_dim < 32 || c.embed_dim > 256 || c.embed_dim % 32) fail(SF_ERR_SHAPE, "embed_dim %d: a multiple of 32 in 32 .. 256 expected", c.embed_dim);
  if (c.mlp_ratio < 1 || c.mlp_ratio > 8) fail(SF_ERR_INVALID, "mlp_ratio %d", c.mlp_ratio);
  if (c.joint_dim < 1 || c.joint_dim > 1024) fail(SF_ERR_SHAPE, "joint_dim %d outside 1 .. 1024", c.joint_dim);
  if (!(c.ln_eps > 0.f)) fail(SF_ERR_INVALID, "ln_eps must be positive");
  for (int i = 0; i < c.n_stages; ++i) {
    const int C = c.embed_dim << i;
    if (c.depths[i] < 1 || c.depths[i] > 64) fail(SF_ERR_INVALID, "stage %d: depth %d", i, c.depths[i]);
    if (c.heads[i] < 1 || C % c.heads[i]) fail(SF_ERR_SHAPE, "stage %d: %d heads do not divide %d channels", i, c.heads[i], C);
    const int D = C / c.heads[i];
    if (D % 4 || D > SWIN_MAX_HEAD_DIM) fail(SF_ERR_UNSUPPORTED, "stage %d: head dim %d (a multiple of 4 up to %d is built)", i, D, SWIN_MAX_HEAD_DIM);
  }
  if ((c.embed_dim << (c.n_stages - 1)) > 1024) fail(SF_ERR_SHAPE, "final width %d above 1024", c.embed_dim << (c.n_stages - 1));
  const int last = c.spec_size / PATCH >> (c.n_stages - 1);
  if (last * last > 256) fail(SF_ERR_SHAPE, "%d final tokens above 256", last * last);
}

int shift_of(const sf_clap_audio_config &c, int res, int j) { return (res <= c.window || (j % 2) == 0) ? 0 : c.window / 2; }

// the GEMMs of the network at B clips
std::vector<LinearDesc> gemms_of(const sf_clap_audio_config &c, int B) {
  std::vector<LinearDesc> g;
  int res = c.spec_size / PATCH;
  for (int i = 0; i < c.n_stages; ++i) {
    const int C = c.embed_dim << i, tok = res * res;
    const std::string st = "stage " + std::to_string(i) + " ";
    g.push_back({st + "qkv", B, tok, C, 3 * C, 0, false});
    g.push_back({st + "proj", B, tok, C, C, 0, true});
    g.push_back({st + "fc1", B, tok, C, c.mlp_ratio * C, 2, false});
    g.push_back({st + "fc2", B, tok, c.mlp_ratio * C, C, 0, true});
    if (i + 1 < c.n_stages) {
      g.push_back({st + "merge", B, tok / 4, 4 * C, 2 * C, 0, false});
      res /= 2;
    }
  }
  return g;
}

}  // namespace

struct sf_clap_audio {
  sf_clap_audio_config cfg;
  DeviceArena arena;
  std::vector<StageW> stages;
  float *patch_w = nullptr, *patch_b = nullptr, *patch_g = nullptr, *patch_beta = nullptr;
  float *head_g = nullptr, *head_beta = nullptr, *p0_w = nullptr, *p0_b = nullptr, *p2_w = nullptr, *p2_b = nullptr;
  int tokens0 = 0;     // tokens per clip behind the patch embed
  int final_C = 0, final_tokens = 0;
};

static int max_batch(const sf_clap_audio *h) {
  // the widest activation (the MLP's hidden rows of the first stage) stays below 2^31 bytes: the GEMM kernels' 32-bit offsets
  const int64_t per = (int64_t)h->tokens0 * h->cfg.embed_dim * std::max(h->cfg.mlp_ratio, 3) * 4;
  return (int)std::min<int64_t>(65535, 0x7FFFFFF0ll / per);
}

// X0 | X1 (residual stream, ping-pong) | T (normalised rows) | A (attention output) | QKV | HID | the tail's pooled, hidden and raw rows
static int64_t ws_bytes_for(const sf_clap_audio *h, int B) {
  const int64_t unit = (int64_t)B * h->tokens0 * h->cfg.embed_dim * 4;
  return 4 * align_up(unit, 256) + align_up(3 * unit, 256) + align_up(h->cfg.mlp_ratio * unit, 256) +
         align_up((int64_t)B * (h->final_C + 2 * h->cfg.joint_dim) * 4, 256);
}

extern "C" {

int sf_clap_audio_create(const sf_clap_audio_config *cfg, const sf_tensor *weights, int n_weights, void *stream, sf_clap_audio **out) {
  SF_API_BEGIN
  if (!cfg || !weights || !out) fail(SF_ERR_INVALID, "null argument");
  *out = nullptr;
  if (n_weights < 1) fail(SF_ERR_INVALID, "no weights");
  const sf_clap_audio_config c = *cfg;
  check_config(c);
  const WeightMap wm(weights, n_weights);
  WeightWants ww;
  auto eng = std::unique_ptr<sf_clap_audio>(new sf_clap_audio());
  eng->cfg = c;
  const int E = c.embed_dim, J = c.joint_dim, NBIAS = (2 * c.window - 1) * (2 * c.window - 1);
  ww.want("patch.w", (int64_t)E * PATCH * PATCH, &eng->patch_w);
  ww.want("patch.b", E, &eng->patch_b);
  ww.want("patch.g", E, &eng->patch_g);
  ww.want("patch.beta", E, &eng->patch_beta);
  eng->stages.resize(c.n_stages);
  int res = c.spec_size / PATCH;
  eng->tokens0 = res * res;
  for (int i = 0; i < c.n_stages; ++i) {
    StageW &st = eng->stages[i];
    st.res = res, st.C = E << i, st.heads = c.heads[i];
    st.blocks.resize(c.depths[i]);
    const int64_t C = st.C, Hd = (int64_t)c.mlp_ratio * C;
    for (int j = 0; j < c.depths[i]; ++j) {
      BlockW &b = st.blocks[j];
      b.shift = shift_of(c, res, j);
      const std::string p = "s" + std::to_string(i) + ".b" + std::to_string(j) + ".";
      ww.want(p + "qkv.w", 3 * C * C, &b.qkv_w);
      ww.want(p + "qkv.b", 3 * C, &b.qkv_b);
      ww.want(p + "rpb", (int64_t)NBIAS * st.heads, &b.rpb);
      ww.want(p + "proj.w", C * C, &b.proj_w);
      ww.want(p + "proj.b", C, &b.proj_b);
      ww.want(p + "fc1.w", Hd * C, &b.fc1_w);
      ww.want(p + "fc1.b", Hd, &b.fc1_b);
      ww.want(p + "fc2.w", C * Hd, &b.fc2_w);
      ww.want(p + "fc2.b", C, &b.fc2_b);
    }
    if (i + 1 < c.n_stages) {
      const std::string p = "s" + std::to_string(i) + ".merge.";
      ww.want(p + "w", 2 * C * 4 * C, &st.merge_w);
      ww.want(p + "b", 2 * C, &st.merge_b);
      res /= 2;
    }
  }
  eng->final_C = eng->stages.back().C;
  eng->final_tokens = res * res;
  ww.want("head.g", eng->final_C, &eng->head_g);
  ww.want("head.beta", eng->final_C, &eng->head_beta);
  ww.want("proj0.w", (int64_t)J * eng->final_C, &eng->p0_w);
  ww.want("proj0.b", J, &eng->p0_b);
  ww.want("proj2.w", (int64_t)J * J, &eng->p2_w);
  ww.want("proj2.b", J, &eng->p2_b);
  hipStream_t s = static_cast<hipStream_t>(stream);
  ww.load(wm, eng->arena, s);   // refuses a missing or mis-sized name before the first HIP call
  SF_HIP(hipStreamSynchronize(s));
  *out = eng.release();
  return SF_OK;
  SF_API_END
}

void sf_clap_audio_destroy(sf_clap_audio *h) { delete h; }

int sf_clap_audio_max_batch(const sf_clap_audio *h) { return h ? max_batch(h) : -1; }

int64_t sf_clap_audio_workspace_bytes(const sf_clap_audio *h, int B) {
  if (!h || B < 1 || B > max_batch(h)) return -1;
  return ws_bytes_for(h, B);
}

int sf_clap_audio_describe(const sf_clap_audio_config *cfg, int B, char *text, int64_t capacity) {
  SF_API_BEGIN
  if (!cfg || !text || capacity < 1) fail(SF_ERR_INVALID, "null argument");
  if (B < 1) fail(SF_ERR_INVALID, "B must be at least 1");
  check_config(*cfg);
  describe_gemms(gemms_of(*cfg, B), "", text, capacity);
  return SF_OK;
  SF_API_END
}

int sf_clap_audio_forward(sf_clap_audio *h, const float *image, int B, float *embedding, float *const *taps, void *ws, int64_t ws_bytes,
                          void *stream) {
  SF_API_BEGIN
  if (!h || !image || !embedding) fail(SF_ERR_INVALID, "null argument");
  if (B < 1) fail(SF_ERR_INVALID, "B must be at least 1");
  if (B > max_batch(h)) fail(SF_ERR_SHAPE, "at most %d clips per call", max_batch(h));
  require_workspace(ws, ws_bytes, ws_bytes_for(h, B));
  const sf_clap_audio_config &c = h->cfg;
  require_gemm_kernels(gemms_of(c, B));
  hipStream_t s = static_cast<hipStream_t>(stream);
  Workspace wsp(ws, ws_bytes);
  const int64_t unit = (int64_t)B * h->tokens0 * c.embed_dim;
  float *x = wsp.alloc_n<float>(unit), *x1 = wsp.alloc_n<float>(unit), *t = wsp.alloc_n<float>(unit), *att = wsp.alloc_n<float>(unit);
  float *qkv = wsp.alloc_n<float>(3 * unit), *hid = wsp.alloc_n<float>(c.mlp_ratio * unit);
  float *tail = wsp.alloc_n<float>((int64_t)B * (h->final_C + 2 * c.joint_dim));
  SF_HIP(launch_patch_embed(image, B, c.spec_size, c.embed_dim, h->patch_w, h->patch_b, h->patch_g, h->patch_beta, c.ln_eps, x, s));
  copy_tap(taps, 0, x, unit, s);
  for (int i = 0; i < c.n_stages; ++i) {
    const StageW &st = h->stages[i];
    const int C = st.C, tok = st.res * st.res, Hd = c.mlp_ratio * C;
    const int64_t M = (int64_t)B * tok;
    for (const BlockW &b : st.blocks) {
      SF_HIP(launch_swin_layernorm(x, M, C, c.ln_eps, 0, 0, 0, t, s));
      SF_HIP(launch_conv_gemm(F32, token_linear_args(t, B, tok, C, 3 * C, b.qkv_w, b.qkv_b, nullptr, 0, qkv), s));
      SF_HIP(launch_window_attention(qkv, B, st.res, st.res, C, st.heads, b.shift, b.rpb, c.mask_value, att, s));
      SF_HIP(launch_conv_gemm(F32, token_linear_args(att, B, tok, C, C, b.proj_w, b.proj_b, x, 0, x1), s));
      SF_HIP(launch_swin_layernorm(x1, M, C, c.ln_eps, 0, 0, 0, t, s));
      SF_HIP(launch_conv_gemm(F32, token_linear_args(t, B, tok, C, Hd, b.fc1_w, b.fc1_b, nullptr, 2, hid), s));
      SF_HIP(launch_conv_gemm(F32, token_linear_args(hid, B, tok, Hd, C, b.fc2_w, b.fc2_b, x1, 0, x), s));
    }
    int64_t floats = M * C;
    if (i + 1 < c.n_stages) {
      SF_HIP(launch_swin_layernorm(x, M / 4, 4 * C, c.ln_eps, 1, st.res, st.res, t, s));
      SF_HIP(launch_conv_gemm(F32, token_linear_args(t, B, tok / 4, 4 * C, 2 * C, st.merge_w, st.merge_b, nullptr, 0, x1), s));
      std::swap(x, x1);
      floats /= 2;
    }
    copy_tap(taps, i + 1, x, floats, s);
  }
  SF_HIP(launch_clap_tail(x, B, h->final_tokens, h->final_C, c.joint_dim, h->head_g, h->head_beta, c.ln_eps, h->p0_w, h->p0_b, h->p2_w, h->p2_b,
                          c.projection_relu, c.normalize, tail, embedding, s));
  return SF_OK;
  SF_API_END
}

int sf_op_window_attention(const float *qkv, int B, int H, int W, int C, int heads, int shift, const float *bias_table, float mask_value, float *out,
                           void *stream) {
  SF_API_BEGIN
  if (!qkv || !bias_table || !out) fail(SF_ERR_INVALID, "null argument");
  if (B < 1 || H < 1 || W < 1 || C < 1 || heads < 1) fail(SF_ERR_INVALID, "B, H, W, C, heads >= 1 expected");
  if (C % heads) fail(SF_ERR_SHAPE, "%d heads do not divide %d channels", heads, C);
  const int D = C / heads;
  if (D % 4 || D > SWIN_MAX_HEAD_DIM) fail(SF_ERR_UNSUPPORTED, "head dim %d: a multiple of 4 up to %d is built", D, SWIN_MAX_HEAD_DIM);
  if (H % SWIN_WINDOW || W % SWIN_WINDOW) fail(SF_ERR_SHAPE, "H = %d, W = %d: multiples of the window (%d) expected", H, W, SWIN_WINDOW);
  if (shift != 0 && shift != SWIN_WINDOW / 2) fail(SF_ERR_UNSUPPORTED, "shift %d: 0 or %d is built", shift, SWIN_WINDOW / 2);
  if (shift && (H == SWIN_WINDOW || W == SWIN_WINDOW)) fail(SF_ERR_SHAPE, "a shifted window needs H, W > %d (the caller sets shift 0 there)", SWIN_WINDOW);
  if ((int64_t)B * H * W * 3 * C >= (1ll << 31) || (int64_t)B * (H / SWIN_WINDOW) * (W / SWIN_WINDOW) * heads >= (1ll << 31))
    fail(SF_ERR_SHAPE, "tensor too large");
  SF_HIP(launch_window_attention(qkv, B, H, W, C, heads, shift, bias_table, mask_value, out, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_logmel_image(const float *mel_power, int B, int n_mels, int T, int ratio, const float *scale, const float *shift, float amin, float *image,
                       void *stream) {
  SF_API_BEGIN
  if (!mel_power || !scale || !shift || !image) fail(SF_ERR_INVALID, "null argument");
  if (B < 1 || n_mels < 1 || ratio < 1 || T < 2) fail(SF_ERR_INVALID, "B, n_mels, ratio >= 1 and T >= 2 expected");
  if (!(amin > 0.f)) fail(SF_ERR_INVALID, "amin must be positive");
  const int64_t S = (int64_t)n_mels * ratio, Tt = S * ratio;
  if (S > 4096 || Tt > 32768) fail(SF_ERR_SHAPE, "image side %lld / %lld frames out of range", (long long)S, (long long)Tt);
  if (T > Tt) fail(SF_ERR_SHAPE, "%d frames exceed the image's %lld: a longer spectrogram is not shrunk", T, (long long)Tt);
  if ((int64_t)B * S * S >= (1ll << 31) || (int64_t)B * n_mels * T >= (1ll << 31)) fail(SF_ERR_SHAPE, "tensor too large");
  const float db_floor = (float)(10.0 * std::log10((double)amin));
  SF_HIP(launch_logmel_image(mel_power, B, n_mels, T, ratio, scale, shift, amin, db_floor, image, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

}  // extern "C"
