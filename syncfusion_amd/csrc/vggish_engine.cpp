// VGGish engine of the FAD evaluation behind the C ABI (replaces the torch.hub VGGish model the frechet_audio_distance package runs at
// main/evaluation.py:7-28): a stack of 3x3 convolutions (+ bias + ReLU) and 2x2 max-pools on channels-last rows, then fully connected
// layers as 1x1 convolutions on one row per example.  fp32 throughout.  Weights are packed once at create time; the forward call
// allocates nothing.  Also the C entry points of the stand-alone pieces in fad.hip (max-pool, moments).
#include <algorithm>
#include <exception>
#include <memory>
#include <vector>

#include "engine_common.h"
#include "fad.h"

using namespace sf;

namespace {

constexpr int IN_LD = 4;            // the examples' rows: one channel in 4 columns (sf_logmel_examples_forward)
constexpr int MAX_STAGES = 64;

struct Stage {
  int cout = 0;                     // 0: max-pool
  int Hi = 0, Wi = 0, cin = 0, cin_ld = 0, cout_ld = 0;
  float *w = nullptr, *bias = nullptr;
};
struct Fc {
  int n = 0, n_ld = 0, k = 0;       // outputs, their row length, reduction length (a multiple of 32)
  int cin = 0;                      // columns read from a source row
  int act = 0;
  float *w = nullptr, *bias = nullptr;
};

}  // namespace

struct sf_vggish {
  DeviceArena arena;
  std::vector<Stage> stages;
  std::vector<Fc> fcs;
  int H = 0, W = 0, n_pools = 0;
  int64_t max_row_floats = 0;       // per example: the largest activation (rows x ld) any layer writes
  int64_t max_fc_floats = 0;
};

static VConvGeom geom_of(const Stage &st) {
  VConvGeom g;
  g.cin = st.cin, g.cout = st.cout, g.T = 1;
  g.Hi = g.Ho = st.Hi, g.Wi = g.Wo = st.Wi;
  g.kt = 1, g.kh = g.kw = 3, g.sh = g.sw = 1, g.pt = 0, g.ph = g.pw = 1;
  return g;
}

// largest batch whose activations stay below 2^31 bytes each (the convolution kernels' 32-bit offsets)
static int max_examples(const sf_vggish *h) {
  const int64_t per = std::max<int64_t>(h->max_row_floats, (int64_t)h->H * h->W * IN_LD) * 4;
  return (int)std::min<int64_t>(65535, (0x7FFFFFF0ll / per));
}

static int64_t ws_bytes_for(const sf_vggish *h, int n) { return 2 * align_up(n * h->max_row_floats * 4, 256) + 2 * align_up(n * h->max_fc_floats * 4, 256); }

extern "C" {

int sf_vggish_create(int n_stages, const int32_t *stages, int n_fc, const int32_t *fc_widths, int H, int W, int final_relu,
                     const void *const *conv_w, const void *const *conv_b, const void *const *fc_w, const void *const *fc_b, void *stream,
                     sf_vggish **out) {
  SF_API_BEGIN
  if (!out || !stages || !fc_widths || !conv_w || !conv_b || !fc_w || !fc_b) fail(SF_ERR_INVALID, "null argument");
  *out = nullptr;
  if (n_stages < 1 || n_stages > MAX_STAGES || n_fc < 1 || n_fc > MAX_STAGES) fail(SF_ERR_INVALID, "1 .. %d stages and fully connected layers expected", MAX_STAGES);
  if (H < 1 || W < 1 || H > 4096 || W > 4096) fail(SF_ERR_INVALID, "example extent %d x %d out of range", H, W);
  // the geometry walk needs no device: every refusal below comes before the first HIP call
  std::vector<Stage> st(n_stages);
  int h = H, w = W, c = 1, ld = IN_LD, n_conv = 0, n_pools = 0;
  int64_t max_rows = 0;
  for (int i = 0; i < n_stages; ++i) {
    Stage &s = st[i];
    s.Hi = h, s.Wi = w, s.cin = c, s.cin_ld = ld;
    if (stages[i] < 0 || stages[i] > 8192) fail(SF_ERR_INVALID, "stage %d: %d channels", i, stages[i]);
    if (stages[i] == 0) {
      if (h < 2 || w < 2) fail(SF_ERR_SHAPE, "stage %d: a %d x %d map cannot be pooled", i, h, w);
      h /= 2, w /= 2;
      s.cout_ld = ld;
      ++n_pools;
    } else {
      if (!conv_w[n_conv] || !conv_b[n_conv]) fail(SF_ERR_MISSING_WEIGHT, "convolution %d has a null weight or bias", n_conv);
      s.cout = stages[i];
      s.cout_ld = pad_to(s.cout, 8);
      c = s.cout, ld = s.cout_ld;
      ++n_conv;
    }
    max_rows = std::max<int64_t>(max_rows, (int64_t)h * w * s.cout_ld);
  }
  if (n_conv == 0) fail(SF_ERR_INVALID, "no convolution among the stages");
  std::vector<Fc> fcs(n_fc);
  int64_t max_fc = 0;
  int in_c = c, in_ld = ld, P = h * w;
  for (int i = 0; i < n_fc; ++i) {
    Fc &f = fcs[i];
    if (fc_widths[i] < 1 || fc_widths[i] > 65536) fail(SF_ERR_INVALID, "fully connected layer %d: width %d", i, fc_widths[i]);
    if (!fc_w[i] || !fc_b[i]) fail(SF_ERR_MISSING_WEIGHT, "fully connected layer %d has a null weight or bias", i);
    if ((int64_t)P * in_ld > (1 << 24)) fail(SF_ERR_SHAPE, "fully connected layer %d reads %lld columns", i, (long long)P * in_ld);
    f.n = fc_widths[i];
    const bool last = i == n_fc - 1;
    f.n_ld = last ? f.n : pad_to(f.n, 8);     // the embeddings leave as a dense (n, D) matrix
    f.cin = P * in_ld;
    f.k = vconv_k(1, f.cin);
    f.act = last ? (final_relu ? 1 : 0) : 1;
    max_fc = std::max<int64_t>(max_fc, f.n_ld);
    (void)in_c;
    in_c = f.n, in_ld = f.n_ld, P = 1;
  }

  hipStream_t s = static_cast<hipStream_t>(stream);
  auto eng = std::unique_ptr<sf_vggish>(new sf_vggish());
  eng->H = H, eng->W = W, eng->n_pools = n_pools, eng->max_row_floats = max_rows, eng->max_fc_floats = max_fc;
  n_conv = 0;
  for (Stage &sg : st) {
    if (!sg.cout) continue;
    const VConvGeom g = geom_of(sg);
    sg.w = eng->arena.alloc_n<float>((int64_t)sg.cout * vconv_k(g.taps(), sg.cin_ld));
    sg.bias = eng->arena.alloc_n<float>(sg.cout);
    SF_HIP(launch_vconv_pack_fwd(static_cast<const float *>(conv_w[n_conv]), g, sg.cin_ld, sg.w, s));
    SF_HIP(hipMemcpyAsync(sg.bias, conv_b[n_conv], (size_t)sg.cout * 4, hipMemcpyDeviceToDevice, s));
    ++n_conv;
  }
  in_c = c, in_ld = ld, P = h * w;
  for (int i = 0; i < n_fc; ++i) {
    Fc &f = fcs[i];
    f.w = eng->arena.alloc_n<float>((int64_t)f.n * f.k);
    f.bias = eng->arena.alloc_n<float>(f.n);
    SF_HIP(launch_pack_fc(static_cast<const float *>(fc_w[i]), f.n, P, in_c, in_ld, f.k, f.w, s));
    SF_HIP(hipMemcpyAsync(f.bias, fc_b[i], (size_t)f.n * 4, hipMemcpyDeviceToDevice, s));
    in_c = f.n, in_ld = f.n_ld, P = 1;
  }
  SF_HIP(hipStreamSynchronize(s));
  eng->stages = st;
  eng->fcs = fcs;
  *out = eng.release();
  return SF_OK;
  SF_API_END
}

void sf_vggish_destroy(sf_vggish *h) { delete h; }

int sf_vggish_max_examples(const sf_vggish *h) { return h ? max_examples(h) : -1; }

int64_t sf_vggish_workspace_bytes(const sf_vggish *h, int n) {
  if (!h || n < 1 || n > max_examples(h)) return -1;
  return ws_bytes_for(h, n);
}

int sf_vggish_forward(sf_vggish *h, const float *examples, int n, float *embeddings, float *const *pool_taps, void *ws, int64_t ws_bytes,
                      void *stream) {
  SF_API_BEGIN
  if (!h || !examples || !embeddings) fail(SF_ERR_INVALID, "null argument");
  if (n < 1) fail(SF_ERR_INVALID, "n must be at least 1");
  if (n > max_examples(h)) fail(SF_ERR_SHAPE, "at most %d examples per call", max_examples(h));
  require_workspace(ws, ws_bytes, ws_bytes_for(h, n));
  hipStream_t s = static_cast<hipStream_t>(stream);
  Workspace wsp(ws, ws_bytes);
  float *buf[2] = {wsp.alloc_n<float>(n * h->max_row_floats), wsp.alloc_n<float>(n * h->max_row_floats)};
  float *fbuf[2] = {wsp.alloc_n<float>(n * h->max_fc_floats), wsp.alloc_n<float>(n * h->max_fc_floats)};
  const float *cur = examples;
  int flip = 0, pool = 0;
  for (const Stage &sg : h->stages) {
    float *dst = buf[flip];
    flip ^= 1;
    if (sg.cout) {
      const VConvGeom g = geom_of(sg);   // T = 1: one example per "frame"
      ConvGemmArgs a = vconv_args(g, n, cur, sg.cin_ld, sg.w, vconv_k(g.taps(), sg.cin_ld), dst, sg.cout_ld);
      a.bias = sg.bias;
      a.n_store = sg.cout_ld;   // columns cout .. cout_ld are written as zeros
      a.act = 1;
      a.solo = 1;
      SF_HIP(launch_conv_gemm(F32, a, s));
    } else {
      SF_HIP(launch_maxpool2x2_cl(cur, n, sg.Hi, sg.Wi, sg.cin_ld, dst, s));
      copy_tap(pool_taps, pool, dst, (int64_t)n * (sg.Hi / 2) * (sg.Wi / 2) * sg.cin_ld, s);
      ++pool;
    }
    cur = dst;
  }
  flip = 0;
  for (size_t i = 0; i < h->fcs.size(); ++i) {
    const Fc &f = h->fcs[i];
    const bool last = i + 1 == h->fcs.size();
    float *dst = last ? embeddings : fbuf[flip];
    flip ^= 1;
    ConvGemmArgs a = linear_args(cur, n, f.cin, f.n, f.w, f.bias, dst);
    a.geom = 1;                 // a 1x1 convolution on a 1x1 map: one row per example
    a.K = f.k;                  // the packed rows are padded to a multiple of 32
    a.out_ld = a.n_store = f.n_ld;
    a.act = f.act;
    a.solo = 1;
    SF_HIP(launch_conv_gemm(F32, a, s));
    cur = dst;
  }
  return SF_OK;
  SF_API_END
}

int sf_op_maxpool2x2_cl(const float *x, int64_t n, int H, int W, int ld, float *y, void *stream) {
  SF_API_BEGIN
  if (!x || !y) fail(SF_ERR_INVALID, "null argument");
  if (n < 1 || H < 2 || W < 2 || ld < 1) fail(SF_ERR_INVALID, "n, ld >= 1 and H, W >= 2 expected");
  if (n * H * W * ld >= (1ll << 40)) fail(SF_ERR_SHAPE, "tensor too large");
  SF_HIP(launch_maxpool2x2_cl(x, n, H, W, ld, y, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_moments(const float *x, int64_t n, int D, double *sum, double *scatter, void *stream) {
  SF_API_BEGIN
  if (!x || !sum || !scatter) fail(SF_ERR_INVALID, "null argument");
  if (n < 1) fail(SF_ERR_INVALID, "n must be at least 1");
  if (D < 1 || D > 128) fail(SF_ERR_SHAPE, "1 .. 128 columns expected, got %d", D);
  if (n >= (1ll << 40)) fail(SF_ERR_SHAPE, "too many rows");
  SF_HIP(launch_moments(x, n, D, sum, scatter, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

}  // extern "C"
