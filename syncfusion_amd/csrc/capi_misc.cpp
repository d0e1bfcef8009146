// Version / error / device probes, the onset glue and the op-level test entry points of the C ABI.
#include <algorithm>
#include <cstring>
#include <cstdlib>
#include <cmath>
#include <exception>

#include "engine_common.h"

using namespace sf;

extern "C" {

const char *sf_version(void) { return "syncfusion_amd 0.1.0 (gfx950)"; }
const char *sf_last_error(void) { return get_error(); }

int sf_device_ok(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1) {
    (void)hipGetLastError();
    return 0;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 0;
  return std::string(prop.gcnArchName).rfind("gfx950", 0) == 0 ? 1 : 0;
}

// Measurement aid (bench.py): the shader clock the chip holds WHILE a workload runs.  sf_clock_probe_start puts a one-wave kernel on `stream`
// (use a side stream) that watches the shader-cycle counter against the constant 100 MHz counter for `microseconds`; sf_clock_probe_read
// waits for it and returns MHz.  One probe at a time per process.
static unsigned long long *g_clock_buf = nullptr;
static hipEvent_t g_clock_ev = nullptr;
int sf_clock_probe_start(double microseconds, void *stream) {
  SF_API_BEGIN
  if (microseconds <= 0.0 || microseconds > 5.0e6) fail(SF_ERR_INVALID, "clock probe: 0 < microseconds <= 5e6");
  if (!g_clock_buf) SF_HIP(hipHostMalloc(reinterpret_cast<void **>(&g_clock_buf), 2 * sizeof(unsigned long long), hipHostMallocDefault));
  if (!g_clock_ev) SF_HIP(hipEventCreateWithFlags(&g_clock_ev, hipEventDisableTiming));
  g_clock_buf[0] = g_clock_buf[1] = 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  SF_HIP(launch_clock_probe(microseconds, g_clock_buf, s));
  SF_HIP(hipEventRecord(g_clock_ev, s));
  return SF_OK;
  SF_API_END
}
int sf_clock_probe_read(double *mhz_out) {
  SF_API_BEGIN
  if (!mhz_out || !g_clock_ev || !g_clock_buf) fail(SF_ERR_INVALID, "clock probe: nothing started");
  SF_HIP(hipEventSynchronize(g_clock_ev));
  *mhz_out = g_clock_buf[1] ? 100.0 * (double)g_clock_buf[0] / (double)g_clock_buf[1] : 0.0;
  return SF_OK;
  SF_API_END
}

int sf_onsets_to_track(const float *logits, int N, int T, const int32_t *start_frame, float frame_rate, float sample_rate,
                       float threshold, float *track, int L, void *stream) {
  SF_API_BEGIN
  if (!logits || !track || N < 1 || T < 1 || L < 1 || frame_rate <= 0.f) fail(SF_ERR_INVALID, "bad argument");
  SF_HIP(launch_onsets_to_track(logits, N, T, start_frame, frame_rate, sample_rate, threshold, track, L, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_frames_preprocess(const uint8_t *frames, int N, int T, int H, int W, int out_h, int out_w, const float *mean3, const float *std3, float *out,
                         void *stream) {
  SF_API_BEGIN
  if (!frames || !out || !mean3 || !std3 || N < 1 || T < 1 || H < 1 || W < 1 || out_h < 1 || out_w < 1) fail(SF_ERR_INVALID, "bad argument");
  for (int i = 0; i < 3; ++i)
    if (!(std3[i] > 0.f)) fail(SF_ERR_INVALID, "std must be positive");
  hipError_t e = launch_frames_preprocess(frames, N, T, H, W, out_h, out_w, mean3, std3, out, static_cast<hipStream_t>(stream));
  if (e == hipErrorInvalidValue) fail(SF_ERR_UNSUPPORTED, "down-scaling factor above 7.5 is not supported");
  SF_HIP(e);
  return SF_OK;
  SF_API_END
}

int64_t sf_frames_augment_workspace_bytes(int N, int T, int out_h, int out_w) {
  if (N < 1 || T < 1 || out_h < 1 || out_w < 1) return -1;
  return frames_augment_workspace_bytes(N, T, out_h, out_w);
}

static_assert(sizeof(sf_augment_clip) == sizeof(AugClip) && sizeof(AugClip) == 48, "sf_augment_clip is the kernels' table entry");
int sf_frames_augment(const uint8_t *frames, int N, int T, int H, int W, int resize_h, int resize_w, int out_h, int out_w,
                      const sf_augment_clip *table_host, const sf_augment_clip *table_dev, const float *mean3, const float *std3, float *out, void *ws,
                      int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!frames || !out || !mean3 || !std3 || !table_host || !table_dev || N < 1 || T < 1 || H < 1 || W < 1 || resize_h < 1 || resize_w < 1 ||
      out_h < 1 || out_w < 1)
    fail(SF_ERR_INVALID, "bad argument");
  for (int i = 0; i < 3; ++i)
    if (!(std3[i] > 0.f)) fail(SF_ERR_INVALID, "std must be positive");
  if (out_h > resize_h || out_w > resize_w)
    fail(SF_ERR_INVALID, "crop (%d, %d) larger than the resized frame (%d, %d)", out_h, out_w, resize_h, resize_w);
  bool any_contrast = false;
  for (int n = 0; n < N; ++n) {   // every way a table could send a kernel out of bounds (or into NaN) is refused here
    const sf_augment_clip &c = table_host[n];
    if (c.top < 0 || c.left < 0 || c.top > resize_h - out_h || c.left > resize_w - out_w)
      fail(SF_ERR_INVALID, "clip %d: crop origin (%d, %d) + (%d, %d) lies outside the resized frame (%d, %d)", n, c.top, c.left, out_h, out_w, resize_h,
           resize_w);
    int seen = 0;
    for (int k = 0; k < 4; ++k)
      if (c.order[k] >= 0 && c.order[k] < 4) seen |= 1 << c.order[k];
    if (seen != 15) fail(SF_ERR_INVALID, "clip %d: order (%d, %d, %d, %d) is not a permutation of 0..3", n, c.order[0], c.order[1], c.order[2], c.order[3]);
    if (c.mask < 0 || c.mask > 15) fail(SF_ERR_INVALID, "clip %d: mask %d outside 0..15", n, c.mask);
    for (int k = 0; k < 4; ++k) {
      if (!std::isfinite(c.factor[k])) fail(SF_ERR_INVALID, "clip %d: factor %d is not finite", n, k);
      if (k < 3 ? c.factor[k] < 0.f : std::fabs(c.factor[k]) > 0.5f) fail(SF_ERR_INVALID, "clip %d: factor %d = %g outside its range", n, k, (double)c.factor[k]);
    }
    any_contrast = any_contrast || (c.mask & 2);
  }
  require_workspace(ws, ws_bytes, frames_augment_workspace_bytes(N, T, out_h, out_w));
  hipError_t e = launch_frames_augment(frames, N, T, H, W, resize_h, resize_w, out_h, out_w, reinterpret_cast<const AugClip *>(table_dev), any_contrast, mean3,
                                       std3, out, static_cast<float *>(ws), static_cast<hipStream_t>(stream));
  if (e == hipErrorInvalidValue) fail(SF_ERR_UNSUPPORTED, "down-scaling factor above 7.5 (or more than 2^31 workgroups) is not supported");
  SF_HIP(e);
  return SF_OK;
  SF_API_END
}

int sf_times_to_track(const double *times, const int32_t *clip_of, int n_times, double sample_rate, int B, int L, float *track, void *stream) {
  SF_API_BEGIN
  if (!track || B < 1 || L < 1 || n_times < 0 || (n_times > 0 && (!times || !clip_of)) || !(sample_rate > 0)) fail(SF_ERR_INVALID, "bad argument");
  SF_HIP(launch_times_to_track(times, clip_of, n_times, sample_rate, B, L, track, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_philox_normal(uint64_t seed, uint32_t k, int64_t elem_offset, int64_t n, float *out, void *stream) {
  SF_API_BEGIN
  if (!out || n < 1 || elem_offset < 0 || elem_offset > INT64_MAX - n) fail(SF_ERR_INVALID, "bad argument");
  SF_HIP(launch_philox_normal(seed, k, elem_offset, n, out, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_vinpaint_update(float *x, const float *v, const float *v_uncond, float scale, const float *source, const uint8_t *mask, const float *sched,
                          const int32_t *step_idx, const uint32_t *seed, int64_t e0, int64_t e1, void *stream) {
  SF_API_BEGIN
  if (!x || !v || !source || !mask || !sched || !step_idx || !seed || e0 < 0 || e1 < e0) fail(SF_ERR_INVALID, "bad argument");
  SF_HIP(launch_vinpaint_update(x, v, v_uncond, scale, source, mask, sched, step_idx, 0, seed, e0, e1, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_vsampler_update_ms(float *x, const float *v, const float *v_uncond, float scale, float *hist, const float *table, const int32_t *step_idx,
                             int64_t e0, int64_t e1, void *stream) {
  SF_API_BEGIN
  if (!x || !v || !hist || !table || !step_idx || e0 < 0 || e1 < e0) fail(SF_ERR_INVALID, "bad argument");
  SF_HIP(launch_vsampler_update_ms(x, v, v_uncond, scale, hist, table, step_idx, 0, e0, e1, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int64_t sf_op_guidance_stats_bytes(int B, int64_t clip_len) {
  if (B < 1 || clip_len < 1) return -1;
  return (int64_t)B * guidance_stats_blocks(clip_len) * 6 * (int64_t)sizeof(double);
}

int sf_op_guidance_stats(const float *v, const float *v_uncond, const float *gtab, const int32_t *step_idx, int B, int64_t clip_len, void *part,
                         int64_t part_bytes, void *stream) {
  SF_API_BEGIN
  if (!v || !gtab || !step_idx || !part || B < 1 || clip_len < 1) fail(SF_ERR_INVALID, "bad argument");
  if ((reinterpret_cast<uintptr_t>(part) & 7) != 0) fail(SF_ERR_INVALID, "partials buffer is not 8-byte aligned");
  if (part_bytes < sf_op_guidance_stats_bytes(B, clip_len)) fail(SF_ERR_WORKSPACE, "partials buffer too small");
  SF_HIP(launch_guidance_stats(v, v_uncond, gtab, step_idx, 0, B, clip_len, static_cast<double *>(part), static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_vsampler_update_g(float *x, const float *v, const float *v_uncond, float *hist, const float *table, const float *gtab,
                            const int32_t *step_idx, const void *part, float rescale, int B, int64_t clip_len, float *factor_out, int64_t e0,
                            int64_t e1, void *stream) {
  SF_API_BEGIN
  if (!x || !v || !hist || !table || !gtab || !step_idx || B < 1 || clip_len < 1 || e0 < 0 || e1 < e0) fail(SF_ERR_INVALID, "bad argument");
  if (e1 > (int64_t)B * clip_len) fail(SF_ERR_INVALID, "the range ends past the last clip");
  if (!(rescale >= 0.0f && rescale <= 1.0f)) fail(SF_ERR_INVALID, "rescale must be inside [0, 1]");
  if (rescale > 0.0f && (!part || (reinterpret_cast<uintptr_t>(part) & 7) != 0)) fail(SF_ERR_INVALID, "rescale > 0 needs the partials of sf_op_guidance_stats");
  SF_HIP(launch_vsampler_update_g(x, v, v_uncond, hist, table, gtab, step_idx, 0, static_cast<const double *>(part), rescale, B, clip_len, factor_out,
                                  e0, e1, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_cut_prefix_crop(const float *gen, const float *y, int B, int C, int L, int cut_length, float *out, int32_t *first_onset, void *stream) {
  SF_API_BEGIN
  if (!gen || !y || !out || !first_onset || B < 1 || C < 1 || L < 1 || cut_length < 1 || cut_length > L) fail(SF_ERR_INVALID, "bad argument");
  SF_HIP(launch_cut_prefix_crop(gen, y, B, C, L, cut_length, out, first_onset, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

}  // extern "C"

#include <vector>
namespace sf {
void resample_bank(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, std::vector<float> &bank, int &orig,
                   int &nnew, int &width);
}
struct sf_resampler {
  int orig = 1, nnew = 1, width = 0;
  float *bank = nullptr;
  ~sf_resampler() {
    if (bank) (void)hipFree(bank);
  }
};

extern "C" {

int sf_resampler_create(int orig_freq, int new_freq, int lowpass_filter_width, float rolloff, sf_resampler **out) {
  SF_API_BEGIN
  if (!out || orig_freq < 1 || new_freq < 1 || lowpass_filter_width < 1 || !(rolloff > 0.f && rolloff <= 1.f)) fail(SF_ERR_INVALID, "bad argument");
  *out = nullptr;
  std::vector<float> bank;
  auto *h = new sf_resampler();
  // rolloff arrives as a C float; the reference passes the Python double 0.99 -- use the nearest double of the decimal
  const double ro = std::round((double)rolloff * 1e6) / 1e6;
  resample_bank(orig_freq, new_freq, lowpass_filter_width, ro, bank, h->orig, h->nnew, h->width);
  hipError_t e = hipMalloc(&h->bank, bank.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(h->bank, bank.data(), bank.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    delete h;
    fail(SF_ERR_HIP, "resampler bank upload: %s", hipGetErrorString(e));
  }
  *out = h;
  return SF_OK;
  SF_API_END
}
void sf_resampler_destroy(sf_resampler *h) { delete h; }
int sf_resampler_out_length(const sf_resampler *h, int L) {
  if (!h || L < 0) return -1;
  return (int)(((int64_t)h->nnew * L + h->orig - 1) / h->orig);   // ceil(new * L / orig)
}
int sf_resampler_forward(sf_resampler *h, const float *x, int R, int L, float *out, void *stream) {
  SF_API_BEGIN
  if (!h || !x || !out || R < 1 || L < 1) fail(SF_ERR_INVALID, "bad argument");
  SF_HIP(launch_resample(x, R, L, h->bank, h->orig, h->nnew, h->width, out, sf_resampler_out_length(h, L), static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

// (dgp: the training forward also writes the data-gradient images of the weight, [C][taps][N] fp32 then its split bf16 image, for
// sf_op_conv1d_bwd_cl_p -- one pack launch per weight and step instead of one per GEMM)
// (prepacked: the images come from sf_train_pack_many -- pk_fw / pk_fwx as sf_op_conv1d_train_images says; nothing is packed here.
//  images_out: query only -- which images would the training forward (with / without a data gradient) read?  Nothing is launched.
//  label_out: query only -- the label of the launch these arguments end in (sf_op_conv1d_variant).  The ConvGemmArgs are finished by the
//  same statements as for a real call: every image is a probe pointer where the real call allocates it, and nothing is launched.)
enum { IMG_FW = 1, IMG_FWX = 2, IMG_DG = 4, IMG_DGX = 8, IMG_UNPLANNABLE = 16 };
static int conv1d_cl_impl(int dtype, const void *x, const float *w, const float *bias, const float *gamma, const float *beta, int groups,
                          float eps, const void *residual, int B, int L, int C, int N, int taps, int stride, int pad, int upsample,
                          void *out, void *ws, int64_t ws_bytes, void *stream, void *dgp, bool prepacked = false, const float *pk_fw = nullptr,
                          const void *pk_fwx = nullptr, int *images_out = nullptr, const char **label_out = nullptr) {
  SF_API_BEGIN
  const bool query = images_out || label_out;
  if (!query && (!x || !w || !out || !ws)) fail(SF_ERR_INVALID, "null argument");
  if (upsample < 1 || (upsample & (upsample - 1))) fail(SF_ERR_UNSUPPORTED, "upsample must be a power of two");
  hipStream_t s = static_cast<hipStream_t>(stream);
  Workspace wk(ws, ws_bytes);
  // a weight image: workspace for a real call, a probe pointer for the label query (the decisions depend on which images exist, not on their contents)
  auto image = [&](int64_t bytes) -> void * { return label_out ? reinterpret_cast<void *>(16) : wk.alloc(bytes); };
  const bool x3 = dtype == SF_F32X;   // fp32 tensors, products from split fp16 operands (needs N * K * 4 more bytes of workspace)
  if (x3) dtype = F32;
  const bool direct = (C % 32) != 0;
  if (direct && N > 32) fail(SF_ERR_UNSUPPORTED, "thin convolution with N > 32");
  const int wdt = direct ? F32 : dtype;
  const int K = taps * C;
  // ---- the launch, without its weight images ---------------------------------------------------------------------------------------------
  ConvGemmArgs a;
  a.src = x;
  a.src_ld = C;
  a.bias = bias;
  a.N = N;
  a.K = K;
  a.cin = C;
  a.taps = taps;
  a.stride = stride;
  a.pad = pad;
  while ((1 << a.up_shift) < upsample) ++a.up_shift;
  a.Lsrc = L;
  a.Lout = (L * upsample + 2 * pad - taps) / stride + 1;
  a.M = B * a.Lout;
  a.out = out;
  a.out_ld = N;
  a.n_store = N;
  a.res = residual;
  a.res_ld = N;
  a.solo = 1;   // op-level entry (the training step's single stream)
  if (groups > 0) {
    GnPlan gp = gn_plan(B, L, C);
    float *slab = query ? nullptr : wk.alloc_n<float>((int64_t)B * gp.nch * groups * 2);
    if (!query) SF_HIP(launch_gn_stats(dtype, x, C, B, L, C, groups, gp.nch, gp.chunk_rows, slab, s));
    a.pro = 1;
    a.G = groups;
    a.nch = gp.nch;
    a.chunk_rows = gp.chunk_rows;
    a.stats = slab;
    a.gamma = gamma;
    a.beta = beta;
    a.eps = eps;
  }
  // ---- weight images -------------------------------------------------------------------------------------------------------------------------
  const void *wp = w;   // fp32 1x1 convolutions: the PyTorch layout (N, C, 1) IS the GEMM's [N][K] (60 % of the training step's convolutions)
  // (the kernels read weights as 16-byte vectors: a view at a storage offset that is not a multiple of 4 floats is packed like the rest)
  const bool need_fw = !(taps == 1 && wdt == F32 && (reinterpret_cast<uintptr_t>(w) % 16) == 0);
  const bool wx_ok = x3 && !direct && (K % 32) == 0;
  // fragment order for the register-staged kernel, as the engine packs it -- but only when THIS launch would take that kernel (the long rows
  // of the training step go to the macro tiles: 131 of these packs per step were written and never read)
  bool want_rs = false;
  if (wx_ok && groups == 0 && (K % 64) == 0 && K <= 1280 && (N % 32) == 0 && (C % 16) == 0) {
    ConvGemmArgs pa = a;
    pa.w = pa.wx = pa.wfrx = &pa;   // every image exists (only whether one does enters the plan)
    want_rs = conv_gemm_plan(dtype, pa).family == CG_RS;
  }
  void *wx_done = nullptr;
  // which images the training step reads of this weight: the fp32 [N][K] matrix only where the chosen kernel is not a split-operand one
  // (or the fragment-order pack needs it as its source), likewise the fp32 data-gradient matrix
  const bool fw_read = !wx_ok || want_rs || !conv_gemm_reads_split_only(dtype, a);
  const bool dgx_ok = conv1d_dgrad_split_ok(x3, N, taps);
  const bool dg_read = !dgx_ok || !conv_gemm_reads_split_only(F32, conv1d_dgrad_args(nullptr, B, L, C, N, taps, pad, nullptr));
  if (images_out) {
    *images_out = (need_fw && fw_read ? IMG_FW : 0) | (wx_ok ? IMG_FWX : 0) | (dg_read ? IMG_DG : 0) | (dgx_ok ? IMG_DGX : 0) |
                  (want_rs || dtype != F32 || stride != 1 || upsample != 1 || taps > 9 ? IMG_UNPLANNABLE : 0);
    return SF_OK;
  }
  if (prepacked) {   // images written by sf_train_pack_many at the start of the step
    if (want_rs || dtype != F32) fail(SF_ERR_UNSUPPORTED, "prepacked images: not for this launch (sf_op_conv1d_train_images says so)");
    if ((need_fw && fw_read && !pk_fw) || (wx_ok && !pk_fwx)) fail(SF_ERR_INVALID, "prepacked images missing (see sf_op_conv1d_train_images)");
    if (need_fw) wp = fw_read ? pk_fw : nullptr;
    wx_done = const_cast<void *>(pk_fwx);
    if (!wx_ok) wx_done = nullptr;
  } else if (dgp) {   // training forward (fp32 tensors): every image of this weight the step reads, in one launch, and only those
    if (dtype != F32 || stride != 1 || upsample != 1 || taps > 9) fail(SF_ERR_UNSUPPORTED, "data-gradient images: fp32 / fp32x stride-1 convolutions of at most 9 taps");
    float *fw = need_fw && fw_read ? wk.alloc_n<float>((int64_t)N * K) : nullptr;
    if (wx_ok) wx_done = wk.alloc((int64_t)N * K * 4);
    float *dg = static_cast<float *>(dgp);
    void *dgx = dgx_ok ? static_cast<void *>(dg + (int64_t)C * taps * N) : nullptr;
    SF_HIP(launch_pack_train(w, N, C, taps, fw, wx_done, dg_read ? dg : nullptr, dgx, s));
    if (fw) wp = fw;
    else if (need_fw) wp = nullptr;   // nobody reads it
  } else if (need_fw) {
    void *packed = image((int64_t)N * K * dsize(wdt));
    if (wx_ok) {   // fp32 matrix and its split image in one pass
      wx_done = image((int64_t)N * K * 4);
      if (!label_out) SF_HIP(launch_pack_conv_x(w, N, C, taps, static_cast<float *>(packed), wx_done, X3_F16, s));
    } else if (!label_out) {
      SF_HIP(launch_pack_conv(wdt, w, N, C, 0, C, taps, C, nullptr, packed, K, 0, s));
    }
    wp = packed;
  }
  if (!direct && dtype != F32 && (K % 64) == 0 && K <= 2048 && (N % 32) == 0 && (C % 16) == 0) {   // as the engine packs it (conv_gemm_rs.hip)
    void *wfr = image((int64_t)N * K * dsize(wdt));
    if (!label_out) SF_HIP(launch_pack_wfr(dtype, wp, N, K, wfr, s));
    a.wfr = wfr;
  }
  if (wx_done) a.wx = wx_done;
  else if (wx_ok) {
    void *wx = image((int64_t)N * K * 4);
    if (!label_out) SF_HIP(launch_pack_wx(static_cast<const float *>(wp), N, K, wx, s));
    a.wx = wx;
  }
  a.w = wp;
  if (want_rs) {
    void *wfrx = image((int64_t)N * K * 4);
    if (!label_out) SF_HIP(launch_pack_wfrx(static_cast<const float *>(wp), N, K, wfrx, s));
    a.wfrx = wfrx;
  }
  const ConvGemmPlan pl = direct ? ConvGemmPlan() : conv_gemm_plan(dtype, a);
  if (label_out) {   // the ConvGemmArgs are finished: name the launch below instead of making it
    if (!direct && !conv_gemm_supported(dtype, a)) fail(SF_ERR_UNSUPPORTED, "no GEMM kernel takes this shape");
    *label_out = direct ? "conv_direct" : pl.label;
    return SF_OK;
  }
  if (direct) SF_HIP(launch_conv_direct(dtype, dtype, a, s));
  else SF_HIP(launch_conv_gemm_planned(dtype, a, pl, s));
  return SF_OK;
  SF_API_END
}

int sf_op_conv1d_cl(int dtype, const void *x, const float *w, const float *bias, const float *gamma, const float *beta, int groups,
                    float eps, const void *residual, int B, int L, int C, int N, int taps, int stride, int pad, int upsample,
                    void *out, void *ws, int64_t ws_bytes, void *stream) {
  return conv1d_cl_impl(dtype, x, w, bias, gamma, beta, groups, eps, residual, B, L, C, N, taps, stride, pad, upsample, out, ws, ws_bytes, stream, nullptr);
}

int64_t sf_op_conv1d_dgrad_pack_bytes(int C, int N, int taps) {
  if (C < 1 || N < 1 || taps < 1 || taps > 9) return -1;
  return (int64_t)C * taps * N * 8;   // the fp32 matrix and its split bf16 image
}

int sf_op_conv1d_train_fwd(int dtype, const float *x, const float *w, const float *bias, const float *gamma, const float *beta, int groups, float eps,
                           const float *residual, int B, int L, int C, int N, int taps, int pad, float *out, void *dgrad_pack, int64_t dgrad_pack_bytes,
                           void *ws, int64_t ws_bytes, void *stream) {
  if (dtype != SF_F32 && dtype != SF_F32X) {
    set_error("sf_op_conv1d_train_fwd: dtype must be SF_F32 or SF_F32X");
    return SF_ERR_INVALID;
  }
  if (dgrad_pack && dgrad_pack_bytes < sf_op_conv1d_dgrad_pack_bytes(C, N, taps)) {
    set_error("sf_op_conv1d_train_fwd: dgrad_pack holds %lld bytes, %lld needed", (long long)dgrad_pack_bytes, (long long)sf_op_conv1d_dgrad_pack_bytes(C, N, taps));
    return SF_ERR_INVALID;
  }
  return conv1d_cl_impl(dtype, x, w, bias, gamma, beta, groups, eps, residual, B, L, C, N, taps, 1, pad, 1, out, ws, ws_bytes, stream, dgrad_pack);
}

int sf_op_conv1d_train_images(int dtype, const float *w, int B, int L, int C, int N, int taps, int pad, int groups) {
  if (dtype != SF_F32 && dtype != SF_F32X) {
    set_error("sf_op_conv1d_train_images: dtype must be SF_F32 or SF_F32X");
    return -1;
  }
  int mask = 0;
  const int rc = conv1d_cl_impl(dtype, nullptr, w, nullptr, nullptr, nullptr, groups, 0.f, nullptr, B, L, C, N, taps, 1, pad, 1, nullptr, nullptr, 0, nullptr, nullptr,
                                false, nullptr, nullptr, &mask);
  return rc == SF_OK ? mask : -1;
}

int sf_op_conv1d_variant(int dtype, int B, int L, int C, int N, int taps, int stride, int pad, int upsample, int groups, char *label, int label_bytes) {
  if (!label || label_bytes < 1) {
    set_error("sf_op_conv1d_variant: no room for the label");
    return SF_ERR_INVALID;
  }
  label[0] = 0;
  if (B < 1 || L < 1 || C < 1 || N < 1 || taps < 1 || stride < 1 || pad < 0 || groups < 0 || upsample < 1 || (int64_t)L * upsample + 2 * pad < taps) {
    set_error("sf_op_conv1d_variant: bad geometry");
    return SF_ERR_INVALID;
  }
  const char *name = nullptr;
  const float *probe = reinterpret_cast<const float *>(16);   // an aligned weight, as a tensor's storage is
  const int rc = conv1d_cl_impl(dtype, nullptr, probe, nullptr, nullptr, nullptr, groups, 0.f, nullptr, B, L, C, N, taps, stride, pad, upsample, nullptr, nullptr, 0,
                                nullptr, nullptr, false, nullptr, nullptr, nullptr, &name);
  if (rc != SF_OK) return rc;
  snprintf(label, (size_t)label_bytes, "%s", name);
  return SF_OK;
}

int sf_train_pack_many(const void *desc_dev, int n_items, int total_tiles, void *stream) {
  SF_API_BEGIN
  SF_HIP(launch_pack_train_many(desc_dev, n_items, total_tiles, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_conv1d_train_fwd_pk(int dtype, const float *x, const float *w, const float *fw, const void *fwx, const float *bias, const float *gamma,
                              const float *beta, int groups, float eps, const float *residual, int B, int L, int C, int N, int taps, int pad, float *out,
                              void *ws, int64_t ws_bytes, void *stream) {
  if (dtype != SF_F32 && dtype != SF_F32X) {
    set_error("sf_op_conv1d_train_fwd_pk: dtype must be SF_F32 or SF_F32X");
    return SF_ERR_INVALID;
  }
  return conv1d_cl_impl(dtype, x, w, bias, gamma, beta, groups, eps, residual, B, L, C, N, taps, 1, pad, 1, out, ws, ws_bytes, stream, nullptr, true, fw, fwx);
}

int sf_op_gn_silu(int dtype, const void *x, const float *gamma, const float *beta, int groups, float eps, int B, int L, int C, void *out,
                  void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!x || !gamma || !beta || !out) fail(SF_ERR_INVALID, "null argument");
  if (groups < 1 || C % groups) fail(SF_ERR_INVALID, "channels must be divisible by groups");
  SF_HIP(launch_gn_silu_ws(dtype, x, C, B, L, C, groups, gamma, beta, eps, out, C, static_cast<float *>(ws), ws ? ws_bytes / 4 : 0,
                           static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_bench_conv1d(int dtype, int B, int L, int C, int N, int taps, int upsample, int path, int tile, int sk, int iters, float *ms_out) {
  SF_API_BEGIN
  if (!ms_out || iters < 1) fail(SF_ERR_INVALID, "bad argument");
  const bool x3 = dtype == SF_F32X;
  if (x3) dtype = F32;
  const size_t es = dsize(dtype);
  const int K = taps * C, Lout = L * upsample, M = B * Lout;
  void *x = nullptr, *w = nullptr, *out = nullptr, *res = nullptr;
  float *bias = nullptr;
  SF_HIP(hipMalloc(&x, (size_t)B * L * C * es));
  // SF_BENCH_COLD=1: rotate through enough weight copies (> 768 MB) that every launch streams its weights from HBM,
  // as inside a denoising step (430 MB of weights per step do not fit the 256 MB Infinity Cache)
  const size_t wbytes = (size_t)N * K * es;
  int ncopy = 1;
  if (const char *e = tune_env("SF_BENCH_COLD")) {
    if (atoi(e) > 0) ncopy = (int)std::min<size_t>(1024, ((size_t)768 << 20) / wbytes + 1);
  }
  SF_HIP(hipMalloc(&w, wbytes * ncopy));
  SF_HIP(hipMalloc(&out, (size_t)M * N * es));
  SF_HIP(hipMalloc(&res, (size_t)M * N * es));
  SF_HIP(hipMalloc(&bias, N * sizeof(float)));
  // non-trivial bit patterns (zero operands clock higher): bf16/f32 values around +-1
  SF_HIP(hipMemset(x, 0x3c, (size_t)B * L * C * es));
  SF_HIP(hipMemset(w, 0xbc, wbytes * ncopy));
  SF_HIP(hipMemset(res, 0x3d, (size_t)M * N * es));
  SF_HIP(hipMemset(bias, 0, N * sizeof(float)));
  ConvGemmArgs a;
  a.src = x;
  a.src_ld = C;
  a.w = w;
  a.bias = bias;
  a.N = N;
  a.K = K;
  a.cin = C;
  a.taps = taps;
  a.pad = taps / 2;
  while ((1 << a.up_shift) < upsample) ++a.up_shift;
  a.Lsrc = L;
  a.Lout = Lout;
  a.M = M;
  a.out = out;
  a.out_ld = N;
  a.n_store = N;
  a.res = res;
  a.res_ld = N;
  g_conv_gemm_force.path = path;
  g_conv_gemm_force.tile = tile;
  g_conv_gemm_force.sk = sk;
  hipEvent_t e0, e1;
  SF_HIP(hipEventCreate(&e0));
  SF_HIP(hipEventCreate(&e1));
  hipError_t err = hipSuccess;
  unsigned *sink = nullptr;   // the touch kernel's dedicated write sink (never a live buffer)
  void *wfr = nullptr;
  if (dtype != F32 && (K % 64) == 0 && K <= 2048 && (N % 32) == 0 && (C % 16) == 0 && !tune_env("SF_BENCH_NO_WFR")) {
    SF_HIP(hipMalloc(&wfr, wbytes * ncopy));   // fragment-ordered copies, same rotation (the values are random either way)
    SF_HIP(hipMemcpy(wfr, w, wbytes * ncopy, hipMemcpyDeviceToDevice));
    a.wfr = wfr;
  }
  void *wx = nullptr;
  if (x3) {   // split-fp16 images of the same rotation of weight copies
    if (K % 32) fail(SF_ERR_UNSUPPORTED, "fp32x needs K %% 32 == 0");
    SF_HIP(hipMalloc(&wx, wbytes * ncopy));
    for (int c = 0; c < ncopy; ++c)
      SF_HIP(launch_pack_wx(reinterpret_cast<const float *>(static_cast<char *>(w) + (size_t)c * wbytes), N, K, static_cast<char *>(wx) + (size_t)c * wbytes, nullptr));
    a.wx = wx;
  }
  for (int i = 0; i < 3 && err == hipSuccess; ++i) err = launch_conv_gemm(dtype, a, nullptr);
  if (err == hipSuccess) {
    SF_HIP(hipDeviceSynchronize());
    SF_HIP(hipEventRecord(e0, nullptr));
    // SF_BENCH_PREFETCH=n: a `touch` kernel of n workgroups reads this launch's weights right before it (1000 + n: the touch kernel
    // alone) -- what an idle-CU prefetch in the PRECEDING kernel of the chain could buy
    int pre = 0;
    if (const char *e = tune_env("SF_BENCH_PREFETCH")) pre = atoi(e);
    if (pre > 0 && pre % 1000 == 0) fail(SF_ERR_INVALID, "SF_BENCH_PREFETCH=%d: the workgroup count (value mod 1000) must be >= 1", pre);
    if (pre > 0) SF_HIP(hipMalloc(reinterpret_cast<void **>(&sink), 64));
    for (int i = 0; i < iters && err == hipSuccess; ++i) {
      a.w = static_cast<char *>(w) + (size_t)(i % ncopy) * wbytes;
      if (wfr) a.wfr = static_cast<char *>(wfr) + (size_t)(i % ncopy) * wbytes;
      if (wx) a.wx = static_cast<char *>(wx) + (size_t)(i % ncopy) * wbytes;
      if (pre > 0) err = launch_touch(a.w, wbytes, pre % 1000, sink, nullptr);
      if (pre < 1000 && err == hipSuccess) err = launch_conv_gemm(dtype, a, nullptr);
    }
    SF_HIP(hipEventRecord(e1, nullptr));
    SF_HIP(hipEventSynchronize(e1));
    SF_HIP(hipEventElapsedTime(ms_out, e0, e1));
    *ms_out /= (float)iters;
  }
  g_conv_gemm_force = ConvGemmForce();
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  for (void *p : {x, w, out, res, (void *)bias}) (void)hipFree(p);
  if (sink) (void)hipFree(sink);
  if (wfr) (void)hipFree(wfr);
  if (wx) (void)hipFree(wx);
  if (err != hipSuccess) fail(SF_ERR_UNSUPPORTED, "variant not applicable: %s", hipGetErrorString(err));
  return SF_OK;
  SF_API_END
}

int64_t sf_op_resnet_mod_cb_workspace_bytes(int B, int L, int C) {
  Workspace dry(nullptr, 0);
  const int64_t M = (int64_t)B * L;
  dry.alloc(2 * (int64_t)C * C * 3 * 4);   // (sized for SF_F32X: 4 bytes per weight / activation)
  dry.alloc(M * C * 4);
  dry.alloc(M * C * 4);
  dry.alloc((int64_t)(C / 128) * M * C * 4);
  dry.alloc((int64_t)B * 32 * 64 * 2 * 4);
  return dry.used();
}

int sf_op_resnet_mod_cb(int dtype, const void *x, const float *w1, const float *b1, const float *w2, const float *b2, const float *gn1_g,
                        const float *gn1_b, const float *gn2_g, const float *gn2_b, int groups, float eps_gn, const float *scale_shift, float eps_ln,
                        int B, int L, int C, int kb, void *h_out, void *m_out, void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (kb != 1 && kb != 2) fail(SF_ERR_INVALID, "kb must be 1 or 2");
  if (!x || !w1 || !b1 || !w2 || !b2 || !gn1_g || !gn1_b || !gn2_g || !gn2_b || !m_out || !ws) fail(SF_ERR_INVALID, "null argument");
  if (!conv_cb_shape_ok(dtype, B, L, C, C, groups) || groups > 64) fail(SF_ERR_UNSUPPORTED, "shape outside the channel-block convolution's coverage");
  hipStream_t s = static_cast<hipStream_t>(stream);
  Workspace wk(ws, ws_bytes);
  const int64_t M = (int64_t)B * L;
  const int S = C / 128 / kb;
  if (kb == 2 && ((C / 128) % 2 || C / groups < 32)) fail(SF_ERR_UNSUPPORTED, "two channel blocks per workgroup need C a multiple of 256 and >= 32 channels per group");
  if (kb == 2 && dtype == SF_F32X) fail(SF_ERR_UNSUPPORTED, "the split-operand form takes one channel block per workgroup");
  const int64_t es = (int64_t)dsize(dtype);
  const int adt = dtype == SF_F32X ? (int)F32 : dtype;   // activations / reducers of the fp32x chain are plain fp32
  char *wp = static_cast<char *>(wk.alloc(2 * (int64_t)C * C * 3 * es));
  void *wp1 = wp, *wp2 = wp + (int64_t)C * C * 3 * es;
  void *act = wk.alloc(M * C * es);
  void *h = h_out ? h_out : wk.alloc(M * C * es);
  float *slab = static_cast<float *>(wk.alloc((int64_t)S * M * C * 4));
  float *stats = static_cast<float *>(wk.alloc((int64_t)B * 32 * 64 * 2 * 4));
  SF_HIP(launch_pack_conv_cb(dtype, w1, C, C, wp1, s));
  SF_HIP(launch_pack_conv_cb(dtype, w2, C, C, wp2, s));
  SF_HIP(launch_gn_silu(adt, x, C, B, L, C, groups, gn1_g, gn1_b, eps_gn, act, C, s));
  ConvCbArgs a;
  a.src = act;
  a.src_ld = C;
  a.wp = wp1;
  a.slab = slab;
  a.B = B;
  a.L = L;
  a.C = a.N = C;
  a.kb = kb;
  SF_HIP(launch_conv_cb(dtype, a, s));
  const CbGnPlan gp = cb_gn_plan(L);
  SF_HIP(launch_cb_reduce_gn(adt, slab, S, B, L, C, b1, h, C, groups, stats, gp, s));
  a.src = h;
  a.wp = wp2;
  a.pro = 1;
  a.G = groups;
  a.nch = gp.nch;
  a.chunk_rows = gp.chunk_rows;
  a.stats = stats;
  a.gamma = gn2_g;
  a.beta = gn2_b;
  a.eps = eps_gn;
  SF_HIP(launch_conv_cb(dtype, a, s));
  SF_HIP(launch_cb_reduce_ln(adt, slab, S, B, L, C, b2, x, C, scale_shift, 2 * C, eps_ln, m_out, C, s));
  return SF_OK;
  SF_API_END
}

int64_t sf_op_resnet_mod_cbd_workspace_bytes(int B, int L, int C, int C2) {
  if (B < 1 || L < 1 || C < 1 || C2 < 0) return -1;
  Workspace dry(nullptr, 0);
  const int64_t M = (int64_t)B * L;
  dry.alloc(2 * (int64_t)C * C * 3 * 2);     // the two fragment-ordered convolution weights
  dry.alloc(M * C * 2);                      // SiLU(GroupNorm(x))
  dry.alloc(M * C * 2);                      // h (when the caller does not ask for it)
  dry.alloc(M * C * 2);                      // m (likewise)
  dry.alloc((int64_t)B * 32 * 64 * 2 * 4);   // chunk statistics (likewise)
  dry.alloc((int64_t)C * (C + C2) * 2);      // InjectChannels weights
  return dry.used();
}

int sf_op_resnet_mod_cbd(int dtype, const void *x, const float *w1, const float *b1, const float *w2, const float *b2, const float *gn1_g,
                         const float *gn1_b, const float *gn2_g, const float *gn2_b, int groups, float eps_gn, const float *scale_shift, float eps_ln,
                         int B, int L, int C, const float *w_inj, const float *b_inj, const void *ctx, int ctx_ld, int C2, const float *badd,
                         void *h_out, void *m_out, void *z_out, float *stats_out, void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!x || !w1 || !b1 || !w2 || !b2 || !gn1_g || !gn1_b || !gn2_g || !gn2_b || !ws) fail(SF_ERR_INVALID, "null argument");
  if (!m_out && !(w_inj && z_out)) fail(SF_ERR_INVALID, "no output requested");
  if (w_inj && (!b_inj || !z_out || C2 < 0 || (C2 > 0 && (!ctx || ctx_ld < C2)))) fail(SF_ERR_INVALID, "InjectChannels operands incomplete");
  // every refusal comes before the first launch: a refused call writes nothing
  if (groups < 1 || groups > 64 || !conv_cb_direct_ok(dtype, B, L, C, C, groups))
    fail(SF_ERR_UNSUPPORTED, "shape outside the direct channel-block epilogues' coverage (16-bit, C = 128, L a multiple of 32, L <= 1024)");
  const int64_t M = (int64_t)B * L;
  ConvGemmArgs ai;   // InjectChannels on the modulated rows: the plain GEMM, as the engine launches it behind the direct chain
  if (w_inj) {
    if (C2 % 32 || ctx_ld % 8) fail(SF_ERR_UNSUPPORTED, "C2 must be a multiple of 32 and ctx_ld of 8");
    ai.src_ld = C;
    ai.src2 = C2 ? ctx : nullptr;
    ai.src2_ld = ctx_ld;
    ai.bias = b_inj;
    ai.M = (int)M;
    ai.N = ai.n_store = C;
    ai.K = C + C2;
    ai.cin = C;
    ai.cin2 = C2;
    ai.taps = 1;
    ai.Lout = ai.Lsrc = L;
    ai.out = z_out;
    ai.out_ld = C;
    ai.res_ld = C;
    ai.short_k = 1;
    if (badd) {
      ai.badd = badd;
      ai.badd_ld = C;
    }
  }
  const int64_t need = sf_op_resnet_mod_cbd_workspace_bytes(B, L, C, w_inj ? C2 : 0);
  if (need < 0 || ws_bytes < need) fail(SF_ERR_WORKSPACE, "workspace too small: need %lld bytes", (long long)need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  Workspace wk(ws, ws_bytes);
  const int64_t es = 2;
  char *wp = static_cast<char *>(wk.alloc(2 * (int64_t)C * C * 3 * es));
  void *wp1 = wp, *wp2 = wp + (int64_t)C * C * 3 * es;
  void *act = wk.alloc(M * C * es);
  void *h = h_out ? h_out : wk.alloc(M * C * es);
  void *m = m_out ? m_out : wk.alloc(M * C * es);
  float *stats = stats_out ? stats_out : static_cast<float *>(wk.alloc((int64_t)B * 32 * 64 * 2 * 4));
  if (w_inj) {
    void *wi = wk.alloc((int64_t)C * (C + C2) * es);
    ai.w = wi;
    ai.src = ai.res = m;
    if (!conv_gemm_supported(dtype, ai)) fail(SF_ERR_UNSUPPORTED, "InjectChannels shape outside the GEMM kernels' coverage");
    SF_HIP(launch_pack_rows(dtype, w_inj, C, C + C2, C + C2, nullptr, wi, C + C2, s));
  }
  SF_HIP(launch_pack_conv_cb(dtype, w1, C, C, wp1, s));
  SF_HIP(launch_pack_conv_cb(dtype, w2, C, C, wp2, s));
  SF_HIP(launch_gn_silu(dtype, x, C, B, L, C, groups, gn1_g, gn1_b, eps_gn, act, C, s));
  ConvCbArgs a;
  a.src = act;
  a.src_ld = C;
  a.wp = wp1;
  a.B = B;
  a.L = L;
  a.C = a.N = C;
  a.G = groups;
  const CbGnPlan gp = cb_gn_plan(L);
  a.nch = gp.nch;
  a.chunk_rows = gp.chunk_rows;
  a.epi = 1;   // direct_gn: h and its chunk statistics
  a.out = h;
  a.out_ld = C;
  a.bias = b1;
  a.stats_out = stats;
  SF_HIP(launch_conv_cb(dtype, a, s));
  a.src = h;
  a.wp = wp2;
  a.pro = 1;
  a.stats = stats;
  a.gamma = gn2_g;
  a.beta = gn2_b;
  a.eps = eps_gn;
  a.epi = 2;   // direct_ln: + bias + x, LayerNorm, Modulation
  a.out = m;
  a.bias = b2;
  a.stats_out = nullptr;
  a.res = x;
  a.res_ld = C;
  a.ss = scale_shift;
  a.ss_ld = 2 * C;
  a.eps_ln = eps_ln;
  SF_HIP(launch_conv_cb(dtype, a, s));
  if (w_inj) SF_HIP(launch_conv_gemm(dtype, ai, s));
  return SF_OK;
  SF_API_END
}

int64_t sf_op_thin_tail_workspace_bytes(int dtype, int C, int C2) {
  if ((dtype != F32 && dtype != BF16 && dtype != F16) || C < 1 || C2 < 0) return -1;
  Workspace dry(nullptr, 0);
  dry.alloc((int64_t)C * 3 * C * (int64_t)dsize(dtype));      // conv2 weights, packed [C][3 C]
  dry.alloc((int64_t)C * (C + C2) * (int64_t)dsize(dtype));   // InjectChannels weights, packed [C][C + C2]
  return dry.used();
}

int sf_op_thin_tail(int dtype, const void *h, const void *x, const void *ctx, int ctx_ld, int c2_real, int C2, const float *stats_in, int nch_in,
                    int chunk_in, const float *w2, const float *b2, const float *gn_g, const float *gn_b, int groups, float eps_gn,
                    const float *scale_shift, float eps_ln, const float *w_inj, const float *b_inj, const float *badd, int B, int L, int C, int rw,
                    void *z_out, float *stats_out, int *rw_out, void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!h || !x || !stats_in || !w2 || !b2 || !gn_g || !gn_b || !scale_shift || !w_inj || !b_inj || !z_out || !ws) fail(SF_ERR_INVALID, "null argument");
  if (dtype != F32 && dtype != BF16 && dtype != F16) fail(SF_ERR_UNSUPPORTED, "dtype: fp32, bf16 or fp16");
  if (B < 1 || L < 1 || C < 8) fail(SF_ERR_INVALID, "bad shape");
  if (C2 < 0 || C2 % 8 || c2_real < 0 || c2_real > C2 || (C2 > 0 && (!ctx || ctx_ld < C2 || ctx_ld % 8))) fail(SF_ERR_INVALID, "context operands inconsistent");
  // the chunks of the input statistics tile the clip exactly: the last one is short, none is empty
  if (nch_in < 1 || chunk_in < 1 || (int64_t)(nch_in - 1) * chunk_in >= L || (int64_t)nch_in * chunk_in < L)
    fail(SF_ERR_INVALID, "nch_in chunks of chunk_in rows do not tile L = %d", L);
  if (rw < 0 || rw % 32) fail(SF_ERR_UNSUPPORTED, "rw must be a multiple of 32 (0: the plan's choice)");
  ThinTailArgs t;
  if (rw == 0) rw = conv_thin_plan(B, L, C).rw;
  t.rw = rw;
  t.nchw = (L + rw - 1) / rw;
  t.h = h;
  t.x = x;
  t.ctx = ctx;
  t.ctx_ld = ctx_ld;
  t.bias2 = b2;
  t.bias3 = b_inj;
  t.gamma = gn_g;
  t.beta = gn_b;
  t.stats_in = stats_in;
  t.ss = scale_shift;
  t.ss_ld = 2 * C;
  t.badd = badd;
  t.badd_ld = C;
  t.out = z_out;
  t.stats_out = stats_out;
  t.B = B;
  t.L = L;
  t.C = C;
  t.C2 = C2;
  t.G = groups;
  t.nch_in = nch_in;
  t.chunk_in = chunk_in;
  t.eps_gn = eps_gn;
  t.eps_ln = eps_ln;
  // every refusal comes before the first launch: a refused call writes nothing
  if (groups < 1 || !thin_tail_supported(dtype, t)) fail(SF_ERR_UNSUPPORTED, "shape outside the thin-level tail's coverage (C / C2 = 8/8, 32/32, 64/32, 64/64; 4 or 8 channels per group)");
  const int64_t need = sf_op_thin_tail_workspace_bytes(dtype, C, C2);
  if (need < 0 || ws_bytes < need) fail(SF_ERR_WORKSPACE, "workspace too small: need %lld bytes", (long long)need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  Workspace wk(ws, ws_bytes);
  const int64_t es = (int64_t)dsize(dtype);
  void *wp2 = wk.alloc((int64_t)C * 3 * C * es), *wp3 = wk.alloc((int64_t)C * (C + C2) * es);
  t.w2 = wp2;
  t.w3 = wp3;
  SF_HIP(launch_pack_conv(dtype, w2, C, C, 0, C, 3, C, nullptr, wp2, 3 * C, 0, s));
  SF_HIP(launch_pack_conv(dtype, w_inj, C, C + c2_real, 0, C, 1, C, nullptr, wp3, C + C2, 0, s));
  if (C2) SF_HIP(launch_pack_conv(dtype, w_inj, C, C + c2_real, C, c2_real, 1, C2, nullptr, wp3, C + C2, C, s));
  SF_HIP(launch_thin_tail(dtype, t, s));
  if (rw_out) *rw_out = rw;
  return SF_OK;
  SF_API_END
}

int64_t sf_op_inject_prenorm_proj_workspace_bytes(int B, int L, int C, int C2, int N) {
  if (B < 1 || L < 1 || C < 32 || C2 < 0 || N < 8) return -1;
  const int64_t M = (int64_t)B * L, K1 = C + (C2 + 31) / 32 * 32;
  return (int64_t)C * K1 * 2 + (int64_t)N * C * 2 + M * C * 2 + M * (C / 32) * 8 + (int64_t)(2 * N + C) * 4 + 4096;
}

int sf_op_inject_prenorm_proj(int dtype, const void *m, const void *ctx, const float *w_inj, const float *b_inj, const float *gamma,
                              const float *beta, float eps, const float *w_q, int B, int L, int C, int C2, int N, void *z_out, void *q_out,
                              int *fused_out, void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!m || !w_inj || !b_inj || !gamma || !beta || !w_q || !z_out || !q_out || !ws) fail(SF_ERR_INVALID, "null argument");
  if (dtype != BF16 && dtype != F16) fail(SF_ERR_UNSUPPORTED, "16-bit dtypes only");
  if (C % 32 || C2 % 32 || N % 32 || (C2 > 0 && !ctx)) fail(SF_ERR_UNSUPPORTED, "C, C2 and N must be multiples of 32");
  const int64_t need = sf_op_inject_prenorm_proj_workspace_bytes(B, L, C, C2, N);
  if (need < 0 || ws_bytes < need) fail(SF_ERR_WORKSPACE, "workspace too small: need %lld bytes", (long long)need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  Workspace wk(ws, ws_bytes);
  const int64_t M = (int64_t)B * L;
  const int K1 = C + C2;
  void *w1 = wk.alloc((int64_t)C * K1 * 2), *w2 = wk.alloc((int64_t)N * C * 2), *tmp = wk.alloc(M * C * 2);
  float *rowpart = static_cast<float *>(wk.alloc(M * (C / 32) * 8));
  float *bias2 = static_cast<float *>(wk.alloc((int64_t)N * 4)), *colsum = static_cast<float *>(wk.alloc((int64_t)N * 4));
  SF_HIP(launch_pack_rows(dtype, w_inj, C, K1, K1, nullptr, w1, K1, s));
  SF_HIP(launch_pack_rows(dtype, w_q, N, C, C, gamma, w2, C, s));          // W (g * xhat + b) = (W diag g) xhat + W b
  SF_HIP(launch_fold_bias(w_q, N, C, beta, nullptr, bias2, s));
  SF_HIP(launch_row_sums(dtype, w2, N, C, colsum, s));
  ConvGemmArgs a;   // InjectChannels
  a.src = m;
  a.src_ld = C;
  a.src2 = ctx;
  a.src2_ld = C2;
  a.w = w1;
  a.bias = b_inj;
  a.M = (int)M;
  a.N = a.n_store = C;
  a.K = K1;
  a.cin = C;
  a.cin2 = C2;
  a.taps = 1;
  a.Lout = a.Lsrc = L;
  a.out = z_out;
  a.out_ld = C;
  a.res = m;
  a.res_ld = C;
  ConvGemmArgs q;   // pre-normed projection
  q.src = z_out;
  q.src_ld = C;
  q.w = w2;
  q.bias = bias2;
  q.M = (int)M;
  q.N = q.n_store = N;
  q.K = q.cin = C;
  q.taps = 1;
  q.Lout = q.Lsrc = L;
  q.out = q_out;
  q.out_ld = N;
  ConvGemmArgs ar = a, ql = q;
  ar.rowpart_out = rowpart;
  ar.rowpart_nt = C / 32;
  ql.ln_part = rowpart;
  ql.ln_nt = C / 32;
  ql.ln_eps = eps;
  ql.ln_colsum = colsum;
  ar.mt_ln = ql.mt_ln = 1;   // the op always offers the macro-tile form (the engine never does: kernels.h, ConvGemmArgs::mt_ln)
  const bool fused = conv_gemm_emits_rowpart(dtype, ar) && conv_gemm_ln_ok(dtype, ql);
  if (fused_out) *fused_out = fused ? 1 : 0;
  if (fused) {
    SF_HIP(launch_conv_gemm(dtype, ar, s));
    SF_HIP(launch_conv_gemm_ln(dtype, ql, s));
  } else {
    if (!conv_gemm_supported(dtype, a) || !conv_gemm_supported(dtype, q)) fail(SF_ERR_UNSUPPORTED, "shape outside the GEMM kernels' coverage");
    SF_HIP(launch_conv_gemm(dtype, a, s));
    SF_HIP(launch_ln_modulate(dtype, z_out, C, nullptr, 0, eps, B, L, C, tmp, C, s));
    q.src = tmp;
    SF_HIP(launch_conv_gemm(dtype, q, s));
  }
  return SF_OK;
  SF_API_END
}

// ---- sf_op_conv1d_epi / sf_op_conv1d_ln: one launch with the whole epilogue exposed (tests/gemm_epilogue_ref.py) --------------------------
// The ConvGemmArgs of the launch, its weight images and its plan, finished by the same statements for the real call and for the query
// (query: every image is a probe pointer, nothing is launched and no device is touched).  ln: launch_conv_gemm_ln's arguments.
namespace {
struct EpiLaunch {
  int dt = F32;
  ConvGemmArgs a;
  ConvGemmPlan pl;
  bool rowpart = false, gnpart = false;
};
int64_t epi_workspace_bytes(const sf_conv1d_epi_desc &d) {
  const int64_t K = (int64_t)d.taps * d.C + d.C2;
  return 16 * (int64_t)d.N * K + 4 * (int64_t)d.N + 8 * 256;   // w, wfr (compute type), wx, wfrx (4 bytes per element), the column sums
}
EpiLaunch epi_build(const sf_conv1d_epi_desc &d, bool ln, bool query, void *ws, int64_t ws_bytes, hipStream_t s) {
  if (d.dtype != SF_F32 && d.dtype != SF_BF16 && d.dtype != SF_F16 && d.dtype != SF_F32X) fail(SF_ERR_INVALID, "unknown dtype %d", d.dtype);
  if (d.B < 1 || d.L < 1 || d.C < 1 || d.C2 < 0 || d.N < 1 || d.taps < 1 || d.stride < 1 || d.pad < 0 || d.upsample < 1 ||
      (int64_t)d.L * d.upsample + 2 * d.pad < d.taps)
    fail(SF_ERR_INVALID, "bad geometry");
  if (d.upsample & (d.upsample - 1)) fail(SF_ERR_UNSUPPORTED, "upsample must be a power of two");
  if ((d.C % 32) || (d.C2 % 32)) fail(SF_ERR_UNSUPPORTED, "C and C2 must be multiples of 32 (the thin path has no such epilogue)");
  if (d.C2 > 0 && d.taps != 1) fail(SF_ERR_UNSUPPORTED, "a second source needs taps == 1");
  if (d.act < 0 || d.act > 3) fail(SF_ERR_UNSUPPORTED, "act must be 0 .. 3");
  if (d.src_x3 && (ln || d.dtype != SF_F32X || d.C2 != 0)) fail(SF_ERR_UNSUPPORTED, "src_x3: pre-split rows are one fp32x source of the plain launch");
  const int Lout = (d.L * d.upsample + 2 * d.pad - d.taps) / d.stride + 1;
  const int64_t M64 = (int64_t)d.B * Lout, K64 = (int64_t)d.taps * d.C + d.C2;
  if (M64 > 0x7FFFFFFF || K64 > 0x7FFFFFFF) fail(SF_ERR_UNSUPPORTED, "more than 2^31 rows");
  if (!query) {
    if (!d.x || !d.w || !d.out || !ws || (d.C2 > 0 && !d.x2)) fail(SF_ERR_INVALID, "null argument");
    if (ws_bytes < epi_workspace_bytes(d)) fail(SF_ERR_WORKSPACE, "workspace too small: need %lld bytes", (long long)epi_workspace_bytes(d));
  }
  if (reinterpret_cast<uintptr_t>(d.w) % 16) fail(SF_ERR_INVALID, "w must be 16-byte aligned");
  EpiLaunch r;
  const bool x3 = d.dtype == SF_F32X;
  const int dt = r.dt = x3 ? F32 : d.dtype;
  const int N = d.N, K = (int)K64;
  Workspace wk(ws, ws_bytes);
  ConvGemmArgs &a = r.a;
  a.src = d.x;
  a.src_ld = d.C;
  a.src2 = d.C2 ? d.x2 : nullptr;
  a.src2_ld = d.C2;
  a.bias = d.bias;
  a.N = a.n_store = N;
  a.K = K;
  a.cin = d.C;
  a.cin2 = d.C2;
  a.taps = d.taps;
  a.stride = d.stride;
  a.pad = d.pad;
  while ((1 << a.up_shift) < d.upsample) ++a.up_shift;
  a.Lsrc = d.L;
  a.Lout = Lout;
  a.M = (int)M64;
  a.out = d.out;
  a.out_ld = N;
  a.res = d.residual;
  a.res_ld = N;
  a.bscale = d.bscale;
  a.bscale_ld = N;
  a.badd = d.badd;
  a.badd_ld = N;
  a.act = d.act;
  a.out_f32 = d.out_f32 ? 1 : 0;
  a.solo = d.solo ? 1 : 0;
  a.mt_ln = d.mt_ln ? 1 : 0;
  a.src_x3 = d.src_x3 ? 1 : 0;
  // ---- weight images, as the engine packs them; the LayerNorm consumer's column sums ------------------------------------------------------
  // Two passes of the same statements: probe pointers first (only whether an image exists enters a plan), so that the entry can refuse
  // before anything is launched; the real images are allocated and packed behind the plan (real = true).
  if (ln) {
    if (!d.ln_part) fail(SF_ERR_INVALID, "ln_part is required");
    if (d.ln_operand == 0 && (d.ln_ss || d.res_ln)) fail(SF_ERR_INVALID, "the accumulator-side form takes no ln_ss / res_ln");
  } else if (d.ln_part || d.ln_ss || d.res_ln) {
    fail(SF_ERR_INVALID, "LayerNorm arguments on the plain launch (sf_op_conv1d_ln takes them)");
  }
  auto set_images = [&](bool real) {
    auto image = [&](int64_t bytes) -> void * { return real ? wk.alloc(bytes) : reinterpret_cast<void *>(256); };
    const void *wp = d.w;   // fp32: the caller's matrix is the GEMM's
    if (dt != F32) {
      void *packed = image((int64_t)N * K * 2);
      if (real) SF_HIP(launch_pack_rows(dt, d.w, N, K, K, nullptr, packed, K, s));
      wp = packed;
      if ((K % 64) == 0 && K <= 2048 && (N % 32) == 0) {   // fragment order for the register-staged kernel (conv_gemm_rs.hip)
        void *wfr = image((int64_t)N * K * 2);
        if (real) SF_HIP(launch_pack_wfr(dt, wp, N, K, wfr, s));
        a.wfr = wfr;
      }
    } else if (x3 && (K % 32) == 0) {
      void *wx = image((int64_t)N * K * 4);
      if (real) SF_HIP(launch_pack_wx(static_cast<const float *>(wp), N, K, wx, s));
      a.wx = wx;
      if ((K % 64) == 0 && K <= 1280 && (N % 32) == 0) {
        void *wfrx = image((int64_t)N * K * 4);
        if (real) SF_HIP(launch_pack_wfrx(static_cast<const float *>(wp), N, K, wfrx, s));
        a.wfrx = wfrx;
      }
    }
    a.w = wp;
    if (ln && d.ln_operand == 0) {
      float *colsum = static_cast<float *>(image((int64_t)N * 4));
      if (real) SF_HIP(launch_row_sums(dt, wp, N, K, colsum, s));
      a.ln_colsum = colsum;
    }
  };
  set_images(false);
  if (ln) {
    a.ln_part = d.ln_part;
    a.ln_nt = d.C / 32;
    a.ln_eps = d.ln_eps;
    if (d.ln_operand != 0) {
      a.ln_ss = d.ln_ss;
      a.ln_ss_ld = 2 * d.C;
      a.res_ln = d.res_ln ? 1 : 0;
    }
  }
  // ---- statistics outputs: armed, and kept only where the plan honours them -------------------------------------------------------------------
  const bool stats_ok = (N % 32) == 0;
  if (d.rowpart && stats_ok) {
    a.rowpart_out = d.rowpart;
    a.rowpart_nt = N / 32;
  }
  if (d.gnpart && stats_ok && !ln) a.gnpart_out = d.gnpart;
  auto plan = [&] { return ln ? conv_gemm_ln_plan(dt, a) : conv_gemm_plan(dt, a); };
  r.pl = plan();
  if (a.rowpart_out && !r.pl.rowpart) {
    a.rowpart_out = nullptr;
    a.rowpart_nt = 0;
  }
  if (a.gnpart_out && !r.pl.gnpart) a.gnpart_out = nullptr;
  r.pl = plan();
  if (r.pl.family == CG_INVALID || !conv_gemm_supported(dt, a)) fail(SF_ERR_UNSUPPORTED, "no GEMM kernel takes these arguments");
  if (a.src_x3 && !r.pl.src_x3) fail(SF_ERR_UNSUPPORTED, "src_x3: the plan (%s) does not read pre-split rows", r.pl.label);
  if ((a.rowpart_out && !r.pl.rowpart) || (a.gnpart_out && !r.pl.gnpart)) fail(SF_ERR_UNSUPPORTED, "the plan moved when a declined output was disarmed");
  r.rowpart = a.rowpart_out != nullptr;
  r.gnpart = a.gnpart_out != nullptr;
  if (!query) {   // the launch is decided and will not be refused: now the images (the plan read only which of them exist)
    const ConvGemmPlan probe = r.pl;
    set_images(true);
    r.pl = plan();
    if (r.pl.family != probe.family || r.pl.tile != probe.tile || r.pl.split != probe.split) fail(SF_ERR_INVALID, "the plan depends on an image's address");
  }
  return r;
}
int epi_variant(const sf_conv1d_epi_desc *d, bool ln, char *label, int label_bytes, int *rowpart_done, int *gnpart_done) {
  SF_API_BEGIN
  if (!d || !label || label_bytes < 1) fail(SF_ERR_INVALID, "null argument");
  label[0] = 0;
  const EpiLaunch r = epi_build(*d, ln, true, nullptr, 0, nullptr);
  snprintf(label, (size_t)label_bytes, "%s", r.pl.label);
  if (rowpart_done) *rowpart_done = r.rowpart ? 1 : 0;
  if (gnpart_done) *gnpart_done = r.gnpart ? 1 : 0;
  return SF_OK;
  SF_API_END
}
}  // namespace

int64_t sf_op_conv1d_epi_workspace_bytes(const sf_conv1d_epi_desc *d) {
  if (!d || d->C < 1 || d->C2 < 0 || d->N < 1 || d->taps < 1) return -1;
  return epi_workspace_bytes(*d);
}

int sf_op_conv1d_epi(const sf_conv1d_epi_desc *d, int *rowpart_done, int *gnpart_done, void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!d) fail(SF_ERR_INVALID, "null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const EpiLaunch r = epi_build(*d, false, false, ws, ws_bytes, s);
  if (rowpart_done) *rowpart_done = r.rowpart ? 1 : 0;
  if (gnpart_done) *gnpart_done = r.gnpart ? 1 : 0;
  SF_HIP(launch_conv_gemm_planned(r.dt, r.a, r.pl, s));
  return SF_OK;
  SF_API_END
}

int sf_op_conv1d_epi_variant(const sf_conv1d_epi_desc *d, char *label, int label_bytes, int *rowpart_done, int *gnpart_done) {
  return epi_variant(d, false, label, label_bytes, rowpart_done, gnpart_done);
}

int sf_op_conv1d_ln(const sf_conv1d_epi_desc *d, int *rowpart_done, void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!d) fail(SF_ERR_INVALID, "null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const EpiLaunch r = epi_build(*d, true, false, ws, ws_bytes, s);
  if (rowpart_done) *rowpart_done = r.rowpart ? 1 : 0;
  SF_HIP(launch_conv_gemm_planned(r.dt, r.a, r.pl, s));
  return SF_OK;
  SF_API_END
}

int sf_op_conv1d_ln_variant(const sf_conv1d_epi_desc *d, char *label, int label_bytes, int *rowpart_done) {
  return epi_variant(d, true, label, label_bytes, rowpart_done, nullptr);
}

// ---- sf_op_conv_cb_tiles: the channel-block convolution behind the TILE statistics of a producing GEMM (conv_cb prologue 2) ----------------
int64_t sf_op_conv_cb_tiles_workspace_bytes(int dtype, int B, int L, int C) {
  if (B < 1 || L < 1 || C < 1 || (dtype != SF_BF16 && dtype != SF_F16 && dtype != SF_F32X)) return -1;
  Workspace dry(nullptr, 0);
  dry.alloc((int64_t)C * C * 3 * (int64_t)dsize(dtype));       // fragment-ordered weights
  dry.alloc((int64_t)(C / 128) * B * L * C * 4);               // the partial slabs
  return dry.used();
}

int sf_op_conv_cb_tiles(int dtype, const void *x, const float *w, const float *bias, const float *gn_g, const float *gn_b, int groups, float eps,
                        const float *tile_stats, int B, int L, int C, void *h_out, float *stats_out, int *nch_out, int *chunk_rows_out, void *ws,
                        int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!x || !w || !bias || !gn_g || !gn_b || !tile_stats || !h_out || !stats_out || !ws) fail(SF_ERR_INVALID, "null argument");
  if (dtype != SF_BF16 && dtype != SF_F16 && dtype != SF_F32X) fail(SF_ERR_UNSUPPORTED, "bf16, fp16 or fp32x");
  if (B < 1 || L < 1 || C < 1 || groups < 1 || groups > 64 || !conv_cb_shape_ok(dtype, B, L, C, C, groups) || !conv_cb_tile_stats_ok(L, C, groups))
    fail(SF_ERR_UNSUPPORTED, "shape outside the tile-statistics prologue of the channel-block convolution");
  const int64_t need = sf_op_conv_cb_tiles_workspace_bytes(dtype, B, L, C);
  if (ws_bytes < need) fail(SF_ERR_WORKSPACE, "workspace too small: need %lld bytes", (long long)need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  Workspace wk(ws, ws_bytes);
  const int64_t M = (int64_t)B * L;
  const int S = C / 128;
  const int adt = dtype == SF_F32X ? (int)F32 : dtype;   // activations and the reducer of the fp32x chain are plain fp32
  void *wp = wk.alloc((int64_t)C * C * 3 * (int64_t)dsize(dtype));
  float *slab = static_cast<float *>(wk.alloc((int64_t)S * M * C * 4));
  const CbGnPlan gp = cb_gn_plan(L);
  if (gp.nch > 32) fail(SF_ERR_UNSUPPORTED, "more than 32 statistics chunks per clip");
  if (nch_out) *nch_out = gp.nch;
  if (chunk_rows_out) *chunk_rows_out = gp.chunk_rows;
  SF_HIP(launch_pack_conv_cb(dtype, w, C, C, wp, s));
  ConvCbArgs a;
  a.src = x;
  a.src_ld = C;
  a.wp = wp;
  a.slab = slab;
  a.B = B;
  a.L = L;
  a.C = a.N = C;
  a.pro = 2;
  a.G = groups;
  a.stats = tile_stats;
  a.gamma = gn_g;
  a.beta = gn_b;
  a.eps = eps;
  SF_HIP(launch_conv_cb(dtype, a, s));
  SF_HIP(launch_cb_reduce_gn(adt, slab, S, B, L, C, bias, h_out, C, groups, stats_out, gp, s));
  return SF_OK;
  SF_API_END
}

// Timing aid: the four launches of the channel-block chain, each averaged over `iters` back-to-back launches on random data
// (ms[0] conv_cb without prologue, ms[1] cb_reduce_gn, ms[2] conv_cb with the GroupNorm+SiLU prologue, ms[3] cb_reduce_ln).
// cold != 0: rotate through enough weight copies that every launch streams its weights from HBM.
int sf_bench_conv_cb(int dtype, int B, int L, int C, int groups, int kb, int cold, int iters, float *ms) {
  SF_API_BEGIN
  if (!ms || iters < 1 || (kb != 1 && kb != 2)) fail(SF_ERR_INVALID, "bad argument");
  if (!conv_cb_shape_ok(dtype, B, L, C, C, groups)) fail(SF_ERR_UNSUPPORTED, "shape outside the channel-block convolution's coverage");
  const int64_t M = (int64_t)B * L;
  const int S = C / 128 / kb;
  const size_t wbytes = (size_t)C * C * 3 * 2;
  int ncopy = 1;
  if (cold) ncopy = (int)std::min<size_t>(256, (768u << 20) / wbytes + 1);
  void *w = nullptr, *x = nullptr, *h = nullptr;
  float *slab = nullptr, *stats = nullptr, *vec = nullptr;
  SF_HIP(hipMalloc(&w, wbytes * ncopy));
  SF_HIP(hipMalloc(&x, M * C * 2));
  SF_HIP(hipMalloc(&h, M * C * 2));
  SF_HIP(hipMalloc(reinterpret_cast<void **>(&slab), (size_t)S * M * C * 4));
  SF_HIP(hipMalloc(reinterpret_cast<void **>(&stats), (size_t)B * 32 * 64 * 2 * 4));
  SF_HIP(hipMalloc(reinterpret_cast<void **>(&vec), (size_t)(4 * C + (size_t)B * 2 * C) * 4));
  SF_HIP(hipMemset(w, 0x11, wbytes * ncopy));     // small finite 16-bit patterns (bf16 / fp16 alike)
  SF_HIP(hipMemset(x, 0x3c, M * C * 2));
  SF_HIP(hipMemset(vec, 0, (size_t)(4 * C + (size_t)B * 2 * C) * 4));
  const CbGnPlan gp = cb_gn_plan(L);
  ConvCbArgs a;
  a.src = x;
  a.src_ld = C;
  a.slab = slab;
  a.B = B;
  a.L = L;
  a.C = a.N = C;
  a.kb = kb;
  a.G = groups;
  a.nch = gp.nch;
  a.chunk_rows = gp.chunk_rows;
  a.stats = stats;
  a.gamma = vec;
  a.beta = vec + C;
  hipEvent_t e0, e1;
  SF_HIP(hipEventCreate(&e0));
  SF_HIP(hipEventCreate(&e1));
  hipError_t err = hipSuccess;
  for (int which = 0; which < 4 && err == hipSuccess; ++which) {
    auto one = [&](int i) -> hipError_t {
      a.wp = static_cast<char *>(w) + (size_t)(i % ncopy) * wbytes;
      switch (which) {
        case 0: a.pro = 0; return launch_conv_cb(dtype, a, nullptr);
        case 1: return launch_cb_reduce_gn(dtype, slab, S, B, L, C, vec + 2 * C, h, C, groups, stats, gp, nullptr);
        case 2: a.pro = 1; return launch_conv_cb(dtype, a, nullptr);
        default: return launch_cb_reduce_ln(dtype, slab, S, B, L, C, vec + 2 * C, x, C, vec + 4 * C, 2 * C, 1e-6f, h, C, nullptr);
      }
    };
    for (int i = 0; i < 3 && err == hipSuccess; ++i) err = one(i);
    if (err != hipSuccess) break;
    SF_HIP(hipDeviceSynchronize());
    SF_HIP(hipEventRecord(e0, nullptr));
    for (int i = 0; i < iters && err == hipSuccess; ++i) err = one(i);
    SF_HIP(hipEventRecord(e1, nullptr));
    SF_HIP(hipEventSynchronize(e1));
    SF_HIP(hipEventElapsedTime(&ms[which], e0, e1));
    ms[which] /= (float)iters;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  for (void *p : {w, x, h, (void *)slab, (void *)stats, (void *)vec}) (void)hipFree(p);
  if (err != hipSuccess) fail(SF_ERR_HIP, "launch failed: %s", hipGetErrorString(err));
  return SF_OK;
  SF_API_END
}

int sf_op_ln_modulate(int dtype, const void *x, const float *scale_shift, float eps, int B, int L, int C, void *out, void *stream) {
  SF_API_BEGIN
  if (!x || !out) fail(SF_ERR_INVALID, "null argument");
  if (scale_shift && (C % 2)) fail(SF_ERR_UNSUPPORTED, "C must be even");
  SF_HIP(launch_ln_modulate(dtype, x, C, scale_shift, 2 * C, eps, B, L, C, out, C, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_attention(int dtype, const void *q, const void *kv, int B, int L, int heads, int head_dim, void *out, void *stream) {
  SF_API_BEGIN
  if (!q || !kv || !out) fail(SF_ERR_INVALID, "null argument");
  const bool x3 = dtype == SF_F32X;   // fp32 tensors, products from split fp16 operands
  SF_HIP(launch_attention(x3 ? (int)F32 : dtype, q, heads * head_dim, kv, 2 * heads * head_dim, B, L, heads, head_dim, out, heads * head_dim,
                          static_cast<hipStream_t>(stream), x3));
  return SF_OK;
  SF_API_END
}

// ---- the same three launchers as the engine calls them in front of a GEMM: output stride and row format exposed (tests/x3rows_ref.py) ------
namespace {
// hipErrorInvalidValue is a launcher's own refusal, returned before it launches anything
void launched(hipError_t e, const char *launcher) {
  if (e == hipErrorInvalidValue) fail(SF_ERR_UNSUPPORTED, "%s does not take these arguments", launcher);
  if (e != hipSuccess) fail(SF_ERR_HIP, "%s -> %s", launcher, hipGetErrorString(e));
}
}  // namespace

int sf_op_gn_silu_rows(int dtype, const void *x, const float *gamma, const float *beta, int groups, float eps, int B, int L, int C, void *out,
                       int out_ld, int xfmt, void *stream) {
  SF_API_BEGIN
  if (!x || !gamma || !beta || !out) fail(SF_ERR_INVALID, "null argument");
  if (dtype != SF_F32 && dtype != SF_BF16 && dtype != SF_F16) fail(SF_ERR_INVALID, "dtype must be SF_F32, SF_BF16 or SF_F16");
  if (B < 1 || L < 1 || C < 1 || out_ld < C) fail(SF_ERR_INVALID, "bad geometry");
  if (groups < 1 || C % groups) fail(SF_ERR_INVALID, "channels must be divisible by groups");
  launched(launch_gn_silu(dtype, x, C, B, L, C, groups, gamma, beta, eps, out, out_ld, static_cast<hipStream_t>(stream), Prefetch(), xfmt != 0),
           "launch_gn_silu");
  return SF_OK;
  SF_API_END
}

int sf_op_ln_modulate_rows(int dtype, const void *x, const float *scale_shift, float eps, int B, int L, int C, void *out, int out_ld, int xfmt,
                           void *stream) {
  SF_API_BEGIN
  if (!x || !out) fail(SF_ERR_INVALID, "null argument");
  if (dtype != SF_F32 && dtype != SF_BF16 && dtype != SF_F16) fail(SF_ERR_INVALID, "dtype must be SF_F32, SF_BF16 or SF_F16");
  if (B < 1 || L < 1 || C < 1 || out_ld < C) fail(SF_ERR_INVALID, "bad geometry");
  launched(launch_ln_modulate(dtype, x, C, scale_shift, 2 * C, eps, B, L, C, out, out_ld, static_cast<hipStream_t>(stream), Prefetch(), xfmt != 0),
           "launch_ln_modulate");
  return SF_OK;
  SF_API_END
}

int sf_op_attention_rows(int dtype, const void *q, int ldq, const void *kv, int ldkv, int B, int L, int heads, int head_dim, void *out, int ldo,
                         int xfmt, void *stream) {
  SF_API_BEGIN
  if (!q || !kv || !out) fail(SF_ERR_INVALID, "null argument");
  if (dtype != SF_F32 && dtype != SF_BF16 && dtype != SF_F16 && dtype != SF_F32X) fail(SF_ERR_INVALID, "unknown dtype %d", dtype);
  if (B < 1 || L < 1 || heads < 1 || head_dim < 1) fail(SF_ERR_INVALID, "bad geometry");
  const int64_t hd = (int64_t)heads * head_dim;
  if (ldq < hd || ldkv < 2 * hd || ldo < hd) fail(SF_ERR_INVALID, "a row stride is shorter than the row");
  const bool x3 = dtype == SF_F32X;
  launched(launch_attention(x3 ? (int)F32 : dtype, q, ldq, kv, ldkv, B, L, heads, head_dim, out, ldo, static_cast<hipStream_t>(stream), x3, xfmt != 0),
           "launch_attention");
  return SF_OK;
  SF_API_END
}

}  // extern "C"
