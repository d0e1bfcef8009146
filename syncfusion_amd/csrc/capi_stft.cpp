// C ABI of the STFT pair and the spectral-gating denoiser (stft.hip): the handle with the window, twiddle and smoothing-tap tables, the
// workspace query, sf_stft_forward, sf_istft_forward, sf_spectral_gate_noise_threshold and sf_spectral_gate.  Arguments are checked
// before the first HIP call, so every refusal is reported without a device.
#include <cmath>
#include <cstring>
#include <vector>

#include "engine_common.h"
#include "stft.h"

using namespace sf;

struct sf_spectral_gate_handle {
  StftTables tab;                     // device pointers into `dev` once uploaded
  std::vector<float> h_window, h_tw_re, h_tw_im, h_ftaps, h_ttaps;
  double nola_min = 0.0;              // min over n < hop of sum_k w[n + k hop]^2, fp64
  void *dev = nullptr;
  ~sf_spectral_gate_handle() {
    if (dev) (void)hipFree(dev);
  }
};

static size_t up256(size_t n) { return (n + 255) / 256 * 256; }

// The tables go to the device in one allocation at the first device call (create itself needs no device).
static void upload(sf_spectral_gate_handle *h) {
  if (h->dev) return;
  const std::vector<float> *src[5] = {&h->h_window, &h->h_tw_re, &h->h_tw_im, &h->h_ftaps, &h->h_ttaps};
  size_t off[6] = {0};
  for (int i = 0; i < 5; ++i) off[i + 1] = off[i] + up256(src[i]->size() * 4);
  std::vector<char> img(off[5], 0);
  for (int i = 0; i < 5; ++i) std::memcpy(&img[off[i]], src[i]->data(), src[i]->size() * 4);
  void *d = nullptr;
  hipError_t e = hipMalloc(&d, off[5]);
  if (e == hipSuccess) e = hipMemcpy(d, img.data(), off[5], hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (d) (void)hipFree(d);
    fail(SF_ERR_HIP, "stft tables upload: %s", hipGetErrorString(e));
  }
  const char *c = static_cast<const char *>(d);
  h->dev = d;
  h->tab.window = reinterpret_cast<const float *>(c + off[0]);
  h->tab.tw_re = reinterpret_cast<const float *>(c + off[1]);
  h->tab.tw_im = reinterpret_cast<const float *>(c + off[2]);
  h->tab.ftaps = reinterpret_cast<const float *>(c + off[3]);
  h->tab.ttaps = reinterpret_cast<const float *>(c + off[4]);
}

// checks shared by the calls that start from a waveform; returns T
static int check_wave(const sf_spectral_gate_handle *h, const float *wav, int B, int L) {
  if (!h || !wav) fail(SF_ERR_INVALID, "null argument");
  if (B < 1 || L < 1) fail(SF_ERR_INVALID, "B and L must be at least 1");
  if (B > 65535) fail(SF_ERR_SHAPE, "at most 65535 rows per call");
  if (L < h->tab.win) fail(SF_ERR_SHAPE, "a row of %d samples is shorter than the window of %d", L, h->tab.win);
  if (h->tab.pad_mode == STFT_PAD_REFLECT && L <= h->tab.pad) fail(SF_ERR_SHAPE, "reflect padding needs L > win / 2 (L = %d, win = %d)", L, h->tab.win);
  const int64_t T = stft_frames(L, h->tab.win, h->tab.hop, h->tab.pad), F = h->tab.n_fft / 2 + 1;
  if ((int64_t)B * T * F >= (1ll << 31) || (int64_t)B * T * h->tab.win >= (1ll << 40)) fail(SF_ERR_SHAPE, "batch too large");
  return (int)T;
}

static void check_nola(const sf_spectral_gate_handle *h) {
  if (!(h->nola_min > 1e-10))
    fail(SF_ERR_INVALID, "window %d with hop %d violates NOLA (the smallest overlap-added squared window is %.3g): the STFT is not invertible",
         h->tab.win, h->tab.hop, h->nola_min);
}

extern "C" {

int sf_spectral_gate_create(int n_fft, int win_length, int hop, int center, int pad_mode, int scale_spectrum, const float *freq_taps, int n_freq_taps,
                            const float *time_taps, int n_time_taps, sf_spectral_gate_handle **out) {
  SF_API_BEGIN
  if (!out || !freq_taps || !time_taps) fail(SF_ERR_INVALID, "null argument");
  *out = nullptr;
  if (n_fft < 256 || n_fft > 4096 || (n_fft & (n_fft - 1))) fail(SF_ERR_INVALID, "n_fft must be a power of two in [256, 4096], got %d", n_fft);
  if (win_length < 2 || win_length > n_fft) fail(SF_ERR_INVALID, "the window must have 2 .. n_fft = %d points, got %d", n_fft, win_length);
  if (hop < 1) fail(SF_ERR_INVALID, "hop must be at least 1");
  if (pad_mode != STFT_PAD_CONSTANT && pad_mode != STFT_PAD_REFLECT) fail(SF_ERR_INVALID, "pad_mode must be 0 (constant) or 1 (reflect)");
  if (n_freq_taps < 1 || n_time_taps < 1 || !(n_freq_taps & 1) || !(n_time_taps & 1) || n_freq_taps > (1 << 20) || n_time_taps > (1 << 20))
    fail(SF_ERR_INVALID, "the smoothing filters must have an odd number of taps, got %d and %d", n_freq_taps, n_time_taps);
  auto *h = new sf_spectral_gate_handle();
  h->tab.n_fft = n_fft, h->tab.win = win_length, h->tab.hop = hop, h->tab.pad = center ? win_length / 2 : 0, h->tab.pad_mode = pad_mode;
  h->tab.n_ftaps = n_freq_taps, h->tab.n_ttaps = n_time_taps;
  std::vector<double> w(win_length);
  double wsum = 0.0;
  for (int i = 0; i < win_length; ++i) wsum += w[i] = 0.5 - 0.5 * std::cos(2.0 * M_PI * i / win_length);   // periodic Hann
  h->h_window.assign(n_fft, 0.f);
  for (int i = 0; i < win_length; ++i) h->h_window[i] = (float)w[i];
  h->tab.fwd_scale = scale_spectrum ? (float)(1.0 / wsum) : 1.f;
  h->tab.inv_scale = scale_spectrum ? (float)wsum : 1.f;
  h->nola_min = 1e300;
  for (int n = 0; n < hop; ++n) {
    double acc = 0.0;
    for (int i = n; i < win_length; i += hop) acc += w[i] * w[i];
    if (acc < h->nola_min) h->nola_min = acc;
  }
  const int bins = n_fft / 2 + 1;
  h->h_tw_re.resize(bins), h->h_tw_im.resize(bins);
  for (int k = 0; k < bins; ++k) {
    h->h_tw_re[k] = (float)std::cos(2.0 * M_PI * k / n_fft);
    h->h_tw_im[k] = (float)-std::sin(2.0 * M_PI * k / n_fft);
  }
  h->h_ftaps.assign(freq_taps, freq_taps + n_freq_taps);
  h->h_ttaps.assign(time_taps, time_taps + n_time_taps);
  *out = h;
  return SF_OK;
  SF_API_END
}

void sf_spectral_gate_destroy(sf_spectral_gate_handle *h) { delete h; }

int sf_spectral_gate_frames(const sf_spectral_gate_handle *h, int L) {
  if (!h || L < h->tab.win) return -1;
  return (int)stft_frames(L, h->tab.win, h->tab.hop, h->tab.pad);
}

int64_t sf_spectral_gate_workspace_bytes(const sf_spectral_gate_handle *h, int B, int L) {
  if (!h || B < 1 || L < h->tab.win) return -1;
  return gate_ws_bytes(h->tab, B, L);
}

int sf_stft_forward(sf_spectral_gate_handle *h, const float *wav, int B, int L, float *spec, void *stream) {
  SF_API_BEGIN
  const int T = check_wave(h, wav, B, L);
  if (!spec) fail(SF_ERR_INVALID, "null argument");
  upload(h);
  SF_HIP(launch_stft(h->tab, wav, B, L, T, spec, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_istft_forward(sf_spectral_gate_handle *h, const float *spec, int B, int T, float *out, int out_len, void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!h || !spec || !out) fail(SF_ERR_INVALID, "null argument");
  if (B < 1 || T < 1 || out_len < 1) fail(SF_ERR_INVALID, "B, T and out_len must be at least 1");
  if (B > 65535) fail(SF_ERR_SHAPE, "at most 65535 rows per call");
  check_nola(h);
  const int64_t n = istft_samples(T, h->tab.win, h->tab.hop, h->tab.pad), F = h->tab.n_fft / 2 + 1;
  if (n < 1 || n >= (1ll << 31) || (int64_t)B * T * F >= (1ll << 31) || (int64_t)B * T * h->tab.win >= (1ll << 40) || (int64_t)B * out_len >= (1ll << 40))
    fail(SF_ERR_SHAPE, "batch too large");
  const int64_t need = up256((size_t)B * T * h->tab.win * 4);
  require_workspace(ws, ws_bytes, need);
  upload(h);
  SF_HIP(launch_istft(h->tab, spec, B, T, static_cast<float *>(ws), out, out_len, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_spectral_gate_noise_threshold(sf_spectral_gate_handle *h, const float *noise, int B, int L, float n_std, float *thresh, void *ws,
                                     int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  const int T = check_wave(h, noise, B, L);
  if (!thresh) fail(SF_ERR_INVALID, "null argument");
  if (!(n_std >= 0.f)) fail(SF_ERR_INVALID, "n_std must be non-negative");
  const int F = h->tab.n_fft / 2 + 1;
  require_workspace(ws, ws_bytes, (int64_t)up256((size_t)B * T * F * 8));
  upload(h);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float *spec = static_cast<float *>(ws);
  SF_HIP(launch_stft(h->tab, noise, B, L, T, spec, s));
  SF_HIP(launch_noise_thresh(spec, B, T, F, n_std, thresh, s));
  return SF_OK;
  SF_API_END
}

int sf_spectral_gate(sf_spectral_gate_handle *h, const float *wav, int B, int L, int stationary, float smooth_b, float thresh_mult, float slope,
                     float prop_decrease, int prop_before_smoothing, const float *thresh, float *spec, float *mask_raw, float *mask_smooth, float *out, void *ws,
                     int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  const int T = check_wave(h, wav, B, L);
  if (!spec || !mask_raw || !mask_smooth || !out) fail(SF_ERR_INVALID, "null argument");
  if (stationary && !thresh) fail(SF_ERR_INVALID, "null argument: the stationary mask needs the thresholds");
  if (!stationary && (!(smooth_b > 0.f) || !(smooth_b <= 1.f))) fail(SF_ERR_INVALID, "the smoothing coefficient must lie in (0, 1], got %g", (double)smooth_b);
  if (!(prop_decrease >= 0.f) || !(prop_decrease <= 1.f)) fail(SF_ERR_INVALID, "prop_decrease must lie in [0, 1]");
  check_nola(h);
  require_workspace(ws, ws_bytes, gate_ws_bytes(h->tab, B, L));
  upload(h);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int F = h->tab.n_fft / 2 + 1;
  const size_t cells = (size_t)B * T * F;
  char *w = static_cast<char *>(ws);
  float *plane = reinterpret_cast<float *>(w);
  float *spec_out = reinterpret_cast<float *>(w + up256(cells * 4));
  float *frames = reinterpret_cast<float *>(w + up256(cells * 4) + up256(cells * 8));
  float *rowmax = reinterpret_cast<float *>(w + up256(cells * 4) + up256(cells * 8) + up256((size_t)B * T * h->tab.win * 4));
  SF_HIP(launch_stft(h->tab, wav, B, L, T, spec, s));
  if (stationary)
    SF_HIP(launch_stat_mask(spec, B, T, F, thresh, rowmax, mask_raw, s));
  else
    SF_HIP(launch_ns_mask(spec, B, T, F, smooth_b, thresh_mult, slope, plane, mask_raw, s));
  SF_HIP(launch_smooth_apply(h->tab, mask_raw, B, T, F, prop_decrease, prop_before_smoothing ? 1 : 0, spec, plane, mask_smooth, spec_out, s));
  SF_HIP(launch_istft(h->tab, spec_out, B, T, frames, out, L, s));
  return SF_OK;
  SF_API_END
}

}  // extern "C"
