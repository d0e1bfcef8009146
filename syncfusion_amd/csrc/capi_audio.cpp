// C ABI of the audio front end (audio_features.hip): the handle with the window, twiddle and filterbank tables, the workspace query,
// sf_logmel_forward, sf_onset_detect and the uncentred pair sf_audio_features_create_framed / sf_logmel_examples_forward.  Arguments are
// checked before the first HIP call, so every refusal is reported without a device.
#include <cmath>
#include <cstring>
#include <exception>
#include <vector>

#include "audio_features.h"
#include "engine_common.h"

using namespace sf;

struct sf_audio_features {
  AudioTables tab;                    // device pointers into `dev` once uploaded
  int win = 0;                        // uncentred handles (sf_audio_features_create_framed): window length <= n_fft
  std::vector<float> h_window, h_tw_re, h_tw_im, h_weights;
  std::vector<int32_t> h_first, h_count, h_offset;
  void *dev = nullptr;
  ~sf_audio_features() {
    if (dev) (void)hipFree(dev);
  }
};

static size_t up256(size_t n) { return (n + 255) / 256 * 256; }

// The tables go to the device in one allocation at the first device call (create itself needs no device).
static void upload(sf_audio_features *h) {
  if (h->dev) return;
  const size_t nw = h->h_window.size() * 4, nt = h->h_tw_re.size() * 4, nm = h->h_first.size() * 4, nf = h->h_weights.size() * 4;
  const size_t o_win = 0, o_re = o_win + up256(nw), o_im = o_re + up256(nt), o_first = o_im + up256(nt), o_count = o_first + up256(nm),
               o_off = o_count + up256(nm), o_w = o_off + up256(nm), total = o_w + up256(nf);
  std::vector<char> img(total, 0);
  std::memcpy(&img[o_win], h->h_window.data(), nw);
  std::memcpy(&img[o_re], h->h_tw_re.data(), nt);
  std::memcpy(&img[o_im], h->h_tw_im.data(), nt);
  std::memcpy(&img[o_first], h->h_first.data(), nm);
  std::memcpy(&img[o_count], h->h_count.data(), nm);
  std::memcpy(&img[o_off], h->h_offset.data(), nm);
  std::memcpy(&img[o_w], h->h_weights.data(), nf);
  void *d = nullptr;
  hipError_t e = hipMalloc(&d, total);
  if (e == hipSuccess) e = hipMemcpy(d, img.data(), total, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (d) (void)hipFree(d);
    fail(SF_ERR_HIP, "audio tables upload: %s", hipGetErrorString(e));
  }
  char *c = static_cast<char *>(d);
  h->dev = d;
  h->tab.window = reinterpret_cast<const float *>(c + o_win);
  h->tab.tw_re = reinterpret_cast<const float *>(c + o_re);
  h->tab.tw_im = reinterpret_cast<const float *>(c + o_im);
  h->tab.fb_first = reinterpret_cast<const int32_t *>(c + o_first);
  h->tab.fb_count = reinterpret_cast<const int32_t *>(c + o_count);
  h->tab.fb_offset = reinterpret_cast<const int32_t *>(c + o_off);
  h->tab.fb_weights = reinterpret_cast<const float *>(c + o_w);
}

// checks shared by the two entry points; returns T
static int check_call(const sf_audio_features *h, const float *wav, int B, int L, const void *ws, int64_t ws_bytes) {
  if (!h || !wav) fail(SF_ERR_INVALID, "null argument");
  if (B < 1 || L < 1) fail(SF_ERR_INVALID, "B and L must be at least 1");
  if (B > 65535) fail(SF_ERR_SHAPE, "at most 65535 clips per call");
  if (h->tab.pad_mode == AUDIO_PAD_NONE) fail(SF_ERR_INVALID, "the handle frames without centring: sf_logmel_examples_forward is its only forward call");
  if (h->tab.pad_mode == AUDIO_PAD_REFLECT && L <= h->tab.n_fft / 2) fail(SF_ERR_SHAPE, "reflect padding needs L > n_fft / 2 (L = %d, n_fft = %d)", L, h->tab.n_fft);
  const int64_t T = audio_frames(L, h->tab.hop);
  if ((int64_t)B * h->tab.n_mels * T >= (1ll << 31) || (int64_t)B * L >= (1ll << 40)) fail(SF_ERR_SHAPE, "batch too large");
  require_workspace(ws, ws_bytes, audio_ws_bytes(h->tab.n_mels, h->tab.hop, B, L));
  return (int)T;
}

// checks and host tables shared by the two create calls; window: periodic Hann of `win` points, zeros up to n_fft
static sf_audio_features *create_handle(int n_fft, int win, int hop, int n_mels, int pad_mode, const int32_t *first_bin, const int32_t *bin_count,
                                        const float *weights, int64_t n_weights) {
  if (n_fft < 256 || n_fft > 4096 || (n_fft & (n_fft - 1))) fail(SF_ERR_INVALID, "n_fft must be a power of two in [256, 4096], got %d", n_fft);
  if (win < 1 || win > n_fft) fail(SF_ERR_INVALID, "the window must have 1 .. n_fft = %d points, got %d", n_fft, win);
  if (hop < 1) fail(SF_ERR_INVALID, "hop must be at least 1");
  if (n_mels < 1) fail(SF_ERR_INVALID, "n_mels must be at least 1");
  const int bins = n_fft / 2 + 1;
  int64_t total = 0;
  std::vector<int32_t> offset(n_mels);
  for (int m = 0; m < n_mels; ++m) {
    if (bin_count[m] < 1) fail(SF_ERR_INVALID, "filter %d has an empty bin range", m);
    if (first_bin[m] < 0 || (int64_t)first_bin[m] + bin_count[m] > bins) fail(SF_ERR_INVALID, "filter %d reaches outside bins 0 .. %d", m, bins - 1);
    offset[m] = (int32_t)total;
    total += bin_count[m];
  }
  if (total != n_weights) fail(SF_ERR_INVALID, "%lld packed weights given, the bin counts add up to %lld", (long long)n_weights, (long long)total);
  auto *h = new sf_audio_features();
  h->tab.n_fft = n_fft, h->tab.hop = hop, h->tab.n_mels = n_mels, h->tab.pad_mode = pad_mode;
  h->win = win;
  h->h_window.assign(n_fft, 0.f);
  for (int i = 0; i < win; ++i) h->h_window[i] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * i / win));   // periodic Hann
  h->h_tw_re.resize(bins), h->h_tw_im.resize(bins);
  for (int k = 0; k < bins; ++k) {
    h->h_tw_re[k] = (float)std::cos(2.0 * M_PI * k / n_fft);
    h->h_tw_im[k] = (float)-std::sin(2.0 * M_PI * k / n_fft);
  }
  h->h_first.assign(first_bin, first_bin + n_mels);
  h->h_count.assign(bin_count, bin_count + n_mels);
  h->h_offset = offset;
  h->h_weights.assign(weights, weights + n_weights);
  return h;
}

extern "C" {

int sf_audio_features_create(int n_fft, int hop, int n_mels, int pad_mode, const int32_t *first_bin, const int32_t *bin_count,
                             const float *weights, int64_t n_weights, sf_audio_features **out) {
  SF_API_BEGIN
  if (!out || !first_bin || !bin_count || !weights) fail(SF_ERR_INVALID, "null argument");
  *out = nullptr;
  if (pad_mode != AUDIO_PAD_CONSTANT && pad_mode != AUDIO_PAD_REFLECT) fail(SF_ERR_INVALID, "pad_mode must be 0 (constant) or 1 (reflect)");
  *out = create_handle(n_fft, n_fft, hop, n_mels, pad_mode, first_bin, bin_count, weights, n_weights);
  return SF_OK;
  SF_API_END
}

int sf_audio_features_create_framed(int n_fft, int win_length, int hop, int n_mels, const int32_t *first_bin, const int32_t *bin_count,
                                    const float *weights, int64_t n_weights, sf_audio_features **out) {
  SF_API_BEGIN
  if (!out || !first_bin || !bin_count || !weights) fail(SF_ERR_INVALID, "null argument");
  *out = nullptr;
  *out = create_handle(n_fft, win_length, hop, n_mels, AUDIO_PAD_NONE, first_bin, bin_count, weights, n_weights);
  return SF_OK;
  SF_API_END
}

void sf_audio_features_destroy(sf_audio_features *h) { delete h; }

int64_t sf_audio_features_workspace_bytes(const sf_audio_features *h, int B, int L) {
  if (!h || B < 1 || L < 1) return -1;
  return audio_ws_bytes(h->tab.n_mels, h->tab.hop, B, L);
}

int sf_logmel_forward(sf_audio_features *h, const float *wav, int B, int L, float amin, float top_db, float *mel_power, float *db, void *ws,
                      int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  const int T = check_call(h, wav, B, L, ws, ws_bytes);
  if (!mel_power && !db) fail(SF_ERR_INVALID, "null argument: neither mel_power nor db asked for");
  if (db && (!(amin > 0.f) || !(top_db >= 0.f))) fail(SF_ERR_INVALID, "amin must be positive and top_db non-negative");
  upload(h);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float *mel = mel_power ? mel_power : static_cast<float *>(ws);
  SF_HIP(launch_mel_power(h->tab, wav, B, L, mel, s));
  if (db) SF_HIP(launch_db_flux(mel, B, h->tab.n_mels, T, amin, (float)(10.0 * std::log10((double)amin)), top_db, 0, 0, db, nullptr, s));
  return SF_OK;
  SF_API_END
}

int sf_onset_detect(sf_audio_features *h, const float *wav, int B, int L, float amin, float top_db, int lag, int pre_max, int post_max,
                    int pre_avg, int post_avg, int wait, float delta, int conf_interval, int capacity, float *envelope, int32_t *count,
                    int32_t *positions, float *confidence, float *strength, void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  const int T = check_call(h, wav, B, L, ws, ws_bytes);
  if (!envelope || !count || !positions || !confidence || !strength) fail(SF_ERR_INVALID, "null argument");
  if (!(amin > 0.f) || !(top_db >= 0.f)) fail(SF_ERR_INVALID, "amin must be positive and top_db non-negative");
  if (lag < 1 || pre_max < 0 || post_max < 1 || pre_avg < 0 || post_avg < 1 || wait < 0 || conf_interval < 1 || capacity < 1)
    fail(SF_ERR_INVALID, "lag, post_max, post_avg, conf_interval, capacity >= 1 and pre_max, pre_avg, wait >= 0 expected");
  upload(h);
  hipStream_t s = static_cast<hipStream_t>(stream);
  char *w = static_cast<char *>(ws);
  float *mel = reinterpret_cast<float *>(w);
  const size_t plane = up256((size_t)B * h->tab.n_mels * T * 4), row = up256((size_t)B * T * 4);
  float *x = reinterpret_cast<float *>(w + plane);
  int32_t *flags = reinterpret_cast<int32_t *>(w + plane + row);
  PeakParams p;
  p.lag = lag, p.shift = lag + h->tab.n_fft / (2 * h->tab.hop);
  p.pre_max = pre_max, p.post_max = post_max, p.pre_avg = pre_avg, p.post_avg = post_avg, p.wait = wait, p.delta = delta;
  p.conf_interval = conf_interval, p.capacity = capacity;
  SF_HIP(launch_mel_power(h->tab, wav, B, L, mel, s));
  SF_HIP(launch_db_flux(mel, B, h->tab.n_mels, T, amin, (float)(10.0 * std::log10((double)amin)), top_db, lag, p.shift, nullptr, envelope, s));
  SF_HIP(launch_peak_pick(envelope, wav, B, T, L, h->tab.hop, p, x, flags, count, positions, confidence, strength, s));
  return SF_OK;
  SF_API_END
}

int sf_logmel_examples_count(const sf_audio_features *h, int L, int frames_per_example) {
  if (!h || h->tab.pad_mode != AUDIO_PAD_NONE || L < 1 || frames_per_example < 1) return -1;
  const int64_t F = L < h->win ? 0 : 1 + (int64_t)(L - h->win) / h->tab.hop;
  return (int)(F / frames_per_example);
}

int sf_logmel_examples_forward(sf_audio_features *h, const float *wav, int B, int L, int frames_per_example, float log_offset, float *examples,
                               float *mel, void *stream) {
  SF_API_BEGIN
  if (!h || !wav) fail(SF_ERR_INVALID, "null argument");
  if (!examples && !mel) fail(SF_ERR_INVALID, "null argument: neither examples nor mel asked for");
  if (h->tab.pad_mode != AUDIO_PAD_NONE) fail(SF_ERR_INVALID, "the handle was not made by sf_audio_features_create_framed");
  if (B < 1 || L < 1 || frames_per_example < 1) fail(SF_ERR_INVALID, "B, L and frames_per_example must be at least 1");
  if (!(log_offset > 0.f)) fail(SF_ERR_INVALID, "log_offset must be positive");
  if (B > 65535) fail(SF_ERR_SHAPE, "at most 65535 clips per call");
  const int E = sf_logmel_examples_count(h, L, frames_per_example);
  if (E < 1) fail(SF_ERR_SHAPE, "a clip of %d samples holds no example of %d frames (window %d, hop %d)", L, frames_per_example, h->win, h->tab.hop);
  const int64_t T = (int64_t)E * frames_per_example;
  if ((int64_t)B * T * h->tab.n_mels * 4 >= (1ll << 31) || T > 65535 * 16) fail(SF_ERR_SHAPE, "batch too large");
  upload(h);
  SF_HIP(launch_framed_logmel(h->tab, h->win, wav, B, L, (int)T, log_offset, examples, mel, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

}  // extern "C"
