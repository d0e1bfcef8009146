#include "engine_common.h"

#include <cstring>

namespace sf {

static thread_local std::string g_err;

void set_error(const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
}
const char *get_error() { return g_err.c_str(); }

void fail(int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  throw EngineError{code};
}

WeightMap::WeightMap(const sf_tensor *w, int n) {
  for (int i = 0; i < n; ++i) {
    if (!w[i].name) continue;
    map_[w[i].name] = {w[i].data, w[i].numel};
  }
}

const float *WeightMap::get(const std::string &name, int64_t numel) const {
  auto it = map_.find(name);
  if (it == map_.end()) fail(SF_ERR_MISSING_WEIGHT, "missing parameter '%s'", name.c_str());
  if (it->second.second != numel)
    fail(SF_ERR_MISSING_WEIGHT, "parameter '%s' has %lld elements, expected %lld", name.c_str(), (long long)it->second.second,
         (long long)numel);
  if (!it->second.first) fail(SF_ERR_MISSING_WEIGHT, "parameter '%s' has a null pointer", name.c_str());
  return static_cast<const float *>(it->second.first);
}

void WeightWants::load(const WeightMap &wm, DeviceArena &arena, hipStream_t s) const {
  for (const Want &w : list_) (void)wm.get(w.name, w.n);
  for (const Want &w : list_) {
    *w.dst = arena.alloc_n<float>(w.n);
    SF_HIP(hipMemcpyAsync(*w.dst, wm.get(w.name, w.n), (size_t)w.n * 4, hipMemcpyDeviceToDevice, s));
  }
}

ConvGemmPlan plan_linear(const LinearDesc &g) {
  // what the plan needs is whether a pointer is set, not where it points
  alignas(16) static float some[4];
  return conv_gemm_plan(F32, token_linear_args(some, g.items, g.tokens, g.K, g.N, some, some, g.res ? some : nullptr, g.act, some));
}

void require_gemm_kernels(const std::vector<LinearDesc> &list) {
  for (const LinearDesc &g : list)
    if (plan_linear(g).family == CG_INVALID)
      fail(SF_ERR_UNSUPPORTED, "%s (M %lld, N %d, K %d): no GEMM kernel takes the shape", g.name.c_str(), g.rows(), g.N, g.K);
}

void describe_gemms(const std::vector<LinearDesc> &list, const std::string &suffix, char *text, int64_t capacity) {
  std::string s;
  for (const LinearDesc &g : list) {
    char line[256];
    snprintf(line, sizeof line, "%s%s: M %lld N %d K %d -> %s\n", g.name.c_str(), suffix.c_str(), g.rows(), g.N, g.K, plan_linear(g).label);
    s += line;
  }
  if ((int64_t)s.size() + 1 > capacity) fail(SF_ERR_INVALID, "text capacity %lld below %lld", (long long)capacity, (long long)s.size() + 1);
  memcpy(text, s.c_str(), s.size() + 1);
}

DeviceArena::~DeviceArena() {
  for (void *p : chunks_) (void)hipFree(p);
}

void *DeviceArena::alloc(int64_t bytes) {
  bytes = align_up(bytes > 0 ? bytes : 1, 256);
  if (bytes > left_) {
    int64_t chunk = bytes > (64ll << 20) ? bytes : (64ll << 20);
    void *p = nullptr;
    SF_HIP(hipMalloc(&p, (size_t)chunk));
    chunks_.push_back(p);
    cur_ = static_cast<char *>(p);
    left_ = chunk;
  }
  void *r = cur_;
  cur_ += bytes;
  left_ -= bytes;
  total_ += bytes;
  return r;
}

float *Packer::copy_f32(const std::string &name, int64_t numel) {
  const float *src = wm.get(name, numel);
  float *dst = arena.alloc_n<float>(numel);
  SF_HIP(hipMemcpyAsync(dst, src, numel * sizeof(float), hipMemcpyDeviceToDevice, s));
  return dst;
}

ConvW Packer::conv(const std::string &wname, const float *bias_dev, int N, int Cin, int taps, bool direct, int cin_pad,
                   const float *nscale, int k_multiple) {
  ConvW c;
  c.N = N;
  c.taps = taps;
  c.direct = direct;
  c.cin = direct ? Cin : cin_pad;
  c.cin2 = 0;
  const int kreal = taps * c.cin;
  c.K = pad_to(kreal, k_multiple);
  const float *w = wm.get(wname, (int64_t)N * Cin * taps);
  const int wdt = direct ? F32 : dt;
  c.w = arena.alloc((int64_t)N * c.K * dsize(wdt));
  if (c.K != kreal) SF_HIP(hipMemsetAsync(c.w, 0, (int64_t)N * c.K * dsize(wdt), s));
  SF_HIP(launch_pack_conv(wdt, w, N, Cin, 0, Cin, taps, c.cin, nscale, c.w, c.K, 0, s));
  c.bias = const_cast<float *>(bias_dev);
  return c;
}

ConvW Packer::linear(const std::string &pre, int N, int K, bool bias) {
  ConvW c;
  c.N = N;
  c.K = K;
  c.cin = K;
  c.taps = 1;
  const float *w = wm.get(pre + ".weight", (int64_t)N * K);
  c.w = arena.alloc((int64_t)N * K * dsize(dt));
  SF_HIP(launch_pack_rows(dt, w, N, K, K, nullptr, c.w, K, s));
  if (bias) c.bias = copy_f32(pre + ".bias", N);
  return c;
}

void DebugTaps::tap(const std::string &name, int dt, const void *x, int ld, int64_t rows, int cols, hipStream_t s) {
  if (!buf) return;
  int64_t n = rows * cols;
  if (used + n > cap) fail(SF_ERR_WORKSPACE, "debug buffer too small at tap '%s'", name.c_str());
  SF_HIP(launch_to_f32(dt, x, ld, rows, cols, buf + used, s));
  entries.push_back({name, used, rows, cols});
  used += n;
}

void DebugTaps::tap_clips(const std::string &name, int dt, const void *x, int ld, int64_t rows_per_clip, int n_clips, int cols, int path,
                          hipStream_t s) {
  if (!buf) return;
  if (clips.empty()) {
    tap(name, dt, x, ld, rows_per_clip * n_clips, cols, s);
    entries.back().path = path;
    return;
  }
  const int64_t per = rows_per_clip * cols, n = per * (int64_t)clips.size();
  if (used + n > cap) fail(SF_ERR_WORKSPACE, "debug buffer too small at tap '%s'", name.c_str());
  int64_t at = used;
  for (int c : clips) {
    if (c < 0 || c >= n_clips) fail(SF_ERR_INVALID, "debug clip %d outside the batch of %d", c, n_clips);
    SF_HIP(launch_to_f32(dt, static_cast<const char *>(x) + (size_t)c * rows_per_clip * ld * dsize(dt), ld, rows_per_clip, cols, buf + at, s));
    at += per;
  }
  entries.push_back({name, used, rows_per_clip * (int64_t)clips.size(), cols, path});
  used += n;
}

}  // namespace sf
