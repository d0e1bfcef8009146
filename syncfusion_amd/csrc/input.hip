// Input side of the path, on the device:
//   * frames_preprocess: decoded uint8 RGB frames (N, T, H, W, 3) -> the onset net's input (N, 3, T, oh, ow) fp32, i.e. the
//     reference's ToTensor -> Resize((112, 112), antialias=True) -> Normalize(mean, std) -> (C, T, H, W) chain
//     (main/dataset_onset.py:47-50,152-165) in ONE pass over the pixels: the antialiased bilinear filter is ATen's separable
//     triangle filter (support = scale when downscaling, weights normalised per output pixel, align_corners = False);
//   * times_to_track: onset times (seconds) -> one-hot impulse track, `track[:, int(t * sr)] = 1` (main/dataset_diffusion.py:58-72),
//     evaluated in double precision like the Python expression.
#include "common.h"
#include "kernels.h"

namespace sf {
namespace {

constexpr int kMaxTaps = 16;

struct AaAxis {
  int first, size;
  float w[kMaxTaps];
};
// ATen `_compute_indices_min_size_weights_aa` for one output index (bilinear: interp_size 2)
__device__ __forceinline__ AaAxis aa_axis(int i, int in_size, float scale) {
  AaAxis a;
  const float support = scale >= 1.0f ? scale : 1.0f;
  const float invscale = scale >= 1.0f ? 1.0f / scale : 1.0f;
  const float center = scale * ((float)i + 0.5f);
  a.first = max((int)(center - support + 0.5f), 0);
  a.size = min(min((int)(center + support + 0.5f), in_size) - a.first, kMaxTaps);
  float tot = 0.f;
  for (int j = 0; j < kMaxTaps; ++j) {
    float w = 0.f;
    if (j < a.size) w = fmaxf(0.f, 1.0f - fabsf(((float)(j + a.first) - center + 0.5f) * invscale));
    a.w[j] = w;
    tot += w;
  }
  const float inv = tot != 0.f ? 1.0f / tot : 0.f;
  for (int j = 0; j < kMaxTaps; ++j) a.w[j] *= inv;
  return a;
}

struct Rgb {
  float r, g, b;
};
// One pixel of the antialiased resize: output index (y, x) of the RESIZED image (a crop passes top + oy, left + ox), scale = in / resized
__device__ __forceinline__ Rgb aa_pixel(const unsigned char *__restrict__ img, int H, int W, int y, int x, float sy, float sx) {
  const AaAxis ay = aa_axis(y, H, sy), ax = aa_axis(x, W, sx);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int j = 0; j < ay.size; ++j) {
    const unsigned char *row = img + ((size_t)(ay.first + j) * W + ax.first) * 3;
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;   // horizontal pass first, like ATen's separable implementation
    for (int i = 0; i < ax.size; ++i) {
      const float w = ax.w[i];
      r0 = fmaf((float)row[3 * i + 0] * (1.0f / 255.0f), w, r0);
      r1 = fmaf((float)row[3 * i + 1] * (1.0f / 255.0f), w, r1);
      r2 = fmaf((float)row[3 * i + 2] * (1.0f / 255.0f), w, r2);
    }
    a0 = fmaf(r0, ay.w[j], a0);
    a1 = fmaf(r1, ay.w[j], a1);
    a2 = fmaf(r2, ay.w[j], a2);
  }
  return Rgb{a0, a1, a2};
}

__global__ void frames_preprocess_kernel(const unsigned char *__restrict__ fr, int NT, int T, int H, int W, int oh, int ow, float sy, float sx,
                                         float m0, float m1, float m2, float is0, float is1, float is2, float *__restrict__ out) {
  const int64_t total = (int64_t)NT * oh * ow;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int ox = (int)(idx % ow);
    const int64_t r = idx / ow;
    const int oy = (int)(r % oh);
    const int nt = (int)(r / oh);
    const Rgb a = aa_pixel(fr + (size_t)nt * H * W * 3, H, W, oy, ox, sy, sx);
    const int n = nt / T, t = nt - n * T;
    const size_t plane = (size_t)oh * ow;
    float *o = out + (((size_t)n * 3) * T + t) * plane + (size_t)oy * ow + ox;
    o[0] = (a.r - m0) * is0;
    o[(size_t)T * plane] = (a.g - m1) * is1;
    o[2 * (size_t)T * plane] = (a.b - m2) * is2;
  }
}

// ---- training transforms: Resize -> crop -> ColorJitter -> Normalize (cfg/data/data-onset-greatesthit-augment.yaml:8-28) -------------------
// Colour operations on a float RGB triple as torchvision 0.14.1 defines them for float tensors (transforms/functional_tensor.py):
// _blend(a, b, f) = clamp(f a + (1 - f) b, 0, 1); gray = 0.2989 r + 0.587 g + 0.114 b.
__device__ __forceinline__ float blend1(float a, float b, float f) { return fminf(fmaxf(f * a + (1.0f - f) * b, 0.f), 1.f); }
__device__ __forceinline__ float gray_of(const Rgb &c) { return 0.2989f * c.r + 0.587f * c.g + 0.114f * c.b; }
// adjust_hue: _rgb2hsv, h <- (h + f) mod 1, _hsv2rgb
__device__ __forceinline__ Rgb hue_shift(const Rgb &c, float f) {
  const float maxc = fmaxf(c.r, fmaxf(c.g, c.b)), minc = fminf(c.r, fminf(c.g, c.b));
  const bool eq = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eq ? 1.0f : maxc);
  const float div = eq ? 1.0f : cr;
  const float rc = (maxc - c.r) / div, gc = (maxc - c.g) / div, bc = (maxc - c.b) / div;
  float h;
  if (maxc == c.r) h = bc - gc;
  else if (maxc == c.g) h = 2.0f + rc - bc;
  else h = 4.0f + gc - rc;
  h = fmodf(h / 6.0f + 1.0f, 1.0f);
  h = h + f;
  h = h - floorf(h);            // Python's % 1.0 (h + f lies in (-0.5, 1.5))
  if (h >= 1.0f) h = 0.f;       // -tiny - floor(-tiny) rounds to 1.0 in fp32; torch.remainder returns a value in [0, 1)
  const float h6 = h * 6.0f;
  const float fl = floorf(h6);
  const float fr = h6 - fl;
  int i = (int)fl % 6;
  const float v = maxc;
  const float p = fminf(fmaxf(v * (1.0f - s), 0.f), 1.f);
  const float q = fminf(fmaxf(v * (1.0f - s * fr), 0.f), 1.f);
  const float t = fminf(fmaxf(v * (1.0f - s * (1.0f - fr)), 0.f), 1.f);
  switch (i) {
    case 0: return Rgb{v, t, p};
    case 1: return Rgb{q, v, p};
    case 2: return Rgb{p, v, t};
    case 3: return Rgb{p, q, v};
    case 4: return Rgb{t, p, v};
    default: return Rgb{v, p, q};
  }
}
// op: 0 brightness, 1 contrast (m = the frame's mean gray), 2 saturation, 3 hue -- ColorJitter.forward's fn_id
__device__ __forceinline__ Rgb colour_op(int op, float f, Rgb c, float m) {
  if (op == 0) return Rgb{blend1(c.r, 0.f, f), blend1(c.g, 0.f, f), blend1(c.b, 0.f, f)};
  if (op == 1) return Rgb{blend1(c.r, m, f), blend1(c.g, m, f), blend1(c.b, m, f)};
  if (op == 2) {
    const float g = gray_of(c);
    return Rgb{blend1(c.r, g, f), blend1(c.g, g, f), blend1(c.b, g, f)};
  }
  return hue_shift(c, f);
}

constexpr int kAugBlock = 256;

// Pass A.  One thread per output pixel, kAugBlock consecutive pixels of ONE frame per block (bpf blocks per frame), so that a wave stores
// contiguous ox and a block's gray partial belongs to one frame.  Gather (resize + crop), then the clip's colour operations in its order
// up to, excluding, contrast.  A clip without contrast is finished here (Normalize included); a clip with contrast leaves the unnormalised
// RGB in `out` and the block's gray sum in part[frame * bpf + block] (fixed order: wave butterfly, then the 4 wave sums in wave order).
__global__ __launch_bounds__(kAugBlock) void frames_augment_a_kernel(const unsigned char *__restrict__ fr, const AugClip *__restrict__ tab, int T, int H,
                                                                     int W, int oh, int ow, int bpf, float sy, float sx, float m0, float m1, float m2,
                                                                     float is0, float is1, float is2, float *__restrict__ out,
                                                                     float *__restrict__ part) {
  __shared__ float wsum[kAugBlock / 64];
  const int nt = blockIdx.x / bpf, bx = blockIdx.x - nt * bpf;
  const int n = nt / T, t = nt - n * T;
  const AugClip &cl = tab[n];   // block-uniform: read through the scalar cache
  const int plane = oh * ow;
  const int pix = bx * kAugBlock + threadIdx.x;
  const bool live = pix < plane;
  int stop = 4;   // position of contrast in the clip's order (4: absent)
  for (int k = 0; k < 4; ++k)
    if (cl.order[k] == 1 && (cl.mask & 2)) stop = k;
  Rgb c{0.f, 0.f, 0.f};
  float *o = nullptr;
  if (live) {
    const int oy = pix / ow, ox = pix - oy * ow;
    c = aa_pixel(fr + (size_t)nt * H * W * 3, H, W, cl.top + oy, cl.left + ox, sy, sx);
    for (int k = 0; k < stop; ++k) {
      const int op = cl.order[k];
      if ((cl.mask >> op) & 1) c = colour_op(op, cl.factor[op], c, 0.f);
    }
    o = out + (((size_t)n * 3) * T + t) * plane + pix;
  }
  if (stop == 4) {
    if (live) {
      o[0] = (c.r - m0) * is0;
      o[(size_t)T * plane] = (c.g - m1) * is1;
      o[2 * (size_t)T * plane] = (c.b - m2) * is2;
    }
    return;   // (block-uniform: a block lies inside one clip)
  }
  if (live) {
    o[0] = c.r;
    o[(size_t)T * plane] = c.g;
    o[2 * (size_t)T * plane] = c.b;
  }
  const float g = wave_sum(live ? gray_of(c) : 0.f);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = g;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < kAugBlock / 64; ++w) s += wsum[w];
    part[(size_t)nt * bpf + bx] = s;
  }
}

// Pass B (clips with contrast only; the other blocks leave at once): the frame's mean gray = its bpf partials summed in block order (every
// thread reads the same bpf floats: one broadcast line), contrast, the operations after it, Normalize -- in place on pass A's fp32 RGB.
__global__ __launch_bounds__(kAugBlock) void frames_augment_b_kernel(const AugClip *__restrict__ tab, int T, int oh, int ow, int bpf, float m0, float m1,
                                                                     float m2, float is0, float is1, float is2, float *__restrict__ out,
                                                                     const float *__restrict__ part) {
  const int nt = blockIdx.x / bpf, bx = blockIdx.x - nt * bpf;
  const int n = nt / T, t = nt - n * T;
  const AugClip &cl = tab[n];   // block-uniform: read through the scalar cache
  int stop = 4;
  for (int k = 0; k < 4; ++k)
    if (cl.order[k] == 1 && (cl.mask & 2)) stop = k;
  if (stop == 4) return;
  const int plane = oh * ow;
  const int pix = bx * kAugBlock + threadIdx.x;
  if (pix >= plane) return;
  float s = 0.f;
  for (int b = 0; b < bpf; ++b) s += part[(size_t)nt * bpf + b];
  const float mean = s / (float)plane;
  float *o = out + (((size_t)n * 3) * T + t) * plane + pix;
  Rgb c{o[0], o[(size_t)T * plane], o[2 * (size_t)T * plane]};
  c = colour_op(1, cl.factor[1], c, mean);
  for (int k = stop + 1; k < 4; ++k) {
    const int op = cl.order[k];
    if ((cl.mask >> op) & 1) c = colour_op(op, cl.factor[op], c, 0.f);
  }
  o[0] = (c.r - m0) * is0;
  o[(size_t)T * plane] = (c.g - m1) * is1;
  o[2 * (size_t)T * plane] = (c.b - m2) * is2;
}

__global__ void times_to_track_kernel(const double *__restrict__ times, const int *__restrict__ clip_of, int n_times, double sample_rate, int L,
                                      float *__restrict__ track) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_times) return;
  const long long pos = (long long)(times[i] * sample_rate);   // Python int(): truncation toward zero
  if (pos >= 0 && pos < L) track[(size_t)clip_of[i] * L + pos] = 1.0f;
}

}  // namespace

hipError_t launch_frames_preprocess(const unsigned char *frames, int N, int T, int H, int W, int oh, int ow, const float *mean, const float *stdv,
                                    float *out, hipStream_t s) {
  const float sy = (float)H / (float)oh, sx = (float)W / (float)ow;
  if (sy > (kMaxTaps - 1) / 2.0f || sx > (kMaxTaps - 1) / 2.0f) return hipErrorInvalidValue;   // filter wider than the tap table
  const int64_t total = (int64_t)N * T * oh * ow;
  const int grid = (int)std::min<int64_t>((total + 255) / 256, 65535);
  hipLaunchKernelGGL(frames_preprocess_kernel, dim3(grid), dim3(256), 0, s, frames, N * T, T, H, W, oh, ow, sy, sx, mean[0], mean[1], mean[2],
                     1.0f / stdv[0], 1.0f / stdv[1], 1.0f / stdv[2], out);
  return hipGetLastError();
}

int64_t frames_augment_workspace_bytes(int N, int T, int oh, int ow) {
  const int64_t bpf = ((int64_t)oh * ow + kAugBlock - 1) / kAugBlock;
  return (int64_t)N * T * bpf * sizeof(float);   // the per-frame gray partials of the contrast mean
}

hipError_t launch_frames_augment(const unsigned char *frames, int N, int T, int H, int W, int rh, int rw, int oh, int ow, const AugClip *table_dev,
                                 bool any_contrast, const float *mean, const float *stdv, float *out, float *part, hipStream_t s) {
  const float sy = (float)H / (float)rh, sx = (float)W / (float)rw;   // the scale of the RESIZE: the crop only selects pixels
  if (sy > (kMaxTaps - 1) / 2.0f || sx > (kMaxTaps - 1) / 2.0f) return hipErrorInvalidValue;   // filter wider than the tap table
  const int64_t bpf = ((int64_t)oh * ow + kAugBlock - 1) / kAugBlock;
  const int64_t blocks = (int64_t)N * T * bpf;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const float is0 = 1.0f / stdv[0], is1 = 1.0f / stdv[1], is2 = 1.0f / stdv[2];
  hipLaunchKernelGGL(frames_augment_a_kernel, dim3((unsigned)blocks), dim3(kAugBlock), 0, s, frames, table_dev, T, H, W, oh, ow, (int)bpf, sy, sx, mean[0],
                     mean[1], mean[2], is0, is1, is2, out, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !any_contrast) return e;
  hipLaunchKernelGGL(frames_augment_b_kernel, dim3((unsigned)blocks), dim3(kAugBlock), 0, s, table_dev, T, oh, ow, (int)bpf, mean[0], mean[1], mean[2], is0,
                     is1, is2, out, part);
  return hipGetLastError();
}

hipError_t launch_times_to_track(const double *times, const int *clip_of, int n_times, double sample_rate, int B, int L, float *track, hipStream_t s) {
  hipError_t e = hipMemsetAsync(track, 0, (size_t)B * L * sizeof(float), s);
  if (e != hipSuccess || n_times == 0) return e;
  hipLaunchKernelGGL(times_to_track_kernel, dim3((n_times + 255) / 256), dim3(256), 0, s, times, clip_of, n_times, sample_rate, L, track);
  return hipGetLastError();
}

}  // namespace sf
