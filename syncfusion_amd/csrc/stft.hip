// Complex STFT, inverse STFT and the spectral-gating denoiser (replaces noisereduce.reduce_noise at script/gh_preprocess_videos.py:91-100).
// fp32 throughout; window, twiddles and the smoothing taps are host-built fp64 tables rounded once.
//
//   stft_kernel          one workgroup per (row, frame): the frame is gathered into LDS with the padding resolved at load time, windowed,
//                        packed as n_fft / 2 complex points, transformed by the radix-2 Stockham FFT of the audio front end (a copy: the
//                        front end's arithmetic stays its own) and unpacked to the complex bins 0 .. n_fft / 2.
//   istft_frames_kernel  one workgroup per (row, frame): the bins are folded back into the packed half-length spectrum, the same stages
//                        run on its conjugate, and the windowed frame goes to scratch.
//   istft_ola_kernel     one thread per output sample: the frames that cover it are added in ascending frame order with the squared
//                        window beside them; no atomics.
//   ns_fwd / ns_bwd      lanes over bins, frames in sequence: the two passes of y = b x + (1 - b) y_prev and the sigmoid mask.  A block of
//                        frames is loaded before the dependent chain runs over it.
//   noise_thresh_kernel  one workgroup per row: plane maximum, then per bin the mean and, in a second pass, the deviation.
//   row_max / stat_mask  plane maximum per row, then the binary mask.
//   smooth_bins / smooth_frames_apply   the separable mask filter with zeros outside the plane, prop_decrease and the multiply into S.
// Every reduction runs in a fixed order and no row reads another row: a row's result does not depend on the batch around it.
#include <cfloat>

#include "stft.h"

namespace sf {

constexpr int ST_THREADS = 256;
constexpr int NS_THREADS = 64;      // one wave of bins per workgroup of the recurrence
constexpr int NS_BLOCK = 8;         // frames loaded ahead of the dependent chain

// ---- M-point Stockham radix-2 FFT in LDS ------------------------------------------------------------------------------------------------------
// lds: 4 arrays of M = n_fft / 2 floats; the first two hold the input (re, im) and the block is synchronised.  On return *zr / *zi point
// at the transform and *fr at the 2 M floats of the other image; the block is synchronised again.
__device__ __forceinline__ void fft_half(const StftTables &tab, float *lds, int tid, const float **zr, const float **zi, float **fr) {
  const int M = tab.n_fft >> 1;
  float *sr = lds, *si = lds + M, *dr = lds + 2 * M, *di = lds + 3 * M;
  const int half = M >> 1;
  for (int Ns = 1; Ns < M; Ns <<= 1) {
    const int tw_step = M / Ns;
    for (int j = tid; j < half; j += ST_THREADS) {
      const int k = j & (Ns - 1);
      const float wr = tab.tw_re[k * tw_step], wi = tab.tw_im[k * tw_step];
      const float ar = sr[j], ai = si[j];
      const float br = sr[j + half], bi = si[j + half];
      const float cr = br * wr - bi * wi, ci = br * wi + bi * wr;
      const int j0 = ((j - k) << 1) + k;
      dr[j0] = ar + cr;
      di[j0] = ai + ci;
      dr[j0 + Ns] = ar - cr;
      di[j0 + Ns] = ai - ci;
    }
    float *tr = sr, *ti = si;
    sr = dr, si = di, dr = tr, di = ti;
    __syncthreads();
  }
  *zr = sr, *zi = si, *fr = dr;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------------------
// dynamic LDS: 8 * n_fft bytes
__global__ __launch_bounds__(ST_THREADS) void stft_kernel(StftTables tab, const float *__restrict__ wav, int L, int T, float2 *__restrict__ spec) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int M = tab.n_fft >> 1;
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  float *sr = lds, *si = lds + M;
  const float *x = wav + (size_t)b * L;
  const long long start = (long long)t * tab.hop - tab.pad;

  for (int n = tid; n < M; n += ST_THREADS) {
    float v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = 2 * n + h;
      long long s = start + i;
      float xv = 0.f;
      if (i < tab.win) {               // the frame is zero-padded at its END up to n_fft points
        if (tab.pad_mode == STFT_PAD_REFLECT) {
          if (s < 0) s = -s;
          if (s >= L) s = 2ll * (L - 1) - s;   // L > pad (checked by the caller): one reflection always lands inside
          xv = x[s];
        } else if (s >= 0 && s < L) {
          xv = x[s];
        }
      }
      v[h] = xv * tab.window[i];
    }
    sr[n] = v[0];
    si[n] = v[1];
  }
  __syncthreads();

  const float *zr, *zi;
  float *unused;
  fft_half(tab, lds, tid, &zr, &zi, &unused);

  float2 *out = spec + ((size_t)b * T + t) * (M + 1);
  for (int k = tid; k <= M; k += ST_THREADS) {
    const int k0 = k & (M - 1), k1 = (M - k) & (M - 1);
    const float a = zr[k0], bb = zi[k0], c = zr[k1], d = zi[k1];
    const float er = 0.5f * (a + c), ei = 0.5f * (bb - d);
    const float orr = 0.5f * (bb + d), oi = -0.5f * (a - c);
    const float wr = tab.tw_re[k], wi = tab.tw_im[k];
    const float xr = er + (wr * orr - wi * oi);
    const float xi = ei + (wr * oi + wi * orr);
    out[k] = make_float2(xr * tab.fwd_scale, xi * tab.fwd_scale);
  }
}

// ---- inverse ------------------------------------------------------------------------------------------------------------------------------------
// X_k, k = 0 .. M, of a real frame -> Z_k = E_k + i O_k, k = 0 .. M - 1, with E_k = (X_k + conj X_{M-k}) / 2 the transform of the even samples
// and O_k = (X_k - conj X_{M-k}) / 2 * exp(+2 pi i k / n_fft) that of the odd ones; z = conj(FFT(conj Z)) / M, x[2n] = Re z[n], x[2n+1] = Im z[n].
// The imaginary parts of bins 0 and M do not enter (as in numpy's irfft).
__global__ __launch_bounds__(ST_THREADS) void istft_frames_kernel(StftTables tab, const float2 *__restrict__ spec, int T, float *__restrict__ frames) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int M = tab.n_fft >> 1;
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  float *sr = lds, *si = lds + M;
  const float2 *X = spec + ((size_t)b * T + t) * (M + 1);

  for (int k = tid; k < M; k += ST_THREADS) {
    float2 a = X[k], c = X[M - k];
    if (k == 0) a.y = 0.f, c.y = 0.f;
    const float er = 0.5f * (a.x + c.x), ei = 0.5f * (a.y - c.y);
    const float dr = 0.5f * (a.x - c.x), di = 0.5f * (a.y + c.y);
    const float wr = tab.tw_re[k], wi = -tab.tw_im[k];
    const float orr = dr * wr - di * wi, oi = dr * wi + di * wr;
    sr[k] = er - oi;                   // Re Z
    si[k] = -(ei + orr);               // -Im Z: the stages run on conj Z
  }
  __syncthreads();

  const float *zr, *zi;
  float *unused;
  fft_half(tab, lds, tid, &zr, &zi, &unused);

  const float sc = tab.inv_scale / (float)M;
  float *f = frames + ((size_t)b * T + t) * tab.win;
  for (int i = tid; i < tab.win; i += ST_THREADS) {
    const int n = i >> 1;
    const float xv = (i & 1) ? -zi[n] : zr[n];
    f[i] = xv * sc * tab.window[i];
  }
}

__global__ __launch_bounds__(ST_THREADS) void istft_ola_kernel(StftTables tab, const float *__restrict__ frames, int T, int n_valid,
                                                               float *__restrict__ out, int out_len) {
  const int j = blockIdx.x * ST_THREADS + threadIdx.x, b = blockIdx.y;
  if (j >= out_len) return;
  float r = 0.f;
  if (j < n_valid) {
    const long long p = (long long)j + tab.pad;            // position in the padded clip
    long long t_lo = p - tab.win + 1 <= 0 ? 0 : (p - tab.win + tab.hop) / tab.hop;   // ceil((p - win + 1) / hop)
    long long t_hi = p / tab.hop;
    if (t_hi > T - 1) t_hi = T - 1;
    float acc = 0.f, env = 0.f;
    for (long long t = t_lo; t <= t_hi; ++t) {             // ascending frames: a fixed order
      const int i = (int)(p - t * tab.hop);
      const float w = tab.window[i];
      acc += frames[((size_t)b * T + t) * tab.win + i];
      env += w * w;
    }
    r = acc / (env > 1e-10f ? env : 1.f);
  }
  out[(size_t)b * out_len + j] = r;
}

// ---- non-stationary mask ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float amp(float2 v) { return sqrtf(v.x * v.x + v.y * v.y); }

__global__ __launch_bounds__(NS_THREADS) void ns_fwd_kernel(const float2 *__restrict__ spec, int T, int F, float b, float *__restrict__ fwd) {
  const int f = blockIdx.x * NS_THREADS + threadIdx.x, row = blockIdx.y;
  if (f >= F) return;
  const float2 *S = spec + (size_t)row * T * F + f;
  float *Y = fwd + (size_t)row * T * F + f;
  const float c = 1.f - b;
  float prev = 0.f;
  for (int t0 = 0; t0 < T; t0 += NS_BLOCK) {
    float a[NS_BLOCK];
#pragma unroll
    for (int u = 0; u < NS_BLOCK; ++u) a[u] = t0 + u < T ? amp(S[(size_t)(t0 + u) * F]) : 0.f;   // independent of the recurrence
    if (t0 == 0) prev = a[0];
#pragma unroll
    for (int u = 0; u < NS_BLOCK; ++u)
      if (t0 + u < T) {
        prev = b * a[u] + c * prev;
        Y[(size_t)(t0 + u) * F] = prev;
      }
  }
}

__global__ __launch_bounds__(NS_THREADS) void ns_bwd_kernel(const float2 *__restrict__ spec, const float *__restrict__ fwd, int T, int F, float b,
                                                            float mult, float slope, float *__restrict__ mask) {
  const int f = blockIdx.x * NS_THREADS + threadIdx.x, row = blockIdx.y;
  if (f >= F) return;
  const float2 *S = spec + (size_t)row * T * F + f;
  const float *Y = fwd + (size_t)row * T * F + f;
  float *Mk = mask + (size_t)row * T * F + f;
  const float c = 1.f - b;
  float prev = 0.f;
  for (int t0 = T - 1; t0 >= 0; t0 -= NS_BLOCK) {
    float a[NS_BLOCK], y[NS_BLOCK];
#pragma unroll
    for (int u = 0; u < NS_BLOCK; ++u) {
      const bool in = t0 - u >= 0;
      a[u] = in ? amp(S[(size_t)(t0 - u) * F]) : 0.f;
      y[u] = in ? Y[(size_t)(t0 - u) * F] : 0.f;
    }
    if (t0 == T - 1) prev = y[0];
#pragma unroll
    for (int u = 0; u < NS_BLOCK; ++u)
      if (t0 - u >= 0) {
        prev = b * y[u] + c * prev;
        const float sm = prev;
        float m = 0.f;                 // a bin silent in every frame: 0 / 0 in the reference, 0 here (the output bin is 0 either way)
        if (sm != 0.f) m = 1.f / (1.f + expf(-(((a[u] - sm) / sm - mult) * slope)));
        Mk[(size_t)(t0 - u) * F] = m;
      }
  }
}

// ---- stationary mask ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_max(float v, float *red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = ST_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ float plane_max(const float2 *S, size_t n, float *red) {
  float mx = 0.f;
  for (size_t i = threadIdx.x; i < n; i += ST_THREADS) mx = fmaxf(mx, amp(S[i]));
  return block_max(mx, red);
}

__device__ __forceinline__ float floor_db_of(float mx) { return 20.f * log10f(fmaxf(mx, 1e-20f)) - 80.f; }
__device__ __forceinline__ float amp_db(float2 v, float floor_db) { return fmaxf(20.f * log10f(fmaxf(amp(v), 1e-20f)), floor_db); }

// mean and deviation are taken relative to the bin's first frame: a constant column gives its value and a deviation of exactly 0
__global__ __launch_bounds__(ST_THREADS) void noise_thresh_kernel(const float2 *__restrict__ spec, int T, int F, float n_std, float *__restrict__ thresh) {
  __shared__ float red[ST_THREADS];
  const int row = blockIdx.x;
  const float2 *S = spec + (size_t)row * T * F;
  const float floor_db = floor_db_of(plane_max(S, (size_t)T * F, red));
  for (int f = threadIdx.x; f < F; f += ST_THREADS) {
    const float v0 = amp_db(S[f], floor_db);
    float sum = 0.f;
    for (int t = 0; t < T; ++t) sum += amp_db(S[(size_t)t * F + f], floor_db) - v0;
    const float mean = v0 + sum / (float)T;
    float dev = 0.f;
    for (int t = 0; t < T; ++t) {      // second pass: no E[x^2] - E[x]^2
      const float d = amp_db(S[(size_t)t * F + f], floor_db) - mean;
      dev += d * d;
    }
    thresh[(size_t)row * F + f] = mean + n_std * sqrtf(dev / (float)T);
  }
}

__global__ __launch_bounds__(ST_THREADS) void row_max_kernel(const float2 *__restrict__ spec, int T, int F, float *__restrict__ rowmax) {
  __shared__ float red[ST_THREADS];
  const int row = blockIdx.x;
  const float mx = plane_max(spec + (size_t)row * T * F, (size_t)T * F, red);
  if (threadIdx.x == 0) rowmax[row] = mx;
}

__global__ __launch_bounds__(ST_THREADS) void stat_mask_kernel(const float2 *__restrict__ spec, int T, int F, const float *__restrict__ thresh,
                                                               const float *__restrict__ rowmax, float *__restrict__ mask) {
  const int t = blockIdx.x, row = blockIdx.y;
  const float floor_db = floor_db_of(rowmax[row]);
  const size_t base = ((size_t)row * T + t) * F;
  for (int f = threadIdx.x; f < F; f += ST_THREADS) mask[base + f] = amp_db(spec[base + f], floor_db) > thresh[(size_t)row * F + f] ? 1.f : 0.f;
}

// ---- mask smoothing -------------------------------------------------------------------------------------------------------------------------------
// out[f] = sum_i taps[i] m[f + n - i], n = (n_taps - 1) / 2, zeros outside 0 .. F - 1 (fftconvolve, mode "same")
__global__ __launch_bounds__(ST_THREADS) void smooth_bins_kernel(StftTables tab, const float *__restrict__ mask, int T, int F, float prop, int prop_first,
                                                                 float *__restrict__ tmp) {
  const int t = blockIdx.x, row = blockIdx.y;
  const size_t base = ((size_t)row * T + t) * F;
  const int n = (tab.n_ftaps - 1) >> 1;
  const float keep = 1.f - prop;
  for (int f = threadIdx.x; f < F; f += ST_THREADS) {
    float acc = 0.f;
    const int i_lo = max(0, f + n - (F - 1)), i_hi = min(tab.n_ftaps - 1, f + n);
    for (int i = i_lo; i <= i_hi; ++i) {
      float m = mask[base + f + n - i];
      if (prop_first) m = m * prop + keep;
      acc += tab.ftaps[i] * m;
    }
    tmp[base + f] = acc;
  }
}

__global__ __launch_bounds__(ST_THREADS) void smooth_frames_apply_kernel(StftTables tab, const float *__restrict__ tmp, int T, int F, float prop,
                                                                         int prop_first, const float2 *__restrict__ spec,
                                                                         float *__restrict__ mask_smooth, float2 *__restrict__ spec_out) {
  const int t = blockIdx.x, row = blockIdx.y;
  const size_t plane = (size_t)row * T * F;
  const int n = (tab.n_ttaps - 1) >> 1;
  const int j_lo = max(0, t + n - (T - 1)), j_hi = min(tab.n_ttaps - 1, t + n);
  for (int f = threadIdx.x; f < F; f += ST_THREADS) {
    float acc = 0.f;
    for (int j = j_lo; j <= j_hi; ++j) acc += tab.ttaps[j] * tmp[plane + (size_t)(t + n - j) * F + f];
    const float m = prop_first ? acc : acc * prop + (1.f - prop);
    const size_t o = plane + (size_t)t * F + f;
    mask_smooth[o] = m;
    const float2 v = spec[o];
    spec_out[o] = make_float2(v.x * m, v.y * m);
  }
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------------
static int64_t round256(int64_t n) { return (n + 255) / 256 * 256; }

int64_t gate_ws_bytes(const StftTables &tab, int B, int L) {
  const int64_t T = stft_frames(L, tab.win, tab.hop, tab.pad), F = tab.n_fft / 2 + 1;
  return round256((int64_t)B * T * F * 4) + round256((int64_t)B * T * F * 8) + round256((int64_t)B * T * tab.win * 4) + round256((int64_t)B * 4);
}

hipError_t launch_stft(const StftTables &tab, const float *wav, int B, int L, int T, float *spec, hipStream_t s) {
  if (B < 1 || B > 65535 || T < 1 || T != stft_frames(L, tab.win, tab.hop, tab.pad)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(stft_kernel, dim3(T, B), dim3(ST_THREADS), (size_t)8 * tab.n_fft, s, tab, wav, L, T, reinterpret_cast<float2 *>(spec));
  return hipGetLastError();
}

hipError_t launch_istft(const StftTables &tab, const float *spec, int B, int T, float *frames, float *out, int out_len, hipStream_t s) {
  const int64_t n_valid = istft_samples(T, tab.win, tab.hop, tab.pad);
  if (B < 1 || B > 65535 || T < 1 || out_len < 1 || n_valid < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(istft_frames_kernel, dim3(T, B), dim3(ST_THREADS), (size_t)8 * tab.n_fft, s, tab, reinterpret_cast<const float2 *>(spec), T, frames);
  hipLaunchKernelGGL(istft_ola_kernel, dim3((out_len + ST_THREADS - 1) / ST_THREADS, B), dim3(ST_THREADS), 0, s, tab, frames, T,
                     (int)(n_valid < out_len ? n_valid : out_len), out, out_len);
  return hipGetLastError();
}

hipError_t launch_ns_mask(const float *spec, int B, int T, int F, float b, float mult, float slope, float *fwd, float *mask, hipStream_t s) {
  const dim3 grid((F + NS_THREADS - 1) / NS_THREADS, B);
  hipLaunchKernelGGL(ns_fwd_kernel, grid, dim3(NS_THREADS), 0, s, reinterpret_cast<const float2 *>(spec), T, F, b, fwd);
  hipLaunchKernelGGL(ns_bwd_kernel, grid, dim3(NS_THREADS), 0, s, reinterpret_cast<const float2 *>(spec), fwd, T, F, b, mult, slope, mask);
  return hipGetLastError();
}

hipError_t launch_noise_thresh(const float *spec, int B, int T, int F, float n_std, float *thresh, hipStream_t s) {
  hipLaunchKernelGGL(noise_thresh_kernel, dim3(B), dim3(ST_THREADS), 0, s, reinterpret_cast<const float2 *>(spec), T, F, n_std, thresh);
  return hipGetLastError();
}

hipError_t launch_stat_mask(const float *spec, int B, int T, int F, const float *thresh, float *rowmax, float *mask, hipStream_t s) {
  hipLaunchKernelGGL(row_max_kernel, dim3(B), dim3(ST_THREADS), 0, s, reinterpret_cast<const float2 *>(spec), T, F, rowmax);
  hipLaunchKernelGGL(stat_mask_kernel, dim3(T, B), dim3(ST_THREADS), 0, s, reinterpret_cast<const float2 *>(spec), T, F, thresh, rowmax, mask);
  return hipGetLastError();
}

hipError_t launch_smooth_apply(const StftTables &tab, const float *mask_raw, int B, int T, int F, float prop, int prop_first, const float *spec,
                               float *tmp, float *mask_smooth, float *spec_out, hipStream_t s) {
  hipLaunchKernelGGL(smooth_bins_kernel, dim3(T, B), dim3(ST_THREADS), 0, s, tab, mask_raw, T, F, prop, prop_first, tmp);
  hipLaunchKernelGGL(smooth_frames_apply_kernel, dim3(T, B), dim3(ST_THREADS), 0, s, tab, tmp, T, F, prop, prop_first,
                     reinterpret_cast<const float2 *>(spec), mask_smooth, reinterpret_cast<float2 *>(spec_out));
  return hipGetLastError();
}

}  // namespace sf
