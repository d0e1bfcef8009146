// Audio front end of the onset-sync evaluation: log-mel spectrogram, spectral-flux onset envelope and peak picking
// (replaces librosa.onset.onset_detect in script/evaluate_onset.py:30 and the MelSpectrogram + power_to_db pair of
// main/module_diffusion.py:120-152).  fp32 throughout; window, twiddles and the filterbank are host-built fp64 tables rounded once.
//
//   mel_power_kernel   one workgroup per (clip, frame).  The centred frame is gathered into LDS with the padding resolved at load time and
//                      multiplied by the window; even / odd samples are packed as one complex sequence of n_fft / 2 points, transformed by a
//                      radix-2 Stockham FFT that ping-pongs between two LDS images (real and imaginary parts in separate arrays: every access
//                      is a 4-byte one at consecutive or stride-2 addresses), and unpacked to the n_fft / 2 + 1 bins of the real transform.
//                      |X|^2 goes back to LDS and each triangular filter sums its own contiguous bin range.
//   db_flux_kernel     one workgroup per clip: plane maximum, then 10 log10 with the top_db floor and the mean positive frame difference.
//   peak_pick_kernel   one workgroup per clip: normalise, the two window tests per frame in parallel, the greedy `wait` pass by one lane,
//                      then the waveform confidences of the onsets found.
// Every reduction runs in a fixed order and no clip reads another clip's data: a clip's result does not depend on the batch around it.
#include <cfloat>

#include "audio_features.h"

namespace sf {

constexpr int AF_THREADS = 256;

// ---- block reductions (fixed tree, result broadcast to every thread) ------------------------------------------------------------------------
template <bool IS_MAX> __device__ __forceinline__ float block_reduce(float v, float *red) {
  const int tid = threadIdx.x;
  __syncthreads();   // red may still be read from a previous reduction
  red[tid] = v;
  __syncthreads();
  for (int s = AF_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = IS_MAX ? fmaxf(red[tid], red[tid + s]) : fminf(red[tid], red[tid + s]);
    __syncthreads();
  }
  return red[0];
}

// ---- real FFT of the packed frame in LDS ------------------------------------------------------------------------------------------------------
// lds: 4 arrays of M = n_fft / 2 floats.  On entry the first two hold z[n] = x[2n] + i x[2n + 1] (already windowed) and the block is
// synchronised; on return the pointer given back holds bins 0 .. M of the real transform, |X_k|^2 (MAGNITUDE = false) or |X_k| (true),
// and the block is synchronised again.  Shared by the centred power front end and the uncentred magnitude one: one FFT in the library.
template <bool MAGNITUDE> __device__ __forceinline__ const float *real_fft_bins(const AudioTables &tab, float *lds, int tid) {
  const int N = tab.n_fft, M = N >> 1;
  float *sr = lds, *si = lds + M, *dr = lds + 2 * M, *di = lds + 3 * M;   // source / destination images, swapped after every stage
  // Stockham radix-2, M points, log2(M) stages
  const int half = M >> 1;
  for (int Ns = 1; Ns < M; Ns <<= 1) {
    const int tw_step = M / Ns;        // exp(-2 pi i k / (2 Ns)) = table[k * M / Ns] of the n_fft-point table
    for (int j = tid; j < half; j += AF_THREADS) {
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

  // unpack to the real transform's bins 0 .. M; power or magnitude
  const float *zr = sr, *zi = si;
  float *pw = dr;                      // M + 1 floats fit the 2 M of the other image (its re and im arrays are adjacent)
  for (int k = tid; k <= M; k += AF_THREADS) {
    const int k0 = k & (M - 1), k1 = (M - k) & (M - 1);
    const float a = zr[k0], bb = zi[k0], c = zr[k1], d = zi[k1];
    const float er = 0.5f * (a + c), ei = 0.5f * (bb - d);
    const float orr = 0.5f * (bb + d), oi = -0.5f * (a - c);
    const float wr = tab.tw_re[k], wi = tab.tw_im[k];
    const float xr = er + (wr * orr - wi * oi);
    const float xi = ei + (wr * oi + wi * orr);
    const float p2 = xr * xr + xi * xi;
    pw[k] = MAGNITUDE ? sqrtf(p2) : p2;
  }
  __syncthreads();
  return pw;
}

// ---- framed power spectrum -> mel power -----------------------------------------------------------------------------------------------------
// dynamic LDS: 4 arrays of M = n_fft / 2 floats (re / im of two images) = 8 * n_fft bytes.
__global__ __launch_bounds__(AF_THREADS) void mel_power_kernel(AudioTables tab, const float *__restrict__ wav, int L, int T,
                                                               float *__restrict__ mel) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int N = tab.n_fft, M = N >> 1;
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  float *sr = lds, *si = lds + M;
  const float *x = wav + (size_t)b * L;
  const int start = t * tab.hop - M;

  // gather: z[n] = w[2n] x[2n] + i w[2n + 1] x[2n + 1]
  for (int n = tid; n < M; n += AF_THREADS) {
    float v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = 2 * n + h;
      int s = start + i;
      float xv = 0.f;
      if (tab.pad_mode == AUDIO_PAD_REFLECT) {
        if (s < 0) s = -s;
        if (s >= L) s = 2 * (L - 1) - s;
        xv = x[s];                      // L > n_fft / 2 (checked by the caller): one reflection always lands inside
      } else if (s >= 0 && s < L) {
        xv = x[s];
      }
      v[h] = xv * tab.window[i];
    }
    sr[n] = v[0];
    si[n] = v[1];
  }
  __syncthreads();

  const float *pw = real_fft_bins<false>(tab, lds, tid);

  for (int m = tid; m < tab.n_mels; m += AF_THREADS) {
    const int first = tab.fb_first[m], cnt = tab.fb_count[m];
    const float *w = tab.fb_weights + tab.fb_offset[m];
    float acc = 0.f;
    for (int i = 0; i < cnt; ++i) acc += w[i] * pw[first + i];
    mel[((size_t)b * tab.n_mels + m) * T + t] = acc;
  }
}

// ---- uncentred frames -> log-mel magnitude examples (the VGGish input of the FAD evaluation) ------------------------------------------------
// One workgroup per (clip, frame): frame t = samples [t hop, t hop + win) times the window, zero-padded at its END to n_fft points, no
// padding of the clip (the caller launches only frames that lie inside it); |X_k|, filterbank, log(mel + offset).  The frame's n_mels
// values go to rows ((b T + t) n_mels + m) of a 4-column channels-last image (column 0 the value, columns 1 .. 3 zero: the layout the
// implicit-GEMM convolution reads with cin_ld = 4) and / or to a plain (B, T, n_mels) magnitude plane.
__global__ __launch_bounds__(AF_THREADS) void framed_logmel_kernel(AudioTables tab, int win, const float *__restrict__ wav, int L, int T,
                                                                   float log_offset, float4 *__restrict__ examples, float *__restrict__ mel) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int M = tab.n_fft >> 1;
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  float *sr = lds, *si = lds + M;
  const float *x = wav + (size_t)b * L + (size_t)t * tab.hop;   // t hop + win <= L for every launched frame

  for (int n = tid; n < M; n += AF_THREADS) {
    const int i = 2 * n;
    sr[n] = i < win ? x[i] * tab.window[i] : 0.f;
    si[n] = i + 1 < win ? x[i + 1] * tab.window[i + 1] : 0.f;
  }
  __syncthreads();

  const float *mag = real_fft_bins<true>(tab, lds, tid);

  for (int m = tid; m < tab.n_mels; m += AF_THREADS) {
    const int first = tab.fb_first[m], cnt = tab.fb_count[m];
    const float *w = tab.fb_weights + tab.fb_offset[m];
    float acc = 0.f;
    for (int i = 0; i < cnt; ++i) acc += w[i] * mag[first + i];
    const size_t row = ((size_t)b * T + t) * tab.n_mels + m;
    if (mel) mel[row] = acc;
    if (examples) examples[row] = make_float4(logf(acc + log_offset), 0.f, 0.f, 0.f);
  }
}

// ---- dB and spectral flux -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float to_db(float p, float amin, float amin_db, float floor_db) {
  const float v = p > amin ? 10.f * log10f(p) : amin_db;
  return fmaxf(v, floor_db);
}

// 256 threads = 64 frame lanes x 4 mel groups; the four partial sums of a frame are added in a fixed order.
__global__ __launch_bounds__(AF_THREADS) void db_flux_kernel(const float *__restrict__ mel, int n_mels, int T, float amin, float amin_db,
                                                             float top_db, int lag, int shift, float *__restrict__ db, float *__restrict__ env) {
  __shared__ float red[AF_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float *P = mel + (size_t)b * n_mels * T;
  const int plane = n_mels * T;
  float mx = 0.f;                      // power is >= 0
  for (int i = tid; i < plane; i += AF_THREADS) mx = fmaxf(mx, P[i]);
  mx = block_reduce<true>(mx, red);
  const float floor_db = (mx > amin ? 10.f * log10f(mx) : amin_db) - top_db;
  __syncthreads();

  if (!env) {
    float *D = db + (size_t)b * plane;
    for (int i = tid; i < plane; i += AF_THREADS) D[i] = to_db(P[i], amin, amin_db, floor_db);
    return;
  }
  float *E = env + (size_t)b * T;
  float *D = db ? db + (size_t)b * plane : nullptr;
  const int off = shift - lag;         // d[t] lands at frame t + off
  for (int i = tid; i < T; i += AF_THREADS)
    if (i < shift) E[i] = 0.f;
  const int lane = tid & 63, grp = tid >> 6;
  const float inv = 1.f / (float)n_mels;
  for (int t0 = 0; t0 < T; t0 += 64) {   // wave-uniform trip count: the barriers below are reached by every thread
    const int t = t0 + lane;
    float acc = 0.f;
    if (t < T) {
      for (int m = grp; m < n_mels; m += 4) {
        const float cur = to_db(P[m * T + t], amin, amin_db, floor_db);
        if (D) D[m * T + t] = cur;
        if (t >= lag) acc += fmaxf(0.f, cur - to_db(P[m * T + t - lag], amin, amin_db, floor_db));
      }
    }
    __syncthreads();
    red[tid] = acc;
    __syncthreads();
    if (grp == 0 && t < T && t >= lag && t + off < T) E[t + off] = ((red[lane] + red[64 + lane]) + (red[128 + lane] + red[192 + lane])) * inv;
  }
}

// ---- peak picking and confidences -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AF_THREADS) void peak_pick_kernel(const float *__restrict__ env, const float *__restrict__ wav, int T, int L, int hop,
                                                               PeakParams p, float *__restrict__ xs, int32_t *__restrict__ flags,
                                                               int32_t *__restrict__ count, int32_t *__restrict__ positions,
                                                               float *__restrict__ confidence, float *__restrict__ strength) {
  __shared__ float red[AF_THREADS];
  __shared__ int n_found;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float *e = env + (size_t)b * T;
  const float *wv = wav + (size_t)b * L;
  float *x = xs + (size_t)b * T;
  int32_t *fl = flags + (size_t)b * T;
  int32_t *pos = positions + (size_t)b * p.capacity;
  float *conf = confidence + (size_t)b * p.capacity, *str = strength + (size_t)b * p.capacity;

  for (int i = tid; i < p.capacity; i += AF_THREADS) {
    pos[i] = -1;
    conf[i] = 0.f;
    str[i] = 0.f;
  }
  float mn = FLT_MAX, mx = -FLT_MAX;
  for (int i = tid; i < T; i += AF_THREADS) {
    mn = fminf(mn, e[i]);
    mx = fmaxf(mx, e[i]);
  }
  mn = block_reduce<false>(mn, red);
  mx = block_reduce<true>(mx, red);
  if (mx == 0.f && mn == 0.f) {        // an all-zero envelope has no onsets (block-uniform exit)
    for (int i = tid; i < T; i += AF_THREADS) {
      x[i] = 0.f;
      fl[i] = 0;
    }
    if (tid == 0) count[b] = 0;
    return;
  }
  const float scale = (mx - mn) + FLT_MIN;
  for (int i = tid; i < T; i += AF_THREADS) x[i] = (e[i] - mn) / scale;
  __syncthreads();
  for (int n = tid; n < T; n += AF_THREADS) {
    const float v = x[n];
    float wmax = v;
    for (int i = max(0, n - p.pre_max), hi = min(T, n + p.post_max); i < hi; ++i) wmax = fmaxf(wmax, x[i]);
    float sum = 0.f;
    const int lo = max(0, n - p.pre_avg), hi = min(T, n + p.post_avg);
    for (int i = lo; i < hi; ++i) sum += x[i];
    const float mean = hi > lo ? sum / (float)(hi - lo) : v;
    fl[n] = (v == wmax && v >= mean + p.delta) ? 1 : 0;
  }
  __syncthreads();
  if (tid == 0) {                      // greedy left-to-right `wait` suppression
    int found = 0;
    long long last = -(1ll << 40);
    for (int n = 0; n < T; ++n)
      if (fl[n] && (long long)n - last > p.wait) {
        if (found < p.capacity) pos[found] = n * hop;
        ++found;
        last = n;
      }
    n_found = found;
    count[b] = found <= p.capacity ? found : -1;
  }
  __syncthreads();
  const int found = min(n_found, p.capacity);

  // w = (|wav| - min |wav|) / (max |wav| - min |wav|); it is monotone in |wav|, so the window maximum is taken on |wav| itself
  float amn = FLT_MAX, amx = 0.f;
  for (int i = tid; i < L; i += AF_THREADS) {
    const float a = fabsf(wv[i]);
    amn = fminf(amn, a);
    amx = fmaxf(amx, a);
  }
  amn = block_reduce<false>(amn, red);
  amx = block_reduce<true>(amx, red);
  const float span = amx - amn;
  for (int k = 0; k < found; ++k) {      // block-uniform trip count
    const int o = pos[k];
    float wm = 0.f;
    for (int i = max(0, o - p.conf_interval) + tid, hi = min(L, o + p.conf_interval); i < hi; i += AF_THREADS) wm = fmaxf(wm, fabsf(wv[i]));
    wm = block_reduce<true>(wm, red);
    if (tid == 0) {
      conf[k] = (wm - amn) / span;
      str[k] = o < L ? (fabsf(wv[o]) - amn) / span : 0.f;
    }
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------
static int64_t round256(int64_t n) { return (n + 255) / 256 * 256; }

int64_t audio_ws_bytes(int n_mels, int hop, int B, int L) {
  const int64_t T = audio_frames(L, hop);
  return round256((int64_t)B * n_mels * T * 4) + 2 * round256((int64_t)B * T * 4);
}

hipError_t launch_mel_power(const AudioTables &tab, const float *wav, int B, int L, float *mel, hipStream_t s) {
  const int T = audio_frames(L, tab.hop);
  if (B > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mel_power_kernel, dim3(T, B), dim3(AF_THREADS), (size_t)8 * tab.n_fft, s, tab, wav, L, T, mel);
  return hipGetLastError();
}

hipError_t launch_framed_logmel(const AudioTables &tab, int win, const float *wav, int B, int L, int T, float log_offset, float *examples,
                                float *mel, hipStream_t s) {
  if (B > 65535 || T < 1 || (int64_t)(T - 1) * tab.hop + win > L) return hipErrorInvalidValue;
  hipLaunchKernelGGL(framed_logmel_kernel, dim3(T, B), dim3(AF_THREADS), (size_t)8 * tab.n_fft, s, tab, win, wav, L, T, log_offset,
                     reinterpret_cast<float4 *>(examples), mel);
  return hipGetLastError();
}

hipError_t launch_db_flux(const float *mel, int B, int n_mels, int T, float amin, float amin_db, float top_db, int lag, int shift, float *db,
                          float *env, hipStream_t s) {
  hipLaunchKernelGGL(db_flux_kernel, dim3(B), dim3(AF_THREADS), 0, s, mel, n_mels, T, amin, amin_db, top_db, lag, shift, db, env);
  return hipGetLastError();
}

hipError_t launch_peak_pick(const float *env, const float *wav, int B, int T, int L, int hop, const PeakParams &p, float *x, int32_t *flags,
                            int32_t *count, int32_t *positions, float *confidence, float *strength, hipStream_t s) {
  hipLaunchKernelGGL(peak_pick_kernel, dim3(B), dim3(AF_THREADS), 0, s, env, wav, T, L, hop, p, x, flags, count, positions, confidence, strength);
  return hipGetLastError();
}

}  // namespace sf
