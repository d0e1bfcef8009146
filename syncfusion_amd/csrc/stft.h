// Complex STFT, inverse STFT with overlap-add and the spectral-gating denoiser built on them (stft.hip; C ABI in capi_stft.cpp).
// All fp32 on the caller's stream, no allocation: scratch comes from a workspace of gate_ws_bytes().  Spectra are stored
// (rows, T, F, 2): F = n_fft / 2 + 1 interleaved complex bins per frame, so the recurrence, the smoothing and the inverse read rows of F.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sf {

enum { STFT_PAD_CONSTANT = 0, STFT_PAD_REFLECT = 1 };

// Device tables of one configuration (owned by the handle in capi_stft.cpp).
struct StftTables {
  int n_fft = 0, win = 0, hop = 0;
  int pad = 0;                       // samples of padding in front of the clip: win / 2 when centred, 0 otherwise
  int pad_mode = 0;
  float fwd_scale = 1.f;             // 1 / sum(w) ("spectrum") or 1
  float inv_scale = 1.f;             // sum(w) or 1
  int n_ftaps = 1, n_ttaps = 1;      // odd lengths of the two smoothing filters
  const float *window = nullptr;     // [n_fft]       periodic Hann of `win` points, zeros behind it
  const float *tw_re = nullptr;      // [n_fft/2 + 1] cos(2 pi k / n_fft)
  const float *tw_im = nullptr;      // [n_fft/2 + 1] -sin(2 pi k / n_fft)
  const float *ftaps = nullptr;      // [n_ftaps] over bins, sum 1
  const float *ttaps = nullptr;      // [n_ttaps] over frames, sum 1
};

// frames of a clip of L samples (0 when the clip is shorter than one window) and samples the inverse returns for T frames
inline int64_t stft_frames(int L, int win, int hop, int pad) { return (int64_t)L + 2 * pad < win ? 0 : ((int64_t)L + 2 * pad - win) / hop + 1; }
inline int64_t istft_samples(int T, int win, int hop, int pad) { return (int64_t)win + (int64_t)(T - 1) * hop - 2 * pad; }
// one bound for every call on (B, L): a real plane (B, T, F), a complex plane (B, T, F, 2), the windowed frames (B, T, win), B floats
int64_t gate_ws_bytes(const StftTables &tab, int B, int L);

// wav (B, L) -> spec (B, T, F, 2)
hipError_t launch_stft(const StftTables &tab, const float *wav, int B, int L, int T, float *spec, hipStream_t s);
// spec (B, T, F, 2) -> out (B, out_len): istft_samples() values per row, zeros (or a cut) up to out_len.  frames: (B, T, win) scratch
hipError_t launch_istft(const StftTables &tab, const float *spec, int B, int T, float *frames, float *out, int out_len, hipStream_t s);
// non-stationary mask: |S| smoothed forward and backward over frames by y = b x + (1 - b) y_prev, mask = sigmoid(((|S| - sm) / sm - mult) slope)
// (0 where sm == 0).  fwd: (B, T, F) scratch
hipError_t launch_ns_mask(const float *spec, int B, int T, int F, float b, float mult, float slope, float *fwd, float *mask, hipStream_t s);
// noise spectra (B, T, F, 2) -> thresh (B, F) = mean_t dB + n_std std_t dB, dB = 20 log10(max(|S|, 1e-20)) floored at the row's maximum - 80
hipError_t launch_noise_thresh(const float *spec, int B, int T, int F, float n_std, float *thresh, hipStream_t s);
// stationary mask: (dB > thresh[row, bin]) as 0 / 1.  rowmax: B floats of scratch
hipError_t launch_stat_mask(const float *spec, int B, int T, int F, const float *thresh, float *rowmax, float *mask, hipStream_t s);
// separable smoothing with zeros outside the plane, prop_decrease (before the filter when prop_first, after it otherwise) and the multiply
// into the spectrum: mask_raw -> mask_smooth (B, T, F), spec_out = spec * mask_smooth.  tmp: (B, T, F) scratch
hipError_t launch_smooth_apply(const StftTables &tab, const float *mask_raw, int B, int T, int F, float prop, int prop_first, const float *spec,
                               float *tmp, float *mask_smooth, float *spec_out, hipStream_t s);

}  // namespace sf
