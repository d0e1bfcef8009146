// Audio front end of the onset-sync evaluation (audio_features.hip): log-mel spectrogram, spectral-flux onset envelope, peak picking.
// Shared by the kernels and their C ABI (capi_audio.cpp).  All fp32, on the caller's stream, no allocation: scratch comes from a
// workspace of audio_ws_bytes().
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sf {

enum { AUDIO_PAD_CONSTANT = 0, AUDIO_PAD_REFLECT = 1, AUDIO_PAD_NONE = 2 /* uncentred frames: launch_framed_logmel only */ };

// Device tables of one front-end configuration (owned by the handle in capi_audio.cpp).
struct AudioTables {
  int n_fft = 0, hop = 0, n_mels = 0, pad_mode = 0;
  const float *window = nullptr;     // [n_fft]       periodic Hann
  const float *tw_re = nullptr;      // [n_fft/2 + 1] cos(2 pi k / n_fft)
  const float *tw_im = nullptr;      // [n_fft/2 + 1] -sin(2 pi k / n_fft)
  const int32_t *fb_first = nullptr; // [n_mels] first bin of the filter
  const int32_t *fb_count = nullptr; // [n_mels] bins it touches
  const int32_t *fb_offset = nullptr;// [n_mels] start of its weights in fb_weights
  const float *fb_weights = nullptr; // packed
};

struct PeakParams {
  int lag, shift;                    // envelope: d[t] lands at frame t + shift - lag
  int pre_max, post_max, pre_avg, post_avg, wait;
  float delta;
  int conf_interval, capacity;
};

inline int audio_frames(int L, int hop) { return 1 + L / hop; }
// mel-power plane (B, n_mels, T) + normalised envelope (B, T) + peak flags (B, T), each rounded up to 256 bytes
int64_t audio_ws_bytes(int n_mels, int hop, int B, int L);

// wav (B, L) -> mel power (B, n_mels, T): one workgroup per (clip, frame), real FFT in LDS
hipError_t launch_mel_power(const AudioTables &tab, const float *wav, int B, int L, float *mel, hipStream_t s);
// uncentred frames of `win` samples (the table's window holds zeros from `win` on) -> log(mel magnitude + log_offset) as 4-column example
// rows ((b T + t) n_mels + m) and / or the (B, T, n_mels) magnitude plane (either may be null); T frames per clip, all inside the clip
hipError_t launch_framed_logmel(const AudioTables &tab, int win, const float *wav, int B, int L, int T, float log_offset, float *examples,
                                float *mel, hipStream_t s);
// mel power -> dB plane (optional) and onset envelope (optional): one workgroup per clip
hipError_t launch_db_flux(const float *mel, int B, int n_mels, int T, float amin, float amin_db, float top_db, int lag, int shift, float *db,
                          float *env, hipStream_t s);
// envelope + waveform -> onsets: one workgroup per clip.  x / flags: (B, T) scratch.
hipError_t launch_peak_pick(const float *env, const float *wav, int B, int T, int L, int hop, const PeakParams &p, float *x, int32_t *flags,
                            int32_t *count, int32_t *positions, float *confidence, float *strength, hipStream_t s);

}  // namespace sf
