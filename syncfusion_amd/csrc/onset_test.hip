// The device step of the onset net's TEST stage: what main/module_onset.py:99-125 (test_step) and :142-183 (log_annotations) take from the
// logits of one batch, without the host.  The reference calls the net again for the annotations, copies logits and labels to the host,
// thresholds them in numpy and writes one file per chunk; Lightning averages the logged loss and metrics over the epoch.  Here
//
//   rows   table row r = clip0 + n of clip n:  pred_frames[r, 0 .. pred_count[r]) = the frames t with logits[n, t] > logit_threshold, ascending
//          (:160-162: the RAW logit is thresholded, not the sigmoid; NaN > x is false: a NaN logit is no onset), the rest of the row -1;
//          target_* the same for labels[n, t] != 0 (np.nonzero, :166).  The "remove consecutive onsets" loop of :170-172 compares index
//          VALUES with 1 and never removes anything: it has no counterpart.
//          One wavefront per clip, 64 frames per pass: ballot of the predicate, position = running base + popcount of the lower lanes.
//          Plain vector stores, no atomics; a clip's rows depend on that clip alone.
//   sums   sums += (N loss, N AP, N Acc, N OnsNumAcc, N) in fp64, loss / metrics being what launch_onset_bce_fwd / launch_onset_metrics
//          (onset_loss.hip) give for the batch: ONE thread adds, in that order; NaN and inf propagate.
//
// Nothing is read back: the epoch tables and the sums stay on the device until the stage ends.
//   ws     onset_loss_ws_bytes(N T) (shared by the loss and the metrics launches, which run one after the other) | 64 bytes: 3 doubles
//          (metrics), 1 float (loss), 2 floats (stats)
#include "common.h"

namespace sf {

namespace {

constexpr int OT_THREADS = 256;
constexpr int OT_WAVES = OT_THREADS / WAVE;
constexpr int64_t OT_TAIL = 64;

__global__ __launch_bounds__(OT_THREADS) void onset_test_rows_kernel(const float *__restrict__ logits, const float *__restrict__ labels, int N, int T,
                                                                     float thr, int64_t clip0, int32_t *__restrict__ pred_count,
                                                                     int32_t *__restrict__ pred_frames, int32_t *__restrict__ target_count,
                                                                     int32_t *__restrict__ target_frames) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int n = (int)blockIdx.x * OT_WAVES + (int)(threadIdx.x / WAVE);   // the same on every lane of a wave
  if (n >= N) return;
  const float *z = logits + (size_t)n * T, *lab = labels + (size_t)n * T;
  const size_t r = (size_t)(clip0 + n);
  int32_t *pf = pred_frames + r * (size_t)T, *tf = target_frames + r * (size_t)T;
  const unsigned long long below = (1ull << lane) - 1ull;
  int np = 0, nt = 0;   // onsets of the passes before: positions stay below the running count, which never exceeds T
  for (int base = 0; base < T; base += WAVE) {
    const int t = base + lane;
    bool p = false, q = false;
    if (t < T) {
      p = z[t] > thr;
      q = lab[t] != 0.f;
    }
    const unsigned long long mp = __ballot(p), mq = __ballot(q);
    if (p) pf[np + __popcll(mp & below)] = t;
    if (q) tf[nt + __popcll(mq & below)] = t;
    np += __popcll(mp);
    nt += __popcll(mq);
  }
  for (int k = np + lane; k < T; k += WAVE) pf[k] = -1;
  for (int k = nt + lane; k < T; k += WAVE) tf[k] = -1;
  if (lane == 0) {
    pred_count[r] = np;
    target_count[r] = nt;
  }
}

__global__ void onset_test_sums_kernel(const float *__restrict__ loss, const double *__restrict__ metrics, int N, double *__restrict__ sums) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const double n = (double)N;
  sums[0] += n * (double)*loss;
  sums[1] += n * metrics[0];
  sums[2] += n * metrics[1];
  sums[3] += n * metrics[2];
  sums[4] += n;
}

}  // namespace

int64_t onset_test_ws_bytes(int N, int T) { return onset_loss_ws_bytes((int64_t)N * T) + OT_TAIL; }

hipError_t launch_onset_test_step(const float *logits, const float *labels, int N, int T, float logit_threshold, float metric_threshold,
                                  int64_t clip0, int32_t *pred_count, int32_t *pred_frames, int32_t *target_count, int32_t *target_frames,
                                  double *sums, void *ws, hipStream_t s) {
  if (!logits || !labels || !pred_count || !pred_frames || !target_count || !target_frames || !sums || !ws || N < 1 || T < 1 || clip0 < 0 ||
      (int64_t)N * T > ONSET_METRICS_MAX)
    return hipErrorInvalidValue;
  const int64_t n = (int64_t)N * T;
  char *tail = static_cast<char *>(ws) + onset_loss_ws_bytes(n);   // a multiple of 256 behind an 8-byte aligned base
  double *metrics = reinterpret_cast<double *>(tail);
  float *loss = reinterpret_cast<float *>(tail + 3 * sizeof(double)), *stats = loss + 1;
  hipLaunchKernelGGL(onset_test_rows_kernel, dim3((unsigned)((N + OT_WAVES - 1) / OT_WAVES)), dim3(OT_THREADS), 0, s, logits, labels, N, T,
                     logit_threshold, clip0, pred_count, pred_frames, target_count, target_frames);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_onset_bce_fwd(logits, labels, n, loss, stats, ws, s);
  if (e != hipSuccess) return e;
  e = launch_onset_metrics(logits, labels, N, T, metric_threshold, metrics, ws, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(onset_test_sums_kernel, dim3(1), dim3(WAVE), 0, s, loss, metrics, N, sums);
  return hipGetLastError();
}

}  // namespace sf
