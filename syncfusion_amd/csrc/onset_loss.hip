// The end of the onset net's training step on the device (main/module_onset.py:268-354, BCLoss): the class-balanced BCE-with-logits loss, its
// gradient, and the three step metrics (AP, Acc, OnsNumAcc) of BCLoss.evaluate -- nothing is read back, nothing that changes per step is a
// kernel argument, so the calls sit inside a captured graph.  The inputs are tiny (16 x 30 logits in the reference's configuration): what
// counts is the launch count and a fixed order of every reduction (no floating-point atomics: the same input gives the same bits).
//
//   loss     pw = (n - sum t) / sum t;  loss = mean(pw t softplus(-z) + (1 - t) softplus(z)) = (pw A + B) / n with A = sum t softplus(-z),
//            B = sum (1 - t) softplus(z): ONE pass gives sum t, A and B, so pw never has to exist before the pass.  One workgroup per
//            OL_CHUNK elements; a single workgroup finishes at once, more write (sum t, A, B) partials that a second launch adds in index order.
//            Sums are carried in fp64.  sum t = 0 gives pw = inf and loss = inf * 0 = NaN, as the reference's BCEWithLogitsLoss does.
//   dz       g / n ((1 - t) sigmoid(z) - pw t (1 - sigmoid(z))), both sigmoid tails from exp(-|z|) (no cancellation); g is read from the device.
//   metrics  scores s = fp32 sigmoid(z); balanced subset = the first b = min(#(t == 1), #(t == 0)) positives and negatives in row-major order;
//            AP = 1/b sum_{positives i} TP(s >= s_i) / CNT(s >= s_i) over the subset (sklearn's step-wise AP with tied scores as one threshold,
//            in integer counts: exact and order-independent); Acc = share of the subset with (s > thr) == t; OnsNumAcc = share of rows whose
//            thresholded predictions, after the reference's left-to-right removal of the later frame of every adjacent pair (a run of L ones
//            keeps ceil(L / 2)), count as many onsets as the row's labels.  b = 0: AP = Acc = NaN (0 / 0 in fp64).
//            Three phases: prep (ONE workgroup: class totals, ordered compaction of the subset's scores by ballot prefix, Acc and OnsNumAcc
//            counts), count (one thread per subset positive, the subset streamed through LDS tiles), final (terms added in a fixed order in fp64).
//            Up to OL_SMALL elements one workgroup runs the three phases in one launch; above, three launches (count on a grid: O(b^2) compares).
//   ws       loss: 3 doubles per workgroup.  metrics: 16 int32 (b, Acc count, row count) | n / 2 + 1 doubles (AP terms) | n floats (subset scores)
#include "common.h"

namespace sf {

namespace {

constexpr int OL_THREADS = 256;
constexpr int OL_WAVES = OL_THREADS / WAVE;
constexpr int OL_CHUNK = 4096;   // loss: elements per workgroup
constexpr int OL_SMALL = 4096;   // metrics: largest N * T that one workgroup takes in one launch
constexpr int OL_TILE = 1024;    // metrics: subset scores per LDS tile

__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum over the workgroup, the same value on every thread: 64-lane butterfly, then the four waves pairwise through LDS (fixed order)
__device__ __forceinline__ double block_sum_d(double v, double *red) {
  v = wave_sum_d(v);
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  const double r = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ int block_sum_i(int v, int *red) {
  v = wave_sum_i(v);
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  const int r = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return r;
}

// ---- loss ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void bce_finish(double st, double a, double b, int64_t n, float *loss, float *stats) {
  const double pw = ((double)n - st) / st;   // st == 0: +inf (n >= 1), and inf * (a == 0) below is NaN: the reference's result
  stats[0] = (float)st;
  stats[1] = (float)pw;
  *loss = (float)((pw * a + b) / (double)n);
}

__global__ __launch_bounds__(OL_THREADS) void onset_bce_fwd_kernel(const float *__restrict__ z, const float *__restrict__ t, int64_t n,
                                                                   double *__restrict__ partial, float *__restrict__ loss,
                                                                   float *__restrict__ stats) {
  __shared__ double red[OL_WAVES];
  const int64_t base = (int64_t)blockIdx.x * OL_CHUNK;
  double st = 0.0, a = 0.0, b = 0.0;
  for (int k = threadIdx.x; k < OL_CHUNK; k += OL_THREADS) {
    const int64_t i = base + k;
    if (i >= n) break;
    const float zi = z[i], ti = t[i];
    st += (double)ti;
    a += (double)(ti * softplus_f(-zi));
    b += (double)((1.f - ti) * softplus_f(zi));
  }
  st = block_sum_d(st, red);
  a = block_sum_d(a, red);
  b = block_sum_d(b, red);
  if (threadIdx.x != 0) return;
  if (gridDim.x == 1) {
    bce_finish(st, a, b, n, loss, stats);
  } else {
    partial[3 * (size_t)blockIdx.x] = st;
    partial[3 * (size_t)blockIdx.x + 1] = a;
    partial[3 * (size_t)blockIdx.x + 2] = b;
  }
}

__global__ __launch_bounds__(OL_THREADS) void onset_bce_final_kernel(const double *__restrict__ partial, int blocks, int64_t n,
                                                                     float *__restrict__ loss, float *__restrict__ stats) {
  __shared__ double red[OL_WAVES];
  double st = 0.0, a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < blocks; i += OL_THREADS) {
    st += partial[3 * (size_t)i];
    a += partial[3 * (size_t)i + 1];
    b += partial[3 * (size_t)i + 2];
  }
  st = block_sum_d(st, red);
  a = block_sum_d(a, red);
  b = block_sum_d(b, red);
  if (threadIdx.x == 0) bce_finish(st, a, b, n, loss, stats);
}

__global__ __launch_bounds__(OL_THREADS) void onset_bce_bwd_kernel(const float *__restrict__ z, const float *__restrict__ t,
                                                                   const float *__restrict__ stats, const float *__restrict__ g, int64_t n,
                                                                   float *__restrict__ dz) {
  const int64_t i = (int64_t)blockIdx.x * OL_THREADS + threadIdx.x;
  if (i >= n) return;
  const float pw = stats[1];
  const float c = (float)((double)*g / (double)n);
  const float zi = z[i], ti = t[i];
  const float e = expf(-fabsf(zi)), r = 1.0f / (1.0f + e);
  const float big = r, small = e * r;                      // sigmoid(|z|), sigmoid(-|z|)
  const float sig = zi >= 0.f ? big : small, oms = zi >= 0.f ? small : big;
  dz[i] = c * ((1.f - ti) * sig - pw * ti * oms);
}

// ---- metrics ------------------------------------------------------------------------------------------------------------------------------
struct MetricsHead {
  int b, correct, match;   // subset half size; subset elements with (s > thr) == t; rows whose onset count equals their label count
};

// ONE workgroup.  sub[0, b) <- the scores of the first b positives, sub[b, 2 b) <- of the first b negatives, both in row-major order.
__device__ MetricsHead metrics_prep(const float *__restrict__ z, const float *__restrict__ t, int N, int T, float thr, float *sub,
                                    int *redi /* LDS, 2 * OL_WAVES */) {
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int n = N * T;
  int p = 0, q = 0;
  for (int i = tid; i < n; i += OL_THREADS) {
    const float ti = t[i];
    p += ti == 1.f;
    q += ti == 0.f;
  }
  p = block_sum_i(p, redi);
  q = block_sum_i(q, redi);
  MetricsHead h;
  h.b = p < q ? p : q;   // 2 b <= p + q <= n: every index below stays inside sub's n floats
  // ordered compaction, OL_THREADS elements per round: rank inside the class = elements of the rounds before + of the waves before + of the
  // lanes before (ballot).  Every quantity that steers the loop is the same on all threads.
  int run_p = 0, run_q = 0, correct = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int base = 0; base < n && (run_p < h.b || run_q < h.b); base += OL_THREADS) {
    const int i = base + tid;
    bool is_p = false, is_q = false;
    float s = 0.f;
    if (i < n) {
      const float ti = t[i];
      is_p = ti == 1.f;
      is_q = ti == 0.f;
      s = sigmoid_f(z[i]);
    }
    const unsigned long long mp = __ballot(is_p), mq = __ballot(is_q);
    if (lane == 0) {
      redi[wave] = __popcll(mp);
      redi[OL_WAVES + wave] = __popcll(mq);
    }
    __syncthreads();
    int off_p = run_p, off_q = run_q;
    for (int w = 0; w < OL_WAVES; ++w) {
      const int cp = redi[w], cq = redi[OL_WAVES + w];
      if (w < wave) {
        off_p += cp;
        off_q += cq;
      }
      run_p += cp;
      run_q += cq;
    }
    __syncthreads();
    const int rp = off_p + __popcll(mp & below), rq = off_q + __popcll(mq & below);
    if (is_p && rp < h.b) {
      sub[rp] = s;
      correct += s > thr;
    }
    if (is_q && rq < h.b) {
      sub[h.b + rq] = s;
      correct += !(s > thr);
    }
  }
  h.correct = block_sum_i(correct, redi);
  // OnsNumAcc, one wave per row: a lane that sits on the first frame of a run of predictions walks the run (it ends at the row's end at the
  // latest) and keeps ceil(L / 2) of it
  int match = 0;
  for (int r = wave; r < N; r += OL_WAVES) {
    const float *zr = z + (size_t)r * T, *tr = t + (size_t)r * T;
    int kept = 0, lab = 0;
    for (int j = lane; j < T; j += WAVE) {
      lab += (int)tr[j];
      if (sigmoid_f(zr[j]) > thr && (j == 0 || !(sigmoid_f(zr[j - 1]) > thr))) {
        int L = 1;
        while (j + L < T && sigmoid_f(zr[j + L]) > thr) ++L;
        kept += (L + 1) >> 1;
      }
    }
    kept = wave_sum_i(kept);
    lab = wave_sum_i(lab);
    match += kept == lab;
  }
  if (lane == 0) redi[wave] = match;
  __syncthreads();
  h.match = (redi[0] + redi[1]) + (redi[2] + redi[3]);
  __syncthreads();
  return h;
}

// terms[i] = TP / CNT of the subset's positive i = i0 + threadIdx.x; the whole workgroup walks the subset in LDS tiles (i0 and b are uniform)
__device__ void metrics_count(const float *sub, int b, int i0, double *terms, float *tile /* LDS, OL_TILE */) {
  const int tid = threadIdx.x, i = i0 + tid;
  const float si = i < b ? sub[i] : 0.f;
  int tp = 0, fp = 0;
  for (int base = 0; base < 2 * b; base += OL_TILE) {
    const int len = 2 * b - base < OL_TILE ? 2 * b - base : OL_TILE;
    __syncthreads();
    for (int k = tid; k < len; k += OL_THREADS) tile[k] = sub[base + k];
    __syncthreads();
    int np = b - base;   // the tile's entries in front of np are positives
    np = np < 0 ? 0 : (np > len ? len : np);
    for (int k = 0; k < np; ++k) tp += tile[k] >= si;
    for (int k = np; k < len; ++k) fp += tile[k] >= si;
  }
  if (i < b) terms[i] = (double)tp / (double)(tp + fp);
}

// ONE workgroup: out = [AP, Acc, OnsNumAcc]
__device__ void metrics_final(const MetricsHead h, const double *terms, int N, double *__restrict__ out, double *redd /* LDS, OL_WAVES */) {
  double s = 0.0;
  for (int i = threadIdx.x; i < h.b; i += OL_THREADS) s += terms[i];
  s = block_sum_d(s, redd);
  if (threadIdx.x == 0) {
    out[0] = s / (double)h.b;
    out[1] = (double)h.correct / (double)(2 * h.b);
    out[2] = (double)h.match / (double)N;
  }
}

__global__ __launch_bounds__(OL_THREADS) void onset_metrics_small_kernel(const float *__restrict__ z, const float *__restrict__ t, int N, int T, float thr,
                                                                         float *sub, double *terms, double *__restrict__ out) {
  __shared__ int redi[2 * OL_WAVES];
  __shared__ double redd[OL_WAVES];
  __shared__ float tile[OL_TILE];
  const MetricsHead h = metrics_prep(z, t, N, T, thr, sub, redi);
  __syncthreads();   // sub is written and read by this workgroup only
  for (int i0 = 0; i0 < h.b; i0 += OL_THREADS) metrics_count(sub, h.b, i0, terms, tile);
  __syncthreads();
  metrics_final(h, terms, N, out, redd);
}

__global__ __launch_bounds__(OL_THREADS) void onset_metrics_prep_kernel(const float *__restrict__ z, const float *__restrict__ t, int N, int T, float thr,
                                                                        float *__restrict__ sub, int *__restrict__ head) {
  __shared__ int redi[2 * OL_WAVES];
  const MetricsHead h = metrics_prep(z, t, N, T, thr, sub, redi);
  if (threadIdx.x == 0) {
    head[0] = h.b;
    head[1] = h.correct;
    head[2] = h.match;
  }
}

__global__ __launch_bounds__(OL_THREADS) void onset_metrics_count_kernel(const float *__restrict__ sub, const int *__restrict__ head,
                                                                         double *__restrict__ terms) {
  __shared__ float tile[OL_TILE];
  const int b = head[0], i0 = (int)blockIdx.x * OL_THREADS;
  if (i0 >= b) return;   // the grid covers n / 2 positives, the batch holds b of them
  metrics_count(sub, b, i0, terms, tile);
}

__global__ __launch_bounds__(OL_THREADS) void onset_metrics_final_kernel(const int *__restrict__ head, const double *__restrict__ terms, int N,
                                                                         double *__restrict__ out) {
  __shared__ double redd[OL_WAVES];
  MetricsHead h;
  h.b = head[0];
  h.correct = head[1];
  h.match = head[2];
  metrics_final(h, terms, N, out, redd);
}

int64_t loss_blocks(int64_t n) { return (n + OL_CHUNK - 1) / OL_CHUNK; }

}  // namespace

int64_t onset_loss_ws_bytes(int64_t n) {
  const int64_t loss = 3 * (int64_t)sizeof(double) * loss_blocks(n);
  const int64_t metrics = 64 + (int64_t)sizeof(double) * (n / 2 + 1) + (int64_t)sizeof(float) * n;
  return ((loss > metrics ? loss : metrics) + 255) / 256 * 256;
}

hipError_t launch_onset_bce_fwd(const float *z, const float *t, int64_t n, float *loss, float *stats, void *ws, hipStream_t s) {
  if (!z || !t || !loss || !stats || !ws || n < 1) return hipErrorInvalidValue;
  const int64_t blocks = loss_blocks(n);
  double *partial = static_cast<double *>(ws);
  hipLaunchKernelGGL(onset_bce_fwd_kernel, dim3((unsigned)blocks), dim3(OL_THREADS), 0, s, z, t, n, partial, loss, stats);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || blocks == 1) return e;
  hipLaunchKernelGGL(onset_bce_final_kernel, dim3(1), dim3(OL_THREADS), 0, s, partial, (int)blocks, n, loss, stats);
  return hipGetLastError();
}

hipError_t launch_onset_bce_bwd(const float *z, const float *t, const float *stats, const float *g, int64_t n, float *dz, hipStream_t s) {
  if (!z || !t || !stats || !g || !dz || n < 1) return hipErrorInvalidValue;
  const int64_t blocks = (n + OL_THREADS - 1) / OL_THREADS;
  hipLaunchKernelGGL(onset_bce_bwd_kernel, dim3((unsigned)blocks), dim3(OL_THREADS), 0, s, z, t, stats, g, n, dz);
  return hipGetLastError();
}

hipError_t launch_onset_metrics(const float *z, const float *t, int N, int T, float threshold, double *out, void *ws, hipStream_t s) {
  if (!z || !t || !out || !ws || N < 1 || T < 1 || (int64_t)N * T > ONSET_METRICS_MAX) return hipErrorInvalidValue;
  const int n = N * T;
  int *head = static_cast<int *>(ws);
  double *terms = reinterpret_cast<double *>(static_cast<char *>(ws) + 64);
  float *sub = reinterpret_cast<float *>(terms + (n / 2 + 1));
  if (n <= OL_SMALL) {
    hipLaunchKernelGGL(onset_metrics_small_kernel, dim3(1), dim3(OL_THREADS), 0, s, z, t, N, T, threshold, sub, terms, out);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(onset_metrics_prep_kernel, dim3(1), dim3(OL_THREADS), 0, s, z, t, N, T, threshold, sub, head);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(onset_metrics_count_kernel, dim3((unsigned)((n / 2 + OL_THREADS - 1) / OL_THREADS)), dim3(OL_THREADS), 0, s, sub, head, terms);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(onset_metrics_final_kernel, dim3(1), dim3(OL_THREADS), 0, s, head, terms, N, out);
  return hipGetLastError();
}

}  // namespace sf
