// VideoOnsetNet training: the op-level C-ABI entry points behind syncfusion_amd/onset_training.py (fp32; the reference trains the onset net in
// fp32: cfg/trainer/trainer-onset*.yaml sets no precision).  Kernels: onset_train.hip, plus the implicit-GEMM forward (launch_conv_gemm, geom 1);
// onset_loss.hip for the loss and the step metrics behind syncfusion_amd/onset_loss.py; onset_test.hip for the test stage (onset_test.py).
#include <algorithm>
#include <exception>

#include "engine_common.h"

using namespace sf;

namespace {

struct VConv {
  VConvGeom g;
  int64_t NT = 0;
  int cin_ld = 0, cout_ld = 0;
};

VConv check_desc(const sf_vconv_desc *d) {
  if (!d) fail(SF_ERR_INVALID, "null descriptor");
  VConv c;
  VConvGeom &g = c.g;
  g.cin = d->cin;
  g.cout = d->cout;
  g.T = d->T;
  g.Hi = d->Hi;
  g.Wi = d->Wi;
  g.kt = d->kt;
  g.kh = d->kh;
  g.kw = d->kw;
  g.sh = d->sh;
  g.sw = d->sw;
  g.pt = d->pt;
  g.ph = d->ph;
  g.pw = d->pw;
  c.cin_ld = d->cin_ld;
  c.cout_ld = d->cout_ld;
  if (d->N < 1 || g.T < 1 || g.Hi < 1 || g.Wi < 1 || g.cin < 1 || g.cout < 1) fail(SF_ERR_INVALID, "N, T, Hi, Wi, cin and cout must be positive");
  if (c.cin_ld < g.cin || c.cin_ld % 4 || c.cout_ld < g.cout || c.cout_ld % 8) fail(SF_ERR_INVALID, "cin_ld >= cin, cin_ld %% 4 == 0, cout_ld >= cout, cout_ld %% 8 == 0");
  if (g.kt < 1 || g.kh < 1 || g.kw < 1 || g.sh < 1 || g.sw < 1 || g.pt < 0 || g.ph < 0 || g.pw < 0) fail(SF_ERR_INVALID, "bad kernel / stride / padding");
  if (2 * g.pt != g.kt - 1) fail(SF_ERR_UNSUPPORTED, "temporal stride 1 with 'same' padding only (2 pt == kt - 1)");
  g.Ho = (g.Hi + 2 * g.ph - g.kh) / g.sh + 1;
  g.Wo = (g.Wi + 2 * g.pw - g.kw) / g.sw + 1;
  if (g.Hi + 2 * g.ph < g.kh || g.Wi + 2 * g.pw < g.kw) fail(SF_ERR_SHAPE, "frame smaller than the kernel");
  c.NT = (int64_t)d->N * g.T;
  if (c.NT * g.Hi * g.Wi > INT32_MAX || c.NT * g.Ho * g.Wo > INT32_MAX) fail(SF_ERR_SHAPE, "too many rows");
  return c;
}

bool dgrad_s1(const VConvGeom &g) { return g.sh == 1 && g.sw == 1 && 2 * g.ph == g.kh - 1 && 2 * g.pw == g.kw - 1; }

int64_t ws_floats(const VConv &c) {
  const VConvGeom &g = c.g;
  const int64_t fwd = (int64_t)g.cout * vconv_k(g.taps(), c.cin_ld);                           // packed forward weights
  const int64_t dg = dgrad_s1(g) ? (int64_t)g.cin * vconv_k(g.taps(), c.cout_ld) : (int64_t)g.taps() * c.cout_ld * c.cin_ld;
  const int64_t wg = (int64_t)vwgrad_splits(c.NT * g.Ho * g.Wo, g, c.cin_ld) * g.cout * g.taps() * c.cin_ld;
  return std::max({fwd, dg, wg}) + 64;
}

}  // namespace

extern "C" {

int64_t sf_op_vconv_workspace_bytes(const sf_vconv_desc *desc) {
  try {
    return ws_floats(check_desc(desc)) * (int64_t)sizeof(float);
  } catch (const EngineError &) {
    return -1;
  }
}

int sf_op_vconv_fwd(const sf_vconv_desc *desc, const float *x, const float *w, float *y, void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  const VConv c = check_desc(desc);
  if (!x || !w || !y || !ws) fail(SF_ERR_INVALID, "null argument");
  if (ws_bytes < ws_floats(c) * 4) fail(SF_ERR_WORKSPACE, "workspace too small: need %lld bytes", (long long)(ws_floats(c) * 4));
  hipStream_t s = static_cast<hipStream_t>(stream);
  float *wpk = static_cast<float *>(ws);
  SF_HIP(launch_vconv_pack_fwd(w, c.g, c.cin_ld, wpk, s));
  SF_HIP(launch_vconv_fwd(x, c.cin_ld, wpk, c.g, c.NT, y, c.cout_ld, s));
  return SF_OK;
  SF_API_END
}

int sf_op_vconv_bwd(const sf_vconv_desc *desc, const float *x, const float *w, const float *dy, float *dx, float *dw, void *ws, int64_t ws_bytes,
                    void *stream) {
  SF_API_BEGIN
  const VConv c = check_desc(desc);
  if (!dy || !ws || (dx && !w) || (dw && !x)) fail(SF_ERR_INVALID, "null argument");
  if (!dx && !dw) fail(SF_ERR_INVALID, "nothing to compute: dx and dw are both null");
  if (ws_bytes < ws_floats(c) * 4) fail(SF_ERR_WORKSPACE, "workspace too small: need %lld bytes", (long long)(ws_floats(c) * 4));
  hipStream_t s = static_cast<hipStream_t>(stream);
  float *wsf = static_cast<float *>(ws);
  if (dx) {
    if (dgrad_s1(c.g)) SF_HIP(launch_vconv_dgrad_s1(dy, c.cout_ld, w, c.g, c.NT, wsf, dx, c.cin_ld, s));
    else if (c.g.kt == 1) SF_HIP(launch_vconv_dgrad_gather(dy, c.cout_ld, w, c.g, c.NT, wsf, dx, c.cin_ld, s));
    else fail(SF_ERR_UNSUPPORTED, "data gradient: stride-1 'same' convolutions or (1, kh, kw) kernels only");
  }
  if (dw) {
    const int S = vwgrad_splits(c.NT * c.g.Ho * c.g.Wo, c.g, c.cin_ld);
    SF_HIP(launch_vconv_wgrad(dy, c.cout_ld, x, c.cin_ld, c.g, c.NT, wsf, S, dw, s));
  }
  return SF_OK;
  SF_API_END
}

int64_t sf_op_bn_train_workspace_bytes(int64_t rows, int C) {
  if (rows < 2 || C < 1) return -1;
  return ((int64_t)2 * bn_train_slices(rows, C) * C + 3 * (int64_t)C) * (int64_t)sizeof(float);
}

int sf_op_bn_train_fwd(const float *x, const float *res, int64_t rows, int C, int ld, const float *gamma, const float *beta, float eps, float momentum,
                       float *running_mean, float *running_var, int64_t *num_batches_tracked, int relu, float *y, float *save_mean, float *save_invstd,
                       void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!x || !gamma || !beta || !y || !save_mean || !save_invstd || !ws) fail(SF_ERR_INVALID, "null argument");
  if (rows < 2 || C < 1 || ld < C || ld % 4) fail(SF_ERR_INVALID, "rows >= 2, C >= 1, ld >= C and ld %% 4 == 0 required");
  const int64_t need = sf_op_bn_train_workspace_bytes(rows, C);
  if (ws_bytes < need) fail(SF_ERR_WORKSPACE, "workspace too small: need %lld bytes", (long long)need);
  SF_HIP(launch_bn_train_fwd(x, res, ld, C, rows, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, relu, y, save_mean,
                             save_invstd, static_cast<float *>(ws), static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_bn_train_bwd(const float *x, const float *y, const float *dy, int64_t rows, int C, int ld, const float *gamma, const float *save_mean,
                       const float *save_invstd, float *dx, float *dres, float *dgamma, float *dbeta, void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!x || !dy || !gamma || !save_mean || !save_invstd || !ws) fail(SF_ERR_INVALID, "null argument");
  if (rows < 2 || C < 1 || ld < C || ld % 4) fail(SF_ERR_INVALID, "rows >= 2, C >= 1, ld >= C and ld %% 4 == 0 required");
  const int64_t need = sf_op_bn_train_workspace_bytes(rows, C);
  if (ws_bytes < need) fail(SF_ERR_WORKSPACE, "workspace too small: need %lld bytes", (long long)need);
  SF_HIP(launch_bn_train_bwd(x, y, dy, ld, C, rows, gamma, save_mean, save_invstd, dx, dres, dgamma, dbeta, static_cast<float *>(ws),
                             static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int64_t sf_op_bn_sync_workspace_bytes(int64_t rows, int C) {
  if (rows < 1 || C < 1) return -1;
  return ((int64_t)2 * bn_train_slices(rows, C) * C + 3 * (int64_t)C) * (int64_t)sizeof(float);
}

namespace {
// the argument checks shared by the four split-phase entry points (a rank may hold a single row; the caller keeps the TOTAL at 2 or more)
void check_bn_sync(int64_t rows, int C, int ld, const void *ws, int64_t ws_bytes) {
  if (rows < 1 || C < 1 || ld < C || ld % 4) fail(SF_ERR_INVALID, "rows >= 1, C >= 1, ld >= C and ld %% 4 == 0 required");
  if (!ws) fail(SF_ERR_INVALID, "null argument");
  const int64_t need = sf_op_bn_sync_workspace_bytes(rows, C);
  if (ws_bytes < need) fail(SF_ERR_WORKSPACE, "workspace too small: need %lld bytes", (long long)need);
}
}  // namespace

int sf_op_bn_sync_stats(const float *x, int64_t rows, int C, int ld, float *local_stats, void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!x || !local_stats) fail(SF_ERR_INVALID, "null argument");
  check_bn_sync(rows, C, ld, ws, ws_bytes);
  SF_HIP(launch_bn_sync_stats(x, ld, C, rows, local_stats, static_cast<float *>(ws), static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_bn_sync_fwd_apply(const float *x, const float *res, int64_t rows, int C, int ld, const float *gathered_stats, const int64_t *row_counts, int world,
                            const float *gamma, const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                            int64_t *num_batches_tracked, int relu, float *y, float *save_mean, float *save_invstd, void *ws, int64_t ws_bytes,
                            void *stream) {
  SF_API_BEGIN
  if (!x || !gathered_stats || !row_counts || !gamma || !beta || !y || !save_mean || !save_invstd) fail(SF_ERR_INVALID, "null argument");
  if (world < 1) fail(SF_ERR_INVALID, "world >= 1 required");
  check_bn_sync(rows, C, ld, ws, ws_bytes);
  SF_HIP(launch_bn_sync_fwd_apply(x, res, ld, C, rows, gathered_stats, row_counts, world, gamma, beta, eps, momentum, running_mean, running_var,
                                  num_batches_tracked, relu, y, save_mean, save_invstd, static_cast<float *>(ws), static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_bn_sync_bwd_sums(const float *x, const float *y, const float *dy, int64_t rows, int C, int ld, const float *save_mean, const float *save_invstd,
                           float *local_sums, float *dgamma, float *dbeta, void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!x || !dy || !save_mean || !save_invstd || !local_sums) fail(SF_ERR_INVALID, "null argument");
  check_bn_sync(rows, C, ld, ws, ws_bytes);
  SF_HIP(launch_bn_sync_bwd_sums(x, y, dy, ld, C, rows, save_mean, save_invstd, local_sums, dgamma, dbeta, static_cast<float *>(ws),
                                 static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_bn_sync_bwd_apply(const float *x, const float *y, const float *dy, int64_t rows, int C, int ld, const float *gathered_sums,
                            const int64_t *row_counts, int world, const float *gamma, const float *save_mean, const float *save_invstd, float *dx,
                            float *dres, void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!x || !dy || !gathered_sums || !row_counts || !gamma || !save_mean || !save_invstd) fail(SF_ERR_INVALID, "null argument");
  if (world < 1) fail(SF_ERR_INVALID, "world >= 1 required");
  if (!dx && !dres) fail(SF_ERR_INVALID, "nothing to compute: dx and dres are both null");
  check_bn_sync(rows, C, ld, ws, ws_bytes);
  SF_HIP(launch_bn_sync_bwd_apply(x, y, dy, ld, C, rows, gathered_sums, row_counts, world, gamma, save_mean, save_invstd, dx, dres,
                                  static_cast<float *>(ws), static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_video_to_cl(const float *x, int N, int C, int T, int H, int W, int ld, float *out, void *stream) {
  SF_API_BEGIN
  if (!x || !out) fail(SF_ERR_INVALID, "null argument");
  if (N < 1 || C < 1 || T < 1 || H < 1 || W < 1 || ld < C) fail(SF_ERR_INVALID, "bad shape");
  SF_HIP(launch_video_to_cl(F32, x, N, C, T, H, W, out, ld, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_video_pool(const float *x, int64_t NT, int HW, int C, int ld, float *out, void *stream) {
  SF_API_BEGIN
  if (!x || !out) fail(SF_ERR_INVALID, "null argument");
  if (NT < 1 || NT > INT32_MAX || HW < 1 || C < 1 || ld < C) fail(SF_ERR_INVALID, "bad shape");
  SF_HIP(launch_spatial_mean(F32, x, ld, (int)NT, HW, C, out, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_video_pool_bwd(const float *dp, int64_t NT, int HW, int C, int ld, float *dx, void *stream) {
  SF_API_BEGIN
  if (!dp || !dx) fail(SF_ERR_INVALID, "null argument");
  if (NT < 1 || HW < 1 || C < 1 || ld < C) fail(SF_ERR_INVALID, "bad shape");
  SF_HIP(launch_pool_bwd(dp, NT, HW, C, ld, dx, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int64_t sf_op_onset_loss_workspace_bytes(int64_t n) {
  if (n < 1 || n > INT32_MAX) return -1;
  return onset_loss_ws_bytes(n);
}

int sf_op_onset_bce_fwd(const float *z, const float *t, int64_t n, float *loss, float *stats, void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!z || !t || !loss || !stats || !ws) fail(SF_ERR_INVALID, "null argument");
  if (n < 1 || n > INT32_MAX) fail(SF_ERR_INVALID, "1 <= n <= 2^31 - 1 required");
  if ((uintptr_t)ws & 7u) fail(SF_ERR_INVALID, "misaligned workspace");
  const int64_t need = onset_loss_ws_bytes(n);
  if (ws_bytes < need) fail(SF_ERR_WORKSPACE, "workspace too small: need %lld bytes", (long long)need);
  SF_HIP(launch_onset_bce_fwd(z, t, n, loss, stats, ws, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_onset_bce_bwd(const float *z, const float *t, const float *stats, const float *g, int64_t n, float *dz, void *stream) {
  SF_API_BEGIN
  if (!z || !t || !stats || !g || !dz) fail(SF_ERR_INVALID, "null argument");
  if (n < 1 || n > INT32_MAX) fail(SF_ERR_INVALID, "1 <= n <= 2^31 - 1 required");
  SF_HIP(launch_onset_bce_bwd(z, t, stats, g, n, dz, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int sf_op_onset_metrics(const float *z, const float *t, int N, int T, float threshold, double *out, void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!z || !t || !out || !ws) fail(SF_ERR_INVALID, "null argument");
  if (N < 1 || T < 1) fail(SF_ERR_INVALID, "N >= 1 and T >= 1 required");
  const int64_t n = (int64_t)N * T;
  if (n > ONSET_METRICS_MAX) fail(SF_ERR_UNSUPPORTED, "step metrics take at most 2^24 logits (the AP count is quadratic in the balanced subset)");
  if (((uintptr_t)ws | (uintptr_t)out) & 7u) fail(SF_ERR_INVALID, "misaligned workspace or output");
  const int64_t need = onset_loss_ws_bytes(n);
  if (ws_bytes < need) fail(SF_ERR_WORKSPACE, "workspace too small: need %lld bytes", (long long)need);
  SF_HIP(launch_onset_metrics(z, t, N, T, threshold, out, ws, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

int64_t sf_op_onset_test_workspace_bytes(int N, int T) {
  if (N < 1 || T < 1 || (int64_t)N * T > ONSET_METRICS_MAX) return -1;
  return onset_test_ws_bytes(N, T);
}

int sf_op_onset_test_step(const float *logits, const float *labels, int N, int T, float logit_threshold, float metric_threshold, int64_t clip0,
                          int64_t capacity, int32_t *pred_count, int32_t *pred_frames, int32_t *target_count, int32_t *target_frames,
                          double *sums, void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!logits || !labels || !pred_count || !pred_frames || !target_count || !target_frames || !sums || !ws) fail(SF_ERR_INVALID, "null argument");
  if (N < 1 || T < 1 || clip0 < 0) fail(SF_ERR_INVALID, "N >= 1, T >= 1 and clip0 >= 0 required");
  if (clip0 > capacity || (int64_t)N > capacity - clip0) fail(SF_ERR_SHAPE, "rows [clip0, clip0 + N) do not fit the tables' capacity");
  if ((int64_t)N * T > ONSET_METRICS_MAX) fail(SF_ERR_UNSUPPORTED, "the test step takes at most 2^24 logits (the step metrics' limit)");
  if (((uintptr_t)ws | (uintptr_t)sums) & 7u) fail(SF_ERR_INVALID, "misaligned workspace or sums");
  const int64_t need = onset_test_ws_bytes(N, T);
  if (ws_bytes < need) fail(SF_ERR_WORKSPACE, "workspace too small: need %lld bytes", (long long)need);
  SF_HIP(launch_onset_test_step(logits, labels, N, T, logit_threshold, metric_threshold, clip0, pred_count, pred_frames, target_count,
                                target_frames, sums, ws, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

}  // extern "C"
