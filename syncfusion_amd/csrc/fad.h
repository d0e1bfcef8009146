// Device pieces of the FAD evaluation besides the front end (fad.hip): channels-last 2x2 max-pool, the fully connected layers' weight
// packer and the fp64 moments of the embeddings.  Shared by the kernels and the VGGish engine / C ABI (vggish_engine.cpp).  fp32 data,
// fp64 moments, on the caller's stream, no allocation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sf {

// rows (n, h, w) x ld -> rows (n, h / 2, w / 2) x ld: the maximum of each 2x2 window, every column alike (zero padding columns stay
// zero); floor division, so the last row / column of an odd extent is dropped.  H, W >= 2.
hipError_t launch_maxpool2x2_cl(const float *x, int64_t n, int H, int W, int ld, float *y, hipStream_t s);
// Linear weight (N, P * C) whose columns run (position, channel) -> out[n][p * ld + c], zeros at c >= C and from P * ld to K (K >= P * ld)
hipError_t launch_pack_fc(const float *w, int N, int P, int C, int ld, int K, float *out, hipStream_t s);
// x (N, D) fp32, D <= 128 -> sum[d] = sum_r x[r][d] and scatter[i][j] = sum_r (x[r][i] - sum[i] / N)(x[r][j] - sum[j] / N), both fp64,
// two passes, every sum in a fixed order (no atomics): identical input gives identical bits, and scatter is exactly symmetric
hipError_t launch_moments(const float *x, int64_t N, int D, double *sum, double *scatter, hipStream_t s);

}  // namespace sf
