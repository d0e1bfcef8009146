// JPEG frames on the device (include/syncfusion_amd.h, "JPEG frames on the device"): three kernels behind sf_jpeg_decode.
//
//   entropy   one wave per segment of the segment table.  Lanes 0..3 build the four Huffman lookup tables of the segment's file in LDS
//             (tables differ per file: optimised tables are common), then the wave walks the bitstream (jpeg_decode.h, the code the host
//             tests run) one block at a time into a 64-entry LDS block -- serially: all lanes run the walk on the same wave-uniform values,
//             which keeps the bit buffer and its branches in scalar registers -- and stores the block as one 128-byte row of int16
//             coefficients in natural order.  The first problem of a file goes into its status word (atomicCAS against 0); the wave stops
//             there, so what it has not reached stays zero (the call zeroes the coefficient area first).
//   idct      one thread per 8x8 block: dequantise, libjpeg's "islow" integer IDCT (jidctint, CONST_BITS 13, PASS1_BITS 2), level shift,
//             clamp -> uint8 component planes of the padded (whole-MCU) extent.  16-byte coefficient loads, 8-byte row stores.
//   colour    16 consecutive pixels of the (N, H, W, 3) output per thread: fancy h2v1 / h2v2 chroma upsampling over the REAL downsampled
//             extent (edge row and column replicated, the MCU padding is never read as a neighbour), integer YCbCr -> RGB, three 16-byte
//             stores.  Files that are not SF_JPEG_OK get zeros.
//
// Workspace: [ int16 coefficients of every file | uint8 planes of every file ], a file's share at desc.coef_offset / desc.plane_offset.
#include "common.h"
#include "jpeg.h"

namespace sf {

namespace {

constexpr int JPEG_PIX_THREADS = 256;
constexpr int JPEG_PX_PER_THREAD = 16;

__device__ __forceinline__ void jpeg_flag(int32_t *status, int image, int code) { atomicCAS(status + image, 0, code); }

__global__ __launch_bounds__(WAVE) void jpeg_entropy_kernel(const uint8_t *__restrict__ bytes, int64_t n_bytes, const sf_jpeg_desc *__restrict__ desc,
                                                            const sf_jpeg_segment *__restrict__ segs, int N, int16_t *__restrict__ coef,
                                                            int32_t *__restrict__ status) {
  __shared__ JpegHuff tabs[4];
  __shared__ int16_t block[64];
  __shared__ uint8_t natural[64];
  __shared__ int problem;
  const int lane = threadIdx.x;
  const sf_jpeg_segment g = segs[blockIdx.x];
  if (g.image < 0 || g.image >= N) return;
  const sf_jpeg_desc &d = desc[g.image];
  if (d.status != SF_JPEG_OK) return;
  const int ncomp = d.ncomp, mcus_x = d.mcus_x;
  const int64_t mcus = (int64_t)mcus_x * d.mcus_y;
  bool sane = (ncomp == 1 || ncomp == 3) && mcus_x >= 1 && d.mcus_y >= 1 && g.first_mcu >= 0 && g.mcu_count >= 0 &&
              (int64_t)g.first_mcu + g.mcu_count <= mcus && g.byte_begin >= 0 && g.byte_begin <= g.byte_end && g.byte_end <= n_bytes;
  for (int c = 0; c < 3 && c < ncomp; ++c)
    sane = sane && d.h[c] >= 1 && d.h[c] <= 2 && d.v[c] >= 1 && d.v[c] <= 2 && d.td[c] >= 0 && d.td[c] <= 1 && d.ta[c] >= 0 && d.ta[c] <= 1;
  if (!sane) {
    if (lane == 0) jpeg_flag(status, g.image, SF_JPEG_ST_BAD_SEGMENT);
    return;
  }
  if (lane < 4) jpeg_build_huff(d.huff_counts[lane], d.huff_values[lane], &tabs[lane]);
  block[lane] = 0;
  {
    const uint8_t order[64] = SF_JPEG_NATURAL_ORDER;
    natural[lane] = order[lane];
  }
  if (lane == 0) problem = 0;
  __syncthreads();
  const int64_t image_blocks = jpeg_image_blocks(d);
  int16_t *img = coef + d.coef_offset;
  JpegBits r;
  r.open(bytes, 0, n_bytes, g.byte_begin, g.byte_end);
  int pred[3] = {0, 0, 0};
  for (int m = g.first_mcu; m < g.first_mcu + g.mcu_count; ++m) {
    const int my = m / mcus_x, mx = m - my * mcus_x;
    int64_t comp_base = 0;
    for (int c = 0; c < ncomp; ++c) {
      const int ch = d.h[c], cv = d.v[c], bw = mcus_x * ch;
      for (int v = 0; v < cv; ++v) {
        for (int h = 0; h < ch; ++h) {
          {   // every lane, on the same (wave-uniform) values: the stores into `block` and `problem` coincide
            const int e = jpeg_decode_block(r, tabs[d.td[c]], tabs[2 + d.ta[c]], natural, &pred[c], block);
            if (e) problem = e;
          }
          __syncthreads();
          const int e = problem;   // the same on every lane
          const int64_t slot = comp_base + (int64_t)(my * cv + v) * bw + mx * ch + h;
          if (!e && slot < image_blocks) img[slot * 64 + lane] = block[lane];
          block[lane] = 0;
          __syncthreads();
          if (e) {
            if (lane == 0) jpeg_flag(status, g.image, e);
            return;
          }
        }
      }
      comp_base += (int64_t)bw * d.mcus_y * cv;
    }
  }
  if (lane == 0 && r.bytes_left() > 0) jpeg_flag(status, g.image, SF_JPEG_ST_TRAILING_BYTES);
}

// jidctint's 1-D pass on eight values; out = DESCALE(., shift).  The sums and products are formed in unsigned arithmetic: inside the
// exactness contract they never leave the int range and the result is jidctint's; on corrupted coefficients they wrap instead of
// overflowing a signed int.
template <int SHIFT> __device__ __forceinline__ void idct_1d(const int *in, int stride, int *out, int ostride) {
  typedef unsigned U;
  const U in0 = (U)in[0], in1 = (U)in[stride], in2 = (U)in[2 * stride], in3 = (U)in[3 * stride], in4 = (U)in[4 * stride], in5 = (U)in[5 * stride],
          in6 = (U)in[6 * stride], in7 = (U)in[7 * stride];
  U z1 = (in2 + in6) * 4433u;
  const U e2 = z1 - in6 * 15137u, e3 = z1 + in2 * 6270u;
  const U e0 = (in0 + in4) * 8192u, e1 = (in0 - in4) * 8192u;
  const U t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  U t0 = in7, t1 = in5, t2 = in3, t3 = in1;
  z1 = t0 + t3;
  U z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const U z5 = (z3 + z4) * 9633u;
  t0 *= 2446u;
  t1 *= 16819u;
  t2 *= 25172u;
  t3 *= 12299u;
  z1 *= (U)-7373;
  z2 *= (U)-20995;
  z3 = z3 * (U)-16069 + z5;
  z4 = z4 * (U)-3196 + z5;
  t0 += z1 + z3;
  t1 += z2 + z4;
  t2 += z2 + z3;
  t3 += z1 + z4;
  constexpr U R = 1u << (SHIFT - 1);
  out[0] = (int)(t10 + t3 + R) >> SHIFT;
  out[7 * ostride] = (int)(t10 - t3 + R) >> SHIFT;
  out[ostride] = (int)(t11 + t2 + R) >> SHIFT;
  out[6 * ostride] = (int)(t11 - t2 + R) >> SHIFT;
  out[2 * ostride] = (int)(t12 + t1 + R) >> SHIFT;
  out[5 * ostride] = (int)(t12 - t1 + R) >> SHIFT;
  out[3 * ostride] = (int)(t13 + t0 + R) >> SHIFT;
  out[4 * ostride] = (int)(t13 - t0 + R) >> SHIFT;
}

typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

__global__ __launch_bounds__(JPEG_PIX_THREADS) void jpeg_idct_kernel(const sf_jpeg_desc *__restrict__ desc, const int16_t *__restrict__ coef,
                                                                     uint8_t *__restrict__ planes) {
  const sf_jpeg_desc &d = desc[blockIdx.y];
  if (d.status != SF_JPEG_OK) return;
  int64_t t = (int64_t)blockIdx.x * JPEG_PIX_THREADS + threadIdx.x, base = 0;
  int c = 0;
  for (; c < d.ncomp; ++c) {
    const int64_t nb = jpeg_comp_blocks(d, c);
    if (t < nb) break;
    t -= nb;
    base += nb;
  }
  if (c >= d.ncomp) return;
  const int bw = jpeg_blocks_w(d, c);
  const int by = (int)(t / bw), bx = (int)(t - (int64_t)by * bw);
  const s16x8 *src = reinterpret_cast<const s16x8 *>(coef + d.coef_offset + (base + t) * 64);
  const u16x8 *q = reinterpret_cast<const u16x8 *>(d.quant[d.tq[c] & 3]);
  int w[64];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const s16x8 cv = src[r];
    const u16x8 qv = q[r];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[r * 8 + k] = (int)((unsigned)(int)cv[k] * (unsigned)qv[k]);
  }
#pragma unroll
  for (int col = 0; col < 8; ++col) idct_1d<11>(w + col, 8, w + col, 8);   // pass 1: columns
  uint8_t *dst = planes + d.plane_offset + base * 64 + ((int64_t)by * 8) * ((int64_t)bw * 8) + bx * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int o[8];
    idct_1d<18>(w + r * 8, 1, o, 1);   // pass 2: rows
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lo |= (uint32_t)min(max(o[k] + 128, 0), 255) << (8 * k);   // (|o| < 2^14 after the descale by 18)
      hi |= (uint32_t)min(max(o[k + 4] + 128, 0), 255) << (8 * k);
    }
    *reinterpret_cast<uint2 *>(dst + (int64_t)r * bw * 8) = make_uint2(lo, hi);
  }
}

// what the colour kernel needs of one file
struct JpegPixInfo {
  const uint8_t *y, *cb, *cr;
  int pw_y, pw_c;   // plane row pitches
  int cw, chh;      // the real downsampled chroma extent
  int mode;         // -1: not decoded, 0: one component, 1: 1x1, 2: h2v1, 3: h2v2; +4: plain replication (downsampled width <= 2)
};

__device__ __forceinline__ JpegPixInfo jpeg_pix_info(const sf_jpeg_desc &d, const uint8_t *planes, int H, int W) {
  JpegPixInfo p;
  p.mode = -1;
  if (d.status != SF_JPEG_OK) return p;
  p.y = planes + d.plane_offset;
  p.pw_y = jpeg_blocks_w(d, 0) * 8;
  if (d.ncomp == 1) {
    p.mode = 0;
    return p;
  }
  p.cb = p.y + jpeg_comp_blocks(d, 0) * 64;
  p.cr = p.cb + jpeg_comp_blocks(d, 1) * 64;
  p.pw_c = jpeg_blocks_w(d, 1) * 8;
  p.cw = (W + d.h[0] - 1) / d.h[0];
  p.chh = (H + d.v[0] - 1) / d.v[0];
  p.mode = d.h[0] == 1 ? 1 : (d.v[0] == 1 ? 2 : 3);
  if (p.mode >= 2 && p.cw <= 2) p.mode += 4;
  return p;
}

__device__ __forceinline__ int jpeg_chroma(const uint8_t *plane, const JpegPixInfo &p, int y, int x) {
  if (p.mode == 1) return plane[(int64_t)y * p.pw_c + x];
  const int i = x >> 1;
  if (p.mode == 2) {
    const uint8_t *row = plane + (int64_t)y * p.pw_c;
    const int c = row[i];
    if (x & 1) return i == p.cw - 1 ? c : (3 * c + row[i + 1] + 2) >> 2;
    return i == 0 ? c : (3 * c + row[i - 1] + 1) >> 2;
  }
  if (p.mode == 3) {
    const int yn = y >> 1;
    int yf = (y & 1) ? yn + 1 : yn - 1;
    yf = min(max(yf, 0), p.chh - 1);
    const uint8_t *near = plane + (int64_t)yn * p.pw_c, *far = plane + (int64_t)yf * p.pw_c;
    const int s = 3 * near[i] + far[i];
    if (x & 1) return i == p.cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
    return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
  }
  return plane[(int64_t)(p.mode == 7 ? y >> 1 : y) * p.pw_c + i];   // 6, 7: replication
}

__global__ __launch_bounds__(JPEG_PIX_THREADS) void jpeg_colour_kernel(const sf_jpeg_desc *__restrict__ desc, int H, int W, int64_t total_px,
                                                                       const uint8_t *__restrict__ planes, uint8_t *__restrict__ out) {
  const int64_t p0 = ((int64_t)blockIdx.x * JPEG_PIX_THREADS + threadIdx.x) * JPEG_PX_PER_THREAD;
  if (p0 >= total_px) return;
  const int64_t hw = (int64_t)H * W;
  int64_t n = p0 / hw;
  const int64_t rem = p0 - n * hw;
  int y = (int)(rem / W), x = (int)(rem - (int64_t)y * W);
  JpegPixInfo p = jpeg_pix_info(desc[n], planes, H, W);
  uint32_t word[JPEG_PX_PER_THREAD * 3 / 4];
#pragma unroll
  for (int k = 0; k < JPEG_PX_PER_THREAD * 3 / 4; ++k) word[k] = 0;
  const int count = (int)min((int64_t)JPEG_PX_PER_THREAD, total_px - p0);
#pragma unroll
  for (int i = 0; i < JPEG_PX_PER_THREAD; ++i) {
    if (i < count) {
      int R = 0, G = 0, B = 0;
      if (p.mode >= 0) {
        const int Y = p.y[(int64_t)y * p.pw_y + x];
        R = G = B = Y;
        if (p.mode > 0) {
          const int cb = jpeg_chroma(p.cb, p, y, x) - 128, cr = jpeg_chroma(p.cr, p, y, x) - 128;
          R = min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
          B = min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
          G = min(max(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
        }
      }
      word[(3 * i) >> 2] |= (uint32_t)R << (8 * ((3 * i) & 3));
      word[(3 * i + 1) >> 2] |= (uint32_t)G << (8 * ((3 * i + 1) & 3));
      word[(3 * i + 2) >> 2] |= (uint32_t)B << (8 * ((3 * i + 2) & 3));
      if (++x == W) {
        x = 0;
        if (++y == H) {
          y = 0;
          ++n;
          if (i + 1 < count) p = jpeg_pix_info(desc[n], planes, H, W);
        }
      }
    }
  }
  uint8_t *dst = out + p0 * 3;
  if (count == JPEG_PX_PER_THREAD) {   // 48 bytes at a multiple of 48 from a 16-byte-aligned base
    u32x4 *d4 = reinterpret_cast<u32x4 *>(dst);
#pragma unroll
    for (int k = 0; k < 3; ++k) d4[k] = u32x4{word[4 * k], word[4 * k + 1], word[4 * k + 2], word[4 * k + 3]};
  } else {
    for (int b = 0; b < count * 3; ++b) dst[b] = (uint8_t)(word[b >> 2] >> (8 * (b & 3)));
  }
}

}  // namespace

hipError_t launch_jpeg_decode(const uint8_t *bytes, int64_t n_bytes, const sf_jpeg_desc *desc_dev, const sf_jpeg_segment *segs_dev, int64_t n_segs,
                              int N, int H, int W, int64_t coef_elems, int64_t max_image_blocks, uint8_t *out, int32_t *status, void *ws,
                              hipStream_t s) {
  int16_t *coef = static_cast<int16_t *>(ws);
  uint8_t *planes = static_cast<uint8_t *>(ws) + coef_elems * 2;
  hipError_t e = hipMemsetAsync(status, 0, (size_t)N * sizeof(int32_t), s);
  if (e != hipSuccess) return e;
  if (coef_elems > 0) {
    e = hipMemsetAsync(coef, 0, (size_t)coef_elems * 2, s);
    if (e != hipSuccess) return e;
  }
  if (n_segs > 0) {
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)n_segs), dim3(WAVE), 0, s, bytes, n_bytes, desc_dev, segs_dev, N, coef, status);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (max_image_blocks > 0) {
    const unsigned gx = (unsigned)((max_image_blocks + JPEG_PIX_THREADS - 1) / JPEG_PIX_THREADS);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(gx, (unsigned)N), dim3(JPEG_PIX_THREADS), 0, s, desc_dev, coef, planes);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const int64_t total_px = (int64_t)N * H * W;
  const int64_t threads = (total_px + JPEG_PX_PER_THREAD - 1) / JPEG_PX_PER_THREAD;
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((threads + JPEG_PIX_THREADS - 1) / JPEG_PIX_THREADS)), dim3(JPEG_PIX_THREADS), 0, s, desc_dev, H, W,
                     total_px, planes, out);
  return hipGetLastError();
}

}  // namespace sf
