// The JPEG entry points of the C ABI: the host parser (jpeg_parse.h), the workspace query and the device decode (jpeg.hip).
#include "engine_common.h"
#include "jpeg.h"
#include "jpeg_parse.h"

using namespace sf;

namespace {

constexpr int JPEG_MAX_BATCH = 65535;   // the IDCT kernel's grid.y

// what a descriptor must say for the kernels to stay inside the workspace and the byte buffer; `why` names the first violation
bool desc_fits(const sf_jpeg_desc &d, int H, int W, int64_t n_bytes, int64_t n_segs, int64_t coef_at, int64_t plane_at, const char **why) {
  *why = nullptr;
  if (d.width != W || d.height != H) *why = "size differs from the batch";
  else if (d.ncomp != 1 && d.ncomp != 3) *why = "component count";
  else if (d.seg_count < 1 || d.seg_begin < 0 || d.seg_begin + d.seg_count > n_segs) *why = "segment range";
  else if (d.data_begin < 0 || d.data_begin > d.data_end || d.data_end > n_bytes) *why = "data range";
  else if (d.coef_offset != coef_at || d.plane_offset != plane_at) *why = "workspace offsets (descriptors of another batch?)";
  if (*why) return false;
  for (int c = 0; c < d.ncomp; ++c) {
    const bool luma_ok = d.ncomp == 1 ? (d.h[0] == 1 && d.v[0] == 1) : ((d.h[0] == 1 && d.v[0] == 1) || (d.h[0] == 2 && (d.v[0] == 1 || d.v[0] == 2)));
    if (c == 0 ? !luma_ok : (d.h[c] != 1 || d.v[c] != 1)) *why = "sampling factors";
    else if (d.tq[c] < 0 || d.tq[c] > 3 || d.quant_precision[d.tq[c]] < 0) *why = "quantisation table selector";
    else if (d.td[c] < 0 || d.td[c] > 1 || d.ta[c] < 0 || d.ta[c] > 1) *why = "Huffman table selector";
    if (*why) return false;
  }
  if (d.mcus_x != (W + 8 * d.h[0] - 1) / (8 * d.h[0]) || d.mcus_y != (H + 8 * d.v[0] - 1) / (8 * d.v[0])) *why = "MCU counts";
  return *why == nullptr;
}

}  // namespace

extern "C" {

int sf_jpeg_parse(const uint8_t *bytes, const int64_t *offsets, int N, sf_jpeg_desc *desc_out, sf_jpeg_segment *segs_out, int64_t seg_capacity,
                  int64_t *n_segs_out) {
  SF_API_BEGIN
  if (!bytes || !offsets || !desc_out || !n_segs_out || N < 1 || N > JPEG_MAX_BATCH) fail(SF_ERR_INVALID, "jpeg parse: null argument or N outside 1..%d", JPEG_MAX_BATCH);
  if (offsets[0] < 0) fail(SF_ERR_INVALID, "jpeg parse: negative offset");
  for (int i = 0; i < N; ++i)
    if (offsets[i + 1] < offsets[i]) fail(SF_ERR_INVALID, "jpeg parse: offsets decrease at file %d", i);
  int64_t n_segs = 0, coef = 0, plane = 0;
  int first_bad = -1;
  for (int i = 0; i < N; ++i) {
    sf_jpeg_desc &d = desc_out[i];
    const int st = jpeg_parse_one(bytes, offsets[i], offsets[i + 1], &d);
    if (st == SF_JPEG_MALFORMED && first_bad < 0) first_bad = i;
    if (st != SF_JPEG_OK) {
      d.seg_count = 0;
      continue;
    }
    d.seg_begin = n_segs;
    d.coef_offset = coef;
    d.plane_offset = plane;
    n_segs += d.seg_count;
    coef += jpeg_coef_elems(d);
    plane += jpeg_plane_bytes(d);
  }
  *n_segs_out = n_segs;
  if (n_segs > INT32_MAX) fail(SF_ERR_SHAPE, "jpeg parse: %lld segments", (long long)n_segs);
  if (segs_out) {
    if (seg_capacity < n_segs) fail(SF_ERR_WORKSPACE, "jpeg parse: %lld segments, room for %lld", (long long)n_segs, (long long)seg_capacity);
    for (int i = 0; i < N; ++i)
      if (desc_out[i].status == SF_JPEG_OK) jpeg_fill_segments(bytes, &desc_out[i], i, segs_out + desc_out[i].seg_begin);
  }
  if (first_bad >= 0) fail(SF_ERR_INVALID, "jpeg parse: file %d is malformed: %s", first_bad, desc_out[first_bad].reason);
  return SF_OK;
  SF_API_END
}

int64_t sf_jpeg_decode_workspace_bytes(const sf_jpeg_desc *desc, int N) {
  if (!desc || N < 1 || N > JPEG_MAX_BATCH) return -1;
  int64_t total = 0;
  for (int i = 0; i < N; ++i) {
    if (desc[i].status != SF_JPEG_OK) continue;
    if (desc[i].ncomp < 1 || desc[i].ncomp > 3 || desc[i].mcus_x < 1 || desc[i].mcus_y < 1) return -1;
    for (int c = 0; c < desc[i].ncomp; ++c)
      if (desc[i].h[c] < 1 || desc[i].h[c] > 4 || desc[i].v[c] < 1 || desc[i].v[c] > 4) return -1;
    total += jpeg_coef_elems(desc[i]) * 2 + jpeg_plane_bytes(desc[i]);
  }
  return total;
}

int sf_jpeg_decode(const uint8_t *bytes_dev, int64_t n_bytes, const sf_jpeg_desc *desc_host, const sf_jpeg_desc *desc_dev, const sf_jpeg_segment *segs_dev,
                   int64_t n_segs, int N, int H, int W, uint8_t *out, int32_t *status_dev, void *ws, int64_t ws_bytes, void *stream) {
  SF_API_BEGIN
  if (!desc_host || !desc_dev || !out || !status_dev || N < 1 || N > JPEG_MAX_BATCH || H < 1 || W < 1 || n_bytes < 0 || n_segs < 0 || n_segs > INT32_MAX)
    fail(SF_ERR_INVALID, "jpeg decode: null argument, or N, H, W, n_bytes, n_segs out of range");
  if ((int64_t)N * H * W > ((int64_t)1 << 40)) fail(SF_ERR_SHAPE, "jpeg decode: more than 2^40 pixels");
  if (reinterpret_cast<uintptr_t>(out) % 16 || reinterpret_cast<uintptr_t>(ws) % 16 || reinterpret_cast<uintptr_t>(desc_dev) % 16)
    fail(SF_ERR_INVALID, "jpeg decode: out, ws and desc_dev must be 16-byte aligned");
  int64_t coef = 0, plane = 0, segs = 0, max_blocks = 0;
  for (int i = 0; i < N; ++i) {   // every way a descriptor could send a kernel out of bounds is refused here
    const sf_jpeg_desc &d = desc_host[i];
    if (d.status != SF_JPEG_OK) continue;
    const char *why = nullptr;
    if (!desc_fits(d, H, W, n_bytes, n_segs, coef, plane, &why)) fail(SF_ERR_INVALID, "jpeg decode: file %d: %s", i, why);
    if (d.seg_begin != segs) fail(SF_ERR_INVALID, "jpeg decode: file %d: segment range out of order", i);
    segs += d.seg_count;
    coef += jpeg_coef_elems(d);
    plane += jpeg_plane_bytes(d);
    max_blocks = std::max<int64_t>(max_blocks, jpeg_image_blocks(d));
  }
  if (segs != n_segs) fail(SF_ERR_INVALID, "jpeg decode: %lld segments given, the descriptors hold %lld", (long long)n_segs, (long long)segs);
  if (n_segs > 0 && (!bytes_dev || !segs_dev)) fail(SF_ERR_INVALID, "jpeg decode: null byte buffer or segment table");
  if (coef * 2 + plane > 0) require_workspace(ws, ws_bytes, coef * 2 + plane);
  SF_HIP(launch_jpeg_decode(bytes_dev, n_bytes, desc_dev, segs_dev, n_segs, N, H, W, coef, max_blocks, out, status_dev, ws, static_cast<hipStream_t>(stream)));
  return SF_OK;
  SF_API_END
}

}  // extern "C"
