// The device JPEG decoder's launcher (jpeg.hip) as capi_jpeg.cpp calls it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "jpeg_decode.h"

namespace sf {

static_assert(offsetof(sf_jpeg_desc, quant) % 16 == 0 && sizeof(sf_jpeg_desc) % 16 == 0, "the IDCT kernel reads quant in 16-byte vectors");
static_assert(sizeof(sf_jpeg_segment) == 32, "sf_jpeg_segment is the entropy kernel's table entry");

// coef_elems: int16 elements of the coefficient area (the planes follow it); max_image_blocks: the largest block count of one file.
// Every argument has been checked by the caller (sf_jpeg_decode).
hipError_t launch_jpeg_decode(const uint8_t *bytes, int64_t n_bytes, const sf_jpeg_desc *desc_dev, const sf_jpeg_segment *segs_dev, int64_t n_segs,
                              int N, int H, int W, int64_t coef_elems, int64_t max_image_blocks, uint8_t *out, int32_t *status, void *ws,
                              hipStream_t s);

}  // namespace sf
