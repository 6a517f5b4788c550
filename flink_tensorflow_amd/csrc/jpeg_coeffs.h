// The record that travels with every image's coefficient row from the host entropy decoder
// (csrc/jpeg.cpp jpeg_entropy_into) to the device back half (kernels/jpeg.hip): plain data,
// included by both sides.
//
// Coefficient row: int16 quantised coefficients, de-zigzagged (index 8 * v + u, v the
// vertical frequency), 64 per block; the blocks of component c start at element
// comp[c].offset and lie in raster order of the MCU-padded plane (bw x bh blocks).
#pragma once
#include <stdint.h>

struct JpegCoeffComponent {
  int32_t h, v;    // sampling factors
  int32_t bw, bh;  // blocks per row / column of the padded plane
  int32_t offset;  // first coefficient of the plane, in int16 elements from the row's start
};

struct alignas(16) JpegCoeffHeader {
  int32_t status;  // 0: the row holds the image; anything else: not taken, decode it on the host
  int32_t ncomp;   // 1 (grayscale) or 3 (YCbCr, chroma 1x1, luma 1x1 / 2x1 / 2x2)
  JpegCoeffComponent comp[3];
  uint16_t qt[3][64];  // each component's quantisation table, zigzag order as the file stores it
  int32_t reserved[15];
};

static_assert(sizeof(JpegCoeffHeader) == 512, "JpegCoeffHeader is a fixed 512-byte record");
