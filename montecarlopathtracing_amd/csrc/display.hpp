// Launch interface of the display transform (display.hip, mcpt.h: display transform): the luminance histogram of a linear fp64 frame and
// its map to 8-bit pixels, both on the frame where it lies in HBM.
#pragma once
#include <hip/hip_runtime_api.h>

#include "display_math.hpp"

namespace mcpt {

// The luminance histogram of pixels d_pixels[0 .. n) of the frame d_img (d_pixels == null: pixels 0 .. n), added into the
// MCPT_DISPLAY_SLOTS counts of d_slots, which the caller has cleared on the same stream.
void launch_display_histogram(const double* d_img, const int32_t* d_pixels, long long n, unsigned long long* d_slots, hipStream_t st);

// The map of the same pixels into d_out, 3 bytes per pixel (rgba: 4, alpha 255) at the pixel's own place; other pixels are not touched.
// Without a list, with d_img aligned to 16 bytes and d_out to 4 (rgba: 16), one lane maps four pixels and writes dwords; otherwise one
// lane maps one pixel and writes bytes.
void launch_display_map(const double* d_img, const int32_t* d_pixels, long long n, const DisplayMap& m, bool rgba, uint8_t* d_out, hipStream_t st);

}  // namespace mcpt
