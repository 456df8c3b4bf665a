// The display transform's per-pixel arithmetic (mcpt.h: display transform), the one copy of it: display.hip compiles it for the GPU,
// display_api.cpp for mcpt_display_host.  fp64, no contraction (-ffp-contract=off), IEEE division, every expression in the order mcpt.h
// writes it; tests/display_ref.py restates it in numpy.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/mcpt.h"

#ifndef MCPT_HD
#if defined(__HIPCC__)
#define MCPT_HD __host__ __device__ __forceinline__
#else
#define MCPT_HD inline
#endif
#endif

namespace mcpt {

MCPT_HD double display_luminance(double r, double g, double b) { return (0.2126 * r + 0.7152 * g) + 0.0722 * b; }

// the histogram slot of a luminance: from the bits of Y (exponent and top three mantissa bits), never from a logarithm
MCPT_HD int display_slot(double Y)
{
    if (!(Y > 0.0) || !(Y < INFINITY)) return 0;                       // skipped: NaN, <= 0, +inf
    uint64_t bits;
    __builtin_memcpy(&bits, &Y, sizeof bits);
    const int b = ((int(bits >> 52) - 1023 + 24) * 8) + int((bits >> 49) & 7);     // (the sign bit is clear: Y > 0)
    if (b < 0) return 1;
    if (b >= MCPT_DISPLAY_BINS) return MCPT_DISPLAY_SLOTS - 1;
    return b + 2;
}

// What the map needs once the parameters are resolved: the exposure e, w * w of REINHARD's white, the curve and the transfer.
struct DisplayMap {
    double e, ww;
    int32_t curve, transfer;
};

// one pixel's three channels c -> three bytes
MCPT_HD void display_pixel(const DisplayMap& m, const double c[3], uint8_t out[3])
{
    double x[3];
    for (int ch = 0; ch < 3; ch++) {
        double v = m.e * c[ch];
        v = v > 0.0 ? v : 0.0;                                         // NaN and negatives: 0
        x[ch] = v < 0x1p64 ? v : 0x1p64;                               // no infinity enters the curve
    }
    double y[3];
    if (m.curve == MCPT_CURVE_REINHARD) {
        const double Yx = display_luminance(x[0], x[1], x[2]);
        const double s = (1.0 + Yx / m.ww) / (1.0 + Yx);
        for (int ch = 0; ch < 3; ch++) y[ch] = Yx == 0.0 ? 0.0 : x[ch] * s;
    } else if (m.curve == MCPT_CURVE_FILMIC) {
        for (int ch = 0; ch < 3; ch++) y[ch] = (x[ch] * (2.51 * x[ch] + 0.03)) / (x[ch] * (2.43 * x[ch] + 0.59) + 0.14);
    } else {
        for (int ch = 0; ch < 3; ch++) y[ch] = x[ch];
    }
    for (int ch = 0; ch < 3; ch++) {
        double v = y[ch] < 1.0 ? y[ch] : 1.0;
        if (m.transfer == MCPT_TRANSFER_SRGB) {
            v = v <= 0.0031308 ? 12.92 * v : 1.055 * pow(v, 1.0 / 2.4) - 0.055;
            out[ch] = static_cast<uint8_t>(floor(v * 255 + 0.5));
        } else {
            v = v * 255;                                               // mcpt_quantize_rgb8's clamp and truncation (v is in [0, 255] already)
            v = v > 0.0 ? v : 0.0;
            v = v < 255.0 ? v : 255.0;
            out[ch] = static_cast<uint8_t>(v);
        }
    }
}

}  // namespace mcpt
