// Launch interface of the lightmap denoiser's kernels (lightmap_denoise.hip, mcpt.h: mcpt_lightmap_denoise): the guides of a map's covered
// texels, the filter's input and its a-trous iterations.  Coverage and dilation are the baker's own (lightmap.hpp), unchanged.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "lightmap.hpp"

namespace mcpt {

// What a tap of the filter reads of its neighbour's guide, one 64-byte record per texel (four 16-byte loads): the texel centre's world
// position, its normal divided by its length, the world length of a texel's side on its face and whether the texel is covered.
// covered == 0: never a neighbour (the rest of the record is 0).
struct alignas(16) LightmapGuide {
    double p[3];
    double n[3];
    double h;
    int32_t covered;
    int32_t pad;
};
static_assert(sizeof(LightmapGuide) == 64, "four 16-byte loads");

// A covered texel between iterations: the irradiance e and its luminance variance v (32 bytes, two 16-byte loads).
struct alignas(32) LightmapPix {
    double e[3];
    double v;
};
static_assert(sizeof(LightmapPix) == 32, "two 16-byte loads");

// The filter of mcpt.h over a W x H map whose coverage launch_lightmap_raster has left in w (w.owner, w.slot_of_face), every texel of
// d_out written: the guides into d_guide [W * H], (e, v) of the covered texels from d_irr and d_err, `iterations` a-trous passes that
// ping-pong between d_buf0 and d_buf1 [W * H each], the last one writing e to d_out and +0.0 to the texels not covered.  iterations == 0:
// d_out is d_irr at the covered texels, bit for bit.  d_out may be d_irr: every input is read before anything is written there.
void launch_lightmap_denoise(const DScene& S, const double* d_uv6, int W, int H, const LightmapWork& w, const double* d_irr, const double* d_err,
                             int iterations, double sigma_l, double sigma_p, LightmapGuide* d_guide, LightmapPix* d_buf0, LightmapPix* d_buf1,
                             double* d_out, hipStream_t st);

}  // namespace mcpt
