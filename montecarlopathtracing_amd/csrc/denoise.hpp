// Launch interface of the first-hit AOVs and the edge-avoiding a-trous denoiser of progressive frames (denoise.hip, mcpt.h:
// mcpt_progressive_aovs / mcpt_progressive_denoise).
#pragma once
#include <hip/hip_runtime_api.h>

#include "kernels.hpp"

namespace mcpt {

// What a tap of the filter reads of its neighbour's guide, one 48-byte record per pixel (three 16-byte loads): the normalised normal
// AOV, the depth and the material.  material < 0: not a surface pixel (not owned, a miss or an emitter) -- never a neighbour.
struct alignas(16) DenoiseGuide {
    double n[3];
    double t;
    int32_t material;
    int32_t pad[3];
};
static_assert(sizeof(DenoiseGuide) == 48, "three 16-byte loads");

// A surface pixel between iterations: the demodulated colour e and its luminance variance v (32 bytes, two 16-byte loads).
struct alignas(32) DenoisePix {
    double e[3];
    double v;
};
static_assert(sizeof(DenoisePix) == 32, "two 16-byte loads");

// One lane per owned pixel pixels[i], from its primary hit hits[i]: material (-1 on a miss), depth, normal and albedo (W*H[*3]) and
// the guide record of the surface pixels.  Other pixels are not touched.
void launch_primary_aov(const DScene& S, const int32_t* d_pixels, int n_pixels, const PrimaryHit* d_hits, int32_t* d_mat, double* d_depth,
                        double* d_normal, double* d_albedo, DenoiseGuide* d_guide, hipStream_t st);
// The filter of mcpt.h over the owned pixels after `done` of N samples (d_cnt: per-pixel counts of an adaptive frame, else null).
// Surface pixels go through `iterations` a-trous passes ping-ponging between d_buf[0] and d_buf[1] (W*H each), the last one writing
// albedo * e to d_out; every other owned pixel gets the estimate of mcpt_progressive_image.  Pixels not owned are not touched.
void launch_denoise(const int32_t* d_pixels, long long n_pixels, int width, int height, const double* d_img, const double* d_mom, int done,
                    const int32_t* d_cnt, int N, const double* d_albedo, const DenoiseGuide* d_guide, int iterations, double sigma_l,
                    double sigma_z, DenoisePix* d_buf0, DenoisePix* d_buf1, double* d_out, hipStream_t st);

}  // namespace mcpt
