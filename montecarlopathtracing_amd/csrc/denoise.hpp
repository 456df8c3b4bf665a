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

// The guide record of the filter guided by sample AOVs (mcpt_progressive_denoise_guided), 64 bytes per pixel (four 16-byte loads): the
// normalised normal AOV, the depth AOV, the demodulation colour m = max(cov * albedo, 0.01) and whether the pixel is filtered (owned,
// ns > 0, ne == 0).  filtered == 0: never a neighbour.  Written by the sample-AOV fold (sample_aov.hip); the first-hit path never sees it.
struct alignas(16) SampleGuide {
    double n[3];
    double t;
    double m[3];
    int32_t filtered;
    int32_t pad;
};
static_assert(sizeof(SampleGuide) == 64, "four 16-byte loads");

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
// The filter of mcpt.h's mcpt_progressive_denoise_guided: as launch_denoise, on the guide records of the sample AOVs; sigma_a weighs the
// difference of the demodulation colours.
void launch_denoise_guided(const int32_t* d_pixels, long long n_pixels, int width, int height, const double* d_img, const double* d_mom, int done,
                           const int32_t* d_cnt, int N, const SampleGuide* d_guide, int iterations, double sigma_l, double sigma_z, double sigma_a,
                           DenoisePix* d_buf0, DenoisePix* d_buf1, double* d_out, hipStream_t st);

// ---- sample AOVs (sample_aov.hip, mcpt.h: mcpt_progressive_sample_aovs)
// The camera rays of samples k = 0 .. G-1 of pixels d_pixels[first .. first + n) under `lens`, sample-major: ray j = k * n + i.
void launch_guide_rays(const DLens& lens, unsigned long long seed, const int32_t* d_pixels, int first, int n, int G, double* d_rays6, hipStream_t st);
// One lane per pixel of the chunk folds its G closest hits (leaf, t, p: launch_trace_closest_leaf of those rays) in k order into the
// counts (ns, ne, nm), the depth, normal and albedo AOVs and the pixel's guide record.
void launch_guide_fold(const DScene& S, const int32_t* d_pixels, int first, int n, int G, const int32_t* d_leaf, const double* d_t, const double* d_p,
                       int32_t* d_counts, double* d_depth, double* d_normal, double* d_albedo, SampleGuide* d_guide, hipStream_t st);

}  // namespace mcpt
