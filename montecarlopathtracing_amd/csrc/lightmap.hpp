// Lightmap baking (mcpt.h: lightmaps): the arithmetic of a UV chart's coverage, the one copy of it -- lightmap.hip compiles it for the GPU,
// lightmap_api.cpp for mcpt_lightmap_raster_host -- and the launch interface of the baker's kernels.  fp64, no contraction
// (-ffp-contract=off), IEEE division, every expression in the order mcpt.h writes it; tests/lightmap_ref.py restates it in numpy.
#pragma once
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mcpt.h"
#include "device_scene.hpp"

#ifndef MCPT_HD
#if defined(__HIPCC__)
#define MCPT_HD __host__ __device__ __forceinline__
#else
#define MCPT_HD inline
#endif
#endif

namespace mcpt {

constexpr int32_t kLightmapMaxSize = 16384;      // texels per side
constexpr int32_t kLightmapMaxDilate = 64;       // rounds
constexpr int32_t kLightmapUnowned = 0x7fffffff; // owner[] while the faces still claim their texels: above every face index

// the centre of texel x of `size` along one axis
MCPT_HD double lightmap_centre(int x, int size) { return (double(x) + 0.5) / double(size); }

// twice the signed area of the chart triangle uv = (au, av, bu, bv, cu, cv)
MCPT_HD double lightmap_area2(const double* uv) { return (uv[2] - uv[0]) * (uv[5] - uv[1]) - (uv[3] - uv[1]) * (uv[4] - uv[0]); }

// the three edge functions of the centre (pu, pv): e[0] = e_a, e[1] = e_b, e[2] = e_c; e / area2 are the weights of corners a, b, c
MCPT_HD void lightmap_edges(const double* uv, double pu, double pv, double* e)
{
    const double au = uv[0], av = uv[1], bu = uv[2], bv = uv[3], cu = uv[4], cv = uv[5];
    e[0] = (bu - pu) * (cv - pv) - (bv - pv) * (cu - pu);
    e[1] = (cu - pu) * (av - pv) - (cv - pv) * (au - pu);
    e[2] = (au - pu) * (bv - pv) - (av - pv) * (bu - pu);
}

// a chart triangle takes part when its area is neither zero nor NaN nor infinite
MCPT_HD bool lightmap_area_ok(double area2) { return area2 != 0.0 && area2 > -INFINITY && area2 < INFINITY; }

MCPT_HD bool lightmap_covers(double area2, const double* e)
{
    return area2 > 0.0 ? (e[0] >= 0.0 && e[1] >= 0.0 && e[2] >= 0.0) : (e[0] <= 0.0 && e[1] <= 0.0 && e[2] <= 0.0);
}

// a face takes part when its geometric normal has a length that is neither zero nor NaN nor infinite
MCPT_HD bool lightmap_normal_ok(const double* n)
{
    const double l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    return l2 > 0.0 && l2 < INFINITY;
}

// The texels along one axis whose centre can lie in [lo, hi] (lo <= hi, both finite), one more on either side, inside the map:
// first .. last, empty when first > last.  The centres outside a chart triangle's bounding box are never tested against it.
MCPT_HD void lightmap_span(double lo, double hi, int size, int& first, int& last)
{
    const double a = floor(lo * double(size) - 0.5) - 1.0, b = ceil(hi * double(size) - 0.5) + 1.0;
    first = a > 0.0 ? (a < double(size) ? int(a) : size) : 0;
    last = b < double(size - 1) ? (b >= 0.0 ? int(b) : -1) : size - 1;
}

// the texel box of the chart triangle uv in a W x H map: x0 .. x1, y0 .. y1; false when it holds no texel
MCPT_HD bool lightmap_box(const double* uv, int W, int H, int& x0, int& x1, int& y0, int& y1)
{
    const double ulo = fmin(uv[0], fmin(uv[2], uv[4])), uhi = fmax(uv[0], fmax(uv[2], uv[4]));
    const double vlo = fmin(uv[1], fmin(uv[3], uv[5])), vhi = fmax(uv[1], fmax(uv[3], uv[5]));
    lightmap_span(ulo, uhi, W, x0, x1);
    lightmap_span(vlo, vhi, H, y0, y1);
    return x0 <= x1 && y0 <= y1;
}

// What a bake keeps between its kernels, all on the device; sizes for a map of n = W * H texels and a scene of t faces.
struct LightmapWork {
    int32_t* owner;                 // [n] step 1's answer (ping of the dilation)
    int32_t* slot_of_face;          // [t] .obj face -> triangle slot (leaf), filled by the raster
    int32_t* big;                   // [t] the slots whose texel box is too large for one wave
    unsigned int* n_big;            // their number (cleared by launch_lightmap_raster)
    unsigned long long* masks;      // [4 * lightmap_blocks(n)] a ballot per wave: which texels are covered
    int32_t* block_counts;          // [lightmap_blocks(n)]
    int32_t* block_offsets;         // [lightmap_blocks(n)]
    int32_t* total;                 // the number of covered texels
};
int lightmap_blocks(long long n);

// Step 1.  owner[y * W + x] = the lowest .obj face whose chart covers the texel's centre, or -1; d_uv6 [t][6] in .obj order, or null for
// the faces' own vt.  Then the count of covered texels (w.total) and what launch_lightmap_texels needs to place them (w.masks,
// w.block_offsets).
void launch_lightmap_raster(const DScene& S, const double* d_uv6, int W, int H, const LightmapWork& w, hipStream_t st);
// Step 2.  The covered texels in ascending order: d_texels[i] = T, d_q6[i] = position and normal of T's centre on its owner (either may
// be null).
void launch_lightmap_texels(const DScene& S, const double* d_uv6, int W, int H, const LightmapWork& w, int32_t* d_texels, double* d_q6, hipStream_t st);
// Step 4.  d_irr[T] = pi * mean[i], d_err[T] = pi * err[i], d_hits[T] = hits[i] for the n_list entries T = d_texels[i]; the caller has
// cleared the maps.  d_err / d_hits (and their sources) may be null.
void launch_lightmap_scatter(const int32_t* d_texels, long long n_list, const double* d_mean, const double* d_stderr, const int32_t* d_hits_in,
                             double* d_irr, double* d_err, int32_t* d_hits, hipStream_t st);
// Step 5, round r: (in, owner_in) -> (out, owner_out), every texel of the W x H map written; channels a texel: 3, or 1 (an occlusion map).
void launch_lightmap_dilate(const double* d_in, const int32_t* d_owner_in, int W, int H, int round, double* d_out, int32_t* d_owner_out, int channels,
                            hipStream_t st);

}  // namespace mcpt
