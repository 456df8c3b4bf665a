// Ambient occlusion (mcpt.h: ambient occlusion): the arithmetic of an entry's fold -- the value of one sample under a falloff, the five
// sums, the standard error, the bent normal and its fallback --, the one copy of it: occlusion.hip compiles it for the GPU,
// occlusion_api.cpp for mcpt_occlusion_fold_host.  fp64, no contraction (-ffp-contract=off), IEEE division, every expression in the order
// mcpt.h writes it; tests/occlusion_ref.py restates it in numpy.  The launch interface of the three kernels is at the end; a map is dilated
// by the lightmap's own kernel on one channel (lightmap.hpp: launch_lightmap_dilate).
#pragma once
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mcpt.h"
#include "visibility.hpp"

namespace mcpt {

// what an entry adds up over its samples, in j order
struct OccSums {
    double s1, s2, b[3];
    int hits, back;
};

MCPT_HD void occlusion_clear(OccSums& a)
{
    a.s1 = 0.0; a.s2 = 0.0; a.b[0] = 0.0; a.b[1] = 0.0; a.b[2] = 0.0;
    a.hits = 0; a.back = 0;
}

// a sample is near when its ray hit something closer than max_distance (a t that is NaN is not near)
MCPT_HD bool occlusion_near(bool hit, double t, double max_distance) { return hit && t < max_distance; }

// the visibility v of one sample: 1.0 when it is not near, otherwise the falloff of x = t / max_distance
MCPT_HD double occlusion_value(int falloff, bool near, double t, double max_distance)
{
    if (!near) return 1.0;
    const double x = t / max_distance;
    return falloff == MCPT_OCCLUSION_HARD ? 0.0 : (falloff == MCPT_OCCLUSION_LINEAR ? x : x * x);
}

// what one sample adds: its visibility, its direction weighted by it, and whether it counts as a hit and as a hit from behind
struct OccSample {
    double v, dv[3];
    bool near, behind;
};

// d = the ray's direction, n = the hit triangle's stored face normal (read only when the sample is near)
MCPT_HD OccSample occlusion_sample(int falloff, double max_distance, const double* d, bool hit, double t, const double* n)
{
    OccSample s;
    s.near = occlusion_near(hit, t, max_distance);
    s.v = occlusion_value(falloff, s.near, t, max_distance);
    s.dv[0] = d[0] * s.v; s.dv[1] = d[1] * s.v; s.dv[2] = d[2] * s.v;
    s.behind = s.near && visibility_back(d, n);
    return s;
}

MCPT_HD void occlusion_add(OccSums& a, const OccSample& s)
{
    a.s1 += s.v;
    a.s2 += s.v * s.v;
    a.b[0] += s.dv[0];
    a.b[1] += s.dv[1];
    a.b[2] += s.dv[2];
    a.hits += s.near ? 1 : 0;
    a.back += s.behind ? 1 : 0;
}

// the radiance query's standard error of the mean of spp samples (dev_common.hpp: progressive_se2): 0 when spp < 2
MCPT_HD double occlusion_stderr(double s1, double s2, int spp)
{
    if (spp < 2) return 0.0;
    const double var = (s2 - s1 * s1 / spp) / (spp - 1);
    return sqrt((var > 0.0 ? var : 0.0) / spp);
}

// The bent normal: b over its length when that is finite and > 0, otherwise the hemisphere rule's n^ of the entry's normal nrm.
MCPT_HD void occlusion_bent(const double* b, const double* nrm, double* out)
{
    const double l = sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
    const bool own = l > 0.0 && l < INFINITY;
    const double m = own ? l : sqrt((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]);
    const double* s = own ? b : nrm;
    out[0] = s[0] / m; out[1] = s[1] / m; out[2] = s[2] / m;
}

// What a query's kernels share: a RayChunk (visibility.hpp) whose list is the call's entries, [n][6] position and normal, in the hit
// workspace the visibility bake uses too (mcpt_device::Visibility), and the two knobs of the fold.
struct OccChunk : RayChunk {
    int falloff;
    double max_distance;
};

// rays6[slot] = query_ray(MCPT_QUERY_KIND_HEMISPHERE, ...) of every ray of the chunk (chunk_kernels.hpp: k_chunk_rays)
void launch_occlusion_rays(const OccChunk& c, hipStream_t st);
// the fold of the chunk's traced rays into ao [n] and (each may be null) stderr1 [n], bent3 [n][3], hits, back [n], at the chunk's entries
void launch_occlusion_fold(const DScene& S, const OccChunk& c, double* d_ao, double* d_stderr1, double* d_bent3, int32_t* d_hits, int32_t* d_back,
                           hipStream_t st);
// The answers of the n_list entries T = d_texels[i] into the maps, which the caller has cleared; every map but d_ao (and its source) may
// be null.
void launch_occlusion_scatter(const int32_t* d_texels, long long n_list, const double* ao, const double* err, const double* bent3, const int32_t* hits,
                              const int32_t* back, double* d_ao, double* d_err, double* d_bent3, int32_t* d_hits, int32_t* d_back, hipStream_t st);

}  // namespace mcpt
