// Baked specular (mcpt.h: baked specular): the arithmetic of the mirror direction a baked surface sample looks its reflection volume up
// along, the one copy of it -- baked_specular.hip compiles it for the GPU, tests/baked_specular_ref.py restates it in numpy -- and the
// launch interface of the kernels.  fp64, no contraction (-ffp-contract=off), every expression in the order mcpt.h writes it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mcpt.h"
#include "baked.hpp"
#include "reflection_volume.hpp"

namespace mcpt {

struct DScene;

// r = d * (n . n) - n * (2 (d . n)): the mirror direction of d about n scaled by |n|^2 -- no division, and the same for n and -n.
// Returns whether r can be looked up: its 1-norm is > 0 and finite.
MCPT_HD bool baked_mirror(const double* d, const double* n, double* r)
{
    const double dn = (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2];
    const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    for (int c = 0; c < 3; c++) r[c] = d[c] * nn - n[c] * (2.0 * dn);
    const double l = (fabs(r[0]) + fabs(r[1])) + fabs(r[2]);
    return l > 0.0 && l < INFINITY;
}

// the exponent a material's Ns is looked up with
MCPT_HD double baked_exponent(double Ns) { return Ns >= 0.0 ? Ns : 0.0; }

// Where a specular launch puts its answers, by ray; every pointer may be null.
struct BakedSpecOut {
    double* spec3;
    double* ks3;
    double* r3;
    double* ns;
    int32_t* slit;
};

// d_out3[r] and d_corners[r] (may be null) of receivers r = 0 .. m-1 (m >= 1): q6 = position, normal; d3 the direction, x the exponent
void launch_reflection_volume_lookup(const ReflVolume& V, const double* d_q6, const double* d_d3, const double* d_x, int64_t m, double* d_out3,
                                     int32_t* d_corners, hipStream_t st);
// One lane per ray, after launch_baked_shade of the same rays under the same flags: the specular term of rays i = 0 .. n-1 with their
// closest hits (leaf, t, p), answers at o[i], ks * R (R under MCPT_BAKED_LIGHTING_ONLY) added to d_radiance3[i] (may be null).
void launch_baked_specular(const DScene& S, const ReflVolume& V, int flags, const double* d_rays6, const int32_t* d_leaf, const double* d_t,
                           const double* d_p, long long n, double* d_radiance3, const BakedSpecOut& o, hipStream_t st);
// One lane per pixel of the chunk counts its samples (sample-major) with slit > 0 into d_count[first + i].
void launch_baked_specular_count(const BakedChunk& c, const int32_t* d_slit, int32_t* d_count, hipStream_t st);

// What the baked calls' loops (baked_api.cpp) add for a specular source: the volume, and where the answers go -- ray by ray from the
// call's first ray (baked radiance), or per pixel (a frame; the per-ray words live in the workspace).
struct BakedSpecular {
    ReflVolume V;
    BakedSpecOut rays;
    int32_t* pixel_slit;
};

}  // namespace mcpt
