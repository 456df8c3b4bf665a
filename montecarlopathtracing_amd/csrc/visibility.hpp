// Probe visibility (mcpt.h: probe visibility): the arithmetic of a probe's octahedral depth map -- the bin of a direction, the depth and the
// back-face test of one sample -- and of the lookup that weighs every corner of an irradiance volume by what its probe sees of the
// receiver, the one copy of it: visibility.hip compiles it for the GPU, visibility_api.cpp for mcpt_visibility_bin and
// mcpt_volume_irradiance_visible_host.  fp64, no contraction (-ffp-contract=off), IEEE division, every expression in the order mcpt.h
// writes it; tests/visibility_ref.py restates it in numpy.  The launch interface of the three kernels is at the end.
#pragma once
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mcpt.h"
#include "volume.hpp"

namespace mcpt {

struct DScene;

// The bin of direction (x, y, z) in an R x R octahedral map, 0 .. R * R - 1.  A direction that is not finite, is zero, or whose 1-norm
// overflows lands in bin 0 (the host helper refuses it first; the kernels do not look), never outside the table.
MCPT_HD int visibility_bin(double x, double y, double z, int R)
{
    const double l = (fabs(x) + fabs(y)) + fabs(z);
    if (!(l > 0.0 && l < INFINITY)) return 0;
    double u = x / l, v = y / l;
    if (z < 0.0) {
        const double u0 = u, v0 = v;
        u = (1.0 - fabs(v0)) * (u0 >= 0.0 ? 1.0 : -1.0);
        v = (1.0 - fabs(u0)) * (v0 >= 0.0 ? 1.0 : -1.0);
    }
    const double top = double(R - 1);
    const double fx = floor((u * 0.5 + 0.5) * double(R)), fy = floor((v * 0.5 + 0.5) * double(R));
    const int bx = fx > 0.0 ? (fx < top ? int(fx) : R - 1) : 0;
    const int by = fy > 0.0 ? (fy < top ? int(fy) : R - 1) : 0;
    return by * R + bx;
}

// the depth a sample adds to its bin: the hit's distance, or max_distance for a miss and for everything beyond it
MCPT_HD double visibility_depth(bool hit, double t, double max_distance) { return hit ? (t < max_distance ? t : max_distance) : max_distance; }

// a hit from behind: the ray runs along the triangle's stored face normal
MCPT_HD bool visibility_back(const double* d, const double* n) { return ((d[0] * n[0] + d[1] * n[1]) + d[2] * n[2]) > 0.0; }

// The factor of the probe at c for a receiver whose biased position is xb: Chebyshev's bound, cubed, on the share of the probe's rays
// towards the receiver that reach as far as it is away.  m = the probe's moments, [R * R][2].
MCPT_HD double visibility_factor(const mcpt_volume_visibility& vp, const double* m, const double* xb, const double* c)
{
    const double vx = xb[0] - c[0], vy = xb[1] - c[1], vz = xb[2] - c[2];
    const double dist = sqrt((vx * vx + vy * vy) + vz * vz);
    double f = 1.0;
    if (!(dist == 0.0)) {
        const int b = visibility_bin(vx / dist, vy / dist, vz / dist, vp.res);
        const double mu = m[b * 2], m2 = m[b * 2 + 1];
        if (!(mu < 0.0)) {
            const double dc = dist < vp.max_distance ? dist : vp.max_distance;
            if (!(dc <= mu)) {
                double var = m2 - mu * mu;
                var = var > 0.0 ? var : 0.0;
                const double delta = dc - mu;
                const double ch = var / (var + delta * delta);
                f = (ch * ch) * ch;
            }
        }
    }
    return f > vp.min_visibility ? f : vp.min_visibility;
}

// volume_corners with a factor per corner: probe P[j] and weight w[j] of corner j after the mask (valid: one byte per probe, or null: all
// ones), the factors and the division by their sum.  q = the receiver's position and normal.  Returns the number of corners whose weight
// is > 0; 0: every weight is 0.0 and the receiver's outputs are +0.0.
MCPT_HD int visibility_corners(const mcpt_volume_grid& g, const mcpt_volume_visibility& vp, const double* moments, const uint8_t* valid, const double* q,
                               int32_t* P, double* w)
{
    int ix[2], iy[2], iz[2];
    double wx[2], wy[2], wz[2];
    volume_axis(q[0], g.origin[0], g.spacing[0], g.nx, ix, wx);
    volume_axis(q[1], g.origin[1], g.spacing[1], g.ny, iy, wy);
    volume_axis(q[2], g.origin[2], g.spacing[2], g.nz, iz, wz);
    const double l = sqrt((q[3] * q[3] + q[4] * q[4]) + q[5] * q[5]);
    const double xb[3] = {q[0] + (q[3] / l) * vp.normal_bias, q[1] + (q[4] / l) * vp.normal_bias, q[2] + (q[5] / l) * vp.normal_bias};
    const size_t per_probe = size_t(vp.res) * size_t(vp.res) * 2;
    double W = 0.0;
    for (int j = 0; j < 8; j++) {
        const int dx = j & 1, dy = (j >> 1) & 1, dz = j >> 2;
        P[j] = (iz[dz] * g.ny + iy[dy]) * g.nx + ix[dx];
        w[j] = (wx[dx] * wy[dy]) * wz[dz];
        if (valid && valid[P[j]] == 0) w[j] = 0.0;
        const double c[3] = {volume_coord(g, 0, ix[dx]), volume_coord(g, 1, iy[dy]), volume_coord(g, 2, iz[dz])};
        w[j] = w[j] * visibility_factor(vp, moments + size_t(P[j]) * per_probe, xb, c);
        W += w[j];
    }
    const bool any = W > 0.0;
    int n = 0;
    for (int j = 0; j < 8; j++) {
        w[j] = any ? w[j] / W : 0.0;
        n += w[j] > 0.0 ? 1 : 0;
    }
    return n;
}

// What the kernels of a call that answers a list chunk by chunk share (a bake here, an occlusion query: occlusion.hpp): the items (probes,
// entries) of one chunk and the workspace their rays live in (HitWork).  Ray (i, j), sample j of the chunk's item i, sits at slot
// i * spp + j of rays6 / leaf / t.
struct RayChunk {
    const double* list;         // all the call's items: [n][3] positions (sphere) or [n][6] positions and normals (hemisphere)
    const int32_t* ids;         // [n] or null
    long long first, count;     // the chunk's items: first .. first + count - 1
    int spp, sample_base;
    unsigned long long seed;
    double* rays6;              // [count * spp][6]
    int32_t* leaf;              // [count * spp] the leaf of the closest hit, -1: a miss
    double* t;                  // [count * spp]
};

// rays6[slot] = query_ray(MCPT_QUERY_KIND_SPHERE, ...) of every ray of the chunk (chunk_kernels.hpp: k_chunk_rays)
void launch_visibility_rays(const RayChunk& c, hipStream_t st);
// the fold of the chunk's traced rays into moments [n][R * R][2] and (each may be null) hits, back, valid [n], at the chunk's probes
void launch_visibility_fold(const DScene& S, const RayChunk& c, const mcpt_visibility_params& vp, double* d_moments, int32_t* d_hits, int32_t* d_back,
                            uint8_t* d_valid, hipStream_t st);
// launch_volume_irradiance with visibility_corners for volume_corners
void launch_volume_irradiance_visible(const mcpt_volume_grid& g, const mcpt_volume_visibility& vp, const double* d_sh27, const double* d_moments,
                                      const uint8_t* d_valid, const double* d_q6, int64_t n, double* d_e3, int32_t* d_corners, hipStream_t st);

}  // namespace mcpt
