// Baked frames (mcpt.h: baked frames): the arithmetic of a lightmap's lookup by chart coordinate and of the radiance a surface sample
// shows under a baked irradiance, the one copy of it -- baked.hip compiles it for the GPU, baked_api.cpp for
// mcpt_lightmap_irradiance_host -- and the launch interface of the kernels.  fp64, no contraction (-ffp-contract=off), IEEE division,
// every expression in the order mcpt.h writes it; tests/baked_ref.py restates it in numpy.
#pragma once
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mcpt.h"
#include "lightmap.hpp"
#include "visibility.hpp"
#include "volume.hpp"

namespace mcpt {

#define MCPT_BAKED_PI 3.141592653589793

// One axis of a lightmap lookup: the two texels i[0], i[1] around chart coordinate u of an axis of `size` texels and their weights.  The
// clamp is done in double, before any conversion to int: a coordinate far outside the map takes the border's texel, a NaN (the device
// form does not look) lands on texel 0, never outside the map.
MCPT_HD void baked_axis(double u, int size, int* i, double* w)
{
    const double top = double(size - 1);
    double s = u * double(size) - 0.5;
    s = s > 0.0 ? s : 0.0;
    s = s < top ? s : top;
    double f = 0.0;
    i[0] = i[1] = 0;
    if (size >= 2) {
        const int fl = int(floor(s));
        i[0] = fl < size - 2 ? fl : size - 2;
        i[1] = i[0] + 1;
        f = s - double(i[0]);
    }
    w[0] = 1.0 - f;
    w[1] = f;
}

// The four taps of chart coordinate (u, v) in a W x H map: texel T[j] and weight w[j] of tap j = dy * 2 + dx, after the owner rule (owner:
// one int32 per texel, or null).  Returns the number of taps whose weight is > 0; 0 under an owner map that leaves nothing: every weight
// is then 0.0 and the lookup's outputs are +0.0.
MCPT_HD int baked_taps(int W, int H, const int32_t* owner, double u, double v, int32_t* T, double* w)
{
    int x[2], y[2];
    double wx[2], wy[2];
    baked_axis(u, W, x, wx);
    baked_axis(v, H, y, wy);
    for (int j = 0; j < 4; j++) {
        const int dx = j & 1, dy = j >> 1;
        T[j] = y[dy] * W + x[dx];
        w[j] = wx[dx] * wy[dy];
    }
    if (owner) {
        double sum = 0.0;
        for (int j = 0; j < 4; j++) {
            if (owner[T[j]] == -1) w[j] = 0.0;
            sum += w[j];
        }
        const bool any = sum > 0.0;
        for (int j = 0; j < 4; j++) w[j] = any ? w[j] / sum : 0.0;
    }
    int c = 0;
    for (int j = 0; j < 4; j++) c += w[j] > 0.0 ? 1 : 0;
    return c;
}

// E[3] from the taps' texels of irr [W * H][3]: per channel the sum in j order from 0.0.  lit == false (nothing owned around): +0.0.
MCPT_HD void baked_blend(const double* irr, const int32_t* T, const double* w, bool lit, double* E)
{
    for (int c = 0; c < 3; c++) E[c] = 0.0;
    if (!lit) return;
    for (int c = 0; c < 3; c++)
        for (int j = 0; j < 4; j++) E[c] += w[j] * irr[size_t(T[j]) * 3 + size_t(c)];
}

// the whole lookup of one chart coordinate; returns the taps
MCPT_HD int baked_lightmap_lookup(int W, int H, const double* irr, const int32_t* owner, double u, double v, double* E)
{
    int32_t T[4];
    double w[4];
    const int c = baked_taps(W, H, owner, u, v, T, w);
    baked_blend(irr, T, w, c > 0, E);
    return c;
}

// the chart coordinate of barycentrics g on the chart row uv = (au, av, bu, bv, cu, cv)
MCPT_HD void baked_chart_uv(const double* uv, double gx, double gy, double gz, double* out)
{
    out[0] = (uv[0] * gx + uv[2] * gy) + uv[4] * gz;
    out[1] = (uv[1] * gx + uv[3] * gy) + uv[5] * gz;
}

// a shading normal that cannot be used: its squared length is 0 or not finite (the lightmap list's fallback rule)
MCPT_HD bool baked_normal_bad(const double* n)
{
    const double l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    return !(l2 > 0.0 && l2 < INFINITY);
}

// n negated when it points along the ray d (MCPT_BAKED_FACE_VIEWER)
MCPT_HD void baked_face_viewer(const double* d, double* n)
{
    if (((d[0] * n[0] + d[1] * n[1]) + d[2] * n[2]) > 0.0)
        for (int c = 0; c < 3; c++) n[c] = -n[c];
}

// the radiance of a surface sample of diffuse colour kd under irradiance E
MCPT_HD void baked_surface_radiance(const double* kd, const double* E, bool lighting_only, double* L)
{
    for (int c = 0; c < 3; c++) L[c] = lighting_only ? E[c] / MCPT_BAKED_PI : (kd[c] * E[c]) / MCPT_BAKED_PI;
}

// A baked source as the kernels read it: device pointers, the structs by value.
struct BakedSource {
    int32_t kind;                   // MCPT_BAKED_VOLUME or MCPT_BAKED_LIGHTMAP
    int32_t visible;                // a volume with moments: mcpt_volume_irradiance_visible's lookup
    mcpt_volume_grid grid;
    mcpt_volume_visibility vis;
    const double* sh27;
    const uint8_t* valid;           // or null
    const double* moments;          // visible != 0
    const double* uv6;              // [t][6] in .obj order, or null: the faces' own vt
    int32_t width, height;
    const double* irr;              // [W * H][3]
    const int32_t* owner;           // [W * H] or null
};

// Where a shading launch puts its answers, by ray; every pointer may be null.
struct BakedOut {
    double* radiance3;
    int32_t* kind;
    int32_t* face;
    double* q6;
    double* uv2;
    double* kd3;
    double* e3;
    int32_t* lit;
};

// A chunk of a baked frame: pixels first .. first + n - 1, G samples each, rays and answers sample-major (j = k * n + i).
struct BakedChunk {
    int first, n, G;
    const double* rays6;            // [n * G][6]
    const int32_t* leaf;            // [n * G] the leaf of the closest hit, -1: a miss
    const double* t;                // [n * G]
    const double* p;                // [n * G][3]
};

// d_e3[i], d_taps[i] (may be null) of chart coordinates uv2[i], i = 0 .. n-1 (n >= 1); d_owner may be null
void launch_lightmap_irradiance(int W, int H, const double* d_irr, const int32_t* d_owner, const double* d_uv2, int64_t n, double* d_e3, int32_t* d_taps,
                                hipStream_t st);
// rays6[k * c.n + i] = camera_ray(lens, seed, c.first + i, k), one lane per ray
void launch_baked_camera_rays(const DLens& lens, unsigned long long seed, const BakedChunk& c, double* d_rays6, hipStream_t st);
// One lane per ray: rays i = 0 .. n-1 with their closest hits (leaf, t, p: launch_trace_closest_leaf's) shaded under B, answers at o[i].
void launch_baked_shade(const DScene& S, const BakedSource& B, int flags, const double* d_rays6, const int32_t* d_leaf, const double* d_t,
                        const double* d_p, long long n, const BakedOut& o, hipStream_t st);
// One lane per pixel of the chunk folds its G shaded samples (rad3, kind, lit: launch_baked_shade's, sample-major) in k order.
void launch_baked_fold(const BakedChunk& c, const double* d_rad3, const int32_t* d_kind, const int32_t* d_lit, double* d_img, int32_t* d_counts3,
                       int32_t* d_litcount, hipStream_t st);

}  // namespace mcpt
