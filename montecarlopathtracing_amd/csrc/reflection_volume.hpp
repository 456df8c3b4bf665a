// Reflection volumes (mcpt.h: baked specular, "reflection volume lookup"): reflection probes on the probes of an mcpt_volume_grid, blended
// by position with the corners and weights the irradiance volume forms -- volume.hpp's volume_corners, visibility.hpp's
// visibility_corners -- the one copy of it: baked_specular.hip compiles it for the GPU, baked_specular_api.cpp for
// mcpt_reflection_volume_lookup_host.  Built from reflection.hpp's pieces: what reflection_lookup forms of a direction and an exponent --
// the level or the two levels, the blend factor, each level's four wrapped taps and their weights -- depends on neither the probe nor the
// corner, so it is formed once per receiver and the loop over the eight corners is loads, multiplies and adds in reflection_lookup's own
// order.  fp64, no contraction (-ffp-contract=off), IEEE division; tests/baked_specular_ref.py restates it in numpy.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/mcpt.h"
#include "reflection.hpp"

namespace mcpt {

// What a direction d and an exponent x select in any chain of description c: `levels` levels (1, or 2 blended by a), and per level the
// chain texel (counted from the chain's first) and the weight of taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1).
struct ReflTaps {
    int levels;
    double a, b;                // levels == 2: value = b * v_0 + a * v_1 with b = 1.0 - a
    int32_t tap[2][4];
    double w[2][4];
};

// one level's taps: reflection_level's, with the level's first texel added
MCPT_HD void reflection_level_taps(int first, int R, const double* d, int32_t* tap, double* w)
{
    double s, t, fx, fy;
    reflection_encode(d[0], d[1], d[2], s, t);
    int x0, y0;
    reflection_axis(s, R, x0, fx);
    reflection_axis(t, R, y0, fy);
    int tx[4] = {x0, x0 + 1, x0, x0 + 1}, ty[4] = {y0, y0, y0 + 1, y0 + 1};
    for (int j = 0; j < 4; j++) {
        reflection_wrap(R, tx[j], ty[j]);
        tap[j] = first + (ty[j] * R + tx[j]);
    }
    w[0] = (1.0 - fx) * (1.0 - fy);
    w[1] = fx * (1.0 - fy);
    w[2] = (1.0 - fx) * fy;
    w[3] = fx * fy;
}

// reflection_lookup's choice of levels for exponent x, and their taps for direction d
MCPT_HD void reflection_taps(const mcpt_reflection_chain& c, const double* d, double x, ReflTaps& T)
{
    const int n = c.num_levels;
    int first[kReflectionMaxLevels];
    for (int l = 0, at = 0; l < n; l++) { first[l] = at; at += c.level_res[l] * c.level_res[l]; }
    T.levels = 1;
    T.a = 0.0; T.b = 1.0;
    int l = 0;
    if (n == 1 || x >= double(c.level_ns[0])) l = 0;
    else if (x <= double(c.level_ns[n - 1])) l = n - 1;
    else {
        l = n - 2;
        for (int m = 0; m < n - 1; m++)
            if (x > double(c.level_ns[m + 1])) { l = m; break; }
        const double w0 = reflection_wt(double(c.level_ns[l])), w1 = reflection_wt(double(c.level_ns[l + 1]));
        T.a = (reflection_wt(x) - w0) / (w1 - w0);
        if (!(T.a == 0.0)) {
            T.levels = 2;
            T.b = 1.0 - T.a;
            reflection_level_taps(first[l + 1], c.level_res[l + 1], d, T.tap[1], T.w[1]);
        }
    }
    reflection_level_taps(first[l], c.level_res[l], d, T.tap[0], T.w[0]);
}

// the value of taps T in the chain p [T][3] of one probe: reflection_lookup's, bit for bit
MCPT_HD void reflection_taps_value(const ReflTaps& T, const double* p, double* v)
{
    const double* m0 = p + size_t(T.tap[0][0]) * 3;
    const double* m1 = p + size_t(T.tap[0][1]) * 3;
    const double* m2 = p + size_t(T.tap[0][2]) * 3;
    const double* m3 = p + size_t(T.tap[0][3]) * 3;
    for (int ch = 0; ch < 3; ch++) v[ch] = ((T.w[0][0] * m0[ch] + T.w[0][1] * m1[ch]) + T.w[0][2] * m2[ch]) + T.w[0][3] * m3[ch];
    if (T.levels == 2) {
        const double* k0 = p + size_t(T.tap[1][0]) * 3;
        const double* k1 = p + size_t(T.tap[1][1]) * 3;
        const double* k2 = p + size_t(T.tap[1][2]) * 3;
        const double* k3 = p + size_t(T.tap[1][3]) * 3;
        for (int ch = 0; ch < 3; ch++) {
            const double v1 = ((T.w[1][0] * k0[ch] + T.w[1][1] * k1[ch]) + T.w[1][2] * k2[ch]) + T.w[1][3] * k3[ch];
            v[ch] = T.b * v[ch] + T.a * v1;
        }
    }
}

// out[3] from the corners' chains, chain [probe][texels][3]: per channel the sum in j order from 0.0; a corner whose weight is 0.0
// contributes nothing and is not read
MCPT_HD void reflection_volume_blend(const ReflTaps& T, const double* chain, size_t texels, const int32_t* P, const double* w, double* out)
{
    for (int ch = 0; ch < 3; ch++) out[ch] = 0.0;
    for (int j = 0; j < 8; j++) {
        if (w[j] == 0.0) continue;
        double v[3];
        reflection_taps_value(T, chain + size_t(P[j]) * texels * 3, v);
        for (int ch = 0; ch < 3; ch++) out[ch] += w[j] * v[ch];
    }
}

// A reflection volume as the kernels read it: device pointers, the structs by value.
struct ReflVolume {
    mcpt_volume_grid grid;
    mcpt_volume_visibility vis;
    mcpt_reflection_chain chain;
    int32_t texels;                 // of one probe's chain
    int32_t visible;                // moments: visibility_corners for volume_corners
    const double* data;             // [nprobes][texels][3]
    const uint8_t* valid;           // or null
    const double* moments;          // visible != 0
};

// The whole lookup of one receiver q = (position, normal) for direction d and exponent x; returns the corners.  VISIBLE is a template
// parameter so that the plain lookup carries none of the other's registers.
template <bool VISIBLE>
MCPT_HD int reflection_volume_lookup(const ReflVolume& V, const double* q, const double* d, double x, double* out)
{
    int32_t P[8];
    double w[8];
    int c;
    if (VISIBLE) c = visibility_corners(V.grid, V.vis, V.moments, V.valid, q, P, w);
    else c = volume_corners(V.grid, V.valid, q, P, w);
    if (c <= 0) {
        for (int ch = 0; ch < 3; ch++) out[ch] = 0.0;
        return 0;
    }
    ReflTaps T;
    reflection_taps(V.chain, d, x, T);
    reflection_volume_blend(T, V.data, size_t(V.texels), P, w, out);
    return c;
}

}  // namespace mcpt
